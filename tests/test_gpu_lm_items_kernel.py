"""GPU (-m gpu): ONE launch of dec_lm_items_kernel through wlx_debug_lm_apply_items: 4 items x 3 rows under [A at 0.7, none, B at 0.4, A at
1.3], A a trigram model, B a unigram model. A selected item's rows and states equal wlx_debug_lm_apply of its entry BIT FOR BIT; everything
else keeps its bits; against lm.py's float64 the bound is that of tests/test_gpu_lm_kernel.py (4 x the deviation of fuse32 on these inputs)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_lm_kernel import fuse32
from whisperlive_amd import _lib
from whisperlive_amd import lm as L

pytestmark = pytest.mark.gpu
GUARD, PLEN, POS, R = 64, 3, 5, 3
ENTRIES = [(0, 0.7), (1, 0.4), (0, 1.3)]        # (model, weight): A, B, A at another weight
SEL = [0, -1, 1, 2]
i32p, f32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))


def models(vocab, eot):    # A: order 3, two contexts, the shorter with > 1024 edges, edges on both sides of every chunk boundary; B: order 1
    rng = np.random.default_rng(eot)
    probs, bows = {}, {}
    for ctx, n in (((2, 1), 40), ((1,), 1500)):
        toks = set(int(t) for t in rng.choice(np.arange(100, eot), size=n, replace=False)) | {20, eot, 8190, 8191, 8192, eot - 1}
        probs[ctx] = {t: float(rng.uniform(-9, -0.5)) for t in toks}
        bows[ctx] = float(rng.uniform(-2, -0.1))
    bows[(20,)] = -0.3
    a = L.NgramLM.from_tables(vocab, eot, 3, rng.uniform(-12, -2, size=eot + 1), probs, bows)
    b = L.NgramLM.from_tables(vocab, eot, 1, rng.uniform(-12, -2, size=eot + 1), {}, {})
    assert b.n_states < a.n_states and b.n_edges == 0 < a.n_edges
    return a, b


def single(lm, w, buf, ldl, tok, pos, parent, nsp, prev):
    buf, out = buf.copy(), np.full(R, -7, np.int32)
    rc = _lib.load().wlx_debug_lm_apply(0, lm.vocab, lm.eot, lm.order, lm.n_states, lm.start_state, *(p(a) for p, a in zip(
        (i32p, i32p, f32p, i32p, f32p, i32p, f32p, i32p), lm.packed())), w, f32p(buf), R, ldl, i32p(tok), i32p(pos), i32p(parent), PLEN, i32p(nsp),
        i32p(prev), i32p(out))
    assert rc == 0, _lib.load().wlx_last_error()
    return buf, out


def items_call(ms, vocab, eot, buf, ldl, sampling, sel, tok, pos, parent, nsp, done, prev, out):
    packed = [m.packed() for m in ms]
    cat = [np.ascontiguousarray(np.concatenate([p[k] for p in packed])) for k in range(8)]
    meta = [np.array([getattr(m, n) for m in ms], np.int32) for n in ("order", "n_states", "start_state")]
    em, ew = np.array([e[0] for e in ENTRIES], np.int32), np.array([e[1] for e in ENTRIES], np.float32)
    return _lib.load().wlx_debug_lm_apply_items(0, vocab, eot, len(ms), *(i32p(a) for a in meta), *(p(a) for p, a in zip(
        (i32p, i32p, f32p, i32p, f32p, i32p, f32p, i32p), cat)), len(ENTRIES), i32p(em), f32p(ew), f32p(buf), len(sel), R, sampling,
        i32p(np.array(sel, np.int32)), ldl, i32p(tok), i32p(pos), i32p(parent), i32p(np.full(len(sel), PLEN, np.int32)), i32p(nsp), i32p(done),
        i32p(prev), i32p(out))


@pytest.mark.parametrize("sampling", [0, 1])
@pytest.mark.parametrize("vocab, eot, ldl", [(16390, 16383, 16392), (8197, 8193, 8199)])      # ldl a multiple of 4 (16-byte path) and not
def test_items_launch_equals_the_single_route_bit_for_bit(gpu, vocab, eot, ldl, sampling):
    a, b = models(vocab, eot)
    ms, rows = [a, b], len(SEL) * R
    deep = a.next_state(a.next_state(a.start_state, 2), 1)
    stale = a.n_states + 999                                    # a state another model left behind: beyond B's (and A's) n_states
    # (prev_state, token, pos, nsp) per row of an item: a prompt position, a plain row under a stale state, a no_speech row
    spec = [(deep, 5, PLEN - 1, 0), (stale if sampling else deep, 20, POS, 0), (deep, 8191, POS, 1)]
    prev, tok, pos, nsp = (np.array([s[i] for s in spec] * len(SEL), np.int32) for i in range(4))
    prev[2 * R:3 * R] = [deep, deep + 1, stale]                 # item 2 decodes under B: every one of them is out of ITS range
    nsp[3 * R + 2] = 0                                          # (item 3 has no no_speech row: its third row is the row of -inf)
    parent_item = np.array([(r + 1) % R for r in range(R)], np.int32)
    parent = np.concatenate([parent_item + k * R for k in range(len(SEL))]).astype(np.int32)
    done = np.zeros(rows, np.int32)
    done[3 * R + 1] = 1                                         # a finished row: left alone in sampling mode, not read in beam mode
    rng = np.random.default_rng(ldl + sampling)
    buf = (rng.standard_normal(rows * ldl + GUARD) * 4).astype(np.float32)
    buf[:rows * ldl].reshape(rows, ldl)[3 * R + 2, :eot + 1] = -np.inf
    before, out = buf.copy(), np.full(rows, -7, np.int32)
    assert items_call(ms, vocab, eot, buf, ldl, sampling, SEL, tok, pos, parent, nsp, done, prev, out) == 0, _lib.load().wlx_last_error()
    got, raw = buf[:rows * ldl].reshape(rows, ldl), before[:rows * ldl].reshape(rows, ldl)
    same = lambda x, y: np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert same(buf[rows * ldl:], before[rows * ldl:])          # the guard words
    ref_dev = dev = 0.0
    for k, e in enumerate(SEL):
        sl = slice(k * R, (k + 1) * R)
        if e < 0:
            assert same(got[sl], raw[sl]) and (out[sl] == -7).all(), k
            continue
        lm, w = ms[ENTRIES[e][0]], ENTRIES[e][1]
        one = np.concatenate([raw[sl].ravel(), before[rows * ldl:]])
        want, want_state = single(lm, w, one, ldl, tok[sl], pos[sl], parent_item, nsp[sl], prev[sl])
        want = want[:R * ldl].reshape(R, ldl)
        for rb in range(R):
            r = k * R + rb
            if sampling and done[r]:
                assert same(got[r], raw[r]) and out[r] == -7, r
                continue
            assert same(got[r], want[rb]) and out[r] == want_state[rb], (k, rb)
            state = lm.start_state if pos[r] < PLEN else lm.next_state(int(prev[r]), int(tok[r]))
            assert out[r] == state, (k, rb)
            assert same(got[r, eot + 1:], raw[r, eot + 1:]), r
            if nsp[r] or not np.isfinite(raw[r, :eot + 1]).any():
                assert same(got[r], raw[r]), r
                continue
            f64 = lm.fuse_row(raw[r], state, w)
            ref_dev = max(ref_dev, float(np.abs(fuse32(lm, raw[r], state, w) - f64).max()))
            dev = max(dev, float(np.abs(got[r] - f64).max()))
            assert np.abs(got[r, :eot + 1] - raw[r, :eot + 1]).max() > 0.1, r       # (the launch acted)
    print("eot %d ldl %d sampling %d: reference %.3e bound %.3e device %.3e" % (eot, ldl, sampling, ref_dev, 4 * ref_dev, dev))
    assert dev <= 4 * ref_dev


def test_a_selection_outside_the_pool_launches_nothing(gpu):
    a, b = models(8197, 8193)
    rows, ldl = 2 * R, 8200
    buf = np.ones(rows * ldl + GUARD, np.float32)
    z, out = np.zeros(rows, np.int32), np.full(rows, -7, np.int32)
    parent = np.arange(rows, dtype=np.int32)
    rc = items_call([a, b], 8197, 8193, buf, ldl, 0, [0, len(ENTRIES)], z, z, parent, z, z, z, out)
    assert rc == _lib.ERR_ARG and b"outside -1..2" in _lib.load().wlx_last_error()
    assert (buf == 1).all() and (out == -7).all()
