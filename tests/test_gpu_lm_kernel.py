"""GPU (-m gpu): ONE launch of dec_lm_kernel (csrc/dec_lm.hip) through wlx_debug_lm_apply against lm.py's float64 restatement.
States exact; ids above eot, the pad columns and the guard words bit for bit; the fused logits within a MEASURED tolerance: 4 x the largest
deviation, on these very inputs, of a NumPy restatement in float32 throughout from the float64 oracle (the factor covers the device's
other reduction order and one to two ulp in expf / logf). The bound never reads device output. Each case prints its figures; a run with
WLX_EXCESS_OUT set leaves them in profiles/lm_kernel_tests_excess.txt."""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import lm as L

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GUARD, PLEN, POS, W = 64, 3, 5, 0.7
# end-of-text per vocabulary: the alphabet ends inside a chunk of 8192 ids, exactly at its end, one id into the next, and where Whisper's does
EOT_OF = {1000: 960, 8192: 8191, 8193: 8192, 51866: 50257}
_figures = []


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("WLX_EXCESS_OUT")
    if out and _figures:
        path = Path(out) / "lm_kernel_tests_excess.txt" if Path(out).is_dir() else ROOT / "profiles" / "lm_kernel_tests_excess.txt"
        with open(path, "w") as f:
            f.write("per case of tests/test_gpu_lm_kernel.py, one run on an MI355X: max |float32 restatement - float64 oracle| (CPU), the bound\n"
                    "(4 x that), max |dec_lm_kernel - float64 oracle|. A record of the margin, not an input to any bound.\n")
            f.writelines("%-40s reference %.3e  bound %.3e  device %.3e\n" % t for t in _figures)


def build(vocab, order, seed):
    """a model with every shape the kernel branches on: a chain of the full depth, a context with more than 1024 edges, one without edges,
    edges on both sides of a chunk boundary (8191 / 8192), a token T[k] that only level k of the deep chain knows"""
    rng = np.random.default_rng(seed)
    eot = EOT_OF[vocab]
    deep = (4, 3, 2, 1)[5 - order:] if order > 1 else ()        # the longest context: its chain is deep, deep[1:], ...
    probs, bows = {}, {}
    T = [20 + k for k in range(4)]
    if order > 1:
        for k in range(len(deep)):
            ctx = deep[k:]
            n = min(eot - 100, 1500 if k == len(deep) - 1 else 40)      # the unigram-adjacent context is the large one
            toks = set(int(t) for t in rng.choice(np.arange(100, eot), size=n, replace=False))
            toks |= {T[k], eot} | {t for t in (8190 + k, 8191, 8192) if t <= eot}
            probs[ctx] = {t: float(rng.uniform(-9, -0.5)) for t in toks}
            bows[ctx] = float(rng.uniform(-2, -0.1))
        bows[(7,)] = -0.7                                       # a context without edges
        for t in T:                                             # a found edge and a fall to the unigram level end in different states
            bows[(t,)] = -0.3
            if order > 2:
                bows[(1, t)] = -0.2
        probs[(L.BOS,)] = {T[0]: -1.0, 50: -2.0}
    uni = rng.uniform(-12, -2, size=eot + 1)
    return L.NgramLM.from_tables(vocab, eot, order, uni, probs, bows), deep, T


def rows_of(lm, deep, T, which):
    """(prev_state, token, pos, nsp, kind) per row"""
    def st(ctx):
        s = lm.start_state
        for t in ctx:
            s = lm.next_state(s, t)
        return s
    d, big, bare = st(deep), st(deep[-1:]), st((7,))
    if which == "a":
        return [(d, 5, PLEN - 1, 0, "plain"), (d, T[0], POS, 0, "plain"), (d, T[1], POS, 0, "plain"), (d, 60, POS, 0, "plain"),
                (big, min(lm.eot + 3, lm.vocab - 1), POS, 0, "plain"), (lm.n_states + 12345, T[0], POS, 0, "plain"), (d, T[0], POS, 1, "plain")]
    return [(bare, T[0], POS, 0, "plain"), (d, T[2], POS, 0, "plain"), (d, T[3], POS, 0, "holes"), (big, 61, POS, 0, "holes"),
            (d, 7, POS, 0, "empty"), (lm.start_state, T[0], POS, 0, "plain"), (0, 7, POS, 0, "plain")]


def fuse32(lm, row, state, w):
    """lm.fuse_row with float32 arithmetic throughout"""
    out = row.astype(np.float32).copy()
    a = out[:lm.eot + 1]
    if not np.isfinite(a).any():
        return out
    levels, above, acc = [], [], np.float32(0)
    while state > 0:
        levels.append(state); above.append(acc)
        acc = np.float32(acc + lm.backoff_weight[state]); state = int(lm.backoff_state[state])
    s = lm.unigram_logp[:lm.eot + 1] + acc
    for n, b in zip(reversed(levels), reversed(above)):
        lo, hi = lm.edge_off[n], lm.edge_off[n + 1]
        s[lm.edge_tok[lo:hi]] = lm.edge_logp[lo:hi] + b

    def lse(x):
        m = x.max()
        return np.float32(m + np.log(np.sum(np.exp(x - m), dtype=np.float32)))
    f = a + np.float32(w) * s
    out[:lm.eot + 1] = f - np.float32(lse(f) - lse(a))
    return out


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("vocab, ldl", [(1000, 1008), (8192, 8192), (8193, 8200), (51866, 51872)])
def test_one_launch_equals_the_float64_restatement(gpu, vocab, ldl, order, which):
    lm, deep, T = build(vocab, order, seed=vocab + order)
    spec = rows_of(lm, deep, T, which)
    rows = len(spec)
    rng = np.random.default_rng(7 * vocab + order)
    buf = (rng.standard_normal(rows * ldl + GUARD) * 4).astype(np.float32)
    logits = buf[:rows * ldl].reshape(rows, ldl)
    for r, (_, _, _, _, kind) in enumerate(spec):
        if kind == "holes":
            logits[r, rng.choice(lm.eot + 1, size=lm.eot // 3, replace=False)] = -np.inf
        elif kind == "empty":
            logits[r, :lm.eot + 1] = -np.inf
    before = buf.copy()
    prev, tok, pos, nsp = (np.array([s[i] for s in spec], dtype=np.int32) for i in range(4))
    parent = np.array([(r + 1) % rows for r in range(rows)], dtype=np.int32)
    state_out = np.full(rows, -7, dtype=np.int32)
    i32p, f32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    off, boff, bw, etok, elogp, enext, uni, unext = lm.packed()
    rc = _lib.load().wlx_debug_lm_apply(0, vocab, lm.eot, lm.order, lm.n_states, lm.start_state, i32p(off), i32p(boff), f32p(bw), i32p(etok),
                                        f32p(elogp), i32p(enext), f32p(uni), i32p(unext), W, f32p(buf), rows, ldl, i32p(tok), i32p(pos),
                                        i32p(parent), PLEN, i32p(nsp), i32p(prev), i32p(state_out))
    assert rc == 0, _lib.load().wlx_last_error()
    want_state = [lm.start_state if p < PLEN else lm.next_state(int(s), int(t)) for s, t, p, _, _ in spec]
    assert state_out.tolist() == want_state
    raw = before[:rows * ldl].reshape(rows, ldl)
    ref_dev = dev = 0.0
    for r in range(rows):
        if nsp[r] or spec[r][4] == "empty":
            assert np.array_equal(logits[r].view(np.uint32), raw[r].view(np.uint32)), r
            continue
        want = lm.fuse_row(raw[r], want_state[r], W)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(logits[r]), fin) and np.array_equal(logits[r][~fin], raw[r][~fin]), r
        assert np.array_equal(logits[r, lm.eot + 1:].view(np.uint32), raw[r, lm.eot + 1:].view(np.uint32)), r
        ref_dev = max(ref_dev, float(np.abs(fuse32(lm, raw[r], want_state[r], W)[fin] - want[fin]).max()))
        dev = max(dev, float(np.abs(logits[r][fin] - want[fin]).max()))
        assert np.abs(logits[r, :lm.eot + 1][fin[:lm.eot + 1]] - raw[r, :lm.eot + 1][fin[:lm.eot + 1]]).max() > 0.1, r     # (the launch acted)
    assert np.array_equal(buf[rows * ldl:].view(np.uint32), before[rows * ldl:].view(np.uint32))
    print("vocab %d order %d rows %s: reference %.3e bound %.3e device %.3e" % (vocab, order, which, ref_dev, 4 * ref_dev, dev))
    _figures.append(("vocab %d ldl %d order %d rows %s" % (vocab, ldl, order, which), ref_dev, 4 * ref_dev, dev))
    assert dev <= 4 * ref_dev


def test_a_refused_table_launches_nothing(gpu):
    lm, _, _ = build(1000, 3, seed=1)
    off, boff, bw, etok, elogp, enext, uni, unext = (a.copy() for a in lm.packed())
    boff[1] = 1                                                 # a backoff link that leads nowhere shorter
    buf = np.ones(1008 + GUARD, np.float32)
    z = np.zeros(1, np.int32)
    out = np.full(1, -7, np.int32)
    i32p, f32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    rc = _lib.load().wlx_debug_lm_apply(0, 1000, lm.eot, 3, lm.n_states, lm.start_state, i32p(off), i32p(boff), f32p(bw), i32p(etok), f32p(elogp),
                                        i32p(enext), f32p(uni), i32p(unext), W, f32p(buf), 1, 1008, i32p(z), i32p(z), i32p(z), 1, i32p(z), i32p(z),
                                        i32p(out))
    assert rc == _lib.ERR_ARG and b"strictly shorter" in _lib.load().wlx_last_error()
    assert (buf == 1).all() and out[0] == -7
