"""GPU tests of the ragged-batch speaker path. The single-item hooks and wlx_spk_embed go through the same launchers with a batch of
one; for the stem, the pooling and the head that is the same kernel, for the filterbank, the mean removal and the MFMA convolution the
launcher picks at n = 1 a kernel without the item table around the same device function. So the bit-for-bit comparisons state that an
item's result does not depend on its neighbours, its position or the table's fill, and for those three also on which of the two
kernels around one body computed it: the
one-launch hooks wlx_spk_debug_conv_batch / _pool_batch against each item as a batch of one, and wlx_spk_embed_batch / embed_many /
identify_speakers on the whole seeded ResNet34 against each segment on its own. The absolute references are the float64 ones of
tests/spk_kernel_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib, spk_weights
from whisperlive_amd.diarization import SpeakerDiarizer, SpeakerEmbedderHIP

from . import spk_kernel_ref as R
from .test_gpu_diarization import SEGMENTS, SPEC, WEIGHT_SEED, _widest_gap_threshold, voice_pcm

pytestmark = pytest.mark.gpu

# item boundaries inside a 16-pixel wave tile and inside a 64-pixel workgroup tile (H = 5: items of 5, 85, 15 and 320 pixels at
# stride 1), a one-column item, odd widths under stride 2
H, WIDTHS = 5, (1, 17, 3, 64)
BIG = 30000.0           # what a neighbour is filled with for the no-bleed check (fp16 holds it; one such tap would swamp any sum)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def run_conv_batch(xs, w, b, rs, stride, relu):
    """(rc, [out fp16 [OH][OW_i][Cout] per item]): the items packed back to back, one launch"""
    Hh, Cin = xs[0].shape[0], xs[0].shape[2]
    Cout, ks = w.shape[0], w.shape[2]
    widths = np.array([x.shape[1] for x in xs], dtype=np.int32)
    shapes = [R.out_hw(Hh, int(W), stride) + (Cout,) for W in widths]
    packed = np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in xs])
    resid = None if rs is None else np.concatenate([np.ascontiguousarray(r).reshape(-1) for r in rs])
    out = np.full(sum(int(np.prod(s)) for s in shapes), np.nan, dtype=np.float16)
    w = np.ascontiguousarray(w, dtype=np.float32)
    rc = _lib.load().wlx_spk_debug_conv_batch(0, R._p(packed.view(np.uint16), C.c_uint16), Hh, len(xs), R._p(widths, C.c_int32), Cin,
                                              R._p(w, C.c_float), R._p(b, C.c_float),
                                              R._p(None if resid is None else resid.view(np.uint16), C.c_uint16), Cout, stride, ks,
                                              int(relu), R._p(out.view(np.uint16), C.c_uint16))
    items, at = [], 0
    for s in shapes:
        items.append(out[at:at + int(np.prod(s))].reshape(s))
        at += int(np.prod(s))
    return rc, items


def _check_conv_batch(Cin, Cout, stride, ks, resid):
    relu = resid
    cases = [R.conv_case(H, W, Cin, Cout, stride, ks, resid, seed=10 + i) for i, W in enumerate(WIDTHS)]
    _, w, b, _ = cases[0]                               # one weight for the whole batch, as in the network
    xs = [c[0] for c in cases]
    rs = [c[3] for c in cases] if resid else None
    rc, got = run_conv_batch(xs, w, b, rs, stride, relu)
    assert rc == 0
    for i, W in enumerate(WIDTHS):
        r = rs[i] if resid else None
        rc1, alone = R.run_conv(xs[i], w, b, r, stride, relu)
        assert rc1 == 0 and got[i].shape == alone.shape and np.isfinite(got[i].astype(np.float32)).all()
        assert (_bits(got[i]) == _bits(alone)).all(), f"item {i} (W = {W}) differs from the item as a batch of one"
        e = R.rel_rms(got[i], R.conv_ref(xs[i], w, b, r, stride, relu))
        print(f"conv batch item W={W} {Cin}->{Cout} s{stride} k{ks} resid={resid}: rel-rms {e:.3e}")
        assert e <= R.REL_RMS, (i, e)
    # no bleed: the even items, then the odd ones, replaced by large values; the others keep their bits
    for loud in (0, 1):
        xl = [np.full_like(x, BIG) if i % 2 == loud else x for i, x in enumerate(xs)]
        rc2, again = run_conv_batch(xl, w, b, rs, stride, relu)
        assert rc2 == 0
        for i in range(len(xs)):
            if i % 2 != loud:
                assert (_bits(again[i]) == _bits(got[i])).all(), f"item {i} changed with its neighbours' input"


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin,Cout", [(32, 64), (64, 32)])
def test_conv_batch(Cin, Cout, stride, ks, resid):
    """the MFMA convolution over four items of one launch (Cout 64: four channel tiles per wave, Cout 32: two)"""
    _check_conv_batch(Cin, Cout, stride, ks, resid)


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_batch_stem(stride, resid):
    """the Cin = 1 form on the vector ALU"""
    _check_conv_batch(1, 32, stride, 3, resid)


@pytest.mark.parametrize("Cn", [64, 128])
def test_pool_batch(Cn):
    F, frames = 3, (2, 5, 130)
    rng = np.random.default_rng(Cn)
    xs = [R.f16(rng.standard_normal((F, T, Cn)) * rng.uniform(0.1, 3.0, (F, 1, Cn)) + rng.standard_normal((F, 1, Cn))) for T in frames]
    packed = np.concatenate([x.reshape(-1) for x in xs])
    fr = np.array(frames, dtype=np.int32)
    out = np.full((len(frames), 2, Cn, F), np.nan, dtype=np.float32)
    rc = _lib.load().wlx_spk_debug_pool_batch(0, R._p(packed.view(np.uint16), C.c_uint16), F, len(frames), R._p(fr, C.c_int32), Cn, 1e-7,
                                              R._p(out, C.c_float))
    assert rc == 0 and np.isfinite(out).all()
    for i, x in enumerate(xs):
        rc1, alone = R.run_pool(x, 1e-7)
        assert rc1 == 0 and (_bits(out[i]) == _bits(alone)).all(), f"item {i} (T = {frames[i]}) differs from the item as a batch of one"


# ------------------------------------------------------------------------------------------------ the whole engine
SECONDS = (0.3, 0.29, 2.5, 0.7, 11.0)


@pytest.fixture(scope="module")
def eng():
    w = spk_weights.fold(spk_weights.random_weights(SPEC, seed=WEIGHT_SEED), SPEC)
    e = SpeakerEmbedderHIP(SPEC, w, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def items(eng):
    """the five segments and `embed` of each alone, computed once before any batch has run"""
    pcms = [voice_pcm(i % 4, s, seed=40 + i) for i, s in enumerate(SECONDS)]
    assert [len(p) for p in pcms] == [4800, 4640, 40000, 11200, 176000]
    return pcms, [eng.embed(p) for p in pcms]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and (_bits(a) == _bits(b)).all())


def test_batch_rows_equal_single_embeds(eng, items):
    pcms, alone = items
    assert alone[1] is None and all(a is not None for i, a in enumerate(alone) if i != 1)
    got = eng.embed_many(pcms)
    assert len(got) == 5 and got[1] is None
    assert all(_same(g, a) for g, a in zip(got, alone)), [_same(g, a) for g, a in zip(got, alone)]
    fb, nn = eng.timings()                                # the batch was the last call
    assert fb > 0 and nn > 0
    # another order, other neighbours: the same rows
    order = [4, 2, 0, 3, 1]
    perm = eng.embed_many([pcms[i] for i in order])
    assert all(_same(perm[k], alone[i]) for k, i in enumerate(order))
    # a batch of one, and a single embed after batches
    for i in (0, 2, 4):
        assert _same(eng.embed_many([pcms[i]])[0], alone[i])
    assert eng.embed_many([pcms[1]]) == [None] and eng.embed_many([]) == []
    assert all(_same(eng.embed(p), a) for p, a in zip(pcms, alone))


def test_more_segments_than_one_call_holds(eng, items):
    """70 segments of 0.7 s (49 s, 70 items): over the 64 items and the 45 s of one call, so embed_many makes several"""
    pcms, alone = items
    got = eng.embed_many([pcms[3]] * 70)
    assert len(got) == 70 and all(_same(g, alone[3]) for g in got)


def test_identify_speakers_equals_one_by_one(eng):
    pcms = [voice_pcm(v, s, seed) for v, s, seed in SEGMENTS]
    thr, _ = _widest_gap_threshold([eng.embed(p) for p in pcms])
    one = SpeakerDiarizer(similarity_threshold=thr, embedder=eng)
    want = [one.identify_speaker(p) for p in pcms]
    assert 2 <= len(set(want)) < len(want), want         # new-speaker and match branches both occur
    many = SpeakerDiarizer(similarity_threshold=thr, embedder=eng)
    assert many.identify_speakers(pcms) == want
    for k in one.speakers:
        assert (many.speakers[k] == one.speakers[k]).all()


def _raw(eng, pcm, lengths, n, out, status):
    f32p = C.POINTER(C.c_float)
    return eng.lib.wlx_spk_embed_batch(eng.h, None if pcm is None else pcm.ctypes.data_as(f32p),
                                       None if lengths is None else lengths.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                       None if out is None else out.ctypes.data_as(f32p),
                                       None if status is None else status.ctypes.data_as(C.POINTER(C.c_int32)))


def test_refusals_leave_the_engine_working(eng, items):
    pcms, alone = items
    E = SPEC.embed_dim
    cap = SPEC.max_seconds * 16000
    good = np.concatenate([pcms[2], pcms[3]])
    good_n = np.array([len(pcms[2]), len(pcms[3])], dtype=np.int64)

    def works():
        out, st = np.full((2, E), np.nan, np.float32), np.full(2, -1, np.int32)
        assert _raw(eng, good, good_n, 2, out, st) == 0 and (st == 0).all()
        assert _same(out[0], alone[2]) and _same(out[1], alone[3])

    works()
    big = np.zeros(cap + 1, np.float32)                    # every buffer below holds what its lengths announce
    out, st = np.full((65, E), 7.0, np.float32), np.full(65, -1, np.int32)
    many_n = np.full(65, 4800, dtype=np.int64)
    refused = [
        ("sum over the cap", (big, np.array([cap // 2, cap // 2 + 1], dtype=np.int64), 2, out, st)),
        ("one item over the cap", (big, np.array([cap + 1], dtype=np.int64), 1, out, st)),
        ("n = 0", (big, many_n, 0, out, st)),
        ("n = 65", (big, many_n, 65, out, st)),
        ("negative length", (big, np.array([4800, -1], dtype=np.int64), 2, out, st)),
        ("null pcm", (None, good_n, 2, out, st)),
        ("null lengths", (good, None, 2, out, st)),
        ("null out", (good, good_n, 2, None, st)),
        ("null status", (good, good_n, 2, out, None)),
    ]
    for what, args in refused:
        assert _raw(eng, *args) == _lib.ERR_ARG, what
        assert (out == 7.0).all() and (st == -1).all(), what          # nothing written
        works()
    # all too short: WLX_OK, zero rows, the distinct status
    out2, st2 = np.full((2, E), 7.0, np.float32), np.full(2, -1, np.int32)
    assert _raw(eng, big, np.array([4799, 0], dtype=np.int64), 2, out2, st2) == 0
    assert (out2 == 0).all() and (st2 == _lib.ERR_TOO_SHORT).all()
    # exactly the cap in two items is served
    out3, st3 = np.zeros((2, E), np.float32), np.full(2, -1, np.int32)
    assert _raw(eng, big, np.array([cap - 4800, 4800], dtype=np.int64), 2, out3, st3) == 0 and (st3 == 0).all()
    assert np.isfinite(out3).all() and np.allclose(np.linalg.norm(out3, axis=1), 1, atol=1e-5)
    works()
