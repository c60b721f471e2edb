"""GPU tests of the speaker front end's ragged form and of the embedding head (csrc/spk.hip), one launch sequence each through
wlx_spk_debug_fbank_batch (spk_fbank_batch_kernel + spk_cmn_batch_kernel) and wlx_spk_debug_head (spk_linear_batch_kernel, then
spk_l2norm_batch_kernel). The ragged filterbank must have the bits of wlx_spk_debug_fbank on each window alone and lie within
test_gpu_spk_kernels.FBANK_ABS of the float64 oracle; the head lies within the bounds derived in tests/spk_kernel_ref.py from the
kernels' summation trees. tests/test_spk_kernel_ref.py shows on the same inputs that the nearest wrong answers lie outside those
bounds. Every tolerance test prints its worst error / bound (profiles/spk_mt_row_kernel_tests_excess.txt keeps one run's figures)."""
from __future__ import annotations

import numpy as np
import pytest

from . import spk_kernel_ref as R
from .test_gpu_spk_kernels import FBANK_ABS

pytestmark = pytest.mark.gpu

F32_SENTINEL, F16_SENTINEL = 0xdeadbeef, 0xbeef


# ------------------------------------------------------------------------------------------------ ragged filterbank
@pytest.mark.parametrize("name", R.FBANK_CASES)
def test_fbank_batch(name):
    """n = 1 (the launcher's table-free kernels), 2, 5 and WLX_SPK_MAX_BATCH windows of one buffer at odd sample offsets, 1 .. 600 frames
    each, two windows sharing samples, offsets descending: spk_item_of / blk0 pick the item of a workgroup, offs.off[i] its samples,
    it.in0 its place in the packed logmel / image. An item read at another offset, averaged over another item's length or placed a frame
    off differs from the single-item hook in bits and from the oracle by more than the bound (test_guard_fbank_batch_case)."""
    pcm, offsets, frames = R.fbank_batch_case(name)
    rc, out, img = R.run_fbank_batch(pcm, offsets, frames)
    assert rc == 0
    total = int(frames.sum())
    assert (out[total:].view(np.uint32) == F32_SENTINEL).all() and (img[total * 80:].view(np.uint16) == F16_SENTINEL).all()
    assert np.isfinite(out[:total]).all()                  # (the sentinel is finite too: the bit comparisons below see unwritten rows)
    ref = R.fbank_batch_ref(pcm, offsets, frames)
    at, worst = 0, 0.0
    for i, (o, T) in enumerate(zip(offsets.tolist(), frames.tolist())):
        rc1, alone, alone_img = R.run_fbank(pcm[o:o + R.item_samples(T)])
        assert rc1 == 0 and alone.shape == (T, 80)
        got, got_img = out[at:at + T], img[at * 80:(at + T) * 80].reshape(80, T)
        assert (got.view(np.uint32) == alone.view(np.uint32)).all(), f"item {i} (T = {T}, offset {o}): frames differ from the window alone"
        assert (got_img.view(np.uint16) == alone_img.view(np.uint16)).all(), f"item {i} (T = {T}, offset {o}): image differs from the window alone"
        if T == 1:
            assert (got.view(np.uint32) == 0).all() and (got_img.view(np.uint16) == 0).all()      # x - x: +0.0 exactly
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref[i]).max()) / FBANK_ABS)
        at += T
    print(f"excess fbank_batch {name}: {worst:.4f}")
    assert worst <= 1.0


def _fbank_refusals():
    pcm = np.zeros(2000, np.float32)
    ok = dict(pcm=pcm, offsets=np.array([1, 3], np.int64), frames=np.array([2, 3], np.int32))
    return ok, [
        ("last frame past n_samples", dict(offsets=np.array([1, 2000 - 400 - 320 + 1], np.int64))),
        ("n_samples short of the window", dict(n_samples=3 + 400 + 320 - 1)),
        ("frames < 1", dict(frames=np.array([2, 0], np.int32))),
        ("negative frames", dict(frames=np.array([-1, 3], np.int32))),
        ("negative offset", dict(offsets=np.array([-1, 3], np.int64))),
        ("n = 0", dict(n=0)),
        ("n = -1", dict(n=-1)),
        ("n = MAX + 1", dict(n=R.MAX_BATCH + 1, offsets=np.ones(R.MAX_BATCH + 1, np.int64), frames=np.ones(R.MAX_BATCH + 1, np.int32))),
        ("n_mels = 0", dict(n_mels=0)),
        ("null pcm", dict(pcm=None, n_samples=2000)),
        ("null offsets", dict(offsets=None, n=2)),
        ("null frames", dict(frames=None, n=2)),
    ]


def test_fbank_batch_refusals():
    """every condition the hook refuses, before any launch and with nothing written; the same arguments without the fault are served"""
    ok, bad = _fbank_refusals()
    rc, out, _ = R.run_fbank_batch(**ok)
    assert rc == 0 and np.abs(out[:5]).max() <= 1e-4        # (silence: the floor in every bin)
    for what, over in bad:
        a = dict(ok)
        a.update(over)
        rc, out, img = R.run_fbank_batch(**a)
        assert rc == 1, what
        assert (out.view(np.uint32) == F32_SENTINEL).all() and (img.view(np.uint16) == F16_SENTINEL).all(), what


# ------------------------------------------------------------------------------------------------ head
@pytest.fixture(scope="module")
def head_refs():
    """float64 references and bounds of every HEAD_CASES entry, computed once for both normalize settings"""
    refs = {}
    for case in R.HEAD_CASES:
        pooled, W, b = R.head_case(*case)
        y = R.head_linear_ref(pooled, W, b)
        by = R.head_linear_bound(pooled, W, b)
        refs[case] = (pooled, W, b, y, by, R.head_norm_ref(y), R.head_norm_bound(y, by))
    return refs


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,E,n", R.HEAD_CASES)
def test_head(head_refs, D, E, n, normalize):
    """spk_linear_body's stride (D = 8: lane 0 alone; 504 / 520: a last trip of some lanes; 5120: ten trips), its row and item indexing
    (blockIdx.x = output, blockIdx.y = item) and spk_l2norm_body's 256 stride (E = 255 / 256 / 257 / 512). A neighbour's bias, a
    shifted weight row, a dropped last piece of D, another item's pooled row or a sum of squares that stops at 256 lie outside the
    bound (test_guard_head_case). Rows of `emb` past n keep their preset bits."""
    pooled, W, b, y, by, z, bz = head_refs[(D, E, n)]
    rc, emb = R.run_head(pooled, W, b, normalize)
    assert rc == 0
    assert (emb[n:].view(np.uint32) == F32_SENTINEL).all() and np.isfinite(emb[:n]).all()
    q = R.excess(emb[:n], z if normalize else y, bz if normalize else by)
    print(f"excess head {'l2norm' if normalize else 'linear'} D={D} E={E} n={n}: {q.max():.4f}")
    assert q.max() <= 1.0, np.unravel_index(np.argmax(q), q.shape)


def test_head_zero_and_tiny_rows():
    """b = 0; an all-zero pooled row gives exact zeros with and without the l2norm (no 0 * inf), a row of norm ~1e-18 and one of ~1e15
    come back with unit norm inside the bound: nothing under the sum of squares may hold a small row back"""
    pooled, W, b = R.head_tiny_case()
    y = R.head_linear_ref(pooled, W, b)
    by = R.head_linear_bound(pooled, W, b)
    z, bz = R.head_norm_ref(y), R.head_norm_bound(y, by)
    rc0, lin = R.run_head(pooled, W, b, 0)
    rc1, emb = R.run_head(pooled, W, b, 1)
    assert rc0 == 0 and rc1 == 0
    assert (lin[0].view(np.uint32) == 0).all() and (emb[0].view(np.uint32) == 0).all()
    q0, q1 = R.excess(lin[:4], y, by), R.excess(emb[:4], z, bz)
    print(f"excess head tiny rows linear: {q0.max():.4f}")
    print(f"excess head tiny rows l2norm: {q1.max():.4f}")
    assert q0.max() <= 1.0 and q1.max() <= 1.0, (q0.max(axis=1), q1.max(axis=1))
    assert np.abs(np.linalg.norm(emb[1:4].astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_head_all_zero_weights():
    """W = 0 and b = 0: every output of every item is exactly +0.0, not NaN, behind the l2norm; and with one zero row of W and a zero in
    b that output alone is exactly zero"""
    pooled, W, b = R.head_case(520, 257, 3)
    rc, emb = R.run_head(pooled, np.zeros_like(W), np.zeros_like(b), 1)
    assert rc == 0 and (emb[:3].view(np.uint32) == 0).all()
    W[256], b[256] = 0, 0
    rc, emb = R.run_head(pooled, W, b, 1)
    assert rc == 0 and (emb[:3, 256].view(np.uint32) == 0).all() and np.isfinite(emb[:3]).all() and (emb[:3, :256] != 0).all()


@pytest.mark.parametrize("what,over", [("D = 12", dict(D=12)), ("D = 0", dict(D=0)), ("D = 4", dict(D=4)), ("E = 0", dict(E=0)),
                                       ("n = 0", dict(n=0)), ("n = -1", dict(n=-1)), ("normalize = 2", dict(normalize=2)),
                                       ("null pooled", dict(pooled=None, n=2, D=16)), ("null W", dict(W=None)),
                                       ("null b", dict(b=None, E=3))])
def test_head_refusals(what, over):
    pooled, W, b = R.head_case(16, 3, 2)
    a = dict(pooled=pooled, W=W, b=b, normalize=1)
    rc, emb = R.run_head(**a)
    assert rc == 0 and np.isfinite(emb[:2]).all()
    a.update(over)
    rc, emb = R.run_head(**a)
    assert rc == 1, what
    assert (emb.view(np.uint32) == F32_SENTINEL).all(), what


def test_head_refuses_null_output():
    import ctypes as C
    pooled, W, b = R.head_case(16, 3, 2)
    assert R._lib().wlx_spk_debug_head(0, R._p(pooled, C.c_float), R._p(W, C.c_float), R._p(b, C.c_float), 2, 16, 3, 1, None) == 1
