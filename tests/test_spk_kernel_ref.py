"""CPU tests of the ragged-filterbank and embedding-head references of tests/spk_kernel_ref.py: the references against plain numpy /
torch arithmetic, and the sensitivity guards of every input set of tests/test_gpu_spk_front_head_kernels.py — the nearest plausible
wrong answer of each kernel lies outside the bound the GPU test applies on the same inputs."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from . import spk_kernel_ref as R
from . import spk_oracle as O
from .test_gpu_spk_kernels import FBANK_ABS


# ------------------------------------------------------------------------------------------------ references
def test_fbank_batch_ref_is_the_oracle_per_window():
    pcm, offsets, frames = R.fbank_batch_case("n5")
    ref = R.fbank_batch_ref(pcm, offsets, frames)
    for i, (o, T) in enumerate(zip(offsets, frames)):
        alone = O.features(pcm[o:o + R.item_samples(int(T))])
        assert ref[i].shape == (T, 80) and np.array_equal(ref[i], alone)
    assert np.array_equal(ref[1], np.zeros((1, 80)))            # T = 1: the mean is the frame


def test_head_refs_match_torch():
    pooled, W, b = R.head_case(520, 257, 3)
    y = R.head_linear_ref(pooled, W, b)
    w16 = torch.from_numpy(W).half().double()
    want = torch.from_numpy(pooled).double() @ w16.T + torch.from_numpy(b).double()
    np.testing.assert_allclose(y, want.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(R.head_norm_ref(y), torch.nn.functional.normalize(want, dim=1).numpy(), rtol=1e-13, atol=1e-15)
    assert np.array_equal(R.head_norm_ref(np.zeros((2, 5))), np.zeros((2, 5)))


def test_head_linear_bound_covers_an_fp32_emulation_of_the_tree():
    """the kernel's order of operations in numpy float32 (products rounded, not fused) stays inside the bound: the bound is not
    tighter than fp32 arithmetic in that order can be"""
    for D, E, n in ((8, 1, 1), (520, 5, 2), (5120, 4, 1)):
        pooled, W, b = R.head_case(D, E, n, seed=3)
        trips = -(-D // 512)
        w = np.zeros((E, trips * 512), np.float32)
        w[:, :D] = R.f16(W).astype(np.float32)
        got = np.zeros((n, E))
        for r in range(n):
            x = np.zeros(trips * 512, np.float32)
            x[:D] = pooled[r]
            p = (w * x).reshape(E, trips, 64, 8).transpose(0, 2, 1, 3).reshape(E, 64, trips * 8)
            acc = np.zeros((E, 64), np.float32)
            for k in range(trips * 8):
                acc = acc + p[:, :, k]
            for o in (32, 16, 8, 4, 2, 1):
                acc = acc[:, :o] + acc[:, o:2 * o]
            got[r] = acc[:, 0] + b
        q = R.excess(got, R.head_linear_ref(pooled, W, b), R.head_linear_bound(pooled, W, b))
        assert 0 < q.max() <= 1.0, (D, E, n, q.max())


# ------------------------------------------------------------------------------------------------ guards: ragged filterbank
@pytest.mark.parametrize("name", [c for c in R.FBANK_CASES if c != "n1"])
def test_guard_fbank_batch_case(name):
    """an item read at its neighbour's sample offset, the mean taken over the neighbour's frame count, and the item started one packed
    frame late lie further from the float64 reference than FBANK_ABS, for every item the error can show on (an item of one frame is
    exactly zero from any offset)"""
    pcm, offsets, frames = R.fbank_batch_case(name)
    ref = R.fbank_batch_ref(pcm, offsets, frames)
    for wrong in ("offset", "mean", "in0"):
        bad = R.fbank_batch_ref(pcm, offsets, frames, wrong=wrong)
        for i, T in enumerate(frames):
            if wrong != "mean" and T == 1:               # (one frame minus its own mean: zero wherever it was read)
                continue
            assert np.abs(bad[i] - ref[i]).max() > 2 * FBANK_ABS, (wrong, i, int(T))     # outside the bound around anything inside it


def test_fbank_batch_cases_cover_the_edges():
    seen = set()
    for name in R.FBANK_CASES:
        pcm, offsets, frames = R.fbank_batch_case(name)
        assert len(pcm) == R.FBANK_SAMPLES and (offsets % 4 != 0).all() and (offsets % 2 == 1).all()
        assert (offsets + [R.item_samples(int(T)) for T in frames] <= len(pcm)).all()
        seen |= {int(T) for T in frames}
    assert seen == set(R.FBANK_FRAMES)
    assert [len(R.fbank_batch_case(c)[2]) for c in ("n1", "n2", "n5", "n64")] == [1, 2, 5, R.MAX_BATCH]
    _, offsets, frames = R.fbank_batch_case("overlap")
    assert offsets[0] < offsets[1] < offsets[0] + R.item_samples(int(frames[0])) - 250 * R.SHIFT         # 250 frames' worth shared
    _, offsets, _ = R.fbank_batch_case("descending")
    assert (np.diff(offsets) < 0).all()


# ------------------------------------------------------------------------------------------------ guards: head
def _outside(q):
    """per item: the share of outputs further than the bound from the reference"""
    return (q > 1.0).mean(axis=1)


@pytest.mark.parametrize("D,E,n", R.HEAD_CASES)
def test_guard_head_case(D, E, n):
    """the bias of output e + 1, a weight row read one element late, the last 8-wide piece of D dropped and the next item's pooled row
    lie outside the linear bound for at least nine outputs in ten of every item, and outside the bound behind the l2norm (where a
    common factor cancels, so E >= 3); the sum of squares over the first 256 outputs alone lies outside the normalised bound wherever
    E > 256"""
    pooled, W, b = R.head_case(D, E, n)
    y = R.head_linear_ref(pooled, W, b)
    by = R.head_linear_bound(pooled, W, b)
    z, bz = R.head_norm_ref(y), R.head_norm_bound(y, by)
    assert (by > 0).all() and (by < 1e-3 * np.abs(y).max()).all()
    kinds = ["wshift", "tail"] + (["bias"] if E > 1 else []) + (["item"] if n > 1 else [])
    for wrong in kinds:
        yw = R.head_linear_ref(pooled, W, b, wrong=wrong)
        assert (_outside(R.excess(yw, y, by)) >= 0.9).all(), wrong
        if E >= 3:
            assert (_outside(R.excess(R.head_norm_ref(yw), z, bz)) >= 0.9).all(), wrong
    if E > 256:
        assert (_outside(R.excess(R.head_norm_ref(y, wrong="ss256"), z, bz)) >= 0.9).all()


def test_guard_head_tiny_case():
    """the rows of the tiny case are what they claim, and a floor of 1e-30 under the sum of squares (the nearest wrong guard against
    the NaN of a zero row) leaves the 1e-18 row far outside its bound"""
    pooled, W, b = R.head_tiny_case()
    y = R.head_linear_ref(pooled, W, b)
    nrm = np.linalg.norm(y, axis=1)
    assert nrm[0] == 0 and 0.5e-18 < nrm[1] < 2e-18 and 0.1 < nrm[2] < 100 and 0.5e15 < nrm[3] < 2e15
    assert 2.0 ** -126 < (y[1] ** 2).sum() < 1e-35              # a normal fp32 number (its terms may be subnormal: head_norm_bound)
    by = R.head_linear_bound(pooled, W, b)
    z, bz = R.head_norm_ref(y), R.head_norm_bound(y, by)
    assert (by[0] == 0).all() and (bz[0] == 0).all() and (z[0] == 0).all()
    np.testing.assert_allclose(np.linalg.norm(z[1:], axis=1), 1.0, rtol=1e-14)
    floored = y / np.sqrt(np.maximum((y ** 2).sum(axis=1, keepdims=True), 1e-30))
    assert (R.excess(floored[1:2], z[1:2], bz[1:2]) > 1e3).all()
    assert R.excess(floored[2:], z[2:], bz[2:]).max() <= 1.0    # the floor changes nothing for ordinary rows
