"""GPU tests (-m gpu) of the clustering kernels (whisperlive_amd/csrc/spk_cluster.hip), one launch each through the hooks
wlx_spk_debug_affinity and wlx_spk_debug_ahc: the distance matrix against float64 NumPy within the bound of a 256-term float32 dot
product, and the one-workgroup average-linkage clustering against file_diarization.cluster_host for EQUALITY of merges, heights (bit
for bit), labels and the cluster count, on matrices built to tie, to chain and to sit at every size where the kernel changes its ways
(one row, one wave, one more than a wave, one more than the 1024-thread workgroup, the cap)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import file_diarization as FD

pytestmark = pytest.mark.gpu

F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
SENTINEL = 7.0
# |err| of a 256-term float32 dot product of unit rows, any summation order: gamma_256 * sum |x_i y_i| <= 256 * 2^-24 / (1 - 256 * 2^-24)
# = 1.53e-5, plus one rounding of the subtraction from 1
AFFINITY_BOUND = 1.6e-5


@pytest.fixture(scope="module")
def lib(gpu):
    return _lib.load()


def unit_rows(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def affinity(lib, X, n=None, dim=None, out=None):
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0] if n is None else n
    dim = X.shape[1] if dim is None else dim
    out = np.full((max(n, 1), max(n, 1)), SENTINEL, np.float32) if out is None else out
    rc = lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(F32P), n, dim, out.ctypes.data_as(F32P))
    return rc, out


def ahc(lib, D, threshold, max_clusters=0, n=None):
    """-> (rc, labels, merges[:n_merges], heights[:n_merges], K, raw) of one wlx_spk_debug_ahc call; D itself must come back unchanged"""
    D = np.ascontiguousarray(D, dtype=np.float32)
    keep = D.copy()
    n = D.shape[0] if n is None else n
    rows = max(n, 2)
    labels = np.full(rows, -7, np.int32)
    merges = np.full((rows - 1, 2), -7, np.int32)
    heights = np.full(rows - 1, SENTINEL, np.float32)
    nm, k = C.c_int32(-7), C.c_int32(-7)
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    rc = lib.wlx_spk_debug_ahc(0, D.ctypes.data_as(F32P), n, C.byref(opts), labels.ctypes.data_as(I32P), merges.ctypes.data_as(I32P),
                               heights.ctypes.data_as(F32P), C.byref(nm), C.byref(k))
    assert np.array_equal(D.view(np.uint32), keep.view(np.uint32)), "the hook wrote the caller's matrix"
    raw = (labels, merges, heights, nm.value, k.value)
    if rc != 0:
        return rc, None, None, None, None, raw
    return rc, labels[:n], merges[:nm.value], heights[:nm.value], k.value, raw


def check(lib, D, threshold, max_clusters=0, what=""):
    want = FD.cluster_host(None, threshold, max_clusters, dist=D)
    rc, labels, merges, heights, K, raw = ahc(lib, D, threshold, max_clusters)
    assert rc == 0, (what, _lib.load().wlx_last_error())
    n = D.shape[0]
    assert len(merges) == len(want.merges), (what, n, len(merges), len(want.merges))
    bad = np.nonzero((merges != want.merges).any(axis=1))[0]
    assert bad.size == 0, (what, n, "first differing merge", int(bad[0]), merges[bad[0]].tolist(), want.merges[bad[0]].tolist())
    hb = np.nonzero(heights.view(np.uint32) != want.heights.view(np.uint32))[0]
    assert hb.size == 0, (what, n, "first differing height", int(hb[0]), float(heights[hb[0]]), float(want.heights[hb[0]]))
    assert np.array_equal(labels, want.labels), (what, n)
    assert K == int(want.labels.max()) + 1 == n - len(merges), (what, n, K)
    assert (raw[2][len(merges):] == SENTINEL).all() and (raw[1][len(merges):] == -7).all(), (what, "rows past n_merges were written")
    return want


# ------------------------------------------------------------------------------------------------------------ distance matrix
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 2048])
def test_affinity_against_float64(lib, n):
    X = unit_rows(n, 256, seed=100 + n)
    rc, got = affinity(lib, X)
    assert rc == 0
    want = 1.0 - X.astype(np.float64) @ X.astype(np.float64).T
    np.fill_diagonal(want, 0.0)
    err = float(np.abs(got - want).max())
    print(f"n {n}: max |err| {err:.3e} (bound {AFFINITY_BOUND:.1e})")
    assert err <= AFFINITY_BOUND
    assert np.array_equal(got.view(np.uint32), got.T.copy().view(np.uint32)), "not exactly symmetric"
    assert (np.diag(got).view(np.uint32) == 0).all(), "diagonal not exactly +0"


def test_affinity_odd_width_and_equal_rows(lib):
    """a width that is no multiple of the K slice, and rows that repeat: distance ~0 off the diagonal, exactly 0 on it"""
    X = unit_rows(70, 50, seed=3)
    X[5] = X[64] = X[0]
    rc, got = affinity(lib, X)
    want = 1.0 - X.astype(np.float64) @ X.astype(np.float64).T
    np.fill_diagonal(want, 0.0)
    assert rc == 0 and float(np.abs(got - want).max()) <= AFFINITY_BOUND
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all() and abs(float(got[5, 64])) <= 2e-7


# ------------------------------------------------------------------------------------------------------------ clustering
def symmetric(upper):
    u = np.triu(upper.astype(np.float32), 1)
    return u + u.T


def matrices(n):
    """name -> symmetric float32 [n][n] with a zero diagonal and every other entry in [0.0625, 1.9]"""
    rng = np.random.default_rng(7000 + n)
    out = {"random": symmetric(rng.random((n, n)) * 1.8 + 0.0625)}
    equal = np.full((n, n), 0.5, np.float32)
    np.fill_diagonal(equal, 0.0)
    out["all equal"] = equal
    out["eighths"] = symmetric(rng.integers(1, 9, size=(n, n)) / 8.0)
    x = np.sort(rng.random(n)).astype(np.float32)
    out["line"] = (np.abs(x[:, None] - x[None, :]) * np.float32(1.8)).astype(np.float32) + np.float32(0.0625) * (1 - np.eye(n, dtype=np.float32))
    g = (np.arange(n, dtype=np.float32) / np.float32(max(n, 2)))          # evenly spaced: chains AND ties
    out["even line"] =(np.abs(g[:, None] - g[None, :]) * np.float32(1.8)).astype(np.float32) + np.float32(0.0625) * (1 - np.eye(n, dtype=np.float32))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 1025, 2048])
def test_ahc_equals_the_host_oracle(lib, n):
    """every kind of matrix stopped part-way and run to one cluster; up to 257 rows also every kind with every option, above that the
    options on the random matrix only (a run to the end at the cap costs the oracle a quarter of a second)"""
    for name, D in matrices(n).items():
        assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()
        check(lib, D, 0.6, what=name + ", threshold 0.6")
        one = check(lib, D, 1.9375, what=name + ", threshold above every distance")
        assert len(one.merges) == n - 1 and (one.labels == 0).all()
        if n > 257 and name != "random":
            continue
        none = check(lib, D, 0.03125, what=name + ", threshold below every distance")
        assert len(none.merges) == 0 and none.labels.tolist() == list(range(n))
        for thr in (0.25, 1.0):
            check(lib, D, thr, what=f"{name}, threshold {thr}")
        for cap in (1, 2, 5):
            forced = check(lib, D, 0.0, cap, what=f"{name}, max_clusters {cap}")
            assert int(forced.labels.max()) + 1 == min(cap, n)
        check(lib, D, 0.6, 2, what=name + ", threshold 0.6 and max_clusters 2")
    if n > 1:
        want = FD.cluster_host(None, 1.0, dist=matrices(n)["all equal"])
        assert want.merges.tolist() == [[0, k] for k in range(1, n)]              # index order, which the kernel equalled above


@pytest.mark.parametrize("n", [3, 63, 64, 65, 257, 1025, 2048])
def test_three_planted_blobs(lib, n):
    """three directions, members within cosine > 0.9 of one another and < 0.2 across: the labels are the planted partition, through
    the distance kernel and the clustering kernel (no case excluded: cluster_host itself must recover it, so a miss is the kernel's)"""
    rng = np.random.default_rng(9000 + n)
    centres = np.linalg.qr(rng.standard_normal((256, 3)))[0].T
    planted = rng.integers(0, 3, size=n)
    planted[:3] = [0, 1, 2]
    X = centres[planted] + 0.012 * rng.standard_normal((n, 256))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    cos = X.astype(np.float64) @ X.astype(np.float64).T
    together = planted[:, None] == planted[None, :]
    assert cos[together].min() > 0.9 and cos[~together].max() < 0.2
    host = FD.cluster_host(X, 0.45)
    assert np.array_equal(host.labels, planted), "cluster_host does not recover the planted partition"
    rc, D = affinity(lib, X)
    assert rc == 0
    got = check(lib, D, 0.45, what="blobs")
    assert np.array_equal(got.labels, planted)


def test_refusals_write_nothing(lib):
    X = unit_rows(4, 8, seed=1)
    for what, kw in (("n = 0", dict(n=0)), ("n over the cap", dict(n=_lib.SPK_CLUSTER_MAX + 1)), ("dim = 0", dict(dim=0)),
                     ("dim over 1024", dict(dim=1025))):
        rc, out = affinity(lib, X, **kw)
        assert rc == _lib.ERR_ARG and (out == SENTINEL).all(), what
    out = np.full((4, 4), SENTINEL, np.float32)
    assert lib.wlx_spk_debug_affinity(0, None, 4, 8, out.ctypes.data_as(F32P)) == _lib.ERR_ARG and (out == SENTINEL).all()
    assert lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(F32P), 4, 8, None) == _lib.ERR_ARG
    D = matrices(4)["random"]
    for what, thr, cap, n in (("NaN threshold", float("nan"), 0, None), ("negative threshold", -0.125, 0, None), ("threshold over 2", 2.125, 0, None),
                              ("negative max_clusters", 0.5, -1, None), ("n = 0", 0.5, 0, 0), ("n over the cap", 0.5, 0, _lib.SPK_CLUSTER_MAX + 1)):
        rc, *_, raw = ahc(lib, D, thr, cap, n=n)
        assert rc == _lib.ERR_ARG, what
        assert (raw[0] == -7).all() and (raw[1] == -7).all() and (raw[2] == SENTINEL).all() and raw[3] == -7 and raw[4] == -7, what
    opts = _lib.wlx_spk_cluster_opts(0.5, 0)
    labels, merges, heights = np.full(4, -7, np.int32), np.full((3, 2), -7, np.int32), np.full(3, SENTINEL, np.float32)
    nm, k = C.c_int32(-7), C.c_int32(-7)
    full = [0, D.ctypes.data_as(F32P), 4, C.byref(opts), labels.ctypes.data_as(I32P), merges.ctypes.data_as(I32P), heights.ctypes.data_as(F32P),
            C.byref(nm), C.byref(k)]
    for i in (1, 3, 4, 5, 6, 7, 8):
        args = list(full)
        args[i] = None
        assert lib.wlx_spk_debug_ahc(*args) == _lib.ERR_ARG, i
        assert (labels == -7).all() and (merges == -7).all() and (heights == SENTINEL).all() and nm.value == -7 and k.value == -7
    assert lib.wlx_spk_debug_ahc(*full) == 0 and k.value >= 1                       # the same arguments, complete, are served
