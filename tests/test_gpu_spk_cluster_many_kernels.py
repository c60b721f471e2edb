"""GPU tests (-m gpu) of the clustering kernels (whisperlive_amd/csrc/spk_cluster.hip) over tables of several files, one launch each through the
hooks wlx_spk_debug_affinity_many and wlx_spk_debug_ahc_many: files of different sizes packed into one call, every file's matrix
bit-equal to wlx_spk_debug_affinity on that file alone, and every file's merges, heights (bit for bit), labels and counts equal to
file_diarization.cluster_host on its matrix and to wlx_spk_debug_ahc — under a threshold and a max_clusters of its own. Rows are unit
vectors of 256 around 8 directions (scripts/spk_cluster_time.py), one file with duplicated rows for tied distances."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import file_diarization as FD

pytestmark = pytest.mark.gpu

F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
SENTINEL = 7.0
SIZES = [2, 3, 63, 64, 65, 130]          # one tile, its edge, one past it, three tiles across


@pytest.fixture(scope="module")
def lib(gpu):
    return _lib.load()


def rows_around(n, dim=256, speakers=8, seed=1):
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((dim, speakers)))[0].T
    x = centres[rng.integers(0, speakers, size=n)] + 0.03 * rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def affinity_one(lib, X):
    out = np.full((len(X), len(X)), SENTINEL, np.float32)
    assert lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(F32P), X.shape[0], X.shape[1], out.ctypes.data_as(F32P)) == 0
    return out


def affinity_many(lib, Xs):
    ns = np.array([len(X) for X in Xs], np.int32)
    packed = np.ascontiguousarray(np.concatenate(Xs))
    out = np.full(int((ns.astype(np.int64) ** 2).sum()), SENTINEL, np.float32)
    rc = lib.wlx_spk_debug_affinity_many(0, packed.ctypes.data_as(F32P), len(Xs), ns.ctypes.data_as(I32P), packed.shape[1], out.ctypes.data_as(F32P))
    assert rc == 0, lib.wlx_last_error()
    at = np.concatenate([[0], np.cumsum(ns.astype(np.int64) ** 2)])
    return [out[at[f]:at[f + 1]].reshape(n, n) for f, n in enumerate(ns)]


def ahc_one(lib, D, threshold, max_clusters):
    n = len(D)
    labels, merges, heights = np.full(n, -7, np.int32), np.full((max(n - 1, 1), 2), -7, np.int32), np.full(max(n - 1, 1), SENTINEL, np.float32)
    nm, k = C.c_int32(-7), C.c_int32(-7)
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    assert lib.wlx_spk_debug_ahc(0, D.ctypes.data_as(F32P), n, C.byref(opts), labels.ctypes.data_as(I32P), merges.ctypes.data_as(I32P),
                                 heights.ctypes.data_as(F32P), C.byref(nm), C.byref(k)) == 0
    return labels, merges[:nm.value], heights[:nm.value], k.value


def ahc_many(lib, Ds, options):
    """-> per file (labels, merges[:n_merges], heights[:n_merges], K, untouched): one wlx_spk_debug_ahc_many call; the matrices
    themselves must come back unchanged, and so must the rows of merges / heights no merge wrote (`untouched`)"""
    ns = np.array([len(D) for D in Ds], np.int32)
    packed = np.ascontiguousarray(np.concatenate([D.reshape(-1) for D in Ds]), dtype=np.float32)
    keep = packed.copy()
    rows = int(ns.sum())
    labels, merges, heights = np.full(rows, -7, np.int32), np.full((rows, 2), -7, np.int32), np.full(rows, SENTINEL, np.float32)
    nm, k = np.full(len(Ds), -7, np.int32), np.full(len(Ds), -7, np.int32)
    opts = (_lib.wlx_spk_cluster_opts * len(Ds))(*[_lib.wlx_spk_cluster_opts(t, c) for t, c in options])
    rc = lib.wlx_spk_debug_ahc_many(0, packed.ctypes.data_as(F32P), len(Ds), ns.ctypes.data_as(I32P), opts, labels.ctypes.data_as(I32P),
                                    merges.ctypes.data_as(I32P), heights.ctypes.data_as(F32P), nm.ctypes.data_as(I32P), k.ctypes.data_as(I32P))
    assert rc == 0, lib.wlx_last_error()
    assert np.array_equal(packed.view(np.uint32), keep.view(np.uint32)), "the hook wrote the caller's matrices"
    out, r0 = [], 0
    for f, n in enumerate(ns):
        m = int(nm[f])
        untouched = bool((merges[r0 + m:r0 + n] == -7).all() and (heights[r0 + m:r0 + n] == SENTINEL).all())
        out.append((labels[r0:r0 + n], merges[r0:r0 + m], heights[r0:r0 + m], int(k[f]), untouched))
        r0 += int(n)
    return out


def check_files(lib, Ds, options, single=True):
    got = ahc_many(lib, Ds, options)
    for f, (D, (thr, cap)) in enumerate(zip(Ds, options)):
        labels, merges, heights, K, untouched = got[f]
        want = FD.cluster_host(None, thr, cap, dist=D)
        what = (f, len(D), thr, cap)
        assert merges.tolist() == want.merges.tolist(), what
        assert np.array_equal(heights.view(np.uint32), want.heights.view(np.uint32)), what
        assert np.array_equal(labels, want.labels) and K == int(want.labels.max()) + 1 == len(D) - len(merges), what
        assert untouched, (what, "rows past n_merges were written")
        if single:
            l1, m1, h1, k1 = ahc_one(lib, D, thr, cap)
            assert np.array_equal(l1, labels) and np.array_equal(m1, merges) and np.array_equal(h1.view(np.uint32), heights.view(np.uint32)) and k1 == K, what
    return got


# ------------------------------------------------------------------------------------------------------------ distance matrices
@pytest.mark.parametrize("dim", [256, 20])          # 20: no multiple of the K slice of 16
def test_affinity_many_has_the_bits_of_the_single_launch(lib, dim):
    Xs = [rows_around(n, dim, seed=10 + n) for n in SIZES]
    Xs[3][7] = Xs[3][0]                             # equal rows: a distance of ~0 off the diagonal
    for f, (X, D) in enumerate(zip(Xs, affinity_many(lib, Xs))):
        assert np.array_equal(D.view(np.uint32), affinity_one(lib, X).view(np.uint32)), (f, len(X))
        assert np.array_equal(D.view(np.uint32), D.T.copy().view(np.uint32)), "not exactly symmetric"
        assert (np.diag(D).view(np.uint32) == 0).all(), "diagonal not exactly +0"


def test_affinity_many_order_and_a_single_file(lib):
    """the largest file first and last, and one file alone: a file's matrix does not depend on its neighbours or its place"""
    Xs = [rows_around(n, seed=30 + n) for n in (130, 2, 65)]
    a, b, c = affinity_many(lib, Xs), affinity_many(lib, Xs[::-1]), affinity_many(lib, Xs[:1])
    for f in range(3):
        assert np.array_equal(a[f].view(np.uint32), b[2 - f].view(np.uint32))
    assert np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ clustering
@pytest.fixture(scope="module")
def wave(lib):
    """the files of SIZES and one at the cap, the fourth with duplicated rows (tied distances); matrices from the device"""
    Xs = [rows_around(n, seed=50 + n) for n in SIZES + [_lib.SPK_CLUSTER_MAX]]
    Xs[3][1] = Xs[3][0]
    Xs[3][9] = Xs[3][8] = Xs[3][2]
    Xs[3][40] = Xs[3][41]
    Ds = affinity_many(lib, Xs)
    ties = Ds[3][np.triu_indices(len(Ds[3]), 1)]
    assert len(np.unique(ties)) < len(ties), "the tie file has no tied distances"
    return Ds


def test_cluster_host_is_deterministic_on_the_wave(wave):
    for D in wave[:-1]:
        a, b = FD.cluster_host(None, 0.45, dist=D), FD.cluster_host(None, 0.45, dist=D.copy())
        assert a.merges.tolist() == b.merges.tolist() and np.array_equal(a.heights.view(np.uint32), b.heights.view(np.uint32))


def test_ahc_many_equals_the_oracle_and_the_single_launch(lib, wave):
    """a threshold and a max_clusters per file: stopped part-way, run to one cluster, no merge at all, and caps that force merges past
    the threshold (8 directions want 8 clusters at 0.45; the caps ask for fewer)"""
    options = [(0.45, 0), (1.9375, 0), (0.45, 3), (0.45, 0), (0.0, 2), (0.03125, 5), (0.45, 0)]
    got = check_files(lib, wave, options)
    assert got[1][3] == 1 and got[2][3] <= 3 and got[4][3] == 2 and got[5][3] == 5 and got[6][3] == 8
    forced = FD.cluster_host(None, 0.45, 3, dist=wave[2])
    assert float(forced.heights.max()) > 0.45, "max_clusters forced no merge past the threshold"


def test_ahc_many_at_the_file_cap(lib):
    """WLX_SPK_MANY_MAX_FILES files of 2..5 rows in one call, options alternating"""
    Xs = [rows_around(2 + f % 4, seed=200 + f) for f in range(_lib.SPK_MANY_MAX_FILES)]
    Ds = affinity_many(lib, Xs)
    options = [((0.45, 0), (1.5, 0), (0.0, 2), (0.9, 1))[f % 4] for f in range(len(Xs))]
    check_files(lib, Ds, options, single=False)


def test_refusals_write_nothing(lib):
    X = rows_around(8, seed=1)
    ok = np.array([3, 5], np.int32)
    out = np.full(3 * 3 + 5 * 5, SENTINEL, np.float32)
    call = lambda n_files, ns, dim=256, x=X, o=out: lib.wlx_spk_debug_affinity_many(
        0, x.ctypes.data_as(F32P) if x is not None else None, n_files, ns.ctypes.data_as(I32P) if ns is not None else None, dim,
        o.ctypes.data_as(F32P) if o is not None else None)
    over = np.full(5, _lib.SPK_CLUSTER_MAX, np.int32)          # 10240 rows, 5 matrices at the cap: over both totals
    for what, rc in (("no file", call(0, ok)), ("65 files", call(65, np.full(65, 2, np.int32))), ("a file of 0 rows", call(2, np.array([3, 0], np.int32))),
                     ("a file over the cap", call(2, np.array([3, _lib.SPK_CLUSTER_MAX + 1], np.int32))), ("rows and matrices over the totals", call(5, over)),
                     ("dim 0", call(2, ok, dim=0)), ("dim 1025", call(2, ok, dim=1025)), ("null X", call(2, ok, x=None)), ("null ns", call(2, None)),
                     ("null out", call(2, ok, o=None))):
        assert rc == _lib.ERR_ARG and (out == SENTINEL).all(), what
    assert call(2, ok) == 0 and not (out == SENTINEL).any()
    D = np.ascontiguousarray(out)
    labels, merges, heights = np.full(8, -7, np.int32), np.full((8, 2), -7, np.int32), np.full(8, SENTINEL, np.float32)
    nm, k = np.full(2, -7, np.int32), np.full(2, -7, np.int32)

    def ahc(n_files=2, ns=ok, options=((0.5, 0), (0.5, 0)), null=None):
        opts = (_lib.wlx_spk_cluster_opts * len(options))(*[_lib.wlx_spk_cluster_opts(t, c) for t, c in options])
        args = [0, D.ctypes.data_as(F32P), n_files, ns.ctypes.data_as(I32P), opts, labels.ctypes.data_as(I32P), merges.ctypes.data_as(I32P),
                heights.ctypes.data_as(F32P), nm.ctypes.data_as(I32P), k.ctypes.data_as(I32P)]
        if null is not None:
            args[null] = None
        return lib.wlx_spk_debug_ahc_many(*args)
    cases = [("no file", dict(n_files=0)), ("a file of 0 rows", dict(ns=np.array([3, 0], np.int32))), ("NaN threshold", dict(options=((0.5, 0), (float("nan"), 0)))),
             ("threshold over 2", dict(options=((2.125, 0), (0.5, 0)))), ("negative max_clusters", dict(options=((0.5, 0), (0.5, -1))))]
    cases += [(f"null argument {i}", dict(null=i)) for i in (1, 3, 4, 5, 6, 7, 8, 9)]
    for what, kw in cases:
        assert ahc(**kw) == _lib.ERR_ARG, what
        assert (labels == -7).all() and (merges == -7).all() and (heights == SENTINEL).all() and (nm == -7).all() and (k == -7).all(), what
    assert ahc() == 0 and (k >= 1).all()
