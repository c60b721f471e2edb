"""GPU tests (-m gpu) of the long form of the offline clustering (include/wlx_spk_long.h): spk_ahc_long_kernel, one launch through
wlx_spk_debug_ahc_long, against file_diarization.cluster_host on the same matrix for EQUALITY of merges, heights (bit for bit), labels
and the cluster count — at the first size the short kernel refuses, across a rebuild of the live list and at the cap — and the two
entry points wlx_spk_cluster_long / wlx_spk_diarize_pcm_long on 2049 rows."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_spk_cluster_kernels as K
from tests import test_gpu_spk_diarize as T
from tests.test_gpu_spk_diarize import eng, slot, spk          # noqa: F401  (fixtures: the small seeded engines and the 12 s item)
from whisperlive_amd import _lib
from whisperlive_amd import file_diarization as FD

pytestmark = pytest.mark.gpu
F32P, I32P, I64P = K.F32P, K.I32P, T.I64P


@pytest.fixture(scope="module")
def lib(gpu):
    return _lib.load()


def ahc_long(lib, D, threshold, max_clusters=0, n=None):
    """-> (rc, labels, merges, heights, n_merges, K) of one wlx_spk_debug_ahc_long call, the outputs prefilled with sentinels"""
    n = D.shape[0] if n is None else n
    labels, merges, heights = np.full(max(n, 2), -7, np.int32), np.full((max(n, 2) - 1, 2), -7, np.int32), np.full(max(n, 2) - 1, K.SENTINEL, np.float32)
    nm, k = C.c_int32(-7), C.c_int32(-7)
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    rc = lib.wlx_spk_debug_ahc_long(0, D.ctypes.data_as(F32P), n, C.byref(opts), labels.ctypes.data_as(I32P), merges.ctypes.data_as(I32P),
                                    heights.ctypes.data_as(F32P), C.byref(nm), C.byref(k))
    return rc, labels, merges, heights, nm.value, k.value


def check(lib, D, threshold, max_clusters=0):
    want = FD.cluster_host(None, threshold, max_clusters, dist=D)
    rc, labels, merges, heights, nm, k = ahc_long(lib, D, threshold, max_clusters)
    assert rc == 0, lib.wlx_last_error()
    assert nm == len(want.merges)
    bad = np.nonzero((merges[:nm] != want.merges).any(axis=1))[0]
    assert bad.size == 0, ("first differing merge", int(bad[0]), merges[bad[0]].tolist(), want.merges[bad[0]].tolist())
    hb = np.nonzero(heights[:nm].view(np.uint32) != want.heights.view(np.uint32))[0]
    assert hb.size == 0, ("first differing height", int(hb[0]), float(heights[hb[0]]), float(want.heights[hb[0]]))
    assert np.array_equal(labels[:len(D)], want.labels) and k == int(want.labels.max()) + 1 == len(D) - nm
    assert (heights[nm:] == K.SENTINEL).all() and (merges[nm:] == -7).all(), "rows past n_merges were written"
    return want


def directions(n, seed, spread=0.03):
    """the distance matrix of unit rows of 256 around 8 directions, and how many of the directions are taken"""
    rng = np.random.default_rng(seed)
    planted = rng.integers(0, 8, size=n)
    X = np.linalg.qr(rng.standard_normal((256, 8)))[0].T[planted] + spread * rng.standard_normal((n, 256))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    return FD.cosine_distances(X), len(set(planted.tolist()))


@pytest.mark.parametrize("n", [2, 63, 1025, 2049, 4097])
def test_ahc_long_equals_the_host_oracle(lib, n):
    """2049: the first size the short kernel refuses; 4097: more than four columns per thread, and the live list is rebuilt on the way"""
    D, groups = directions(n, 50 + n)
    assert len(check(lib, D, 0.45).merges) == n - groups


@pytest.mark.parametrize("kind,threshold,cap", [("all equal", 0.6, 0), ("eighths", 0.6, 0), ("line", 1.9375, 0), ("even line", 0.6, 0),
                                                ("random", 0.0, 1500)])
def test_ahc_long_ties_chains_and_forced_merges(lib, kind, threshold, cap):
    """ties everywhere, ties among eighths, points on a line (every round invalidates cached neighbours), and max_clusters forcing
    merges past a threshold that allows none"""
    want = check(lib, K.matrices(2049)[kind], threshold, cap)
    assert cap == 0 or len(want.merges) == 2049 - cap


def test_ahc_long_at_the_cap(lib):
    """8192 random unit rows of 256 (pairwise distances far above 0.45: a dot of 0.55 is nine standard deviations of 1/16) and a planted
    group of 256 near-identical rows with rows 0, 8190 and 8191 in it: 255 merges, which the oracle makes within seconds"""
    n = _lib.SPK_LONG_MAX
    rng = np.random.default_rng(8192)
    X = rng.standard_normal((n, 256))
    group = np.concatenate([[0, n - 2, n - 1], rng.choice(np.arange(1, n - 2), 253, replace=False)])
    X[group] = X[0] + 0.01 * rng.standard_normal((256, 256))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    want = check(lib, FD.cosine_distances(X), 0.45)
    assert len(want.merges) == 255 and sorted(np.nonzero(want.labels == 0)[0].tolist()) == sorted(group.tolist())


def test_cluster_long_2049_rows(lib, spk):
    """wlx_spk_cluster_long (distance matrix, clustering and centroids of the long form; the matrix itself is held to its bound in the
    next test, which can download it): 8 well-separated directions, which the oracle recovers from its own matrix"""
    rng = np.random.default_rng(2049)
    planted = rng.integers(0, 8, size=2049)
    X = np.linalg.qr(rng.standard_normal((T.E, 8)))[0].T[planted] + 0.01 * rng.standard_normal((2049, T.E))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    want = FD.cluster_host(X, 0.45)
    assert int(want.labels.max()) == 7 and (want.labels[:, None] == want.labels[None, :]).tolist() == (planted[:, None] == planted[None, :]).tolist()
    labels, cent = spk.cluster_long(X, 0.45)
    assert np.array_equal(labels, want.labels) and cent.shape == (8, T.E) and np.abs(cent - want.centroids).max() <= 1e-5
    short, cent_short = spk.cluster(X[:2048], 0.45)                              # where both forms serve n: the same bits
    again, cent_again = spk.cluster_long(X[:2048], 0.45)
    assert np.array_equal(short, again) and np.array_equal(cent_short.view(np.uint32), cent_again.view(np.uint32))


def test_diarize_pcm_long_2049_windows(spk, slot):
    windows = [(80 * i, 4800) for i in range(2049)]
    windows[700] = (56000, 4799)
    labels, cent, emb, D = spk.diarize_resident_long(slot, 0, windows, 0.0, 5, want_embeddings=True, want_distances=True)
    rows = spk.embed_resident(slot, 0, windows)
    took = [i for i in range(2049) if i != 700]
    assert rows[700] is None and labels[700] == -1 and not emb[700].any() and D.shape == (2048, 2048)
    assert all((T._bits(emb[i]) == T._bits(rows[i])).all() for i in took), "rows differ from wlx_spk_embed_pcm_batch on the same ranges"
    X = emb[took].astype(np.float64)
    exact = 1.0 - X @ X.T
    np.fill_diagonal(exact, 0.0)
    assert np.abs(D - exact).max() <= K.AFFINITY_BOUND and np.array_equal(D, D.T) and (np.diag(D) == 0).all()
    want = FD.cluster_host(emb[took], 0.0, 5, dist=D)
    assert np.array_equal(labels[took], want.labels) and len(cent) == 5 and np.abs(cent - want.centroids).max() <= 1e-5
    # the statuses, raw: one short window among 2049
    o = diarize_long_raw(spk, slot, windows)
    assert o["rc"] == 0 and o["status"][700] == _lib.ERR_TOO_SHORT and (np.delete(o["status"], 700) == 0).all() and o["k"].value == 1


def diarize_long_raw(spk, slot, windows, n=None, threshold=2.0, max_clusters=0, null=()):
    starts, counts = np.array([a for a, _ in windows], dtype=np.int64), np.array([c for _, c in windows], dtype=np.int64)
    o = dict(labels=np.full(len(windows), -7, np.int32), status=np.full(len(windows), -7, np.int32), k=C.c_int32(-7))
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    args = [spk.h, slot.engine._h, slot.sid, 0, starts.ctypes.data_as(I64P), counts.ctypes.data_as(I64P), len(windows) if n is None else n,
            C.byref(opts), o["labels"].ctypes.data_as(I32P), o["status"].ctypes.data_as(I32P), None, None, None, C.byref(o["k"])]
    for i in null:
        args[i] = None
    o["rc"] = spk.lib.wlx_spk_diarize_pcm_long(*args)
    return o


def test_refusals_write_nothing(lib, spk, slot):
    D = K.matrices(4)["random"]
    for thr, cap, n in ((float("nan"), 0, None), (-0.125, 0, None), (2.125, 0, None), (0.5, -1, None), (0.5, 0, 0), (0.5, 0, _lib.SPK_LONG_MAX + 1)):
        rc, labels, merges, heights, nm, k = ahc_long(lib, D, thr, cap, n=n)
        assert rc == _lib.ERR_ARG and (labels == -7).all() and (merges == -7).all() and (heights == K.SENTINEL).all() and nm == k == -7, (thr, cap, n)
    assert lib.wlx_spk_debug_ahc_long(0, None, 4, None, None, None, None, None, None) == _lib.ERR_ARG
    windows = [(0, 4800)] * 4
    for kw in (dict(n=0), dict(n=_lib.SPK_LONG_MAX + 1), dict(threshold=2.125), dict(max_clusters=-1), dict(null=(4,)), dict(null=(8,)), dict(null=(13,))):
        o = diarize_long_raw(spk, slot, windows, **kw)
        assert o["rc"] == _lib.ERR_ARG and (o["labels"] == -7).all() and (o["status"] == -7).all() and o["k"].value == -7, kw
    X = K.unit_rows(4, T.E, seed=1)
    labels, k, opts = np.full(4, -7, np.int32), C.c_int32(-7), _lib.wlx_spk_cluster_opts(0.5, 0)
    for n, dim, emb in ((0, T.E, X), (_lib.SPK_LONG_MAX + 1, T.E, X), (4, T.E + 1, X), (4, T.E, None)):
        rc = spk.lib.wlx_spk_cluster_long(spk.h, emb.ctypes.data_as(F32P) if emb is not None else None, n, dim, C.byref(opts),
                                          labels.ctypes.data_as(I32P), None, C.byref(k))
        assert rc == _lib.ERR_ARG and (labels == -7).all() and k.value == -7, (n, dim)
