"""GPU tests (-m gpu) of offline diarization through the C-ABI: wlx_spk_diarize_pcm embeds a window grid of a slot item's resident PCM
in as many ragged passes as the engine's max_seconds needs and clusters the rows behind one wait; wlx_spk_cluster clusters host
embeddings. A small seeded speaker engine with max_seconds = 6, so that a dozen 1.5 s windows cross several passes. Rows against
wlx_spk_embed_pcm_batch bit for bit, labels against file_diarization.cluster_host on the matrix the device clustered."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import pytest

from tests import helpers as H
from whisperlive_amd import _lib, spk_weights
from whisperlive_amd import file_diarization as FD
from whisperlive_amd.diarization import SpeakerEmbedderHIP

pytestmark = pytest.mark.gpu

SPEC = spk_weights.SpkSpec(n_mels=16, planes=32, blocks=(1, 1, 1, 1), embed_dim=32, max_seconds=6)
E = SPEC.embed_dim
N = 12 * 16000                # samples resident in item 0
SENTINEL = 7.0
W = 24000                     # 1.5 s
# the grid 0, 0.75 s, ... (every window overlaps its neighbours), one range twice, one odd start and length, the shortest, the last samples
WINDOWS = [(k * 12000, W) for k in range(12)] + [(36000, W), (4001, 9999), (50, 4800), (N - W, W)]
F32P, I32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def spk(gpu):
    e = SpeakerEmbedderHIP(SPEC, spk_weights.fold(spk_weights.random_weights(SPEC, seed=11), SPEC), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


@pytest.fixture(scope="module")
def slot(eng):
    """item 0: 12 s whose colour changes every 3 s (two alternating noise colours); item 1 holds nothing"""
    rng = np.random.default_rng(2025)
    pieces = []
    for k in range(4):
        x = rng.standard_normal(3 * 16000)
        if k % 2:
            x = np.convolve(x, np.ones(24) / 24.0, mode="same") * 4.0
        pieces.append(0.1 * x)
    s = eng.create_slot(2, 5)
    s.pcm_put(np.concatenate(pieces).astype(np.float32))
    yield s
    s.close()


@pytest.fixture(scope="module")
def rows(spk, slot):
    """wlx_spk_embed_pcm_batch of every window of WINDOWS (in the groups its own cap needs), computed once before any diarize call"""
    assert slot.pcm_count() == N
    return spk.embed_resident(slot, 0, WINDOWS)


def diarize(spk, slot, item, windows, threshold=0.45, max_clusters=0, n=None, want=("emb", "dist", "cent")):
    """one raw wlx_spk_diarize_pcm call, every output prefilled with sentinels -> dict"""
    starts = np.array([a for a, _ in windows], dtype=np.int64)
    counts = np.array([c for _, c in windows], dtype=np.int64)
    n = len(windows) if n is None else n
    cap = max(len(windows), min(n, 4096), 1)
    o = dict(labels=np.full(cap, -7, np.int32), status=np.full(cap, -7, np.int32), emb=np.full((cap, E), SENTINEL, np.float32),
             dist=np.full((cap, cap), SENTINEL, np.float32), cent=np.full((cap, E), SENTINEL, np.float32), k=C.c_int32(-7))
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    p = lambda name: o[name].ctypes.data_as(F32P) if name in want else None
    o["rc"] = spk.lib.wlx_spk_diarize_pcm(spk.h, slot.engine._h, slot.sid, item, starts.ctypes.data_as(I64P), counts.ctypes.data_as(I64P), n,
                                          C.byref(opts), o["labels"].ctypes.data_as(I32P), o["status"].ctypes.data_as(I32P), p("emb"),
                                          p("dist"), p("cent"), C.byref(o["k"]))
    return o


def untouched(o):
    return ((o["labels"] == -7).all() and (o["status"] == -7).all() and (o["emb"] == SENTINEL).all() and (o["dist"] == SENTINEL).all()
            and (o["cent"] == SENTINEL).all() and o["k"].value == -7)


def cluster(spk, X, threshold, max_clusters=0, n=None, dim=None):
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0] if n is None else n
    dim = X.shape[1] if dim is None else dim
    labels, cent, k = np.full(X.shape[0], -7, np.int32), np.full(X.shape, SENTINEL, np.float32), C.c_int32(-7)
    opts = _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    rc = spk.lib.wlx_spk_cluster(spk.h, X.ctypes.data_as(F32P), n, dim, C.byref(opts), labels.ctypes.data_as(I32P), cent.ctypes.data_as(F32P),
                                 C.byref(k))
    return rc, labels, cent, k.value


def test_rows_labels_and_centroids(spk, slot, rows):
    before = slot.pcm()
    n = len(WINDOWS)
    assert sum(c for _, c in WINDOWS) > 3 * SPEC.max_seconds * 16000                # several passes
    o = diarize(spk, slot, 0, WINDOWS, threshold=2.0)
    assert o["rc"] == 0 and (o["status"][:n] == 0).all() and (o["labels"][:n] == 0).all() and o["k"].value == 1
    for i, r in enumerate(rows):
        assert (_bits(o["emb"][i]) == _bits(r)).all(), f"window {WINDOWS[i]} differs from wlx_spk_embed_pcm_batch on the same range"
    assert (_bits(o["emb"][3]) == _bits(o["emb"][12])).all()                        # the range given twice
    D = o["dist"][:n, :n].copy()
    X = o["emb"][:n].copy()
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()
    exact = 1.0 - X.astype(np.float64) @ X.astype(np.float64).T
    np.fill_diagonal(exact, 0.0)
    assert np.abs(D - exact).max() <= 32 * 2.0 ** -24 / (1 - 32 * 2.0 ** -24) + 2.0 ** -23      # a 32-term float32 dot product, one rounding of 1 - dot
    assert (o["dist"][n:] == SENTINEL).all() and (o["dist"][:, n:] == SENTINEL).all() and (o["emb"][n:] == SENTINEL).all()
    # thresholds from the matrix itself: its quartiles, so that the clustering stops part-way
    off = np.sort(D[np.triu_indices(n, 1)])
    for thr, cap in [(0.0, 0), (float(off[len(off) // 4]), 0), (float(off[len(off) // 2]), 0), (float(off[len(off) // 4]), 3), (0.0, 2)]:
        o = diarize(spk, slot, 0, WINDOWS, threshold=thr, max_clusters=cap)
        assert o["rc"] == 0
        assert np.array_equal(o["dist"][:n, :n].view(np.uint32), D.view(np.uint32))  # the same windows: the same matrix
        want = FD.cluster_host(X, thr, cap, dist=D)
        K = int(want.labels.max()) + 1
        print(f"threshold {thr:.4f} cap {cap}: {K} clusters, device ms {spk.cluster_timings()}")
        assert np.array_equal(o["labels"][:n], want.labels) and o["k"].value == K
        assert np.abs(o["cent"][:K] - want.centroids).max() <= 1e-5 and (o["cent"][K:] == SENTINEL).all()
        rc, labels, cent, k = cluster(spk, X, thr, cap)
        assert rc == 0 and np.array_equal(labels, o["labels"][:n]) and k == K
        assert np.abs(cent[:K] - want.centroids).max() <= 1e-5 and (cent[K:] == SENTINEL).all()
        if thr > 0:
            assert K <= n - 1                                                       # (windows 3 and 12 are one range: distance 0)
    # without the optional outputs: the same labels
    bare = diarize(spk, slot, 0, WINDOWS, threshold=float(off[len(off) // 2]), want=())
    assert bare["rc"] == 0
    mid = diarize(spk, slot, 0, WINDOWS, threshold=float(off[len(off) // 2]))
    assert np.array_equal(bare["labels"][:n], mid["labels"][:n]) and bare["k"].value == mid["k"].value
    assert (bare["emb"] == SENTINEL).all() and (bare["dist"] == SENTINEL).all() and (bare["cent"] == SENTINEL).all()
    # the Python face
    labels, cent, emb, dist = spk.diarize_resident(slot, 0, WINDOWS, float(off[len(off) // 2]), want_embeddings=True, want_distances=True)
    assert np.array_equal(labels, mid["labels"][:n]) and cent.shape == (mid["k"].value, E)
    assert (_bits(emb) == _bits(X)).all() and (_bits(dist) == _bits(D)).all()
    got_labels, got_cent = spk.cluster(X, float(off[len(off) // 2]))
    assert np.array_equal(got_labels, labels) and np.abs(got_cent - cent).max() <= 1e-6
    # the resident audio was only read
    after = slot.pcm()
    assert slot.pcm_count() == N and np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_dist_out_is_the_matrix_before_the_clustering(spk, slot):
    """dist_out against wlx_spk_debug_affinity on the returned rows, bit for bit: with 2 windows (one tile) and 65 (one row past a tile),
    with and without centroids behind the clustering. Threshold 2 merges everything, so the matrix on the device is overwritten in place
    down to one cluster: dist_out is the download made before that."""
    for m in (2, 65):
        windows = [(k * 2000, 4800 + 16 * k) for k in range(m)]                     # 0.3 s and a little more: several passes at m = 65
        for want in (("emb", "dist"), ("emb", "dist", "cent")):
            o = diarize(spk, slot, 0, windows, threshold=2.0, want=want)
            assert o["rc"] == 0 and o["k"].value == 1 and (o["labels"][:m] == 0).all() and (o["status"][:m] == 0).all()
            X = np.ascontiguousarray(o["emb"][:m])
            D = np.full((m, m), SENTINEL, np.float32)
            assert spk.lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(F32P), m, E, D.ctypes.data_as(F32P)) == 0
            assert (D != SENTINEL).all()
            assert (_bits(o["dist"]) == _bits(D)).all(), (m, want)
            assert (o["cent"] == SENTINEL).all() if "cent" not in want else (o["cent"][1:] == SENTINEL).all() and (o["cent"][0] != SENTINEL).all()


def test_a_short_window_in_the_middle(spk, slot, rows):
    windows = WINDOWS[:5] + [(20000, 4799)] + WINDOWS[5:9] + [(N, 0)]
    took = [i for i, (_, c) in enumerate(windows) if c >= 4800]
    full = diarize(spk, slot, 0, [windows[i] for i in took], threshold=0.0, max_clusters=3)
    o = diarize(spk, slot, 0, windows, threshold=0.0, max_clusters=3)
    n, m = len(windows), len(took)
    assert o["rc"] == 0 and o["status"][:n].tolist() == [0] * 5 + [_lib.ERR_TOO_SHORT] + [0] * 4 + [_lib.ERR_TOO_SHORT]
    assert o["labels"][5] == -1 and o["labels"][10] == -1 and (o["emb"][5] == 0).all() and (o["emb"][10] == 0).all()
    assert np.array_equal(o["labels"][took], full["labels"][:m]) and o["k"].value == full["k"].value == 3
    assert (_bits(o["emb"][took]) == _bits(full["emb"][:m])).all()
    # dist_out is [m][m], packed: m is not the caller's n here
    flat = o["dist"].reshape(-1)
    assert (_bits(flat[:m * m].reshape(m, m)) == _bits(full["dist"][:m, :m])).all() and (flat[m * m:] == SENTINEL).all()
    for i, w in zip(took, [0, 1, 2, 3, 4, 5, 6, 7, 8]):
        assert (_bits(o["emb"][i]) == _bits(rows[w])).all()
    # nothing long enough: WLX_OK, no cluster, nothing launched
    before = spk.timings()
    o = diarize(spk, slot, 0, [(0, 4799), (N - 10, 10)])
    assert o["rc"] == 0 and (o["status"][:2] == _lib.ERR_TOO_SHORT).all() and (o["labels"][:2] == -1).all() and o["k"].value == 0
    assert (o["emb"][:2] == 0).all() and (o["dist"] == SENTINEL).all() and (o["cent"] == SENTINEL).all() and spk.timings() == before


def test_one_window(spk, slot, rows):
    o = diarize(spk, slot, 0, WINDOWS[2:3])
    assert o["rc"] == 0 and o["labels"][0] == 0 and o["status"][0] == 0 and o["k"].value == 1 and o["dist"][0, 0] == 0
    assert (_bits(o["emb"][0]) == _bits(rows[2])).all() and (_bits(o["cent"][0]) == _bits(rows[2])).all()
    # one window that takes part beside a short one
    o = diarize(spk, slot, 0, [(0, 100), WINDOWS[2]])
    assert o["rc"] == 0 and o["labels"][:2].tolist() == [-1, 0] and o["k"].value == 1 and (_bits(o["emb"][1]) == _bits(rows[2])).all()
    rc, labels, cent, k = cluster(spk, rows[2][None, :], 0.45)
    assert rc == 0 and labels.tolist() == [0] and k == 1 and (_bits(cent[0]) == _bits(rows[2])).all()


def test_refusals_write_nothing(spk, slot, rows):
    nan = float("nan")
    cap = SPEC.max_seconds * 16000
    cases = [
        ("n = 0", dict(n=0), _lib.ERR_ARG),
        ("n over the cap", dict(windows=[(0, 4800)] * 4, n=_lib.SPK_CLUSTER_MAX + 1), _lib.ERR_ARG),
        ("NaN threshold", dict(threshold=nan), _lib.ERR_ARG),
        ("negative threshold", dict(threshold=-0.125), _lib.ERR_ARG),
        ("threshold over 2", dict(threshold=2.125), _lib.ERR_ARG),
        ("negative max_clusters", dict(max_clusters=-1), _lib.ERR_ARG),
        ("one window over max_seconds", dict(windows=WINDOWS[:2] + [(0, cap + 1)]), _lib.ERR_ARG),
        ("negative start", dict(windows=[(0, 4800), (-1, 4800)]), _lib.ERR_ARG),
        ("negative count", dict(windows=[(0, -1)]), _lib.ERR_ARG),
        ("item outside the slot", dict(item=2), _lib.ERR_ARG),
        ("no PCM resident in the item", dict(item=1), _lib.ERR_STATE),
        ("one sample past the resident count", dict(windows=WINDOWS[:3] + [(N - 4800 + 1, 4800)]), _lib.ERR_STATE),
    ]
    for what, kw, want in cases:
        kw = dict(dict(item=0, windows=WINDOWS[:4]), **kw)
        o = diarize(spk, slot, kw.pop("item"), kw.pop("windows"), **kw)
        assert o["rc"] == want, (what, o["rc"])
        assert untouched(o), what
    # a window of exactly max_seconds is served
    assert diarize(spk, slot, 0, [(0, cap), WINDOWS[0]])["rc"] == 0
    # null pointers
    a, c = np.array([0, 12000], np.int64), np.array([W, W], np.int64)
    labels, status, k = np.full(2, -7, np.int32), np.full(2, -7, np.int32), C.c_int32(-7)
    opts = _lib.wlx_spk_cluster_opts(0.45, 0)
    full = [spk.h, slot.engine._h, slot.sid, 0, a.ctypes.data_as(I64P), c.ctypes.data_as(I64P), 2, C.byref(opts), labels.ctypes.data_as(I32P),
            status.ctypes.data_as(I32P), None, None, None, C.byref(k)]
    for i in (0, 1, 4, 5, 7, 8, 9, 13):
        args = list(full)
        args[i] = None
        assert spk.lib.wlx_spk_diarize_pcm(*args) == _lib.ERR_ARG, i
        assert (labels == -7).all() and (status == -7).all() and k.value == -7
    assert spk.lib.wlx_spk_diarize_pcm(*full) == 0 and k.value in (1, 2)
    # wlx_spk_cluster
    X = np.stack(rows[:4])
    for what, kw in (("n = 0", dict(n=0)), ("n over the cap", dict(n=_lib.SPK_CLUSTER_MAX + 1)), ("another dim", dict(dim=E - 1)),
                     ("NaN threshold", dict(threshold=nan)), ("negative threshold", dict(threshold=-0.125)),
                     ("threshold over 2", dict(threshold=2.125)), ("negative max_clusters", dict(max_clusters=-1))):
        kw = dict(dict(threshold=0.45), **kw)
        rc, labels, cent, kk = cluster(spk, X, **kw)
        assert rc == _lib.ERR_ARG and (labels == -7).all() and (cent == SENTINEL).all() and kk == -7, what
    rc, labels, cent, kk = cluster(spk, X, 0.45)
    assert rc == 0 and 1 <= kk <= 4


def test_busy_slot_is_refused(spk, eng, slot):
    """a slot serves one call at a time: while a long generate runs on it in another thread, wlx_spk_diarize_pcm returns WLX_ERR_STATE
    and writes nothing"""
    ids = H.token_ids_for(H.TINY_EN.vocab)
    T = slot.logmel_resident(0)
    slot.encode(1, seek=[0], seg=[T - 1])
    started, stop = threading.Event(), threading.Event()

    def decode_loop():
        kw = dict(beam_size=5, max_length=300, suppress_tokens=H.default_suppress(ids) + [ids.eot])
        while not stop.is_set():
            try:
                started.set()
                slot.generate([[ids.sot]], H.engine_ids(ids), **kw)
            except _lib.WlxError as err:                    # (the diarize call got the slot first)
                assert err.code == _lib.ERR_STATE

    th = threading.Thread(target=decode_loop)
    th.start()
    seen = False
    try:
        started.wait()
        for _ in range(400):
            o = diarize(spk, slot, 0, WINDOWS[:2])
            if o["rc"] == _lib.ERR_STATE:
                assert untouched(o)
                seen = True
                break
            assert o["rc"] == 0
    finally:
        stop.set()
        th.join()
    assert seen
    assert slot.pcm_count() == N and diarize(spk, slot, 0, WINDOWS[:2])["rc"] == 0
