"""GPU tests (-m gpu) of wlx_spk_diarize_many through the C-ABI: a wave of files, each in an item of its own of one slot, embedded in
shared ragged passes and clustered side by side behind one wait. The yardstick is wlx_spk_diarize_pcm on each file alone (computed
once, before any many-call): labels, status, cluster counts, rows and centroids bit for bit — the same path on a wave of one, so
test_every_file_of_the_wave_against_independent_references anchors the wave to wlx_spk_embed_pcm_batch and cluster_host as well, and
test_the_shared_buffers_hold_no_state runs the three clustering calls after one another on one engine. A small seeded speaker engine
with max_seconds = 6 (four 1.5 s windows per pass), so that passes end inside files and span files.
(The matrix cap WLX_SPK_MANY_MAX_CELLS cannot be passed by arguments the other caps admit — at most 8192 rows in files of at most
2048 give at most 4 x 2048^2 cells — so its refusal has no case here; diarization.plan_diarize_many is tested on it with caps of its own.)"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from whisperlive_amd import _lib, spk_weights
from whisperlive_amd.diarization import SpeakerEmbedderHIP

pytestmark = pytest.mark.gpu

SPEC = spk_weights.SpkSpec(n_mels=16, planes=32, blocks=(1, 1, 1, 1), embed_dim=32, max_seconds=6)
E = SPEC.embed_dim
SENTINEL = 7.0
W = 24000                     # 1.5 s
ITEMS = 6
SECONDS = {0: 12.0, 1: 7.0, 2: 3.1, 4: 2.0, 5: 9.0}          # item 3 holds nothing; item 5 is the slot's last: the largest offset
F32P, I32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def grid(seconds, hop=12000):
    n = int(seconds * 16000)
    return [(a, W) for a in range(0, n - W + 1, hop)]


# file -> (item, windows, threshold, max_clusters). Passes of four windows: the first file's five windows end one pass inside it, the
# second pass spans files "a" and "b", and so on down the wave
FILES = {
    "a": (0, grid(12.0)[:5], 0.45, 0),
    "b": (1, grid(7.0) + [(100, 4799)] + [(7 * 16000 - 9999, 9999)], 0.0, 2),          # a short window inside, an odd one at the very end
    "last": (5, grid(9.0, 8000), 0.02, 3),
    "one": (2, [(0, 100), (1600, W)], 0.45, 0),                                       # m = 1 beside a short window
    "none": (4, [(0, 4799), (32000 - 10, 10)], 0.45, 0),                               # m = 0: only short windows
    "long": (0, grid(12.0) + [(36000, W), (4001, 9999)], 1.0, 0),                      # (item 0 again: never in one call with "a")
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def spk(gpu):
    e = SpeakerEmbedderHIP(SPEC, spk_weights.fold(spk_weights.random_weights(SPEC, seed=11), SPEC), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def slot(gpu):
    """every item its own audio: noise whose colour changes every 1.5 s, seeded per item"""
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    s = eng.create_slot(ITEMS, 5)
    for item, seconds in SECONDS.items():
        rng = np.random.default_rng(300 + item)
        x = rng.standard_normal(int(seconds * 16000))
        for k, at in enumerate(range(0, len(x), W)):
            if (k + item) % 2:
                x[at:at + W] = np.convolve(x[at:at + W], np.ones(24) / 24.0, mode="same") * 4.0
        s.pcm_put((0.1 * x).astype(np.float32), item=item)
    yield s
    s.close()
    eng.close()


def single(spk, slot, item, windows, threshold, max_clusters):
    """wlx_spk_diarize_pcm on one file, sentinels behind what it writes -> dict"""
    n = len(windows)
    starts, counts = np.array([a for a, _ in windows], np.int64), np.array([c for _, c in windows], np.int64)
    o = dict(labels=np.full(n, -7, np.int32), status=np.full(n, -7, np.int32), emb=np.full((n, E), SENTINEL, np.float32),
             cent=np.full((n, E), SENTINEL, np.float32))
    k, opts = C.c_int32(-7), _lib.wlx_spk_cluster_opts(threshold, max_clusters)
    o["rc"] = spk.lib.wlx_spk_diarize_pcm(spk.h, slot.engine._h, slot.sid, item, starts.ctypes.data_as(I64P), counts.ctypes.data_as(I64P), n,
                                          C.byref(opts), o["labels"].ctypes.data_as(I32P), o["status"].ctypes.data_as(I32P),
                                          o["emb"].ctypes.data_as(F32P), None, o["cent"].ctypes.data_as(F32P), C.byref(k))
    o["k"] = k.value
    return o


@pytest.fixture(scope="module")
def alone(spk, slot):
    """every file of FILES through wlx_spk_diarize_pcm, once, before any many-call"""
    got = {name: single(spk, slot, *f) for name, f in FILES.items()}
    assert all(o["rc"] == 0 for o in got.values())
    return got


def many(spk, slot, files, want=("emb", "cent"), null=None, n_files=None, items=None):
    """one raw wlx_spk_diarize_many call over `files` [(item, windows, threshold, max_clusters)], outputs prefilled with sentinels"""
    counts = np.array([len(f[1]) for f in files], np.int32)
    flat = [w for f in files for w in f[1]]
    total = max(len(flat), 1)
    starts, samples = np.array([a for a, _ in flat] or [0], np.int64), np.array([c for _, c in flat] or [0], np.int64)
    its = np.array([f[0] for f in files] if items is None else items, np.int32)
    opts = (_lib.wlx_spk_cluster_opts * len(files))(*[_lib.wlx_spk_cluster_opts(f[2], f[3]) for f in files])
    o = dict(labels=np.full(total, -7, np.int32), status=np.full(total, -7, np.int32), fstat=np.full(len(files), -7, np.int32),
             k=np.full(len(files), -7, np.int32), emb=np.full((total, E), SENTINEL, np.float32), cent=np.full((total, E), SENTINEL, np.float32))
    p = lambda name: o[name].ctypes.data_as(F32P) if name in want else None
    args = [spk.h, slot.engine._h, slot.sid, len(files) if n_files is None else n_files, its.ctypes.data_as(I32P), counts.ctypes.data_as(I32P),
            starts.ctypes.data_as(I64P), samples.ctypes.data_as(I64P), opts, o["labels"].ctypes.data_as(I32P), o["status"].ctypes.data_as(I32P),
            o["fstat"].ctypes.data_as(I32P), o["k"].ctypes.data_as(I32P), p("emb"), p("cent")]
    if null is not None:
        args[null] = None
    o["rc"] = spk.lib.wlx_spk_diarize_many(*args)
    o["at"] = np.concatenate([[0], np.cumsum(counts)])
    return o


def untouched(o):
    return all((o[name] == -7).all() for name in ("labels", "status", "fstat", "k")) and (o["emb"] == SENTINEL).all() and (o["cent"] == SENTINEL).all()


def same_as_alone(o, f, want, what):
    """file f of the many-call `o` against its wlx_spk_diarize_pcm result `want`, every output bit for bit"""
    a, b = int(o["at"][f]), int(o["at"][f + 1])
    assert o["fstat"][f] == 0 and o["k"][f] == want["k"], (what, int(o["fstat"][f]), int(o["k"][f]), want["k"])
    assert np.array_equal(o["labels"][a:b], want["labels"]) and np.array_equal(o["status"][a:b], want["status"]), what
    assert (_bits(o["emb"][a:b]) == _bits(want["emb"])).all(), (what, "rows differ from wlx_spk_diarize_pcm")
    K = want["k"]
    assert (_bits(o["cent"][a:a + K]) == _bits(want["cent"][:K])).all(), (what, "centroids differ from wlx_spk_diarize_pcm")
    assert (o["cent"][a + K:b] == SENTINEL).all(), (what, "centroid rows past K were written")


def test_every_file_equals_the_single_call(spk, slot, alone):
    before = {item: slot.pcm(item) for item in SECONDS}
    names = ["a", "b", "last", "one", "none"]
    assert len(FILES["a"][1]) % 4 == 1 and sum(len(FILES[n][1]) for n in names) > 16          # passes end inside files and span them
    o = many(spk, slot, [FILES[n] for n in names])
    assert o["rc"] == 0, spk.lib.wlx_last_error()
    for f, name in enumerate(names):
        same_as_alone(o, f, alone[name], name)
    assert alone["one"]["k"] == 1 and alone["none"]["k"] == 0 and alone["b"]["k"] == 2 and 1 <= alone["last"]["k"] <= 3
    assert (alone["none"]["labels"] == -1).all() and alone["b"]["status"].tolist().count(_lib.ERR_TOO_SHORT) == 1
    # another order, other neighbours, the longest file: a file's results do not depend on the wave around it
    for names in (["none", "last", "long", "one"], ["long"], ["one"], ["none", "one"]):
        o = many(spk, slot, [FILES[n] for n in names])
        assert o["rc"] == 0
        for f, name in enumerate(names):
            same_as_alone(o, f, alone[name], name)
    # without the optional outputs: the same labels and counts
    bare = many(spk, slot, [FILES[n] for n in ("a", "b", "one")], want=())
    full = many(spk, slot, [FILES[n] for n in ("a", "b", "one")])
    assert bare["rc"] == 0 and np.array_equal(bare["labels"], full["labels"]) and np.array_equal(bare["k"], full["k"])
    assert (bare["emb"] == SENTINEL).all() and (bare["cent"] == SENTINEL).all()
    # the resident audio was only read
    for item, pcm in before.items():
        assert np.array_equal(pcm.view(np.uint32), slot.pcm(item).view(np.uint32))


def test_every_file_of_the_wave_against_independent_references(spk, slot):
    """the wave of test_every_file_equals_the_single_call anchored to what shares no clustering code with it: every row to
    wlx_spk_embed_pcm_batch on the same range bit for bit; labels and K to file_diarization.cluster_host on the matrix
    wlx_spk_debug_affinity gives for the file's returned rows (the matrix the device clustered, so no threshold sits on a rounding
    difference); centroids to cluster_host's within the 1e-5 of test_gpu_spk_diarize.py"""
    from whisperlive_amd import file_diarization as FD
    names = ["a", "b", "last", "one", "none"]
    want_rows = {n: spk.embed_resident(slot, FILES[n][0], FILES[n][1]) for n in names}          # before the many-call
    o = many(spk, slot, [FILES[n] for n in names])
    assert o["rc"] == 0, spk.lib.wlx_last_error()
    for f, name in enumerate(names):
        _item, windows, thr, cap = FILES[name]
        a, b = int(o["at"][f]), int(o["at"][f + 1])
        took = [i for i, (_, c) in enumerate(windows) if c >= _lib.SPK_MIN_SAMPLES]
        m = len(took)
        assert o["fstat"][f] == 0
        for i, row in enumerate(want_rows[name]):
            assert (row is None) == (i not in took)
            if row is None:
                assert o["status"][a + i] == _lib.ERR_TOO_SHORT and o["labels"][a + i] == -1 and (o["emb"][a + i] == 0).all(), (name, i)
            else:
                assert o["status"][a + i] == 0 and (_bits(o["emb"][a + i]) == _bits(row)).all(), (name, i, "differs from wlx_spk_embed_pcm_batch")
        if m == 0:
            assert o["k"][f] == 0 and (o["cent"][a:b] == SENTINEL).all()
            continue
        X = np.ascontiguousarray(o["emb"][a:b][took])
        D = np.full((m, m), SENTINEL, np.float32)
        assert spk.lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(F32P), m, E, D.ctypes.data_as(F32P)) == 0
        want = FD.cluster_host(X, thr, cap, dist=D)
        K = int(want.labels.max()) + 1
        assert o["k"][f] == K and np.array_equal(o["labels"][a:b][took], want.labels), (name, K, int(o["k"][f]))
        assert np.abs(o["cent"][a:a + K] - want.centroids).max() <= 1e-5 and (o["cent"][a + K:b] == SENTINEL).all(), name
    assert [int(k) for k in o["k"]][3:] == [1, 0] and o["k"][1] == 2 and 1 <= o["k"][2] <= 3


# ---- the one table behind every clustering call: the three calls of test_the_shared_buffers_hold_no_state, outputs padded with sentinels
PAD = 3
WAVE = [(0, grid(12.0)[:5], 0.45, 0), (1, [(0, W), (100, 4799), (12000, W)], 0.0, 2), (5, grid(9.0)[:3], 0.02, 3)]          # 5, 2 and 3 windows take part
PCM_WINDOWS = [(0, W), (50, 100), (24000, W), (36000, 9999)]                                                               # 3 of 4 take part


def _call_wave(spk, slot):
    total = sum(len(f[1]) for f in WAVE)
    counts = np.array([len(f[1]) for f in WAVE], np.int32)
    flat = [w for f in WAVE for w in f[1]]
    starts, samples = np.array([a for a, _ in flat], np.int64), np.array([c for _, c in flat], np.int64)
    its = np.array([f[0] for f in WAVE], np.int32)
    opts = (_lib.wlx_spk_cluster_opts * len(WAVE))(*[_lib.wlx_spk_cluster_opts(f[2], f[3]) for f in WAVE])
    o = dict(labels=np.full(total + PAD, -7, np.int32), status=np.full(total + PAD, -7, np.int32), fstat=np.full(len(WAVE) + PAD, -7, np.int32),
             k=np.full(len(WAVE) + PAD, -7, np.int32), emb=np.full((total + PAD, E), SENTINEL, np.float32),
             cent=np.full((total + PAD, E), SENTINEL, np.float32))
    rc = spk.lib.wlx_spk_diarize_many(spk.h, slot.engine._h, slot.sid, len(WAVE), its.ctypes.data_as(I32P), counts.ctypes.data_as(I32P),
                                      starts.ctypes.data_as(I64P), samples.ctypes.data_as(I64P), opts, o["labels"].ctypes.data_as(I32P),
                                      o["status"].ctypes.data_as(I32P), o["fstat"].ctypes.data_as(I32P), o["k"].ctypes.data_as(I32P),
                                      o["emb"].ctypes.data_as(F32P), o["cent"].ctypes.data_as(F32P))
    assert rc == 0, spk.lib.wlx_last_error()
    # behind every written range: the pads, and the centroid rows past each file's K
    assert all((o[n][-PAD:] == -7).all() for n in ("labels", "status", "fstat", "k")) and (o["emb"][-PAD:] == SENTINEL).all()
    at = 0
    for f, n in enumerate(counts):
        assert 1 <= o["k"][f] <= n and (o["cent"][at + o["k"][f]:at + n] == SENTINEL).all()
        at += n
    assert (o["cent"][at:] == SENTINEL).all() and (o["status"][:total] != -7).all() and (o["emb"][:total] != SENTINEL).all()
    return o


def _call_pcm(spk, slot):
    n, m = len(PCM_WINDOWS), 3
    starts, counts = np.array([a for a, _ in PCM_WINDOWS], np.int64), np.array([c for _, c in PCM_WINDOWS], np.int64)
    o = dict(labels=np.full(n + PAD, -7, np.int32), status=np.full(n + PAD, -7, np.int32), emb=np.full((n + PAD, E), SENTINEL, np.float32),
             dist=np.full(m * m + PAD, SENTINEL, np.float32), cent=np.full((n + PAD, E), SENTINEL, np.float32), k=np.full(1 + PAD, -7, np.int32))
    opts = _lib.wlx_spk_cluster_opts(0.0, 2)
    rc = spk.lib.wlx_spk_diarize_pcm(spk.h, slot.engine._h, slot.sid, 0, starts.ctypes.data_as(I64P), counts.ctypes.data_as(I64P), n, C.byref(opts),
                                     o["labels"].ctypes.data_as(I32P), o["status"].ctypes.data_as(I32P), o["emb"].ctypes.data_as(F32P),
                                     o["dist"].ctypes.data_as(F32P), o["cent"].ctypes.data_as(F32P), o["k"].ctypes.data_as(I32P))
    assert rc == 0, spk.lib.wlx_last_error()
    assert o["k"][0] == 2 and o["status"][:n].tolist() == [0, _lib.ERR_TOO_SHORT, 0, 0] and o["labels"][1] == -1
    assert (o["labels"][-PAD:] == -7).all() and (o["status"][-PAD:] == -7).all() and (o["k"][1:] == -7).all()
    assert (o["emb"][n:] == SENTINEL).all() and (o["dist"][m * m:] == SENTINEL).all() and (o["cent"][2:] == SENTINEL).all()
    assert (o["emb"][:n] != SENTINEL).all() and (o["dist"][:m * m] != SENTINEL).all() and (o["cent"][:2] != SENTINEL).all()
    return o


def _call_cluster(spk, slot):
    X = np.random.default_rng(41).standard_normal((3, E))
    X = np.ascontiguousarray(X / np.linalg.norm(X, axis=1, keepdims=True), dtype=np.float32)
    o = dict(labels=np.full(3 + PAD, -7, np.int32), cent=np.full((3 + PAD, E), SENTINEL, np.float32), k=np.full(1 + PAD, -7, np.int32))
    opts = _lib.wlx_spk_cluster_opts(0.0, 2)
    rc = spk.lib.wlx_spk_cluster(spk.h, X.ctypes.data_as(F32P), 3, E, C.byref(opts), o["labels"].ctypes.data_as(I32P), o["cent"].ctypes.data_as(F32P),
                                 o["k"].ctypes.data_as(I32P))
    assert rc == 0, spk.lib.wlx_last_error()
    assert o["k"][0] == 2 and sorted(o["labels"][:3].tolist()) in ([0, 0, 1], [0, 1, 1])
    assert (o["labels"][3:] == -7).all() and (o["k"][1:] == -7).all() and (o["cent"][2:] == SENTINEL).all() and (o["cent"][:2] != SENTINEL).all()
    return o


def test_the_shared_buffers_hold_no_state(gpu, slot):
    """one table, one matrix area and one set of pinned landing buffers serve wlx_spk_diarize_many, wlx_spk_diarize_pcm and
    wlx_spk_cluster. On ONE engine: a wave of three files (5, 2 and 3 windows take part), a wlx_spk_diarize_pcm of 4 windows (one short)
    with dist_out, a wlx_spk_cluster of 3 host rows, the wave again — a small file after a larger one on the same rows, on matrix offset 0
    and in the same landing buffers. Every output of every call, its sentinel pads included, has the bits the same call gives as the
    FIRST clustering call of a fresh engine."""
    def fresh():
        return SpeakerEmbedderHIP(SPEC, spk_weights.fold(spk_weights.random_weights(SPEC, seed=11), SPEC), device=0)

    first = {}
    for call in (_call_wave, _call_pcm, _call_cluster):
        e = fresh()
        try:
            first[call] = call(e, slot)
        finally:
            e.close()
    e = fresh()
    try:
        for step, call in enumerate((_call_wave, _call_pcm, _call_cluster, _call_wave)):
            got = call(e, slot)
            for name, want in first[call].items():
                same = (_bits(got[name]) == _bits(want)).all() if want.dtype == np.float32 else np.array_equal(got[name], want)
                assert same, (step, call.__name__, name, "differs from the first clustering call of a fresh engine")
    finally:
        e.close()


def test_the_python_face(spk, slot, alone):
    names = ["a", "b", "last", "one", "none"]
    got = spk.diarize_many(slot, [FILES[n][0] for n in names], [FILES[n][1] for n in names], [FILES[n][2] for n in names],
                           [FILES[n][3] for n in names], want_embeddings=True)
    for name, (labels, cent, emb) in zip(names, got):
        want = alone[name]
        assert np.array_equal(labels, want["labels"]) and cent.shape == (want["k"], E)
        assert (_bits(cent) == _bits(want["cent"][:want["k"]])).all() and (_bits(emb) == _bits(want["emb"])).all()
    one = spk.diarize_resident(slot, 5, FILES["last"][1], 0.02, 3)
    assert np.array_equal(one[0], got[2][0]) and (_bits(one[1]) == _bits(got[2][1])).all()
    # an item that holds nothing: that file's own error, returned in its place
    got = spk.diarize_many(slot, [0, 3, 5], [FILES["a"][1], [(0, W)], FILES["last"][1]], [0.45, 0.45, 0.02], [0, 0, 3])
    assert isinstance(got[1], _lib.WlxError) and got[1].code == _lib.ERR_STATE
    assert np.array_equal(got[0][0], alone["a"]["labels"]) and np.array_equal(got[2][0], alone["last"]["labels"])


def test_a_file_that_is_not_resident_costs_only_itself(spk, slot, alone):
    empty = (3, [(0, W), (12000, W)], 0.45, 0)                                          # nothing was ever put into item 3
    past = (1, grid(7.0)[:3] + [(7 * 16000 - 4800 + 1, 4800)], 0.45, 0)                 # one sample past the resident count
    for bad, where in ((empty, 1), (past, 0), (empty, 2)):
        files = [FILES["a"], FILES["last"]]
        files.insert(where, bad)
        o = many(spk, slot, files)
        assert o["rc"] == 0
        a, b = int(o["at"][where]), int(o["at"][where + 1])
        assert o["fstat"][where] == _lib.ERR_STATE and o["k"][where] == 0 and (o["labels"][a:b] == -1).all()
        assert (o["status"][a:b] == _lib.ERR_STATE).all() and (o["emb"][a:b] == 0).all() and (o["cent"][a:b] == SENTINEL).all()
        for f, name in ((0 if where else 1, "a"), (1 if where == 2 else 2, "last")):
            same_as_alone(o, f, alone[name], name)
    o = many(spk, slot, [empty])                                                        # alone: WLX_OK, nothing launched
    assert o["rc"] == 0 and o["fstat"][0] == _lib.ERR_STATE and o["k"][0] == 0


def test_refusals_write_nothing(spk, slot, alone):
    cap = SPEC.max_seconds * 16000
    a, b = FILES["a"], FILES["b"]
    short = [(0, 100)]
    cases = [
        ("no file", dict(files=[a], n_files=0)),
        ("65 files", dict(files=[a], n_files=_lib.SPK_MANY_MAX_FILES + 1)),
        ("a file over WLX_SPK_CLUSTER_MAX windows", dict(files=[a, (1, short * (_lib.SPK_CLUSTER_MAX + 1), 0.45, 0)])),
        ("over WLX_SPK_MANY_MAX_ROWS windows in all", dict(files=[(i, short * _lib.SPK_CLUSTER_MAX, 0.45, 0) for i in (0, 1, 2, 4)] + [(5, short, 0.45, 0)])),
        ("NaN threshold", dict(files=[a, (1, b[1], float("nan"), 0)])),
        ("threshold over 2", dict(files=[(0, a[1], 2.125, 0), b])),
        ("negative max_clusters", dict(files=[a, (1, b[1], 0.45, -1)])),
        ("negative start", dict(files=[a, (1, [(0, W), (-1, W)], 0.45, 0)])),
        ("negative count", dict(files=[a, (1, [(0, -1)], 0.45, 0)])),
        ("a window over max_seconds", dict(files=[a, (1, [(0, cap + 1)], 0.45, 0)])),
        ("an item outside the slot", dict(files=[a, (ITEMS, b[1], 0.45, 0)])),
        ("a negative item", dict(files=[a, (-1, b[1], 0.45, 0)])),
        ("an item named twice", dict(files=[a, b, FILES["long"]])),
    ]
    for what, kw in cases:
        o = many(spk, slot, **kw)
        assert o["rc"] == _lib.ERR_ARG, (what, o["rc"])
        assert untouched(o), what
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12):                                       # every required pointer
        o = many(spk, slot, [a, b], null=i)
        assert o["rc"] == _lib.ERR_ARG and untouched(o), i
    # the rows cap itself is served: 8192 windows, all of them too short, nothing to launch
    o = many(spk, slot, [(i, short * _lib.SPK_CLUSTER_MAX, 0.45, 0) for i in (0, 1, 2, 4)], want=())
    assert o["rc"] == 0 and (o["k"] == 0).all() and (o["status"] == _lib.ERR_TOO_SHORT).all()
    # a window of exactly max_seconds is served, and the complete arguments of the cases above are
    assert many(spk, slot, [(0, [(0, cap), (0, W)], 0.45, 0), b])["rc"] == 0
    o = many(spk, slot, [a, b])
    assert o["rc"] == 0
    same_as_alone(o, 0, alone["a"], "a")
    same_as_alone(o, 1, alone["b"], "b")


def test_cluster_timings_report_the_many_call(spk, slot, alone):
    assert many(spk, slot, [FILES["a"], FILES["b"], FILES["last"]])["rc"] == 0
    aff, ahc = spk.cluster_timings()
    print(f"wlx_spk_diarize_many, 3 files: distance matrices {aff:.3f} ms, clustering {ahc:.3f} ms (HIP events)")
    assert 0.0 < aff < 50.0 and 0.0 < ahc < 50.0


# ------------------------------------------------------------------------------------------------------------ end to end
def test_transcribe_many_with_diarize_equals_the_per_file_route(gpu, spk):
    """three files (a WAV, a FLAC, a waveform) as one job with wave_put and diarize: ONE diarize_many call behind the wave's last decode
    group, and on every file the speakers of segments and words that transcribe + FileDiarizer.diarize give for that file alone
    (rest.diarize_file_segments, the `diarize=true` route of one upload)"""
    from tests import batched_common as BC
    from tests import test_gpu_many_files as MANY
    from whisperlive_amd import file_diarization as FD
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.rest import diarize_file_segments
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(H.TINY_EN, 5), spec=H.TINY_EN, hf_tokenizer=synthetic_tokenizer(H.TINY_EN.vocab), max_batch=8)
    try:
        f = MANY._files()
        audios = [f["A"], f["B"], f["C"]]
        clips = [{"start": 0, "end": 2 * BC.SR}, {"start": 3 * BC.SR, "end": 6 * BC.SR}]
        kw = dict(MANY.KW, chunk_length=3, vad_filter=False, batch_size=4, word_timestamps=True)
        caps = [2, 3, 2]
        pipe = BatchedInferencePipeline(hip)
        # threshold 0: the caps alone decide, so every file has as many speakers as its cap (five windows each)
        want = []
        for audio, cap in zip(audios, caps):
            segments, _info = pipe.transcribe(audio, clip_timestamps=[dict(c) for c in clips], **kw)
            segments = list(segments)
            resident = hip.resident_file_audio()
            assert resident is not None and len(segments) == 2
            want.append(diarize_file_segments(segments, FD.FileDiarizer(spk, 0.0, cap), lambda _ch: resident))
        calls = []
        real = spk.diarize_many
        spk.diarize_many = lambda *a, **k: (calls.append([len(w) for w in a[2]]), real(*a, **k))[1]
        try:
            out = pipe.transcribe_many(audios, clip_timestamps=[clips] * 3, diarize=FD.FileDiarizer(spk, 0.0), max_speakers=caps, wave_put=True, **kw)
        finally:
            del spk.diarize_many
        assert calls == [[5, 5, 5]]                                                      # one job for the wave: 15 windows, passes of four
        for (segments, info), (seg_speakers, word_speakers, speakers), cap in zip(out, want, caps):
            assert [s.speaker for s in segments] == seg_speakers and info.speakers == speakers and len(speakers) == cap
            assert [[w.speaker for w in s.words] for s in segments] == word_speakers and all(s.words for s in segments)
    finally:
        hip.close()
        hip.engine.close()
