"""CPU: offline file diarization (whisperlive_amd/file_diarization.py) — the clustering oracle `cluster_host` against an exhaustive
restatement written here, the window grid, turns, speaker assignment, known-name matching, and the endpoint's `diarize` form field over
a scripted transcriber and a scripted embedder."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_rest import FILE, ScriptedTranscriber, Served, _clean_model_cache, _verbose  # noqa: F401  (the fixture is autouse)
from whisperlive_amd import _lib
from whisperlive_amd import file_diarization as FD
from whisperlive_amd.types import Segment, Word


# ------------------------------------------------------------------------------------------------------------ clustering
def naive_cluster(dist, threshold, max_clusters=0):
    """The rules of wlx_spk_cluster with nothing clever: every round looks at every pair of live clusters (O(n^3) in all), keeps the
    smallest (distance, i, j), and updates the merged row element by element in float32."""
    D = np.array(dist, dtype=np.float32)
    n = D.shape[0]
    size = [np.float32(1)] * n
    alive = [True] * n
    parent = list(range(n))
    merges, heights = [], []
    while sum(alive) > 1:
        best = None
        for i in range(n):
            if alive[i]:
                for j in range(i + 1, n):
                    if alive[j] and (best is None or D[i, j] < best[0]):          # (i, j) rise: '<' keeps the first of a tie
                        best = (D[i, j], i, j)
        d, i, j = best
        if d > np.float32(threshold) and (max_clusters == 0 or sum(alive) <= max_clusters):
            break
        for k in range(n):
            if alive[k] and k != i and k != j:
                v = np.float32(np.float32(np.float32(size[i] * D[k, i]) + np.float32(size[j] * D[k, j])) / np.float32(size[i] + size[j]))
                D[k, i] = D[i, k] = v
        size[i] = np.float32(size[i] + size[j])
        alive[j] = False
        parent[j] = i
        merges.append((i, j))
        heights.append(d)
    roots = [k for k in range(n) if alive[k]]
    labels = []
    for k in range(n):
        while not alive[k]:
            k = parent[k]
        labels.append(roots.index(k))
    return np.array(labels, np.int32), np.array(merges, np.int32).reshape(-1, 2), np.array(heights, np.float32)


def unit_rows(n, dim=16, seed=0):
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def same(got, want):
    assert np.array_equal(got.labels, want[0]) and got.labels.dtype == np.int32
    assert np.array_equal(got.merges, want[1])
    assert np.array_equal(got.heights.view(np.uint32), want[2].view(np.uint32))          # bit for bit


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64])
def test_cluster_host_equals_the_exhaustive_search(n):
    X = unit_rows(n, seed=n)
    D = FD.cosine_distances(X)
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()
    for thr, cap in ((0.0, 0), (0.7, 0), (0.95, 0), (2.0, 0), (0.0, 3), (0.7, 2)):
        same(FD.cluster_host(X, thr, cap), naive_cluster(D, thr, cap))
        same(FD.cluster_host(None, thr, cap, dist=D), naive_cluster(D, thr, cap))
    got = FD.cluster_host(X, 0.95)
    K = int(got.labels.max()) + 1
    assert got.centroids.shape == (K, X.shape[1]) and np.allclose(np.linalg.norm(got.centroids, axis=1), 1.0, atol=1e-6)
    first = [int(np.nonzero(got.labels == c)[0][0]) for c in range(K)]
    assert first == sorted(first)                                                  # numbered by lowest member
    assert FD.cluster_host(None, 0.5, dist=D).centroids is None


def test_all_equal_distances_merge_in_index_order():
    n = 12
    D = np.full((n, n), 0.5, np.float32)                   # (0.5: every average of equal values is exact)
    np.fill_diagonal(D, 0.0)
    got = FD.cluster_host(None, 1.0, dist=D)
    assert got.merges.tolist() == [[0, k] for k in range(1, n)] and (got.heights == 0.5).all() and (got.labels == 0).all()
    same(got, naive_cluster(D, 1.0))
    none = FD.cluster_host(None, 0.25, dist=D)
    assert none.merges.shape == (0, 2) and none.labels.tolist() == list(range(n))


@pytest.mark.parametrize("n", [9, 40])
def test_many_ties_on_a_matrix_of_eighths(n):
    rng = np.random.default_rng(n)
    D = rng.integers(1, 9, size=(n, n)).astype(np.float32) / 8.0
    D = np.triu(D, 1) + np.triu(D, 1).T
    for thr, cap in ((0.25, 0), (0.5, 0), (1.0, 0), (0.0, 4)):
        same(FD.cluster_host(None, thr, cap, dist=D), naive_cluster(D, thr, cap))


def test_max_clusters_forces_merges_past_the_threshold():
    X = unit_rows(20, seed=5)
    D = FD.cosine_distances(X)
    free = FD.cluster_host(X, 0.0)
    assert free.labels.tolist() == list(range(20))                                 # nothing is closer than 0
    for cap in (1, 2, 5):
        got = FD.cluster_host(X, 0.0, cap)
        assert int(got.labels.max()) + 1 == cap and len(got.merges) == 20 - cap and (got.heights > 0).all()
        same(got, naive_cluster(D, 0.0, cap))
    assert int(FD.cluster_host(X, 2.0, 5).labels.max()) == 0                       # a cap never stops merges under the threshold


def test_partition_equals_scipy_average_linkage():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    X = unit_rows(48, seed=11)
    D = FD.cosine_distances(X)
    thr = 0.8
    Z = hierarchy.linkage(squareform(D.astype(np.float64), checks=False), method="average")
    assert np.abs(Z[:, 2] - thr).min() > 1e-4                                      # tie-free at the cut
    want = hierarchy.fcluster(Z, t=thr, criterion="distance")
    got = FD.cluster_host(X, thr).labels
    pairs = lambda lab: lab[:, None] == lab[None, :]
    assert np.array_equal(pairs(got), pairs(want))


# ------------------------------------------------------------------------------------------------------------ windows
def test_plan_windows():
    assert FD.plan_windows([(1.0, 1.29)]) == []                                     # under 0.3 s
    assert FD.plan_windows([(1.0, 1.3)]) == [(16000, 4800, 0)]
    assert FD.plan_windows([(2.0, 3.5)]) == [(32000, 24000, 0)]                     # exactly one window long
    assert FD.plan_windows([(0.0, 1.0)]) == [(0, 16000, 0)]                         # shorter: one window of the whole span
    assert FD.plan_windows([(0.0, 3.0)]) == [(0, 24000, 0), (12000, 24000, 0), (24000, 24000, 0)]          # the grid ends flush
    assert FD.plan_windows([(0.0, 3.2)]) == [(0, 24000, 0), (12000, 24000, 0), (24000, 24000, 0), (27200, 24000, 0)]   # one more, flush
    got = FD.plan_windows([(0.0, 0.1), (10.0, 11.0), (20.0, 22.0)], window_s=1.0, hop_s=0.5)
    assert got == [(160000, 16000, 1), (320000, 16000, 2), (328000, 16000, 2), (336000, 16000, 2)]
    with pytest.raises(ValueError):
        FD.plan_windows([(0, 1)], window_s=0.2)


def test_turns_from_labels():
    windows = FD.plan_windows([(0.0, 3.0), (10.0, 11.0)])
    assert len(windows) == 4
    # centres at 0.75, 1.5, 2.25 s: the cuts lie at 1.125 and 1.875 s; the second span is one window
    assert FD.turns_from_labels(windows, [0, 0, 1, 1]) == [(0.0, 1.875, 0), (1.875, 3.0, 1), (10.0, 11.0, 1)]
    assert FD.turns_from_labels(windows, [0, 1, 0, 2]) == [(0.0, 1.125, 0), (1.125, 1.875, 1), (1.875, 3.0, 0), (10.0, 11.0, 2)]
    # a window that took no part leaves its share to its neighbours
    assert FD.turns_from_labels(windows, [0, -1, 1, -1]) == [(0.0, 1.5, 0), (1.5, 3.0, 1)]
    assert FD.turns_from_labels([], []) == []


def _seg(start, end, words=None):
    return Segment(1, 0, start, end, " x", [1], -0.1, 1.0, 0.0, words, 0.0)


def test_assign_speakers():
    turns = [(0.0, 2.0, "A"), (2.0, 4.0, "B"), (6.0, 7.0, "A")]
    # without words: the longest overlap; a tie goes to the earlier turn; no overlap, no speaker
    segs = [_seg(0.5, 2.4), _seg(1.0, 3.0), _seg(4.5, 5.5), _seg(3.5, 6.9)]
    per_seg, per_word = FD.assign_speakers(segs, turns)
    assert per_seg == ["A", "A", None, "A"] and per_word == [None] * 4
    # with words: each word its own turn, the segment the speaker that covers most of the words' duration
    words = [Word(1.0, 1.5, " a", 0.9), Word(1.5, 2.5, " b", 0.9), Word(2.5, 3.75, " c", 0.9), Word(5.0, 5.5, " d", 0.9)]
    per_seg, per_word = FD.assign_speakers([_seg(1.0, 5.5, words)], turns)
    assert per_word == [["A", "A", "B", None]] and per_seg == ["A"]                # A: 0.5 + 1.0 s, B: 1.25 s
    words = [Word(1.5, 2.0, " a", 0.9), Word(2.0, 3.0, " b", 0.9)]
    assert FD.assign_speakers([_seg(1.5, 3.0, words)], turns)[0] == ["B"]
    assert FD.assign_speakers([_seg(0.0, 1.0)], []) == ([None], [None])
    assert FD.merge_spans([_seg(0.0, 1.0), _seg(1.0, 2.0), _seg(5.0, 6.0), _seg(5.5, 5.75), _seg(9.0, 9.0)]) == [(0.0, 2.0), (5.0, 6.0)]


def test_known_names():
    e = np.eye(4, dtype=np.float32)
    cent = np.stack([e[0], (e[1] + 0.2 * e[2]) / np.linalg.norm(e[1] + 0.2 * e[2]), e[3]]).astype(np.float32)
    assert FD.match_known(cent, {"ann": e[1], "bob": e[0] * 3.0}, 0.45) == {0: "bob", 1: "ann"}
    assert FD.match_known(cent, {"ann": e[2]}, 0.45) == {}                          # cosine 0.196 < 0.55
    # each name once: the better match takes it
    two = np.stack([(e[0] + 0.5 * e[1]) / np.linalg.norm(e[0] + 0.5 * e[1]), e[0]]).astype(np.float32)
    assert FD.match_known(two, {"ann": e[0]}, 0.45) == {1: "ann"}
    assert FD.match_known(two, None, 0.45) == {} and FD.match_known(None, {"ann": e[0]}, 0.45) == {}


class ScriptedEmbedder:
    """diarize_resident answers a script: the label of a window is the number of script boundaries at or before its centre"""

    def __init__(self, boundaries_s, centroids):
        self.boundaries, self.centroids, self.calls = boundaries_s, np.asarray(centroids, np.float32), []

    def diarize_resident(self, slot, item, windows, threshold, max_clusters=0):
        self.calls.append((slot, item, list(windows), threshold, max_clusters))
        raw = [sum((s + n / 2.0) / 16000.0 >= b for b in self.boundaries) if n >= 4800 else -1 for s, n in windows]
        order = []
        for r in raw:
            if r >= 0 and r not in order:
                order.append(r)
        return np.array([order.index(r) if r >= 0 else -1 for r in raw], np.int32), self.centroids[: len(order)]


def test_file_diarizer_labels_names_and_host_route():
    resident = SimpleNamespace(slot="slot", item=3, n_samples=10 * 16000)
    emb = ScriptedEmbedder([4.0], np.eye(2))
    d = FD.FileDiarizer(emb, max_speakers=4)
    turns = d.diarize(resident, [(0.0, 6.0), (8.0, 12.0)])
    assert emb.calls[0][:2] == ("slot", 3) and emb.calls[0][3:] == (0.45, 4)
    assert all(s + n <= resident.n_samples for s, n in emb.calls[0][2])            # the span past the file is cut to it
    assert [t[2] for t in turns] == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_01"] and turns[0][0] == 0.0 and turns[-1][1] == 10.0
    assert turns[0][1] == turns[1][0] and 3.5 < turns[0][1] < 4.5
    assert FD.speakers_in_order(turns) == ["SPEAKER_00", "SPEAKER_01"]
    named = d.diarize(resident, [(0.0, 6.0)], known={"ann": np.array([0.0, 2.0], np.float32)})
    assert [t[2] for t in named] == ["SPEAKER_00", "ann"]
    assert d.diarize(resident, [(1.0, 1.1)]) == []

    class OnlyEmbeds:                                           # no clustering entry point: cluster_host clusters the windows
        def embed_resident(self, slot, item, ranges):
            return [None if n < 4800 else np.array([1.0, 0.0] if s < 4 * 16000 else [0.0, 1.0], np.float32) for s, n in ranges]
    turns = FD.FileDiarizer(OnlyEmbeds()).diarize(resident, [(0.0, 8.0)])
    assert [t[2] for t in turns] == ["SPEAKER_00", "SPEAKER_01"]
    with pytest.raises(ValueError):
        FD.FileDiarizer(emb, distance_threshold=2.5)


# ------------------------------------------------------------------------------------------------------------ the endpoint
class ResidentTranscriber(ScriptedTranscriber):
    def resident_file_audio(self, channel=None):
        return SimpleNamespace(slot="slot", item=0 if channel is None else channel, n_samples=3728 * 16000)


def test_rest_diarize_field():
    emb = ScriptedEmbedder([100.0], np.eye(2))
    base = [FILE, ("response_format", "verbose_json"), ("language", "de"), ("timestamp_granularities", "word")]
    with Served(ResidentTranscriber(), embedder_factory=lambda path, device: emb) as s:
        # absent (or false): today's answer, byte for byte, and no embedder is asked for
        want = json.dumps(_verbose(True), ensure_ascii=False, separators=(",", ":")).encode("utf-8")
        assert s.post(base)[2] == want and s.post(base + [("diarize", "false")])[2] == want and not emb.calls
        st, _, body = s.post(base + [("diarize", "true"), ("max_speakers", "3")])
        assert st == 200
        got = json.loads(body)
        assert got["speakers"] == ["SPEAKER_00", "SPEAKER_01"] and emb.calls[-1][4] == 3
        assert [g["speaker"] for g in got["segments"]] == ["SPEAKER_00", "SPEAKER_01"]
        assert [[w["speaker"] for w in g["words"]] for g in got["segments"]] == [["SPEAKER_00", "SPEAKER_00"], ["SPEAKER_01"]]
        for g in got["segments"]:                               # nothing else changed
            g.pop("speaker")
            for w in g["words"]:
                w.pop("speaker")
        got.pop("speakers")
        assert got == _verbose(True)
        # without word times: segments only
        st, _, body = s.post(base[:3] + [("diarize", "1")])
        got = json.loads(body)
        assert st == 200 and [g["speaker"] for g in got["segments"]] == ["SPEAKER_00", "SPEAKER_01"] and "words" not in got["segments"][0]
        for bad in ([("diarize", "maybe")], [("diarize", "true"), ("max_speakers", "-1")], [("diarize", "true"), ("max_speakers", "x")]):
            assert s.post(base + bad)[0] == 400
    with Served(ResidentTranscriber(), diarization_model="/nonexistent/wespeaker.bin") as s:
        st, _, body = s.post(base + [("diarize", "true")])
        assert st == 400 and b"no speaker-embedding checkpoint" in body
    with Served(ScriptedTranscriber(), embedder_factory=lambda path, device: emb) as s:          # nothing resident to read
        st, _, body = s.post(base + [("diarize", "true")])
        assert st == 400 and b"resident" in body


def test_a_diarize_request_is_not_pooled():
    emb = ScriptedEmbedder([100.0], np.eye(2))

    class Pipeline:
        def __init__(self, t):
            self.t = t

        def transcribe(self, data, **kw):
            kw.pop("batch_size"), kw.pop("vad_filter")
            return self.t.transcribe(data, vad_filter=True, **kw)

        def iter_many(self, *a, **k):
            raise AssertionError("a diarize request went through the batcher")
    with Served(ResidentTranscriber(), embedder_factory=lambda path, device: emb, file_batch_size=2, file_batch_window_ms=5,
                model_factory=lambda model, device, max_batch=1: ResidentTranscriber(), pipeline_factory=Pipeline) as s:
        st, _, body = s.post([FILE, ("response_format", "verbose_json"), ("diarize", "true")])
        assert st == 200 and json.loads(body)["speakers"] == ["SPEAKER_00", "SPEAKER_01"] and s.server.batcher.jobs == 0


def test_exports_hold_the_new_symbols():
    for name in ("wlx_spk_cluster", "wlx_spk_diarize_pcm", "wlx_spk_debug_affinity", "wlx_spk_debug_ahc", "wlx_spk_debug_cluster_timings"):
        assert name in _lib.EXPORTS
    assert "spk_cluster.hip" in _lib.SOURCES and _lib.SPK_CLUSTER_MAX == 2048
