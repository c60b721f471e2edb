"""Offline diarization of a whole file: a sliding grid of windows over the speech spans, one embedding per window, all windows
clustered at once (average linkage on cosine distances), turns cut at the midpoints between window centres, and every word (or
segment) given the turn it overlaps longest. The live sessions keep the reference's online rule (diarization.SpeakerDiarizer); this is
the route of the file endpoint's ``diarize=true``.

* ``cluster_host``       — the NumPy float32 restatement of the clustering rules of include/wlx.h (wlx_spk_cluster): the oracle of the
                           GPU tests (which ask for equality of merges, heights and labels), and the route of an embedder without the
                           entry points or of more than ``_lib.SPK_CLUSTER_MAX`` windows.
* ``plan_windows``       — the window grid over the spans, in samples at 16 kHz.
* ``turns_from_labels``  — windows + labels -> (start_s, end_s, cluster) turns.
* ``assign_speakers``    — turns -> a speaker per word and per segment.
* ``match_known``        — clusters renamed after enrolled speakers.
* ``FileDiarizer``       — the above on the audio a transcription left resident on the device
                           (``SpeakerEmbedderHIP.diarize_resident``: wlx_spk_diarize_pcm, every window embedded and clustered behind ONE wait);
                           ``diarize_many`` does a wave of files in one device call (``SpeakerEmbedderHIP.diarize_many``:
                           wlx_spk_diarize_many), the turns per file those of ``diarize``.
* ``label_segments``     — ``assign_speakers`` with the gaps closed: what the file routes put on segments and words.
"""
from __future__ import annotations

import logging
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib

SAMPLE_RATE = 16000
MIN_WINDOW_S = 0.3            # what the speaker engine refuses to embed (WLX_ERR_TOO_SHORT under 4800 samples)


class Clustering(NamedTuple):
    labels: np.ndarray        # int32 [n]: clusters numbered 0..K-1 by their lowest member
    merges: np.ndarray        # int32 [n_merges][2]: (i, j), i < j, j merged into i
    heights: np.ndarray       # float32 [n_merges]: the distance of each merge
    centroids: Optional[np.ndarray]   # float32 [K][D]: the normalised mean of each cluster's rows (None without X)


def cosine_distances(X) -> np.ndarray:
    """float32 [n][n] = 1 - X X^T of unit rows, the diagonal set to 0 (the matrix spk_affinity_kernel computes, up to summation order)"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    D = (np.float32(1.0) - X @ X.T).astype(np.float32)
    D = np.minimum(D, D.T)                   # (BLAS does not promise a symmetric product)
    np.fill_diagonal(D, 0.0)
    return D


def cluster_host(X, threshold: float, max_clusters: int = 0, dist=None) -> Clustering:
    """Average-linkage agglomerative clustering by the rules of wlx_spk_cluster, in float32. `X`: unit rows [n][D] (may be None with
    `dist`); `dist`: cluster this symmetric matrix instead of `cosine_distances(X)` (it is not modified).
    Clusters are named by their lowest member. Each round takes the pair (i, j), i < j, of live clusters with the smallest
    (distance, i, j); stops when that distance is > threshold and (max_clusters == 0 or live <= max_clusters), or at one cluster;
    merges j into i with d(k, i) = (n_i d(k, i) + n_j d(k, j)) / (n_i + n_j), every operation rounded to float32."""
    D = np.array(cosine_distances(X) if dist is None else dist, dtype=np.float32)
    n = D.shape[0]
    if D.shape != (n, n) or n < 1:
        raise ValueError("dist must be a square matrix of at least one row")
    threshold = np.float32(threshold)
    size = np.ones(n, dtype=np.float32)
    alive = np.ones(n, dtype=bool)
    parent = np.arange(n)
    # The pairs of live clusters, i < j, in the upper triangle (inf elsewhere), and per row its nearest neighbour ABOVE it: the smallest
    # (distance, j) over j > i — np.argmin returns the first minimum. The best pair with i as its lower member is (nnd[i], i, nn[i]), so
    # the first minimum of nnd is the smallest (distance, i, j). A row is searched again only when its cached neighbour was merged
    # (tests/test_file_diarization_host.py holds this against the exhaustive search of every round).
    inf = np.float32(np.inf)
    upper = np.where(np.triu(np.ones((n, n), dtype=bool), 1), D, inf)
    nn = upper.argmin(axis=1)
    nnd = upper[np.arange(n), nn]
    merges, heights = [], []
    live = n
    while live > 1:
        i = int(nnd.argmin())
        j, d = int(nn[i]), nnd[i]
        if not np.isfinite(d):
            break
        if d > threshold and (max_clusters == 0 or live <= max_clusters):
            break
        ni, nj = size[i], size[j]
        new = (ni * D[i] + nj * D[j]) / (ni + nj)      # float32 scalars and rows: three roundings per element, as the kernel's
        others = alive.copy()
        others[i] = others[j] = False
        D[i, others] = new[others]
        D[others, i] = new[others]
        size[i] = ni + nj
        alive[j] = False
        parent[j] = i
        upper[j, :] = np.inf
        upper[:, j] = np.inf
        ks = np.nonzero(others)[0]
        lo, hi = ks[ks < i], ks[ks > i]
        upper[lo, i] = new[lo]
        upper[i, hi] = new[hi]
        nnd[j] = inf
        stale = np.nonzero(alive & ((nn == i) | (nn == j)))[0]          # (row i among them: nn[i] was j)
        better = lo[(new[lo] < nnd[lo]) | ((new[lo] == nnd[lo]) & (i < nn[lo]))]
        nn[better], nnd[better] = i, new[better]
        again = upper[stale].argmin(axis=1)
        nn[stale], nnd[stale] = again, upper[stale, again]
        merges.append((i, j))
        heights.append(d)
        live -= 1
    roots = np.nonzero(alive)[0]
    rank = np.full(n, -1, dtype=np.int32)
    rank[roots] = np.arange(len(roots), dtype=np.int32)
    labels = np.empty(n, dtype=np.int32)
    for k in range(n):                                 # parent[k] < k: the root of every lower row is known
        labels[k] = rank[k] if alive[k] else labels[parent[k]]
    centroids = None
    if X is not None:
        X = np.ascontiguousarray(X, dtype=np.float32)
        centroids = np.zeros((len(roots), X.shape[1]), dtype=np.float32)
        for c in range(len(roots)):
            s = X[labels == c].astype(np.float64).sum(axis=0)
            norm = np.linalg.norm(s)
            centroids[c] = (s / norm if norm > 0 else s).astype(np.float32)
    return Clustering(labels, np.array(merges, dtype=np.int32).reshape(-1, 2), np.array(heights, dtype=np.float32), centroids)


# ------------------------------------------------------------------------------------------------------------ windows and turns
def plan_windows(spans: Sequence[Tuple[float, float]], window_s: float = 1.5, hop_s: float = 0.75,
                 sample_rate: int = SAMPLE_RATE) -> List[Tuple[int, int, int]]:
    """(start, n_samples, span_index) triples in samples for the spans [start_s, end_s]: a span under 0.3 s has no window; one no
    longer than the window is one window of the whole span; otherwise windows start at 0, hop, 2 hop, ... while they fit, plus a last
    one flush with the span's end when the grid does not end there."""
    if window_s < MIN_WINDOW_S or hop_s <= 0:
        raise ValueError("window_s must be at least 0.3 s and hop_s positive")
    W, H, short = int(round(window_s * sample_rate)), max(1, int(round(hop_s * sample_rate))), int(round(MIN_WINDOW_S * sample_rate))
    out: List[Tuple[int, int, int]] = []
    for index, (a, b) in enumerate(spans):
        s0, s1 = max(0, int(round(a * sample_rate))), int(round(b * sample_rate))
        n = s1 - s0
        if n < short:
            continue
        if n <= W:
            out.append((s0, n, index))
            continue
        at = 0
        while at + W <= n:
            out.append((s0 + at, W, index))
            at += H
        if at - H + W != n:
            out.append((s1 - W, W, index))
    return out


def turns_from_labels(windows: Sequence[Tuple[int, int, int]], labels: Sequence[int],
                      sample_rate: int = SAMPLE_RATE) -> List[Tuple[float, float, int]]:
    """Windows of `plan_windows` (in order) and a label each (negative: the window took no part) -> turns (start_s, end_s, label). A
    window owns the part of its span from the midpoint between its centre and the previous window's to the midpoint towards the next
    one's; the first and the last labelled window of a span own it to the span's ends. Neighbouring pieces with one label fuse."""
    by_span: Dict[int, List[Tuple[int, int, int]]] = {}
    for (start, n, span), lab in zip(windows, labels):
        if int(lab) >= 0:
            by_span.setdefault(span, []).append((start, n, int(lab)))
    turns: List[List] = []
    for span in sorted(by_span, key=lambda s: by_span[s][0][0]):
        ws = by_span[span]
        lo = min(s for s, _, _ in ws)
        hi = max(s + n for s, n, _ in ws)
        centres = [s + n / 2.0 for s, n, _ in ws]
        for k, (_, _, lab) in enumerate(ws):
            a = lo if k == 0 else (centres[k - 1] + centres[k]) / 2.0
            b = hi if k == len(ws) - 1 else (centres[k] + centres[k + 1]) / 2.0
            a, b = a / sample_rate, b / sample_rate
            if turns and turns[-1][2] == lab and turns[-1][3] == span and turns[-1][1] == a:
                turns[-1][1] = b
            else:
                turns.append([a, b, lab, span])
    return [(a, b, lab) for a, b, lab, _ in turns]


def _best_turn(start: float, end: float, turns) -> Optional[object]:
    """the speaker of the turn [start, end] overlaps longest; the earlier turn on a tie; None without overlap"""
    best, best_overlap = None, 0.0
    for a, b, who in turns:
        overlap = min(end, b) - max(start, a)
        if overlap > best_overlap:
            best, best_overlap = who, overlap
    return best


def assign_speakers(segments, turns) -> Tuple[List[Optional[object]], List[Optional[List[Optional[object]]]]]:
    """-> (speaker per segment, per segment the speaker of each word or None when it has no words). A word, or a segment without
    words, takes the turn it overlaps longest (the earlier one on a tie, None without overlap); a segment with words takes the
    speaker that covers most of its words' duration (the first such speaker in word order on a tie)."""
    turns = sorted(turns, key=lambda t: (t[0], t[1]))
    seg_speakers, word_speakers = [], []
    for seg in segments:
        words = getattr(seg, "words", None)
        if not words:
            seg_speakers.append(_best_turn(seg.start, seg.end, turns))
            word_speakers.append(None)
            continue
        per_word = [_best_turn(w.start, w.end, turns) for w in words]
        cover: Dict[object, float] = {}
        for w, who in zip(words, per_word):
            if who is not None:
                cover[who] = cover.get(who, 0.0) + max(0.0, w.end - w.start)
        best, best_cover = None, -1.0
        for who, c in cover.items():                   # (dicts keep insertion order: word order)
            if c > best_cover:
                best, best_cover = who, c
        seg_speakers.append(best)
        word_speakers.append(per_word)
    return seg_speakers, word_speakers


def label_segments(segments, turns) -> Tuple[List[Optional[object]], List[Optional[List[Optional[object]]]]]:
    """`assign_speakers` with the gaps closed, as the file routes answer: a segment that overlaps no turn takes the speaker of the turn
    nearest in time, a word that overlaps none its segment's speaker. Without turns everything stays None."""
    per_seg, per_word = assign_speakers(segments, turns)
    seg_speakers: List[Optional[object]] = []
    word_speakers: List[Optional[List[Optional[object]]]] = []
    for seg, who, words in zip(segments, per_seg, per_word):
        if who is None and turns:
            who = min(turns, key=lambda t: max(t[0] - seg.end, seg.start - t[1], 0.0))[2]
        seg_speakers.append(who)
        word_speakers.append(None if words is None else [w if w is not None else who for w in words])
    return seg_speakers, word_speakers


def match_known(centroids, known: Optional[Dict[str, np.ndarray]], distance_threshold: float) -> Dict[int, str]:
    """{cluster: name} for clusters whose centroid has cosine >= 1 - distance_threshold with an enrolled unit embedding: pairs are
    taken best cosine first, each name and each cluster once (ties: the lower cluster, then the earlier name)."""
    if not known or centroids is None or len(centroids) == 0:
        return {}
    names = list(known)
    K = np.stack([np.asarray(known[name], dtype=np.float64) / max(np.linalg.norm(known[name]), 1e-30) for name in names])
    sims = np.asarray(centroids, dtype=np.float64) @ K.T
    pairs = sorted(((-sims[c, k], c, k) for c in range(sims.shape[0]) for k in range(len(names))))
    out: Dict[int, str] = {}
    used = set()
    for neg, c, k in pairs:
        if -neg < 1.0 - distance_threshold:
            break
        if c in out or k in used:
            continue
        out[c] = names[k]
        used.add(k)
    return out


def merge_spans(segments, gap_s: float = 0.0) -> List[Tuple[float, float]]:
    """the [start, end] of the segments, sorted, with overlapping or touching ones (or closer than gap_s) fused"""
    spans: List[List[float]] = []
    for a, b in sorted((float(s.start), float(s.end)) for s in segments):
        if b <= a:
            continue
        if spans and a <= spans[-1][1] + gap_s:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    return [(a, b) for a, b in spans]


class FileDiarizer:
    """Offline diarization on device-resident audio. `embedder`: SpeakerEmbedderHIP, or anything with
    `diarize_resident(slot, item, windows, threshold, max_clusters)` -> (labels, centroids), or only `embed_resident` (the windows are
    then clustered by `cluster_host`). distance_threshold 0.45 is SpeakerDiarizer's similarity_threshold 0.55 stated as a distance;
    it is UNPINNED (no real checkpoint has been available to tune it on). max_speakers 0 = no cap."""

    def __init__(self, embedder, distance_threshold: float = 0.45, max_speakers: int = 0, window_s: float = 1.5, hop_s: float = 0.75):
        if not 0.0 <= distance_threshold <= 2.0:
            raise ValueError("distance_threshold is a cosine distance in [0, 2]")
        if max_speakers < 0:
            raise ValueError("max_speakers must be 0 (no cap) or positive")
        self.embedder, self.distance_threshold, self.max_speakers = embedder, float(distance_threshold), int(max_speakers)
        self.window_s, self.hop_s = float(window_s), float(hop_s)
        self.many_on_device = True          # diarize_many: the wave in one device call where the embedder has one (False: the per-file loop)

    def cluster_windows(self, resident, windows) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """-> (label per window, -1 where it took no part; centroids [K][D])"""
        ranges = [(s, n) for s, n, _ in windows]
        on_device = getattr(self.embedder, "diarize_resident", None)
        if on_device is not None and len(ranges) <= _lib.SPK_CLUSTER_MAX:
            return on_device(resident.slot, resident.item, ranges, self.distance_threshold, self.max_speakers)
        if on_device is not None:
            logging.warning(f"file diarization: {len(ranges)} windows exceed the device's {_lib.SPK_CLUSTER_MAX}; clustering on the host")
        embs = self.embedder.embed_resident(resident.slot, resident.item, ranges)
        took = [i for i, e in enumerate(embs) if e is not None]
        labels = np.full(len(ranges), -1, dtype=np.int32)
        if not took:
            return labels, None
        X = np.stack([np.asarray(embs[i], dtype=np.float32) for i in took])
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
        got = cluster_host(X, self.distance_threshold, self.max_speakers)
        labels[took] = got.labels
        return labels, got.centroids

    def windows_of(self, resident, spans) -> List[Tuple[int, int, int]]:
        """the window grid of `diarize` over the spans, cut to the resident audio"""
        limit = resident.n_samples / float(SAMPLE_RATE)
        spans = [(max(0.0, a), min(limit, b)) for a, b in spans if min(limit, b) > max(0.0, a)]
        windows = plan_windows(spans, self.window_s, self.hop_s)
        return [(s, min(n, resident.n_samples - s), i) for s, n, i in windows if s < resident.n_samples]

    def _turns(self, windows, labels, centroids, known) -> List[Tuple[float, float, str]]:
        names = match_known(centroids, known, self.distance_threshold)
        return [(a, b, names.get(lab, "SPEAKER_%02d" % lab)) for a, b, lab in turns_from_labels(windows, labels)]

    def diarize(self, resident, spans, known: Optional[Dict[str, np.ndarray]] = None) -> List[Tuple[float, float, str]]:
        """turns (start_s, end_s, speaker) over the merged [start, end] spans of the ASR segments, on `resident` (engine.ResidentPcm):
        speakers are SPEAKER_00, SPEAKER_01, ... in order of first appearance, or the name of `known` a cluster matches"""
        windows = self.windows_of(resident, spans)
        if not windows:
            return []
        labels, centroids = self.cluster_windows(resident, windows)
        return self._turns(windows, labels, centroids, known)

    def diarize_many(self, residents, spans_per_file, known: Optional[Dict[str, np.ndarray]] = None,
                     max_speakers: Optional[Sequence[int]] = None) -> List[List[Tuple[float, float, str]]]:
        """`diarize` of a wave of files, `residents[f]` (engine.ResidentPcm, different items of ONE slot) with the spans
        `spans_per_file[f]` -> the turns per file, those `diarize` gives for that file. With `diarize_many` on the embedder the windows
        of all files go to the device together (SpeakerEmbedderHIP.diarize_many: wlx_spk_diarize_many, one wait per call); a file with
        more than _lib.SPK_CLUSTER_MAX windows keeps the host route of `cluster_windows`, and an embedder without `diarize_many` gets
        the loop over `diarize`. max_speakers: a cap per file in place of the diarizer's own. A file whose audio is not resident
        raises the error `diarize` raises for it."""
        if len(residents) != len(spans_per_file) or (max_speakers is not None and len(max_speakers) != len(residents)):
            raise ValueError("diarize_many: one resident, one list of spans and one max_speakers per file")
        caps = [self.max_speakers if c is None else int(c) for c in (max_speakers if max_speakers is not None else [None] * len(residents))]
        if any(c < 0 for c in caps):
            raise ValueError("max_speakers must be 0 (no cap) or positive")
        windows = [self.windows_of(r, spans) for r, spans in zip(residents, spans_per_file)]
        turns: List[List[Tuple[float, float, str]]] = [[] for _ in residents]
        on_device = getattr(self.embedder, "diarize_many", None) if self.many_on_device else None
        together = [f for f, ws in enumerate(windows) if ws and on_device is not None and len(ws) <= _lib.SPK_CLUSTER_MAX
                    and residents[f].slot is residents[0].slot]
        for f, ws in enumerate(windows):          # the per-file route: no many-call, too many windows, another slot
            if ws and f not in together:
                one = self if caps[f] == self.max_speakers else FileDiarizer(self.embedder, self.distance_threshold, caps[f], self.window_s, self.hop_s)
                labels, centroids = one.cluster_windows(residents[f], ws)
                turns[f] = self._turns(ws, labels, centroids, known)
        if together:
            got = on_device(residents[together[0]].slot, [residents[f].item for f in together], [[(s, n) for s, n, _ in windows[f]] for f in together],
                            self.distance_threshold, [caps[f] for f in together])
            for f, result in zip(together, got):
                if isinstance(result, Exception):
                    raise result
                turns[f] = self._turns(windows[f], result[0], result[1], known)
        return turns


def speakers_in_order(turns) -> List[str]:
    """the speakers of the turns, each once, in order of first appearance"""
    seen: List[str] = []
    for _, _, who in turns:
        if who not in seen:
            seen.append(who)
    return seen
