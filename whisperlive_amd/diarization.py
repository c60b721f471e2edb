"""Speaker labels for completed transcript segments — the `enable_diarization` option of the WhisperLive protocol (reference:
whisper_live/diarization.py, created per client in whisper_live/server.py:346-363 and called inline on the transcription thread from
base.py `_identify_speaker`).

* ``SpeakerEmbedderHIP`` — ctypes binding of the wlx_spk_* entry points: one WeSpeaker ResNet34 engine on one GPU. ``embed(pcm)``
                           returns the L2-normalised embedding, or None under 0.3 s; ``embed_many(pcms)`` the same for a list of
                           segments, packed by ``plan_embed_groups`` into as few wlx_spk_embed_batch passes as the engine's
                           buffers allow (a file's segments; the streaming server embeds one at a time).
                           ``embed_resident(slot, item, ranges)`` / ``embed_ring(ring, ranges)`` do the same on (start, n_samples)
                           ranges of audio that is ALREADY in HBM (a slot item's PCM, a session's PCM ring): nothing is uploaded
                           (wlx_spk_embed_pcm_batch / wlx_spk_embed_ring_batch). ``cluster(X, threshold)`` and
                           ``diarize_resident(slot, item, windows, threshold)`` cluster embeddings, or embed and cluster a whole
                           file's windows, on the device (wlx_spk_cluster / wlx_spk_diarize_pcm; file_diarization.py). ``shared_embedder``
                           keeps one per (checkpoint, device), loaded by the first client that asks for diarization.
* ``SpeakerDiarizer``    — the reference's online clustering, unchanged in behaviour: cosine similarity against the running
                           centroids, threshold 0.55, 0.9 / 0.1 running average with renormalisation, closest speaker at the cap,
                           ``speaker_names``, ``enroll_speaker``, ``reset``, labels ``SPEAKER_%02d``. ``embedder`` is any callable
                           (pcm float32, sample_rate) -> unit vector or None, so the clustering is testable without a GPU.
                           ``identify_speakers(audios)`` labels a list of segments: every embedding first (one ``embed_many``
                           call when the embedder has it), then the same clustering step in order, so the labels are those of
                           ``identify_speaker`` called once per segment. ``identify_speakers_resident(source, ranges)`` is
                           the same on ranges of device-resident audio (``ResidentPcm`` or a PCM ring).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .engine import ResidentPcm
from .spk_weights import SpkSpec

MIN_SECONDS = 0.3


def plan_embed_groups(lengths: Sequence[int], cap_samples: int, max_items: int = _lib.SPK_MAX_BATCH) -> List[List[int]]:
    """Indices of `lengths` (samples per segment) grouped greedily, in order, into batches of one wlx_spk_embed_batch call each:
    a group holds at most `max_items` segments and at most `cap_samples` samples in all. A segment longer than the cap is a group of
    its own (the caller cuts it to the cap, as `embed` does)."""
    if cap_samples < 1 or max_items < 1:
        raise ValueError("cap_samples and max_items must be positive")
    groups: List[List[int]] = []
    cur: List[int] = []
    total = 0
    for i, n in enumerate(lengths):
        n = int(n)
        if cur and (len(cur) >= max_items or total + n > cap_samples):
            groups.append(cur)
            cur, total = [], 0
        cur.append(i)
        total += n
    if cur:
        groups.append(cur)
    return groups


def plan_diarize_many(n_windows: Sequence[int], n_taking_part: Optional[Sequence[int]] = None, max_files: int = _lib.SPK_MANY_MAX_FILES,
                      max_rows: int = _lib.SPK_MANY_MAX_ROWS, max_cells: int = _lib.SPK_MANY_MAX_CELLS) -> List[List[int]]:
    """A list of files -> consecutive wlx_spk_diarize_many calls, as lists of file indices in order: a call is closed when the next
    file would take it over `max_files` files, over `max_rows` windows in all (n_windows, short ones counted) or over `max_cells`
    floats of distance matrices (the sum of m^2, m = n_taking_part: the windows of at least 0.3 s; n_windows where it is not given).
    A file of more than _lib.SPK_CLUSTER_MAX windows fits no call: ValueError."""
    m_of = list(n_windows) if n_taking_part is None else list(n_taking_part)
    if len(m_of) != len(n_windows):
        raise ValueError("n_taking_part must have one entry per file")
    calls: List[List[int]] = []
    cur: List[int] = []
    rows = cells = 0
    for f, (n, m) in enumerate(zip(n_windows, m_of)):
        n, m = int(n), int(m)
        if n < 0 or m < 0 or m > n or n > _lib.SPK_CLUSTER_MAX:
            raise ValueError(f"file {f}: {n} windows ({m} taking part) outside 0..{_lib.SPK_CLUSTER_MAX}")
        if cur and (len(cur) >= max_files or rows + n > max_rows or cells + m * m > max_cells):
            calls.append(cur)
            cur, rows, cells = [], 0, 0
        cur.append(f)
        rows, cells = rows + n, cells + m * m
    if cur:
        calls.append(cur)
    return calls


class SpeakerEmbedderHIP:
    """one wlx_spk engine: `weights` are the FOLDED tensors of spk_weights.fold()"""

    def __init__(self, spec: SpkSpec, weights: Dict[str, np.ndarray], device: int = 0):
        self.lib = _lib.load()
        self.spec = spec
        self.device = device
        cs = _lib.wlx_spk_spec(spec.n_mels, spec.planes, (C.c_int32 * 4)(*spec.blocks), spec.embed_dim, spec.max_seconds,
                               float(spec.pool_eps))
        arr, keep = _lib.tensor_array(weights)      # (keep: alive until the create call returns)
        h = C.c_void_p()
        _lib.check(self.lib.wlx_spk_create(C.byref(cs), arr, len(weights), device, C.byref(h)))
        del keep
        self.h = h

    @classmethod
    def from_checkpoint(cls, path: str, device: int = 0, **kw) -> "SpeakerEmbedderHIP":
        from .spk_weights import load
        spec, w = load(path, **kw)
        return cls(spec, w, device)

    def embed(self, pcm, sample_rate: int = 16000) -> Optional[np.ndarray]:
        if sample_rate != 16000:
            raise ValueError("the speaker engine takes 16 kHz audio")
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        cap = self.spec.max_seconds * 16000
        if len(pcm) > cap:              # (the session buffer holds 45 s; a longer enrolment clip is cut, not refused)
            pcm = pcm[:cap]
        out = np.zeros(self.spec.embed_dim, dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        rc = self.lib.wlx_spk_embed(self.h, pcm.ctypes.data_as(f32p), len(pcm), out.ctypes.data_as(f32p))
        if rc == _lib.ERR_TOO_SHORT:
            return None
        _lib.check(rc)
        return out

    __call__ = embed

    def embed_many(self, pcms, sample_rate: int = 16000) -> List[Optional[np.ndarray]]:
        """`embed` of every segment of `pcms`, None where one is under 0.3 s; each embedding has the bits `embed` gives for that
        segment alone. One wlx_spk_embed_batch call per group of plan_embed_groups."""
        if sample_rate != 16000:
            raise ValueError("the speaker engine takes 16 kHz audio")
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        cap = self.spec.max_seconds * 16000
        pcms = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1)[:cap] for p in pcms]
        result: List[Optional[np.ndarray]] = [None] * len(pcms)
        f32p = C.POINTER(C.c_float)
        for group in plan_embed_groups([len(p) for p in pcms], cap):
            packed = np.ascontiguousarray(np.concatenate([pcms[i] for i in group]))
            lengths = np.array([len(pcms[i]) for i in group], dtype=np.int64)
            out = np.zeros((len(group), self.spec.embed_dim), dtype=np.float32)
            status = np.zeros(len(group), dtype=np.int32)
            _lib.check(self.lib.wlx_spk_embed_batch(self.h, packed.ctypes.data_as(f32p), lengths.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    len(group), out.ctypes.data_as(f32p), status.ctypes.data_as(C.POINTER(C.c_int32))))
            for row, i in enumerate(group):
                if status[row] == _lib.ERR_TOO_SHORT:
                    continue
                _lib.check(int(status[row]))
                result[i] = out[row].copy()
        return result

    def _embed_ranges(self, ranges, call) -> List[Optional[np.ndarray]]:
        """(start, n_samples) ranges -> embeddings through `call(starts, counts, n, out, status)`, one call per group of
        plan_embed_groups; a range longer than the engine's max_seconds is cut to it, as `embed` cuts a segment"""
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        cap = self.spec.max_seconds * 16000
        ranges = [(int(a), min(int(n), cap)) for a, n in ranges]
        result: List[Optional[np.ndarray]] = [None] * len(ranges)
        f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        for group in plan_embed_groups([n for _, n in ranges], cap):
            starts = np.array([ranges[i][0] for i in group], dtype=np.int64)
            counts = np.array([ranges[i][1] for i in group], dtype=np.int64)
            out = np.zeros((len(group), self.spec.embed_dim), dtype=np.float32)
            status = np.zeros(len(group), dtype=np.int32)
            _lib.check(call(starts.ctypes.data_as(i64p), counts.ctypes.data_as(i64p), len(group), out.ctypes.data_as(f32p),
                            status.ctypes.data_as(C.POINTER(C.c_int32))))
            for row, i in enumerate(group):
                if status[row] == _lib.ERR_TOO_SHORT:
                    continue
                _lib.check(int(status[row]))
                result[i] = out[row].copy()
        return result

    def embed_resident(self, slot, item: int, ranges) -> List[Optional[np.ndarray]]:
        """`embed` of samples [start, start + n) of the PCM resident in `item` of `slot`, for every (start, n) of `ranges`; None where a
        range is under 0.3 s. No audio is uploaded; each embedding has the bits `embed` gives for those samples. Raises WlxError
        (ERR_STATE) when a range is not resident. The slot's lock is held for the calls: a slot serves one call at a time."""
        with slot.lock:
            return self._embed_ranges(ranges, lambda *a: self.lib.wlx_spk_embed_pcm_batch(self.h, slot.engine._h, slot.sid, int(item), *a))

    def embed_ring(self, ring, ranges) -> List[Optional[np.ndarray]]:
        """the same on ABSOLUTE stream positions of a device PCM ring (whisperlive_amd.engine.PcmRing); ERR_STATE when a range has been
        trimmed away or has not arrived"""
        return self._embed_ranges(ranges, lambda *a: self.lib.wlx_spk_embed_ring_batch(self.h, ring._h, *a))

    def cluster(self, X, threshold: float, max_clusters: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """wlx_spk_cluster: average-linkage clustering of the unit rows X [n][embed_dim] (n <= _lib.SPK_CLUSTER_MAX) at the cosine
        DISTANCE `threshold` on the device -> (labels int32 [n], numbered by first appearance; centroids float32 [K][embed_dim]).
        file_diarization.cluster_host states the rules."""
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("X must be [n][embed_dim]")
        n, dim = X.shape
        opts = _lib.wlx_spk_cluster_opts(float(threshold), int(max_clusters))
        labels, cent, k = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), dim), dtype=np.float32), C.c_int32()
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self.lib.wlx_spk_cluster(self.h, X.ctypes.data_as(f32p), n, dim, C.byref(opts), labels.ctypes.data_as(i32p),
                                            cent.ctypes.data_as(f32p), C.byref(k)))
        return labels[:n], cent[:k.value].copy()

    def diarize_resident(self, slot, item: int, windows, threshold: float, max_clusters: int = 0,
                         want_embeddings: bool = False, want_distances: bool = False):
        """wlx_spk_diarize_pcm: every (start, n_samples) window of the PCM resident in `item` of `slot` embedded and all of them
        clustered on the device behind one wait (up to _lib.SPK_CLUSTER_MAX windows, each within max_seconds) ->
        (labels int32 [n], -1 for a window under 0.3 s; centroids float32 [K][embed_dim]), and with want_embeddings / want_distances
        also the rows [n][embed_dim] and the distance matrix [m][m] over the windows that took part."""
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        windows = [(int(a), int(c)) for a, c in windows]
        n, dim = len(windows), self.spec.embed_dim
        starts = np.array([a for a, _ in windows], dtype=np.int64)
        counts = np.array([c for _, c in windows], dtype=np.int64)
        opts = _lib.wlx_spk_cluster_opts(float(threshold), int(max_clusters))
        labels, status = np.full(max(n, 1), -1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        cent, k = np.zeros((max(n, 1), dim), dtype=np.float32), C.c_int32()
        m = int((counts >= 4800).sum())
        emb = np.zeros((max(n, 1), dim), dtype=np.float32) if want_embeddings else None
        dist = np.zeros((m, m), dtype=np.float32) if want_distances and m else None
        f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        ptr = lambda a: a.ctypes.data_as(f32p) if a is not None else None
        with slot.lock:
            _lib.check(self.lib.wlx_spk_diarize_pcm(self.h, slot.engine._h, slot.sid, int(item), starts.ctypes.data_as(i64p),
                                                    counts.ctypes.data_as(i64p), n, C.byref(opts), labels.ctypes.data_as(i32p),
                                                    status.ctypes.data_as(i32p), ptr(emb), ptr(dist), ptr(cent), C.byref(k)))
        out = (labels[:n], cent[:k.value].copy())
        if want_embeddings:
            out += (emb[:n],)
        if want_distances:
            out += (dist,)
        return out

    def diarize_many(self, slot, items, windows_per_file, thresholds, max_clusters=0, want_embeddings: bool = False) -> list:
        """wlx_spk_diarize_many: `diarize_resident` of a wave of files — file f the (start, n_samples) windows `windows_per_file[f]` of
        the PCM resident in item `items[f]` of `slot` — with ONE wait per call: the windows of all files share the embed passes, and the
        files are clustered side by side in one launch. `thresholds` / `max_clusters`: one value, or one per file. -> per file
        (labels, centroids[, rows]) with the bits of `diarize_resident` on that file, or the WlxError of that file alone (ERR_STATE:
        nothing resident behind its item, a window past its end) — returned, not raised. More files than one call takes are cut into
        consecutive calls (`plan_diarize_many`); a file over _lib.SPK_CLUSTER_MAX windows is a ValueError."""
        if self.h is None:
            raise _lib.WlxError("speaker engine is closed")
        n_files, dim = len(items), self.spec.embed_dim
        per_file = lambda v: [v] * n_files if np.isscalar(v) else list(v)
        thresholds, max_clusters = per_file(thresholds), per_file(max_clusters)
        if not (len(windows_per_file) == len(thresholds) == len(max_clusters) == n_files):
            raise ValueError("diarize_many: items, windows_per_file, thresholds and max_clusters must have one entry per file")
        windows_per_file = [[(int(a), int(c)) for a, c in ws] for ws in windows_per_file]
        out: list = [None] * n_files
        f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        ptr = lambda a: a.ctypes.data_as(f32p) if a is not None else None
        for call in plan_diarize_many([len(ws) for ws in windows_per_file],
                                      [sum(c >= _lib.SPK_MIN_SAMPLES for _, c in ws) for ws in windows_per_file]):
            counts = np.array([len(windows_per_file[f]) for f in call], dtype=np.int32)
            total = max(int(counts.sum()), 1)
            flat = [w for f in call for w in windows_per_file[f]]
            starts = np.array([a for a, _ in flat] or [0], dtype=np.int64)
            samples = np.array([c for _, c in flat] or [0], dtype=np.int64)
            its = np.array([int(items[f]) for f in call], dtype=np.int32)
            opts = (_lib.wlx_spk_cluster_opts * len(call))(*[_lib.wlx_spk_cluster_opts(float(thresholds[f]), int(max_clusters[f])) for f in call])
            labels, status = np.full(total, -1, dtype=np.int32), np.zeros(total, dtype=np.int32)
            fstat, ks = np.zeros(len(call), dtype=np.int32), np.zeros(len(call), dtype=np.int32)
            cent = np.zeros((total, dim), dtype=np.float32)
            emb = np.zeros((total, dim), dtype=np.float32) if want_embeddings else None
            with slot.lock:
                _lib.check(self.lib.wlx_spk_diarize_many(self.h, slot.engine._h, slot.sid, len(call), its.ctypes.data_as(i32p),
                                                         counts.ctypes.data_as(i32p), starts.ctypes.data_as(i64p), samples.ctypes.data_as(i64p),
                                                         opts, labels.ctypes.data_as(i32p), status.ctypes.data_as(i32p),
                                                         fstat.ctypes.data_as(i32p), ks.ctypes.data_as(i32p), ptr(emb), ptr(cent)))
            at = 0
            for j, f in enumerate(call):
                n = int(counts[j])
                if fstat[j] != 0:
                    err = _lib.WlxError(f"libwlx error {int(fstat[j])}: wlx_spk_diarize_many: item {int(its[j])}: no PCM resident behind "
                                        f"a window of file {f}")
                    err.code = int(fstat[j])
                    out[f] = err
                else:
                    out[f] = (labels[at:at + n].copy(), cent[at:at + int(ks[j])].copy()) + ((emb[at:at + n].copy(),) if want_embeddings else ())
                at += n
        return out

    def cluster_timings(self) -> Tuple[float, float]:
        """device milliseconds of the last clustering: (distance matrix, agglomeration)"""
        a, b = C.c_float(), C.c_float()
        _lib.check(self.lib.wlx_spk_debug_cluster_timings(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timings(self) -> Tuple[float, float]:
        """device milliseconds of the last embed: (filterbank, network)"""
        a, b = C.c_float(), C.c_float()
        _lib.check(self.lib.wlx_spk_debug_timings(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.wlx_spk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_shared: Dict[Tuple[str, int], SpeakerEmbedderHIP] = {}
_shared_mu = threading.Lock()


def shared_embedder(checkpoint: str, device: int = 0) -> SpeakerEmbedderHIP:
    """one engine per (checkpoint, device), created by the first client that asks for diarization"""
    with _shared_mu:
        key = (checkpoint, device)
        if key not in _shared or _shared[key].h is None:
            _shared[key] = SpeakerEmbedderHIP.from_checkpoint(checkpoint, device)
        return _shared[key]


def close_shared():
    with _shared_mu:
        for e in _shared.values():
            e.close()
        _shared.clear()


class SpeakerDiarizer:
    """Online speaker clustering on unit-norm embeddings, behaving as the reference's class of the same name
    (whisper_live/diarization.py). `embedder`: a callable (pcm, sample_rate) -> embedding or None; None = the HIP engine of
    `embedding_model` on `device`, loaded on first use. `hf_token` is accepted for the reference's signature; the look-up of
    artifacts.resolve_diarization_model reads the hub's own environment."""

    def __init__(self, similarity_threshold=0.55, max_speakers=10, embedding_model="pyannote/wespeaker-voxceleb-resnet34-LM",
                 hf_token=None, speaker_names=None, embedder: Optional[Callable] = None, device: int = 0):
        self.similarity_threshold = similarity_threshold
        self.max_speakers = max_speakers
        self.speaker_names = [] if not speaker_names else list(speaker_names)
        self.speakers = {}          # label -> running centroid (unit norm), in order of first appearance
        self._created = 0           # speakers made by identify_speaker since the last reset (enrolments do not count)
        self._embed = embedder
        self._checkpoint_name = embedding_model
        self._device = device

    def _auto_label(self) -> str:
        return "SPEAKER_%02d" % self._created

    def _ensure_embedder(self):
        if self._embed is None:
            from .artifacts import resolve_diarization_model
            path = resolve_diarization_model(self._checkpoint_name)
            if path is None:
                raise FileNotFoundError(f"no speaker-embedding checkpoint found for '{self._checkpoint_name}'")
            self._embed = shared_embedder(path, self._device)

    def _compute_embedding(self, audio_np, sample_rate=16000):
        """unit-norm embedding of the audio, None under MIN_SECONDS"""
        self._ensure_embedder()
        if len(audio_np) < sample_rate * MIN_SECONDS:
            return None
        emb = self._embed(audio_np, sample_rate)
        if emb is None:
            return None
        emb = np.asarray(emb)
        return emb / np.linalg.norm(emb)

    def _closest(self, emb):
        """(label, similarity) of the centroid nearest to `emb`: the first one in insertion order on a tie, (None, -1.0)
        when there is none (or none above -1)"""
        ids = list(self.speakers)
        if not ids:
            return None, -1.0
        sims = [float(np.dot(emb, self.speakers[i])) for i in ids]       # cosine: both sides are unit vectors
        k = int(np.argmax(sims))            # first maximum, as a strict '>' scan finds it
        return (ids[k], sims[k]) if sims[k] > -1.0 else (None, -1.0)

    def identify_speaker(self, audio_np, sample_rate=16000):
        """the label of the segment's speaker, or None when the audio is too short to embed"""
        return self._assign(self._compute_embedding(audio_np, sample_rate))

    def identify_speakers(self, audios, sample_rate=16000) -> List[Optional[str]]:
        """`identify_speaker` of every segment of `audios`, in order, with all embeddings computed first: through the embedder's
        `embed_many` (one call for all segments of at least MIN_SECONDS) when it has one, else one call per segment"""
        self._ensure_embedder()
        audios = list(audios)
        many = getattr(self._embed, "embed_many", None)
        if many is None:
            embs = [self._compute_embedding(a, sample_rate) for a in audios]
        else:
            asked = [i for i, a in enumerate(audios) if len(a) >= sample_rate * MIN_SECONDS]
            embs = [None] * len(audios)
            for i, emb in zip(asked, many([audios[i] for i in asked], sample_rate) if asked else []):
                if emb is not None:
                    emb = np.asarray(emb)
                    embs[i] = emb / np.linalg.norm(emb)
        return [self._assign(emb) for emb in embs]

    def supports_resident(self, source) -> bool:
        """True when `identify_speakers_resident` can serve `source` (a ResidentPcm, or a PCM ring): the embedder has the entry
        point. An embedder that is not loaded yet is loaded to find out, as `identify_speakers` would."""
        if source is None:
            return False
        self._ensure_embedder()
        return hasattr(self._embed, "embed_resident" if isinstance(source, ResidentPcm) else "embed_ring")

    def identify_speakers_resident(self, source, ranges) -> List[Optional[str]]:
        """`identify_speakers` on (start, n_samples) ranges of 16 kHz audio that is resident on the device: `source` is a ResidentPcm
        (a slot item) or a PCM ring (absolute stream positions). Every embedding first, without an upload; then the same clustering
        step in order, so the labels equal `identify_speakers` on the same samples. An error of the embedder (a range that is not
        resident) is raised before any speaker is touched."""
        self._ensure_embedder()
        ranges = [(int(a), int(n)) for a, n in ranges]
        if isinstance(source, ResidentPcm):
            embs = self._embed.embed_resident(source.slot, source.item, ranges)
        else:
            embs = self._embed.embed_ring(source, ranges)
        units = []
        for (_, n), emb in zip(ranges, embs):
            if emb is None or n < 16000 * MIN_SECONDS:
                units.append(None)
            else:
                emb = np.asarray(emb)
                units.append(emb / np.linalg.norm(emb))
        return [self._assign(emb) for emb in units]

    def _assign(self, emb):
        """the clustering step: the label for a unit-norm embedding (None stays None), the centroids updated"""
        if emb is None:
            return None
        who, sim = self._closest(emb)
        if sim >= self.similarity_threshold:
            # matched: the centroid moves a tenth of the way and goes back onto the unit sphere
            c = self.speakers[who] * 0.9 + emb * 0.1
            self.speakers[who] = c / np.linalg.norm(c)
            return who
        if len(self.speakers) >= self.max_speakers:
            # at the cap nobody new is created: the nearest speaker takes the segment, its centroid unchanged
            return who or self._auto_label()
        # a new speaker: the next of `speaker_names` while they last, then the numbered label
        who = self.speaker_names[self._created] if self._created < len(self.speaker_names) else self._auto_label()
        self._created += 1
        self.speakers[who] = emb
        return who

    def enroll_speaker(self, speaker_name, audio_np, sample_rate=16000):
        """store the audio's embedding as `speaker_name`'s centroid; False when the audio is too short"""
        emb = self._compute_embedding(audio_np, sample_rate)
        if emb is not None:
            self.speakers[speaker_name] = emb
        return emb is not None

    def reset(self):
        """forget every speaker, enrolled ones included; numbering starts again at 0"""
        self.speakers = {}
        self._created = 0
