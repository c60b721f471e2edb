"""OpenAI-style file transcription endpoint: ``POST /v1/audio/transcriptions`` (multipart form -> text / json / verbose_json /
srt / vtt, or server-sent events with ``stream=true``).

A restatement of the reference's handler (whisper_live/server.py:490-598, 692-867) on the standard library — ``http.server`` and a
multipart parser of its own, as ws.py does for WebSockets — with two deliberate differences:

  * the reference builds a new ``WhisperModel`` per request; here every request runs on the GPU's SHARED transcriber, the one the
    ``single_model`` WebSocket sessions use (``ServeClientHIP.MODELS``: a process that runs both servers holds one copy of the
    weights), on a slot of the transcriber's pool that is handed back when the request ends. Requests rotate over ``devices`` as
    connections do (sharding.assign_gpu);
  * the uploaded file is not written to a temporary file: ``transcribe`` takes the bytes, decodes WAV / FLAC
    (whisperlive_amd/audio_io.py) and hands the frames to the device front end (``Slot.put_frames``).

The middleware order is the reference's (Starlette runs the last one added first): rate limit, then the API key, then CORS, then
routing — so a 429 or a 401 carries no CORS headers, and every request counts against the limit, whatever it asks for.

``TranscriptionServer.run(enable_rest=True)`` still raises NotImplementedError: this module is the endpoint, started on its own
(``RestServer(...).start()`` or ``python -m whisperlive_amd.rest``); wiring the flag to it is a separate change.
"""
from __future__ import annotations

import collections
import contextlib
import json
import logging
import re
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from . import metrics as wl_metrics
from ._lib import WlxError as _WlxError
from .sharding import assign_gpu

SUPPORTED_FORMATS = ["json", "text", "srt", "verbose_json", "vtt"]
ROUTE = "/v1/audio/transcriptions"
_CORS_METHODS = "DELETE, GET, HEAD, OPTIONS, PATCH, POST, PUT"


# ------------------------------------------------------------------------------------------------------------ multipart
class Part:
    __slots__ = ("name", "filename", "content_type", "data")

    def __init__(self, name: str, filename: Optional[str], content_type: Optional[str], data: bytes):
        self.name, self.filename, self.content_type, self.data = name, filename, content_type, data

    @property
    def text(self) -> str:
        return self.data.decode("utf-8", "replace")


def _boundary_of(content_type: str) -> bytes:
    if not content_type or not content_type.lower().lstrip().startswith("multipart/form-data"):
        raise ValueError("Content-Type must be multipart/form-data")
    m = re.search(r';\s*boundary=(?:"([^"]+)"|([^;\s]+))', content_type, re.I)
    if not m:
        raise ValueError("multipart/form-data without a boundary")
    b = (m.group(1) or m.group(2)).encode("latin-1")
    if not 1 <= len(b) <= 70:
        raise ValueError("multipart boundary must be 1..70 characters")
    return b


def _delimiter_end(body: bytes, pos: int) -> Optional[Tuple[int, bool]]:
    """`pos` is just behind '--boundary'. A real delimiter line goes on with '--' (the last one) or optional blanks and CRLF;
    -> (position behind the line, last?) or None when these bytes only look like a boundary (file content)."""
    if body[pos:pos + 2] == b"--":
        return pos + 2, True
    q = pos
    while q < len(body) and body[q:q + 1] in (b" ", b"\t"):
        q += 1
    if body[q:q + 2] == b"\r\n":
        return q + 2, False
    return None


def parse_multipart(body: bytes, content_type: str) -> List[Part]:
    """multipart/form-data -> parts in order (repeated names kept). Raises ValueError for anything malformed."""
    delim = b"--" + _boundary_of(content_type)
    if body.startswith(delim):
        start = 0
    else:
        start = body.find(b"\r\n" + delim)
        if start < 0:
            raise ValueError("multipart body without its boundary")
        start += 2
    end = _delimiter_end(body, start + len(delim))
    if end is None:
        raise ValueError("malformed multipart boundary line")
    pos, last = end
    parts: List[Part] = []
    while not last:
        head_end = body.find(b"\r\n\r\n", pos)
        if head_end < 0:
            raise ValueError("multipart part without a header block")
        headers: Dict[str, str] = {}
        for line in body[pos:head_end].split(b"\r\n"):
            if not line:
                continue
            k, sep, v = line.decode("utf-8", "replace").partition(":")
            if not sep:
                raise ValueError("malformed multipart part header")
            headers[k.strip().lower()] = v.strip()
        disp = headers.get("content-disposition", "")
        if not disp.lower().startswith("form-data"):
            raise ValueError("multipart part without a form-data Content-Disposition")
        params = {m.group(1).lower(): (m.group(2) if m.group(2) is not None else m.group(3))
                  for m in re.finditer(r';\s*([A-Za-z*]+)=(?:"((?:[^"\\]|\\.)*)"|([^;\s]*))', disp)}
        if "name" not in params:
            raise ValueError("multipart part without a name")
        data_start = head_end + 4
        search = data_start - 2                    # (an empty part: the CRLF of the blank line is the delimiter's)
        while True:
            i = body.find(b"\r\n" + delim, search)
            if i < 0:
                raise ValueError("multipart part without a closing boundary")
            end = _delimiter_end(body, i + 2 + len(delim))
            if end is not None:
                break
            search = i + 2                         # boundary-like bytes inside the content
        parts.append(Part(params["name"], params.get("filename"), headers.get("content-type"), body[data_start:max(data_start, i)]))
        pos, last = end
    return parts


def normalize_form_list(values: Sequence[str]) -> List[str]:
    """repeated and / or comma-separated form fields -> one list (server.py:540-548)"""
    out: List[str] = []
    for value in values or []:
        if isinstance(value, str):
            out.extend(item.strip() for item in value.split(",") if item.strip())
    return out


# ------------------------------------------------------------------------------------------------------------ rendering
def _json_bytes(obj) -> bytes:
    """Starlette's JSONResponse rendering (what FastAPI sends for a returned dict)"""
    return json.dumps(obj, ensure_ascii=False, allow_nan=False, indent=None, separators=(",", ":")).encode("utf-8")


def _stamp(t: float) -> str:
    return f"{int(t // 3600):02}:{int((t % 3600) // 60):02}:{t % 60:06.3f}"


def _words(seg) -> list:
    return [{"word": w.word, "start": w.start, "end": w.end, "probability": w.probability} for w in seg.words]


def _shown(seg, translated: bool) -> str:
    """the text a response shows for a segment: its translation for a request with target_language, else its text"""
    return (seg.translation if translated else seg.text).strip()


def render_subtitles(segments, response_format: str, translated: bool = False) -> str:
    """A segment that carries a channel (a multichannel request) has its cue text prefixed `[ch N] `. translated: the cues carry the
    segments' translations (file_translation.translate_segments), on the source's times."""
    output = []
    for i, seg in enumerate(segments, 1):
        start, end = _stamp(seg.start), _stamp(seg.end)
        ch = getattr(seg, "channel", None)
        cue = ("" if ch is None else f"[ch {ch}] ") + _shown(seg, translated)
        if response_format == "srt":
            output.append(f"{i}\n{start.replace('.', ',')} --> {end.replace('.', ',')}\n{cue}\n")
        else:
            output.append(f"{start} --> {end}\n{cue}\n")
    return "\n".join(output)


def render_text(segments, multichannel: bool = False, translated: bool = False) -> str:
    """the `text` of a response: the segments joined with spaces; a multichannel request gets one line per segment, in time order.
    translated: the same of the segments' translations."""
    return ("\n" if multichannel else " ").join([_shown(s, translated) for s in segments])


def parse_bool_field(value: Optional[str], name: str) -> bool:
    """the truthiness parsing of the `stream` form field, for any boolean field; _HttpError 400 for anything else"""
    s = (value or "").strip().lower()
    if s not in _TRUE and s not in _FALSE:
        raise _HttpError(400, {"error": f"{name} must be a boolean"})
    return s in _TRUE


def keyword_scope(transcriber, keywords: Sequence[str], keywords_boost: Optional[str], compact: bool = False):
    """The `keywords` (repeatable) and `keywords_boost` form fields -> the context manager under which the upload is decoded
    (WhisperModelHIP.keyword_bias on the request's thread), or None without keywords. compact=True compiles the compact form, the
    one a pooled job decodes under (many_files.py): the pooled route validates with it and does not enter the scope. _HttpError 400: a boost that is not a finite
    number, an empty keyword, a boost without keywords, a table past a cap (the message names it: nodes, edges), a transcriber that
    does not bias."""
    boost = None
    if keywords_boost is not None and keywords_boost.strip():
        try:
            boost = float(keywords_boost)
        except ValueError:
            boost = float("nan")
        if boost != boost or boost in (float("inf"), float("-inf")):
            raise _HttpError(400, {"error": "keywords_boost must be a finite number"})
    if not keywords:
        if boost is not None:
            raise _HttpError(400, {"error": "keywords_boost needs at least one keywords field"})
        return None
    if not hasattr(transcriber, "keyword_bias"):
        raise _HttpError(400, {"error": "keywords: this server's transcriber does not bias"})
    try:
        return transcriber.keyword_bias(phrases=list(keywords), boost=boost, **({"compact": True} if compact else {}))
    except ValueError as e:
        raise _HttpError(400, {"error": f"keywords: {e}"})


def file_channels(data: bytes) -> int:
    """channel count of a WAV / FLAC upload from its header (0: not readable there; the transcription then says what is wrong)"""
    try:
        if data[:4] == b"fLaC" and len(data) >= 42 and (data[4] & 0x7F) == 0:
            return ((data[20] >> 1) & 7) + 1
        if data[:4] == b"RIFF":
            from .audio_io import _wav_parse
            return int(_wav_parse(data)[1])
    except Exception:  # noqa: BLE001
        pass
    return 0


def speaker_labels_per_channel(segments, diarizer, resident_of) -> Dict[int, str]:
    """speaker_labels_for_segments for a multichannel transcription: each segment's audio is read from its OWN channel's resident
    item (`resident_of(channel)` -> engine.ResidentPcm or None), one embedding call per channel. -> {segment index: speaker}"""
    labels: Dict[int, str] = {}
    for ch in sorted({s.channel for s in segments if s.channel is not None}):
        index = [i for i, s in enumerate(segments) if s.channel == ch]
        got = speaker_labels_for_segments([segments[i] for i in index], None, diarizer, resident=resident_of(ch))
        labels.update({index[k]: v for k, v in got.items()})
    return labels


def segment_sample_ranges(segments, n_samples: int, sample_rate: int = 16000) -> List[Tuple[int, int, int]]:
    """(segment index, start, end) in samples for every segment with audio in [0, n_samples): int(t * sample_rate), clamped to the
    file; an empty segment or one outside the file has no entry (server.py:588-592)"""
    ranges = []
    for index, segment in enumerate(segments):
        start = max(0, int(segment.start * sample_rate))
        end = min(int(n_samples), int(segment.end * sample_rate))
        if end > start:
            ranges.append((index, start, end))
    return ranges


def speaker_labels_for_segments(segments, audio_np, diarizer, sample_rate: int = 16000, resident=None) -> Dict[int, str]:
    """server.py:585-598. A diarizer with `identify_speakers` gets all non-empty ranges in one call (SpeakerDiarizer embeds them in
    batches on the device); the labels are those of the one-by-one loop, which any other diarizer still gets.
    `resident`: the file's 16 kHz audio where the transcription left it on the device (engine.ResidentPcm), or None. With it, and a
    diarizer that can read it (`identify_speakers_resident`), the segments are embedded from there and `audio_np` is not touched.
    `audio_np` may be a callable that returns the waveform: it is called only when the host route is taken (the file is then decoded a
    second time), which is also where a resident route that fails before any speaker was assigned ends up."""
    if diarizer is None or (audio_np is None and resident is None):
        return {}
    if resident is not None and sample_rate == 16000 and _reads_resident(diarizer, resident):
        ranges = segment_sample_ranges(segments, resident.n_samples, sample_rate)
        try:
            speakers = diarizer.identify_speakers_resident(resident, [(start, end - start) for _, start, end in ranges])
            return {index: speaker for (index, _, _), speaker in zip(ranges, speakers) if speaker}
        except _WlxError as e:          # evicted or released under us: refused before any launch and before any clustering step
            logging.warning(f"speaker labels: the resident audio could not be read ({e}); decoding the file again")
    if callable(audio_np):
        audio_np = audio_np()
    if audio_np is None:
        return {}
    ranges = segment_sample_ranges(segments, len(audio_np), sample_rate)
    if hasattr(diarizer, "identify_speakers"):
        speakers = diarizer.identify_speakers([audio_np[start:end] for _, start, end in ranges], sample_rate)
    else:
        speakers = [diarizer.identify_speaker(audio_np[start:end], sample_rate) for _, start, end in ranges]
    return {index: speaker for (index, _, _), speaker in zip(ranges, speakers) if speaker}


def _reads_resident(diarizer, resident) -> bool:
    if not hasattr(diarizer, "identify_speakers_resident"):
        return False
    supports = getattr(diarizer, "supports_resident", None)
    return bool(supports(resident)) if supports is not None else True


def diarize_file_segments(segments, diarizer, resident_of, known=None, multichannel: bool = False):
    """The `diarize=true` route: offline diarization (file_diarization.FileDiarizer) of the audio the transcription left on the device,
    once per channel of a multichannel request. `resident_of(channel)` -> engine.ResidentPcm or None (channel None: a mono request).
    -> (speaker per segment, per segment the speaker of each word or None, speakers in order of first appearance). The speakers of a
    multichannel request carry their channel (`CH1_SPEAKER_00`): the clusters of two channels are not the same people; a name of
    `known` stays as it is. A word that overlaps no turn (one of no duration) takes its segment's speaker, a segment that overlaps
    none the speaker of the turn nearest in time. ValueError: nothing resident to read."""
    from .file_diarization import label_segments, merge_spans
    seg_speakers: List[Optional[str]] = [None] * len(segments)
    word_speakers: List[Optional[List[Optional[str]]]] = [None] * len(segments)
    speakers: List[str] = []
    channels = sorted({s.channel for s in segments if getattr(s, "channel", None) is not None}) if multichannel else [None]
    for ch in channels:
        index = [i for i, s in enumerate(segments) if ch is None or s.channel == ch]
        if not index:
            continue
        resident = resident_of(ch)
        if resident is None:
            raise ValueError("diarize needs the file's audio resident on the device; this request's was not kept there")
        turns = diarizer.diarize(resident, merge_spans([segments[i] for i in index]), known=known)
        if ch is not None:
            turns = [(a, b, who if known and who in known else f"CH{ch}_{who}") for a, b, who in turns]
        per_seg, per_word = label_segments([segments[i] for i in index], turns)
        for k, i in enumerate(index):
            seg_speakers[i], word_speakers[i] = per_seg[k], per_word[k]
        for _, _, who in turns:
            if who not in speakers:
                speakers.append(who)
    return seg_speakers, word_speakers, speakers


class _Upload:
    """one request waiting in the batcher"""
    __slots__ = ("transcriber", "key", "data", "per_file", "shared", "done", "result", "error")

    def __init__(self, transcriber, key, data, per_file, shared):
        self.transcriber, self.key, self.data, self.per_file, self.shared = transcriber, key, data, per_file, shared
        self.done, self.result, self.error = threading.Event(), None, None


def grammar_scope(transcriber, grammar: Sequence[str], grammar_repeat: Optional[str], keywords=None, keywords_boost=None):
    """The `grammar` (repeatable: one phrase per field) and `grammar_repeat` form fields -> the context manager under which the upload
    is decoded (WhisperModelHIP.grammar on the request's thread), or None without a grammar. 400: a repeat flag that is no boolean or
    comes without a grammar, an empty phrase, a grammar together with keywords, a list past a limit (the message names it: states,
    edges), a transcriber that takes no grammar."""
    repeat = True
    if grammar_repeat is not None and grammar_repeat.strip():
        repeat = parse_bool_field(grammar_repeat, "grammar_repeat")
        if not grammar:
            raise _HttpError(400, {"error": "grammar_repeat needs at least one grammar field"})
    if not grammar:
        return None
    if keywords or (keywords_boost is not None and keywords_boost.strip()):
        raise _HttpError(400, {"error": "grammar cannot be combined with keywords: a file decodes under one of them"})
    if not hasattr(transcriber, "grammar"):
        raise _HttpError(400, {"error": "grammar: this server's transcriber takes no grammar"})
    try:
        return transcriber.grammar(phrases=list(grammar), repeat=repeat)
    except ValueError as e:
        raise _HttpError(400, {"error": f"grammar: {e}"})


def pool_upload(has_batcher: bool, multichannel: bool, known_speaker_names, known_speaker_references) -> bool:
    """whether an upload joins the pooled jobs: keywords do not keep it out (each file of a job has its own table); multichannel
    files and known speakers do"""
    return bool(has_batcher) and not multichannel and not known_speaker_names and not known_speaker_references


class FileBatcher:
    """Pools concurrent uploads into BatchedInferencePipeline.iter_many jobs (RestServer keeps one per GPU). One worker thread: it takes the oldest waiting upload,
    collects for `window_s` seconds the uploads that arrive for the same transcriber with equal group-wide decode options (`shared`:
    task, beam size, temperature, word_timestamps, ... — compared as a whole; language, prompt and hotwords are per file and may
    differ), `batch_size` of them at the most (one wave of a transcriber built with max_batch = 2 x batch_size), and runs them as
    one job; uploads with other options wait for the next job. Each request is answered from its own result as soon as the job yields
    it. `make_pipeline(transcriber)` -> the pipeline (anything with `iter_many`). `jobs` counts the jobs run."""

    def __init__(self, make_pipeline: Callable, batch_size: int, window_s: float, wave_put: bool = False):
        self.make_pipeline, self.batch_size, self.window_s = make_pipeline, int(batch_size), float(window_s)
        self.wave_put = bool(wave_put)      # a job's files go up in one Slot.put_many call per wave (iter_many(wave_put=True))
        self.jobs = 0
        self._waiting: List[_Upload] = []
        self._cv = threading.Condition()
        self._closed = False
        self._thread = threading.Thread(target=self._run, name="wlx-rest-batcher", daemon=True)
        self._thread.start()

    def submit(self, transcriber, data: bytes, per_file: dict, shared: dict):
        up = _Upload(transcriber, (id(transcriber), repr(sorted(shared.items()))), data, per_file, shared)
        with self._cv:
            if self._closed:
                raise RuntimeError("the server is shutting down")
            self._waiting.append(up)
            self._cv.notify_all()
        up.done.wait()
        if up.error is not None:
            raise up.error
        return up.result

    def close(self):
        with self._cv:
            self._closed = True
            self._cv.notify_all()
        self._thread.join()

    def _collect(self) -> Optional[List[_Upload]]:
        """the next job's uploads: the oldest one and those of its key that arrive within the window (None: closed and drained)"""
        with self._cv:
            while not self._waiting:
                if self._closed:
                    return None
                self._cv.wait()
            key, deadline = self._waiting[0].key, time.monotonic() + self.window_s
            while True:
                same = [u for u in self._waiting if u.key == key]
                left = deadline - time.monotonic()
                if len(same) >= self.batch_size or left <= 0 or self._closed:
                    break
                self._cv.wait(left)
            job = same[: self.batch_size]
            self._waiting = [u for u in self._waiting if u not in job]
            return job

    def _run(self):
        while True:
            job = self._collect()
            if job is None:
                return
            self.jobs += 1
            transcriber = job[0].transcriber
            try:
                results = self.make_pipeline(transcriber).iter_many(
                    [u.data for u in job], batch_size=self.batch_size, vad_filter=True,
                    **{name: [u.per_file[name] for u in job] for name in ("language", "initial_prompt", "hotwords")}, **job[0].shared,
                    **({"diarize": [u.per_file.get("diarize") or False for u in job], "max_speakers": [int(u.per_file.get("max_speakers") or 0) for u in job]}
                       if any(u.per_file.get("diarize") for u in job) else {}),
                    **({"keywords": [u.per_file.get("keywords") for u in job], "keywords_boost": [u.per_file.get("keywords_boost") for u in job]}
                       if any(u.per_file.get("keywords") for u in job) else {}),
                    **({"wave_put": True} if self.wave_put else {}))
                for index, segments, info in results:
                    up = job[index]
                    if info is None:
                        up.error = segments
                    else:
                        up.result = (segments, info)
                    up.done.set()
            except Exception as e:  # noqa: BLE001 — an error of the job as a whole is every waiting request's error
                for up in job:
                    if not up.done.is_set():
                        up.error = e
            finally:
                for up in job:
                    if not up.done.is_set():
                        if up.error is None and up.result is None:
                            up.error = RuntimeError("the pooled job ended without this file's result")
                        up.done.set()
                release = getattr(transcriber, "release_slot", None)
                if release is not None:
                    try:
                        release()
                    except Exception:  # noqa: BLE001
                        logging.exception("rest: release_slot failed")


class _HttpError(Exception):
    def __init__(self, status: int, payload: dict):
        super().__init__(payload.get("error", ""))
        self.status, self.payload = status, payload


_TRUE = {"true", "1", "yes", "on", "t", "y"}
_FALSE = {"false", "0", "no", "off", "f", "n", ""}


# ------------------------------------------------------------------------------------------------------------ the server
class RestServer:
    """Threaded HTTP server of the endpoint. ``model``: what the transcriber of a GPU is built from (a size name or a model
    directory, as the WebSocket server's faster_whisper_custom_model_path); ``model_factory(model, device_index)`` replaces the
    construction, as in TranscriptionServer. ``start()`` returns once the socket listens (``port`` 0: see ``.port``);
    ``shutdown()`` waits for the requests in flight and leaves no thread behind."""

    pipeline_factory: Optional[Callable] = None        # (transcriber) -> the pipeline of a file; None: BatchedInferencePipeline
    batcher: Optional["FileBatcher"] = None            # set when file_batch_window_ms > 0

    def __init__(self, host: str, port: int, model: str, *, devices: Sequence[int] = (0,), api_key: Optional[str] = None,
                 cors_origins: Optional[str] = None, rate_limit_rpm: int = 0, model_factory: Optional[Callable] = None,
                 max_body_bytes: int = 512 << 20, diarization_model: Optional[str] = None,
                 embedder_factory: Optional[Callable] = None, file_batch_size: int = 0, file_batch_window_ms: int = 0,
                 pipeline_factory: Optional[Callable] = None, translation_model: Optional[str] = None,
                 translator_factory: Optional[Callable] = None, file_batch_wave_put: bool = False):
        self.host, self.port, self.model = host, int(port), model
        self.file_batch_wave_put = bool(file_batch_wave_put)     # the pooled jobs put each wave of files in one call (FileBatcher.wave_put)
        # a small100 / M2M100 checkpoint (a directory or a hub id, resolved as the WebSocket server resolves its own): requests may then
        # carry target_language. translator_factory: (directory, device index) -> translator; None = translation.shared_translator
        self.translation_model = translation_model
        self.translator_factory = translator_factory
        # 0: a file is decoded one window after another (WhisperModelHIP.transcribe). N > 0: the GPU's shared transcriber is built with
        # max_batch = N and a file goes through BatchedInferencePipeline, N speech chunks per decode step
        self.file_batch_size = int(file_batch_size)
        if not 0 <= self.file_batch_size <= 64:
            raise ValueError("file_batch_size must be 0 (sequential decoding) or 1..64 chunks per decode step")
        # 0: every request runs its pipeline alone, as before. W > 0: uploads that arrive within W ms of one another, and decode with
        # the same group-wide options, run as ONE BatchedInferencePipeline.iter_many job (FileBatcher below); the transcriber is then
        # built with max_batch = 2 N: N chunks per decode step in front of a wave of up to N files
        self.file_batch_window_ms = int(file_batch_window_ms)
        if self.file_batch_window_ms < 0:
            raise ValueError("file_batch_window_ms must be 0 (off) or a number of milliseconds")
        if self.file_batch_window_ms > 0 and not 1 <= self.file_batch_size <= 32:
            raise ValueError("file_batch_window_ms needs file_batch_size 1..32 (the chunks per decode step of the pooled job)")
        self.pipeline_factory = pipeline_factory
        self.devices = list(devices) if devices else [0]
        if any(d < 0 for d in self.devices):
            raise ValueError("devices must be non-negative GPU indices")
        self.api_key = api_key
        self.origins = [o.strip() for o in cors_origins.split(",")] if cors_origins else []
        self.rate_limit_rpm = int(rate_limit_rpm)
        self.model_factory = model_factory
        self.max_body_bytes = int(max_body_bytes)
        self.diarization_model = diarization_model
        self.embedder_factory = embedder_factory
        self._rate_lock = threading.Lock()
        self._rate_buckets: Dict[str, collections.deque] = {}
        self._n_requests = 0
        self._req_lock = threading.Lock()
        self._httpd: Optional[ThreadingHTTPServer] = None
        self._thread: Optional[threading.Thread] = None
        # last, when nothing above can refuse the arguments any more: one batcher (one worker thread) per GPU, so that the pooled jobs
        # of different devices run side by side; `batcher` is the first device's
        self._batchers: Dict[int, FileBatcher] = {}
        self._pooled_diarizers: Dict[int, object] = {}
        self._pooled_diarizers_mu = threading.Lock()
        if self.file_batch_window_ms > 0:
            self._batchers = {d: FileBatcher(self._pipeline, self.file_batch_size, self.file_batch_window_ms / 1000.0, self.file_batch_wave_put) for d in self.devices}
            self.batcher = self._batchers[self.devices[0]]

    # ---- life cycle
    def start(self) -> "RestServer":
        server = self

        class Handler(_Handler):
            rest = server

        self._httpd = ThreadingHTTPServer((self.host, self.port), Handler)
        self._httpd.daemon_threads = False          # server_close() joins the request threads
        self.port = self._httpd.server_address[1]
        self._thread = threading.Thread(target=self._httpd.serve_forever, kwargs={"poll_interval": 0.05}, name="wlx-rest")
        self._thread.start()
        logging.info(f"OpenAI-compatible API started on http://{self.host}:{self.port}")
        return self

    def shutdown(self):
        if self._httpd is not None:
            self._httpd.shutdown()
            self._httpd.server_close()
            self._httpd = None
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        for b in getattr(self, "_batchers", {}).values():
            b.close()

    def serve_forever(self):
        self.start()
        try:
            while self._thread is not None and self._thread.is_alive():
                self._thread.join(0.5)
        except KeyboardInterrupt:
            pass
        finally:
            self.shutdown()

    # ---- the pieces of a request
    def rate_limited(self, client_ip: str) -> bool:
        if self.rate_limit_rpm <= 0:
            return False
        now = time.time()
        with self._rate_lock:
            bucket = self._rate_buckets.setdefault(client_ip, collections.deque())
            while bucket and bucket[0] < now - 60:
                bucket.popleft()
            if len(bucket) >= self.rate_limit_rpm:
                return True
            bucket.append(now)
        return False

    def _next_device(self) -> int:
        with self._req_lock:
            i = self._n_requests
            self._n_requests += 1
        return self.devices[assign_gpu(i, len(self.devices))]

    def transcriber_for(self, device_index: int):
        """the GPU's shared transcriber: the cache (and lock) of the single_model WebSocket sessions"""
        from .serve_client import ServeClientHIP
        with ServeClientHIP.MODELS_LOCK:
            if device_index not in ServeClientHIP.MODELS:
                kw = {"max_batch": self.file_batch_size * (2 if self.batcher is not None else 1)} if self.file_batch_size > 0 else {}
                if self.model_factory is not None:
                    ServeClientHIP.MODELS[device_index] = self.model_factory(self.model, device_index, **kw)
                else:
                    ServeClientHIP.MODELS[device_index] = ServeClientHIP.create_model(self.model, device_index, **kw)
            return ServeClientHIP.MODELS[device_index]

    def transcribe_file(self, transcriber, data: bytes, multichannel: bool = False, **kw):
        """-> (iterable of segments or None, info or None). file_batch_size = 0: today's sequential path, exactly. Otherwise the batched
        pipeline with the VAD chunking; its segments arrive lazily, group by group. multichannel: always the batched pipeline on the
        shared transcriber, each channel on its own; a transcriber that cannot hold the channels and one chunk is a 400."""
        if multichannel:
            from .batched import BatchedInferencePipeline
            channels, max_batch = max(1, file_channels(data)), int(getattr(transcriber, "max_batch", 1))
            if max_batch < channels + 1:
                raise _HttpError(400, {"error": f"multichannel: a file of {channels} channels needs a transcriber that holds {channels + 1} "
                                                f"items, this server's holds {max_batch} (start it with a file batch size >= {channels + 1})"})
            batch = min(self.file_batch_size if self.file_batch_size > 0 else max_batch, max_batch - channels)
            try:
                return BatchedInferencePipeline(transcriber).transcribe(data, vad_filter=True, batch_size=batch, multichannel=True, **kw)
            except ValueError as e:              # a shape the device front end refuses: there is no host route
                raise _HttpError(400, {"error": str(e)})
        if self.file_batch_size <= 0:
            return transcriber.transcribe(data, vad_filter=False, **kw)
        return self._pipeline(transcriber).transcribe(data, vad_filter=True, batch_size=self.file_batch_size, **kw)

    def _pipeline(self, transcriber):
        if self.pipeline_factory is not None:
            return self.pipeline_factory(transcriber)
        from .batched import BatchedInferencePipeline
        return BatchedInferencePipeline(transcriber)

    def transcribe_pooled(self, transcriber, data: bytes, *, device_index: Optional[int] = None, language=None, initial_prompt=None,
                          hotwords=None, diarize=None, max_speakers: int = 0, keywords=None, keywords_boost=None, **shared):
        """`transcribe_file` through the batcher (file_batch_window_ms > 0): the upload joins the uploads that arrive within the window
        and decode with the same `shared` options; -> (list of segments, info) of this upload, or its own error raised here, in the
        request's thread, where the single route would have raised it. Nothing is left for `resident_file_audio` after a pooled job
        (many_files.py), so speaker labels fall back to the second decode; requests with known speakers are not pooled at all.
        diarize: the FileDiarizer of a `diarize=true` upload (pooled_file_diarizer) with its max_speakers — the job finds the speakers
        while the wave's files are still resident: the segments and words come back with `.speaker`, the info with `.speakers`."""
        per_file = dict(language=language, initial_prompt=initial_prompt, hotwords=hotwords, diarize=diarize or False, max_speakers=int(max_speakers),
                        keywords=keywords, keywords_boost=keywords_boost)       # (per file: each upload of a job decodes under its own table)
        return self._batchers.get(device_index, self.batcher).submit(transcriber, data, per_file, shared)

    def translator_for(self, device_index: int, target_language: str):
        """the GPU's shared translator for a request with target_language; ValueError = a 400 (no model configured, or a language
        code the model does not know)"""
        from .file_translation import check_target_language
        if not self.translation_model:
            raise ValueError("target_language: this server has no translation model (start it with --translation_model DIR)")
        if self.translator_factory is not None:
            translator = self.translator_factory(self.translation_model, device_index)
        else:
            from .artifacts import resolve_translation_model
            from .translation import shared_translator
            directory = resolve_translation_model(self.translation_model)
            if directory is None:
                raise ValueError(f"target_language: the translation model {self.translation_model!r} cannot be resolved on this server")
            translator = shared_translator(directory, device_index)
        check_target_language(translator, target_language)
        return translator

    @staticmethod
    def resident_audio(transcriber):
        """the file the calling thread just transcribed, where it lies on the device (engine.ResidentPcm), or None: a transcriber
        without the front end, a file that went the host route, a slot already released"""
        get = getattr(transcriber, "resident_file_audio", None)
        try:
            return get() if get is not None else None
        except Exception:  # noqa: BLE001 — labelling then takes the host route
            logging.exception("rest: resident_file_audio failed")
            return None

    def create_rest_diarizer(self, known_speaker_names, known_speaker_references, device_index: int):
        """server.py:550-583 on this GPU's shared embedder; ValueError = a 400"""
        speaker_names = normalize_form_list(known_speaker_names)
        speaker_references = known_speaker_references or []
        if speaker_references and not speaker_names:
            raise ValueError("known_speaker_references requires matching known_speaker_names")
        if speaker_names and speaker_references and len(speaker_names) != len(speaker_references):
            raise ValueError("known_speaker_names and known_speaker_references must have the same length")
        if not speaker_names and not speaker_references:
            return None
        from .artifacts import resolve_diarization_model
        from .audio_io import load_audio
        from .diarization import SpeakerDiarizer, shared_embedder
        path = resolve_diarization_model(self.diarization_model)
        if path is None and self.embedder_factory is None:
            raise ValueError("known speakers requested but no speaker-embedding checkpoint is available on this server")
        embedder = (self.embedder_factory or shared_embedder)(path, device_index)
        diarizer = SpeakerDiarizer(max_speakers=max(10, len(speaker_names)), speaker_names=speaker_names, embedder=embedder,
                                   device=device_index)
        for speaker_name, reference in zip(speaker_names, speaker_references):
            audio_np = load_audio(reference.data)
            if not diarizer.enroll_speaker(speaker_name, audio_np):
                raise ValueError(f"known_speaker_references for '{speaker_name}' is too short")
        return diarizer


    def create_file_diarizer(self, device_index: int, max_speakers: int = 0):
        """the offline diarizer of a `diarize=true` request on this GPU's shared embedder; ValueError = a 400"""
        from .artifacts import resolve_diarization_model
        from .diarization import shared_embedder
        from .file_diarization import FileDiarizer
        path = resolve_diarization_model(self.diarization_model)
        if path is None and self.embedder_factory is None:
            raise ValueError("known speakers requested but no speaker-embedding checkpoint is available on this server")
        return FileDiarizer((self.embedder_factory or shared_embedder)(path, device_index), max_speakers=max_speakers)

    def pooled_file_diarizer(self, device_index: int):
        """ONE diarizer per GPU for the `diarize=true` uploads that go through the batcher: the job runs one diarize_many per diarizer
        and wave (many_files.py), so the pooled requests share theirs and carry max_speakers per file; ValueError = a 400"""
        with self._pooled_diarizers_mu:
            if device_index not in self._pooled_diarizers:
                self._pooled_diarizers[device_index] = self.create_file_diarizer(device_index, 0)
            return self._pooled_diarizers[device_index]


class _Handler(BaseHTTPRequestHandler):
    rest: RestServer = None           # set by RestServer.start()
    server_version = "whisperlive-amd-rest"
    timeout = 60                      # seconds a socket read or write may stall: a stuck client does not hold shutdown() for ever
    DRAIN_BYTES = 16 << 20            # of an unread body, this much is read and dropped before an early answer (see _drain)
    _body_unread = 0
    _expects_continue = False

    def _drain(self):
        """Before an answer that did not read the body: read and drop what the client is still sending (a bounded amount), so that
        it sees the status and not a reset connection. A client that waits for 100 Continue has sent nothing."""
        left = 0 if self._expects_continue else min(self._body_unread, self.DRAIN_BYTES)
        self._body_unread = 0
        try:
            while left > 0:
                chunk = self.rfile.read(min(left, 1 << 16))
                if not chunk:
                    break
                left -= len(chunk)
        except OSError:                # (a timeout among them) the answer is still attempted
            pass

    def log_message(self, fmt, *args):          # the access log goes where the rest of the server logs
        logging.debug("rest %s - %s", self.address_string(), fmt % args)

    # ---- responses
    def _send(self, status: int, body: bytes, content_type: str, extra: Optional[Dict[str, str]] = None, cors: bool = True):
        self._drain()
        self.send_response(status)
        self.send_header("Content-Type", content_type)
        self.send_header("Content-Length", str(len(body)))
        self.send_header("Connection", "close")
        for k, v in (self._cors_simple() if cors else {}).items():
            self.send_header(k, v)
        for k, v in (extra or {}).items():
            self.send_header(k, v)
        self.end_headers()
        if self.command != "HEAD":
            self.wfile.write(body)
        self.close_connection = True

    def _json(self, status: int, obj, **kw):
        self._send(status, _json_bytes(obj), "application/json", **kw)

    def _text(self, status: int, text: str, **kw):
        self._send(status, text.encode("utf-8"), "text/plain; charset=utf-8", **kw)

    # ---- CORS (Starlette's CORSMiddleware with allow_credentials, every method and every header allowed)
    def _origin_allowed(self, origin: str) -> bool:
        return "*" in self.rest.origins or origin in self.rest.origins

    def _cors_simple(self) -> Dict[str, str]:
        origin = self.headers.get("Origin")
        if origin is None:
            return {}
        h = {"Access-Control-Allow-Credentials": "true"}
        if "*" in self.rest.origins and "Cookie" not in self.headers:
            h["Access-Control-Allow-Origin"] = "*"
        elif self._origin_allowed(origin):
            h["Access-Control-Allow-Origin"] = origin
            h["Vary"] = "Origin"
        return h

    def _preflight(self):
        origin = self.headers.get("Origin")
        h = {"Access-Control-Allow-Methods": _CORS_METHODS, "Access-Control-Max-Age": "600",
             "Access-Control-Allow-Credentials": "true", "Vary": "Origin"}
        req_headers = self.headers.get("Access-Control-Request-Headers")
        if req_headers is not None:
            h["Access-Control-Allow-Headers"] = req_headers
        if self._origin_allowed(origin):
            h["Access-Control-Allow-Origin"] = origin
            self._text(200, "OK", extra=h, cors=False)
        else:
            self._text(400, "Disallowed CORS origin", extra=h, cors=False)

    # ---- the middleware chain, then routing
    def _dispatch(self):
        rest = self.rest
        try:
            self._body_unread = max(0, int(self.headers.get("Content-Length", "0")))
        except ValueError:
            self._body_unread = 0
        # `Expect: 100-continue`: the go-ahead is sent by _form, after the checks that need no body — a client that waits for it gets
        # its 401 / 413 / 429 without having sent the upload
        self._expects_continue = (self.request_version == "HTTP/1.1" and self.headers.get("Expect", "").strip().lower() == "100-continue")
        if rest.rate_limited(self.client_address[0] if self.client_address else "unknown"):
            return self._json(429, {"error": "Rate limit exceeded"}, cors=False)
        if rest.api_key and self.headers.get("Authorization", "") != f"Bearer {rest.api_key}":
            return self._json(401, {"error": "Invalid or missing API key"}, cors=False)
        if self.command == "OPTIONS" and "Origin" in self.headers and "Access-Control-Request-Method" in self.headers:
            return self._preflight()
        path = self.path.split("?", 1)[0]
        if path != ROUTE:
            return self._json(404, {"detail": "Not Found"})
        if self.command != "POST":
            return self._json(405, {"detail": "Method Not Allowed"}, extra={"Allow": "POST"})
        try:
            self._transcriptions()
        except _HttpError as e:
            wl_metrics.track_rest_request(endpoint="transcriptions", status=e.status)
            self._json(e.status, e.payload)

    do_GET = do_POST = do_PUT = do_DELETE = do_PATCH = do_HEAD = do_OPTIONS = _dispatch

    # ---- POST /v1/audio/transcriptions (server.py:733-859)
    def _form(self):
        try:
            length = int(self.headers.get("Content-Length", ""))
        except ValueError:
            raise _HttpError(400, {"error": "Content-Length is required"})
        if length < 0:
            raise _HttpError(400, {"error": "Content-Length is required"})
        if length > self.rest.max_body_bytes:
            raise _HttpError(413, {"error": f"Request body of {length} bytes exceeds the limit of {self.rest.max_body_bytes}"})
        if self._expects_continue:
            self.wfile.write(b"HTTP/1.1 100 Continue\r\n\r\n")
            self.wfile.flush()
            self._expects_continue = False
        try:
            body = self.rfile.read(length)
        except TimeoutError:
            self._body_unread = 0
            raise _HttpError(408, {"error": "Timed out reading the request body"})
        self._body_unread = 0
        if len(body) != length:
            raise _HttpError(400, {"error": "Request body shorter than its Content-Length"})
        try:
            return parse_multipart(body, self.headers.get("Content-Type", ""))
        except ValueError as e:
            raise _HttpError(400, {"error": str(e)})

    def _transcriptions(self):
        parts = self._form()
        fields: Dict[str, List[Part]] = {}
        for p in parts:
            fields.setdefault(p.name, []).append(p)

        def one(name, default=None):
            return fields[name][-1].text if name in fields else default

        def many(name):
            return [p.text for p in fields.get(name, [])]

        if "file" not in fields:
            raise _HttpError(400, {"error": "Missing required form field 'file'"})
        file = fields["file"][0]
        model = one("model", "whisper-1")
        language, prompt, hotwords = one("language"), one("prompt"), one("hotwords")
        response_format = one("response_format", "json")
        try:
            temperature = float(one("temperature", "0.0"))
        except ValueError:
            raise _HttpError(400, {"error": "temperature must be a number"})
        stream_s = (one("stream", "false") or "").strip().lower()
        if stream_s not in _TRUE and stream_s not in _FALSE:
            raise _HttpError(400, {"error": "stream must be a boolean"})
        multichannel = parse_bool_field(one("multichannel", "false"), "multichannel")
        diarize = parse_bool_field(one("diarize", "false"), "diarize")
        target_language = (one("target_language") or "").strip() or None
        try:
            max_speakers = int(one("max_speakers", "0") or "0")
        except ValueError:
            max_speakers = -1
        if max_speakers < 0:
            raise _HttpError(400, {"error": "max_speakers must be a non-negative integer"})
        timestamp_granularities = normalize_form_list(many("timestamp_granularities") + many("timestamp_granularities[]")) or None
        chunking_strategy = one("chunking_strategy")
        include = many("include") + many("include[]") or None
        known_speaker_names = many("known_speaker_names") + many("known_speaker_names[]")
        keywords, keywords_boost = many("keywords") + many("keywords[]"), one("keywords_boost")
        grammar, grammar_repeat = many("grammar") + many("grammar[]"), one("grammar_repeat")
        known_speaker_references = fields.get("known_speaker_references", []) + fields.get("known_speaker_references[]", [])
        want_words = bool(timestamp_granularities and "word" in timestamp_granularities)
        rest = self.rest

        if stream_s in _TRUE:
            if multichannel:     # the segments of a multichannel file are ordered only when its last group is done: nothing to stream
                raise _HttpError(400, {"error": "multichannel cannot be combined with stream: send the request without stream"})
            if keywords or keywords_boost:
                raise _HttpError(400, {"error": "keywords cannot be combined with stream: send the request without stream"})
            if grammar or grammar_repeat:
                raise _HttpError(400, {"error": "grammar cannot be combined with stream: send the request without stream"})
            return self._stream(file, language, prompt, temperature, want_words, target_language)

        ignored_params = []
        if chunking_strategy:
            ignored_params.append(f"chunking_strategy='{chunking_strategy}'")
        if include:
            ignored_params.append(f"include={include}")
        if ignored_params:
            logging.warning(f"Unsupported OpenAI params ignored: {', '.join(ignored_params)}")
        if response_format not in SUPPORTED_FORMATS:
            raise _HttpError(400, {"error": f"Unsupported response_format. Supported: {SUPPORTED_FORMATS}"})
        if model != "whisper-1":
            logging.warning(f"Model '{model}' requested; using '{rest.model}' as fallback.")
        if file.data[:4] not in (b"fLaC", b"RIFF"):
            raise _HttpError(400, {"error": "Unsupported audio: the file is neither WAV nor FLAC"})

        transcriber = None
        try:
            device_index = rest._next_device()
            translator = None
            if target_language is not None:         # refused before the file is decoded
                try:
                    translator = rest.translator_for(device_index, target_language)
                except ValueError as e:
                    raise _HttpError(400, {"error": str(e)})
            transcriber = rest.transcriber_for(device_index)
            mc = {"multichannel": True} if multichannel else {}
            # a diarize=true upload without known speakers is pooled too: the job finds its speakers while the wave is resident
            pooled = pool_upload(rest.batcher is not None, multichannel, known_speaker_names, known_speaker_references)
            pooled_diarizer = None
            # (where the GPU's embedder has the wave call, diarize_many: without it pooling would only queue the per-file route)
            if pooled and diarize and response_format == "verbose_json":
                try:
                    pooled_diarizer = rest.pooled_file_diarizer(device_index)
                except ValueError as e:
                    raise _HttpError(400, {"error": str(e)})
                if not hasattr(pooled_diarizer.embedder, "diarize_many"):
                    pooled, pooled_diarizer = False, None
            # keywords: the table is compiled (and refused: 400) before the file is decoded. An upload that is not pooled is decoded in this
            # thread under it (the segments may arrive lazily: they are drawn inside the scope); a pooled one carries its keywords into the
            # job, where every file decodes under its own table in the compact form (many_files.py: a decode group takes a table per
            # item) — so that is the form its list is checked in here, and the scope is not entered.
            # grammar: compiled (and refused: 400) before the file is decoded too. One grammar serves a whole decode group, so an upload with
            # one is not pooled with other uploads: it is decoded in this thread under its grammar.
            gram = grammar_scope(transcriber, grammar, grammar_repeat, keywords, keywords_boost)
            if gram is not None:
                pooled, pooled_diarizer = False, None
            bias = keyword_scope(transcriber, keywords, keywords_boost, compact=pooled)
            with (bias if bias is not None and not pooled else contextlib.nullcontext()), (gram if gram is not None else contextlib.nullcontext()):
                if pooled:
                    segments, info = rest.transcribe_pooled(transcriber, file.data, device_index=device_index, language=language, initial_prompt=prompt,
                                                            temperature=temperature, word_timestamps=want_words, hotwords=hotwords,
                                                            diarize=pooled_diarizer, max_speakers=max_speakers,
                                                            keywords=list(keywords) if bias is not None else None,
                                                            keywords_boost=float(keywords_boost) if bias is not None and keywords_boost is not None and keywords_boost.strip() else None)
                else:
                    segments, info = rest.transcribe_file(transcriber, file.data, language=language, initial_prompt=prompt,
                                                          temperature=temperature, word_timestamps=want_words, hotwords=hotwords, **mc)
                segments = list(segments or [])
            text = render_text(segments, multichannel)
            translated = target_language is not None
            if translated:      # the whole transcript as one translation job, whichever route transcribed it
                from .file_translation import translate_segments
                segments = translate_segments(segments, translator, target_language)
                translation = render_text(segments, multichannel, translated=True)
            if response_format == "text":
                wl_metrics.track_rest_request(endpoint="transcriptions", status=200)
                return self._text(200, translation if translated else text)
            if response_format == "json":
                wl_metrics.track_rest_request(endpoint="transcriptions", status=200)
                return self._json(200, {"text": text, "translation": translation} if translated else {"text": text})
            if response_format == "verbose_json":
                verbose = {"task": "transcribe", "language": info.language if info else language,
                           "duration": info.duration if info else 0.0, "text": text, "segments": []}
                if translated:
                    verbose["target_language"] = target_language
                    verbose["translation"] = translation
                speaker_labels = {}
                try:
                    rest_diarizer = rest.create_rest_diarizer(known_speaker_names, known_speaker_references, device_index)
                except ValueError as e:
                    raise _HttpError(400, {"error": str(e)})
                word_speakers = None
                if diarize and pooled_diarizer is not None:
                    # the pooled job has labelled the segments (many_files._speakers), by the rules of diarize_file_segments
                    seg_speakers = [getattr(seg, "speaker", None) for seg in segments]
                    word_speakers = [[getattr(w, "speaker", None) for w in seg.words] if getattr(seg, "words", None) else None for seg in segments]
                    verbose["speakers"] = list(getattr(info, "speakers", None) or [])
                    speaker_labels = {i: who for i, who in enumerate(seg_speakers) if who}
                elif diarize:
                    # offline: every window of the file clustered at once (file_diarization.py); enrolled speakers only name clusters
                    resident_of = (getattr(transcriber, "resident_file_audio", lambda c: None) if multichannel
                                   else lambda _ch: rest.resident_audio(transcriber))
                    try:
                        file_diarizer = rest.create_file_diarizer(device_index, max_speakers)
                        seg_speakers, word_speakers, verbose["speakers"] = diarize_file_segments(
                            segments, file_diarizer, resident_of, known=dict(rest_diarizer.speakers) if rest_diarizer is not None else None,
                            multichannel=multichannel)
                    except ValueError as e:
                        raise _HttpError(400, {"error": str(e)})
                    speaker_labels = {i: who for i, who in enumerate(seg_speakers) if who}
                elif rest_diarizer is not None and multichannel:
                    speaker_labels = speaker_labels_per_channel(segments, rest_diarizer, getattr(transcriber, "resident_file_audio", lambda c: None))
                elif rest_diarizer is not None:
                    # from the audio the transcription left in the thread's slot (held until _release below); the file is decoded
                    # a second time only when nothing is resident (host-resampled rate, an engine without the front end)
                    from . import audio_io
                    speaker_labels = speaker_labels_for_segments(segments, lambda: audio_io.load_audio(file.data), rest_diarizer,
                                                                 resident=rest.resident_audio(transcriber))
                for index, seg in enumerate(segments):
                    seg_dict = {"id": seg.id, "seek": seg.seek, "start": seg.start, "end": seg.end, "text": seg.text.strip(),
                                "tokens": seg.tokens, "temperature": seg.temperature, "avg_logprob": seg.avg_logprob,
                                "compression_ratio": seg.compression_ratio, "no_speech_prob": seg.no_speech_prob}
                    if translated:
                        seg_dict["translation"] = seg.translation.strip()
                    if multichannel:
                        seg_dict["channel"] = seg.channel
                    if index in speaker_labels:
                        seg_dict["speaker"] = speaker_labels[index]
                    if want_words:
                        seg_dict["words"] = _words(seg)
                        if word_speakers is not None and word_speakers[index] is not None:
                            for word, who in zip(seg_dict["words"], word_speakers[index]):
                                if who:
                                    word["speaker"] = who
                    verbose["segments"].append(seg_dict)
                wl_metrics.track_rest_request(endpoint="transcriptions", status=200)
                return self._json(200, verbose)
            wl_metrics.track_rest_request(endpoint="transcriptions", status=200)
            return self._text(200, render_subtitles(segments, response_format, translated))
        except _HttpError:
            raise
        except Exception as e:  # noqa: BLE001 — server.py:853-856
            wl_metrics.track_rest_request(endpoint="transcriptions", status=500)
            wl_metrics.track_error("rest_transcription")
            self._release(transcriber)          # before the answer: the client may act on it at once
            transcriber = None
            return self._json(500, {"error": str(e)})
        finally:
            self._release(transcriber)

    @staticmethod
    def _release(transcriber):
        """the request thread ends here: its slot goes back to the transcriber's pool"""
        release = getattr(transcriber, "release_slot", None)
        if release is not None:
            try:
                release()
            except Exception:  # noqa: BLE001
                logging.exception("rest: release_slot failed")

    def _stream(self, file, language, prompt, temperature, want_words, target_language=None):
        """server.py:490-537: one `data:` event per segment, `[DONE]` at the end, an error as an event of its own. With
        target_language the translations follow the last segment in ONE event ({"target_language", "translations": [{id,
        translation}]}): the transcript is translated as one job, once it is complete."""
        translator = None
        if target_language is not None:
            try:
                device_index = self.rest._next_device()
                translator = self.rest.translator_for(device_index, target_language)
            except ValueError as e:
                raise _HttpError(400, {"error": str(e)})
        self.send_response(200)
        self.send_header("Content-Type", "text/event-stream; charset=utf-8")
        self.send_header("Cache-Control", "no-cache")
        self.send_header("Connection", "close")
        for k, v in self._cors_simple().items():
            self.send_header(k, v)
        self.end_headers()
        self.close_connection = True

        def emit(s: str):
            self.wfile.write(s.encode("utf-8"))
            self.wfile.flush()

        transcriber = None
        try:
            try:
                transcriber = self.rest.transcriber_for(device_index if translator is not None else self.rest._next_device())
                segments, _info = self.rest.transcribe_file(transcriber, file.data, language=language, initial_prompt=prompt,
                                                            temperature=temperature, word_timestamps=want_words)
                seen = []
                for seg in segments or []:
                    seg_dict = {"id": seg.id, "start": seg.start, "end": seg.end, "text": seg.text.strip()}
                    if want_words:
                        seg_dict["words"] = _words(seg)
                    emit(f"data: {json.dumps(seg_dict)}\n\n")
                    if translator is not None:
                        seen.append(seg)
                if translator is not None:
                    from .file_translation import translate_segments
                    done = translate_segments(seen, translator, target_language)
                    emit("data: " + json.dumps({"target_language": target_language, "translations": [
                        {"id": s.id, "translation": s.translation.strip()} for s in done]}) + "\n\n")
                emit("data: [DONE]\n\n")
            except (BrokenPipeError, ConnectionResetError):
                raise
            except Exception as e:  # noqa: BLE001
                emit(f"data: {json.dumps({'error': str(e)})}\n\n")
        except (BrokenPipeError, ConnectionResetError):
            logging.debug("rest: the client went away mid-stream")
        finally:
            self._release(transcriber)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="OpenAI-style transcription endpoint on the MI355X engine")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", "-p", type=int, default=8000)
    ap.add_argument("--model_path", "-m", default="small", help="model size name or model directory")
    ap.add_argument("--devices", default="0", help="comma-separated GPU indices to rotate requests over")
    ap.add_argument("--api_key", default=None)
    ap.add_argument("--cors_origins", default=None, help="comma-separated allowed origins")
    ap.add_argument("--rate_limit_rpm", type=int, default=0, help="requests per minute per client IP (0 = unlimited)")
    ap.add_argument("--max_body_mb", type=int, default=512)
    ap.add_argument("--diarization_model", default=None)
    ap.add_argument("--translation_model", default=None,
                    help="small100 / M2M100 checkpoint directory (or hub id): requests may then carry target_language")
    ap.add_argument("--metrics_port", type=int, default=0)
    ap.add_argument("--file_batch_size", type=int, default=0,
                    help="speech chunks decoded per step by the batched long-form pipeline (0 = decode a file window after window)")
    ap.add_argument("--file_batch_window_ms", type=int, default=0,
                    help="pool uploads that arrive within this many milliseconds into one job whose decode steps mix files "
                         "(needs --file_batch_size; 0 = every request runs alone)")
    ap.add_argument("--file_batch_wave_put", action="store_true",
                    help="the pooled jobs of --file_batch_window_ms put each wave of files on the device in one call (off by default)")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    if a.metrics_port > 0:
        wl_metrics.start_metrics_server(a.metrics_port)
    RestServer(a.host, a.port, a.model_path, devices=[int(x) for x in a.devices.split(",") if x != ""], api_key=a.api_key,
               cors_origins=a.cors_origins, rate_limit_rpm=a.rate_limit_rpm, max_body_bytes=a.max_body_mb << 20,
               diarization_model=a.diarization_model, file_batch_size=a.file_batch_size,
               file_batch_window_ms=a.file_batch_window_ms, translation_model=a.translation_model,
               file_batch_wave_put=a.file_batch_wave_put).serve_forever()


if __name__ == "__main__":
    main()
