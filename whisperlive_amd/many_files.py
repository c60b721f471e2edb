"""BatchedInferencePipeline.transcribe_many / iter_many: many files as ONE job whose decode groups mix files.

A decode step is bound by launch latency, so throughput comes from rows per step; ``transcribe`` fills them from one file, which a
20-second voicemail does not. Here a job of F files is the file plan of batched.py once more — a file is a source whose chunks share
the decode groups, as a channel is in multichannel.py — except that every source has its own length, language, prompt, clips and
result. Each file's result is what ``transcribe(audios[i], **kwargs_i)`` returns: ids from 1, times on the file's own timeline,
its own ``info``.

Waves. The decode groups write items 0 .. batch_size - 1 of the calling thread's slot and the files sit behind them, file k of a wave
in item batch_size + k, so a wave holds at most ``max_batch - batch_size`` files. A slot's PCM is one allocation with one row per
item, every row as long as the longest audio the slot was EVER asked to hold (the library grows the rows and never shrinks them): a
wave is closed early when (files + batch_size) x longest x 4 bytes would pass ``WAVE_PCM_BUDGET`` (4 GiB), or when its rows would lie
further apart than the chunk gather addresses (``multichannel.source_rows_addressable``: files x row length, in whole 30 s windows,
at most 2^31 - 1 samples). The row length of that second rule is the slot's, not the wave's: the longest of this wave's files and
``Slot.pcm_longest``, what earlier waves, earlier jobs and other routes on this thread's slot have put there — so every wave is
sized when the job gets to it (``next_wave``), and a 50-minute file in front of 48 voicemails leaves waves of at most 44 of them, not
one wave of 48 that the kernel would refuse. A file that alone passes the budget runs as a wave of one, and so does a file whose header does not
give its length (a FLAC stream with total_samples 0). Input order is kept, nothing is sorted by length. The lengths are read from the
files' headers before anything is put (``resident_samples``); files given as paths or file objects are read once, when the job starts.
The budget is a rule for closing waves, NOT the slot's footprint: the library allocates max_batch rows of the longest length (PCM, and
feature buffers sized with them) and keeps them — a one-hour file on max_batch 60 is about 13.8 GB of PCM rows alone, whatever its wave.

Per wave: every file is put into its own item by the route ``transcribe`` takes (``batched._put_audio``: FLAC and telephony WAV
decoded on the device, other files through ``put_frames``, a waveform through ``pcm_put``, the host fallback for refused shapes); ONE
gate pass covers the wave (``probs_pcm_many`` with the files' own counts — consecutive passes only around a file that failed or was
empty, and where the wave's audio passes the 3600 s one pass takes in all); the language is per file; the chunks are pooled in (file, start) order and decoded ``batch_size``
at a time, each item of a group with its own file's prompt (tokenizer of that file's language and task) and source item; word
timestamps are aligned for the whole group in one ``align`` call per start sequence (``wlx_align_batch``). A file is yielded when the
group of its last chunk has finished, files in input order.

Speakers. ``diarize=True`` (the pipeline's ``file_diarizer``, made from the configured speaker checkpoint when there is none), a
``FileDiarizer``, or a list with one of those or False per file; ``max_speakers`` an int or a list (None: the diarizer's own cap). The
sources of a wave are still resident when its last decode group has finished, and only then are all its transcripts known: so with
``diarize`` on, the files of a wave are yielded TOGETHER, in input order, after the wave's last group, behind ONE
``FileDiarizer.diarize_many`` job per diarizer over ``merge_spans(segments)`` of every file (wlx_spk_diarize_many: the windows of all
files share the embed passes, the files are clustered side by side, one wait). Every segment and word of a diarized file gets
``.speaker`` by ``file_diarization.label_segments`` (``assign_speakers`` with the gaps closed, as the REST route answers), and its
``info`` gets ``.speakers``, the speakers in order of first appearance. A failed file still yields (index, exception, None).

Language. A file with ``language=None`` on a multilingual model is detected on its own leading chunks, as ``_language`` does, and the
window the detection encodes is the one ``_language`` builds — the leading chunks' features glued, plus its dummy frame — so that the
probabilities are the single-file run's. No device entry point glues features, so the leading chunks of all files of the wave are cut
in shared ``logmel_chunks`` launches, their features glued on the host, and the windows of all files are encoded as ONE batch and
read by ONE batched ``detect_language``. ``language_detection_segments > 1`` keeps the per-file path of ``_language`` (its vote
stops early, window by window); ``multilingual=True`` (a language per chunk) decodes as in ``generate_segment_batched``, over the group.

Errors. A damaged or unreadable file (ValueError from the readers, WLX_ERR_DATA from the device decoders, OSError from a path) costs
that file only: it yields (index, exception, None) and the wave goes on without it; ``on_error="raise"`` raises there instead. So does
a file every route refuses (WLX_ERR_ARG, nothing launched: more than the 3600 s one item holds), as a ValueError. Any
other device error is raised as ``transcribe`` raises it. A file without speech yields [] and an info with duration_after_vad == 0.

``multichannel=True`` is not part of this route. After a job nothing is left for ``resident_file_audio``: item 0 is a destination of
the decode groups, and the sources are overwritten by the next wave. That is why the speakers are found INSIDE the job (``diarize``),
while the wave's sources still lie behind their items: a caller cannot diarize a pooled file afterwards.
"""
from __future__ import annotations

import contextlib
import inspect
import time
from typing import List, Optional, Sequence

import numpy as np

from . import biasing as _biasing
from . import grammar as _grammar
from . import vad as _vad
from . import word_timing as _wt
from .batched import MAX_DEC_ROWS, DeviceChunks, _collect_ranges, _file_bytes, _options, _put_audio, _put_audio_many, _segment, _vad_options
from ._lib import ERR_ARG as _ERR_ARG, WlxError as _WlxError
from .engine import FlacFrames, ResidentPcm, _at_16k, _wav_at_16k
from .file_diarization import FileDiarizer, label_segments, merge_spans, speakers_in_order
from .multichannel import source_rows_addressable
from .tokenizer import Tokenizer
from .transcriber import EncoderOutput, restore_speech_timestamps
from .types import TranscriptionInfo

WAVE_PCM_BUDGET = 4 << 30            # bytes of resident PCM rows one wave may ask of the slot: (files + batch_size) x longest x 4
GATE_MAX_SAMPLES = 3600 * 16000      # what one wlx_vad_probs_pcm_batch pass takes in all (include/wlx.h)
PER_FILE = ("language", "initial_prompt", "hotwords", "prefix", "clip_timestamps")      # keywords that may be a list, one entry per file


def check_batch(batch_size: int, max_batch: int):
    """the files of a wave stay resident behind the decode group's destination items: at least one item must be left for them"""
    if batch_size > max_batch - 1:
        raise ValueError(f"many files: batch_size {batch_size} exceeds max_batch {max_batch} - 1 file = {max_batch - 1} (the job's files "
                         f"stay resident in the slot's items behind the decode group): create the model with max_batch >= "
                         f"{batch_size + 1} or lower batch_size")


def next_wave(lengths: Sequence[Optional[int]], start: int, batch_size: int, max_batch: int, budget: int = WAVE_PCM_BUDGET,
              stride: int = 0) -> List[int]:
    """the wave that starts at file `start`: consecutive file indices (module docstring). lengths: samples at 16 kHz per file, None
    where the header does not say — such a file runs as a wave of one, since neither rule can be checked for it. stride: the longest
    audio the slot has been asked to hold so far (Slot.pcm_longest): its rows are never shorter than that, whatever this wave holds,
    so the reach of the chunk gather is checked against max(stride, the wave's longest)."""
    room = max_batch - batch_size
    cur: List[int] = []
    longest = 0
    for i in range(start, len(lengths)):
        n = lengths[i]
        if n is None:
            return cur or [i]
        grown = max(longest, max(0, int(n)))
        if cur and (len(cur) >= room or (len(cur) + 1 + batch_size) * grown * 4 > budget
                    or not source_rows_addressable(len(cur) + 1, max(grown, stride))):
            break
        cur.append(i)
        longest = grown
    return cur


def plan_waves(lengths: Sequence[Optional[int]], batch_size: int, max_batch: int, budget: int = WAVE_PCM_BUDGET,
               stride: int = 0) -> List[List[int]]:
    """every wave of a job on a slot whose rows are `stride` samples long when it starts: `next_wave` again and again, the stride
    growing to the longest file of the waves before (the job itself sizes each wave from Slot.pcm_longest when it gets there, which
    also knows the files whose header gave no length)"""
    check_batch(batch_size, max_batch)
    waves: List[List[int]] = []
    at = 0
    while at < len(lengths):
        wave = next_wave(lengths, at, batch_size, max_batch, budget, stride)
        waves.append(wave)
        stride = max([stride] + [int(lengths[i]) for i in wave if lengths[i] is not None])
        at = wave[-1] + 1
    return waves


def resident_samples(audio) -> Optional[int]:
    """the samples at 16 kHz a waveform or the bytes of a file will occupy, from the header alone (an upper estimate for ADPCM);
    None where the header does not say (a FLAC stream whose encoder left total_samples 0, a container that is neither): the file then
    runs as a wave of its own, and the put says what is wrong with it, if anything"""
    if isinstance(audio, np.ndarray):
        return int(audio.shape[0])
    if audio[:4] == b"fLaC":
        frames = FlacFrames(audio)
        return _at_16k(frames.total_samples, frames.sample_rate) or None
    if audio[:4] == b"RIFF":
        return _wav_at_16k(audio) or None
    return None


def per_file_arguments(a: dict, n_files: int) -> List[dict]:
    """transcribe's arguments by name -> one dict per file: a keyword of PER_FILE given as a list with one entry per file is taken
    apart (a wrong length is a ValueError); everything else is the same for every file. `initial_prompt` is a list of token ids when
    every entry is an int, `clip_timestamps` a list of clips when any entry is a dict: those are one value, for every file."""
    split = {}
    for name in PER_FILE:
        v = a[name]
        if not isinstance(v, (list, tuple)):
            continue
        if name == "initial_prompt" and v and all(isinstance(t, (int, np.integer)) for t in v):
            continue
        if name == "clip_timestamps" and any(isinstance(c, dict) for c in v):
            continue
        if name == "clip_timestamps" and not v:
            continue
        if len(v) != n_files:
            raise ValueError(f"{name}: a list of {len(v)} entries for {n_files} files (one entry per file, or one value for all)")
        split[name] = list(v)
    return [{**a, **{name: v[i] for name, v in split.items()}} for i in range(n_files)]


BIAS_KEYWORDS = ("keywords", "keywords_boost", "logit_bias")     # job keywords of keyword boosting; each may be a list, one entry per file


def per_file_tables(model, bias_args: dict, n_files: int) -> list:
    """the job's `keywords` / `keywords_boost` / `logit_bias` -> per file a biasing.CompactTable, None (nothing to add) or the
    ValueError its table was refused with (the cap named). `keywords`: a list of strings is ONE list for every file; a list with one
    entry per file, each None or a list of phrases, is per file. `keywords_boost`: a number or a list of numbers (or None) per file;
    `logit_bias`: a dict or a list of dicts (or None) per file. Equal lists share one table object."""
    kw, boost, lb = (bias_args.get(name) for name in BIAS_KEYWORDS)
    if kw is None and lb is None:
        if boost is not None:
            raise ValueError("keywords_boost needs keywords")
        return [None] * n_files

    def spread(v, what, per_file):
        if per_file:
            if len(v) != n_files:
                raise ValueError(f"{what}: a list of {len(v)} entries for {n_files} files (one entry per file, or one value for all)")
            return list(v)
        return [v] * n_files
    is_list = lambda k: isinstance(k, (list, tuple))
    token_list = lambda k: is_list(k) and len(k) > 0 and all(isinstance(t, (int, np.integer)) for t in k)
    # per file: every entry is None or a list of phrases (a list whose entries are all token lists is ONE list of phrases)
    kws = spread(kw, "keywords", is_list(kw) and len(kw) > 0 and all(k is None or is_list(k) for k in kw) and not all(token_list(k) for k in kw))
    boosts = spread(boost, "keywords_boost", isinstance(boost, (list, tuple)))
    lbs = spread(lb, "logit_bias", isinstance(lb, (list, tuple)))
    if not hasattr(model, "compile_keywords"):
        raise ValueError("keywords: this transcriber does not bias")
    out, seen = [], {}
    for k, b, l in zip(kws, boosts, lbs):
        if k is None and l is None:
            out.append(None)
            continue
        key = repr((k, b, sorted(l.items()) if isinstance(l, dict) else l))
        if key not in seen:
            try:
                t = model.compile_keywords(k, b, l, compact=True)
                seen[key] = None if t.empty else t
            except ValueError as e:
                seen[key] = e
        out.append(seen[key])
    return out


def fit_tables(wave: List[int], tables: list):
    """the longest head of `wave` whose distinct tables fit one biasing.BiasSet (at least one file: a single table always fits, its
    own caps were checked when it was compiled), and that set (None: no file of it has a table)"""
    bias_set = _biasing.BiasSet()
    for k, i in enumerate(wave):
        t = tables[i]
        if t is None or isinstance(t, Exception):
            continue
        if k and not bias_set.fits(t):
            wave = wave[:k]
            break
        bias_set.add(t)
    return wave, (bias_set if len(bias_set) else None)


def per_file_diarizers(pipe, diarize, max_speakers, n_files: int) -> List[tuple]:
    """the `diarize` / `max_speakers` arguments -> one (FileDiarizer or None, cap or None) per file. `diarize`: False | True |
    FileDiarizer, or a list with one of those per file; True is the pipeline's `file_diarizer` (made once from the configured speaker
    checkpoint). `max_speakers`: None (the diarizer's own), an int, or a list with one of those per file."""
    def spread(v, what):
        if isinstance(v, (list, tuple)):
            if len(v) != n_files:
                raise ValueError(f"{what}: a list of {len(v)} entries for {n_files} files (one entry per file, or one value for all)")
            return list(v)
        return [v] * n_files
    caps = spread(max_speakers, "max_speakers")
    for c in caps:
        if c is not None and (isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0):
            raise ValueError(f"max_speakers {c!r}: 0 (no cap), a positive integer or None")
    out = []
    for d, c in zip(spread(diarize, "diarize"), caps):
        if d is True:
            d = _pipeline_diarizer(pipe)
        elif d is False or d is None:
            d = None
        elif not hasattr(d, "diarize"):
            raise ValueError(f"diarize {d!r}: False, True or a FileDiarizer")
        out.append((d, None if c is None else int(c)))
    return out


def _pipeline_diarizer(pipe):
    """`diarize=True`: the pipeline's own FileDiarizer, on the shared embedder of the configured speaker checkpoint"""
    d = getattr(pipe, "file_diarizer", None)
    if d is None:
        from .artifacts import resolve_diarization_model
        from .diarization import shared_embedder
        path = resolve_diarization_model(None)
        if path is None:
            raise ValueError("diarize=True: no speaker checkpoint is configured (set pipe.file_diarizer, or pass a FileDiarizer)")
        d = pipe.file_diarizer = FileDiarizer(shared_embedder(path, int(getattr(pipe.model, "device_index", 0) or 0)))
    return d


class _File:
    """one file of a wave, from its put to its result"""

    def __init__(self, index: int, a: dict, audio, item: int, diarizer=None, max_speakers: Optional[int] = None):
        self.index, self.a, self.audio, self.item = index, a, audio, item
        self.diarizer, self.max_speakers = diarizer, max_speakers
        self.error = None
        self.n_samples = 0
        self.clips: List[dict] = []
        self.from_vad = False
        self.ranges: list = []
        self.meta: list = []
        self.tokenizer = self.options = self.info = self.prompt = None
        self.language = (None, None, None)
        self.segments: list = []
        self.left = 0                       # chunks not decoded yet
        self.table = None                   # the file's keyword table (biasing.CompactTable) and the set of its wave's tables
        self.bias_set = None
        self.last_speech = 0.0


def transcribe_many(pipe, audios, *, batch_size: int = 8, on_error: str = "return", **kwargs) -> list:      # (wave_put rides in kwargs)
    out: list = [None] * len(audios)
    for index, segments, info in iter_many(pipe, audios, batch_size=batch_size, on_error=on_error, **kwargs):
        out[index] = (segments, info)
    return out


def iter_many(pipe, audios, *, batch_size: int = 8, on_error: str = "return", **kwargs):
    """-> generator of (index, segments: List[Segment], info) — or (index, exception, None) — file by file as the groups finish, in
    input order. `audios`: a sequence of what `transcribe` takes; kwargs: every keyword of `_transcribe`, those of PER_FILE also as a
    list with one entry per file. The arguments are checked here, before the first file is read (module docstring).
    Each job leaves `pipe.many_timing` = {"front_s": seconds its waves spent before their first decode (puts, gate, language),
    "total_s": seconds up to the end of the last wave finished, "waves": waves finished} — what scripts/many_files_time.py reports;
    the next job on the pipeline replaces it.
    wave_put=True: the files of a wave go up in ONE Slot.put_many call (one wait) instead of one put per file; a slot without put_many
    keeps the per-file puts. Results are the same either way; the default stays per-file puts."""
    if on_error not in ("return", "raise"):
        raise ValueError(f"on_error {on_error!r}: 'return' or 'raise'")
    wave_put = bool(kwargs.pop("wave_put", False))
    bias_args = {name: kwargs.pop(name, None) for name in BIAS_KEYWORDS}
    grammar, grammar_repeat = kwargs.pop("grammar", None), kwargs.pop("grammar_repeat", True)
    diarize, max_speakers = kwargs.pop("diarize", False), kwargs.pop("max_speakers", None)
    if kwargs.pop("multichannel", False):
        raise ValueError("transcribe_many: multichannel=True is not part of this route (transcribe the files one by one with "
                         "transcribe(..., multichannel=True))")
    if isinstance(audios, (str, bytes, bytearray, np.ndarray)) or hasattr(audios, "read"):
        raise TypeError("transcribe_many takes a sequence of files or waveforms; one file goes to transcribe")
    audios = list(audios)
    bound = inspect.signature(pipe._transcribe).bind(None, batch_size=batch_size, **kwargs)
    bound.apply_defaults()
    a = dict(bound.arguments)
    model = pipe.model
    if a["multilingual"] and not model.model.is_multilingual:
        model.logger.warning("The current model is English-only but the multilingual parameter is set to"
                             "True; setting to False instead.")
        a["multilingual"] = False
    batch_size, beam_size = int(a["batch_size"]), int(a["beam_size"])
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}: at least one chunk per decode")
    if batch_size * beam_size > MAX_DEC_ROWS:
        raise ValueError(f"batch_size {batch_size} x beam_size {beam_size} = {batch_size * beam_size} decoder rows: "
                         f"one decode step holds at most {MAX_DEC_ROWS}")
    max_batch = int(getattr(model, "max_batch", batch_size))
    check_batch(batch_size, max_batch)
    per_file = per_file_arguments(a, len(audios))
    diarizers = per_file_diarizers(pipe, diarize, max_speakers, len(audios))
    tables = per_file_tables(pipe.model, bias_args, len(audios))        # compiled here, before any audio work
    job = _job(pipe, audios, per_file, a, batch_size, max_batch, on_error, wave_put, diarizers, tables)
    if grammar is None:
        return job
    # ONE grammar for all files (a grammar per file is not served: one grammar serves a whole decode group, and groups mix files)
    if any(t is not None for t in tables):
        raise ValueError("grammar and keywords / logit_bias in one job: a slot decodes under one of them")
    if not hasattr(pipe.model, "compile_grammar"):
        raise ValueError("grammar: this transcriber takes no grammar")
    return _under_grammar(job, pipe.model.compile_grammar(grammar, grammar_repeat))


def _under_grammar(job, gram):
    """`job`, every step of it taken under the calling thread's grammar scope (left again before the file is handed out)"""
    it = iter(job)
    while True:
        with _grammar.scope(gram):
            try:
                item = next(it)
            except StopIteration:
                return
        yield item


def _job(pipe, audios, per_file, a, batch_size, max_batch, on_error, wave_put: bool = False, diarizers=None, tables=None):
    model = pipe.model
    tables = tables if tables is not None else [None] * len(audios)
    if on_error == "raise":
        for t in tables:
            if isinstance(t, Exception):
                raise t
    timing = pipe.many_timing = {"front_s": 0.0, "total_s": 0.0, "waves": 0}
    t_job = time.perf_counter()
    loaded, lengths = [], []
    for audio in audios:                    # paths and file objects are read once; a file that cannot be read fails at its turn
        if not isinstance(audio, np.ndarray):
            try:
                audio = _file_bytes(audio)
            except OSError as e:
                audio = e
        loaded.append(audio)
        lengths.append(0 if isinstance(audio, Exception) else resident_samples(audio))       # (a file that was not read is never put)
    slot = model._slot(rows=int(a["beam_size"]))
    if model.feature_extractor.sampling_rate != 16000 or not all(hasattr(slot, m) for m in ("logmel_chunks", "pcm_put", "pcm")):
        raise ValueError("transcribe_many needs the device front end (Slot.logmel_chunks), which this engine lacks")
    vad_parameters = a["vad_parameters"]
    if a["vad_filter"]:
        vad_parameters = _vad_options(vad_parameters, a["chunk_length"] or model.feature_extractor.chunk_length)
    at = 0
    while at < len(audios):
        # sized when the job gets there: the slot's rows are as long as the longest audio it was ever asked to hold — by an earlier wave,
        # an earlier job or another route on this thread's slot — and the chunk gather's reach is measured in rows of THAT length
        wave = next_wave(lengths, at, batch_size, max_batch, stride=int(getattr(slot, "pcm_longest", 0)))
        wave, bias_set = fit_tables(wave, tables)       # (a wave closes early where its distinct tables would overflow a pool cap)
        at = wave[-1] + 1
        files = [_File(i, per_file[i], loaded[i], batch_size + k, *(diarizers[i] if diarizers else ())) for k, i in enumerate(wave)]
        for f in files:
            if isinstance(tables[f.index], Exception):
                f.audio = tables[f.index]               # a refused table costs only its file: it fails at its turn, like a file not read
            else:
                f.table = tables[f.index]
            f.bias_set = bias_set
        for i in wave:
            loaded[i] = None                # (the job does not hold a file's bytes past its wave)
        yield from _wave(pipe, slot, files, a, vad_parameters, batch_size, on_error, timing, wave_put)
        timing["waves"] += 1
        timing["total_s"] = time.perf_counter() - t_job


def _wave(pipe, slot, files: List[_File], a, vad_parameters, batch_size, on_error, timing, wave_put: bool = False):
    model = pipe.model
    sampling_rate = model.feature_extractor.sampling_rate
    t0 = time.perf_counter()
    if hasattr(model, "_tls"):
        model._tls.file_audio = None          # (what an earlier call of this thread left resident is about to be overwritten)
    # ---- every file into its own item: one by one, or (wave_put, on a slot that has put_many) the wave in one call with one wait
    put = None
    if wave_put and hasattr(slot, "put_many"):
        put = _put_audio_many(model, slot, [f.audio for f in files], [f.item for f in files])
    for k, f in enumerate(files):
        try:
            if isinstance(f.audio, Exception):
                raise f.audio
            if put is not None and isinstance(put[k], Exception):
                raise put[k]
            f.n_samples, _host, _device = put[k] if put is not None else _put_audio(model, slot, f.audio, f.item)
        except (ValueError, OSError, _WlxError) as e:
            if isinstance(e, _WlxError):
                # a refusal (nothing was launched: the file is longer than the 3600 s an item holds) is this file's error; any other
                # device error is raised as transcribe raises it
                if getattr(e, "code", None) != _ERR_ARG:
                    raise
                e = ValueError(f"the device front end refused the audio: {e}")
            if on_error == "raise":
                raise e
            f.error = e
        f.audio = None
    good = [f for f in files if f.error is None]

    # ---- clips: explicit, one gate pass over the wave, or the whole of a short file
    chunk_length = a["chunk_length"] or model.feature_extractor.chunk_length
    gated = []
    for f in good:
        if f.a["clip_timestamps"]:
            f.clips = [dict(c) for c in f.a["clip_timestamps"]]
        elif a["vad_filter"]:
            gated.append(f)
            f.from_vad = True
        elif f.n_samples / sampling_rate < chunk_length:
            f.clips = [{"start": 0, "end": f.n_samples}]
        else:
            raise RuntimeError("No clip timestamps found. "
                               "Set 'vad_filter' to True or provide 'clip_timestamps'.")
    if gated:
        _gate(model, slot, gated, vad_parameters, sampling_rate)
    for f in good:
        f.clips = [c for c in f.clips if c["end"] > c["start"]]
        f.ranges, f.meta = _collect_ranges(f.clips, sampling_rate, chunk_length) if f.clips else ([], [])
        f.left = len(f.ranges)

    # ---- language, tokenizer, options, info: per file
    _languages(pipe, slot, good, a, batch_size)
    for f in good:
        language, probability, all_probs = f.language
        f.tokenizer = Tokenizer(model.hf_tokenizer, model.model.is_multilingual, task=f.a["task"], language=language)
        f.options = _options(f.tokenizer, f.a, f.clips)
        f.info = TranscriptionInfo(language=language, language_probability=probability, duration=f.n_samples / sampling_rate,
                                   duration_after_vad=sum(c["end"] - c["start"] for c in f.clips) / sampling_rate,
                                   transcription_options=f.options, vad_options=vad_parameters if f.from_vad else f.a["vad_parameters"],
                                   all_language_probs=all_probs)
    timing["front_s"] += time.perf_counter() - t0

    # ---- the chunks of all files pooled in (file, start) order, batch_size per decode; a file leaves when its last chunk is done
    pool = [(f, c) for f in good for c in range(len(f.ranges))]
    order = iter(files)
    pending = next(order, None)

    held = any(f.diarizer is not None for f in files)          # speakers: the wave leaves together, behind its last group

    def finished(last: bool = False):
        nonlocal pending
        if held and not last:
            return
        if held:
            _speakers(slot, good)
        while pending is not None and (pending.error is not None or pending.left == 0):
            f, pending = pending, next(order, None)
            yield (f.index, f.error, None) if f.error is not None else (f.index, f.segments, f.info)

    yield from finished(last=not pool)
    for g in range(0, len(pool), batch_size):
        group = pool[g:g + batch_size]
        with slot.lock:
            results = _decode_group(pipe, slot, group)
        for (f, _c), result in zip(group, results):
            for segment in result:
                seg = _segment(segment, f.options, len(f.segments) + 1)
                if f.from_vad:
                    seg = restore_speech_timestamps([seg], f.clips, sampling_rate)[0]
                f.segments.append(seg)
            f.left -= 1
        if a["log_progress"]:
            model.logger.info("batched transcription: %d / %d chunks of the wave", min(g + batch_size, len(pool)), len(pool))
        yield from finished(last=g + batch_size >= len(pool))


def _speakers(slot, files: List[_File]):
    """the speakers of a wave whose transcripts are complete and whose sources are still resident behind their items: one
    FileDiarizer.diarize_many job per diarizer, then `.speaker` on every segment and word and `.speakers` on the info"""
    by_diarizer: dict = {}
    for f in files:
        if f.diarizer is not None:
            by_diarizer.setdefault(id(f.diarizer), []).append(f)
    for group in by_diarizer.values():
        diarizer = group[0].diarizer
        residents = [ResidentPcm(slot, f.item, f.n_samples) for f in group]
        spans = [merge_spans(f.segments) for f in group]
        many = getattr(diarizer, "diarize_many", None)
        if many is not None:
            turns = many(residents, spans, max_speakers=[f.max_speakers for f in group])
        else:          # anything with `diarize` alone: file by file
            turns = [diarizer.diarize(r, s) for r, s in zip(residents, spans)]
        for f, file_turns in zip(group, turns):
            per_seg, per_word = label_segments(f.segments, file_turns)
            for seg, who, words in zip(f.segments, per_seg, per_word):
                seg.speaker = who
                for word, w in zip(seg.words or [], words or []):
                    word.speaker = w
            f.info.speakers = speakers_in_order(file_turns)


def _gate(model, slot, gated: List[_File], vad_parameters, sampling_rate):
    """the speech clips of every gated file: one pass of the network over neighbouring items (a new pass starts behind a file that is
    not gated — failed, empty, given explicit clips — and where one pass would take more than GATE_MAX_SAMPLES in all)"""
    vad_model = model._vad_model()
    on_device = hasattr(vad_model, "probs_pcm_many") and getattr(vad_model, "device", None) == getattr(slot.engine, "device", -1)
    runs: List[List[_File]] = []
    for f in gated:
        if not on_device or f.n_samples <= 0:
            with slot.lock:          # no device gate, or nothing to read: the host statement, on this file alone
                wave = slot.pcm(f.item) if f.n_samples > 0 else np.zeros(0, np.float32)
            f.clips = _vad.get_speech_timestamps(wave, vad_parameters, sampling_rate, model=vad_model)
            continue
        run = runs[-1] if runs else None
        if run is None or run[-1].item + 1 != f.item or sum(x.n_samples for x in run) + f.n_samples > GATE_MAX_SAMPLES:
            runs.append([f])
        else:
            run.append(f)
    for run in runs:
        with slot.lock:
            probs = vad_model.probs_pcm_many(slot, [f.n_samples for f in run], first_item=run[0].item)
        for f, p in zip(run, probs):
            f.clips = _vad.speech_segments_from_probs_native(p, f.n_samples, vad_parameters, sampling_rate)


def _languages(pipe, slot, files: List[_File], a, batch_size):
    """f.language = (language, probability, all probabilities or None) for every file: the one given, or detected on the file's own
    leading chunks — the windows of all files that need it encoded as one batch (module docstring)"""
    model = pipe.model
    segments, threshold = a["language_detection_segments"], a["language_detection_threshold"]
    detect = []
    for f in files:
        if f.a["language"] is not None or not model.model.is_multilingual:
            f.language = pipe._language(None, f.a["language"], segments, threshold)
        elif segments != 1:
            lead = DeviceChunks(slot, f.ranges, slot.pcm, [f.item] * len(f.ranges), f.n_samples)
            f.language = pipe._language(lead, None, segments, threshold, group_size=batch_size)
        else:
            detect.append(f)
    if not detect:
        return
    need = model.feature_extractor.nb_max_frames
    # the leading chunks _language would read, known from the ranges alone: a chunk of n samples has (n + 160) // 160 frames, the last
    # of which (the pad frame) is cut off
    lead = []
    for f in detect:
        have = 0
        for c, rg in enumerate(f.ranges):
            if have >= need:
                break
            lead.append((f, c))
            have += (sum(e - s for s, e in rg) + 160) // 160 - 1
    parts = {id(f): [] for f in detect}
    with slot.lock:
        for g in range(0, len(lead), batch_size):
            group = lead[g:g + batch_size]
            DeviceChunks(slot, [f.ranges[c] for f, c in group], slot.pcm, [f.item for f, _ in group]).to_device()
            for i, (f, _c) in enumerate(group):
                parts[id(f)].append(slot.features(i)[..., :-1])
        dummy = np.full((model.model.n_mels, 1), -1.5, dtype="float32")       # (_language: a dummy feature to account for empty audio)
        windows = [np.concatenate(parts[id(f)] + [dummy], axis=1)[:, :need] for f in detect]
        for g in range(0, len(detect), batch_size):
            group = detect[g:g + batch_size]
            for i, w in enumerate(windows[g:g + batch_size]):
                slot.set_features(w, item=i)
            slot.encode(len(group), seek=[0] * len(group), seg=[w.shape[1] for w in windows[g:g + batch_size]])
            slot._enc_generation += 1
            results = model.model.detect_language(EncoderOutput(slot, len(group), slot._enc_generation))
            for f, res in zip(group, results):
                all_probs = [(token[2:-2], p) for token, p in res]
                f.language = (all_probs[0][0], all_probs[0][1], all_probs)
                model.logger.info("Detected language '%s' with probability %.2f", all_probs[0][0], all_probs[0][1])


def _prompt(pipe, f: _File) -> List[int]:
    if f.prompt is None:
        o = f.options
        f.prompt = pipe.model.get_prompt(
            f.tokenizer, previous_tokens=(f.tokenizer.encode(o.initial_prompt) if o.initial_prompt is not None else []),
            without_timestamps=o.without_timestamps, hotwords=o.hotwords)
    return f.prompt


def _decode_group(pipe, slot, group) -> list:
    """`forward` for a group whose chunks come from different files: (file, chunk index) per item -> per item the sub-segment dicts
    on that file's concatenated timeline. One log-mel cut, one encode; one generate per distinct length limit (one, unless
    `max_new_tokens` meets prompts of different lengths); with word timestamps one align call per distinct start sequence."""
    model = pipe.model
    n = len(group)
    chunks = DeviceChunks(slot, [f.ranges[c] for f, c in group], slot.pcm, [f.item for f, _ in group])
    frames = chunks.to_device()
    slot.encode(n, seek=[0] * n, seg=[min(t - 1, 3000) for t in frames])
    slot._enc_generation += 1
    encoder_output = EncoderOutput(slot, n, slot._enc_generation)

    prompts, limits = [], []
    for f, _c in group:
        prompt = _prompt(pipe, f)
        o = f.options
        max_length = len(prompt) + o.max_new_tokens if o.max_new_tokens is not None else model.max_length
        if max_length > model.max_length:
            raise ValueError(
                f"The length of the prompt is {len(prompt)}, and the `max_new_tokens` "
                f"{max_length - len(prompt)}. Thus, the combined length of the prompt "
                f"and `max_new_tokens` is: {max_length}. This exceeds the "
                f"`max_length` of the Whisper model: {model.max_length}. "
                "You should either reduce the length of your prompt, or "
                "reduce the value of `max_new_tokens`, "
                f"so that their combined length is less that {model.max_length}.")
        prompts.append(prompt.copy())
        limits.append(max_length)
    if group[0][0].options.multilingual:          # a language per chunk, as generate_segment_batched detects it
        detected = model.model.detect_language(encoder_output)
        for i, (f, _c) in enumerate(group):
            prompts[i][prompts[i].index(f.tokenizer.language)] = f.tokenizer.tokenizer.token_to_id(detected[i][0][0])

    outputs = [None] * n
    for limit in sorted(set(limits)):
        idx = [i for i in range(n) if limits[i] == limit]
        o = group[idx[0]][0].options               # (what a generate call takes from the options is the same for every file of a job)
        # keyword boosting per file: the decode runs under an item_scope of the tables of the files ITS items come from (a subset
        # carries its own), all of them in the wave's one set; a job without tables decodes as it always did
        biased = group[idx[0]][0].bias_set is not None      # (a group without a table in a wave that has some: every item deselected, the set stays)
        scope = _biasing.item_scope([group[i][0].table for i in idx], group[idx[0]][0].bias_set) if biased else contextlib.nullcontext()
        with scope:
            results = model.model.generate(
                encoder_output if len(idx) == n else encoder_output.select(idx), [prompts[i] for i in idx], beam_size=o.beam_size,
                patience=o.patience, length_penalty=o.length_penalty, max_length=limit, suppress_blank=o.suppress_blank,
                suppress_tokens=o.suppress_tokens, return_scores=True, return_no_speech_prob=True,
                sampling_temperature=o.temperatures[0], repetition_penalty=o.repetition_penalty,
                no_repeat_ngram_size=o.no_repeat_ngram_size)
        for i, result in zip(idx, results):
            seq_len = len(result.sequences_ids[0])
            cum_logprob = result.scores[0] * (seq_len ** o.length_penalty)
            outputs[i] = dict(avg_logprob=cum_logprob / (seq_len + 1), no_speech_prob=result.no_speech_prob,
                              tokens=result.sequences_ids[0])

    segmented, sizes = [], []
    for (f, c), output in zip(group, outputs):
        subsegments, size = pipe._subsegments(f.tokenizer, f.meta[c], output)
        segmented.append(subsegments)
        sizes.append(size)
    if group[0][0].options.word_timestamps:
        _word_timestamps(pipe, group, encoder_output, segmented, sizes)
    return segmented


def _word_timestamps(pipe, group, encoder_output, segmented, sizes):
    """add_word_timestamps per run of chunks of one file (its tokenizer, its last-speech time), on alignments that were computed for the
    WHOLE group first: every chunk that has text, whatever its file, in one align call per distinct start sequence"""
    model = pipe.model
    texts = [[t for sub in window for t in sub["tokens"] if t < f.tokenizer.eot] for (f, _c), window in zip(group, segmented)]
    aligned = {}
    by_start = {}
    for i, ((f, _c), flat) in enumerate(zip(group, texts)):
        if flat:
            by_start.setdefault(tuple(f.tokenizer.sot_sequence), []).append(i)
    for start, idx in by_start.items():
        res = model.model.align(encoder_output.select(idx), list(start), [texts[i] for i in idx], [sizes[i] for i in idx])
        for i, r in zip(idx, res):
            aligned[i] = _wt.unpack_alignment(r)
    end = 0
    while end < len(group):
        base = end
        f = group[base][0]
        while end < len(group) and group[end][0] is f:
            end += 1

        def align_fn(text_tokens, _num_frames, window, base=base):
            return aligned[base + window]

        align_fn.align_many = lambda requests, base=base: [aligned[base + r[2]] for r in requests]
        o = f.options
        got = _wt.add_word_timestamps(segmented[base:end], f.tokenizer, align_fn, 0, model.tokens_per_second, model.frames_per_second,
                                      o.prepend_punctuations, o.append_punctuations, f.last_speech)
        if got is not None:
            f.last_speech = got
