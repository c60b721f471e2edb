"""BatchedInferencePipeline — batched long-form transcription on the MI355X engine.

The duck type of ``BatchedInferencePipeline`` in whisper_live/transcriber/transcriber_faster_whisper.py:113-571: the audio is
cut into speech chunks of at most ``chunk_length`` seconds, ``batch_size`` chunks are decoded per step — each on its own, with no
conditioning on previous text — and the segments are put back on the file's timeline. Host logic restated statement for statement
from those lines; where the reference delegates to un-vendored ``faster_whisper.vad`` the project's own statements hold
(``vad.get_speech_timestamps``, ``vad.collect_chunks(..., max_duration=chunk_length)``), and times of VAD chunks are mapped back
with ``restore_speech_timestamps`` as ``WhisperModelHIP.transcribe`` does (the reference's literal text does not restore them).

Device route (a real engine): the audio becomes resident ONCE in item 0 of the calling thread's slot (``put_frames`` for a file,
``pcm_put`` for a waveform), the gate reads it there (``wlx_vad_probs_pcm``), and per group of ``batch_size`` chunks one sequence
runs: ``wlx_logmel_chunks`` (one launch of each log-mel kernel cuts the group's chunks out of the resident PCM into the slot's
feature items), ``encode``, optionally ``detect_language``, ``generate``. An engine whose slots lack those methods (the host-logic
test doubles) takes the host-chunk route: ``collect_chunks`` + one feature-extractor call per chunk, as the reference does.

One plan, two routes. ``_plan`` is the procedure of a file transcription written once — batch checks, slot, clips (explicit, gate or
short file), chunks pooled in order (channel, start), ``DeviceChunks``, language, tokenizer, options, info — over a ``Resident``
description of the audio; a mono file is a file with one channel whose source is item 0. The mono route (``_transcribe``) keeps what
is its own: ``_resident_mono`` (the host routes, the down-mix, the lazy host copy, the gate on item 0), segments yielded as groups
finish with running ids, ``last_speech_timestamp`` on the pipeline. The multichannel route's own is in multichannel.py. Both decode
through ``_groups`` and build their segments with ``_segment``.
"""
from __future__ import annotations

import inspect
from contextlib import nullcontext
from math import ceil
from typing import BinaryIO, Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import vad as _vad
from . import word_timing as _wt
from ._lib import ERR_ARG as _ERR_ARG, ERR_DATA as _ERR_DATA, LM_MAXRANGES as _MAXRANGES, WlxError as _WlxError
from .engine import ResidentPcm
from .multichannel import language_channel, pool_chunks
from .tokenizer import Tokenizer
from .transcriber import EncoderOutput, get_compression_ratio, get_suppressed_tokens, pad_or_trim, restore_speech_timestamps
from .types import Segment, TranscriptionInfo, TranscriptionOptions, Word
from .vad import VadOptions

MAX_DEC_ROWS = 320          # decoder rows of one step (include/wlx.h wlx_slot_create)


class DeviceChunks:
    """The `features` of the device route: the chunks of one file as sample ranges of PCM resident in items of `slot`, one source item
    per chunk. Nothing is computed until a group is decoded (`generate_segment_batched`); slicing gives the group.
    `src_item`: an int — every chunk reads that item (the mono route: a group goes out through wlx_logmel_chunks, and a chunk that
    falls back may land in the source and evict it) — or a list with one item per chunk (multichannel: the chunks of several channels
    pooled into one list; a group goes out through wlx_logmel_chunks_multi, and the sources lie behind every group's destination
    items, so nothing a group does evicts one). `host_audio(item)` returns the 16 kHz host copy of a source — fetched from the device
    only when something on the host needs it (a chunk that falls back)."""

    def __init__(self, slot, ranges: List[List[Tuple[int, int]]], host_audio, src_item: Union[int, List[int]] = 0, n_resident: int = 0):
        self.slot, self.ranges, self._host, self.src_item, self.n_resident = slot, ranges, host_audio, src_item, n_resident
        self.shared = {"resident": True}        # one state for every slice: a fallback into the source item evicts the source
        self.channels = None                    # multichannel: the file channel of each chunk (sliced with the chunks)

    def __len__(self):
        return len(self.ranges)

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("DeviceChunks is cut into groups with slices")
        src = self.src_item[key] if isinstance(self.src_item, list) else self.src_item
        g = DeviceChunks(self.slot, self.ranges[key], self._host, src, self.n_resident)
        g.channels = self.channels[key] if self.channels is not None else None
        g.shared = self.shared
        return g

    @property
    def shape(self):
        return (len(self.ranges), self.slot.engine.spec.n_mels, 3000)

    def host_audio(self, item: int = 0) -> np.ndarray:
        if not callable(self._host):
            return self._host
        copies = self.shared.setdefault("host", {})
        if item not in copies:
            copies[item] = self._host(item)
        return copies[item]

    def to_device(self) -> List[int]:
        """The group's features into items 0 .. len - 1 of the slot -> frames per item (incl. the pad frame)."""
        slot, n = self.slot, len(self.ranges)
        one = not isinstance(self.src_item, list)
        src = [self.src_item] * n if one else self.src_item          # the source item of each chunk
        if not one and n > min(src):
            raise ValueError(f"a group of {n} chunks would overwrite source item {min(src)}")
        if not self.shared["resident"]:              # (only the one source of a mono file is ever evicted: the check above)
            slot.pcm_put(self.host_audio(src[0]), item=src[0])
            self.shared["resident"] = True
        frames = [0] * n
        ok = [len(r) <= _MAXRANGES for r in self.ranges]
        a = 0
        while a < n:                                 # runs of chunks the kernel takes: one launch of each kernel per run, whatever the mix of sources
            if not ok[a]:
                a += 1
                continue
            b = a
            while b < n and ok[b]:
                b += 1
            frames[a:b] = slot.logmel_chunks(self.ranges[a:b], src_item=self.src_item if one else src[a:b], first_item=a)
            a = b
        for i in range(n):                           # more ranges than the kernel's table holds: the host concatenation, this chunk alone
            if not ok[i]:
                audio = self.host_audio(src[i])
                frames[i] = slot.logmel(np.concatenate([audio[s:e] for s, e in self.ranges[i]]), item=i)
                if i in src:
                    self.shared["resident"] = False
        return frames


class BatchedInferencePipeline:
    def __init__(self, model):
        self.model = model
        self.last_speech_timestamp = 0.0

    # ---- (:121-174)
    def forward(self, features, tokenizer, chunks_metadata, options):
        # multichannel: the group carries the file channel of each of its chunks; the word-timestamp pass then runs per run of equal
        # channel, each with its own channel's last-speech time, kept in the state all groups of the file share (a group that
        # straddles a channel boundary aligns once per run)
        channels = getattr(features, "channels", None)
        encoder_output, outputs = self.generate_segment_batched(features, tokenizer, options)

        segmented_outputs = []
        segment_sizes = []
        for chunk_metadata, output in zip(chunks_metadata, outputs):
            subsegments, segment_size = self._subsegments(tokenizer, chunk_metadata, output)
            segment_sizes.append(segment_size)
            segmented_outputs.append(subsegments)
        if options.word_timestamps:
            # chunk after chunk (the route add_word_timestamps takes where it is not given a group form), with the last-speech time carried along
            def aligners(base):
                """the align functions for a list of windows that starts at window `base` of the group"""
                def align_fn(text_tokens, _num_frames, window):
                    window += base
                    return _wt.unpack_alignment(self.model.model.align(
                        encoder_output.select([window]), tokenizer.sot_sequence, [text_tokens], segment_sizes[window])[0])

                # ... or, where the model's align takes a group, every chunk that has text in ONE call (wlx_align_batch), as the reference does
                def align_many_fn(requests):
                    res = self.model.model.align(encoder_output.select([base + r[2] for r in requests]), tokenizer.sot_sequence,
                                                 [r[0] for r in requests], [segment_sizes[base + r[2]] for r in requests])
                    return [_wt.unpack_alignment(r) for r in res]

                # (handed over on the function, the form add_word_timestamps also takes: the call keeps the nine positional arguments a
                # stand-in for add_word_timestamps is written against)
                align_fn.align_many = align_many_fn
                return align_fn

            # a mono group is one run (channel None) whose last-speech time lives on the pipeline; a multichannel file keeps one per channel
            runs = channels if channels is not None else [None] * len(segmented_outputs)
            last = {None: self.last_speech_timestamp} if channels is None else features.shared.setdefault("last_speech", {})
            end = 0
            while end < len(runs):
                base = end
                while end < len(runs) and runs[end] == runs[base]:
                    end += 1
                got = _wt.add_word_timestamps(
                    segmented_outputs[base:end], tokenizer, aligners(base), 0, self.model.tokens_per_second,
                    self.model.frames_per_second, options.prepend_punctuations, options.append_punctuations, last.get(runs[base], 0.0))
                if got is not None:
                    last[runs[base]] = got
            if channels is None:
                self.last_speech_timestamp = last[None]
        return segmented_outputs

    def _subsegments(self, tokenizer, chunk_metadata, output):
        """one chunk's decode -> (its sub-segment dicts on the concatenated timeline, the chunk's size in frames)"""
        duration = chunk_metadata["end_time"] - chunk_metadata["start_time"]
        segment_size = int(ceil(duration) * self.model.frames_per_second)
        subsegments, seek, single_timestamp_ending = self.model._split_segments_by_timestamps(
            tokenizer=tokenizer, tokens=output["tokens"], time_offset=chunk_metadata["start_time"],
            segment_size=segment_size, segment_duration=duration, seek=0)
        return [
            dict(text=tokenizer.decode(subsegment["tokens"]), avg_logprob=output["avg_logprob"],
                 no_speech_prob=output["no_speech_prob"], tokens=subsegment["tokens"], start=subsegment["start"],
                 end=subsegment["end"], compression_ratio=get_compression_ratio(tokenizer.decode(subsegment["tokens"])),
                 seek=int(chunk_metadata["start_time"] * self.model.frames_per_second))
            for subsegment in subsegments], segment_size

    # ---- (:176-254)
    def generate_segment_batched(self, features, tokenizer, options):
        batch_size = features.shape[0]

        prompt = self.model.get_prompt(
            tokenizer,
            previous_tokens=(tokenizer.encode(options.initial_prompt) if options.initial_prompt is not None else []),
            without_timestamps=options.without_timestamps, hotwords=options.hotwords)

        if options.max_new_tokens is not None:
            max_length = len(prompt) + options.max_new_tokens
        else:
            max_length = self.model.max_length

        if max_length > self.model.max_length:
            raise ValueError(
                f"The length of the prompt is {len(prompt)}, and the `max_new_tokens` "
                f"{max_length - len(prompt)}. Thus, the combined length of the prompt "
                f"and `max_new_tokens` is: {max_length}. This exceeds the "
                f"`max_length` of the Whisper model: {self.model.max_length}. "
                "You should either reduce the length of your prompt, or "
                "reduce the value of `max_new_tokens`, "
                f"so that their combined length is less that {self.model.max_length}.")

        if isinstance(features, DeviceChunks):
            # feature_extractor(chunk)[..., :-1] padded to 3000, on the device: the pad frame stays out of the encoder's window
            slot = features.slot
            frames = features.to_device()
            slot.encode(batch_size, seek=[0] * batch_size, seg=[min(t - 1, 3000) for t in frames])
            slot._enc_generation += 1
            encoder_output = EncoderOutput(slot, batch_size, slot._enc_generation)
        else:
            encoder_output = self.model.encode(features)
        prompts = [prompt.copy() for _ in range(batch_size)]

        if options.multilingual:
            language_tokens = [tokenizer.tokenizer.token_to_id(segment_langs[0][0])
                               for segment_langs in self.model.model.detect_language(encoder_output)]
            language_token_index = prompt.index(tokenizer.language)

            for i, language_token in enumerate(language_tokens):
                prompts[i][language_token_index] = language_token

        results = self.model.model.generate(
            encoder_output, prompts, beam_size=options.beam_size, patience=options.patience,
            length_penalty=options.length_penalty, max_length=max_length, suppress_blank=options.suppress_blank,
            suppress_tokens=options.suppress_tokens, return_scores=True, return_no_speech_prob=True,
            sampling_temperature=options.temperatures[0], repetition_penalty=options.repetition_penalty,
            no_repeat_ngram_size=options.no_repeat_ngram_size)

        output = []
        for result in results:
            seq_len = len(result.sequences_ids[0])
            cum_logprob = result.scores[0] * (seq_len ** options.length_penalty)
            output.append(dict(avg_logprob=cum_logprob / (seq_len + 1), no_speech_prob=result.no_speech_prob,
                               tokens=result.sequences_ids[0]))
        return encoder_output, output

    # ---- (:256-532)
    def _transcribe(
        self,
        audio: Union[str, BinaryIO, np.ndarray],
        language: Optional[str] = None,
        task: str = "transcribe",
        log_progress: bool = False,
        beam_size: int = 5,
        best_of: int = 5,
        patience: float = 1,
        length_penalty: float = 1,
        repetition_penalty: float = 1,
        no_repeat_ngram_size: int = 0,
        temperature: Union[float, List[float], Tuple[float, ...]] = [0.0, 0.2, 0.4, 0.6, 0.8, 1.0],
        compression_ratio_threshold: Optional[float] = 2.4,
        log_prob_threshold: Optional[float] = -1.0,
        no_speech_threshold: Optional[float] = 0.6,
        condition_on_previous_text: bool = True,
        prompt_reset_on_temperature: float = 0.5,
        initial_prompt: Optional[Union[str, Iterable[int]]] = None,
        prefix: Optional[str] = None,
        suppress_blank: bool = True,
        suppress_tokens: Optional[List[int]] = [-1],
        without_timestamps: bool = True,
        max_initial_timestamp: float = 1.0,
        word_timestamps: bool = False,
        prepend_punctuations: str = "\"'“¿([{-",
        append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
        multilingual: bool = False,
        vad_filter: bool = True,
        vad_parameters: Optional[Union[dict, VadOptions]] = None,
        max_new_tokens: Optional[int] = None,
        chunk_length: Optional[int] = None,
        clip_timestamps: Optional[List[dict]] = None,
        hallucination_silence_threshold: Optional[float] = None,
        batch_size: int = 8,
        hotwords: Optional[str] = None,
        language_detection_threshold: Optional[float] = 0.5,
        language_detection_segments: int = 1,
    ) -> Tuple[Iterable[Segment], TranscriptionInfo]:
        """Transcribe audio in chunks, `batch_size` chunks per decode, and return (segment generator, TranscriptionInfo).
        Arguments as the reference's (:302-377); compression_ratio_threshold, log_prob_threshold, no_speech_threshold,
        condition_on_previous_text, prompt_reset_on_temperature, prefix, max_initial_timestamp and
        hallucination_silence_threshold are accepted and unused there too. `clip_timestamps`: dicts with "start" / "end" in samples."""
        a = dict(locals())                     # the arguments by name, as `transcribe` binds them for the multichannel route
        features, chunks_metadata, _channels, vad_clips, tokenizer, options, info = _plan(
            self, a, lambda slot: _resident_mono(self.model, slot, audio), max_batch=getattr(self.model, "max_batch", None))
        segments = self._batched_segments_generator(features, tokenizer, chunks_metadata, int(batch_size), options, log_progress)
        if vad_clips is not None:
            segments = self._restored(segments, vad_clips[0], self.model.feature_extractor.sampling_rate)
        return segments, info

    def transcribe(self, audio, *args, multichannel: bool = False, target_language: Optional[str] = None, translator=None, **kwargs):
        """The reference's transcribe — every argument of `_transcribe` above, by position or by name — and keyword-only options
        the reference does not have. multichannel=False is `_transcribe`, untouched. multichannel=True: every channel of the file is
        transcribed on its own while the chunks of all channels share the decode groups; segments carry `channel` and come sorted by
        (start, channel) — whisperlive_amd/multichannel.py. target_language (with `translator`, a translation.HipTranslator): the
        segments come back as a LIST, each with `.translation` — the whole file as one translation job (file_translation.py); None
        changes nothing. (`__wrapped__` below: the signature introspection reports is the reference's, which is what a caller
        written against the reference binds to.)"""
        if target_language is not None:
            from .file_translation import check_target_language, translate_segments
            if translator is None:              # before the file is transcribed, as iter_many refuses it
                raise ValueError("target_language needs a translator")
            check_target_language(translator, target_language)
            segments, info = self.transcribe(audio, *args, multichannel=multichannel, **kwargs)
            return translate_segments(segments, translator, target_language), info
        if not multichannel:
            return self._transcribe(audio, *args, **kwargs)
        from .multichannel import transcribe_multichannel
        bound = inspect.signature(self._transcribe).bind(audio, *args, **kwargs)
        bound.apply_defaults()
        return transcribe_multichannel(self, dict(bound.arguments))

    transcribe.__wrapped__ = _transcribe

    def iter_many(self, audios, *, batch_size: int = 8, on_error: str = "return", **kwargs):
        """Many files as ONE job whose decode groups mix files (whisperlive_amd/many_files.py): yields (index, segments, info) per
        file — what `transcribe(audios[index], ...)` returns, the segments as a list — or (index, exception, None) for a damaged file.
        target_language= (one code, or a list with a code or None per file) with translator=: each file's segments carry
        `.translation`, one translation job per file as it finishes.
        wave_put: bool = False (a keyword of the job, beside those of `transcribe`): True puts the files of a wave in one Slot.put_many
        call with one wait (a slot without it keeps the per-file puts); the results are the same, the default stays one put per file.
        diarize= (False | True | FileDiarizer, or a list with one per file) and max_speakers=: the files of a wave are yielded together
        after its last decode group, their segments and words carrying `.speaker` (one diarize_many job per wave; many_files.py)."""
        from .many_files import iter_many
        target_language, translator = kwargs.pop("target_language", None), kwargs.pop("translator", None)
        if target_language is None:
            return iter_many(self, audios, batch_size=batch_size, on_error=on_error, **kwargs)
        from .file_translation import check_target_language, per_file_languages, translated_job
        if isinstance(audios, (str, bytes, bytearray, np.ndarray)) or hasattr(audios, "read"):
            raise TypeError("transcribe_many takes a sequence of files or waveforms; one file goes to transcribe")
        audios = list(audios)
        languages = per_file_languages(target_language, len(audios))
        for lang in {x for x in languages if x is not None}:
            check_target_language(translator, lang)
        if translator is None and any(x is not None for x in languages):
            raise ValueError("target_language needs a translator")
        return translated_job(iter_many(self, audios, batch_size=batch_size, on_error=on_error, **kwargs), languages, translator)

    def transcribe_many(self, audios, *, batch_size: int = 8, on_error: str = "return", **kwargs):
        """`iter_many` to the end -> [(segments, info) or (exception, None)] in input order (wave_put=True: see `iter_many`)"""
        if kwargs.get("target_language") is not None:
            audios = list(audios) if isinstance(audios, (list, tuple)) or hasattr(audios, "__next__") else audios
            job = self.iter_many(audios, batch_size=batch_size, on_error=on_error, **kwargs)
            out: list = [None] * len(audios)
            for index, segments, info in job:
                out[index] = (segments, info)
            return out
        kwargs.pop("target_language", None)
        kwargs.pop("translator", None)
        from .many_files import transcribe_many
        return transcribe_many(self, audios, batch_size=batch_size, on_error=on_error, **kwargs)

    def _language(self, features, language, language_detection_segments, language_detection_threshold, group_size=None):
        """-> (language, probability, all probabilities or None): the language given (an English-only model knows one), or the one
        detected on the leading `features` of a multilingual model. group_size: see _leading_features"""
        model = self.model
        if language is not None:
            if not model.model.is_multilingual and language != "en":
                model.logger.warning("The current model is English-only but the language parameter is set to '%s'; "
                                     "using 'en' instead." % language)
                language = "en"
            return language, 1, None
        if not model.model.is_multilingual:
            return "en", 1, None
        need = language_detection_segments * model.feature_extractor.nb_max_frames
        language, language_probability, all_language_probs = model.detect_language(
            features=np.concatenate(
                self._leading_features(features, need, group_size)
                + [np.full((model.model.n_mels, 1), -1.5, dtype="float32")], axis=1),  # a dummy feature to account for empty audio
            language_detection_segments=language_detection_segments,
            language_detection_threshold=language_detection_threshold)
        model.logger.info("Detected language '%s' with probability %.2f", language, language_probability)
        return language, language_probability, all_language_probs

    def _leading_features(self, features, need_frames: int, group_size: Optional[int] = None) -> List[np.ndarray]:
        """the first chunks' features ([..., :-1] each) on the host, as many as the language vote reads. group_size: chunks per
        log-mel launch (default: every item of the slot; multichannel keeps the groups in front of the source items)"""
        if not isinstance(features, DeviceChunks):
            return list(features)
        out, have = [], 0
        slot = features.slot
        step = int(group_size or slot.max_batch)
        with slot.lock:
            for a in range(0, len(features), step):
                if have >= need_frames:
                    break
                group = features[a:a + step]
                group.to_device()
                for i in range(len(group)):
                    if have >= need_frames:
                        break
                    out.append(slot.features(i)[..., :-1])
                    have += out[-1].shape[-1]
        return out

    @staticmethod
    def _restored(segments, speech_chunks, sampling_rate):
        """times in the concatenated speech -> the file's timeline, segment by segment as the groups finish"""
        for seg in segments:
            yield restore_speech_timestamps([seg], speech_chunks, sampling_rate)[0]

    def _groups(self, features, tokenizer, chunks_metadata, batch_size, options, log_progress):
        """decode `batch_size` chunks at a time, under the slot's lock on the device route -> (index of the group's first chunk, what
        `forward` returns for the group), group by group"""
        lock = features.slot.lock if isinstance(features, DeviceChunks) else nullcontext()
        for i in range(0, len(features), batch_size):
            with lock:
                results = self.forward(features[i: i + batch_size], tokenizer, chunks_metadata[i: i + batch_size], options)
            yield i, results
            if log_progress:
                self.model.logger.info("batched transcription: %d / %d chunks", min(i + batch_size, len(features)), len(features))

    # ---- (:534-571)
    def _batched_segments_generator(self, features, tokenizer, chunks_metadata, batch_size, options, log_progress):
        seg_idx = 0
        for _i, results in self._groups(features, tokenizer, chunks_metadata, batch_size, options, log_progress):
            for result in results:
                for segment in result:
                    seg_idx += 1
                    yield _segment(segment, options, seg_idx)
        self.last_speech_timestamp = 0.0


def _segment(result: dict, options, seg_id: int = 0, channel: Optional[int] = None) -> Segment:
    """one sub-segment dict of `forward` -> the Segment the caller gets"""
    return Segment(
        seek=result["seek"], id=seg_id, text=result["text"], start=round(result["start"], 3), end=round(result["end"], 3),
        words=(None if not options.word_timestamps else [Word(**word) for word in result["words"]]),
        tokens=result["tokens"], avg_logprob=result["avg_logprob"], no_speech_prob=result["no_speech_prob"],
        compression_ratio=result["compression_ratio"], temperature=options.temperatures[0], channel=channel)


class Resident(NamedTuple):
    """The audio of one file as a route left it for `_plan`: `n_samples` at 16 kHz per channel, channel c resident in item
    `items[c]` of the slot."""
    n_samples: int
    items: List[int]
    host_audio: object                  # the host waveform, or a callable (item) -> its host copy, fetched when something asks
    gate: Callable                      # (vad_parameters, vad_model) -> the speech clips of each channel
    device: bool = True                 # False: the audio is on the host only (mono, an engine without the front end)
    multichannel: bool = False          # True: chunks and segments carry their channel, even when there is one


def _plan(pipe, a: dict, make_resident: Callable, max_batch: Optional[int] = None):
    """The file plan behind both routes of BatchedInferencePipeline.transcribe: from its arguments `a` (by name, defaults applied) to
    what the segment generators decode. make_resident(slot) -> Resident is the route's own way of reading the audio, called once the
    batch has been checked and the slot taken; max_batch: the mono route's limit on batch_size (multichannel checks its own, which
    depends on the channel count, in make_resident).
    -> (features, chunks_metadata, the channel of each chunk or None (mono), the gate's clips per channel or None (times need no
    restoring), tokenizer, options, info). The chunks of all channels are pooled in order (channel, start); a mono file is a file
    with one channel."""
    model = pipe.model
    sampling_rate = model.feature_extractor.sampling_rate
    a = dict(a)
    if a["multilingual"] and not model.model.is_multilingual:
        model.logger.warning("The current model is English-only but the multilingual parameter is set to"
                             "True; setting to False instead.")
        a["multilingual"] = False
    batch_size, beam_size = int(a["batch_size"]), int(a["beam_size"])
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}: at least one chunk per decode")
    if max_batch is not None and batch_size > int(max_batch):
        raise ValueError(f"batch_size {batch_size} exceeds this transcriber's max_batch {int(max_batch)} (the items one slot holds): "
                         f"create the model with max_batch >= {batch_size}")
    if batch_size * beam_size > MAX_DEC_ROWS:
        raise ValueError(f"batch_size {batch_size} x beam_size {beam_size} = {batch_size * beam_size} decoder rows: "
                         f"one decode step holds at most {MAX_DEC_ROWS}")
    slot = model._slot(rows=beam_size)
    if hasattr(model, "_tls"):
        model._tls.file_audio = None          # (what an earlier call of this thread left resident is about to be overwritten)
    res = make_resident(slot)
    n_samples = res.n_samples
    duration = n_samples / sampling_rate

    chunk_length = a["chunk_length"] or model.feature_extractor.chunk_length
    clip_timestamps, vad_parameters = a["clip_timestamps"], a["vad_parameters"]
    from_vad = False
    # if no segment split is provided, use vad_model and generate segments
    if clip_timestamps:
        clips = [[dict(c) for c in clip_timestamps] for _ in res.items]          # explicit clips apply to every channel
    elif a["vad_filter"]:
        vad_parameters = _vad_options(vad_parameters, chunk_length)
        clips = res.gate(vad_parameters, model._vad_model())
        from_vad = True
    # run the audio if it is less than 30 sec even without clip_timestamps
    elif duration < chunk_length:
        clips = [[{"start": 0, "end": n_samples}] for _ in res.items]
    else:
        raise RuntimeError("No clip timestamps found. "
                           "Set 'vad_filter' to True or provide 'clip_timestamps'.")
    clips = [[c for c in cl if c["end"] > c["start"]] for cl in clips]
    speech = [sum(c["end"] - c["start"] for c in cl) for cl in clips]
    duration_after_vad = sum(speech) / sampling_rate

    ranges, chunks_metadata, channels = pool_chunks(
        [_collect_ranges(cl, sampling_rate, chunk_length) if cl else ([], []) for cl in clips])
    if res.device:
        features = DeviceChunks(slot, ranges, res.host_audio, [res.items[c] for c in channels] if res.multichannel else res.items[0],
                                n_samples)
        if n_samples > 0 and hasattr(model, "_tls"):
            # what reads the file after the transcription (speaker labels) finds each channel in its item: resident_file_audio
            handles = [ResidentPcm(slot, i, n_samples, features.shared) for i in res.items]
            model._tls.file_audio = handles if res.multichannel else handles[0]
    else:
        wave = _resolve(res.host_audio, slot)
        features = [model.feature_extractor(np.concatenate([wave[s:e] for s, e in rg]))[..., :-1] for rg in ranges]

    # one language for the file: the one given, or detected on the channel with the most speech — multichannel in groups of batch_size
    # chunks, so that the detection's log-mel launches stay in front of the source items too
    lc = language_channel(speech)
    lead = features[channels.index(lc): channels.index(lc) + channels.count(lc)] if lc in channels else features[0:0]
    language, language_probability, all_language_probs = pipe._language(
        lead, a["language"], a["language_detection_segments"], a["language_detection_threshold"],
        group_size=batch_size if res.multichannel else None)

    tokenizer = Tokenizer(model.hf_tokenizer, model.model.is_multilingual, task=a["task"], language=language)
    if not res.device:
        features = np.stack([pad_or_trim(feature) for feature in features]) if features else []
    elif res.multichannel:
        features.channels = channels            # every group is cut with its chunks' channels (forward reads them)
    options = _options(tokenizer, a, (clip_timestamps or clips) if res.multichannel else clips[0])
    info = TranscriptionInfo(language=language, language_probability=language_probability, duration=duration,
                             duration_after_vad=duration_after_vad, transcription_options=options,
                             vad_options=vad_parameters, all_language_probs=all_language_probs)
    return features, chunks_metadata, channels if res.multichannel else None, clips if from_vad else None, tokenizer, options, info


def _resident_mono(model, slot, audio) -> Resident:
    """The mono route's audio: a file is down-mixed and resampled into item 0 on the device (a FLAC file decoded there too), a
    waveform uploaded; an engine without the front end, or a shape the front end refuses, keeps the audio on the host."""
    sampling_rate = model.feature_extractor.sampling_rate
    n_samples, host_audio, device = _put_audio(model, slot, audio, 0)

    def gate(vad_parameters, vad_model):
        if (device and n_samples > 0 and hasattr(vad_model, "probs_pcm")
                and getattr(vad_model, "device", None) == getattr(slot.engine, "device", -1)):
            with slot.lock:
                return [_vad.get_speech_timestamps_pcm(slot, n_samples, vad_parameters, sampling_rate, model=vad_model)]
        return [_vad.get_speech_timestamps(_resolve(host_audio, slot), vad_parameters, sampling_rate, model=vad_model)]

    return Resident(n_samples, [0], host_audio, gate, device)


def _put_audio(model, slot, audio, item: int = 0):
    """One file or waveform into item `item` of `slot`, by the route its kind takes -> (samples at 16 kHz, host audio, device).
    A FLAC file and a telephony WAV file are decoded on the device (Slot.put_flac / put_wav), any other file is decoded on the host
    and down-mixed and resampled on the device (put_frames), a waveform is uploaded (pcm_put); a shape the front end refuses is
    down-mixed and resampled on the host and uploaded as a waveform. host audio: the waveform where one exists on the host, else
    `slot.pcm` (item -> the host copy, fetched only when something asks). device False: an engine without the front end, nothing
    was put. A damaged file is a ValueError. (The mono route puts its one file into item 0, a job of many files each into its own.)"""
    sampling_rate = model.feature_extractor.sampling_rate
    device = all(hasattr(slot, m) for m in ("logmel_chunks", "pcm_put", "pcm"))
    host_audio = n_samples = None
    if not isinstance(audio, np.ndarray):
        from .audio_io import frames_to_mono, read_audio, wav_served
        from .engine import resample_supported
        data = _file_bytes(audio)
        # a FLAC file is decoded on the device (Slot.put_flac leaves resident what put_frames(read_flac(file)) would), and so is a
        # telephony WAV file the probe says the device serves (Slot.put_wav: G.711, IMA / MS ADPCM); a stream that route does not serve
        # keeps the host decode below, a damaged one is a ValueError
        on_device = False
        compressed = None
        if device and sampling_rate == 16000 and data[:4] == b"fLaC" and hasattr(slot, "put_flac"):
            compressed = ("FLAC", slot.put_flac)
        elif device and sampling_rate == 16000 and hasattr(slot, "put_wav") and wav_served(data):
            compressed = ("WAV", slot.put_wav)
        if compressed is not None:
            try:
                with slot.lock:
                    n_samples, _ = compressed[1](data, item=item)
                on_device = True
            except _WlxError as e:
                if e.code == _ERR_DATA:
                    raise ValueError(f"damaged {compressed[0]} stream: {e}") from e
                if e.code != _ERR_ARG:
                    raise
        if not on_device:
            file_frames, file_sr = read_audio(data)
            on_device = (device and sampling_rate == 16000 and file_frames.shape[0] > 0 and hasattr(slot, "put_frames")
                         and resample_supported(file_sr, file_frames.shape[1]))
            if on_device:
                try:
                    with slot.lock:
                        n_samples = slot.put_frames(file_frames, file_sr, item=item)
                except _WlxError as e:
                    if e.code != _ERR_ARG:             # only a REFUSED shape (nothing was launched) keeps the host route
                        raise
                    on_device = False
            if not on_device:
                audio = frames_to_mono(file_frames, file_sr, sampling_rate)
        if on_device:
            host_audio = slot.pcm                      # fetched only when something on the host needs it
    if n_samples is None:
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        host_audio, n_samples = audio, audio.shape[0]
        if device and n_samples > 0:
            with slot.lock:
                slot.pcm_put(audio, item=item)
    return n_samples, host_audio, device


def _put_audio_many(model, slot, audios, items) -> list:
    """`_put_audio` for a wave: audios[k] into item items[k], the files whose route runs on the device going up together in
    Slot.put_many calls (one per run of neighbouring items, 64 entries at the most each) -> per file what `_put_audio` returns, or the
    exception it would have raised (ValueError for a damaged file, OSError) — returned, so that one file costs only itself.
    The kind of each file is chosen exactly as `_put_audio` chooses it: FLAC magic -> the FLAC bytes, `wav_served` -> the WAV bytes, any
    other file is read on the host and gives frames when `resample_supported`, a waveform gives PCM; anything else (an empty waveform,
    a shape the resampler does not serve, a slot without the front end) takes `_put_audio`, per file. An entry the device REFUSES
    falls back to `_put_audio` for that file alone; a damaged one is the ValueError `_put_audio` raises."""
    sampling_rate = model.feature_extractor.sampling_rate
    device = all(hasattr(slot, m) for m in ("logmel_chunks", "pcm_put", "pcm", "put_many")) and sampling_rate == 16000
    out: list = [None] * len(audios)
    entries: list = [None] * len(audios)
    for k, audio in enumerate(audios):
        try:
            if isinstance(audio, Exception):
                raise audio
            if not device:
                continue
            if isinstance(audio, np.ndarray):
                if audio.shape[0] > 0:
                    entries[k] = ("pcm", np.ascontiguousarray(audio, dtype=np.float32))
                continue
            from .audio_io import read_audio, wav_served
            from .engine import resample_supported
            data = _file_bytes(audio)
            if data[:4] == b"fLaC" and hasattr(slot, "put_flac"):
                entries[k] = ("flac", data)
            elif hasattr(slot, "put_wav") and wav_served(data):
                entries[k] = ("wav", data)
            else:
                file_frames, file_sr = read_audio(data)
                if file_frames.shape[0] > 0 and hasattr(slot, "put_frames") and resample_supported(file_sr, file_frames.shape[1]):
                    entries[k] = ("frames", file_frames, file_sr)
        except (ValueError, OSError, TypeError) as e:
            out[k] = e
    runs: list = []                           # runs of entries whose items are neighbours: one put_many each
    for k, ent in enumerate(entries):
        if ent is None:
            continue
        if runs and runs[-1][-1] + 1 == k and items[runs[-1][-1]] + 1 == items[k]:
            runs[-1].append(k)
        else:
            runs.append([k])
    for run in runs:
        with slot.lock:
            results = slot.put_many([entries[k] for k in run], first_item=items[run[0]])
        for k, r in zip(run, results):
            if isinstance(r, _WlxError):
                if r.code == _ERR_DATA:
                    out[k] = ValueError(f"damaged {entries[k][0].upper()} stream: {r}")
                elif r.code != _ERR_ARG:
                    raise r
                entries[k] = None             # refused: nothing was launched for it, the file takes its other routes alone
            else:
                out[k] = (r[0], entries[k][1] if entries[k][0] == "pcm" else slot.pcm, True)
    for k, audio in enumerate(audios):
        if out[k] is None:
            try:
                out[k] = _put_audio(model, slot, audio, items[k])
            except (ValueError, OSError, _WlxError) as e:
                out[k] = e
    return out


def _file_bytes(audio) -> bytes:
    """the bytes of what is not a waveform: a path, bytes or a file object; anything else is refused"""
    if not isinstance(audio, (str, bytes, bytearray)) and not hasattr(audio, "read"):
        raise TypeError("audio must be a float32 numpy waveform at 16 kHz, or a WAV / FLAC path, bytes or file object")
    from .audio_io import _read_all
    return _read_all(audio)


def _vad_options(vad_parameters, chunk_length) -> VadOptions:
    """the gate's options of a batched transcription: chunks of at most chunk_length seconds, whatever the caller's dict says"""
    if vad_parameters is None:
        return VadOptions(max_speech_duration_s=chunk_length, min_silence_duration_ms=160)
    if isinstance(vad_parameters, dict):
        if "max_speech_duration_s" in vad_parameters.keys():
            vad_parameters.pop("max_speech_duration_s")
        return VadOptions(**vad_parameters, max_speech_duration_s=chunk_length)
    return vad_parameters


def _options(tokenizer, a: dict, clip_timestamps) -> TranscriptionOptions:
    """the options a batched transcription decodes with, from transcribe's arguments `a` (by name): no conditioning on previous text,
    the first temperature only, no initial-timestamp limit, as the reference forces them"""
    temperature = a["temperature"]
    return TranscriptionOptions(
        beam_size=a["beam_size"], best_of=a["best_of"], patience=a["patience"], length_penalty=a["length_penalty"],
        repetition_penalty=a["repetition_penalty"], no_repeat_ngram_size=a["no_repeat_ngram_size"],
        log_prob_threshold=a["log_prob_threshold"], no_speech_threshold=a["no_speech_threshold"],
        compression_ratio_threshold=a["compression_ratio_threshold"],
        temperatures=(list(temperature[:1]) if isinstance(temperature, (list, tuple)) else [temperature]),
        initial_prompt=a["initial_prompt"], prefix=a["prefix"], suppress_blank=a["suppress_blank"],
        suppress_tokens=get_suppressed_tokens(tokenizer, a["suppress_tokens"]),
        prepend_punctuations=a["prepend_punctuations"], append_punctuations=a["append_punctuations"],
        max_new_tokens=a["max_new_tokens"], hotwords=a["hotwords"], word_timestamps=a["word_timestamps"],
        hallucination_silence_threshold=None, condition_on_previous_text=False, clip_timestamps=clip_timestamps,
        prompt_reset_on_temperature=0.5, multilingual=a["multilingual"], without_timestamps=a["without_timestamps"],
        max_initial_timestamp=0.0)


def _resolve(host_audio, slot) -> np.ndarray:
    if callable(host_audio):
        with slot.lock:
            return host_audio()
    return host_audio


def _collect_ranges(clip_timestamps: Sequence[dict], sampling_rate: int, max_duration: float):
    """vad.collect_chunks(audio, clip_timestamps, max_duration=max_duration) without the audio: per chunk the sample ranges it
    concatenates, and the same metadata (start_time / end_time on the concatenated timeline, segments)."""
    _chunks, meta = _vad.collect_chunks(_Spans(), list(clip_timestamps), sampling_rate, max_duration=max_duration)
    return [[(c["start"], c["end"]) for c in m["segments"]] for m in meta], meta


class _Spans:
    """stands in for the waveform in collect_chunks: a slice of it is an empty array (only the bookkeeping is wanted)"""

    def __getitem__(self, key):
        return np.zeros(0, dtype=np.float32)
