"""BatchedInferencePipeline.transcribe(multichannel=True): every channel of a file transcribed on its own, in shared decode groups.

A two-party call recording carries one speaker per channel; the down-mix every other route starts from sums overlapping talk and
throws the channel's speaker identity away. Here the file's C channels become resident — one upload, no down-mix — in the LAST C items
of the calling thread's slot (item max_batch - C + c: ``Slot.put_frames_split`` / ``put_flac_split``), the gate reads all of them in one
pass (``SileroHIPModel.probs_pcm_many``), and the chunks of all channels are pooled in order (channel, start) and decoded
``batch_size`` at a time whatever their channel: per group ``logmel_chunks`` with one source item per chunk
(``wlx_logmel_chunks_multi``), ``encode``, ``generate`` and — with ``word_timestamps`` — ``align_batch``. The destination items of a
group are 0 .. batch_size - 1 and ``batch_size <= max_batch - C``, so no group ever overwrites a source. Nothing but the one upload and
the range tables crosses PCIe. There is NO host route: a shape the device front end refuses is a ValueError.

The procedure itself — batch checks, clips, chunks, language, options, info — is ``batched._plan``, the one the mono route follows
(a mono file is a file with one channel whose source is item 0). This module keeps what is the route's own: how the channels become
resident (``_make_resident``: the last C items, the ``_NO_HOST`` refusals, ``check_batch``, ``source_rows_addressable``, the one gate
pass) and how the segments leave (``_segments``: all of them, sorted by (start, channel), when the last group is done).

The functions above ``_make_resident`` are host logic only (tests/test_multichannel_host.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import vad as _vad
from ._lib import ERR_ARG as _ERR_ARG, ERR_DATA as _ERR_DATA, WlxError as _WlxError
from .engine import FlacFrames, resample_supported
from .transcriber import restore_speech_timestamps
from .types import Segment


def check_batch(batch_size: int, max_batch: int, channels: int):
    """the C channels take the last C items of the slot; a decode group's destination items must stay in front of them"""
    if batch_size > max_batch - channels:
        raise ValueError(f"multichannel: batch_size {batch_size} exceeds max_batch {max_batch} - {channels} channels = "
                         f"{max_batch - channels} (the file's channels stay resident in the slot's last {channels} items): "
                         f"create the model with max_batch >= {batch_size + channels} or lower batch_size")


def pool_chunks(per_channel: Sequence[Tuple[list, list]]):
    """per channel (chunk ranges, chunk metadata), each in start order -> (ranges, metadata, channel per chunk) of all channels in
    order (channel, start)"""
    ranges, meta, channels = [], [], []
    for c, (rg, md) in enumerate(per_channel):
        ranges.extend(rg)
        meta.extend(md)
        channels.extend([c] * len(rg))
    return ranges, meta, channels


def language_channel(speech_samples: Sequence[int]) -> int:
    """the channel the file's language is detected on: the one with the most speech after the gate, the lowest index on a tie"""
    best = 0
    for c, n in enumerate(speech_samples):
        if n > speech_samples[best]:
            best = c
    return best


def order_segments(segments: List[Segment]) -> List[Segment]:
    """segments of all channels, each on its own channel's timeline -> sorted by (start, channel), ids 1..N in that order"""
    out = sorted(segments, key=lambda s: (s.start, s.channel))          # (stable: equal keys keep their decode order)
    for i, s in enumerate(out):
        s.id = i + 1
    return out


def parse_waveform(audio: np.ndarray) -> np.ndarray:
    """1-D waveform -> [n, 1]; 2-D [n, C] stays; anything else is refused"""
    if audio.ndim == 1:
        return audio[:, None]
    if audio.ndim != 2:
        raise ValueError(f"multichannel: a waveform is [n] or [n, channels] at 16 kHz, not {audio.ndim}-dimensional")
    return audio


_NO_HOST = "multichannel=True has no host route: convert the file, or transcribe its down-mix with multichannel=False"


def _make_resident(model, slot, audio, batch_size: int):
    """-> batched.Resident: the file's channels resident in the last C items of the slot, and the gate that reads all of them"""
    from .batched import Resident, _file_bytes
    sampling_rate = model.feature_extractor.sampling_rate
    if sampling_rate != 16000 or not all(hasattr(slot, m) for m in ("put_frames_split", "logmel_chunks", "pcm")):
        raise ValueError(f"multichannel=True needs the device front end (Slot.put_frames_split), which this engine lacks. {_NO_HOST}")
    max_batch = int(getattr(slot, "max_batch", getattr(model, "max_batch", batch_size)))
    wav = None              # the bytes of a telephony WAV file the device decodes itself
    if isinstance(audio, np.ndarray):
        frames = parse_waveform(audio)
        frames = frames if frames.dtype == np.int16 else np.ascontiguousarray(frames, dtype=np.float32)
        rate, flac = 16000, None
    else:
        from .audio_io import read_audio, wav_probe, wav_served
        data = _file_bytes(audio)
        if data[:4] == b"fLaC":
            import ctypes as C
            from . import _lib
            lib = slot.lib
            info = _lib.wlx_flac_info()
            rc = lib.wlx_flac_probe(data, len(data), C.byref(info))
            if rc == _ERR_DATA:
                raise ValueError(f"damaged FLAC stream: {lib.wlx_last_error().decode()}")
            if rc != 0 or not info.served:
                raise ValueError(f"FLAC stream of {info.sample_rate} Hz x {info.channels} channels x {info.bits_per_sample} bits: the device "
                                 f"front end does not serve it. {_NO_HOST}")
            flac, frames, rate = FlacFrames(data), None, info.sample_rate
            channels = info.channels
        elif hasattr(slot, "put_wav_split") and wav_served(data):
            # a telephony WAV file the device decodes (G.711, IMA / MS ADPCM): its bytes go up as they are (Slot.put_wav_split); one the
            # probe does not serve is decoded by read_audio below and takes the frames' route
            info = wav_probe(data)
            flac, wav, frames, rate, channels = None, data, None, info.sample_rate, info.channels
        else:
            frames, rate = read_audio(data)
            flac = None
    if flac is None and wav is None:
        channels = frames.shape[1]
        if frames.shape[0] == 0:
            raise ValueError("multichannel: empty audio")
        if not resample_supported(rate, channels):
            raise ValueError(f"{rate} Hz x {channels} channels: the device front end does not serve this shape. {_NO_HOST}")
    if channels >= max_batch:
        raise ValueError(f"multichannel: {channels} channels need a transcriber with max_batch >= {channels + 1}, this one has {max_batch}")
    check_batch(batch_size, max_batch, channels)
    first = max_batch - channels
    try:
        with slot.lock:
            if wav is not None:
                n, _ = slot.put_wav_split(wav, first)
            else:
                n = slot.put_frames_split(flac if flac is not None else frames, rate, first)
    except _WlxError as e:
        if e.code == _ERR_DATA:
            raise ValueError(f"damaged {'WAV' if wav is not None else 'FLAC'} stream: {e}") from e
        if e.code == _ERR_ARG:
            raise ValueError(f"the device front end refused the audio ({e}). {_NO_HOST}") from e
        raise
    if not source_rows_addressable(channels, n):          # before any decode, not from the middle of the generator
        raise ValueError(f"multichannel: {channels} channels of {n} samples lie further apart in the slot than the chunk "
                         "gather addresses (2^31 - 1 samples)")
    items = [first + c for c in range(channels)]

    def gate(vad_parameters, vad_model):
        if hasattr(vad_model, "probs_pcm_many") and getattr(vad_model, "device", None) == getattr(slot.engine, "device", -1):
            with slot.lock:                  # the gate of ALL channels in one pass over the network
                probs = vad_model.probs_pcm_many(slot, [n] * channels, first_item=first)
            return [_vad.speech_segments_from_probs_native(p, n, vad_parameters, sampling_rate) for p in probs]
        with slot.lock:                      # a gate with no device path reads the host copy, channel by channel
            waves = [slot.pcm(i) for i in items]
        return [_vad.get_speech_timestamps(w, vad_parameters, sampling_rate, model=vad_model) for w in waves]

    return Resident(n, items, slot.pcm, gate, multichannel=True)


def source_rows_addressable(channels: int, n_samples: int) -> bool:
    """wlx_logmel_chunks_multi addresses every source row from the lowest one with a 32-bit offset (csrc/logmel.hip keeps a range's
    physical start as an int): the C neighbouring rows, each as long as the slot's PCM buffers become for n_samples (whole 30 s
    windows), must span at most 2^31 - 1 samples. Eight channels of one hour are 4.6e8: what the front end serves always fits."""
    cap = -(-max(int(n_samples), 1) // 480000) * 480000
    return channels * cap <= 0x7FFFFFFF


def transcribe_multichannel(pipe, a: dict):
    """The body of BatchedInferencePipeline.transcribe(multichannel=True); `a`: that method's arguments by name, defaults applied.
    -> (segment generator, info): segments sorted by (start, channel) with ids 1..N in that order, each with its `channel` and times
    on its own channel's timeline; info.duration = the file's, info.duration_after_vad = the sum over channels. One language for the
    file. The plan is batched._plan, the one the mono route follows; what is this route's own is how the audio becomes resident."""
    from .batched import _plan
    features, meta, channels, vad_clips, tokenizer, options, info = _plan(
        pipe, a, lambda slot: _make_resident(pipe.model, slot, a["audio"], int(a["batch_size"])))
    return _segments(pipe, features, tokenizer, meta, channels, int(a["batch_size"]), options, a["log_progress"], vad_clips), info


def _segments(pipe, features, tokenizer, meta, channels, batch_size, options, log_progress, vad_clips: Optional[list]):
    """decode the pooled chunks group by group, restore each segment's times on its own channel's timeline, then yield all of them in
    (start, channel) order (the order is known only when the last group is done)"""
    from .batched import _segment
    sampling_rate = pipe.model.feature_extractor.sampling_rate
    out: List[Segment] = []
    for i, results in pipe._groups(features, tokenizer, meta, batch_size, options, log_progress):
        for ch, result in zip(channels[i:], results):
            for segment in result:
                seg = _segment(segment, options, channel=ch)
                if vad_clips is not None:
                    seg = restore_speech_timestamps([seg], vad_clips[ch], sampling_rate)[0]
                out.append(seg)
    yield from order_segments(out)
