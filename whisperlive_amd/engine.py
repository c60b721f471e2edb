"""Python face of the C-ABI engine (include/wlx.h): one ``HipWhisperEngine`` per GPU, ``Slot`` objects for
concurrent streams. numpy in / numpy out; all arithmetic happens in libwlx.so on the MI355X."""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import WlxError, check
from .specs import WhisperSpec


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@dataclass
class TokenIds:
    sot: int
    eot: int
    no_timestamps: int
    timestamp_begin: int
    no_speech: int
    blank: int = -1


@dataclass
class GenerationResult:
    """Mirror of ctranslate2.models.WhisperGenerationResult as the reference reads it
    (whisper_live/transcriber/transcriber_faster_whisper.py:1409-1414; whisper_live/batch_inference.py:357-368)."""
    sequences_ids: List[List[int]]
    scores: List[float]
    no_speech_prob: float
    sequences: Optional[List[List[str]]] = None


class HipWhisperEngine:
    """Weights repacked for gfx950 + kernels; thread-safe for concurrent calls on distinct slots."""

    def __init__(self, spec: WhisperSpec, weights: Dict[str, "np.ndarray"], device: int = 0):
        self.lib = _lib.load()
        self.spec = spec
        self.device = device
        cs = _lib.wlx_spec(spec.n_mels, spec.d_model, spec.n_heads, spec.enc_layers, spec.dec_layers, spec.ffn,
                           spec.vocab, spec.n_audio_ctx, spec.n_text_ctx)
        arr, keep = _lib.tensor_array(weights)      # (keep: alive until the create call returns)
        h = C.c_void_p()
        check(self.lib.wlx_engine_create(C.byref(cs), arr, len(weights), device, C.byref(h)))
        self._h = h
        self._lock = threading.Lock()

    def close(self):
        if getattr(self, "_h", None):
            self.lib.wlx_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        import sys
        if sys.is_finalizing():      # interpreter shutdown: daemon session threads may still be inside a call; the
            return                   # process is about to return the device memory anyway
        try:
            self.close()
        except Exception:
            pass

    def create_ring(self, capacity_samples: int = 0) -> "PcmRing":
        """A device-resident PCM ring for one client stream (include/wlx.h wlx_ring_*)."""
        h = C.c_void_p()
        check(self.lib.wlx_ring_create(self._h, int(capacity_samples), C.byref(h)))
        return PcmRing(self, h)

    def create_ring_group(self, fmt: int, channels: int, rate: int, capacity_samples: int = 0) -> "PcmRingGroup":
        """The lanes of one multichannel client stream (include/wlx.h wlx_ring_group_*): one device PCM ring per channel, filled
        together from the interleaved packets in their wire format (_lib.PCM_*)."""
        return PcmRingGroup(self, fmt, channels, rate, capacity_samples)

    def create_slot(self, max_batch: int = 1, max_rows_per_item: int = 5) -> "Slot":
        sid = C.c_int32(-1)
        check(self.lib.wlx_slot_create(self._h, max_batch, max_rows_per_item, C.byref(sid)))
        return Slot(self, sid.value, max_batch, max_rows_per_item)


def resample_supported(sample_rate: int, channels: int = 1) -> bool:
    """True when wlx_pcm_put_frames serves this file shape; other files keep the host route of audio_io.load_audio. Restates the
    library's rule (include/wlx.h RATES, csrc/resample.hip resample_ratio): at most 8 channels; for up / down = 16000 / rate reduced,
    max(up, down) <= 640, and the tap table plus the input span of 64 outputs fit 64 KB of LDS."""
    from math import gcd
    if sample_rate <= 0 or not 1 <= channels <= _lib.PCM_MAX_CHANNELS:
        return False
    g = gcd(16000, int(sample_rate))
    up, down = 16000 // g, int(sample_rate) // g
    if max(up, down) > _lib.RESAMPLE_MAX_RATIO:
        return False
    half_len = 0 if up == down else 10 * max(up, down)
    span = ((_lib.RESAMPLE_MIN_TILE - 1) * down + 2 * half_len) // up + 2
    return 4 * (2 * half_len + 1 + span) <= _lib.RESAMPLE_MAX_LDS


def _packet(raw, frame_bytes: int):
    """a packet (bytes, or a C-contiguous array of wire samples) -> (object to keep alive, address, frames); ValueError unless whole frames"""
    if isinstance(raw, np.ndarray):
        raw = np.ascontiguousarray(raw)
        nbytes, ptr = raw.nbytes, raw.ctypes.data
    else:
        raw = bytes(raw)
        nbytes, ptr = len(raw), C.cast(C.c_char_p(raw), C.c_void_p).value
    if nbytes % frame_bytes:
        raise ValueError(f"packet of {nbytes} bytes is not a whole number of {frame_bytes}-byte frames")
    return raw, ptr, nbytes // frame_bytes


def _sample_bytes(fmt: int) -> int:
    """bytes of one wire sample (_lib.PCM_*; the 8-bit formats are every other code the library takes)"""
    return {_lib.PCM_F32: 4, _lib.PCM_S16: 2}.get(int(fmt), 1)


def _append_frames(ring, entry, rows: int, raw, flush: bool, max_resident: Optional[int], trim: Optional[int]):
    """One packet to `entry` (wlx_ring_append_frames / wlx_ring_group_append_frames) of `ring` (a PcmRing or a PcmRingGroup with a
    wire format) -> (new[rows][n]: the new 16 kHz samples, one row per lane, dropped, base, resident)"""
    raw, ptr, n = _packet(raw, ring._frame_bytes)
    want, have = C.c_int64(0), C.c_int64(0)
    check(ring.lib.wlx_resample_stream_count(ring.format[2], ring._frames_seen + n, 1, C.byref(want)))   # the flushed count bounds the other
    check(ring.lib.wlx_resample_stream_count(ring.format[2], ring._frames_seen, 0, C.byref(have)))
    cap = max(want.value - have.value, 0)
    out = np.empty((rows, cap), np.float32)
    k, d, b, r = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(entry(ring._h, ptr if n else None, n, 1 if flush else 0, ring.MAX_RESIDENT if max_resident is None else int(max_resident),
                ring.TRIM if trim is None else int(trim), _f32p(out), cap, C.byref(k), C.byref(d), C.byref(b), C.byref(r)))
    ring._frames_seen += n
    return out[:, : k.value], d.value, b.value, r.value


class PcmRing:
    """The device-side mirror of ServeClientBase.frames_np (whisper_live/backend/base.py:173-234): a client's packets are appended
    ONCE, the VAD gate and the log-mel front end read them in HBM. Positions are absolute stream sample positions."""
    MAX_RESIDENT = 45 * 16000          # base.py:191 (45 s) ...
    TRIM = 30 * 16000                  # ... :192-193 (the oldest 30 s go)

    def __init__(self, engine: "HipWhisperEngine", handle):
        self.engine, self.lib, self._h = engine, engine.lib, handle
        self.device = getattr(engine, "device", 0)

    def append(self, samples: np.ndarray, max_resident: Optional[int] = None, trim: Optional[int] = None) -> Tuple[int, int, int]:
        """-> (samples dropped by this call, first resident position, resident count)"""
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        d, b, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.wlx_ring_append(self._h, _f32p(x), x.shape[0], self.MAX_RESIDENT if max_resident is None else int(max_resident),
                                       self.TRIM if trim is None else int(trim), C.byref(d), C.byref(b), C.byref(r)))
        return d.value, b.value, r.value

    def set_format(self, fmt: int, channels: int, rate: int) -> None:
        """Give the ring a wire format (_lib.PCM_*; once, before the first append): packets then go through append_frames."""
        check(self.lib.wlx_ring_set_format(self._h, int(fmt), int(channels), int(rate)))
        self.format = (int(fmt), int(channels), int(rate))
        self._frame_bytes = int(channels) * _sample_bytes(fmt)
        self._frames_seen = 0

    def append_frames(self, raw, flush: bool = False, max_resident: Optional[int] = None, trim: Optional[int] = None):
        """One packet in the wire format (bytes, or a C-contiguous array of wire samples) -> (the packet's new 16 kHz samples, samples
        dropped by this call, first resident position, resident count). The packet crosses PCIe as it is; the new samples come back
        in the same wait. flush=True completes the stream to the one-shot length and closes it."""
        new, d, b, r = _append_frames(self, self.lib.wlx_ring_append_frames, 1, raw, flush, max_resident, trim)
        return new[0], d, b, r

    def state(self) -> Tuple[int, int]:
        b, r = C.c_int64(0), C.c_int64(0)
        check(self.lib.wlx_ring_state(self._h, C.byref(b), C.byref(r)))
        return b.value, r.value

    def close(self):
        if getattr(self, "_h", None):
            self.lib.wlx_ring_destroy(self._h)
            self._h = None


class _PcmRingLane(PcmRing):
    """Lane c of a PcmRingGroup: a PcmRing for every reader (state, the VAD gate, logmel_ring, the speaker engine). The library refuses
    its append / set_format / append_frames (WLX_ERR_STATE); close() only drops the borrowed handle, the group owns the memory."""

    def __init__(self, group: "PcmRingGroup", channel: int, handle):
        super().__init__(group.engine, handle)
        self.group, self.channel = group, channel
        self.format = (group.format[0], 1, group.format[2])
        self._frame_bytes = group._frame_bytes // group.channels
        self._frames_seen = 0

    def close(self):
        self._h = None


class PcmRingGroup:
    """One device PCM ring per channel of a multichannel live stream (wlx_ring_group_*): `append_frames` takes the interleaved packet
    as it came off the socket and fills every lane in one launch; `lane(c)` is the ring the session of channel c reads."""
    MAX_RESIDENT, TRIM = PcmRing.MAX_RESIDENT, PcmRing.TRIM

    def __init__(self, engine: "HipWhisperEngine", fmt: int, channels: int, rate: int, capacity_samples: int = 0):
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= _lib.PCM_MAX_CHANNELS:
            raise ValueError(f"channels {channels!r} outside 1..{_lib.PCM_MAX_CHANNELS}")
        if fmt not in (_lib.PCM_F32, _lib.PCM_S16, _lib.PCM_U8, _lib.PCM_MULAW, _lib.PCM_ALAW):
            raise ValueError(f"unknown sample format {fmt!r}")
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or not resample_supported(int(rate), int(channels)):
            raise ValueError(f"sample rate {rate!r} Hz is not a rate the device resampler serves")
        if capacity_samples < 0:
            raise ValueError("negative capacity")
        self.engine, self.lib = engine, engine.lib
        self.device = getattr(engine, "device", 0)
        self.format = (int(fmt), int(channels), int(rate))
        self.channels = int(channels)
        self._frame_bytes = self.channels * _sample_bytes(fmt)
        self._frames_seen = 0
        h = C.c_void_p()
        check(self.lib.wlx_ring_group_create(engine._h, int(capacity_samples), int(fmt), self.channels, int(rate), C.byref(h)))
        self._h = h
        self._lanes: List[_PcmRingLane] = []
        for c in range(self.channels):
            lh = C.c_void_p()
            check(self.lib.wlx_ring_group_lane(self._h, c, C.byref(lh)))
            self._lanes.append(_PcmRingLane(self, c, lh))

    def lane(self, c: int) -> PcmRing:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < self.channels:
            raise IndexError(f"lane {c!r} outside 0..{self.channels - 1}")
        if not self._h:
            raise RuntimeError("the ring group is closed")
        return self._lanes[c]

    def append_frames(self, raw, flush: bool = False, max_resident: Optional[int] = None, trim: Optional[int] = None):
        """One interleaved packet in the wire format -> (new[channels][n]: each lane's new 16 kHz samples, samples dropped per lane by
        this call, first resident position, resident count — the same on every lane). flush=True completes the stream and closes it."""
        if not self._h:
            raise RuntimeError("the ring group is closed")
        return _append_frames(self, self.lib.wlx_ring_group_append_frames, self.channels, raw, flush, max_resident, trim)

    def state(self) -> Tuple[int, int]:
        return self._lanes[0].state()

    def close(self):
        if getattr(self, "_h", None):
            for ln in self._lanes:
                ln.close()
            self.lib.wlx_ring_group_destroy(self._h)
            self._h = None


MAX_ITEM_SAMPLES = 3600 * 16000          # what one slot item holds (include/wlx.h: "audio chunk too long" past it)


def _at_16k(n_frames: int, sample_rate: int) -> int:
    """frames at sample_rate -> samples at 16 kHz, rounded up (0 where the rate is not known)"""
    return -(-int(n_frames) * 16000 // int(sample_rate)) if sample_rate and sample_rate > 0 else 0


def _wav_at_16k(data: bytes) -> int:
    """an upper estimate of the 16 kHz samples per channel in a telephony WAV file, from its header (0: not readable there)"""
    try:
        from .audio_io import WAVE_IMA_ADPCM, WAVE_MS_ADPCM, _wav_parse
        tag, ch, rate, bits, body = _wav_parse(data)
        frames = len(body) * 2 // ch if tag in (WAVE_IMA_ADPCM, WAVE_MS_ADPCM) else len(body) // (ch * max(1, bits // 8))
        return _at_16k(frames, rate)
    except Exception:  # noqa: BLE001 — the library says what is wrong with the file
        return 0


class ResidentPcm:
    """16 kHz mono audio resident in item `item` of `slot` (after pcm_put / put_frames): `n_samples` of it — what a reader on the device
    (SpeakerEmbedderHIP.embed_resident) needs to find it. The handle does not own the slot: the thread that made it keeps the slot
    until it is done with the handle. `intact()`: the item still holds those samples, as far as the handle can tell — `state`, when
    given, is the dict whose "resident" entry the owner clears when it overwrites the item (batched.DeviceChunks.shared)."""

    def __init__(self, slot: "Slot", item: int, n_samples: int, state: Optional[dict] = None):
        self.slot, self.item, self.n_samples, self.state = slot, int(item), int(n_samples), state

    def intact(self) -> bool:
        if self.slot.sid < 0 or self.n_samples <= 0 or (self.state is not None and not self.state.get("resident", False)):
            return False
        count = getattr(self.slot, "pcm_count", None)           # (a test double of a slot without the entry point: not resident)
        if count is None:
            return False
        with self.slot.lock:
            return count(self.item) == self.n_samples


class FlacFrames:
    """The frames of a FLAC file, still compressed: what Slot.put_frames takes in place of decoded frames (Slot.put_flac makes one).
    sample_rate: STREAMINFO's, read here without the library (0 when the first metadata block is not a STREAMINFO: the library then
    says what is wrong with the stream); info: the stream's shape (_lib.wlx_flac_info) once put_frames has taken the frames."""

    def __init__(self, data: bytes):
        self.data = bytes(data)
        d = self.data
        ok = len(d) >= 42 and d[:4] == b"fLaC" and (d[4] & 0x7F) == 0
        self.sample_rate = int.from_bytes(d[18:21], "big") >> 4 if ok else 0
        self.total_samples = int.from_bytes(d[21:26], "big") & ((1 << 36) - 1) if ok else 0      # (0: the encoder did not say)
        self.info = None


class Slot:
    """One unit of concurrency (own HIP stream + scratch). Not re-entrant: one call at a time per slot."""

    def __init__(self, engine: HipWhisperEngine, sid: int, max_batch: int, rows: int):
        self.engine, self.sid, self.max_batch, self.rows = engine, sid, max_batch, rows
        self.lib, self._h = engine.lib, engine._h
        self.lock = threading.Lock()
        # the longest audio, in samples per item, any call has asked this slot to hold: a floor of the row stride of its PCM buffers,
        # which the library grows to the longest request (whole 30 s windows) and never shrinks. What sizes its source rows against the
        # 2^31 - 1 samples wlx_logmel_chunks_multi addresses (many_files.next_wave) reads it; the library has no entry point that tells.
        self.pcm_longest = 480000

    def _grew(self, n_samples) -> None:
        if 0 < int(n_samples) <= MAX_ITEM_SAMPLES:           # (a longer request is refused before anything grows)
            self.pcm_longest = max(self.pcm_longest, int(n_samples))

    def close(self):
        if self.sid >= 0 and self.engine._h:
            self.lib.wlx_slot_destroy(self.engine._h, self.sid)
        self.sid = -1

    # ---- features
    def logmel(self, pcm: np.ndarray, item: int = 0) -> int:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        nf = C.c_int32(0)
        self._grew(pcm.shape[0])
        check(self.lib.wlx_logmel(self.engine._h, self.sid, item, _f32p(pcm), pcm.shape[0], C.byref(nf)))
        return nf.value

    def pcm_put(self, pcm: np.ndarray, item: int = 0):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        self._grew(pcm.shape[0])
        check(self.lib.wlx_pcm_put(self.engine._h, self.sid, item, _f32p(pcm), pcm.shape[0]))

    def put_frames(self, frames: np.ndarray, sample_rate: int, item: int = 0) -> int:
        """File frames [n, channels] (int16, or anything else as float32; or a FlacFrames: a FLAC file's frames, still compressed) at
        `sample_rate` -> 16 kHz mono float32 resident in the
        item's PCM buffer, converted, down-mixed and resampled on the device (wlx_pcm_put_frames). -> samples resident.
        Raises WlxError for a rate the device resampler does not serve (see `resample_supported`)."""
        if isinstance(frames, FlacFrames):         # still compressed: the library decodes them on the device (STREAMINFO's rate holds)
            n, info = C.c_int64(0), _lib.wlx_flac_info()
            self._grew(_at_16k(frames.total_samples, frames.sample_rate))      # (the buffers grow before the frames are decoded)
            check(self.lib.wlx_pcm_put_flac(self.engine._h, self.sid, item, frames.data, len(frames.data), C.byref(info), C.byref(n)))
            frames.info = info
            self._grew(n.value)
            return n.value
        x = np.asarray(frames)
        if x.ndim == 1:
            x = x[:, None]
        fmt = _lib.PCM_S16 if x.dtype == np.int16 else _lib.PCM_F32
        x = np.ascontiguousarray(x, dtype=np.int16 if fmt == _lib.PCM_S16 else np.float32)
        n = C.c_int64(0)
        self._grew(_at_16k(x.shape[0], sample_rate))
        check(self.lib.wlx_pcm_put_frames(self.engine._h, self.sid, item, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], fmt,
                                          int(sample_rate), C.byref(n)))
        self._grew(n.value)
        return n.value

    def put_frames_split(self, frames: np.ndarray, sample_rate: int, first_item: int = 0) -> int:
        """File frames [n, channels] (or a FlacFrames) -> channel c as 16 kHz mono float32 resident in item first_item + c: ONE upload,
        no down-mix, each item bit-identical to put_frames(frames[:, c]) (wlx_pcm_put_frames_split / wlx_pcm_put_flac_split).
        -> samples resident in each of the `channels` items. Raises WlxError (ERR_ARG) for a shape the device front end refuses and for
        first_item + channels > max_batch: nothing is launched, every item is left as it was."""
        if isinstance(frames, FlacFrames):
            n, info = C.c_int64(0), _lib.wlx_flac_info()
            self._grew(_at_16k(frames.total_samples, frames.sample_rate))
            check(self.lib.wlx_pcm_put_flac_split(self.engine._h, self.sid, first_item, frames.data, len(frames.data), C.byref(info), C.byref(n)))
            frames.info = info
            self._grew(n.value)
            return n.value
        x = np.asarray(frames)
        if x.ndim == 1:
            x = x[:, None]
        fmt = _lib.PCM_S16 if x.dtype == np.int16 else _lib.PCM_F32
        x = np.ascontiguousarray(x, dtype=np.int16 if fmt == _lib.PCM_S16 else np.float32)
        n = C.c_int64(0)
        self._grew(_at_16k(x.shape[0], sample_rate))
        check(self.lib.wlx_pcm_put_frames_split(self.engine._h, self.sid, first_item, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1],
                                                fmt, int(sample_rate), C.byref(n)))
        self._grew(n.value)
        return n.value

    def put_flac_split(self, data: bytes, first_item: int = 0):
        """The bytes of a FLAC file -> channel c resident in item first_item + c, decoded and resampled on the device with one split launch
        (wlx_pcm_put_flac_split); each item bit-identical to put_frames(audio_io.read_flac(data)[0][:, c]). -> (samples resident per
        item, info). WlxError codes as put_flac."""
        frames = FlacFrames(data)
        n = self.put_frames_split(frames, frames.sample_rate, first_item)
        return n, frames.info

    def put_flac(self, data: bytes, item: int = 0):
        """The bytes of a FLAC file -> 16 kHz mono float32 resident in the item's PCM buffer: indexed on the host, decoded, down-mixed and
        resampled on the device (wlx_pcm_put_flac); bit-identical to put_frames(audio_io.read_flac(data)). -> (samples resident, info)
        with info = the stream's shape (a _lib.wlx_flac_info). Raises WlxError: code ERR_ARG for a stream the device route does not
        serve (nothing launched, the item untouched: decode on the host), ERR_DATA for a damaged stream.
        It goes through put_frames, the one way file frames reach the slot: the frames are handed over still compressed (FlacFrames)."""
        frames = FlacFrames(data)
        n = self.put_frames(frames, frames.sample_rate, item)
        return n, frames.info

    def put_wav(self, data: bytes, item: int = 0):
        """The bytes of a G.711 (mu-law / A-law), IMA ADPCM or MS ADPCM WAV file -> 16 kHz mono float32 resident in the item's PCM
        buffer: probed on the host, decoded, down-mixed and resampled on the device (wlx_pcm_put_wav); bit-identical to
        put_frames(audio_io.read_wav(data)). -> (samples resident, info) with info = the file's shape (a _lib.wlx_wav_info). Raises
        WlxError: code ERR_ARG for a file the device route does not serve (any other tag among them; nothing launched, the item
        untouched: decode on the host), ERR_DATA for a damaged one."""
        data = bytes(data)
        n, info = C.c_int64(0), _lib.wlx_wav_info()
        self._grew(_wav_at_16k(data))
        check(self.lib.wlx_pcm_put_wav(self.engine._h, self.sid, item, data, len(data), C.byref(info), C.byref(n)))
        self._grew(n.value)
        return n.value, info

    def put_wav_split(self, data: bytes, first_item: int = 0):
        """put_wav without the down-mix: channel c resident in item first_item + c after one upload and one split launch
        (wlx_pcm_put_wav_split); each item bit-identical to put_frames(audio_io.read_wav(data)[0][:, c]). -> (samples resident per
        item, info). WlxError codes as put_wav."""
        data = bytes(data)
        n, info = C.c_int64(0), _lib.wlx_wav_info()
        self._grew(_wav_at_16k(data))
        check(self.lib.wlx_pcm_put_wav_split(self.engine._h, self.sid, first_item, data, len(data), C.byref(info), C.byref(n)))
        self._grew(n.value)
        return n.value, info

    def put_many(self, entries, first_item: int = 0, with_info: bool = False) -> list:
        """A wave of files and waveforms into items first_item, first_item + 1, ... with ONE wait (wlx_pcm_put_many). An entry is
        ("pcm", waveform) | ("frames", frames [n, channels], sample_rate) | ("flac", bytes) | ("wav", bytes): what pcm_put, put_frames,
        put_flac and put_wav take, and each item ends up bit-identical to that call's. -> per entry (samples resident, info or None), or
        the WlxError of that entry alone (code ERR_ARG: refused, its item untouched; ERR_DATA: damaged) — it is returned, not raised.
        info: the probe's wlx_flac_info / wlx_wav_info when `with_info` (a second pass over the file's bytes on the host), else None.
        More than _lib.PUT_MANY_MAX entries are cut into consecutive calls. A WlxError of a CALL (bad items, no memory, HIP) is raised."""
        out: list = []
        for at in range(0, len(entries), _lib.PUT_MANY_MAX):
            out += self._put_many_call(entries[at:at + _lib.PUT_MANY_MAX], first_item + at, with_info)
        return out

    def _put_many_call(self, entries, first_item: int, with_info: bool) -> list:
        n = len(entries)
        arr, res, keep = (_lib.wlx_put_entry * n)(), (_lib.wlx_put_result * n)(), []
        for k, ent in enumerate(entries):
            kind, x = ent[0], ent[1]
            if kind == "pcm":
                x = np.ascontiguousarray(x, dtype=np.float32)
                arr[k].kind, arr[k].data, arr[k].n = _lib.PUT_PCM, x.ctypes.data, x.shape[0]
                self._grew(x.shape[0])
            elif kind == "frames":
                x = np.asarray(x)
                if x.ndim == 1:
                    x = x[:, None]
                fmt = _lib.PCM_S16 if x.dtype == np.int16 else _lib.PCM_F32
                x = np.ascontiguousarray(x, dtype=np.int16 if fmt == _lib.PCM_S16 else np.float32)
                arr[k].kind, arr[k].data, arr[k].n = _lib.PUT_FRAMES, x.ctypes.data, x.shape[0]
                arr[k].channels, arr[k].sample_format, arr[k].sample_rate = x.shape[1], fmt, int(ent[2])
                self._grew(_at_16k(x.shape[0], int(ent[2])))
            elif kind in ("flac", "wav"):
                x = bytes(x)
                arr[k].kind, arr[k].n = (_lib.PUT_FLAC if kind == "flac" else _lib.PUT_WAV), len(x)
                arr[k].data = C.cast(C.c_char_p(x), C.c_void_p).value
                if kind == "flac":
                    head = FlacFrames(x)                  # (STREAMINFO's count and rate; the bytes are not copied)
                    self._grew(_at_16k(head.total_samples, head.sample_rate))
                else:
                    self._grew(_wav_at_16k(x))
            else:
                raise ValueError(f"put_many: unknown entry kind {kind!r} (pcm, frames, flac, wav)")
            keep.append(x)
        check(self.lib.wlx_pcm_put_many(self.engine._h, self.sid, first_item, n, arr, res))
        out = []
        for k, ent in enumerate(entries):
            if res[k].status != 0:
                err = WlxError(f"libwlx error {res[k].status}: put_many entry {k} ({ent[0]}) was "
                               f"{'refused' if res[k].status == _lib.ERR_ARG else 'found damaged'}")
                err.code = res[k].status
                out.append(err)
                continue
            self._grew(res[k].n_out)
            info = None
            if with_info and ent[0] == "flac":
                info = _lib.wlx_flac_info()
                check(self.lib.wlx_flac_probe(keep[k], len(keep[k]), C.byref(info)))
            elif with_info and ent[0] == "wav":
                info = _lib.wlx_wav_info()
                check(self.lib.wlx_wav_probe(keep[k], len(keep[k]), C.byref(info)))
            out.append((int(res[k].n_out), info))
        return out

    def pcm(self, item: int = 0) -> np.ndarray:
        """Host copy of the item's resident PCM (16 kHz mono float32)."""
        n = C.c_int64(0)
        check(self.lib.wlx_pcm_get(self.engine._h, self.sid, item, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        if n.value:
            check(self.lib.wlx_pcm_get(self.engine._h, self.sid, item, _f32p(out), out.size, C.byref(n)))
        return out

    def pcm_count(self, item: int = 0) -> int:
        """samples of PCM resident in the item (0: none)"""
        n = C.c_int64(0)
        check(self.lib.wlx_pcm_get(self.engine._h, self.sid, item, None, 0, C.byref(n)))
        return n.value

    def logmel_ring(self, ring: "PcmRing", ranges: Sequence[Tuple[int, int]], item: int = 0) -> int:
        """log-mel of the concatenation of ring ranges [(start, end), ...] (absolute positions) -> frames; see wlx_logmel_ring"""
        rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        nf = C.c_int32(0)
        self._grew(int((rg[:, 1] - rg[:, 0]).sum()) if rg.size else 0)
        check(self.lib.wlx_logmel_ring(self.engine._h, self.sid, item, ring._h, rg.ctypes.data_as(C.POINTER(C.c_int64)), rg.shape[0], C.byref(nf)))
        return nf.value

    def logmel_chunks(self, chunks: Sequence[Sequence[Tuple[int, int]]], src_item: Union[int, Sequence[int]] = 0,
                      first_item: int = 0) -> List[int]:
        """One launch of each log-mel kernel for len(chunks) chunks of the resident PCM of `src_item`: chunk c = the concatenation of
        its [(start, end), ...] sample ranges -> features of item first_item + c. -> frames per chunk; see wlx_logmel_chunks.
        A sequence `src_item` names one source item PER CHUNK (the channels of a file): wlx_logmel_chunks_multi, still one launch."""
        off = np.zeros(len(chunks) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in chunks])
        rg = np.ascontiguousarray(np.asarray([r for c in chunks for r in c], dtype=np.int64).reshape(-1, 2))
        nf = np.zeros(max(1, len(chunks)), dtype=np.int32)
        if not isinstance(src_item, (int, np.integer)):
            src = np.ascontiguousarray(list(src_item), dtype=np.int32)
            if src.shape != (len(chunks),):
                raise ValueError(f"{src.size} source items for {len(chunks)} chunks")
            check(self.lib.wlx_logmel_chunks_multi(self.engine._h, self.sid, _i32p(src), rg.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(off),
                                                   len(chunks), first_item, _i32p(nf)))
            return nf[: len(chunks)].tolist()
        check(self.lib.wlx_logmel_chunks(self.engine._h, self.sid, src_item, rg.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(off),
                                         len(chunks), first_item, _i32p(nf)))
        return nf[: len(chunks)].tolist()

    def logmel_resident(self, item: int = 0) -> int:
        nf = C.c_int32(0)
        check(self.lib.wlx_logmel_resident(self.engine._h, self.sid, item, C.byref(nf)))
        return nf.value

    def features(self, item: int = 0) -> np.ndarray:
        nf = C.c_int32(0)
        check(self.lib.wlx_features_get(self.engine._h, self.sid, item, None, 0, C.byref(nf)))
        out = np.empty((self.engine.spec.n_mels, nf.value), dtype=np.float32)
        check(self.lib.wlx_features_get(self.engine._h, self.sid, item, _f32p(out), out.size, C.byref(nf)))
        return out

    def set_features(self, feats: np.ndarray, item: int = 0):
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        self._grew(feats.shape[-1] * 160)
        check(self.lib.wlx_features_set(self.engine._h, self.sid, item, _f32p(feats), feats.shape[0], feats.shape[1]))

    # ---- encoder
    def encode(self, batch: int = 1, seek: Optional[Sequence[int]] = None, seg: Optional[Sequence[int]] = None):
        sk = np.asarray(seek if seek is not None else [0] * batch, dtype=np.int32)
        if seg is None:
            sg_p = None
        else:
            sg = np.asarray(seg, dtype=np.int32)
            sg_p = _i32p(sg)
        check(self.lib.wlx_encode(self.engine._h, self.sid, batch, _i32p(sk), sg_p))

    def encoder_output(self, item: int = 0) -> np.ndarray:
        out = np.empty((self.engine.spec.n_audio_ctx, self.engine.spec.d_model), dtype=np.float32)
        check(self.lib.wlx_encoder_output_get(self.engine._h, self.sid, item, _f32p(out), out.size))
        return out

    # ---- decoder
    def _opts(self, ids: TokenIds, beam_size, patience, num_hypotheses, length_penalty, repetition_penalty,
              no_repeat_ngram_size, max_length, suppress_blank, suppress_tokens, max_initial_timestamp_index,
              sampling_topk, sampling_temperature, seed):
        o = _lib.wlx_gen_opts()
        o.beam_size, o.patience, o.num_hypotheses = int(beam_size), float(patience), int(num_hypotheses)
        o.length_penalty, o.repetition_penalty = float(length_penalty), float(repetition_penalty)
        o.no_repeat_ngram_size, o.max_length = int(no_repeat_ngram_size), int(max_length)
        o.suppress_blank = 1 if suppress_blank else 0
        st = np.asarray(list(suppress_tokens) if suppress_tokens is not None else [], dtype=np.int32)
        o.suppress_tokens = _i32p(st) if st.size else None
        o.n_suppress_tokens = int(st.size)
        o.max_initial_timestamp_index = int(max_initial_timestamp_index)
        o.sampling_topk, o.sampling_temperature, o.seed = int(sampling_topk), float(sampling_temperature), int(seed)
        o.ids = _lib.wlx_token_ids(ids.sot, ids.eot, ids.no_timestamps, ids.timestamp_begin, ids.no_speech, ids.blank)
        return o, st

    def generate(self, prompts: Sequence[Sequence[int]], ids: TokenIds, *, beam_size=5, patience=1.0, num_hypotheses=1,
                 length_penalty=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, max_length=448,
                 suppress_blank=True, suppress_tokens=(), max_initial_timestamp_index=50, sampling_topk=0,
                 sampling_temperature=0.0, seed=0, enc_items: Optional[Sequence[int]] = None) -> List[GenerationResult]:
        batch = len(prompts)
        o, keep = self._opts(ids, beam_size, patience, num_hypotheses, length_penalty, repetition_penalty,
                             no_repeat_ngram_size, max_length, suppress_blank, suppress_tokens,
                             max_initial_timestamp_index, sampling_topk, sampling_temperature, seed)
        stride = max(len(p) for p in prompts)
        pr = np.zeros((batch, stride), dtype=np.int32)
        pl = np.zeros(batch, dtype=np.int32)
        for i, p in enumerate(prompts):
            pr[i, :len(p)] = p
            pl[i] = len(p)
        nh = max(1, int(num_hypotheses))
        toks = np.zeros((batch, nh, 448), dtype=np.int32)
        nt = np.zeros((batch, nh), dtype=np.int32)
        sc = np.zeros((batch, nh), dtype=np.float32)
        nsp = np.zeros(batch, dtype=np.float32)
        items = np.asarray(enc_items, dtype=np.int32) if enc_items is not None else None
        check(self.lib.wlx_generate_ex(self.engine._h, self.sid, batch, _i32p(items) if items is not None else None,
                                       _i32p(pr), _i32p(pl), stride, C.byref(o),
                                       _i32p(toks), 448, _i32p(nt), _f32p(sc), _f32p(nsp)))
        out = []
        for b in range(batch):
            seqs = [toks[b, h, :nt[b, h]].tolist() for h in range(nh) if np.isfinite(sc[b, h])]
            scores = [float(sc[b, h]) for h in range(nh) if np.isfinite(sc[b, h])]
            out.append(GenerationResult(seqs, scores, float(nsp[b])))
        return out

    # ---- keyword boosting
    def set_bias(self, table) -> None:
        """Install a biasing.BiasTable on the slot (wlx_bias_set): every decode step of its generate calls, and of the debug_search
        hooks, then runs the bias launch in front of the search. The buffers sit at fixed addresses: captured step graphs are re-used
        across tables. WlxError (ERR_ARG) for a table the library refuses; the installed one stays."""
        if table.vocab != self.engine.spec.vocab:
            raise ValueError(f"the bias table was compiled for a vocabulary of {table.vocab}, the model has {self.engine.spec.vocab}")
        off, tok, nxt = (np.ascontiguousarray(a, dtype=np.int32) for a in (table.edge_off, table.edge_tok, table.edge_next))
        ids, vals = np.ascontiguousarray(table.tok_ids, dtype=np.int32), np.ascontiguousarray(table.tok_vals, dtype=np.float32)
        check(self.lib.wlx_bias_set(self.engine._h, self.sid, table.n_nodes, _i32p(off), _i32p(tok), _i32p(nxt), float(table.boost),
                                    ids.size, _i32p(ids), _f32p(vals)))
        self._bias_table, self._grammar = table, None       # (one mode at a time: the last set call decides)

    def set_bias_items(self, bias_set) -> None:
        """Install a biasing.BiasSet on the slot (wlx_bias_set_items): the slot decodes in per-item mode, every item deselected until
        `select_bias`. WlxError (ERR_ARG) for a set the library refuses; whatever is installed stays."""
        if len(bias_set) < 1:
            raise ValueError("an empty BiasSet installs nothing: clear_bias")
        if bias_set.vocab != self.engine.spec.vocab:
            raise ValueError(f"the bias set was compiled for a vocabulary of {bias_set.vocab}, the model has {self.engine.spec.vocab}")
        nn, off, tok, nxt, boosts, nt, ids, vals = bias_set.packed()
        check(self.lib.wlx_bias_set_items(self.engine._h, self.sid, len(bias_set), _i32p(nn), _i32p(off), _i32p(tok), _i32p(nxt),
                                          _f32p(boosts), _i32p(nt), _i32p(ids), _f32p(vals)))
        self._bias_table, self._bias_set_version, self._grammar = bias_set, bias_set.version, None

    def select_bias(self, indices: Sequence[int]) -> None:
        """indices[b]: the table (an index into the installed set, -1: none) of item b of the following generate calls (wlx_bias_select)"""
        sel = np.ascontiguousarray(list(indices), dtype=np.int32)
        check(self.lib.wlx_bias_select(self.engine._h, self.sid, sel.size, _i32p(sel)))

    def clear_bias(self) -> None:
        """Decode without a bias table again (wlx_bias_clear)."""
        check(self.lib.wlx_bias_clear(self.engine._h, self.sid))
        self._bias_table = self._grammar = None

    # ---- grammar-constrained decoding
    def set_grammar(self, grammar) -> None:
        """Install a grammar.Grammar on the slot (wlx_grammar_set): every decode step of its generate calls, and of the debug_search
        hooks, then runs the grammar launch in front of the search, in place of a keyword table's (one mode at a time). The buffers sit
        at fixed addresses: captured step graphs are re-used across grammars. WlxError (ERR_ARG) for a table the library refuses; what is
        installed stays."""
        if grammar.vocab != self.engine.spec.vocab:
            raise ValueError(f"the grammar was compiled for a vocabulary of {grammar.vocab}, the model has {self.engine.spec.vocab}")
        off, tok, nxt, acc = (np.ascontiguousarray(a, dtype=np.int32) for a in (grammar.edge_off, grammar.edge_tok, grammar.edge_next, grammar.accept))
        check(self.lib.wlx_grammar_set(self.engine._h, self.sid, int(grammar.eot), grammar.n_states, _i32p(off), _i32p(tok), _i32p(nxt), _i32p(acc)))
        self._grammar, self._bias_table = grammar, None

    def clear_grammar(self) -> None:
        """Decode without a grammar again (wlx_grammar_clear): the step is the launch list of a slot that never had one."""
        check(self.lib.wlx_grammar_clear(self.engine._h, self.sid))
        self._grammar = None

    def align(self, tokens: Sequence[int], n_sot: int, num_frames: int, heads: Sequence[Tuple[int, int]], eot: int,
              median_filter_width: int = 7, item: int = 0):
        """ctranslate2 Whisper.align for one encoded item: tokens = start_sequence + [no_timestamps] + text + [eot].
        Returns (text_indices, time_indices, text_token_probs)."""
        tk = np.ascontiguousarray(tokens, dtype=np.int32)
        hd = np.ascontiguousarray(np.asarray(heads, dtype=np.int32).reshape(-1, 2))
        cap = tk.size + 1500 + 8
        ti = np.zeros(cap, dtype=np.int32)
        fi = np.zeros(cap, dtype=np.int32)
        n_path = C.c_int32(0)
        probs = np.zeros(max(1, tk.size - n_sot - 2), dtype=np.float32)
        check(self.lib.wlx_align(self.engine._h, self.sid, item, _i32p(tk), tk.size, n_sot, int(num_frames), int(median_filter_width),
                                 _i32p(hd), hd.shape[0], int(eot), _i32p(ti), _i32p(fi), cap, C.byref(n_path), _f32p(probs)))
        return ti[: n_path.value].copy(), fi[: n_path.value].copy(), probs

    def align_batch(self, token_lists: Sequence[Sequence[int]], n_sot: int, num_frames: Sequence[int], heads: Sequence[Tuple[int, int]],
                    eot: int, median_filter_width: int = 7, items: Optional[Sequence[int]] = None):
        """`align` for a group of entries in one wlx_align_batch call (one launch sequence, one wait; softmax / median / DTW on the
        device): entry i is token_lists[i] over num_frames[i] on encoder item items[i] (None = identity, repeats allowed).
        Returns one (text_indices, time_indices, text_token_probs) per entry. At most _lib.ALIGN_MAX_BATCH entries, odd filter
        widths up to _lib.ALIGN_MAX_MEDIAN."""
        n = len(token_lists)
        if n == 0:
            return []
        nt = np.asarray([len(t) for t in token_lists], dtype=np.int32)
        stride = int(nt.max())
        tk = np.zeros((n, stride), dtype=np.int32)
        for i, t in enumerate(token_lists):
            tk[i, :nt[i]] = t
        nfr = np.ascontiguousarray(num_frames, dtype=np.int32)
        if nfr.shape != (n,):
            raise ValueError(f"{nfr.size} num_frames for {n} entries")
        it = np.ascontiguousarray(items, dtype=np.int32) if items is not None else None
        if it is not None and it.shape != (n,):
            raise ValueError(f"{it.size} items for {n} entries")
        hd = np.ascontiguousarray(np.asarray(heads, dtype=np.int32).reshape(-1, 2))
        cap = stride + 1500 + 8
        ti = np.zeros((n, cap), dtype=np.int32)
        fi = np.zeros((n, cap), dtype=np.int32)
        n_path = np.zeros(n, dtype=np.int32)
        pstride = max(1, stride - n_sot - 2)
        probs = np.zeros((n, pstride), dtype=np.float32)
        check(self.lib.wlx_align_batch(self.engine._h, self.sid, n, _i32p(it) if it is not None else None, _i32p(tk), _i32p(nt), stride,
                                       n_sot, _i32p(nfr), int(median_filter_width), _i32p(hd), hd.shape[0], int(eot),
                                       _i32p(ti), _i32p(fi), cap, _i32p(n_path), _f32p(probs), pstride))
        return [(ti[i, : n_path[i]].copy(), fi[i, : n_path[i]].copy(), probs[i, : max(0, int(nt[i]) - n_sot - 2)].copy()) for i in range(n)]

    def align_timings(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last align_batch: (decoder passes with the score capture, post-processing behind them)"""
        a, b = C.c_float(0), C.c_float(0)
        check(self.lib.wlx_debug_align_timings(self.engine._h, self.sid, C.byref(a), C.byref(b)))
        return a.value, b.value

    def detect_language(self, batch: int, sot: int, lang_ids: Sequence[int]) -> np.ndarray:
        li = np.asarray(lang_ids, dtype=np.int32)
        probs = np.zeros((batch, li.size), dtype=np.float32)
        check(self.lib.wlx_detect_language(self.engine._h, self.sid, batch, sot, _i32p(li), li.size, _f32p(probs)))
        return probs

    def timings(self) -> dict:
        t = _lib.wlx_timings()
        check(self.lib.wlx_timings_get(self.engine._h, self.sid, C.byref(t)))
        return {"logmel_ms": t.logmel_ms, "encode_ms": t.encode_ms, "generate_ms": t.generate_ms, "decode_steps": t.decode_steps}

    # ---- test hooks
    def debug_decode_logits(self, tokens: Sequence[int]) -> np.ndarray:
        tk = np.asarray(tokens, dtype=np.int32)
        out = np.empty((tk.size, self.engine.spec.vocab), dtype=np.float32)
        check(self.lib.wlx_debug_decode_logits(self.engine._h, self.sid, _i32p(tk), tk.size, _f32p(out)))
        return out

    def debug_logits(self, rows: int) -> np.ndarray:
        """the slot's logits buffer [rows, V] as the LAST decoder pass left it (wlx_debug_logits_get)"""
        out = np.empty((rows, self.engine.spec.vocab), dtype=np.float32)
        check(self.lib.wlx_debug_logits_get(self.engine._h, self.sid, _f32p(out), rows, out.size))
        return out

    def debug_search(self, logits: np.ndarray, prompt: Sequence[int], ids: TokenIds, **kw) -> GenerationResult:
        logits = np.ascontiguousarray(logits, dtype=np.float32)   # [steps, rows, V]
        d = dict(beam_size=5, patience=1.0, num_hypotheses=1, length_penalty=1.0, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, max_length=448, suppress_blank=True, suppress_tokens=(),
                 max_initial_timestamp_index=50, sampling_topk=0, sampling_temperature=0.0, seed=0)
        d.update(kw)
        o, keep = self._opts(ids, **d)
        pr = np.asarray(prompt, dtype=np.int32)
        nh = max(1, int(d["num_hypotheses"]))
        toks = np.zeros((nh, 448), dtype=np.int32)
        nt = np.zeros(nh, dtype=np.int32)
        sc = np.zeros(nh, dtype=np.float32)
        check(self.lib.wlx_debug_search(self.engine._h, self.sid, _f32p(logits), logits.shape[0], _i32p(pr), pr.size,
                                        C.byref(o), _i32p(toks), 448, _i32p(nt), _f32p(sc)))
        seqs = [toks[h, :nt[h]].tolist() for h in range(nh) if np.isfinite(sc[h])]
        return GenerationResult(seqs, [float(x) for x in sc if np.isfinite(x)], 0.0)

    def debug_search_batch(self, logits: np.ndarray, prompts: Sequence[Sequence[int]], ids: TokenIds, **kw) -> List[GenerationResult]:
        """`debug_search` for len(prompts) items in one call: logits [steps, items * R, V], item b's rows are [b * R, (b + 1) * R)
        (R = beam_size in beam mode, num_hypotheses when sampling)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        d = dict(beam_size=5, patience=1.0, num_hypotheses=1, length_penalty=1.0, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, max_length=448, suppress_blank=True, suppress_tokens=(),
                 max_initial_timestamp_index=50, sampling_topk=0, sampling_temperature=0.0, seed=0)
        d.update(kw)
        o, keep = self._opts(ids, **d)
        batch = len(prompts)
        stride = max(len(p) for p in prompts)
        pr = np.zeros((batch, stride), dtype=np.int32)
        pl = np.zeros(batch, dtype=np.int32)
        for i, p in enumerate(prompts):
            pr[i, :len(p)] = p
            pl[i] = len(p)
        nh = max(1, int(d["num_hypotheses"]))
        toks = np.zeros((batch, nh, 448), dtype=np.int32)
        nt = np.zeros((batch, nh), dtype=np.int32)
        sc = np.zeros((batch, nh), dtype=np.float32)
        check(self.lib.wlx_debug_search_batch(self.engine._h, self.sid, _f32p(logits), logits.shape[0], batch, _i32p(pr), _i32p(pl), stride,
                                              C.byref(o), _i32p(toks), 448, _i32p(nt), _f32p(sc)))
        return [GenerationResult([toks[b, h, :nt[b, h]].tolist() for h in range(nh) if np.isfinite(sc[b, h])],
                                 [float(sc[b, h]) for h in range(nh) if np.isfinite(sc[b, h])], 0.0) for b in range(batch)]

    def debug_time_decode_step(self, rows: int, t: int, iters: int = 50) -> float:
        ms = C.c_float(0)
        check(self.lib.wlx_debug_time_decode_step(self.engine._h, self.sid, rows, t, iters, C.byref(ms)))
        return ms.value

    def debug_profile_step(self, rows: int, t: int, iters: int = 20) -> List[dict]:
        cap = 64
        arr = (_lib.wlx_kernel_stat * cap)()
        n = C.c_int32(0)
        check(self.lib.wlx_debug_profile_step(self.engine._h, self.sid, rows, t, iters, arr, cap, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches_per_step, avg_us=arr[i].avg_us,
                     total_us=arr[i].total_us_per_step, bytes_per_launch=arr[i].bytes_per_launch) for i in range(n.value)]

    def debug_trace_step(self, rows: int, t: int, with_search: bool = True):
        """In-kernel timeline of one decode step (libwlx_trace.so only). Returns (names, records[n][2049][8] u64); record 0 of a launch is unused."""
        stride = (2048 + 1) * 8
        cap_launch = 320
        buf = np.zeros(cap_launch * stride, dtype=np.uint64)
        names = C.create_string_buffer(cap_launch * 48)
        n = C.c_int32(0)
        check(self.lib.wlx_debug_trace_step(self.engine._h, self.sid, rows, t, 1 if with_search else 0,
                                            buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size, names, C.byref(n)))
        nl = n.value
        nm = [names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode() for i in range(nl)]
        return nm, buf[: nl * stride].reshape(nl, 2049, 8)
