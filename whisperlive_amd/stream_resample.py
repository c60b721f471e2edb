"""Host restatement of the live path's stream resampler (include/wlx.h wlx_ring_append_frames; csrc/resample.hip, the stream form).

A live session may announce its own wire format — ``sample_rate``, ``channels`` and ``audio_format`` (float32, int16, uint8, G.711
mu-law / A-law) in its first JSON message — and send its packets as they come off the capture device or the telephony leg. The
device converts, down-mixes and resamples them packet by packet. ``StreamResampler`` is the same stream on the host, in float64:

* the fallback of a wire-format session that has no device ring (a scripted engine, a ring switched off after an error) — the
  session keeps J, M and the raw tail HERE at all times (``advance``), so the fallback takes over at any packet boundary without a
  gap or a repeated sample;
* the CPU oracle of the tests: ``feed`` ... ``flush`` over ANY cutting of a stream equals scipy.signal.resample_poly of the whole.

Rule of the stream (up / down = 16000 / rate reduced, half_len = 10 * max(up, down), 0 at 16 kHz): with J' input frames seen, the
outputs that exist are those whose newest input does, floor((half_len + m * down) / up) <= J' - 1; a flush completes them to the
one-shot length ceil(J' * up / down) with zeros behind the end. Output m = sum_j mono[j] * h[half_len + m * down - j * up], h =
up * firwin(2 * half_len + 1, 1 / max(up, down), window = ("kaiser", 5.0)): scipy.signal.resample_poly's default filter, which is
what audio_io.load_audio applies to a file."""
from __future__ import annotations

from math import gcd
from typing import Tuple, Union

import numpy as np

from . import _lib
from .engine import resample_supported

TARGET_RATE = 16000
# protocol name -> (wlx.h sample-format code, numpy dtype of one sample on the wire)
WIRE_FORMATS = {
    "float32": (_lib.PCM_F32, np.dtype("<f4")),
    "int16": (_lib.PCM_S16, np.dtype("<i2")),
    "uint8": (_lib.PCM_U8, np.dtype(np.uint8)),
    "mulaw": (_lib.PCM_MULAW, np.dtype(np.uint8)),
    "alaw": (_lib.PCM_ALAW, np.dtype(np.uint8)),
}
_BY_CODE = {code: (name, dt) for name, (code, dt) in WIRE_FORMATS.items()}


def ratio(rate: int) -> Tuple[int, int]:
    g = gcd(TARGET_RATE, int(rate))
    return TARGET_RATE // g, int(rate) // g


def half_len(up: int, down: int) -> int:
    return 0 if up == down else 10 * max(up, down)


def reach(up: int, down: int) -> int:
    """input frames of history an output can need (csrc/resample.hip resample_reach): ceil(2 half_len / up) + 2"""
    return -(-2 * half_len(up, down) // up) + 2


def stream_count(rate: int, frames_seen: int, flush: bool = False) -> int:
    """M' as a function of J' alone (wlx_resample_stream_count)"""
    up, down = ratio(rate)
    if flush:
        return -(-frames_seen * up // down)
    a = frames_seen * up - 1 - half_len(up, down)
    return 0 if a < 0 else a // down + 1


def decode_mulaw(codes) -> np.ndarray:
    """G.711 mu-law bytes -> their 16-bit linear values (int32), the kernel's integer arithmetic"""
    u = (~np.asarray(codes, dtype=np.uint8)).astype(np.int32) & 255
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return np.where(u & 128, 132 - t, t - 132).astype(np.int32)


def decode_alaw(codes) -> np.ndarray:
    """G.711 A-law bytes -> their 16-bit linear values (int32)"""
    a = (np.asarray(codes, dtype=np.uint8).astype(np.int32) ^ 0x55) & 255
    s = (a >> 4) & 7
    t = (a & 15) << 4
    t = np.where(s == 0, t + 8, (t + 0x108) << np.maximum(s - 1, 0))
    return np.where(a & 128, t, -t).astype(np.int32)


def decode_samples(x: np.ndarray, code: int) -> np.ndarray:
    """wire samples of format `code` -> float32, every value exact"""
    if code == _lib.PCM_F32:
        return np.asarray(x, dtype=np.float32)
    if code == _lib.PCM_S16:
        return x.astype(np.float32) * np.float32(1.0 / 32768.0)
    if code == _lib.PCM_U8:
        return (x.astype(np.int32) - 128).astype(np.float32) * np.float32(1.0 / 128.0)
    lin = decode_mulaw(x) if code == _lib.PCM_MULAW else decode_alaw(x)
    return lin.astype(np.float32) * np.float32(1.0 / 32768.0)


def mono_f32(frames: np.ndarray, code: int) -> np.ndarray:
    """[n, channels] wire frames -> the kernel's mono: the float32 mean, channels added in order, one division"""
    x = decode_samples(frames, code)
    s = x[:, 0].copy()
    if x.shape[1] > 1:
        for c in range(1, x.shape[1]):
            s = s + x[:, c]
        s = s / np.float32(x.shape[1])
    return s.astype(np.float32)


def _i0(x: np.ndarray) -> np.ndarray:
    q = 0.25 * x * x
    term, s = np.ones_like(x), np.ones_like(x)
    for k in range(1, 60):
        term = term * q / (k * k)
        s = s + term
    return s


def design(up: int, down: int) -> np.ndarray:
    """float64 taps [2 half_len + 1] = up * firwin(2 half_len + 1, 1 / max(up, down), window=("kaiser", 5.0)); [1.0] at 16 kHz"""
    if up == down:
        return np.ones(1)
    mx, hl = max(up, down), half_len(up, down)
    m = np.arange(-hl, hl + 1, dtype=np.float64)
    a = np.pi * m / mx
    sinc = np.ones_like(m)
    nz = m != 0
    sinc[nz] = np.sin(a[nz]) / a[nz]
    w = _i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (m / hl) ** 2))) / _i0(np.array([5.0]))[0]
    h = sinc / mx * w
    return up * (h / h.sum())


def check_format(audio_format: Union[str, int], channels: int, rate: int) -> Tuple[int, np.dtype]:
    """-> (format code, sample dtype); ValueError for what wlx_ring_set_format refuses"""
    ent = WIRE_FORMATS.get(audio_format) if isinstance(audio_format, str) else \
        ((audio_format, _BY_CODE[audio_format][1]) if audio_format in _BY_CODE else None)
    if ent is None:
        raise ValueError(f"Unsupported audio_format: {audio_format}")
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= _lib.PCM_MAX_CHANNELS:
        raise ValueError(f"Unsupported channels: {channels} (1..{_lib.PCM_MAX_CHANNELS})")
    if isinstance(rate, bool) or not isinstance(rate, int) or not resample_supported(rate, channels):
        raise ValueError(f"Unsupported sample_rate: {rate} Hz is not a rate the device resampler serves")
    return ent


def packet_frames(raw, dtype: np.dtype, channels: int) -> np.ndarray:
    """a packet (bytes, or an array of wire samples, interleaved) -> [n, channels]; ValueError when it does not hold whole frames"""
    if isinstance(raw, (bytes, bytearray, memoryview)):
        fb = channels * dtype.itemsize
        if len(raw) % fb:
            raise ValueError(f"packet of {len(raw)} bytes is not a whole number of {fb}-byte frames")
        x = np.frombuffer(raw, dtype=dtype)
    else:
        x = np.asarray(raw)
        if x.dtype != dtype:
            raise ValueError(f"packet of dtype {x.dtype}, the stream's format takes {dtype}")
        if x.size % channels:
            raise ValueError(f"packet of {x.size} samples is not a whole number of {channels}-channel frames")
    return x.reshape(-1, channels)


class StreamResampler:
    """One stream: J frames seen, M outputs emitted, the raw tail (the last <= reach frames, in the wire format)."""

    def __init__(self, audio_format: Union[str, int], channels: int, rate: int):
        self.code, self.dtype = check_format(audio_format, channels, rate)
        self.channels, self.rate = channels, rate
        self.up, self.down = ratio(rate)
        self.half_len, self.reach = half_len(self.up, self.down), reach(self.up, self.down)
        self.J = self.M = 0
        self.closed = False
        self.tail = np.zeros((0, channels), self.dtype)
        self._h = None

    @property
    def frame_bytes(self) -> int:
        return self.channels * self.dtype.itemsize

    def frames(self, raw) -> np.ndarray:
        return packet_frames(raw, self.dtype, self.channels)

    def _step(self, raw, flush: bool, compute: bool):
        if self.closed:
            raise RuntimeError("the stream has been flushed")
        x = self.frames(raw)
        n = x.shape[0]
        m1 = stream_count(self.rate, self.J + n, flush)
        win = np.concatenate((self.tail, x), axis=0) if n else self.tail
        out = self._outputs(win, self.J - self.tail.shape[0], self.J + n, self.M, m1) if compute else None
        if n:
            self.tail = win[max(0, win.shape[0] - self.reach):].copy()
        n_new = m1 - self.M
        self.J += n
        self.M = m1
        self.closed = bool(flush)
        return out, n_new

    def _outputs(self, win: np.ndarray, j_base: int, j_end: int, m0: int, m1: int) -> np.ndarray:
        if m1 <= m0:
            return np.zeros(0, np.float32)
        mono = mono_f32(win, self.code)
        m = np.arange(m0, m1, dtype=np.int64)
        if self.half_len == 0:
            return mono[m - j_base].copy()
        if self._h is None:
            self._h = design(self.up, self.down)
        x64 = mono.astype(np.float64)
        t = self.half_len + m * self.down
        jh = t // self.up
        ph = t - jh * self.up
        acc = np.zeros(m.shape[0], np.float64)
        # oldest input first, as upfirdn adds them (the order only matters to the last bits of a float64 sum)
        for k in range(int(((2 * self.half_len - ph) // self.up).max()), -1, -1):
            j, idx = jh - k, ph + k * self.up
            ok = (j >= max(j_base, 0)) & (j < j_end) & (idx <= 2 * self.half_len)
            xv = np.where(ok, x64[np.clip(j - j_base, 0, max(x64.shape[0] - 1, 0))] if x64.shape[0] else 0.0, 0.0)
            acc += xv * np.where(ok, self._h[np.clip(idx, 0, 2 * self.half_len)], 0.0)
        return acc.astype(np.float32)

    def feed(self, raw, flush: bool = False) -> np.ndarray:
        """-> the packet's new 16 kHz samples (float32); flush=True also closes the stream"""
        return self._step(raw, flush, True)[0]

    def advance(self, raw, flush: bool = False) -> int:
        """book-keeping only (the device computed the samples): -> how many outputs the packet completed"""
        return self._step(raw, flush, False)[1]

    def flush(self) -> np.ndarray:
        return self.feed(np.zeros((0, self.channels), self.dtype), flush=True)


class ChannelStreamResamplers:
    """The host route and CPU oracle of a MULTICHANNEL live stream (include/wlx.h wlx_ring_group_append_frames): one StreamResampler
    per channel over that channel's column of the de-interleaved packet — no mean, no division. All channels see the same cutting, so
    J, M and `closed` are the same on every one of them; `advance` keeps them in step while the device computes the samples."""

    def __init__(self, audio_format: Union[str, int], channels: int, rate: int):
        self.code, self.dtype = check_format(audio_format, channels, rate)
        self.channels, self.rate = channels, rate
        self.lanes = [StreamResampler(audio_format, 1, rate) for _ in range(channels)]

    @property
    def frame_bytes(self) -> int:
        return self.channels * self.dtype.itemsize

    @property
    def J(self) -> int:
        return self.lanes[0].J

    @property
    def M(self) -> int:
        return self.lanes[0].M

    @property
    def closed(self) -> bool:
        return self.lanes[0].closed

    def frames(self, raw) -> np.ndarray:
        return packet_frames(raw, self.dtype, self.channels)

    def feed(self, raw, flush: bool = False) -> list:
        """-> per channel, the packet's new 16 kHz samples (float32)"""
        x = self.frames(raw)
        return [ln.feed(np.ascontiguousarray(x[:, c]), flush) for c, ln in enumerate(self.lanes)]

    def advance(self, raw, flush: bool = False) -> int:
        """book-keeping only: -> how many outputs per channel the packet completed"""
        x = self.frames(raw)
        return [ln.advance(np.ascontiguousarray(x[:, c]), flush) for c, ln in enumerate(self.lanes)][0]
