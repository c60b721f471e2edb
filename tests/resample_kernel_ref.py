"""numpy restatement of the audio front end's kernel (csrc/resample.hip) and the ctypes runner of its one-launch-per-block hook
(wlx_debug_resample).

The restatement computes exactly what the kernel computes: taps designed in float64 WITHOUT scipy (sinc x Kaiser(5.0), unit gain at
DC, times `up`), rounded to float32 once; mono = the float32 channel mean (channels added in order, one division); output m
accumulated in float32 over k = 0, 1, ... of mono[jh - k] * h[ph + k * up] with jh = (half_len + m * down) // up and ph the
remainder, each step one fused multiply-add (the float64 product of two float32 values is exact, so float32(float64 sum) is the
fused result up to a double rounding that needs a 29-bit tie).

RESAMPLE_ATOL is the bound of every comparison against scipy.signal.resample_poly on float64 input, on the GPU too. It comes from
this restatement's own error, not from the kernel: tests/test_resample_ref.py measures the restatement's largest absolute error
against scipy over the grid below (every rate, the edge lengths, speech-like input of peak 1 and unit impulses) and asserts that it
stays within a quarter of the constant. The factor four is the room for a kernel that orders its float32 sums differently: the
error of a float32 sum of n terms grows like sqrt(n) to n roundings, reordering about 60 terms stays well inside 4x."""
from __future__ import annotations

import ctypes as C
from math import gcd

import numpy as np

RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000]
# measured: 7.371e-7 (the restatement against scipy's float64 result, largest over the whole grid: 192000 Hz, 241 taps per output,
# speech-like input, 3 s + 1 frame); four times that, rounded up in the third digit
RESAMPLE_ATOL = 2.95e-6
# The steep down-sampling rates the kernel serves with a smaller tile (1024 outputs' input span would not fit its LDS): more taps per
# output than any rate above, so a bound of their own, derived the same way over the same grid with 1 s + 1 frame as the long length.
# measured: 9.136e-7 (384000 Hz, 481 taps per output, speech-like input, 1 s + 1 frame); four times that, rounded up
STEEP_RATES = [176400, 352800, 384000]
RESAMPLE_ATOL_STEEP = 3.66e-6
# the steepest ratio the kernel serves (1 / 159: the tap table and the span of 64 outputs are 16380 of the 16384 floats of LDS) and
# the first it refuses for its LDS (1 / 160)
STEEPEST_RATE, FIRST_REFUSED_STEEP_RATE = 2544000, 2560000
F32, S16 = 0, 1
ERR_ARG = 1
MAX_CHANNELS = 8


def ratio(rate: int):
    g = gcd(16000, rate)
    return 16000 // g, rate // g


def _i0(x: np.ndarray) -> np.ndarray:
    q = 0.25 * x * x
    term, s = np.ones_like(x), np.ones_like(x)
    for k in range(1, 60):
        term = term * q / (k * k)
        s = s + term
    return s


def design(up: int, down: int):
    """-> (half_len, float64 taps [2 half_len + 1]) = up * firwin(2 half_len + 1, 1 / max(up, down), window=("kaiser", 5.0))"""
    if up == down:
        return 0, np.ones(1)
    mx = max(up, down)
    hl = 10 * mx
    m = np.arange(-hl, hl + 1, dtype=np.float64)
    a = np.pi * m / mx
    sinc = np.ones_like(m)
    nz = m != 0
    sinc[nz] = np.sin(a[nz]) / a[nz]
    w = _i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (m / hl) ** 2))) / _i0(np.array([5.0]))[0]
    h = sinc / mx * w
    return hl, up * (h / h.sum())


def out_len(n: int, up: int, down: int) -> int:
    return -(-n * up // down)


def reach(up: int, down: int) -> int:
    """the smallest legal block_frames (include/wlx.h): ceil(2 half_len / up) + 2"""
    hl = 0 if up == down else 10 * max(up, down)
    return -(-2 * hl // up) + 2


def mono_f32(frames: np.ndarray) -> np.ndarray:
    """[n, ch] int16 / float32 -> the kernel's mono: S16 scaled by 1 / 32768, channels added in order in float32, one division"""
    x = np.asarray(frames)
    if x.ndim == 1:
        x = x[:, None]
    x = x.astype(np.float32) * np.float32(1.0 / 32768.0) if x.dtype == np.int16 else x.astype(np.float32)
    s = x[:, 0].copy()
    if x.shape[1] > 1:
        for c in range(1, x.shape[1]):
            s = s + x[:, c]
        s = s / np.float32(x.shape[1])
    return s.astype(np.float32)


def resample_ref(mono: np.ndarray, up: int, down: int) -> np.ndarray:
    """the kernel's arithmetic on float32 mono samples -> float32 [ceil(n up / down)]"""
    x = np.asarray(mono, dtype=np.float32)
    n = x.shape[0]
    hl, h64 = design(up, down)
    h = h64.astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    m = np.arange(out_len(n, up, down), dtype=np.int64)
    t = hl + m * down
    jh = t // up
    ph = t - jh * up
    acc = np.zeros(m.shape[0], np.float32)
    if m.shape[0] == 0:
        return acc
    for k in range(int(((2 * hl - ph) // up).max()) + 1):
        j, idx = jh - k, ph + k * up
        ok = (j >= 0) & (j < n) & (idx <= 2 * hl)
        xv = np.where(ok, x64[np.clip(j, 0, n - 1)], 0.0)
        hv = np.where(ok, h[np.clip(idx, 0, 2 * hl)], 0.0)
        acc = (xv * hv + acc.astype(np.float64)).astype(np.float32)
    return acc


def scipy_ref(mono: np.ndarray, up: int, down: int) -> np.ndarray:
    """what audio_io.load_audio computes today: resample_poly on the float64 copy of the float32 mono samples"""
    from scipy.signal import resample_poly
    x = np.asarray(mono, dtype=np.float32).astype(np.float64)
    return x.copy() if up == down else resample_poly(x, up, down)


def speech_like(n: int, rate: int, seed: int = 1234, peak: float = 1.0) -> np.ndarray:
    """whisperlive_amd.synthetic.speech_like_pcm's recipe at `rate` Hz and `n` samples, scaled to `peak` (float64)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    sig = np.sin(2 * np.pi * 120 * t)
    for f, a in ((700, 0.6), (1200, 0.4), (2600, 0.25)):
        sig = sig + a * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    sig = sig * (0.5 * (1 + np.sin(2 * np.pi * 4 * t))) + rng.normal(0, 0.01, n)
    return peak * sig / max(np.max(np.abs(sig)), 1e-30)


def grid_lengths(rate: int, seconds: int = 3):
    """1, 2, down - 1, down, down + 1, one shorter than the filter's reach, 3 s + 1 frame (those that are >= 1, once each)"""
    up, down = ratio(rate)
    out = []
    for n in (1, 2, down - 1, down, down + 1, reach(up, down) - 1, seconds * rate + 1):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def grid_signals(n: int, rate: int, seed: int = 0):
    """name -> float32 mono input of n frames: speech-like of peak 1, a unit impulse at the first frame and at the last"""
    first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
    first[0], last[-1] = 1.0, 1.0
    return {"speech": speech_like(n, rate, seed=1234 + seed).astype(np.float32), "impulse_first": first, "impulse_last": last}


def multichannel(n: int, rate: int, channels: int, fmt: int) -> np.ndarray:
    """[n, channels] frames whose channels carry DIFFERENT signals (another seed and gain each), float32 or int16"""
    cols = [speech_like(n, rate, seed=77 + 13 * c, peak=1.0 / (1 + 0.5 * c)) for c in range(channels)]
    x = np.stack(cols, axis=1)
    if fmt == S16:
        return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the hook
def run_hook(frames: np.ndarray, rate: int, block_frames: int = 0, fill: float = -7.25, extra: int = 5, device: int = 0,
             channels=None, n_frames=None, fmt=None):
    """wlx_debug_resample on [n, ch] frames -> (rc, out buffer of n_out + extra floats pre-filled with `fill`, n_out).
    channels / n_frames / fmt override what the array says (for the refused shapes)."""
    from whisperlive_amd import _lib
    lib = _lib.load()
    x = np.asarray(frames)
    if x.ndim == 1:
        x = x[:, None]
    f = (S16 if x.dtype == np.int16 else F32) if fmt is None else fmt
    x = np.ascontiguousarray(x, dtype=np.int16 if x.dtype == np.int16 else np.float32)
    n = x.shape[0] if n_frames is None else n_frames
    ch = x.shape[1] if channels is None else channels
    cap = (out_len(min(max(n, 0), x.shape[0]), *ratio(rate)) if rate > 0 and max(ratio(rate)) <= 640 else 0) + extra
    out = np.full(cap, fill, np.float32)
    n_out = C.c_int64(-1)
    rc = lib.wlx_debug_resample(device, x.ctypes.data_as(C.c_void_p), n, ch, f, rate, block_frames,
                                out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n_out))
    return rc, out, n_out.value
