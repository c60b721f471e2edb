"""CPU tests of the live path's stream resampler: the host-only planner wlx_resample_stream_count against the Python formula, the
host restatement whisperlive_amd/stream_resample.py StreamResampler against scipy.signal.resample_poly of the WHOLE stream under any
cutting into packets, and the G.711 / uint8 decode of all 256 codes."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd import stream_resample as SR

RATES = [8000, 11025, 44100, 48000]


def lib_count(rate, J, flush):
    n = C.c_int64(-1)
    rc = _lib.load().wlx_resample_stream_count(rate, J, 1 if flush else 0, C.byref(n))
    return rc, n.value


def py_count(rate, J, flush):
    """the issue's rule, searched for rather than solved: the outputs whose newest input exists"""
    up, down = R.ratio(rate)
    hl = 0 if up == down else 10 * max(up, down)
    if flush:
        return R.out_len(J, up, down)
    m = 0
    while (hl + m * down) // up <= J - 1:
        m += 1
    return m


def test_planner_equals_the_formula_is_monotone_and_sums_over_cuttings():
    rng = np.random.default_rng(5)
    for rate in RATES + [16000, 12000, 96000]:
        up, down = R.ratio(rate)
        prev = 0
        for J in sorted(set([0, 1, 2, 3, R.reach(up, down) - 1, R.reach(up, down), 4000] + rng.integers(0, 700, 12).tolist())):
            rc, got = lib_count(rate, J, False)
            assert rc == 0 and got == py_count(rate, J, False) == SR.stream_count(rate, J, False), (rate, J)
            assert got >= prev, (rate, J)
            prev = got
            rc, fl = lib_count(rate, J, True)
            assert rc == 0 and fl == R.out_len(J, up, down) == SR.stream_count(rate, J, True) and fl >= got, (rate, J)
        # per-call counts of a cutting sum to the planner's total
        n = int(rng.integers(3000, 6000))
        cuts = np.sort(rng.integers(0, n + 1, 40))
        sr = SR.StreamResampler("int16", 1, rate)
        counts = [sr.advance(np.zeros(b - a, np.int16)) for a, b in zip([0] + cuts.tolist(), cuts.tolist() + [n])]
        assert sum(counts) == lib_count(rate, n, False)[1] == sr.M
        counts.append(sr.advance(np.zeros(0, np.int16), flush=True))
        assert sum(counts) == lib_count(rate, n, True)[1] == R.out_len(n, up, down)
    assert lib_count(16000, 777, False) == (0, 777)                         # the copy path has no latency
    assert lib_count(44101, 10, False)[0] == _lib.ERR_ARG and lib_count(8000, -1, False)[0] == _lib.ERR_ARG


def cuttings(n, seed):
    rng = np.random.default_rng(seed)
    rand = np.sort(rng.integers(0, n + 1, 60)).tolist()
    return {
        "random": rand,
        "one_frame": list(range(1, 65)) + rand,                              # 1-frame packets, then random ones
        "with_empty": sorted(rand + rand[::3] + [0, 0, n, n]),               # repeated cut values: empty packets
    }


def feed_all(sr, frames, cuts):
    edges = [0] + sorted(cuts) + [frames.shape[0]]
    parts = [sr.feed(frames[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    parts.append(sr.flush())
    return np.concatenate(parts), [p.shape[0] for p in parts]


@pytest.mark.parametrize("rate", RATES)
def test_stream_resampler_equals_scipy_of_the_whole_stream_under_any_cutting(rate):
    up, down = R.ratio(rate)
    n = 3000 + (rate * 7) % 3000
    x = R.speech_like(n, rate, seed=rate).astype(np.float32)
    want = R.scipy_ref(x, up, down)
    outs = {}
    for name, cuts in cuttings(n, rate).items():
        sr = SR.StreamResampler("float32", 1, rate)
        got, counts = feed_all(sr, x[:, None], cuts)
        assert got.dtype == np.float32 and got.shape == want.shape == (SR.stream_count(rate, n, True),), (name, got.shape)
        err = float(np.abs(got - want).max())
        print(f"{rate} Hz, {name}: max abs error against scipy {err:.3e}")
        assert err <= R.RESAMPLE_ATOL / 4, (name, err)       # the bound tests/test_resample_ref.py holds a host restatement to
        assert sr.J == n and sr.M == want.shape[0] and sr.closed
        outs[name] = got
    assert np.array_equal(outs["random"], outs["one_frame"]) and np.array_equal(outs["random"], outs["with_empty"])
    with pytest.raises(RuntimeError):
        sr.feed(x[:1, None])


def test_stream_resampler_stereo_int16_and_copy_path():
    frames = R.multichannel(3500, 48000, 2, R.S16)
    up, down = R.ratio(48000)
    got, _ = feed_all(SR.StreamResampler("int16", 2, 48000), frames, cuttings(3500, 1)["with_empty"])
    want = R.scipy_ref(R.mono_f32(frames), up, down)
    assert np.abs(got - want).max() <= R.RESAMPLE_ATOL / 4
    # 16 kHz: conversion and down-mix only, bit for bit, no latency
    sr = SR.StreamResampler("int16", 2, 16000)
    a, b = sr.feed(frames[:1000].tobytes()), sr.feed(frames[1000:])
    assert a.shape[0] == 1000 and np.array_equal(np.concatenate((a, b, sr.flush())), R.mono_f32(frames))
    # advance() (the device computed the samples) leaves the same state as feed(): the fallback continues without a gap
    s1, s2 = SR.StreamResampler("int16", 2, 48000), SR.StreamResampler("int16", 2, 48000)
    s1.feed(frames[:1234]); assert s2.advance(frames[:1234]) == s1.M
    assert (s1.J, s1.M) == (s2.J, s2.M) and np.array_equal(s1.tail, s2.tail)
    assert np.array_equal(s1.feed(frames[1234:], flush=True), s2.feed(frames[1234:], flush=True))


def test_refusals_of_the_host_side():
    for bad in (("mp3", 1, 8000), ("mulaw", 0, 8000), ("mulaw", 9, 8000), ("int16", 1, 44101), ("int16", 1, 0), (2, 1, 8000)):
        with pytest.raises(ValueError):
            SR.StreamResampler(*bad)
    sr = SR.StreamResampler("int16", 2, 8000)
    with pytest.raises(ValueError):
        sr.feed(b"\x00" * 6)                                  # one and a half frames
    assert (sr.J, sr.M) == (0, 0)


def test_g711_and_u8_decode_all_256_codes():
    codes = np.arange(256, dtype=np.uint8)
    mu, al = SR.decode_mulaw(codes), SR.decode_alaw(codes)
    assert (mu[0xFF], mu[0x7F], mu[0x00], mu[0x80]) == (0, 0, -32124, 32124)
    assert (al[0xD5], al[0x55], al[0xAA], al[0x2A]) == (8, -8, 32256, -32256)
    # odd symmetry: the sign bit flips the value
    assert np.array_equal(mu[:128], -mu[128:]) and np.array_equal(al[:128], -al[128:])
    # monotone per sign: mu-law codes are stored complemented (0x80 the largest, 0xFF zero); A-law with its even bits inverted
    assert np.all(np.diff(mu[128:]) < 0) and np.all(np.diff(mu[:128]) > 0)
    pos = al[(np.arange(128) | 0x80) ^ 0x55]                  # positive A-law values in the order of their magnitude field
    assert np.all(np.diff(pos) > 0) and np.array_equal(al[np.arange(128) ^ 0x55], -pos)
    assert np.abs(mu).max() == 32124 and np.abs(al).max() == 32256
    for fmt, lin, scale in (("mulaw", mu, 32768), ("alaw", al, 32768), ("uint8", codes.astype(np.int32) - 128, 128)):
        f = SR.decode_samples(codes, SR.WIRE_FORMATS[fmt][0])
        assert f.dtype == np.float32
        k = f.astype(np.float64) * 32768
        assert np.array_equal(k, np.round(k)) and np.array_equal(f.astype(np.float64), lin / scale)   # exactly k / 32768
    assert np.array_equal(SR.decode_samples(codes, _lib.PCM_U8), (codes.astype(np.float32) - 128.0) / 128.0)   # the server's uint8 rule
