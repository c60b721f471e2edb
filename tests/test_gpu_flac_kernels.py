"""GPU: the FLAC frame decoder and finish kernel (csrc/flac.hip, csrc/flac_core.h) through wlx_debug_flac_decode — the integers the device
decodes equal the MD5-pinned Python decoder's, exactly, over the matrix of tests/flac_cases.py (block sizes with 8- and 16-bit size
codes and short last frames, 8 / 12 / 16 / 24 bits, 1 / 2 / 3 / 8 channels, every subframe type, LPC orders x precision x shift, both
Rice methods, partition orders 0 / largest / empty first partition, k = 0 and 14, escape partitions, wasted bits, the four channel
assignments, the 25-bit side channel, variable block size with 36-bit sample numbers, 65 and 130 frames) and a real encoder's file."""
import ctypes as C
import os

import numpy as np
import pytest

from . import flac_cases as FC

pytestmark = pytest.mark.gpu

JFK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_head.flac")
CASES = FC.cases()


def _decode(data: bytes, cap: int):
    from whisperlive_amd import _lib
    lib = _lib.load()
    out = np.full(cap + 8, -123456789, np.int32)
    n, ch = C.c_int64(0), C.c_int32(0)
    _lib.check(lib.wlx_debug_flac_decode(0, data, len(data), out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n), C.byref(ch)))
    assert (out[n.value * ch.value:] == -123456789).all()                 # nothing written past the stream's samples
    return out[:n.value * ch.value].reshape(n.value, ch.value).astype(np.int64)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_decode_equals_the_python_decoder(gpu, case):
    from whisperlive_amd import audio_io
    x, _ = audio_io.read_flac(case["data"], verify_md5=True)
    want = np.round(x.astype(np.float64) * (1 << (case["bps"] - 1))).astype(np.int64)
    assert np.array_equal(want, case["pcm"])
    got = _decode(case["data"], want.size)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_device_decode_of_a_real_encoders_file(gpu):
    from whisperlive_amd import audio_io
    with open(JFK, "rb") as f:
        data = f.read()
    x, _ = audio_io.read_flac(data, verify_md5=True)
    want = np.round(x.astype(np.float64) * (1 << 23)).astype(np.int64)
    got = _decode(data, want.size)
    assert got.shape == (147456, 2) and np.array_equal(got, want)


def test_a_buffer_too_small_is_refused_before_any_launch(gpu):
    from whisperlive_amd import _lib
    case = CASES[0]
    out = np.zeros(4, np.int32)
    n, ch = C.c_int64(0), C.c_int32(0)
    rc = _lib.load().wlx_debug_flac_decode(0, case["data"], len(case["data"]), out.ctypes.data_as(C.POINTER(C.c_int32)), 4, C.byref(n), C.byref(ch))
    assert rc == _lib.ERR_ARG and not out.any()
