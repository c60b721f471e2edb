"""GPU: the ADPCM block decoder (csrc/adpcm.hip adpcm_decode_kernel, csrc/adpcm_core.h) through wlx_debug_adpcm_decode — the int16 values the
device decodes equal the host oracle's (audio_io.read_wav, pinned by tests/test_wav_telephony_host.py) exactly, at the smallest shapes
that can still go wrong: IMA block_align 36 (the minimum with a whole word per channel: 65 samples mono) and 256, MS 32 and 256 (and 33:
a block that is no whole number of dwords, the kernel's byte-store copy), mono and stereo, custom MS coefficients; 1, 2 and 65 blocks
(more than one wave of lanes, and a workgroup's last partial group of blocks); a `fact` cut inside the last block; 8 channels at
block_align 4096 (the LDS bound: one workgroup holds few blocks). The streams are seeded random nibbles behind valid headers, which
reach every clamp."""
import ctypes as C

import numpy as np
import pytest

from . import wav_writer as W

pytestmark = pytest.mark.gpu

CUSTOM = [(128, 64), (300, -100), (-20, 250)]
CASES = []
for _ch in (1, 2):
    for _nb in (1, 2, 65):
        CASES += [("ima", W.TAG_IMA, _nb, _ch, 36 * _ch, W.MS_COEFS), ("ima", W.TAG_IMA, _nb, _ch, 256, W.MS_COEFS),
                  ("ms", W.TAG_MS, _nb, _ch, 32, W.MS_COEFS), ("ms", W.TAG_MS, _nb, _ch, 256, W.MS_COEFS)]
    CASES += [("ms-custom", W.TAG_MS, 65, _ch, 256, CUSTOM), ("ms-odd", W.TAG_MS, 65, _ch, 32 + _ch, W.MS_COEFS)]
CASES += [("ms-odd-bytes", W.TAG_MS, 67, 1, 35, W.MS_COEFS), ("ima-8ch", W.TAG_IMA, 9, 8, 4096, W.MS_COEFS), ("ms-8ch", W.TAG_MS, 9, 8, 4096, W.MS_COEFS),
          ("ima-300", W.TAG_IMA, 300, 1, 36, W.MS_COEFS)]


def _decode(data: bytes, cap: int):
    from whisperlive_amd import _lib
    lib = _lib.load()
    out = np.full(cap + 8, -12345, np.int16)
    n, ch = C.c_int64(0), C.c_int32(0)
    _lib.check(lib.wlx_debug_adpcm_decode(0, data, len(data), out.ctypes.data_as(C.POINTER(C.c_int16)), cap, C.byref(n), C.byref(ch)))
    assert (out[n.value * ch.value:] == -12345).all()                     # nothing written past the file's samples
    return out[:n.value * ch.value].reshape(n.value, ch.value).astype(np.int64)


def _want(data):
    from whisperlive_amd import audio_io
    x, _ = audio_io.read_wav(data)
    return np.round(x.astype(np.float64) * 32768.0).astype(np.int64)


@pytest.mark.parametrize("name,tag,nb,ch,ba,coefs", CASES, ids=[f"{c[0]}-{c[2]}x{c[3]}ch-{c[4]}" for c in CASES])
def test_device_decode_equals_the_host_decoder(gpu, name, tag, nb, ch, ba, coefs):
    data = W.random_adpcm(tag, nb, ch, ba, rate=12345, seed=nb + ch + ba, coefs=coefs)       # (any rate: the hook does not resample)
    want = _want(data)
    got = _decode(data, want.size)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("tag", [W.TAG_IMA, W.TAG_MS])
def test_a_fact_cut_inside_a_block_and_a_partial_block_behind(gpu, tag):
    data = W.random_adpcm(tag, 70, 2, 72, seed=5, fact=70 * 60 - 100, partial=40)
    want = _want(data)
    assert want.shape[0] == 70 * 60 - 100
    got = _decode(data, want.size)
    assert np.array_equal(got, want)


def test_encoded_audio_and_refusals(gpu):
    from whisperlive_amd import _lib
    pcm = W.speech_like(3000, 2, seed=8)
    for data in (W.write_ima(pcm, 8000, 256, fact=True), W.write_ms(pcm, 8000, 256, fact=True)):
        want = _want(data)
        assert want.shape == (3000, 2) and np.array_equal(_decode(data, want.size), want)
    lib = _lib.load()
    out = np.zeros(16, np.int16)
    n, ch = C.c_int64(0), C.c_int32(0)
    args = (out.ctypes.data_as(C.POINTER(C.c_int16)), 16, C.byref(n), C.byref(ch))
    small = W.random_adpcm(W.TAG_IMA, 2, 1, 36)
    assert lib.wlx_debug_adpcm_decode(0, small, len(small), *args) == _lib.ERR_ARG              # 130 samples into 16
    mulaw = W.write_g711(pcm, 8000, W.TAG_MULAW)
    assert lib.wlx_debug_adpcm_decode(0, mulaw, len(mulaw), *args) == _lib.ERR_ARG              # not an ADPCM tag
    bad = bytearray(small)
    bad[bad.index(b"data") + 8 + 2] = 99
    assert lib.wlx_debug_adpcm_decode(0, bytes(bad), len(bad), *args) == _lib.ERR_DATA
