"""CPU: the telephony WAVE formats on the host — audio_io.read_wav for G.711 mu-law / A-law (tags 7 / 6), IMA ADPCM (0x11) and MS ADPCM
(0x02), and the host-only probe wlx_wav_probe.

The IMA nibble arithmetic and the G.711 tables are pinned by tests/golden/adpcm_golden.npz, recorded from Python's audioop
(tests/golden/make_adpcm_golden.py); nothing here imports audioop.

MS ADPCM has no library to record from; it is pinned by a known-answer block worked out by hand from the format's rules
(predicted = (sample1 * c1 + sample2 * c2) >> 8; new = clamp16(predicted + signed nibble * delta); delta = max(16, (ADAPT[nibble] *
delta) >> 8); ADAPT = 230 230 230 230 307 409 512 614 768 614 512 409 307 230 230 230):

  mono, block_align 10, predictor index 1 = (512, -256), delta 16, sample1 100, sample2 50, nibble bytes 0x3F 0x80 0x71
  -> samples per block (10 - 7) * 2 + 2 = 8:  out[0] = sample2 = 50, out[1] = sample1 = 100, then
  nibble 3:  predicted (100 * 512 - 50 * 256) >> 8 = 38400 >> 8 = 150;  150 + 3 * 16 = 198;    delta (230 * 16) >> 8 = 14 -> 16
  nibble F:  (198 * 512 - 100 * 256) >> 8 = 75776 >> 8 = 296;           296 - 1 * 16 = 280;    delta (230 * 16) >> 8 = 14 -> 16
  nibble 8:  (280 * 512 - 198 * 256) >> 8 = 92672 >> 8 = 362;           362 - 8 * 16 = 234;    delta (768 * 16) >> 8 = 48
  nibble 0:  (234 * 512 - 280 * 256) >> 8 = 48128 >> 8 = 188;           188 + 0      = 188;    delta (230 * 48) >> 8 = 43
  nibble 7:  (188 * 512 - 234 * 256) >> 8 = 36352 >> 8 = 142;           142 + 7 * 43 = 443;    delta (614 * 43) >> 8 = 103
  nibble 1:  (443 * 512 - 188 * 256) >> 8 = 178688 >> 8 = 698;          698 + 1 * 103 = 801
  = 50 100 198 280 234 188 443 801

  and the floor of a NEGATIVE prediction (an arithmetic shift, not a division that rounds toward zero), predictor index 3 = (192, 64),
  delta 16, sample1 -3, sample2 -1, block_align 8, nibble byte 0x00:
  nibble 0:  (-3 * 192 - 1 * 64) >> 8 = -640 >> 8 = -3 (-2.5 floored);  out = -1 -3 -3, then
  nibble 0:  (-3 * 192 - 3 * 64) >> 8 = -768 >> 8 = -3;                 out = -1 -3 -3 -3
"""
import os
import struct

import numpy as np
import pytest

from whisperlive_amd import _lib, audio_io

from . import wav_writer as W

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adpcm_golden.npz"))


def _ints(x):
    v = x.astype(np.float64) * 32768.0
    assert np.array_equal(v, np.round(v))               # every value an int16 / 32768, exactly
    return v.astype(np.int64)


def _probe(data):
    info = _lib.wlx_wav_info()
    rc = _lib.load().wlx_wav_probe(bytes(data), len(data), info)
    return rc, info


# ------------------------------------------------------------------------------------------------ decode against the pins
@pytest.mark.parametrize("tag,name", [(W.TAG_MULAW, "mulaw"), (W.TAG_ALAW, "alaw")])
@pytest.mark.parametrize("extensible", [False, True])
def test_g711_every_code_is_the_recorded_linear_value(tag, name, extensible):
    codes = bytes(range(256)) * 2
    x, sr = audio_io.read_wav(W.container(tag, 2, 8000, 8, 2, codes, extensible=extensible))
    assert sr == 8000 and x.dtype == np.float32 and x.shape == (256, 2)
    assert np.array_equal(_ints(x).ravel(), np.tile(GOLD[name].astype(np.int64), 2))


def test_ima_blocks_decode_to_the_audioop_recording():
    blocks = b"".join(W.ima_pack([(int(p), int(i))], [n.tolist()], 1)
                      for p, i, n in zip(GOLD["ima_pred"], GOLD["ima_index"], GOLD["ima_nibbles"]))
    x, sr = audio_io.read_wav(W.container(W.TAG_IMA, 1, 8000, 4, 256, blocks))
    got = _ints(x).reshape(len(GOLD["ima_pred"]), 505)
    assert np.array_equal(got[:, 0], GOLD["ima_pred"]) and np.array_equal(got[:, 1:], GOLD["ima_out"])


def test_ima_stereo_words_are_interleaved_by_channel():
    """two recorded streams as the two channels of ONE stereo block sequence: channel c's words are every second 4-byte word"""
    k = 6
    heads = [(int(GOLD["ima_pred"][k + c]), int(GOLD["ima_index"][k + c])) for c in range(2)]
    nibs = [GOLD["ima_nibbles"][k + c].tolist() for c in range(2)]
    x, _ = audio_io.read_wav(W.container(W.TAG_IMA, 2, 8000, 4, 512, W.ima_pack(heads, nibs, 2)))
    got = _ints(x)
    assert got.shape == (505, 2)
    for c in range(2):
        assert np.array_equal(got[1:, c], GOLD["ima_out"][k + c])


def test_ms_known_answer_blocks():
    blk = W.ms_pack([(1, 16, 100, 50)], [[3, 15, 8, 0, 7, 1]], 1, 10)
    x, _ = audio_io.read_wav(W.container(W.TAG_MS, 1, 8000, 4, 10, blk, fmt_extra=W.ms_fmt_extra(8, W.MS_COEFS)))
    assert _ints(x)[:, 0].tolist() == [50, 100, 198, 280, 234, 188, 443, 801]
    blk = W.ms_pack([(3, 16, -3, -1)], [[0, 0]], 1, 8)
    x, _ = audio_io.read_wav(W.container(W.TAG_MS, 1, 8000, 4, 8, blk, fmt_extra=W.ms_fmt_extra(4, W.MS_COEFS)))
    assert _ints(x)[:, 0].tolist() == [-1, -3, -3, -3]


def test_ms_stereo_header_fields_run_over_the_channels_and_nibbles_alternate():
    """the known-answer stream as the RIGHT channel of a stereo block whose left channel is silence (predictor 2 = (0, 0), nibbles 0)"""
    blk = W.ms_pack([(2, 16, 0, 0), (1, 16, 100, 50)], [[0] * 6, [3, 15, 8, 0, 7, 1]], 2, 20)
    x, _ = audio_io.read_wav(W.container(W.TAG_MS, 2, 8000, 4, 20, blk, fmt_extra=W.ms_fmt_extra(8, W.MS_COEFS)))
    got = _ints(x)
    assert got[:, 0].tolist() == [0] * 8 and got[:, 1].tolist() == [50, 100, 198, 280, 234, 188, 443, 801]


def test_ms_coefficients_come_from_the_fmt_chunk_and_default_to_the_standard_seven():
    custom = [(128, 64), (300, -100)]
    blk = W.ms_pack([(1, 16, 100, 50)], [[0, 0]], 1, 8)
    x, _ = audio_io.read_wav(W.container(W.TAG_MS, 1, 8000, 4, 8, blk, fmt_extra=W.ms_fmt_extra(4, custom)))
    a = (100 * 300 - 50 * 100) >> 8
    assert _ints(x)[:, 0].tolist() == [50, 100, a, (a * 300 - 100 * 100) >> 8]
    x, _ = audio_io.read_wav(W.container(W.TAG_MS, 1, 8000, 4, 8, blk, fmt_extra=W.ms_fmt_extra(4, None)))
    b = (100 * 512 - 50 * 256) >> 8
    assert _ints(x)[:, 0].tolist() == [50, 100, b, (b * 512 - 100 * 256) >> 8]


# ------------------------------------------------------------------------------------------------ frame counts
@pytest.mark.parametrize("ch", [1, 2, 8])
@pytest.mark.parametrize("tag", [W.TAG_IMA, W.TAG_MS])
def test_channels_fact_cut_and_dropped_partial_block(tag, ch):
    ba = 64 * ch
    spb = (W.ima_samples_per_block if tag == W.TAG_IMA else W.ms_samples_per_block)(ba, ch)
    pcm = W.speech_like(2 * spb + 17, ch, seed=ch)
    write = W.write_ima if tag == W.TAG_IMA else W.write_ms
    whole, _ = audio_io.read_wav(write(pcm, 8000, ba))
    assert whole.shape == (3 * spb, ch)                                      # the last block is padded out by the writer
    assert np.abs(_ints(whole)[: len(pcm)] - pcm).mean() < 1500               # (a codec, not a copy: it resembles its input)
    cut, _ = audio_io.read_wav(write(pcm, 8000, ba, fact=True))
    assert cut.shape == (len(pcm), ch) and np.array_equal(cut, whole[: len(pcm)])
    part, _ = audio_io.read_wav(write(pcm, 8000, ba, partial=ba - 1))
    assert np.array_equal(part, whole)
    big, _ = audio_io.read_wav(write(pcm, 8000, ba, fact=10 ** 6))             # a `fact` past the blocks does not invent samples
    assert np.array_equal(big, whole)
    zero, _ = audio_io.read_wav(write(pcm, 8000, ba, fact=0))
    assert np.array_equal(zero, whole)
    rc, info = _probe(write(pcm, 8000, ba, fact=True, partial=5))
    assert rc == 0 and info.served == 1
    assert (info.format_tag, info.channels, info.sample_rate, info.bits_per_sample, info.block_align, info.samples_per_block,
            info.n_frames, info.data_bytes) == (tag, ch, 8000, 4, ba, spb, len(pcm), 3 * ba + 5)


def test_g711_frames_and_probe_fields():
    pcm = W.speech_like(1001, 2, seed=3)
    for tag in (W.TAG_MULAW, W.TAG_ALAW):
        for ext in (False, True):
            data = W.write_g711(pcm, 8000, tag, extensible=ext, junk=True)
            x, sr = audio_io.read_wav(data)
            assert sr == 8000 and x.shape == (1001, 2) and np.abs(_ints(x) - pcm).max() <= 1024
            rc, info = _probe(data)
            assert rc == 0 and info.served == 1 and info.format_tag == tag and info.n_frames == 1001 and info.samples_per_block == 1
            assert data[info.data_offset: info.data_offset + info.data_bytes] == W.g711_encode(pcm, tag).tobytes()
            assert audio_io.wav_served(data) and audio_io.wav_probe(data).n_frames == 1001


# ------------------------------------------------------------------------------------------------ refusals
def test_probe_finds_a_damaged_block_header():
    data = bytearray(W.random_adpcm(W.TAG_IMA, 5, 2, 72, seed=1))
    rc, info = _probe(data)
    assert rc == 0 and info.served == 1
    data[info.data_offset + 3 * 72 + 4 + 2] = 89                                   # block 3, channel 1: step index 89
    rc, _ = _probe(data)
    assert rc == _lib.ERR_DATA and b"step index 89" in _lib.load().wlx_last_error()
    with pytest.raises(ValueError, match="damaged WAV stream"):
        audio_io.read_wav(bytes(data))
    with pytest.raises(ValueError, match="damaged WAV stream"):
        audio_io.wav_served(bytes(data))
    data = bytearray(W.random_adpcm(W.TAG_MS, 5, 2, 64, seed=2, coefs=W.MS_COEFS[:3]))
    rc, info = _probe(data)
    assert rc == 0 and info.served == 1
    data[info.data_offset + 4 * 64 + 1] = 3                                        # block 4, channel 1: predictor index 3 of 3 pairs
    rc, _ = _probe(data)
    assert rc == _lib.ERR_DATA and b"predictor index 3" in _lib.load().wlx_last_error()
    with pytest.raises(ValueError, match="damaged WAV stream"):
        audio_io.read_wav(bytes(data))


def test_probe_refuses_a_file_without_fmt_or_data():
    good = W.random_adpcm(W.TAG_IMA, 2, 1, 36)
    for bad in (b"RIFF\x04\0\0\0WAVE", good.replace(b"fmt ", b"fmt_"), good.replace(b"data", b"dat_"), b"RIFX" + good[4:], good[:11]):
        rc, _ = _probe(bad)
        assert rc == _lib.ERR_DATA


@pytest.mark.parametrize("data", [
    W.random_adpcm(W.TAG_IMA, 3, 1, 38),                # 34 bytes behind the header: not whole 4-byte words
    W.random_adpcm(W.TAG_IMA, 3, 2, 36),                # 28 bytes behind two headers: not whole words of both channels
    W.random_adpcm(W.TAG_MS, 3, 3, 3 * 7 + 5),          # 10 nibbles for 3 channels
    W.container(W.TAG_IMA, 1, 8000, 4, 2, bytes(20)),   # shorter than its header
    W.random_adpcm(W.TAG_IMA, 3, 9, 9 * 8),             # 9 channels
    W.random_adpcm(W.TAG_IMA, 3, 1, 36, rate=44101),    # a rate the resampler does not serve
    W.random_adpcm(W.TAG_IMA, 1, 1, 16384),             # a block past the decoder's LDS
    W.random_adpcm(W.TAG_IMA, 0, 1, 36),                # no whole block
    W.container(W.TAG_MULAW, 1, 8000, 16, 2, bytes(64)),   # G.711 of 16 bits
    W.container(W.TAG_MULAW, 9, 8000, 8, 9, bytes(90)),
    W.container(0x31, 1, 8000, 0, 65, bytes(650)),      # GSM 6.10
], ids=["ima-words", "ima-stereo-words", "ms-nibbles", "ima-short", "nine-channels", "44101", "lds", "empty", "g711-16bit", "g711-nine", "gsm"])
def test_probe_says_unserved(data):
    rc, info = _probe(data)
    assert rc == 0 and info.served == 0
    assert not audio_io.wav_served(data)


def test_a_nine_channel_and_a_44101_hz_file_still_decode_on_the_host():
    for data, shape in ((W.random_adpcm(W.TAG_IMA, 3, 9, 72), (27, 9)), (W.random_adpcm(W.TAG_MS, 3, 1, 36, rate=44101), (180, 1))):
        x, _ = audio_io.read_wav(data)
        assert x.shape == shape
    with pytest.raises(ValueError, match="unsupported ADPCM layout"):
        audio_io.read_wav(W.random_adpcm(W.TAG_IMA, 3, 1, 38))
    with pytest.raises(ValueError, match="unsupported WAVE format tag 49"):
        audio_io.read_wav(W.container(0x31, 1, 8000, 0, 65, bytes(650)))


# ------------------------------------------------------------------------------------------------ tags 1 and 3 are as they were
def _pcm16(x, rate=8000, tag=1, bits=16):
    return W.container(tag, x.shape[1], rate, bits, x.shape[1] * bits // 8, x.tobytes())


def test_pcm_and_float_files_are_read_as_before_and_probe_unserved():
    rng = np.random.RandomState(5)
    s16 = rng.randint(-32768, 32768, size=(333, 2)).astype("<i2")
    x, sr = audio_io.read_wav(_pcm16(s16))
    assert sr == 8000 and np.array_equal(x, s16.astype(np.float32) / 32768.0)
    y, _ = audio_io.read_audio(_pcm16(s16))
    assert y.dtype == np.int16 and np.array_equal(y, s16)
    f32 = rng.randn(100, 1).astype("<f4")
    x, _ = audio_io.read_wav(_pcm16(f32, tag=3, bits=32))
    assert np.array_equal(x, f32)
    for data, n in ((_pcm16(s16), 333), (_pcm16(f32, tag=3, bits=32), 100)):
        rc, info = _probe(data)
        assert rc == 0 and info.served == 0 and info.n_frames == n
        assert not audio_io.wav_served(data)
    assert audio_io._wav_parse(_pcm16(s16))[:4] == (1, 2, 8000, 16)


def test_struct_and_prototypes_match_the_header():
    import ctypes as C
    assert C.sizeof(_lib.wlx_wav_info) == 6 * 4 + 3 * 8 + 8
    lib = _lib.load()
    assert len(lib.wlx_pcm_put_wav.argtypes) == len(lib.wlx_pcm_put_flac.argtypes) == 7
    assert len(lib.wlx_pcm_put_wav_split.argtypes) == 7 and len(lib.wlx_debug_adpcm_decode.argtypes) == 7
    assert struct.calcsize("<6i3qi4x") == C.sizeof(_lib.wlx_wav_info)
