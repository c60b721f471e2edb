"""CPU: wlx_flac_probe (host only) — what the frame index of csrc/flac.hip accepts, refuses (WLX_ERR_ARG: a shape the device route does
not take) and finds damaged (WLX_ERR_DATA), before anything would be launched."""
import numpy as np
import pytest

from whisperlive_amd import _lib, audio_io

from . import flac_writer as W


def _stream(n=600, ch=2, bps=16, rate=16000, bs=200, seed=3, **kw):
    rng = np.random.RandomState(seed)
    pcm = rng.randint(-(1 << (bps - 1)), 1 << (bps - 1), size=(n, ch)).astype(np.int64)
    return W.encode_stream(pcm, rate, bps, W.split_blocks(n, bs), **kw), pcm


def _code(data):
    try:
        return 0, audio_io.flac_probe(bytes(data))
    except _lib.WlxError as e:
        return e.code, None


def test_intact_stream_is_ok():
    data, pcm = _stream(padding=40)
    rc, info = _code(data)
    assert rc == 0 and (info.n_frames, info.total_samples, info.served) == (3, 600, 1)


def test_no_magic_is_damage():
    data, _ = _stream()
    assert _code(b"fLaX" + data[4:])[0] == _lib.ERR_DATA
    assert _code(b"")[0] == _lib.ERR_DATA


def test_truncated_in_the_metadata_is_damage():
    data, _ = _stream()
    assert _code(data[:20])[0] == _lib.ERR_DATA
    assert _code(data[:4])[0] == _lib.ERR_DATA


def test_truncated_in_the_last_frame_is_damage():
    data, _ = _stream()
    for cut in (1, 2, 3, 50):
        assert _code(data[:-cut])[0] == _lib.ERR_DATA, cut


def _frame_starts(data, pcm, bs=200):
    frames = W.encode_frames(pcm, 16000, 16, W.split_blocks(pcm.shape[0], bs))
    first = len(data) - sum(len(f) for f in frames)
    return [first + sum(len(f) for f in frames[:i]) for i in range(len(frames))], frames


def test_a_flipped_byte_in_a_frame_body_is_damage():
    data, pcm = _stream()
    starts, frames = _frame_starts(data, pcm)
    for f in range(3):
        b = bytearray(data)
        b[starts[f] + len(frames[f]) // 2] ^= 0x10
        assert _code(b)[0] == _lib.ERR_DATA, f


def test_a_flipped_byte_in_a_frame_header_is_damage():
    data, pcm = _stream()
    starts, _ = _frame_starts(data, pcm)
    for f in range(3):
        for off in (2, 3, 4):                       # block size / rate codes, channel / width codes, the frame number
            b = bytearray(data)
            b[starts[f] + off] ^= 0x10
            assert _code(b)[0] == _lib.ERR_DATA, (f, off)


def test_a_false_sync_inside_a_frame_is_not_a_frame():
    """an 8-bit VERBATIM subframe whose samples spell, at a byte-aligned position, a complete frame header with a correct CRC-8 and the
    expected next frame number: only the CRC-16 in front of it tells it from a frame start"""
    rate, bps, n = 16000, 8, 64
    fake = W.frame_header(n, rate, 1, bps, 1, False, W.INDEPENDENT)         # frame number 1: what follows frame 0
    rng = np.random.RandomState(5)
    pcm = rng.randint(-100, 100, size=(2 * n, 1)).astype(np.int64)
    at = 20                                                                  # header (6 bytes) + subframe header (1): samples are byte-aligned
    pcm[at:at + len(fake), 0] = np.frombuffer(fake, np.int8)
    data = W.encode_stream(pcm, rate, bps, [n, n])
    assert data.count(fake) == 2                                             # the false one inside frame 0, the true one of frame 1
    rc, info = _code(data)
    assert rc == 0 and info.n_frames == 2 and info.total_samples == 2 * n
    one = W.metadata(W.streaminfo(pcm[:n], rate, bps, n, n)) + W.encode_frames(pcm[:n], rate, bps, [n])[0]
    rc, info = _code(one)                                                    # the frame alone: ONE frame, not two
    assert rc == 0 and info.n_frames == 1 and info.total_samples == n
    x, _ = audio_io.read_flac(data)
    assert np.array_equal(np.round(x * 128).astype(np.int64), pcm)


def test_a_32_bit_stream_is_indexed_and_not_served():
    rng = np.random.RandomState(1)
    pcm = rng.randint(-(1 << 31), 1 << 31, size=(300, 2)).astype(np.int64)
    rc, info = _code(W.encode_stream(pcm, 16000, 32, [200, 100]))
    assert rc == 0 and info.served == 0 and (info.bits_per_sample, info.n_frames, info.total_samples) == (32, 2, 300)


def test_an_unserved_rate_is_indexed_and_not_served():
    data, _ = _stream(rate=44101)
    rc, info = _code(data)
    assert rc == 0 and info.served == 0 and info.sample_rate == 44101 and info.n_frames == 3


def test_a_changed_channel_count_in_frame_2_is_refused():
    data, pcm = _stream()
    frames = W.encode_frames(pcm, 16000, 16, [200, 200, 200])
    mono = W.encode_frame(pcm[200:400, :1], 16000, 16, 1)
    bad = data[:len(data) - sum(len(f) for f in frames)] + frames[0] + mono + frames[2]
    assert _code(bad)[0] == _lib.ERR_ARG


@pytest.mark.parametrize("head", [b"OggS", b"ID3\x04"])
def test_other_containers_are_refused_not_damaged(head):
    data, _ = _stream()
    assert _code(head + data)[0] == _lib.ERR_ARG
