"""GPU: the channel-split front end and the multi-source chunk gather through the C ABI on a tiny engine (max_batch 4):
wlx_pcm_put_frames_split, wlx_pcm_put_flac_split, wlx_logmel_chunks_multi. Everything is held bit for bit to the one-channel entry
points that exist already."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R

from . import flac_writer as W

pytestmark = pytest.mark.gpu

B = 4


@pytest.fixture(scope="module")
def engine(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7), device=0)
    yield eng
    eng.close()


@pytest.fixture()
def slots(engine):
    s, ref = engine.create_slot(B, 5), engine.create_slot(1, 5)
    yield s, ref
    s.close()
    ref.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _mono(ref, frames, rate):
    ref.put_frames(np.ascontiguousarray(frames), rate)
    return ref.pcm()


# ------------------------------------------------------------------------------------------------ put_frames_split
@pytest.mark.parametrize("rate,fmt,ch,first", [(44100, R.F32, 2, 2), (48000, R.S16, 3, 1), (16000, R.F32, 2, 0)],
                         ids=["44k_f32_stereo", "48k_s16_3ch", "16k_copy"])
def test_put_frames_split_equals_put_frames_of_each_channel(slots, rate, fmt, ch, first):
    s, ref = slots
    frames = R.multichannel(rate // 4 + 7, rate, ch, fmt)
    if rate == 16000:
        frames[::3, 1] = np.float32(-0.0)
    keep = np.linspace(-1, 1, 777, dtype=np.float32)
    others = [i for i in range(B) if not first <= i < first + ch]
    for i in others:
        s.pcm_put(keep, item=i)
    n = s.put_frames_split(frames, rate, first)
    assert n == R.out_len(frames.shape[0], *R.ratio(rate))
    for c in range(ch):
        got = s.pcm(first + c)
        assert got.shape[0] == n and np.array_equal(_bits(got), _bits(_mono(ref, frames[:, c:c + 1], rate))), ("channel", c)
    for i in others:                                                   # the items outside the C named ones keep what they held
        assert s.pcm_count(i) == 777 and np.array_equal(_bits(s.pcm(i)), _bits(keep))


def _split_rc(engine, s, frames, rate, first, channels=None, fmt=None):
    from whisperlive_amd import _lib
    x = np.ascontiguousarray(frames, np.float32)
    n = C.c_int64(-1)
    rc = engine.lib.wlx_pcm_put_frames_split(engine._h, s.sid, first, x.ctypes.data_as(C.c_void_p), x.shape[0],
                                             x.shape[1] if channels is None else channels, _lib.PCM_F32 if fmt is None else fmt, rate,
                                             C.byref(n))
    return rc, n.value


def test_put_frames_split_refusals_leave_every_item_as_it_was(engine, slots):
    from whisperlive_amd import _lib
    s, _ = slots
    before = [np.full(100 + i, 0.25 * (i + 1), np.float32) for i in range(B)]
    for i in range(B):
        s.pcm_put(before[i], item=i)
    x = R.multichannel(3000, 44100, 3, R.F32)
    for kw in (dict(rate=44100, first=2), dict(rate=44100, first=-1), dict(rate=44100, first=B), dict(rate=44101, first=0),
               dict(rate=44100, first=0, fmt=2), dict(rate=44100, first=0, channels=0), dict(rate=44100, first=0, channels=9)):
        rc, n = _split_rc(engine, s, x, **kw)                         # first + 3 > max_batch, first outside, unserved rate, bad format ...
        assert rc == _lib.ERR_ARG and n == -1, kw
        for i in range(B):
            assert np.array_equal(_bits(s.pcm(i)), _bits(before[i])), (kw, i)


# ------------------------------------------------------------------------------------------------ put_flac_split
def _flac(rate, ch, n, blocksize, assignment, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    x = np.sin(6.2831853 * t * rng.uniform(200, 900, size=(1, ch)) / rate) * 9000 + rng.randint(-300, 300, size=(n, ch))
    pcm = np.round(x).astype(np.int64)
    return W.encode_stream(pcm, rate, 16, W.split_blocks(n, blocksize), subframe={"type": "fixed", "order": 2, "k": 9}, assignment=assignment)


FLACS = {
    # stereo: left/side, side/right and mid/side frames in turn; 1152-sample blocks with a short last one
    "stereo_mixed_44k": lambda: _flac(44100, 2, 5 * 1152 + 301, 1152, lambda f: (W.LEFT_SIDE, W.SIDE_RIGHT, W.MID_SIDE)[f % 3], 1),
    # ... and 576-sample blocks that divide the stream, at a rate that up-samples
    "stereo_mixed_8k": lambda: _flac(8000, 2, 6 * 576, 576, lambda f: (W.MID_SIDE, W.LEFT_SIDE, W.SIDE_RIGHT)[f % 3], 2),
    "three_channels_16k": lambda: _flac(16000, 3, 4 * 1152 + 77, 1152, W.INDEPENDENT, 3),
}


@pytest.mark.parametrize("name", sorted(FLACS))
def test_put_flac_split_equals_put_frames_of_each_decoded_channel(slots, name):
    from whisperlive_amd import audio_io
    s, ref = slots
    data = FLACS[name]()
    frames, rate = audio_io.read_flac(data)
    ch = frames.shape[1]
    first = B - ch
    s.pcm_put(np.ones(55, np.float32), item=0)
    n, info = s.put_flac_split(data, first)
    assert (info.sample_rate, info.channels, info.total_samples, info.served) == (rate, ch, frames.shape[0], 1)
    assert n == R.out_len(frames.shape[0], *R.ratio(rate))
    for c in range(ch):
        got = s.pcm(first + c)
        assert got.shape[0] == n and np.array_equal(_bits(got), _bits(_mono(ref, frames[:, c:c + 1], rate))), ("channel", c)
    assert s.pcm_count(0) == 55


def test_put_flac_split_damaged_and_refused_streams(engine, slots):
    from whisperlive_amd import _lib
    s, _ = slots
    good = FLACS["stereo_mixed_8k"]()
    for i in range(B):
        s.pcm_put(np.full(64, 0.5, np.float32), item=i)

    def rc_of(data, first):
        n, info = C.c_int64(-1), _lib.wlx_flac_info()
        return engine.lib.wlx_pcm_put_flac_split(engine._h, s.sid, first, data, len(data), C.byref(info), C.byref(n)), n.value

    assert rc_of(good, B - 1) == (_lib.ERR_ARG, -1)                    # first_item + channels > max_batch
    assert rc_of(good, -1) == (_lib.ERR_ARG, -1)
    rng = np.random.RandomState(2)
    wide = W.encode_stream(rng.randint(-(1 << 31), 1 << 31, size=(300, 2)).astype(np.int64), 16000, 32, [200, 100])
    assert rc_of(wide, 0) == (_lib.ERR_ARG, -1)                        # a 32-bit stream: the shape wlx_pcm_put_flac refuses
    assert [s.pcm_count(i) for i in range(B)] == [64] * B             # refusals: every item as it was
    # a flipped body byte: the HOST index finds the CRC-16 wrong, before any launch (the device-side failure is the next test)
    bad = bytearray(good)
    bad[len(bad) // 2] ^= 0x20
    assert rc_of(bytes(bad), 1) == (_lib.ERR_DATA, -1)
    with pytest.raises(_lib.WlxError) as ei:
        s.put_flac_split(bytes(bad), 1)
    assert ei.value.code == _lib.ERR_DATA


def test_a_frame_that_fails_on_the_device_leaves_none_of_the_items_resident(engine, slots):
    """the frame's CRC-8 / CRC-16 are recomputed after the damage, so the host index accepts the stream and the DEVICE decoder meets
    the bad frame: its residual is a run of zero bits, a unary count that does not end inside the frame"""
    from whisperlive_amd import _lib
    s, _ = slots
    rng = np.random.RandomState(5)
    pcm = rng.randint(-2000, 2000, size=(2 * 576, 2)).astype(np.int64)
    frames = W.encode_frames(pcm, 16000, 16, [576, 576], subframe={"type": "fixed", "order": 1, "k": 11})
    f1 = bytearray(frames[1])
    body = bytearray(f1[:-2])
    for k in range(8, len(body) - 1):                                   # well inside the residual: the decoder desynchronises
        body[k] = 0x00                                                  # (a run of zero bits is a unary count that never ends in the frame)
    f1 = bytes(body) + W.crc16(bytes(body)).to_bytes(2, "big")
    info = W.streaminfo(pcm, 16000, 16, 576, 576)
    data = W.metadata(info) + frames[0] + f1
    for i in range(B):
        s.pcm_put(np.full(64, 0.5, np.float32), item=i)
    n, fi = C.c_int64(-1), _lib.wlx_flac_info()
    rc = engine.lib.wlx_pcm_put_flac_split(engine._h, s.sid, 1, data, len(data), C.byref(fi), C.byref(n))
    assert rc == _lib.ERR_DATA and n.value == -1
    assert [s.pcm_count(i) for i in range(B)] == [64, 0, 0, 64]        # the two named items hold nothing, the others what they held


# ------------------------------------------------------------------------------------------------ wlx_logmel_chunks_multi
@pytest.fixture()
def two_sources(slots):
    """items 2 and 3 of the slot hold two different channels of different use: 40000 samples each"""
    s, ref = slots
    x = R.multichannel(40000, 16000, 2, R.F32) * np.float32(0.5)
    assert s.put_frames_split(x, 16000, 2) == 40000
    return s, ref, x


CHUNKS = [[(100, 16100)], [(0, 3000), (3000, 9000), (12345, 20001), (30000, 40000)], [(20000, 39999)]]
SOURCES = [3, 2, 3]


def test_chunks_multi_is_bit_identical_to_logmel_of_each_chunks_own_channel(two_sources):
    s, ref, x = two_sources
    frames = s.logmel_chunks(CHUNKS, src_item=SOURCES, first_item=0)
    for c, (rg, src) in enumerate(zip(CHUNKS, SOURCES)):
        cat = np.concatenate([x[a:b, src - 2] for a, b in rg])
        assert frames[c] == ref.logmel(cat) == (cat.shape[0] + 160) // 160
        assert np.array_equal(_bits(s.features(c)), _bits(ref.features())), ("chunk", c)
    # the sources are still resident and unchanged, destinations that are no source hold no PCM
    assert [s.pcm_count(i) for i in range(B)] == [0, 0, 40000, 40000]
    assert np.array_equal(_bits(s.pcm(2)), _bits(x[:, 0])) and np.array_equal(_bits(s.pcm(3)), _bits(x[:, 1]))


def test_single_source_multi_call_equals_logmel_chunks(two_sources):
    s, _ref, _x = two_sources
    a = s.logmel_chunks(CHUNKS[:2], src_item=3, first_item=0)
    want = [s.features(i).copy() for i in range(2)]
    b = s.logmel_chunks(CHUNKS[:2], src_item=[3, 3], first_item=0)
    assert a == b
    for i in range(2):
        assert np.array_equal(_bits(s.features(i)), _bits(want[i]))


def _multi_rc(engine, s, chunks, sources, first=0, null_src=False, null_ranges=False):
    off = np.zeros(len(chunks) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in chunks])
    rg = np.ascontiguousarray(np.asarray([r for c in chunks for r in c], np.int64).reshape(-1, 2))
    src = np.ascontiguousarray(sources, np.int32)
    nf = np.full(len(chunks), -1, np.int32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    rc = engine.lib.wlx_logmel_chunks_multi(engine._h, s.sid, None if null_src else src.ctypes.data_as(i32p),
                                            None if null_ranges else rg.ctypes.data_as(i64p), off.ctypes.data_as(i32p), len(chunks), first,
                                            nf.ctypes.data_as(i32p))
    return rc, nf


def test_chunks_multi_refusals_leave_the_features_unchanged(engine, two_sources):
    from whisperlive_amd import _lib
    s, _ref, _x = two_sources
    s.logmel_chunks(CHUNKS[:2], src_item=[2, 3], first_item=0)
    before = [s.features(i).copy() for i in range(2)]
    s.pcm_put(np.ones(500, np.float32), item=1)                          # item 1: 500 samples resident; item 0: none
    one = [[(0, 400)]]
    cases = [
        (dict(chunks=one, sources=[2], null_src=True), _lib.ERR_ARG),
        (dict(chunks=one, sources=[2], null_ranges=True), _lib.ERR_ARG),
        (dict(chunks=one, sources=[B]), _lib.ERR_ARG), (dict(chunks=one, sources=[-1]), _lib.ERR_ARG),          # a source outside the slot
        (dict(chunks=one, sources=[0]), _lib.ERR_STATE),                                                           # ... with no PCM resident
        (dict(chunks=[[(0, 400)], [(0, 501)]], sources=[2, 1]), _lib.ERR_STATE),       # past the resident count of THAT chunk's source
        (dict(chunks=[[(0, 400)], [(100, 100)]], sources=[2, 3]), _lib.ERR_ARG),       # an empty range
        (dict(chunks=[[(0, 400), (300, 500)]], sources=[2]), _lib.ERR_ARG),            # overlapping
        (dict(chunks=[[(i, i + 1) for i in range(0, 2 * 257, 2)]], sources=[2]), _lib.ERR_ARG),                  # more than WLX_LM_MAXRANGES
        (dict(chunks=one * 2, sources=[2, 3], first=B - 1), _lib.ERR_ARG),             # destination items out of range
    ]
    for kw, want in cases:
        rc, nf = _multi_rc(engine, s, **kw)
        assert rc == want and np.all(nf == -1), kw
    assert s.logmel_chunks([[(0, 400)], [(0, 500)]], src_item=[2, 1], first_item=0) == [3, 4]      # (the neighbours of the refused cases are served)
    s.logmel_chunks(CHUNKS[:2], src_item=[2, 3], first_item=0)
    for i in range(2):
        assert np.array_equal(_bits(s.features(i)), _bits(before[i]))
    rc, _ = _multi_rc(engine, s, one, [0])
    assert rc == _lib.ERR_STATE
    for i in range(2):                                                   # a refusal writes nothing: the features of the last good call stand
        assert np.array_equal(_bits(s.features(i)), _bits(before[i]))
