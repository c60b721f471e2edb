"""GPU: the ragged kernels of wlx_pcm_put_many, one launch each (wlx_debug_resample_many, wlx_debug_flac_decode_many): every entry of a
ragged launch is BIT-IDENTICAL to the single-entry hook run on that entry alone (wlx_debug_resample; wlx_debug_resample_stream without
cuts for the G.711 codes, which the file hook does not take; wlx_debug_flac_decode), and the FLAC integers equal audio_io.read_flac."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import flac_cases as FC
from . import flac_writer as FW
from .put_many_cases import broken_frame_stream, flac_stream as _stream_of

pytestmark = pytest.mark.gpu

F32, S16, MULAW, ALAW = 0, 1, 4, 5
SENTINEL = np.float32(-777.25)


def _lib():
    from whisperlive_amd import _lib as L
    return L, L.load()


def _out_len(n, rate):
    from math import gcd
    g = gcd(16000, rate)
    up, down = 16000 // g, rate // g
    return (n * up + down - 1) // down


def _reach(rate):
    from math import gcd
    g = gcd(16000, rate)
    up, down = 16000 // g, rate // g
    return (2 * 10 * max(up, down) + up - 1) // up + 2


@functools.lru_cache(maxsize=None)
def _frames(n, ch, fmt, seed):
    rng = np.random.RandomState(seed)
    if fmt == F32:
        x = (rng.standard_normal((n, ch)) * 0.3).astype(np.float32)
        x[0, 0] = -0.0                                    # the copy path keeps the sign of a zero
        return x
    if fmt == S16:
        return rng.randint(-32768, 32768, size=(n, ch)).astype(np.int16)
    return rng.randint(0, 256, size=(n, ch)).astype(np.uint8)          # every G.711 code


@functools.lru_cache(maxsize=None)
def _single(n, ch, fmt, rate, seed):
    """the entry alone through the single-entry hook -> float32 bits"""
    L, lib = _lib()
    x = _frames(n, ch, fmt, seed)
    cap = _out_len(n, rate)
    out = np.full(cap + 1, SENTINEL, np.float32)
    got = C.c_int64(-1)
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    if fmt in (F32, S16):
        L.check(lib.wlx_debug_resample(0, x.ctypes.data_as(C.c_void_p), n, ch, fmt, rate, 0, out.ctypes.data_as(f32p), cap, C.byref(got)))
    else:
        L.check(lib.wlx_debug_resample_stream(0, x.ctypes.data_as(C.c_void_p), n, ch, fmt, rate, None, 0, 2, out.ctypes.data_as(f32p), cap,
                                              C.byref(got), None))
    assert got.value == cap
    return out[:cap].view(np.uint32).copy()


def _many(specs):
    """one ragged launch over specs [(n, ch, fmt, rate, seed)] -> per entry float32 bits; checks that nothing else was written"""
    L, lib = _lib()
    n = len(specs)
    xs = [_frames(s[0], s[1], s[2], s[4]) for s in specs]
    lens = [_out_len(s[0], s[3]) for s in specs]
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum([v + 3 for v in lens[:-1]])                    # three floats between neighbours: a write past an entry shows
    cap = int(offs[-1] + lens[-1] + 3)
    out = np.full(cap, SENTINEL, np.float32)
    ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in xs])
    nfr = np.asarray([s[0] for s in specs], np.int64)
    chs = np.asarray([s[1] for s in specs], np.int32)
    fmts = np.asarray([s[2] for s in specs], np.int32)
    rates = np.asarray([s[3] for s in specs], np.int32)
    got = np.full(n, -1, np.int64)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.check(lib.wlx_debug_resample_many(0, n, ptrs, nfr.ctypes.data_as(i64p), chs.ctypes.data_as(i32p), fmts.ctypes.data_as(i32p),
                                        rates.ctypes.data_as(i32p), out.ctypes.data_as(C.POINTER(C.c_float)), offs.ctypes.data_as(i64p), cap,
                                        got.ctypes.data_as(i64p)))
    assert got.tolist() == lens
    mask = np.ones(cap, bool)
    res = []
    for k in range(n):
        a = int(offs[k])
        res.append(out[a:a + lens[k]].view(np.uint32))
        mask[a:a + lens[k]] = False
    assert (out[mask] == SENTINEL).all()
    return res


# (frames, channels, format, rate, seed). 48 kHz is 1 / 3: 3069, 3072 and 3075 frames give 1023, 1024 and 1025 outputs, one tile and one
# output into the second; 11025 Hz runs the smallest tile (64 outputs), 16 kHz the copy path
ONE_TILE = [(1, 1, F32, 8000, 1), (_reach(44100) - 1, 2, S16, 44100, 2), (3069, 1, F32, 48000, 3), (3072, 2, MULAW, 48000, 4),
            (1023, 1, F32, 16000, 5), (1024, 8, S16, 16000, 6), (40, 1, ALAW, 11025, 7), (1, 8, MULAW, 8000, 8)]
MANY_TILES = [(3075, 1, S16, 48000, 9), (1025, 2, F32, 16000, 10), (9000, 2, ALAW, 8000, 11), (7000, 1, F32, 11025, 12),
              (30000, 2, F32, 44100, 13), (5000, 8, F32, 8000, 14), (2500, 1, MULAW, 8000, 15), (12000, 1, S16, 44100, 16)]


def _check(specs):
    for spec, got in zip(specs, _many(specs)):
        want = _single(*spec[:4], spec[4])
        assert got.shape == want.shape and np.array_equal(got, want), spec


def test_every_entry_of_a_ragged_resample_launch_equals_the_single_entry_hook(gpu):
    mixed = [v for pair in zip(MANY_TILES, ONE_TILE) for v in pair]     # one-tile entries sit between many-tile entries
    _check(mixed)
    _check(list(reversed(mixed)))


@pytest.mark.parametrize("spec", [MANY_TILES[4], ONE_TILE[0], MANY_TILES[1]])
def test_a_ragged_launch_of_one_entry(gpu, spec):
    _check([spec])


def test_a_ragged_launch_of_64_entries(gpu):
    pool = ONE_TILE + MANY_TILES[:3] + MANY_TILES[6:7]
    _check([pool[(5 * k) % len(pool)] for k in range(64)])


def test_the_copy_path_keeps_a_negative_zero(gpu):
    got = _many([(1025, 1, F32, 16000, 10), (1023, 1, F32, 16000, 5)])
    for g, (n, seed) in zip(got, ((1025, 10), (1023, 5))):
        assert np.array_equal(g, _frames(n, 1, F32, seed)[:, 0].view(np.uint32)) and g[0] == 0x80000000


def test_bad_arguments_are_refused_before_any_launch(gpu):
    L, lib = _lib()
    x = _frames(100, 1, F32, 1)
    out = np.full(300, SENTINEL, np.float32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(n, rate, cap, off=0):
        ptrs = (C.c_void_p * 1)(x.ctypes.data)
        a = [np.asarray([v], t) for v, t in ((100, np.int64), (1, np.int32), (F32, np.int32), (rate, np.int32), (off, np.int64))]
        got = np.zeros(1, np.int64)
        return lib.wlx_debug_resample_many(0, n, ptrs, a[0].ctypes.data_as(i64p), a[1].ctypes.data_as(i32p), a[2].ctypes.data_as(i32p),
                                           a[3].ctypes.data_as(i32p), out.ctypes.data_as(C.POINTER(C.c_float)), a[4].ctypes.data_as(i64p), cap,
                                           got.ctypes.data_as(i64p))
    assert call(0, 8000, 300) == L.ERR_ARG and call(65, 8000, 300) == L.ERR_ARG
    assert call(1, 44101, 300) == L.ERR_ARG                              # an unserved rate
    assert call(1, 8000, 199) == L.ERR_ARG and call(1, 8000, 300, off=101) == L.ERR_ARG      # 200 outputs do not fit
    assert (out == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ FLAC
def _flac_single(data, cap):
    L, lib = _lib()
    out = np.full(cap, -123456789, np.int32)
    n, ch = C.c_int64(0), C.c_int32(0)
    L.check(lib.wlx_debug_flac_decode(0, data, len(data), out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n), C.byref(ch)))
    return out[: n.value * ch.value].reshape(n.value, ch.value)


def _flac_many(datas, sizes):
    """one ragged decode of the files -> (per entry int32 [n, ch], per entry status)"""
    L, lib = _lib()
    n = len(datas)
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum([v + 5 for v in sizes[:-1]])
    cap = int(offs[-1] + sizes[-1] + 5)
    out = np.full(cap, -123456789, np.int32)
    keep = [bytes(d) for d in datas]
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p).value for d in keep])
    nb = np.asarray([len(d) for d in keep], np.int64)
    nfr, chs, st = np.zeros(n, np.int64), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.check(lib.wlx_debug_flac_decode_many(0, n, ptrs, nb.ctypes.data_as(i64p), out.ctypes.data_as(i32p), offs.ctypes.data_as(i64p), cap,
                                           nfr.ctypes.data_as(i64p), chs.ctypes.data_as(i32p), st.ctypes.data_as(i32p)))
    res, mask = [], np.ones(cap, bool)
    for k in range(n):
        a, m = int(offs[k]), int(nfr[k] * chs[k])
        assert m == sizes[k]
        res.append(out[a:a + m].reshape(int(nfr[k]), int(chs[k])))
        mask[a:a + m] = False
    assert (out[mask] == -123456789).all()                                # nothing written between or behind the entries
    return res, st.tolist()


def test_every_entry_of_a_ragged_flac_decode_equals_the_single_file_hook_and_read_flac(gpu):
    from whisperlive_amd import audio_io
    wanted = ("bs16_8bit_mono_verbatim_last1", "bs17_16bit_stereo_fixed0to4", "bs192_24bit_midside_lpc8",
              "bs4096_16bit_leftside_lpc32_first_partition_empty", "bs300_24bit_sideright_25bit_side_escape24",
              "assignments_independent_leftside_sideright_midside", "k0_escape0_escape8_constant")
    by_name = {c["name"]: c for c in FC.cases()}
    files = [(by_name[nm]["data"], by_name[nm]["pcm"], by_name[nm]["bps"]) for nm in wanted]
    # entries of 63, 65, 1 and 64 frames in front: the second and the fourth straddle a 64-lane wave; then the case matrix
    counted = [_stream_of(63, 16, 8, 1, 1), _stream_of(65, 16, 16, 2, 2, FW.MID_SIDE), _stream_of(1, 4096, 24, 1, 3),
               _stream_of(64, 16, 16, 2, 4, FW.LEFT_SIDE), _stream_of(3, 4096, 16, 2, 5, FW.SIDE_RIGHT)]
    files = [(d, p, b) for (d, p), b in zip(counted, (8, 16, 24, 16, 16))] + files
    got, status = _flac_many([f[0] for f in files], [f[1].size for f in files])
    assert status == [0] * len(files)
    for (data, pcm, bps), g in zip(files, got):
        assert np.array_equal(g, pcm)
        assert np.array_equal(g, _flac_single(data, pcm.size))
        x, _ = audio_io.read_flac(data)
        assert np.array_equal(np.round(x.astype(np.float64) * (1 << (bps - 1))).astype(np.int64), g)


def test_a_frame_that_fails_on_the_device_costs_its_entry_alone(gpu):
    from whisperlive_amd import _lib as L
    good, pcm = _stream_of(5, 64, 16, 1, 7)
    bad = broken_frame_stream()
    got, status = _flac_many([good, bad[0], good], [pcm.size, bad[1].size, pcm.size])
    assert status == [0, L.ERR_DATA, 0]
    assert np.array_equal(got[0], pcm) and np.array_equal(got[2], pcm)
    assert not got[1][64:128].any()                                       # the failed frame's samples are zeros
    assert np.array_equal(got[1][:64], bad[1][:64]) and np.array_equal(got[1][128:], bad[1][128:])
