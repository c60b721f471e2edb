"""GPU: the channel-split instantiation of the audio front end's kernel through its hook (wlx_debug_resample_split): row c of the
output is BIT-IDENTICAL to wlx_debug_resample of the one-channel array frames[:, c] — the split form reads sample r * channels + c
where the mono form reads sample r, and shares everything else."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_kernel_ref as R

pytestmark = pytest.mark.gpu

FILL = np.float32(-7.25)
EXTRA = 5
TILE = 1024                 # outputs per workgroup at every rate below (csrc/resample.hip RS_TILE: none of them is steep enough to halve it)


def run_split(frames, rate, block_frames=0, rows=None, channels=None, fmt=None):
    """wlx_debug_resample_split on [n, ch] frames -> (rc, out [rows][cap] pre-filled with FILL, n_out); rows >= channels leaves
    unused rows behind the written ones"""
    from whisperlive_amd import _lib
    lib = _lib.load()
    x = np.asarray(frames)
    f = (R.S16 if x.dtype == np.int16 else R.F32) if fmt is None else fmt
    x = np.ascontiguousarray(x, dtype=np.int16 if x.dtype == np.int16 else np.float32)
    ch = x.shape[1] if channels is None else channels
    served = rate > 0 and max(R.ratio(rate)) <= 640
    cap = (R.out_len(x.shape[0], *R.ratio(rate)) if served else 0) + EXTRA
    out = np.full((rows if rows is not None else max(ch, 1) + 1, cap), FILL, np.float32)
    n_out = C.c_int64(-1)
    rc = lib.wlx_debug_resample_split(0, x.ctypes.data_as(C.c_void_p), x.shape[0], ch, f, rate, block_frames,
                                      out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n_out))
    return rc, out, n_out.value


def _frames(n, rate, channels, fmt):
    """channels with DIFFERENT contents: R.multichannel's, but channel 1 (when there is one) all zeros and channel FULL(channels)
    full scale, so a leak between channels cannot hide; at 16 kHz float32 every fourth frame of the silent channel (of channel 0 of
    a mono file) is a negative zero"""
    x = R.multichannel(n, rate, channels, fmt).copy()
    if channels > 1:
        x[:, 1] = 0
        x[:, FULL(channels)] = 32767 if fmt == R.S16 else 1.0
    if rate == 16000 and fmt == R.F32:
        x[::4, min(1, channels - 1)] = np.float32(-0.0)
    return x


def FULL(channels):
    """the full-scale channel: the last one, or channel 0 of a stereo file (whose last channel is the silent one)"""
    return channels - 1 if channels > 2 else 0


def _check(frames, rate, block_frames=0):
    ch = frames.shape[1]
    rc, out, n_out = run_split(frames, rate, block_frames)
    assert rc == 0 and n_out == R.out_len(frames.shape[0], *R.ratio(rate))
    for c in range(ch):
        rc1, one, n1 = R.run_hook(np.ascontiguousarray(frames[:, c:c + 1]), rate, block_frames)
        assert rc1 == 0 and n1 == n_out
        assert np.array_equal(out[c, :n_out].view(np.uint32), one[:n_out].view(np.uint32)), ("channel", c)
    assert np.all(out[:ch, n_out:] == FILL), "floats behind a row's n_out were written"
    assert np.all(out[ch:] == FILL), "an unused row was written"
    return out[:ch, :n_out]


@pytest.mark.parametrize("fmt", [R.F32, R.S16], ids=["f32", "s16"])
@pytest.mark.parametrize("rate", [16000, 8000, 48000, 44100, 11025])
def test_each_channel_is_bit_identical_to_the_mono_kernel_on_that_channel(gpu, rate, fmt):
    up, down = R.ratio(rate)
    tile = TILE
    # output counts 1 (or the fewest an up-sampling rate gives), one below, at and one above the tile: the frame counts on both sides
    # of each target, since ceil(n up / down) skips counts when up > down
    ns = sorted({max(1, q) for t in (1, tile - 1, tile, tile + 1) for q in (t * down // up, -(-t * down // up))})
    outs = [R.out_len(n, up, down) for n in ns]
    assert outs[0] == R.out_len(1, up, down) and any(o < tile for o in outs[1:]) and tile in outs and any(o > tile for o in outs)
    for channels in (1, 2, 3, 8):
        for n in ns:
            got = _check(_frames(n, rate, channels, fmt), rate)
            if channels > 1:                                     # nothing leaks: the silent channel stays silent beside a full-scale one
                assert not got[1].any() and np.abs(got[FULL(channels)]).max() > 0.5
    if rate == 16000 and fmt == R.F32:
        x = _frames(64, rate, 2, fmt)
        got = _check(x, rate)
        assert np.array_equal(got.view(np.uint32), x.T.view(np.uint32)) and (got[1].view(np.uint32)[::4] == 0x80000000).all()


def _seam_block(up, down, hl):
    """a block_frames a few frames over the filter's reach whose first seam is one frame off a multiple of `down`
    (tests/test_gpu_resample_kernels.py _seam_block)"""
    for bf in range(R.reach(up, down) + 1, R.reach(up, down) + 20000):
        per = ((bf - 2) * up - 2 * hl) // down + 1
        seam = (hl + (per - 1) * down) // up + 1
        if per >= 2 and seam % down in (1, down - 1):
            return bf, seam
    raise AssertionError("no such block size")


@pytest.mark.parametrize("rate", [8000, 48000, 44100, 11025])
def test_block_seams_do_not_change_a_bit_of_any_channel(gpu, rate):
    up, down = R.ratio(rate)
    bf, seam = _seam_block(up, down, 10 * max(up, down))
    frames = _frames(3 * bf + 11, rate, 3, R.S16)
    assert seam < frames.shape[0]
    one = _check(frames, rate)                                   # a single block ...
    many = _check(frames, rate, bf)                              # ... and blocks at the filter's reach plus a few frames
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))


def test_refused_shapes_leave_the_output_untouched(gpu):
    x = R.multichannel(4000, 44100, 2, R.F32)
    for kw in (dict(rate=44100, channels=0), dict(rate=44100, channels=R.MAX_CHANNELS + 1), dict(rate=44101), dict(rate=44100, fmt=2)):
        rc, out, _ = run_split(x, rows=R.MAX_CHANNELS + 2, **kw)
        assert rc == R.ERR_ARG, kw
        assert np.all(out == FILL), kw
