"""GPU: the audio front end's kernel through its one-launch-per-block hook (wlx_debug_resample) against scipy.signal.resample_poly
on float64 input, within RESAMPLE_ATOL (tests/resample_kernel_ref.py: four times the numpy restatement's own error)."""
import numpy as np
import pytest

from tests import resample_kernel_ref as R

pytestmark = pytest.mark.gpu


def _check(frames, rate, block_frames=0):
    up, down = R.ratio(rate)
    want = R.scipy_ref(R.mono_f32(frames), up, down)
    rc, out, n_out = R.run_hook(frames, rate, block_frames)
    assert rc == 0 and n_out == want.shape[0] == R.out_len(frames.shape[0], up, down)
    err = float(np.abs(out[:n_out].astype(np.float64) - want).max()) if n_out else 0.0
    assert np.all(out[n_out:] == np.float32(-7.25)), "floats past n_out were written"
    return err, out[:n_out]


@pytest.mark.parametrize("rate", R.RATES)
def test_grid_against_scipy(gpu, rate):
    worst = (0.0, None)
    for n in R.grid_lengths(rate):
        cases = [(name, x[:, None]) for name, x in R.grid_signals(n, rate).items()]
        cases += [(f"ch{ch}_fmt{fmt}", R.multichannel(n, rate, ch, fmt)) for fmt in (R.F32, R.S16) for ch in (1, 2, 6)]
        for name, frames in cases:
            err, _ = _check(frames, rate)
            if err > worst[0]:
                worst = (err, (n, name))
    print(f"{rate} Hz: max abs error {worst[0]:.3e} at {worst[1]} (bound {R.RESAMPLE_ATOL:.3e})")
    assert worst[0] <= R.RESAMPLE_ATOL, worst


@pytest.mark.parametrize("rate", R.STEEP_RATES)
def test_steep_rates_against_scipy(gpu, rate):
    """176.4 / 352.8 / 384 kHz run with tiles of 256 / 128 / 512 outputs: the same grid (1 s + 1 frame as the long length)"""
    worst = (0.0, None)
    for n in R.grid_lengths(rate, seconds=1):
        cases = [(name, x[:, None]) for name, x in R.grid_signals(n, rate).items()]
        cases += [("ch2_s16", R.multichannel(n, rate, 2, R.S16)), ("ch6_f32", R.multichannel(n, rate, 6, R.F32))]
        for name, frames in cases:
            err, _ = _check(frames, rate)
            worst = max(worst, (err, (n, name)))
    print(f"{rate} Hz: max abs error {worst[0]:.3e} at {worst[1]} (bound {R.RESAMPLE_ATOL_STEEP:.3e})")
    assert worst[0] <= R.RESAMPLE_ATOL_STEEP, worst


def test_served_rates_are_what_python_says(gpu):
    """engine.resample_supported is the library's rule: the hook serves a rate exactly when it says so, on both sides of each limit"""
    from whisperlive_amd.engine import resample_supported
    for rate in R.RATES + R.STEEP_RATES + [16000, 768000, R.STEEPEST_RATE, R.FIRST_REFUSED_STEEP_RATE, 10240000, 44101, 8001]:
        up, down = R.ratio(rate)
        x = R.grid_signals(down + 1, rate)["speech"] if max(up, down) <= 640 else np.zeros(8, np.float32)
        rc, out, n_out = R.run_hook(x, rate)
        assert (rc == 0) == resample_supported(rate, 1) and rc in (0, R.ERR_ARG), rate
        if rc == 0:
            assert n_out == R.out_len(x.shape[0], up, down), rate
        else:
            assert np.all(out == np.float32(-7.25)), rate


def test_restatement_predicts_the_kernel_at_the_steepest_rate(gpu):
    """1 / 159 fills the LDS to four floats with the smallest tile (64 outputs); three tiles and a bit"""
    rate = R.STEEPEST_RATE
    x = R.grid_signals(159 * (3 * 64 + 5) + 1, rate)["speech"]
    rc, out, n_out = R.run_hook(x, rate)
    assert rc == 0 and n_out == 3 * 64 + 6
    assert np.abs(out[:n_out] - R.resample_ref(x, *R.ratio(rate))).max() <= R.RESAMPLE_ATOL / 4
    assert np.all(out[n_out:] == np.float32(-7.25))


def test_restatement_predicts_the_kernel(gpu):
    """the numpy restatement is the kernel's arithmetic: at most a quarter of the tolerance apart (bit-equal but for double rounding)"""
    for rate in (11025, 44100, 192000):
        x = R.grid_signals(2 * rate // 10 + 1, rate)["speech"]
        rc, out, n_out = R.run_hook(x, rate)
        assert rc == 0
        assert np.abs(out[:n_out] - R.resample_ref(x, *R.ratio(rate))).max() <= R.RESAMPLE_ATOL / 4


@pytest.mark.parametrize("fmt", [R.F32, R.S16])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_16k_is_the_float32_channel_mean_bit_for_bit(gpu, channels, fmt):
    frames = R.multichannel(2049, 16000, channels, fmt)
    rc, out, n_out = R.run_hook(frames, 16000)
    assert rc == 0 and n_out == 2049
    x = frames.astype(np.float32) / np.float32(32768.0) if fmt == R.S16 else frames
    assert np.array_equal(out[:n_out], x.mean(axis=1) if channels > 1 else x[:, 0])
    if fmt == R.F32:                                                    # a negative zero stays one: the samples are copied, not filtered
        z = np.zeros((4, channels), np.float32)
        z[1::2] = np.float32(-0.0)
        rc, out, n_out = R.run_hook(z, 16000)
        assert rc == 0 and np.array_equal(out[:4].view(np.uint32), z[:, 0].view(np.uint32))
    assert np.all(out[n_out:] == np.float32(-7.25))


def _seam_block(up, down, hl):
    """a block_frames whose first seam (the frame after the first block's last) is one frame off a multiple of `down`"""
    for bf in range(R.reach(up, down) + 1, R.reach(up, down) + 20000):
        per = ((bf - 2) * up - 2 * hl) // down + 1
        seam = (hl + (per - 1) * down) // up + 1
        if per >= 2 and seam % down in (1, down - 1):
            return bf, seam
    raise AssertionError("no such block size")


@pytest.mark.parametrize("rate", [44100, 48000])
def test_block_seams_do_not_change_a_bit(gpu, rate):
    up, down = R.ratio(rate)
    hl = 10 * max(up, down)
    small = R.reach(up, down)                       # the smallest legal block: one output per launch
    frames = R.multichannel(3 * small + 7, rate, 2, R.F32)
    err, one = _check(frames, rate)                 # a single block
    assert err <= R.RESAMPLE_ATOL
    assert R.out_len(frames.shape[0], up, down) >= 3
    _, many = _check(frames, rate, small)
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))
    bf, seam = _seam_block(up, down, hl)
    frames = R.multichannel(3 * bf + 11, rate, 2, R.S16)
    assert seam < frames.shape[0] and seam % down in (1, down - 1)
    err, one = _check(frames, rate)
    assert err <= R.RESAMPLE_ATOL
    _, many = _check(frames, rate, bf)
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))


def test_refused_shapes_leave_the_output_untouched(gpu):
    x = R.multichannel(4000, 44100, 2, R.F32)
    up, down = R.ratio(44100)
    refused = [
        dict(rate=44100, channels=0), dict(rate=44100, channels=R.MAX_CHANNELS + 1),
        dict(rate=0), dict(rate=-44100), dict(rate=44100, n_frames=-1),
        dict(rate=44101), dict(rate=16001), dict(rate=7999),            # ratios over 640
        dict(rate=R.FIRST_REFUSED_STEEP_RATE),                          # 1 / 160: the span of the smallest tile does not fit the LDS
        dict(rate=44100, n_frames=1 << 62),                             # n_frames * up would leave int64
        dict(rate=44100, block_frames=R.reach(up, down) - 1), dict(rate=44100, block_frames=1), dict(rate=44100, block_frames=-5),
        dict(rate=44100, fmt=2),
    ]
    for kw in refused:
        rc, out, _ = R.run_hook(x, **kw)
        assert rc == R.ERR_ARG, kw
        assert np.all(out == np.float32(-7.25)), kw
    rc, out, n_out = R.run_hook(x[:300], 44100, R.reach(up, down))      # ... and the smallest legal block is served
    assert rc == 0 and n_out == R.out_len(300, up, down)
