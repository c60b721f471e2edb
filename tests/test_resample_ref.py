"""CPU: the numpy restatement of the resampling kernel (tests/resample_kernel_ref.py) against scipy.signal.resample_poly on float64
input — the comparison that fixes RESAMPLE_ATOL for the GPU tests."""
import numpy as np
import pytest

from tests import resample_kernel_ref as R


@pytest.fixture(scope="module")
def grid_errors():
    """(rate, n, signal) -> max abs error of the restatement against scipy, computed once"""
    errs = {}
    for rate in R.RATES:
        up, down = R.ratio(rate)
        for n in R.grid_lengths(rate):
            for name, x in R.grid_signals(n, rate).items():
                got, want = R.resample_ref(x, up, down), R.scipy_ref(x, up, down)
                assert got.dtype == np.float32 and got.shape == want.shape, (rate, n, name, got.shape, want.shape)
                errs[(rate, n, name)] = float(np.abs(got - want).max())
    return errs


@pytest.mark.parametrize("rate", R.RATES)
def test_taps_match_firwin(rate):
    from scipy.signal import firwin
    up, down = R.ratio(rate)
    hl, h = R.design(up, down)
    assert hl == 10 * max(up, down) and max(up, down) <= 640 and (2 * hl + 1) * 4 <= 51 * 1024
    want = up * firwin(2 * hl + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    assert np.abs(h - want).max() <= 1e-12


@pytest.mark.parametrize("rate", R.RATES)
def test_output_length_is_scipys(rate):
    from scipy.signal import resample_poly
    up, down = R.ratio(rate)
    for n in R.grid_lengths(rate):
        assert R.out_len(n, up, down) == resample_poly(np.zeros(n), up, down).shape[0]


def test_restatement_within_a_quarter_of_the_tolerance(grid_errors):
    worst = max(grid_errors, key=grid_errors.get)
    print(f"restatement vs scipy: max abs error {grid_errors[worst]:.4e} at {worst}")
    assert grid_errors[worst] <= R.RESAMPLE_ATOL / 4, (worst, grid_errors[worst])


def test_tolerance_is_under_half_a_16_bit_lsb():
    assert R.RESAMPLE_ATOL < 2 ** -16
    assert R.RESAMPLE_ATOL_STEEP < 2 ** -16


def test_restatement_within_a_quarter_of_the_steep_tolerance():
    worst = (0.0, None)
    for rate in R.STEEP_RATES:
        up, down = R.ratio(rate)
        for n in R.grid_lengths(rate, seconds=1):
            for name, x in R.grid_signals(n, rate).items():
                got, want = R.resample_ref(x, up, down), R.scipy_ref(x, up, down)
                assert got.shape == want.shape
                worst = max(worst, (float(np.abs(got - want).max()), (rate, n, name)))
    print(f"restatement vs scipy, steep rates: max abs error {worst[0]:.4e} at {worst[1]}")
    assert worst[0] <= R.RESAMPLE_ATOL_STEEP / 4, worst


def test_python_restates_the_librarys_served_rates():
    """engine.resample_supported (what transcribe asks before it takes the device route) on both sides of each limit"""
    from whisperlive_amd.engine import resample_supported
    for rate in R.RATES + R.STEEP_RATES + [16000, 768000, R.STEEPEST_RATE]:
        assert resample_supported(rate, 2), rate
    for rate in (R.FIRST_REFUSED_STEEP_RATE, 10240000, 44101, 16001, 7999, 0, -8000):
        assert not resample_supported(rate, 2), rate
    assert resample_supported(44100, 8) and not resample_supported(44100, 9) and not resample_supported(44100, 0)


def test_sixteen_khz_is_the_channel_mean_bit_for_bit():
    x = R.multichannel(257, 16000, 2, R.F32)
    assert np.array_equal(R.resample_ref(R.mono_f32(x), 1, 1), x.mean(axis=1))
    x6 = R.multichannel(257, 16000, 6, R.F32)
    assert np.array_equal(R.mono_f32(x6), x6.mean(axis=1))


def test_mono_of_int16_is_read_wavs_scaling():
    x = R.multichannel(100, 16000, 1, R.S16)
    assert np.array_equal(R.mono_f32(x), x[:, 0].astype(np.float32) / 32768.0)
