"""GPU tests of the speaker kernels of csrc/spk.hip, one launch each (a batch of one) through wlx_spk_debug_fbank / _conv / _pool,
against the float64 references of tests/spk_kernel_ref.py on the same fp16-rounded operands (bound: spk_kernel_ref.REL_RMS, derived
there) and, for the filterbank, the float64 restatement of tests/spk_oracle.py."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import logmel as olm

from . import spk_kernel_ref as R
from . import spk_oracle as O

pytestmark = pytest.mark.gpu

FBANK_ABS = 2e-3        # log units against the float64 oracle


@pytest.mark.parametrize("seconds", [0.3, 1.0, 7.3, 45.0])
def test_fbank(seconds):
    """Kaldi filterbank of speech-like audio: frame count 1 + (N - 400) // 160, every log-mel value (per-bin mean removed) within
    2e-3 of the float64 oracle, and the fp16 image the stem reads is exactly the rounding of those values, transposed."""
    pcm = olm.speech_like_pcm(seconds, seed=int(seconds * 10))[:int(round(seconds * 16000))].astype(np.float32)
    rc, frames, image = R.run_fbank(pcm)
    assert rc == 0
    ref = O.features(pcm)
    assert frames.shape == ref.shape == (O.n_frames(len(pcm)), 80)
    err = float(np.abs(frames.astype(np.float64) - ref).max())
    print(f"fbank {seconds} s: {frames.shape[0]} frames, max abs error {err:.3e} log units")
    assert np.isfinite(frames).all() and err <= FBANK_ABS, err
    assert (image.view(np.uint16) == frames.T.astype(np.float16).view(np.uint16)).all()


def test_fbank_of_silence_is_the_floor():
    """all-zero audio: every bin sits on the float32-epsilon floor log(2^-23) = -15.9, so the mean-subtracted features are zero to
    the rounding of an fp32 mean of 98 equal values (a few ulp of 16: under 1e-4)"""
    rc, frames, image = R.run_fbank(np.zeros(16000, dtype=np.float32))
    assert rc == 0 and np.abs(frames).max() <= 1e-4 and np.abs(image.astype(np.float32)).max() <= 1e-4


def _check_conv(H, W, Cin, Cout, stride, ks, resid, relu, bias=True):
    x, w, b, r = R.conv_case(H, W, Cin, Cout, stride, ks, resid)
    if not bias:
        b = None
    rc, got = R.run_conv(x, w, b, r, stride, relu)
    assert rc == 0
    ref = R.conv_ref(x, w, b, r, stride, relu)
    assert got.shape == ref.shape and np.isfinite(got.astype(np.float32)).all()      # (NaN fill: every output element was written)
    e = R.rel_rms(got, ref)
    print(f"conv {H}x{W} {Cin}->{Cout} s{stride} k{ks} resid={resid} relu={relu}: rel-rms {e:.3e}")
    assert e <= R.REL_RMS, e


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("Cin,Cout,stride,ks", R.NETWORK_CONVS)
def test_conv_network_shapes(Cin, Cout, stride, ks, resid):
    """every (Cin, Cout, stride) of ResNet34, 3 x 3 and the 1 x 1 shortcut, on a 20 x 37 image (740 pixels: 11 full workgroup tiles
    and a ragged one), plain and with residual + ReLU"""
    _check_conv(20, 37, Cin, Cout, stride, ks, resid, relu=resid)


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("H,W,Cin,Cout,stride,ks", R.EDGE_CONVS)
def test_conv_edge_shapes(H, W, Cin, Cout, stride, ks, resid):
    """spk_kernel_ref.EDGE_CONVS: odd H and W under stride 2, W of 1 / 2 / 17, H W off the tile, a single pixel, 40 pixels against
    K = 2304, a Cout that is a multiple of 32 only, H = 5 with W = 1 / 17 under stride 2 at Cout 32 and 64; ReLU on without residual
    and off with it"""
    _check_conv(H, W, Cin, Cout, stride, ks, resid, relu=not resid)


def test_conv_without_bias():
    _check_conv(6, 11, 64, 64, 1, 3, resid=False, relu=False, bias=False)


@pytest.mark.parametrize("stride,resid", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("H,W", [(80, 28), (7, 9), (3, 1)])
def test_conv_stem(H, W, stride, resid):
    """the first convolution (Cin = 1, K = 9) on the vector ALU"""
    x, w, b, r = R.conv_case(H, W, 1, 32, stride, 3, resid)
    rc, got = R.run_conv(x, w, b, r, stride, True)
    assert rc == 0
    e = R.rel_rms(got, R.conv_ref(x, w, b, r, stride, True))
    print(f"stem {H}x{W} s{stride} resid={resid}: rel-rms {e:.3e}")
    assert np.isfinite(got.astype(np.float32)).all() and e <= R.REL_RMS, e


@pytest.mark.parametrize("bad", [dict(Cin=48), dict(Cout=40), dict(stride=3), dict(ks=5), dict(Cin=1, ks=1)])
def test_conv_refuses_what_it_cannot_serve(bad):
    a = dict(H=4, W=4, Cin=32, Cout=32, stride=1, ks=3)
    a.update(bad)
    rng = np.random.default_rng(0)
    x = R.f16(rng.standard_normal((a["H"], a["W"], a["Cin"])))
    w = rng.standard_normal((a["Cout"], a["Cin"], a["ks"], a["ks"])).astype(np.float32)
    rc, out = R.run_conv(x, w, None, None, a["stride"], False, fill=7.0)
    assert rc == 1 and (out == np.float16(7.0)).all()


@pytest.mark.parametrize("T", [2, 563])
def test_pool(T):
    """statistics pooling of a 10 x T x 256 image (T = 563: the last stage of 45 s), channel-major mean then std; a tenth of the
    channels constant over time (variance exactly zero: std = sqrt(eps))"""
    rng = np.random.default_rng(T)
    x = R.f16(rng.standard_normal((10, T, 256)) * rng.uniform(0.1, 3.0, (10, 1, 256)) + rng.standard_normal((10, 1, 256)))
    x[:, :, ::10] = x[:, :1, ::10]
    eps = 1e-7
    rc, got = R.run_pool(x, eps)
    assert rc == 0 and np.isfinite(got).all()
    ref = R.pool_ref(x, eps)
    e_mean, e_std = R.rel_rms(got[0], ref[0]), R.rel_rms(got[1], ref[1])
    print(f"pool T={T}: rel-rms mean {e_mean:.3e} std {e_std:.3e}")
    assert e_mean <= R.REL_RMS and e_std <= R.REL_RMS
    # constant channels: the only deviation from sqrt(eps) is the fp32 rounding of the mean, at most T 2^-24 |x| per frame
    const = got[1][::10].astype(np.float64)
    slack = T * 2.0 ** -24 * float(np.abs(x[:, 0, ::10].astype(np.float64)).max())
    assert (const >= np.sqrt(eps) * (1 - 1e-6)).all() and (const <= np.sqrt(eps + slack ** 2) * (1 + 1e-6)).all()
