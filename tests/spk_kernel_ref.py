"""numpy references and ctypes runners for the one-launch hooks of the speaker kernels (wlx_spk_debug_fbank / _conv / _pool).
The references work in float64 on the SAME fp16-rounded operands the kernel receives, so what is left between the two is the
kernel's fp32 accumulation and the fp16 rounding of its output: the project's standing bound of 2e-3 rel-rms covers both (one
fp16 rounding is 2^-11 / sqrt(3) = 2.8e-4 rel-rms; an fp32 sum of K <= 2304 products adds about sqrt(K) 2^-24 = 3e-6)."""
from __future__ import annotations

import ctypes as C

import numpy as np

REL_RMS = 2e-3

# (Cin, Cout, stride, ksize) of every MFMA convolution of ResNet34: conv1 / conv2 of the four stages, the three shortcuts
NETWORK_CONVS = [(32, 32, 1, 3), (32, 64, 2, 3), (64, 64, 1, 3), (64, 128, 2, 3), (128, 128, 1, 3), (128, 256, 2, 3), (256, 256, 1, 3),
                 (32, 64, 2, 1), (64, 128, 2, 1), (128, 256, 2, 1)]
# (H, W, Cin, Cout, stride, ksize): odd H and W under stride 2; W of 1, 2 and 17; H W not a multiple of the 16-pixel wave tile or
# the 64-pixel workgroup tile; the 40 pixels x K = 2304 of a 0.3 s segment in the last stage; one tile exactly; H = 5 with
# W = 1 / 17 under stride 2 with two and with four channel tiles per wave (one item: the launcher's table-free n = 1 kernel)
EDGE_CONVS = [(7, 9, 32, 64, 2, 3), (5, 3, 64, 128, 2, 3), (7, 9, 32, 64, 2, 1), (10, 1, 32, 32, 1, 3), (10, 1, 64, 128, 2, 3),
              (10, 2, 32, 32, 1, 3), (3, 17, 64, 64, 1, 3), (3, 17, 128, 256, 2, 3), (1, 1, 32, 32, 1, 3), (1, 5, 32, 64, 2, 1),
              (10, 4, 256, 256, 1, 3), (13, 5, 128, 128, 1, 3), (4, 4, 32, 32, 1, 3), (8, 8, 64, 64, 1, 3), (9, 29, 32, 96, 1, 3),
              (5, 1, 32, 32, 2, 3), (5, 1, 32, 64, 2, 3), (5, 17, 32, 32, 2, 3), (5, 17, 32, 64, 2, 3)]


def f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def rel_rms(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(((got - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-30))


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def conv_case(H, W, Cin, Cout, stride, ks, resid, seed=0):
    rng = np.random.default_rng(seed + 1000 * Cin + Cout + 7 * H + W)
    OH, OW = out_hw(H, W, stride)
    x = f16(rng.standard_normal((H, W, Cin)))
    w = f16(rng.standard_normal((Cout, Cin, ks, ks)) / np.sqrt(Cin * ks * ks)).astype(np.float32)
    b = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    r = f16(rng.standard_normal((OH, OW, Cout))) if resid else None
    return x, w, b, r


def conv_ref(x, w, b, r, stride, relu):
    """float64 convolution of x fp16 [H][W][Cin] with w [Cout][Cin][ks][ks] (padding ks // 2) -> [OH][OW][Cout]"""
    H, W, Cin = x.shape
    Cout, _, ks, _ = w.shape
    pad = ks // 2
    OH, OW = out_hw(H, W, stride)
    xp = np.zeros((H + 2 * pad, W + 2 * pad, Cin), dtype=np.float64)
    xp[pad:pad + H, pad:pad + W] = x.astype(np.float64)
    out = np.zeros((OH, OW, Cout), dtype=np.float64)
    w64 = w.astype(np.float64)
    for kh in range(ks):
        for kw in range(ks):
            tap = xp[kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            out += tap @ w64[:, :, kh, kw].T
    if b is not None:
        out += b.astype(np.float64)
    if r is not None:
        out += r.astype(np.float64)
    return np.maximum(out, 0.0) if relu else out


def pool_ref(x, eps):
    """x fp16 [F][T][C] -> float64 [2][C][F]: mean over T, sqrt(unbiased variance + eps)"""
    x64 = x.astype(np.float64)
    return np.stack([x64.mean(axis=1).T, np.sqrt(x64.var(axis=1, ddof=1) + eps).T])


# ------------------------------------------------------------------------------------------------ runners (need a GPU)
def _lib():
    from whisperlive_amd import _lib as L
    return L.load()


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def run_conv(x, w, b, r, stride, relu, fill=None):
    """(rc, out fp16 [OH][OW][Cout])"""
    H, W, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[2]
    OH, OW = out_hw(H, W, stride)
    x = np.ascontiguousarray(x)
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.full((OH, OW, Cout), np.nan if fill is None else fill, dtype=np.float16)
    rc = _lib().wlx_spk_debug_conv(0, _p(x.view(np.uint16), C.c_uint16), H, W, Cin, _p(w, C.c_float), _p(b, C.c_float),
                                   _p(None if r is None else np.ascontiguousarray(r).view(np.uint16), C.c_uint16), Cout, stride, ks,
                                   int(relu), _p(out.view(np.uint16), C.c_uint16))
    return rc, out


def run_pool(x, eps):
    F, T, Cn = x.shape
    x = np.ascontiguousarray(x)
    out = np.full((2, Cn, F), np.nan, dtype=np.float32)
    rc = _lib().wlx_spk_debug_pool(0, _p(x.view(np.uint16), C.c_uint16), F, T, Cn, float(eps), _p(out, C.c_float))
    return rc, out


def run_fbank(pcm, n_mels=80):
    """(rc, frames float32 [T][n_mels], image fp16 [n_mels][T])"""
    pcm = np.ascontiguousarray(pcm, dtype=np.float32)
    T = 1 + (len(pcm) - 400) // 160
    frames = np.full((T, n_mels), np.nan, dtype=np.float32)
    image = np.zeros((n_mels, T), dtype=np.float16)
    n = C.c_int32()
    rc = _lib().wlx_spk_debug_fbank(0, _p(pcm, C.c_float), len(pcm), n_mels, _p(frames, C.c_float), _p(image.view(np.uint16), C.c_uint16),
                                    T, C.byref(n))
    assert rc != 0 or n.value == T
    return rc, frames, image
