"""numpy references and ctypes runners for the one-launch hooks of the speaker kernels (wlx_spk_debug_fbank / _conv / _pool, and
below them wlx_spk_debug_fbank_batch / _head with bounds of their own, derived where they stand).
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


# ------------------------------------------------------------------------------------------------ ragged filterbank (wlx_spk_debug_fbank_batch)
U32 = 2.0 ** -24          # unit roundoff of fp32
MAX_BATCH = 64            # WLX_SPK_MAX_BATCH
FRAME, SHIFT = 400, 160
FBANK_FRAMES = (1, 2, 3, 255, 256, 257, 600)      # T = 1: the mean removal leaves exact zeros; the 256-thread stride edge; three trips
FBANK_SAMPLES = 128000                            # 8 s: every window of up to 600 frames (96240 samples) fits from any offset below
FBANK_MAX_OFFSET = FBANK_SAMPLES - (FRAME + SHIFT * (max(FBANK_FRAMES) - 1))
FBANK_CASES = ("n1", "n2", "n5", "n64", "overlap", "descending")


def item_samples(T):
    return FRAME + SHIFT * (T - 1)


def fbank_batch_case(name):
    """(pcm float32 [FBANK_SAMPLES], offsets int64 [n], frames int32 [n]): windows of one speech-like buffer at distinct ODD sample
    offsets (so no window starts on a 16-byte boundary), frame counts drawn from FBANK_FRAMES with every value present once n allows
    it and neighbours of different length. `overlap`: two windows that share most of their samples, as file diarization cuts them;
    `descending`: offsets falling while the items' packed positions rise."""
    from oracle import logmel as olm
    rng = np.random.default_rng(FBANK_CASES.index(name) + 77)
    pcm = olm.speech_like_pcm(FBANK_SAMPLES / 16000.0, seed=91)[:FBANK_SAMPLES].astype(np.float32)
    n = {"n1": 1, "n2": 2, "n5": 5, "n64": MAX_BATCH, "overlap": 3, "descending": 4}[name]
    if name == "n1":
        frames = [257]
    elif name == "n2":
        frames = [1, 600]
    elif name == "overlap":
        frames = [256, 255, 3]
    elif name == "descending":
        frames = [3, 257, 2, 256]
    elif name == "n5":
        frames = [600, 1, 255, 2, 257]
    else:
        perm = [int(t) for t in rng.permutation(FBANK_FRAMES)]
        frames = (perm * (n // len(perm) + 1))[:n]
        frames[-1] = perm[1]                               # (n = 64 = 9 * 7 + 1 would end on perm[0], the first item's length)
    offsets = 2 * rng.choice(FBANK_MAX_OFFSET // 2, size=n, replace=False) + 1
    if name == "overlap":
        offsets[1] = offsets[0] + 3 * SHIFT + 2            # 253 frames of item 1 lie inside item 0, shifted by two samples
    if name == "descending":
        offsets = np.sort(offsets)[::-1]
    frames = np.array(frames, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    assert (offsets % 2 == 1).all() and len(set(offsets.tolist())) == n and (offsets <= FBANK_MAX_OFFSET).all()
    assert all(frames[i] != frames[(i + 1) % n] for i in range(n)) or n == 1
    return pcm, offsets, frames


def fbank_batch_ref(pcm, offsets, frames, wrong=None):
    """float64 features of every item, [T_i][80] each (tests/spk_oracle.py: Kaldi filterbank, per-bin mean over the item's frames
    removed). `wrong` gives the nearest wrong answers of the ragged kernels: "offset" reads item i at item i + 1's sample offset,
    "mean" takes the mean over the NEXT item's frame count from item i's first packed frame on (spk_cmn_batch_kernel with another
    item's W), "in0" starts item i one packed frame late (the last item: one early)."""
    from . import spk_oracle as O
    n = len(frames)
    offs = [int(offsets[(i + 1) % n]) if wrong == "offset" else int(offsets[i]) for i in range(n)]
    raw = [O.fbank(pcm[offs[i]:offs[i] + item_samples(int(frames[i]))]) for i in range(n)]
    packed = np.concatenate(raw)
    in0 = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(int)
    out = []
    for i in range(n):
        T, a = int(frames[i]), int(in0[i])
        if wrong == "in0":
            a = a + 1 if i < n - 1 else a - 1
        rows = packed[a:a + T]
        Tm = int(frames[(i + 1) % n]) if wrong == "mean" else T
        out.append(rows - packed[a:a + Tm].sum(axis=0, keepdims=True) / Tm)       # (behind the last item: what the buffer holds)
    return out


def run_fbank_batch(pcm, offsets, frames, n=None, n_samples=None, n_mels=80, sentinel_rows=3):
    """(rc, frames_out float32 [sum T + sentinel_rows][n_mels], image_out fp16 [(sum T + sentinel_rows) * n_mels]); both preset to
    sentinel patterns (float32 bits 0xdeadbeef, fp16 bits 0xbeef) so that the caller can see what was written"""
    pcm = None if pcm is None else np.ascontiguousarray(pcm, dtype=np.float32)
    offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    frames = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
    n = len(frames) if n is None else n
    rows = int(np.maximum(frames, 0).sum()) + sentinel_rows if frames is not None else sentinel_rows
    out = np.full((rows, n_mels), 0xdeadbeef, dtype=np.uint32).view(np.float32)
    img = np.full(rows * n_mels, 0xbeef, dtype=np.uint16)
    rc = _lib().wlx_spk_debug_fbank_batch(0, _p(pcm, C.c_float), len(pcm) if n_samples is None else n_samples, n, _p(offsets, C.c_int64),
                                          _p(frames, C.c_int32), n_mels, _p(out, C.c_float), _p(img, C.c_uint16))
    return rc, out, img.view(np.float16)


# ------------------------------------------------------------------------------------------------ embedding head (wlx_spk_debug_head)
# (D, E, n): D = 8 one 8-wide piece on lane 0 alone; 504 / 512 / 520 around the 512-wide trip; 5120 the product's pool_dim. E around the
# l2norm's 256-thread stride. n = 64: WLX_SPK_MAX_BATCH rows in one launch. (5120, 256, 64) is the product's head at a full batch.
HEAD_CASES = ((8, 1, 1), (504, 3, 3), (512, 255, 64), (520, 257, 3), (5120, 512, 1), (5120, 256, 64))


def head_case(D, E, n, seed=0):
    """(pooled float32 [n][D], W float32 [E][D], b float32 [E]): seeded normal data, every pooled row and every row of W with a scale of
    its own, so that another item's row, a neighbour's bias or a shifted weight row is a different number and not a permutation of
    the same statistics"""
    rng = np.random.default_rng(seed + 7 * D + 3 * E + n)
    pooled = (rng.standard_normal((n, D)) * np.geomspace(0.3, 3.0, n)[:, None] + 0.1).astype(np.float32)
    W = (rng.standard_normal((E, D)) * (np.geomspace(0.5, 2.0, E)[:, None] / np.sqrt(D))).astype(np.float32)
    b = (0.5 * rng.standard_normal(E) + 0.05 * np.arange(E) / max(E, 1)).astype(np.float32)
    return pooled, W, b


def head_tiny_case():
    """D = 512, E = 3, n = 4 with b = 0: row 0 of `pooled` all zero (the head output is exactly zero), row 1 scaled so that its output
    has norm ~1e-18 (sum of squares ~1e-36: a normal fp32 number, far under any floor one might put under it), row 2 ordinary, row 3
    large (norm ~1e15)"""
    pooled, W, b = head_case(512, 3, 4, seed=5)
    b[:] = 0
    pooled[0] = 0
    y = head_linear_ref(pooled, W, b)
    pooled[1] *= np.float32(1e-18 / np.linalg.norm(y[1]))
    pooled[3] *= np.float32(1e15 / np.linalg.norm(y[3]))
    return pooled, W, b


def head_linear_ref(pooled, W, b, wrong=None):
    """float64 W16 x + b on the fp16-rounded W the kernel reads. `wrong`: "bias" adds the bias of output e + 1, "wshift" reads every
    weight row one element late, "tail" drops the last 8-wide piece of D, "item" takes the next item's pooled row."""
    x = np.asarray(pooled, np.float64)
    w = f16(W).astype(np.float64)
    bb = np.asarray(b, np.float64)
    if wrong == "bias":
        bb = np.roll(bb, -1)
    if wrong == "wshift":
        w = np.roll(w.reshape(-1), -1).reshape(w.shape)
    if wrong == "tail":
        w = w.copy()
        w[:, -8:] = 0
    if wrong == "item":
        x = np.roll(x, -1, axis=0)
    return x @ w.T + bb


def head_linear_bound(pooled, W, b):
    """per-output bound of |kernel - float64| for the linear layer, from the kernel's own summation tree (spk_linear_body): lane l owns the
    8-wide pieces at 8 l + 512 k and adds their products to one accumulator in order — a serial chain of L = 8 ceil(D / 512) terms at
    the most; wave_sum folds the 64 accumulators in 6 levels (xor 32, 16, .. 1: lane 0 ends with ((l, l + 32), + 16 ..)); lane 0 adds
    the bias. Every fp32 operation returns its exact result times (1 + delta), |delta| <= U32, so the error of the output is at most
    U32 times the sum of the magnitudes of every intermediate result on the way: the products (their own rounding when the compiler
    does not fuse them into the add), every partial sum of the chains, every node of the reduction tree and the output itself. That
    sum A is computed here in float64 in the kernel's order. An intermediate differs from its exact value by the error gathered below
    it, which is second order: each rounding is counted by at most depth = L + 7 results above it, hence the 1 / (1 - depth U32). The
    float64 reference's own error (D 2^-53 sum |w x|) is added. fp16 -> fp32 of W is exact; nothing here is near under- or overflow."""
    x = np.asarray(pooled, np.float64)
    w = f16(W).astype(np.float64)
    bb = np.asarray(b, np.float64)
    n, D = x.shape
    E = w.shape[0]
    trips = -(-D // 512)
    Dp = trips * 512
    wp = np.zeros((E, Dp))
    wp[:, :D] = w
    real = (np.arange(Dp) < D).reshape(trips, 64, 8).transpose(1, 0, 2).reshape(64, trips * 8)      # the adds that exist
    bound = np.zeros((n, E))
    for r in range(n):
        xp = np.zeros(Dp)
        xp[:D] = x[r]
        p = wp * xp
        chain = np.cumsum(p.reshape(E, trips, 64, 8).transpose(0, 2, 1, 3).reshape(E, 64, trips * 8), axis=2)
        S = np.abs(p).sum(axis=1)
        A = S + (np.abs(chain) * real).sum(axis=(1, 2))
        v = chain[:, :, -1]
        for o in (32, 16, 8, 4, 2, 1):
            v = v[:, :o] + v[:, o:2 * o]
            A += np.abs(v).sum(axis=1)
        A += np.abs(v[:, 0] + bb)
        bound[r] = U32 * A / (1 - (trips * 8 + 7) * U32) + D * 2.0 ** -53 * (S + np.abs(bb))
    return bound


def head_norm_ref(y, wrong=None):
    """y / |y| per row in float64, an all-zero row staying zero. `wrong` = "ss256": the sum of squares over the first 256 elements only
    (spk_l2norm_body without its stride loop)"""
    y = np.asarray(y, np.float64)
    nrm = np.linalg.norm(y[:, :256] if wrong == "ss256" else y, axis=1, keepdims=True)
    return np.divide(y, nrm, out=np.zeros_like(y), where=nrm > 0)


def head_norm_bound(y, by):
    """bound of |kernel - float64| behind the l2norm for linear outputs y (float64, exact) known to by = head_linear_bound. The kernel
    normalises its own yh = y + e, |e_i| <= by_i. With m = |y| - |by| <= |yh|:
        yh / |yh| - y / |y| = e / |yh| + y (|y| - |yh|) / (|y| |yh|),  ||yh| - |y|| = |2 y.e + e.e| / (|yh| + |y|) <= (2 sum |y_j| by_j + |by|^2) / 2 m
    so the move is at most d_i = by_i / m + |z_i| (sum_j |y_j| by_j + |by|^2 / 2) / m^2 with z = y / |y|. Then the kernel's own arithmetic
    on yh (spk_l2norm_body): the sum of squares is a sum of positive terms — per thread a chain of ceil(E / 256) squares, 6 levels of
    wave_sum, 3 adds over the four waves: relative error g = (ceil(E / 256) + 9) U32 / (1 - ..), plus 2^-150 absolute for each of at most 2 E
    results that could fall into the subnormal range; sqrtf to 1 ulp and the division to 2.5 ulp (what the compiler promises without its
    correctly-rounded default: 2 U32 and 5 U32), the final product one rounding: relative error of an output
    rho = (g / 2 + 8 U32) (1 + 2^-10) over its exact value yh_i / |yh|, which is at most |z_i| + d_i. A zero row (by = 0) has bound 0."""
    y = np.asarray(y, np.float64)
    by = np.asarray(by, np.float64)
    E = y.shape[1]
    out = np.zeros_like(y)
    for r in range(y.shape[0]):
        ny, nb = np.linalg.norm(y[r]), np.linalg.norm(by[r])
        if ny == 0:
            assert nb == 0
            continue
        m = ny - nb
        assert m > 0.5 * ny
        z = np.abs(y[r]) / ny
        d = by[r] / m + z * ((np.abs(y[r]) * by[r]).sum() + 0.5 * nb * nb) / (m * m)
        k = -(-E // 256) + 9
        g = k * U32 / (1 - k * U32) + 2 * E * 2.0 ** -150 / (m * m)
        rho = (0.5 * g + 8 * U32) * (1 + 2.0 ** -10)
        out[r] = d + rho * (z + d) + 2.0 ** -52 * z
    return out


def excess(got, ref, bound):
    """max |got - ref| / bound; an element with bound 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return q


def run_head(pooled, W, b, normalize, n=None, D=None, E=None, extra_rows=2):
    """(rc, emb float32 [n + extra_rows][E]) preset to the bits 0xdeadbeef"""
    nn, DD = pooled.shape if pooled is not None else (1, 8)
    EE = len(b) if b is not None else 1
    n, D, E = nn if n is None else n, DD if D is None else D, EE if E is None else E
    pooled = None if pooled is None else np.ascontiguousarray(pooled, np.float32)
    W = None if W is None else np.ascontiguousarray(W, np.float32)
    b = None if b is None else np.ascontiguousarray(b, np.float32)
    emb = np.full((max(nn, 1) + extra_rows, max(EE, 1)), 0xdeadbeef, dtype=np.uint32).view(np.float32)
    rc = _lib().wlx_spk_debug_head(0, _p(pooled, C.c_float), _p(W, C.c_float), _p(b, C.c_float), n, D, E, int(normalize), _p(emb, C.c_float))
    return rc, emb
