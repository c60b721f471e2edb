"""float64 references of the decode GEMV chain (csrc/dec_gemv.hip dec_gemv2_kernel, dec_vocab.hip dec_vocab_kernel) and of the fused
dec_cq_cross_attn_kernel (csrc/decoder.hip) as the wlx_debug_dec_gemv / wlx_debug_dec_cq_cross_attn hooks launch them one at a time,
their per-element error bounds, the nearest plausible wrong answers the bounds must exclude, the case list and the hook runners. The
pattern is tests/whisper_kernel_ref.py's, whose U16 / U32 / SUB16 / SLACK, excess, garbage, ln_ref / ln_bound, acc_bound, to16 and
cross-attention reference are used here, not copied. No figure observed on a GPU enters a bound.

What a launch computes, read from the kernels (IN, OUT, XS are the template arguments GemvIn, GemvOut, GemvXsrc):
  rows   IN_LN   h = fp16(LayerNorm(x) gamma + beta) over K columns, two-pass statistics, eps = 1e-5 inside the square root, with
                 x = X (XS PLAIN), x = (X + slab 0) + slab 1 in fp32 (SLABS), or x = float(tok_emb[token]) + pos_emb[position]
                 in fp32 (EMBED; workgroup 0 also stores x to X and the token to intok[cache row][position]);
         IN_F16  h = Xh;
         IN_XATTN h = fp16(sum_sp w_sp o_sp / sum_sp w_sp), w_sp = exp(m_sp - max m) l_sp over the eight split partials of row m's
                 group m / R, query lane m % R;
  acc    = sum_k h_k w_k with w = fp16(W), fp32 accumulation, the K range cut over waves (and over the two K slices of OUT_SLAB);
  o      = acc + bias (OUT_F32 without a bias — the vocabulary projection: o = acc);
  stores OUT_F16 Yh = fp16(o qscale); OUT_GELU_F16 Yh = fp16(gelu_erf(o) qscale); OUT_F32 Y = o; OUT_RESID Xres = r + o with r = Xres
         or, XS SLABS, r = (Xres + slab 0) + slab 1 — the sum is written back to Xres, the slabs stay as they are; OUT_SLAB
         slab[s] = acc of K slice s (+ bias on slice 0 ONLY: `if (blockIdx.y != 0) bias_e = 0`), nothing else is written;
         OUT_QKV columns [0, d) Yh = fp16(o qscale), columns [d, 2d) / [2d, 3d) to Kc / Vc at row_cache[m] * cache_row_stride +
         row_pos[m] * d, fp16(o) unscaled.

Bounds (first order, SLACK on every product of relative terms as in whisper_kernel_ref):
  h      IN_LN: ln_bound's b16 — the prologue is layernorm_kernel's arithmetic (float4 partial sums, six DPP levels, mean by a
         rounded reciprocal, rsqrtf, three roundings of the output) — plus, for SLABS / EMBED, the row's own fp32 additions: the
         row is off by dx_i <= 2 U32 (|X| + |s0| + |s1|)_i (EMBED: U32 |x_i|); with dxm = max_i dx_i the mean moves by <= dxm and,
         since d rstd / d x_j = -rstd^3 (x_j - mean) / d and sqrt(var) rstd <= 1, rstd by <= 2 dxm rstd^2: the fp32 value moves by
         <= |gamma| rstd dxm (2 + 2 |x - mean| rstd), which is added to e32 before the fp16 rounding.
         IN_XATTN: a weight w_sp carries the exponential (2 ulp of an argument of size <= Rm = max m - min m: 4 (Rm + 1) U32, Rm
         clamped at 104 as in xa_ref) and one product: ew = (4 (Rm + 1) + 2) U32; numerator and denominator are eight products and
         additions each, then a reciprocal and a product: e32 = (2 ew + 20 U32) sum_sp f_sp |o_sp|, f_sp = w_sp / sum w; fp16: to16.
         IN_F16: exact.
  acc    |kernel - float64| <= sum_k bh_k |w_k| (the kernel's fp16 rows against the unrounded float64 rows) + acc_bound(sum_k (|h_k|
         + bh_k) |w_k|, K): K fp32 accumulation steps in whatever association — the split over waves, chunks and the cross-wave
         sum through LDS are an association of the same K - 1 additions.
  o      one more rounding: e_o = e_acc + U32 (|o| + e_acc).
  stores F16 / QKV q: qscale e_o + U32 |y|, then to16; K / V: to16(o, e_o); GELU: 1.13 e_o + 0.5 |o| E_ERF + 4 U32 (|g| + |o|)
         (gemm_logical's derivation for the same gelu_erf), then to16; F32: e_o (no bias: e_acc); RESID: e_o + U32 |r + o| + the
         two roundings of r under SLABS, 2 U32 (|Xres| + |s0| + |s1|); SLAB: e_o of the slice (K / 2 steps).

Out of scope: the (IN, OUT, XS) instantiations of the pick sweep the engine never builds (the split combine with more than one row
tile, slab rows under more than one row tile outside the prompt prefill, fp32 rows out with a bias) and the first-generation
dec_gemv_kernel."""
from __future__ import annotations

import numpy as np

from . import whisper_kernel_ref as R
from .mt_kernel_ref import SUB16, U16, U32, _f16, _ptr
from .whisper_kernel_ref import SLACK, acc_bound, excess, garbage, ln_bound, ln_ref, to16

IN_LN, IN_F16, IN_XATTN = 0, 1, 2
OUT_F16, OUT_GELU, OUT_F32, OUT_RESID, OUT_QKV, OUT_SLAB = range(6)
X_PLAIN, X_SLABS, X_EMBED = 0, 1, 2
KS = 2                      # WLX_FC2_KS
XSPLIT, T_TEXT = R.XSPLIT, R.T_TEXT
MAX_ROWS = 320              # WLX_MAX_DEC_ROWS
NAME_CAP = 96


def spec(inm, out, xs, M, K, N, name, busy=0, d=0, Rq=5, ):
    return dict(inm=inm, out=out, xs=xs, M=M, K=K, N=N, name=name, busy=busy, d=d, Rq=Rq)


def spec_id(s):
    return "in%d-out%d-xs%d-M%d-K%d-N%d%s%s" % (s["inm"], s["out"], s["xs"], s["M"], s["K"], s["N"], "-busy" if s["busy"] else "",
                                                ("-R%d" % s["Rq"]) if s["inm"] == IN_XATTN else "")


def family(s):
    return "in%d_out%d_xs%d" % (s["inm"], s["out"], s["xs"])


# ------------------------------------------------------------------ the case list
# (in, out, xs, M, K, N, kernel name launch_dec_gemv runs [, busy_device, QKV width d, R of the split combine]). The names are the
# answers of dec_gemv_kernel_name on an MI355X (256 CUs enter the 32- / 48-row tile rule of the residual projections), pinned here as
# tests/test_gemv_picks.py pins the engine's shapes. N is two to eight 16-column tiles unless a launch rule reads it: the four-tile
# forms need N / 16 >= 128 and a multiple of 4 (N = 2048; QKV: d = 704, N = 2112), the 32- / 48-row tiles more workgroups than CUs
# (N = d_model), large-v3's first MLP projection is N = 5120 (at 16 rows two column tiles of one row tile; at 17..32 rows two row tiles;
# at 48 rows gemv_chunked cuts it into 16-row tiles of four column tiles, so the two-to-one LDS fallback of gemv2_cfg_staging is not
# reached through launch_dec_gemv any more — the case pins what runs). A QKV launch splits its columns at d = N / 3, which the kernel reads
# from GemvParams::d, not from K.
G2 = "dec_gemv2_kernel<%s>"
VOC = "dec_vocab_kernel<%s>"


# ------------------------------------------------------------------ inputs
def gv_case(s, seed=0):
    """inputs and garbage-filled destinations of one launch. Rows: X N(0.3, 1) (slabs +-(0.25 + 0.5 |N(0, 1)|): never near zero, and LayerNorm
    statistics over X alone are far off), Xh 1 + N(0, 1), partials 1 + N(0, 1) with m = 2 N(0, 1) and l in [1, 100]; gamma with zeros and negative entries,
    beta 1 + 0.5 N(0, 1); W = (1 + N(0, 1)) / sqrt(K): with rows of mean ~1 every k-tile carries ~32 / sqrt(K) >= 0.45 of every
    output and every K slice sqrt(K) / 2 of it, far above the bounds (<= 0.1, test_dec_gemv_kernel_ref.py asserts it); bias 3 N(0, 1), under
    GELU shifted so that o spreads over [-4, 4]. Every stride is wider than its row, every destination holds two rows more than
    M, the caches one position more than the highest in use; gaps, spare rows, unaddressed cache rows / positions and the
    other slabs hold +-1000."""
    inm, out, xs, M, K, N = s["inm"], s["out"], s["xs"], s["M"], s["K"], s["N"]
    rng = np.random.default_rng(seed * 1000003 + inm * 7 + out * 11 + xs * 13 + M * 17 + K * 3 + N + s["busy"] + s["Rq"] * 29)
    c = dict(s, KT=K // 32, KTS=K // 64 if out == OUT_SLAB else 0, H=K // 64, qscale=0.125 if out in (OUT_QKV, OUT_F16) else 1.0)
    if out == OUT_QKV:
        c["d"] = s["d"] or N // 3
    MR = M + 2
    c["W"] = ((1 + rng.standard_normal((N, K))) / np.sqrt(K)).astype(np.float32)
    c["bias"] = None if (out == OUT_F32) else (3 * rng.standard_normal(N)).astype(np.float32)
    ldres = N + 4
    slab_used = xs == X_SLABS or out == OUT_SLAB
    if inm == IN_LN:
        ldx = K + 4
        c["ldx"] = ldx
        X = garbage(rng, MR * ldx)
        if xs != X_EMBED:
            X.reshape(MR, ldx)[:M, :K] = 0.3 + rng.standard_normal((M, K))
        c["X"] = X.astype(np.float32)
        g = rng.standard_normal(K)
        g[::7] = 0.0
        g[3::11] = -np.abs(g[3::11]) - 0.5
        c["gamma"] = g.astype(np.float32)
        c["beta"] = (1.0 + 0.5 * rng.standard_normal(K)).astype(np.float32)
        sld = ldx
        sw = K
    elif inm == IN_F16:
        c["ldxh"] = K + 8
        Xh = garbage(rng, MR * c["ldxh"])
        Xh.reshape(MR, -1)[:M, :K] = 1.0 + rng.standard_normal((M, K))
        c["Xh"] = _f16(Xh)
        sld, sw = ldres, N
    else:
        Rq, H = s["Rq"], K // 64
        G = -(-M // Rq)
        c["groups"] = G
        c["part_o"] = _f16(1.0 + rng.standard_normal((G, H, XSPLIT, 16, 64)))
        ml = np.zeros((G, H, 16, XSPLIT, 2))
        ml[..., 0] = 2 * rng.standard_normal((G, H, 16, XSPLIT))
        ml[..., 1] = rng.uniform(1, 100, (G, H, 16, XSPLIT))
        c["part_ml"] = ml.astype(np.float32)
        sld, sw = ldres, N
    if slab_used:
        c["slab_stride"] = MR * sld + 8
        sl = garbage(rng, KS * c["slab_stride"])
        if xs == X_SLABS:
            for q in range(KS):
                v = rng.standard_normal((M, sw))
                sl[q * c["slab_stride"]:q * c["slab_stride"] + MR * sld].reshape(MR, sld)[:M, :sw] = np.sign(v) * (0.25 + 0.5 * np.abs(v))
        c["slab"] = sl.astype(np.float32)
        c["sld"], c["sw"] = sld, sw
    if out == OUT_QKV:
        d = c["d"]
        pos_all = rng.permutation(40)[:M] if M <= 40 else np.arange(M) % 40
        cache_rows = M + 3
        c["row_pos"] = np.asarray(pos_all, np.int32)
        c["row_cache"] = rng.permutation(cache_rows)[:M].astype(np.int32)
        c["npos"] = int(c["row_pos"].max()) + 2
        c["crs"] = c["npos"] * d + 8
        c["cache_rows"] = cache_rows
        c["Kc"] = _f16(garbage(rng, cache_rows * c["crs"]))
        c["Vc"] = _f16(garbage(rng, cache_rows * c["crs"]))
        c["ldyh"] = d + 8
        c["Yh"] = _f16(garbage(rng, MR * c["ldyh"]))
        if xs == X_EMBED:
            ntok = 37
            c["tok_emb"] = _f16(0.3 + rng.standard_normal((ntok, K)))
            c["pos_emb"] = (0.5 * rng.standard_normal((c["npos"], K))).astype(np.float32)
            c["emb_token"] = rng.integers(0, ntok, M).astype(np.int32)
            c["intok"] = rng.integers(-9999, -1, cache_rows * T_TEXT).astype(np.int32)
    elif out in (OUT_F16, OUT_GELU):
        c["ldyh"] = N + 8
        c["Yh"] = _f16(garbage(rng, MR * c["ldyh"]))
    elif out == OUT_F32:
        c["ldy"] = (N + 3) // 4 * 4 + 4
        c["Y"] = garbage(rng, MR * c["ldy"]).astype(np.float32)
    if out in (OUT_RESID, OUT_SLAB):
        c["ldxres"] = ldres
    if out == OUT_RESID:
        Xr = garbage(rng, MR * ldres)
        Xr.reshape(MR, ldres)[:M, :N] = rng.standard_normal((M, N))
        c["Xres"] = Xr.astype(np.float32)
    if out == OUT_GELU:        # centre o: bias = -(column mean of acc) + 1.5 N(0, 1)
        acc = gv_rows(c)[0] @ gv_w16(c).T
        c["bias"] = (-acc.mean(0) + 1.5 * rng.standard_normal(N)).astype(np.float32)
    return c


def gv_w16(c):
    return c["W"].astype(np.float16).astype(np.float64)


def _slabs(c):
    M, ld, w, st = c["M"], c["sld"], c["sw"], c["slab_stride"]
    return [c["slab"][q * st:q * st + M * ld].reshape(M, ld)[:, :w].astype(np.float64) for q in range(KS)]


def gv_xrows(c, wrong=None):
    """(x float64 [M][K], dx bound of the kernel's fp32 row) of a LayerNorm prologue. wrong: "slab_missing" (slab 1 not added),
    "slab_twice" (slab 0 added twice)"""
    M, K = c["M"], c["K"]
    if c["xs"] == X_EMBED:
        x = c["tok_emb"][c["emb_token"]].astype(np.float64) + c["pos_emb"][c["row_pos"]].astype(np.float64)
        return x, U32 * np.abs(x)
    X = c["X"].reshape(-1, c["ldx"])[:M, :K].astype(np.float64)
    if c["xs"] == X_PLAIN:
        return X, np.zeros_like(X)
    s0, s1 = _slabs(c)
    x = X + s0 + (0 if wrong == "slab_missing" else s1) + (s0 if wrong == "slab_twice" else 0)
    return x, 2 * U32 * (np.abs(X) + np.abs(s0) + np.abs(s1))


def gv_rows(c, wrong=None):
    """(h float64 [M][K] unrounded, bh: bound of |kernel fp16 row - h|). wrong: the slab wrongs of gv_xrows, "ln_without_slabs"
    (statistics over X alone, applied to X + slabs), "drop_split" (split 3 left out of the combine)"""
    M, K = c["M"], c["K"]
    if c["inm"] == IN_F16:
        h = c["Xh"].reshape(-1, c["ldxh"])[:M, :K].astype(np.float64)
        return h, np.zeros_like(h)
    if c["inm"] == IN_LN:
        x, dx = gv_xrows(c, wrong)
        g, b = c["gamma"].astype(np.float64), c["beta"].astype(np.float64)
        if wrong == "ln_without_slabs":
            X = c["X"].reshape(-1, c["ldx"])[:M, :K].astype(np.float64)
            mean = X.mean(-1, keepdims=True)
            var = ((X - mean) ** 2).mean(-1, keepdims=True)
            return (x - mean) / np.sqrt(var + R.LN_EPS) * g + b, None
        y = ln_ref(x, g, b)
        e32, _ = ln_bound(x, g, b)
        mean = x.mean(-1, keepdims=True)
        r = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + R.LN_EPS)
        dxm = dx.max(-1, keepdims=True)
        e32 = e32 + SLACK * np.abs(g) * r * dxm * (2 + 2 * np.abs(x - mean) * r)
        return y, to16(y, e32)
    Rq, H = c["Rq"], c["H"]
    m_idx = np.arange(M)
    grp, qi = m_idx // Rq, m_idx % Rq
    po = c["part_o"].astype(np.float64)[grp, :, :, qi, :]                   # [M][H][8][64]
    ml = c["part_ml"].astype(np.float64)[grp, :, qi, :, :]                  # [M][H][8][2]
    mm, ll = ml[..., 0], ml[..., 1]
    w = np.exp(mm - mm.max(-1, keepdims=True)) * ll
    if wrong == "drop_split":
        w[..., 3] = 0.0
    f = w / w.sum(-1, keepdims=True)
    h = np.einsum("mhs,mhsd->mhd", f, po)
    Rm = np.minimum(mm.max(-1) - mm.min(-1), 104.0)
    ew = (4 * (Rm + 1) + 2) * U32
    e32 = SLACK * (2 * ew + 20 * U32)[..., None] * np.einsum("mhs,mhsd->mhd", f, np.abs(po))
    h, e32 = h.reshape(M, K), e32.reshape(M, K)
    return h, to16(h, e32)


def gv_logical(c, wrong=None):
    """{destination: (float64 values, bound)} of one launch: "Yh" [M][N or d], "Y" [M][N], "Xres" [M][N], "K" / "V" [M][d], "slab"
    [KS][M][N], "X" [M][K] and "intok" [M] (EMBED). wrong (the answers of a broken kernel; bounds are the right answer's): the
    wrongs of gv_rows, "drop_ktile" (one k-tile of one wave left out of every sum: the last 32 columns of K, of the first K slice under OUT_SLAB), "bias_both" (OUT_SLAB:
    both slices add the bias), "qscale_on_k", "ragged_clamped" (the last N % 16 columns of the vocabulary taken from the tile
    before: the clamped pair), "resid_slab_missing" / "resid_slab_twice" (XS SLABS under OUT_RESID)."""
    M, K, N, out = c["M"], c["K"], c["N"], c["out"]
    h, bh = gv_rows(c, wrong if wrong in ("slab_missing", "slab_twice", "ln_without_slabs", "drop_split") and c["inm"] != IN_F16 else None)
    if bh is None:
        bh = np.zeros_like(h)
    w = gv_w16(c)
    aw = np.abs(w)
    res = {}

    def acc_of(k0, k1):
        hh, ww = h[:, k0:k1], w[:, k0:k1]
        if wrong == "drop_ktile" and k0 == 0:
            hh = hh.copy()
            hh[:, k1 - 32:] = 0.0
        acc = hh @ ww.T
        e = bh[:, k0:k1] @ aw[:, k0:k1].T + acc_bound((np.abs(h[:, k0:k1]) + bh[:, k0:k1]) @ aw[:, k0:k1].T, k1 - k0)
        return acc, e

    bias = np.zeros(N) if c["bias"] is None else c["bias"].astype(np.float64)
    if out == OUT_SLAB:
        vals, bnds = [], []
        for s_ in range(KS):
            acc, e = acc_of(s_ * K // KS, (s_ + 1) * K // KS)
            o = acc + (bias if (s_ == 0 or wrong == "bias_both") else 0.0)
            vals.append(o)
            bnds.append(SLACK * (e + U32 * (np.abs(o) + e)) + 1e-30)
        res["slab"] = (np.stack(vals), np.stack(bnds))
        return res
    acc, e = acc_of(0, K)
    o = acc + bias
    eo = e if c["bias"] is None else e + U32 * (np.abs(o) + e)
    if out == OUT_F32:
        if wrong == "ragged_clamped" and N % 16:
            n0 = N // 16 * 16
            o = o.copy()
            o[:, n0:] = o[:, n0 - 16:n0 - 16 + N % 16]
        res["Y"] = (o, SLACK * eo + 1e-30)
    elif out in (OUT_F16, OUT_GELU):
        if out == OUT_GELU:
            g = R.gelu64(o)
            eo = 1.13 * eo + 0.5 * np.abs(o) * R.E_ERF + 4 * U32 * (np.abs(g) + np.abs(o))
            o = g
        y = o * c["qscale"]
        res["Yh"] = (y, to16(y, SLACK * (c["qscale"] * eo + U32 * np.abs(y))))
    elif out == OUT_RESID:
        x0 = c["Xres"].reshape(-1, c["ldxres"])[:M, :N].astype(np.float64)
        r, er = x0, 0.0
        if c["xs"] == X_SLABS:
            s0, s1 = _slabs(c)
            r = x0 + s0 + (0 if wrong == "resid_slab_missing" else s1) + (s0 if wrong == "resid_slab_twice" else 0)
            er = 2 * U32 * (np.abs(x0) + np.abs(s0) + np.abs(s1))
        y = r + o
        res["Xres"] = (y, SLACK * (eo + er + U32 * np.abs(y)) + 1e-30)
    else:
        d = c["d"]
        q = o[:, :d] * c["qscale"]
        res["Yh"] = (q, to16(q, SLACK * (c["qscale"] * eo[:, :d] + U32 * np.abs(q))))
        kk = o[:, d:2 * d] * (c["qscale"] if wrong == "qscale_on_k" else 1.0)
        res["K"] = (kk, to16(o[:, d:2 * d], SLACK * eo[:, d:2 * d]))
        res["V"] = (o[:, 2 * d:], to16(o[:, 2 * d:], SLACK * eo[:, 2 * d:]))
        if c["xs"] == X_EMBED:
            x, dx = gv_xrows(c)
            res["X"] = (x, SLACK * dx + 1e-30)
            res["intok"] = (c["emb_token"].astype(np.float64), np.full(M, 0.5))
    return res


def gv_emulate32(c):
    """the launch in numpy float32 in another association: LayerNorm by ln_emulate32 on the fp32 row (slabs added last first), the
    combine over the splits reversed, the K sum reversed, every store rounded as the kernel rounds it"""
    M, K, N, out = c["M"], c["K"], c["N"], c["out"]
    f32 = np.float32
    if c["inm"] == IN_F16:
        h = c["Xh"].reshape(-1, c["ldxh"])[:M, :K].astype(f32)
    elif c["inm"] == IN_LN:
        if c["xs"] == X_EMBED:
            x = c["pos_emb"][c["row_pos"]] + c["tok_emb"][c["emb_token"]].astype(f32)
        else:
            x = c["X"].reshape(-1, c["ldx"])[:M, :K]
            if c["xs"] == X_SLABS:
                s0, s1 = (s.astype(f32) for s in _slabs(c))
                x = (s1 + s0) + x
        xrow = x.astype(f32)
        h = R.ln_emulate32(xrow, c["gamma"], c["beta"]).astype(np.float16).astype(f32)
    else:
        m_idx = np.arange(M)
        grp, qi = m_idx // c["Rq"], m_idx % c["Rq"]
        po = c["part_o"].astype(f32)[grp, :, :, qi, :][:, :, ::-1]
        ml = c["part_ml"][grp, :, qi, :, :][:, :, ::-1]
        w = (np.exp(ml[..., 0] - ml[..., 0].max(-1, keepdims=True)) * ml[..., 1]).astype(f32)
        h = (np.einsum("mhs,mhsd->mhd", w, po) / w.sum(-1, dtype=f32)[..., None]).astype(np.float16).astype(f32).reshape(M, K)
    w16 = c["W"].astype(np.float16).astype(f32)
    bias = np.zeros(N, f32) if c["bias"] is None else c["bias"]
    res = {}
    if out == OUT_SLAB:
        res["slab"] = np.stack([(h[:, s_ * K // KS:(s_ + 1) * K // KS][:, ::-1] @ w16[:, s_ * K // KS:(s_ + 1) * K // KS][:, ::-1].T).astype(f32)
                                + (bias if s_ == 0 else f32(0)) for s_ in range(KS)])
        return res
    o = ((h[:, ::-1] @ w16[:, ::-1].T).astype(f32) + bias).astype(f32)
    if out == OUT_F32:
        res["Y"] = o
    elif out == OUT_F16:
        res["Yh"] = (o * f32(c["qscale"])).astype(np.float16)
    elif out == OUT_GELU:
        res["Yh"] = R.gelu64(o.astype(np.float64)).astype(f32).astype(np.float16)
    elif out == OUT_RESID:
        r = c["Xres"].reshape(-1, c["ldxres"])[:M, :N]
        if c["xs"] == X_SLABS:
            s0, s1 = (s.astype(f32) for s in _slabs(c))
            r = (s1 + s0) + r
        res["Xres"] = (o + r).astype(f32)
    else:
        d = c["d"]
        res["Yh"] = (o[:, :d] * f32(c["qscale"])).astype(np.float16)
        res["K"], res["V"] = o[:, d:2 * d].astype(np.float16), o[:, 2 * d:].astype(np.float16)
        if c["xs"] == X_EMBED:
            res["X"], res["intok"] = xrow, c["emb_token"].copy()
    return res


# ------------------------------------------------------------------ where the values lie
_ARRAY_OF = {"Yh": "Yh", "Y": "Y", "Xres": "Xres", "K": "Kc", "V": "Vc", "slab": "slab", "X": "X", "intok": "intok"}
OUT_ARRAYS = ("Yh", "Y", "Xres", "Kc", "Vc", "slab", "X", "intok")


def gv_index(c, pos_shift=0, row_shift=0):
    """{destination: flat indices into its array, shaped like its logical values}: the documented layouts. pos_shift / row_shift
    give the places a broken kernel would use (K / V one position on; row M - 1 stored once more in row M's slot — see gv_place)."""
    M, N = c["M"], c["N"]
    m = (np.arange(M) + row_shift)[:, None]
    idx = {}
    out = c["out"]
    if out in (OUT_F16, OUT_GELU):
        idx["Yh"] = m * c["ldyh"] + np.arange(N)[None]
    elif out == OUT_F32:
        idx["Y"] = m * c["ldy"] + np.arange(N)[None]
    elif out == OUT_RESID:
        idx["Xres"] = m * c["ldxres"] + np.arange(N)[None]
    elif out == OUT_SLAB:
        idx["slab"] = (np.arange(KS) * c["slab_stride"])[:, None, None] + (m * c["ldxres"] + np.arange(N)[None])[None]
    else:
        d = c["d"]
        idx["Yh"] = m * c["ldyh"] + np.arange(d)[None]
        kv = (c["row_cache"].astype(np.int64) * c["crs"] + (c["row_pos"].astype(np.int64) + pos_shift) * d)[:, None] + np.arange(d)[None]
        idx["K"], idx["V"] = kv, kv
        if c["xs"] == X_EMBED:
            idx["X"] = m * c["ldx"] + np.arange(c["K"])[None]
            idx["intok"] = c["row_cache"].astype(np.int64) * T_TEXT + c["row_pos"]
    return idx


def gv_arrays(c):
    """fresh copies of the in / out arrays of the case the hook copies in and out"""
    return {n: c[n].copy() for n in OUT_ARRAYS if n in c}


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def gv_check(c, got, ref=None):
    """(worst excess over every element some thread owns, per-destination excess dict, True when every other byte of every in / out
    array kept its bits)"""
    ref = ref or gv_logical(c)
    idx = gv_index(c)
    per, clean = {}, True
    owned = {n: np.zeros(a.shape, bool) for n, a in got.items()}
    for name, (val, bound) in ref.items():
        arr = _ARRAY_OF[name]
        v = got[arr][idx[name]]
        owned[arr][idx[name]] = True
        per[name] = excess(v, val, bound)
    for n, a in got.items():
        clean = clean and bool((_bits(a)[~owned[n]] == _bits(c[n])[~owned[n]]).all())
    return max(per.values()), per, clean


def gv_place(c, vals, pos_shift=0, dup_last_row=False):
    """the arrays a kernel leaves that stores `vals` (destination -> values, rounded to the array's type here) through the documented
    layout — or through a broken one: K / V at row_pos + pos_shift; dup_last_row: row M - 1 written once more into row M's slot"""
    got = gv_arrays(c)
    idx = gv_index(c, pos_shift=pos_shift)
    for name, v in vals.items():
        arr = got[_ARRAY_OF[name]]
        ix = idx[name] if name in ("K", "V") else gv_index(c)[name]
        arr[ix] = np.asarray(v).astype(arr.dtype)
        if dup_last_row and name not in ("K", "V", "intok"):
            one = gv_index(c, row_shift=1)[name]
            last = (slice(None), -1) if name == "slab" else (-1,)
            arr[one[last]] = np.asarray(v)[last].astype(arr.dtype)
    return got


def gv_wrongs(c):
    """the wrong answers that exist for the case, by name: value wrongs (gv_logical) and placement wrongs (gv_place)"""
    w = ["drop_ktile", "dup_last_row"]
    if c["xs"] == X_SLABS and c["inm"] == IN_LN:
        w += ["slab_missing", "slab_twice", "ln_without_slabs"]
    if c["xs"] == X_SLABS and c["out"] == OUT_RESID:
        w += ["resid_slab_missing", "resid_slab_twice"]
    if c["out"] == OUT_SLAB:
        w += ["bias_both", "slab_swapped"]
    if c["out"] == OUT_QKV:
        w += ["qscale_on_k", "kv_pos_plus1"]
    if c["out"] == OUT_F32 and c["N"] % 16:
        w.append("ragged_clamped")
    if c["inm"] == IN_XATTN:
        w.append("drop_split")
    return w


def gv_wrong_arrays(c, wrong):
    """the arrays a kernel broken in the named way leaves (values rounded as the right kernel rounds them)"""
    if wrong == "dup_last_row":
        return gv_place(c, {n: v for n, (v, _) in gv_logical(c).items()}, dup_last_row=True)
    if wrong == "kv_pos_plus1":
        return gv_place(c, {n: v for n, (v, _) in gv_logical(c).items()}, pos_shift=1)
    if wrong == "slab_swapped":
        return gv_place(c, {"slab": gv_logical(c)["slab"][0][::-1]})
    return gv_place(c, {n: v for n, (v, _) in gv_logical(c, wrong).items()})


# ------------------------------------------------------------------ the hook
def run_gemv(c, device=0, arrays=None, **over):
    """-> (rc, dict of the copied-back in / out arrays, kernel name) of one wlx_debug_dec_gemv call; `over` replaces arguments of the
    argument struct or, by array name, an input array (refusal tests); `arrays` replaces the in / out arrays (chained launches)"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    got = arrays if arrays is not None else gv_arrays(c)
    a = _lib.wlx_debug_dec_gemv_args()
    ln = lambda n: len(got[n]) if n in got else (c[n].size if n in c and c[n] is not None else 0)
    vals = dict(in_mode=c["inm"], out_mode=c["out"], xsrc=c["xs"], M=c["M"], K=c["K"], KT=c["KT"], N=c["N"], busy_device=c["busy"],
                KTS=c["KTS"], H=c["H"], R=c["Rq"], d=c.get("d", 0), qscale=c["qscale"],
                ldx=c.get("ldx", 0), ldxh=c.get("ldxh", 0), ldyh=c.get("ldyh", 0), ldy=c.get("ldy", 0), ldxres=c.get("ldxres", 0),
                cache_row_stride=c.get("crs", 0), slab_stride=c.get("slab_stride", 0),
                x_len=ln("X"), xh_len=ln("Xh"), part_o_len=ln("part_o"), part_ml_len=ln("part_ml"), slab_len=ln("slab"),
                tok_emb_len=ln("tok_emb"), pos_emb_len=ln("pos_emb"), yh_len=ln("Yh"), y_len=ln("Y"), xres_len=ln("Xres"),
                kc_len=ln("Kc"), vc_len=ln("Vc"), intok_len=ln("intok"))
    ins = {n: c.get(n) for n in ("W", "bias", "gamma", "beta", "Xh", "part_o", "part_ml", "tok_emb", "pos_emb", "emb_token", "row_pos", "row_cache")}
    for k, v in over.items():
        if k in vals:
            vals[k] = v
        else:
            ins[k] = v
    for k, v in vals.items():
        setattr(a, k, v)
    f = lambda n: _ptr(None if ins[n] is None else np.ascontiguousarray(ins[n], np.float32), C.c_float)
    h = lambda x: None if x is None else _ptr(np.ascontiguousarray(x).view(np.uint16), C.c_uint16)
    i = lambda x: None if x is None else _ptr(np.ascontiguousarray(x, np.int32), C.c_int32)
    keep = [np.ascontiguousarray(ins[n]) if ins[n] is not None else None for n in ins]        # (alive across the call)
    name = C.create_string_buffer(NAME_CAP)
    W = np.ascontiguousarray(ins["W"], np.float32)
    rc = lib.wlx_debug_dec_gemv(device, C.byref(a), _ptr(W, C.c_float), f("bias"), f("gamma"), f("beta"), _ptr(got.get("X"), C.c_float),
                                h(ins["Xh"]), h(ins["part_o"]), f("part_ml"), _ptr(got.get("slab"), C.c_float), h(ins["tok_emb"]),
                                f("pos_emb"), i(ins["emb_token"]), i(ins["row_pos"]), i(ins["row_cache"]), h(got.get("Yh")),
                                _ptr(got.get("Y"), C.c_float), _ptr(got.get("Xres"), C.c_float), h(got.get("Kc")), h(got.get("Vc")),
                                i(got.get("intok")), name, NAME_CAP)
    del keep
    return rc, got, name.value.decode()


# ------------------------------------------------------------------ fused LayerNorm + query projection + cross-attention partials
CQ_D, CQ_H = 768, 12
# (R, groups, rows): R 1 / 5 / 16, one and three groups, the last group short where R > 1
CQ_CASES = [(1, 1, 1), (1, 3, 3), (5, 1, 5), (5, 3, 13), (16, 1, 16), (16, 3, 39), (5, 1, 3)]


def cq_case(Rq, groups, rows, seed=0):
    """x float32 [rows][ldx], gamma / beta, Wq [768][768] = 0.25 N(0, 1) / sqrt(768) (queries of spread ~0.03 after the 1 / 8: scores
    of spread ~2 against N(0, 1) keys: every split holds a share of every row's mass), bias 0.3 N(0, 1); K / V, their packed
    images, the padded keys and group_item (out of order, with repeats) are xa_case's "uniform" case; partials prefilled +-1000"""
    c = R.xa_case(CQ_H, Rq, groups, rows, 3, "uniform", seed=seed + 11)
    rng = np.random.default_rng(seed * 7919 + Rq * 131 + groups * 17 + rows)
    proj = gv_case(spec(IN_LN, OUT_F16, X_PLAIN, rows, CQ_D, CQ_D, G2 % "6, 3, 0, 0, 1, 1, 0"), seed=seed + 5)
    proj["W"] = (0.25 * rng.standard_normal((CQ_D, CQ_D)) / np.sqrt(CQ_D)).astype(np.float32)
    proj["bias"] = (0.3 * rng.standard_normal(CQ_D)).astype(np.float32)
    c["proj"] = proj
    return c


def cq_ref(c, dead_last=True, **wrong):
    """xa_ref on the float64 query of the projection's reference with its fp16 bound (gv_logical "Yh")"""
    q, qb = gv_logical(c["proj"])["Yh"]
    return R.xa_ref(c, q=q, qb=qb, dead_last=dead_last, **wrong), (q, qb)


def cq_live(c):
    """mask [groups][16] of the query lanes that hold a row of their own"""
    g = np.arange(c["groups"])[:, None] * c["R"] + np.arange(16)[None]
    return (np.arange(16)[None] < c["R"]) & (g < c["rows"])


def run_cq(c, device=0, **over):
    """-> (rc, dict part_o / part_m / part_l / part_ml) of one wlx_debug_dec_cq_cross_attn call"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    p = c["proj"]
    a = dict(ldx=p["ldx"], qscale=p["qscale"], d=CQ_D, item_stride=c["item_stride"], n_items=c["n_items"], H=c["H"], R=c["R"],
             groups=c["groups"], rows=c["rows"])
    a.update({k: v for k, v in over.items() if k in a})
    gi = np.ascontiguousarray(over.get("group_item", c["group_item"]), np.int32)
    x, g, b, W, bias = (np.ascontiguousarray(p[n], np.float32) for n in ("X", "gamma", "beta", "W", "bias"))
    kp, vp = np.ascontiguousarray(c["kp"]), np.ascontiguousarray(c["vp"])
    po, ml = c["part_o"].copy(), c["part_ml"].copy()
    u16 = lambda z: _ptr(z.view(np.uint16), C.c_uint16)
    rc = lib.wlx_debug_dec_cq_cross_attn(device, _ptr(x, C.c_float), a["ldx"], _ptr(g, C.c_float), _ptr(b, C.c_float), _ptr(W, C.c_float),
                                         _ptr(bias, C.c_float), a["qscale"], a["d"], u16(kp), u16(vp), a["item_stride"], a["n_items"],
                                         a["H"], a["R"], a["groups"], a["rows"], _ptr(gi, C.c_int32), u16(po), _ptr(ml, C.c_float))
    return rc, dict(part_o=po, part_m=ml[..., 0], part_l=ml[..., 1], part_ml=ml)


# ------------------------------------------------------------------ the case list (literal)
# (in, out, xs, M, K, N, busy_device, d of a QKV launch, R of the split combine, template arguments of the kernel that runs)
_ROWS = [
    (0, 4, 0, 1, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 0"),
    (0, 4, 0, 5, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 0"),
    (0, 4, 0, 16, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 0"),
    (0, 4, 0, 17, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 0"),
    (0, 4, 1, 1, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 1"),
    (0, 4, 1, 5, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 1"),
    (0, 4, 1, 8, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 1"),
    (0, 4, 1, 9, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 1"),
    (0, 4, 1, 16, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 1"),
    (0, 4, 2, 1, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 5, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 8, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 9, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 16, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 17, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 33, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (0, 4, 2, 64, 384, 96, 0, 32, 5, "2, 15, 0, 4, 1, 1, 2"),
    (1, 3, 0, 1, 384, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 5, 384, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 384, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 384, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 33, 384, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 64, 384, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 65, 384, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 1, 5, 384, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 1"),
    (1, 3, 1, 16, 384, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 1"),
    (1, 3, 0, 5, 1536, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 1536, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 1536, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 60, 1536, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (0, 0, 0, 1, 384, 64, 0, 0, 5, "2, 15, 0, 0, 1, 1, 0"),
    (0, 0, 0, 5, 384, 64, 0, 0, 5, "2, 15, 0, 0, 1, 1, 0"),
    (0, 0, 0, 16, 384, 64, 0, 0, 5, "2, 15, 0, 0, 1, 1, 0"),
    (0, 0, 0, 17, 384, 64, 0, 0, 5, "2, 15, 0, 0, 1, 1, 0"),
    (2, 3, 0, 3, 384, 64, 0, 0, 1, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 5, 384, 64, 0, 0, 5, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 13, 384, 64, 0, 0, 5, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 16, 384, 64, 0, 0, 16, "6, 1, 2, 3, 1, 1, 0"),
    (0, 1, 0, 1, 384, 128, 0, 0, 5, "2, 15, 0, 1, 1, 1, 0"),
    (0, 1, 0, 5, 384, 128, 0, 0, 5, "2, 15, 0, 1, 1, 1, 0"),
    (0, 1, 0, 16, 384, 128, 0, 0, 5, "2, 15, 0, 1, 1, 1, 0"),
    (0, 1, 0, 17, 384, 2048, 0, 0, 5, "2, 15, 0, 1, 4, 1, 0"),
    (0, 1, 0, 60, 384, 2048, 0, 0, 5, "2, 15, 0, 1, 4, 1, 0"),
    (1, 5, 0, 1, 1536, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 5, 1536, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 16, 1536, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 17, 1536, 64, 0, 0, 5, "6, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 60, 1536, 64, 0, 0, 5, "6, 1, 1, 5, 1, 1, 0"),
    (0, 4, 0, 1, 512, 96, 0, 32, 5, "4, 2, 0, 4, 1, 1, 0"),
    (0, 4, 0, 5, 512, 96, 0, 32, 5, "4, 2, 0, 4, 1, 1, 0"),
    (0, 4, 0, 16, 512, 96, 0, 32, 5, "4, 2, 0, 4, 1, 1, 0"),
    (0, 4, 0, 17, 512, 96, 0, 32, 5, "4, 2, 0, 4, 1, 1, 0"),
    (0, 4, 1, 5, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 1"),
    (0, 4, 1, 8, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 1"),
    (0, 4, 1, 9, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 1"),
    (0, 4, 1, 16, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 1"),
    (0, 4, 2, 5, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 8, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 9, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 16, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 17, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 33, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (0, 4, 2, 64, 512, 96, 0, 32, 5, "2, 2, 0, 4, 1, 1, 2"),
    (1, 3, 0, 1, 512, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 5, 512, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 512, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 512, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 33, 512, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 64, 512, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 65, 512, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 1, 5, 512, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 1"),
    (1, 3, 1, 16, 512, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 1"),
    (1, 3, 0, 5, 2048, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 2048, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 2048, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 60, 2048, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (0, 0, 0, 1, 512, 64, 0, 0, 5, "4, 2, 0, 0, 1, 1, 0"),
    (0, 0, 0, 5, 512, 64, 0, 0, 5, "4, 2, 0, 0, 1, 1, 0"),
    (0, 0, 0, 16, 512, 64, 0, 0, 5, "4, 2, 0, 0, 1, 1, 0"),
    (0, 0, 0, 17, 512, 64, 0, 0, 5, "4, 2, 0, 0, 1, 1, 0"),
    (2, 3, 0, 3, 512, 64, 0, 0, 1, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 5, 512, 64, 0, 0, 5, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 13, 512, 64, 0, 0, 5, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 16, 512, 64, 0, 0, 16, "4, 1, 2, 3, 1, 1, 0"),
    (0, 1, 0, 1, 512, 128, 0, 0, 5, "4, 2, 0, 1, 1, 1, 0"),
    (0, 1, 0, 5, 512, 128, 0, 0, 5, "4, 2, 0, 1, 1, 1, 0"),
    (0, 1, 0, 16, 512, 128, 0, 0, 5, "4, 2, 0, 1, 1, 1, 0"),
    (0, 1, 0, 17, 512, 2048, 0, 0, 5, "4, 2, 0, 1, 4, 1, 0"),
    (0, 1, 0, 60, 512, 2048, 0, 0, 5, "4, 2, 0, 1, 4, 1, 0"),
    (1, 5, 0, 1, 2048, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 5, 2048, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 16, 2048, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 17, 2048, 64, 0, 0, 5, "4, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 60, 2048, 64, 0, 0, 5, "4, 1, 1, 5, 1, 1, 0"),
    (0, 4, 0, 1, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 0, 5, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 0, 16, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 0, 17, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 1, 1, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 1"),
    (0, 4, 1, 5, 768, 96, 0, 32, 5, "4, 3, 0, 4, 1, 1, 1"),
    (0, 4, 1, 8, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 1"),
    (0, 4, 1, 9, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 1"),
    (0, 4, 1, 16, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 1"),
    (0, 4, 2, 1, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 5, 768, 96, 0, 32, 5, "4, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 8, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 9, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 16, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 17, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 33, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 2, 64, 768, 96, 0, 32, 5, "3, 3, 0, 4, 1, 1, 2"),
    (0, 4, 0, 17, 768, 2112, 0, 704, 5, "6, 3, 0, 4, 4, 1, 0"),
    (0, 4, 0, 33, 768, 2112, 0, 704, 5, "6, 3, 0, 4, 4, 1, 0"),
    (0, 4, 0, 60, 768, 2112, 0, 704, 5, "6, 3, 0, 4, 4, 1, 0"),
    (0, 4, 0, 320, 768, 2112, 0, 704, 5, "6, 3, 0, 4, 4, 1, 0"),
    (1, 3, 0, 1, 768, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 5, 768, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 768, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 768, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 33, 768, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 64, 768, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 65, 768, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 1, 5, 768, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 1"),
    (1, 3, 1, 16, 768, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 1"),
    (1, 3, 0, 5, 3072, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 3072, 64, 0, 0, 5, "12, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 3072, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 60, 3072, 64, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (0, 0, 0, 1, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (0, 0, 0, 5, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (0, 0, 0, 16, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (0, 0, 0, 17, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (0, 0, 0, 60, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (0, 0, 0, 320, 768, 64, 0, 0, 5, "6, 3, 0, 0, 1, 1, 0"),
    (2, 3, 0, 3, 768, 64, 0, 0, 1, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 5, 768, 64, 0, 0, 5, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 13, 768, 64, 0, 0, 5, "6, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 16, 768, 64, 0, 0, 16, "6, 1, 2, 3, 1, 1, 0"),
    (0, 1, 0, 1, 768, 128, 0, 0, 5, "6, 3, 0, 1, 1, 1, 0"),
    (0, 1, 0, 5, 768, 128, 0, 0, 5, "6, 3, 0, 1, 1, 1, 0"),
    (0, 1, 0, 16, 768, 128, 0, 0, 5, "6, 3, 0, 1, 1, 1, 0"),
    (0, 1, 0, 17, 768, 2048, 0, 0, 5, "6, 3, 0, 1, 4, 1, 0"),
    (0, 1, 0, 60, 768, 2048, 0, 0, 5, "6, 3, 0, 1, 4, 1, 0"),
    (1, 5, 0, 1, 3072, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 5, 3072, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 16, 3072, 64, 0, 0, 5, "12, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 17, 3072, 64, 0, 0, 5, "6, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 60, 3072, 64, 0, 0, 5, "6, 1, 1, 5, 1, 1, 0"),
    (0, 4, 0, 1, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 0"),
    (0, 4, 0, 5, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 0"),
    (0, 4, 0, 16, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 0"),
    (0, 4, 0, 17, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 0"),
    (0, 4, 0, 8, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 0"),
    (0, 4, 0, 9, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 0"),
    (0, 4, 1, 1, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 1"),
    (0, 4, 1, 5, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 1"),
    (0, 4, 1, 8, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 1"),
    (0, 4, 1, 9, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 1"),
    (0, 4, 1, 16, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 1"),
    (0, 4, 2, 1, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 5, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 8, 1024, 96, 0, 32, 5, "8, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 9, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 16, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 17, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 33, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 2"),
    (0, 4, 2, 64, 1024, 96, 0, 32, 5, "4, 4, 0, 4, 1, 1, 2"),
    (0, 4, 0, 17, 1024, 2112, 0, 704, 5, "4, 4, 0, 4, 4, 1, 0"),
    (0, 4, 0, 33, 1024, 2112, 0, 704, 5, "4, 4, 0, 4, 4, 1, 0"),
    (0, 4, 0, 60, 1024, 2112, 0, 704, 5, "4, 4, 0, 4, 4, 1, 0"),
    (1, 3, 0, 1, 1024, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 5, 1024, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 1024, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 1024, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 33, 1024, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 64, 1024, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 65, 1024, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 1, 5, 1024, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 1"),
    (1, 3, 1, 16, 1024, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 1"),
    (1, 3, 0, 5, 4096, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 4096, 64, 0, 0, 5, "8, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 4096, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 60, 4096, 64, 0, 0, 5, "4, 1, 1, 3, 1, 1, 0"),
    (0, 0, 0, 1, 1024, 64, 0, 0, 5, "8, 4, 0, 0, 1, 1, 0"),
    (0, 0, 0, 5, 1024, 64, 0, 0, 5, "8, 4, 0, 0, 1, 1, 0"),
    (0, 0, 0, 16, 1024, 64, 0, 0, 5, "4, 4, 0, 0, 1, 1, 0"),
    (0, 0, 0, 17, 1024, 64, 0, 0, 5, "4, 4, 0, 0, 1, 1, 0"),
    (0, 0, 0, 8, 1024, 64, 0, 0, 5, "8, 4, 0, 0, 1, 1, 0"),
    (0, 0, 0, 9, 1024, 64, 0, 0, 5, "4, 4, 0, 0, 1, 1, 0"),
    (2, 3, 0, 3, 1024, 64, 0, 0, 1, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 5, 1024, 64, 0, 0, 5, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 13, 1024, 64, 0, 0, 5, "4, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 16, 1024, 64, 0, 0, 16, "4, 1, 2, 3, 1, 1, 0"),
    (0, 1, 0, 1, 1024, 128, 0, 0, 5, "8, 4, 0, 1, 1, 1, 0"),
    (0, 1, 0, 5, 1024, 128, 0, 0, 5, "8, 4, 0, 1, 1, 1, 0"),
    (0, 1, 0, 16, 1024, 128, 0, 0, 5, "4, 4, 0, 1, 1, 1, 0"),
    (0, 1, 0, 8, 1024, 128, 0, 0, 5, "8, 4, 0, 1, 1, 1, 0"),
    (0, 1, 0, 9, 1024, 128, 0, 0, 5, "4, 4, 0, 1, 1, 1, 0"),
    (0, 1, 0, 17, 1024, 2048, 0, 0, 5, "4, 4, 0, 1, 4, 1, 0"),
    (0, 1, 0, 60, 1024, 2048, 0, 0, 5, "4, 4, 0, 1, 4, 1, 0"),
    (1, 5, 0, 1, 4096, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 5, 4096, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 16, 4096, 64, 0, 0, 5, "8, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 17, 4096, 64, 0, 0, 5, "4, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 60, 4096, 64, 0, 0, 5, "4, 1, 1, 5, 1, 1, 0"),
    (0, 4, 0, 1, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 0"),
    (0, 4, 0, 5, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 0"),
    (0, 4, 0, 16, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 0"),
    (0, 4, 0, 17, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 0"),
    (0, 4, 0, 8, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 0"),
    (0, 4, 0, 9, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 0"),
    (0, 4, 1, 1, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 1"),
    (0, 4, 1, 5, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 1"),
    (0, 4, 1, 8, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 1"),
    (0, 4, 1, 9, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 1"),
    (0, 4, 1, 16, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 1"),
    (0, 4, 2, 1, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 5, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 8, 1280, 96, 0, 32, 5, "10, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 9, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 16, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 17, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 33, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 2"),
    (0, 4, 2, 64, 1280, 96, 0, 32, 5, "5, 5, 0, 4, 1, 1, 2"),
    (0, 4, 0, 17, 1280, 2112, 0, 704, 5, "5, 5, 0, 4, 4, 1, 0"),
    (0, 4, 0, 33, 1280, 2112, 0, 704, 5, "5, 5, 0, 4, 4, 1, 0"),
    (0, 4, 0, 60, 1280, 2112, 0, 704, 5, "5, 5, 0, 4, 4, 1, 0"),
    (1, 3, 0, 1, 1280, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 5, 1280, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 1280, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 1280, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 33, 1280, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 64, 1280, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 65, 1280, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (1, 3, 1, 5, 1280, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 1"),
    (1, 3, 1, 16, 1280, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 1"),
    (1, 3, 0, 5, 5120, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 16, 5120, 64, 0, 0, 5, "10, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 17, 5120, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 60, 5120, 64, 0, 0, 5, "5, 1, 1, 3, 1, 1, 0"),
    (0, 0, 0, 1, 1280, 64, 0, 0, 5, "10, 5, 0, 0, 1, 1, 0"),
    (0, 0, 0, 5, 1280, 64, 0, 0, 5, "10, 5, 0, 0, 1, 1, 0"),
    (0, 0, 0, 16, 1280, 64, 0, 0, 5, "5, 5, 0, 0, 1, 1, 0"),
    (0, 0, 0, 17, 1280, 64, 0, 0, 5, "5, 5, 0, 0, 1, 1, 0"),
    (0, 0, 0, 8, 1280, 64, 0, 0, 5, "10, 5, 0, 0, 1, 1, 0"),
    (0, 0, 0, 9, 1280, 64, 0, 0, 5, "5, 5, 0, 0, 1, 1, 0"),
    (2, 3, 0, 3, 1280, 64, 0, 0, 1, "5, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 5, 1280, 64, 0, 0, 5, "5, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 13, 1280, 64, 0, 0, 5, "5, 1, 2, 3, 1, 1, 0"),
    (2, 3, 0, 16, 1280, 64, 0, 0, 16, "5, 1, 2, 3, 1, 1, 0"),
    (0, 1, 0, 1, 1280, 128, 0, 0, 5, "10, 5, 0, 1, 1, 1, 0"),
    (0, 1, 0, 5, 1280, 128, 0, 0, 5, "10, 5, 0, 1, 1, 1, 0"),
    (0, 1, 0, 16, 1280, 128, 0, 0, 5, "5, 5, 0, 1, 1, 1, 0"),
    (0, 1, 0, 8, 1280, 128, 0, 0, 5, "10, 5, 0, 1, 1, 1, 0"),
    (0, 1, 0, 9, 1280, 128, 0, 0, 5, "5, 5, 0, 1, 1, 1, 0"),
    (0, 1, 0, 17, 1280, 2048, 0, 0, 5, "5, 5, 0, 1, 4, 1, 0"),
    (0, 1, 0, 60, 1280, 2048, 0, 0, 5, "5, 5, 0, 1, 4, 1, 0"),
    (1, 5, 0, 1, 5120, 64, 0, 0, 5, "10, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 5, 5120, 64, 0, 0, 5, "10, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 16, 5120, 64, 0, 0, 5, "10, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 17, 5120, 64, 0, 0, 5, "5, 1, 1, 5, 1, 1, 0"),
    (1, 5, 0, 60, 5120, 64, 0, 0, 5, "5, 1, 1, 5, 1, 1, 0"),
    (0, 1, 0, 320, 768, 2048, 0, 0, 5, "6, 3, 0, 1, 4, 1, 0"),
    (0, 4, 0, 49, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 0, 65, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 4, 0, 48, 768, 96, 0, 32, 5, "6, 3, 0, 4, 1, 1, 0"),
    (0, 1, 0, 5, 1280, 5120, 0, 0, 5, "10, 5, 0, 1, 2, 1, 0"),
    (0, 1, 0, 9, 1280, 5120, 0, 0, 5, "5, 5, 0, 1, 2, 1, 0"),
    (0, 1, 0, 16, 1280, 5120, 0, 0, 5, "5, 5, 0, 1, 2, 1, 0"),
    (0, 1, 0, 17, 1280, 5120, 0, 0, 5, "5, 5, 0, 1, 2, 2, 0"),
    (0, 1, 0, 32, 1280, 5120, 0, 0, 5, "5, 5, 0, 1, 2, 2, 0"),
    (0, 1, 0, 48, 1280, 5120, 0, 0, 5, "5, 5, 0, 1, 4, 1, 0"),
    (0, 1, 0, 17, 1024, 3136, 0, 0, 5, "4, 4, 0, 1, 1, 2, 0"),
    (0, 1, 0, 32, 1024, 3136, 0, 0, 5, "4, 4, 0, 1, 1, 2, 0"),
    (0, 4, 0, 17, 1280, 2544, 0, 848, 5, "5, 5, 0, 4, 1, 2, 0"),
    (0, 4, 0, 32, 1280, 2544, 0, 848, 5, "5, 5, 0, 4, 1, 2, 0"),
    (1, 3, 0, 65, 768, 768, 0, 0, 5, "6, 1, 1, 3, 1, 1, 0"),
    (1, 3, 0, 120, 768, 768, 0, 0, 5, "6, 1, 1, 3, 1, 2, 0"),
    (1, 3, 0, 320, 768, 768, 0, 0, 5, "6, 1, 1, 3, 1, 2, 0"),
    (1, 3, 0, 120, 1280, 1280, 0, 0, 5, "5, 1, 1, 3, 1, 3, 0"),
    (1, 3, 0, 17, 768, 64, 1, 0, 5, "6, 1, 1, 3, 2, 1, 0"),
    (1, 3, 0, 60, 768, 64, 1, 0, 5, "6, 1, 1, 3, 2, 1, 0"),
    (1, 3, 0, 60, 1280, 64, 1, 0, 5, "5, 1, 1, 3, 2, 1, 0"),
    (0, 2, 0, 5, 384, 256, 0, 0, 5, "12, 3, 1"),
    (0, 2, 1, 5, 384, 256, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 1, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 5, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 16, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 17, 384, 265, 0, 0, 5, "12, 3, 2"),
    (0, 2, 0, 33, 384, 265, 0, 0, 5, "12, 3, 3"),
    (0, 2, 0, 49, 384, 265, 0, 0, 5, "12, 3, 4"),
    (0, 2, 0, 64, 384, 265, 0, 0, 5, "12, 3, 4"),
    (0, 2, 0, 65, 384, 265, 0, 0, 5, "12, 3, 4"),
    (0, 2, 0, 120, 384, 265, 0, 0, 5, "12, 3, 4"),
    (0, 2, 1, 1, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 1, 5, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 1, 16, 384, 265, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 5, 384, 288, 0, 0, 5, "12, 3, 1"),
    (0, 2, 1, 5, 384, 288, 0, 0, 5, "12, 3, 1"),
    (0, 2, 0, 5, 512, 256, 0, 0, 5, "16, 4, 1"),
    (0, 2, 1, 5, 512, 256, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 1, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 5, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 16, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 17, 512, 265, 0, 0, 5, "16, 4, 2"),
    (0, 2, 0, 33, 512, 265, 0, 0, 5, "16, 4, 3"),
    (0, 2, 0, 49, 512, 265, 0, 0, 5, "16, 4, 4"),
    (0, 2, 0, 64, 512, 265, 0, 0, 5, "16, 4, 4"),
    (0, 2, 0, 65, 512, 265, 0, 0, 5, "16, 4, 4"),
    (0, 2, 0, 120, 512, 265, 0, 0, 5, "16, 4, 4"),
    (0, 2, 1, 1, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 1, 5, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 1, 16, 512, 265, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 5, 512, 288, 0, 0, 5, "16, 4, 1"),
    (0, 2, 1, 5, 512, 288, 0, 0, 5, "16, 4, 1"),
    (0, 2, 0, 1, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 5, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 16, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 17, 768, 256, 0, 0, 5, "24, 6, 2"),
    (0, 2, 0, 33, 768, 256, 0, 0, 5, "24, 6, 3"),
    (0, 2, 0, 49, 768, 256, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 64, 768, 256, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 65, 768, 256, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 120, 768, 256, 0, 0, 5, "24, 6, 4"),
    (0, 2, 1, 1, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 5, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 16, 768, 256, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 1, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 5, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 16, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 17, 768, 265, 0, 0, 5, "24, 6, 2"),
    (0, 2, 0, 33, 768, 265, 0, 0, 5, "24, 6, 3"),
    (0, 2, 0, 49, 768, 265, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 64, 768, 265, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 65, 768, 265, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 120, 768, 265, 0, 0, 5, "24, 6, 4"),
    (0, 2, 1, 1, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 5, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 16, 768, 265, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 1, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 5, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 16, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 17, 768, 288, 0, 0, 5, "24, 6, 2"),
    (0, 2, 0, 33, 768, 288, 0, 0, 5, "24, 6, 3"),
    (0, 2, 0, 49, 768, 288, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 64, 768, 288, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 65, 768, 288, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 120, 768, 288, 0, 0, 5, "24, 6, 4"),
    (0, 2, 1, 1, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 5, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 1, 16, 768, 288, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 5, 1024, 256, 0, 0, 5, "32, 4, 1"),
    (0, 2, 1, 5, 1024, 256, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 1, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 5, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 16, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 17, 1024, 265, 0, 0, 5, "32, 4, 2"),
    (0, 2, 0, 33, 1024, 265, 0, 0, 5, "32, 4, 3"),
    (0, 2, 0, 49, 1024, 265, 0, 0, 5, "32, 4, 4"),
    (0, 2, 0, 64, 1024, 265, 0, 0, 5, "32, 4, 4"),
    (0, 2, 0, 65, 1024, 265, 0, 0, 5, "32, 4, 4"),
    (0, 2, 0, 120, 1024, 265, 0, 0, 5, "32, 4, 4"),
    (0, 2, 1, 1, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 1, 5, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 1, 16, 1024, 265, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 5, 1024, 288, 0, 0, 5, "32, 4, 1"),
    (0, 2, 1, 5, 1024, 288, 0, 0, 5, "32, 4, 1"),
    (0, 2, 0, 5, 1280, 256, 0, 0, 5, "40, 5, 1"),
    (0, 2, 1, 5, 1280, 256, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 1, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 5, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 16, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 17, 1280, 265, 0, 0, 5, "40, 5, 2"),
    (0, 2, 0, 33, 1280, 265, 0, 0, 5, "40, 5, 3"),
    (0, 2, 0, 49, 1280, 265, 0, 0, 5, "40, 5, 3"),
    (0, 2, 0, 64, 1280, 265, 0, 0, 5, "40, 5, 3"),
    (0, 2, 0, 65, 1280, 265, 0, 0, 5, "40, 5, 3"),
    (0, 2, 0, 120, 1280, 265, 0, 0, 5, "40, 5, 3"),
    (0, 2, 1, 1, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 1, 5, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 1, 16, 1280, 265, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 5, 1280, 288, 0, 0, 5, "40, 5, 1"),
    (0, 2, 1, 5, 1280, 288, 0, 0, 5, "40, 5, 1"),
    (0, 2, 0, 5, 768, 51865, 0, 0, 5, "24, 6, 1"),
    (0, 2, 0, 60, 768, 265, 0, 0, 5, "24, 6, 4"),
    (0, 2, 0, 320, 768, 265, 0, 0, 5, "24, 6, 4"),
]
CASES = [spec(i, o, x, M, K, N, (VOC if (o == OUT_F32) else G2) % a, busy=b, d=d, Rq=r) for i, o, x, M, K, N, b, d, r, a in _ROWS]
# what the hook refuses because no lean kernel serves it (d_model 512 with fewer than five slab / embedding rows has no instantiation)
NOT_LEAN = [spec(IN_LN, OUT_QKV, X_SLABS, 1, 512, 96, "", d=32), spec(IN_LN, OUT_QKV, X_EMBED, 1, 512, 96, "", d=32)]
# cases whose float64 reference is about a GFLOP: the host test runs one wrong answer on them, not all
def is_big(s):
    return s["M"] * s["K"] * s["N"] > 3e8

