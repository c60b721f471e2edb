"""float64 references of the Whisper kernels that the wlx_debug_layernorm / _attn_encoder / _dec_cross_attn / _dec_self_attn hooks
launch one at a time (csrc/gemm.hip layernorm_kernel, attention.hip, decoder.hip), their per-element error bounds, the nearest
plausible wrong answers the bounds must exclude, the case lists, and the hook runners. Inputs are the fp16-rounded (attention) or
fp32 (LayerNorm) values the kernels see; everything is computed in float64 with numpy. No figure observed on a GPU enters a bound:
every constant is derived in the docstring of the bound from the arithmetic the kernel performs. The bounds are first order in
the unit roundoffs. SLACK covers what that drops: with n roundings of relative size <= u each, prod (1 + d_i) - 1 is at most
n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1), i.e. the first-order figure n u times
1 / (1 - n u). The largest first-order relative figure any bound here charges is below 0.02 (eps_p of an attention weight with
R <= 104 and 48 tiles: 4 * 105 * 49 U32 = 1.3e-3; 2 (K + 2) U32 = 4.6e-4 at K = 3840; the fp16 terms U16 = 4.9e-4), so
1 / (1 - 0.02) < 1.05 bounds the dropped terms of every product of such factors."""
from __future__ import annotations

import numpy as np

from .mt_kernel_ref import SUB16, U16, U32, _f16, _ptr

SLACK = 1.05
T_AUDIO, T_PAD, T_TEXT, XSPLIT = 1500, 1536, 448, 8
LN_EPS = float(np.float32(1e-5))


def garbage(rng, shape):
    """+-1000 filler of everything a kernel must not read or write (every value distinct enough to notice a move)"""
    return rng.uniform(-1000, 1000, shape)


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (> 1: outside the bound); inf when anything is not finite"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


# ------------------------------------------------------------------ LayerNorm
def ln_ref(x, gamma, beta, mean_terms=None, eps_outside=False):
    """two-pass float64 LayerNorm of the rows of x (float32 values) over the last axis, eps = float32(1e-5) inside the square root.
    The two flags give the wrong answers: the mean summed over the first mean_terms columns only (still divided by d; a reduction
    that loses its last float4), and 1 / (sqrt(var) + eps) instead of 1 / sqrt(var + eps)."""
    x = np.asarray(x, np.float64)
    d = x.shape[-1]
    mean = x[..., :mean_terms or d].sum(-1, keepdims=True) / d
    var = ((x - mean) ** 2).sum(-1, keepdims=True) / d
    r = 1.0 / (np.sqrt(var) + LN_EPS) if eps_outside else 1.0 / np.sqrt(var + LN_EPS)
    return (x - mean) * r * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def ln_wrong_mean_short(x, gamma, beta):
    return ln_ref(x, gamma, beta, mean_terms=x.shape[-1] - 4)


def ln_wrong_eps_outside(x, gamma, beta):
    return ln_ref(x, gamma, beta, eps_outside=True)


def ln_bound(x, gamma, beta):
    """(e32, b16): bounds of |kernel fp32 value - float64| and of |kernel fp16 output - float64|, per element.
    The kernel (one wave per row): s = sum of the row, every element passing through at most D = 4 ceil(d / 256) + 6 fp32 additions
    (4 per float4 and lane, 6 shuffle levels), mean = s / d (one more rounding; 2 U32 charged) — so |mean_k - mean| <= em = (D + 2)
    U32 mean|x|. a_i = fl(x_i - mean_k) is off by em + U32 |x_i - mean|. Since sum_i (x_i - mean - t)^2 = d var + d t^2 exactly, the
    kernel's variance is (var + t^2)(1 + theta), |t| <= em, |theta| <= (D + 6) U32 (rounded difference squared, the square, the D sum
    levels, the division), plus eps and the rounding of that sum; rsqrtf is charged 1 ulp = 2 U32. The relative error of rstd is
    therefore at most er = em^2 / (var + eps) + (D + 11) U32 (the halving by the square root is not taken). The output
    ((x - mean_k) rstd_k) gamma + beta adds three roundings: e32 = |gamma| r (em + U32 |x - mean| + |x - mean| (er + 3 U32)) + U32 |y|.
    fp16: U16 |y| + SUB16 + (1 + U16) e32."""
    x = np.asarray(x, np.float64)
    g = np.abs(np.asarray(gamma, np.float64))
    d = x.shape[-1]
    D = 4 * -(-d // 256) + 6
    y = ln_ref(x, gamma, beta)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(var + LN_EPS)
    em = (D + 2) * U32 * np.abs(x).mean(-1, keepdims=True)
    er = em ** 2 / (var + LN_EPS) + (D + 11) * U32
    dev = np.abs(x - mean)
    e32 = SLACK * (g * r * (em + U32 * dev + dev * (er + 3 * U32)) + U32 * np.abs(y)) + 1e-30
    return e32, U16 * np.abs(y) + SUB16 + (1 + U16) * e32


def ln_emulate32(x, gamma, beta):
    """the kernel's arithmetic in numpy float32 in another association (numpy's pairwise sums over the reversed row)"""
    x = np.asarray(x, np.float32)
    d = np.float32(x.shape[-1])
    mean = x[..., ::-1].sum(-1, keepdims=True, dtype=np.float32) / d
    a = x - mean
    var = (a * a)[..., ::-1].sum(-1, keepdims=True, dtype=np.float32) / d
    r = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
    return a * r * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)


LN_DS = (128, 384, 768, 1024, 1280, 1536, 2048)
LN_MS = (1, 3, 4, 5, 1500)
LN_CASES = [(d, M) for d in LN_DS for M in LN_MS]


def ln_case(d, M, seed=0):
    """rows by kind (row % 6): 0 mean 0.5 / spread 0.03 (both wrong answers move it by far more than fp16), 1 standard normal, 2 mean
    1e3 / spread 1e-2, 3 constant (variance 0), 4 one huge element, 5 spread 30; gamma with zeros and negative entries; ldx > d
    and ldo > d on every other case with garbage in the gap; the float32 copy on every other d"""
    rng = np.random.default_rng(seed * 7919 + d * 13 + M)
    wide = (LN_DS.index(d) + LN_MS.index(M)) % 2 == 1
    ldx, ldo = (d + 12, d + 8) if wide else (d, d)
    x = garbage(rng, (M, ldx))
    for r in range(M):
        kind = r % 6
        row = rng.standard_normal(d)
        if kind == 0:
            row = 0.5 + 0.03 * row
        elif kind == 2:
            row = 1e3 + 1e-2 * row
        elif kind == 3:
            row = np.full(d, 3.0)
        elif kind == 4:
            row[int(rng.integers(d))] = 3e4
        elif kind == 5:
            row = 30 * row
        x[r, :d] = row
    gamma = rng.standard_normal(d)
    gamma[::7] = 0.0
    gamma[3::11] = -np.abs(gamma[3::11]) - 0.5
    beta = rng.standard_normal(d)
    return dict(x=x.astype(np.float32), gamma=gamma.astype(np.float32), beta=beta.astype(np.float32), d=d, M=M, ldx=ldx, ldo=ldo,
                out32=LN_DS.index(d) % 2 == 0)


# ------------------------------------------------------------------ softmax(q k^T) v with the statistics the bounds need
def attn_block(q, k, v, a_steps=128, n_exp=2, p16=True, n_acc=None):
    """(O, bound32, s) of softmax(q k^T) v for q [nq][64], k / v [nk][64] (float64 views of fp16 values); bound32 [nq][64] bounds
    |kernel fp32 value before the output rounding - O|:
      eps_p = U32 (a_steps A + 4 (R + 1) (n_exp + 1)): relative error of a weight p_j — the 64-term dot product of exact fp16
        products, each fp32 accumulation step charged 2 U32 on MFMA (a_steps = 128) or U32 on FMA chains (64), A = max_j sum_d
        |q_d k_jd|; and n_exp exponentials per weight (its own and the running-max / merge corrections), each 2 ulp of an argument
        of size <= R = max s - min s, as in mt_kernel_ref.attn_bound;
      a relative error eps of the weights moves O by at most 2 eps S, S = sum_j p_j |v_j| / sum_j p_j; the fp32 accumulation of acc
        over n_acc keys (2 U32 per MFMA step) and of l (in-lane and across lanes, <= nk + 16 steps), the rescales and the final
        division add (3 n_acc + 32) U32 S;
      p16: the weights enter the second MFMA rounded to fp16 while l sums them in fp32: U16 S, plus SUB16 per key for weights below
        the fp16 normal range: SUB16 sum_j |v_j| / l with l >= 1 (weights relative to the row maximum; a rescale by alpha <= 1 only
        shrinks that absolute error)."""
    s = q @ k.T
    A = (np.abs(q) @ np.abs(k).T).max(1, keepdims=True)
    R = s.max(1, keepdims=True) - s.min(1, keepdims=True)
    p = np.exp(s - s.max(1, keepdims=True))
    l = p.sum(1, keepdims=True)
    O = (p @ v) / l
    S = (p @ np.abs(v)) / l
    nk = k.shape[0]
    eps_p = U32 * (a_steps * A + 4 * (R + 1) * (n_exp + 1))
    b = 2 * eps_p * S + (3 * (n_acc or nk) + 32) * U32 * S
    if p16:
        b = b + U16 * S + SUB16 * np.abs(v).sum(0, keepdims=True) / l
    return O, SLACK * b, s


def to16(ref, e32):
    """bound of an fp16 output whose fp32 value is within e32 of ref"""
    return U16 * np.abs(ref) + SUB16 + (1 + U16) * e32


# ------------------------------------------------------------------ encoder attention
ENC_PATTERNS = ("dom32", "rising", "falling", "uniform")
# (T, H, items, pattern): T = 1500 with H 6 / 12 / 20 on both kernels (items * T >= 4000: eight waves), workgroup counts that are not
# multiples of 8 on both (T 129 H 3 items 1: 3 * 3 = 9; T 1500 H 3 items 3: 12 * 9 = 108), tile and query-block edges from the smallest
# legal T
ENC_CASES = [
    (1500, 6, 1, "dom32"), (1500, 12, 1, "rising"), (1500, 20, 1, "uniform"),
    (1500, 6, 3, "falling"), (1500, 12, 3, "dom32"), (1500, 20, 3, "rising"), (1500, 3, 3, "uniform"),
    (65, 6, 1, "dom32"), (127, 6, 1, "rising"), (128, 6, 1, "dom32"), (129, 3, 1, "falling"), (1472, 6, 1, "dom32"),
    (1473, 6, 1, "uniform"), (1499, 6, 1, "dom32"), (1501, 6, 1, "dom32"), (1535, 6, 1, "falling"),
    (65, 2, 62, "dom32"), (129, 3, 32, "uniform"), (1473, 6, 3, "dom32"), (1535, 3, 3, "rising"),
]
ENC_REFUSED = [(64, 6, 1, "dom32")]      # below three key tiles: the hook refuses it (refusal tests)


def enc_special(T, h):
    """the 32 keys head h's "dom32" queries single out: the interior tile 1 (keys 32..63) on even heads, the last tile on odd ones"""
    t = 1 if h % 2 == 0 else (T - 1) // 32
    return t * 32 + np.arange(32)


def enc_dom_index(T):
    """which of the head's 32 special keys query row i asks for: shifted by one every 16 rows, so that the probe rows (i % 16 == 5)
    take no position away"""
    i = np.arange(T)
    return (i + i // 16) % 32


def enc_case(T, H, items, pattern, seed=0):
    """Q / K [items][T][ld], V^T [items][H * 64][ldvt], O prefilled; wide strides, +-1000 in every unread column, in V^T columns >= T
    (the padding of the last tile) and between items. Scores: "dom32": dims 0..31 of K are one-hot over the head's 32 special keys and
    query i asks for special key enc_dom_index(T)[i] with weight 8 (softmax weight ~0.66 at T = 1500), so each of the 32 positions of an interior
    and of the last tile is the dominant key of some row — what separates the K and the V^T key orders inside a tile; the other
    patterns run along the keys in dim 0 (rising / falling across tiles, near-uniform). In every pattern rows i % 16 == 5 are probe
    rows: q = 8 e_32 and K[T - 1][32] = 1, i.e. they look at the LAST LIVE key (a dropped last key, or a padded key read as the
    clamped row T - 1, moves them by far more than the bound)."""
    rng = np.random.default_rng(seed * 100003 + T * 31 + H * 7 + items + ENC_PATTERNS.index(pattern) * 1009)
    w, tpad = 64 * H, (T + 31) // 32 * 32
    ldq, ldk, ldvt, ldo = w + 64, w + 8, tpad + 8, w + 4
    isq, isk, isv, iso = T * ldq + 16, T * ldk + 8, w * ldvt + 24, T * ldo + 8
    q = garbage(rng, (items, isq))
    k = garbage(rng, (items, isk))
    vt = garbage(rng, (items, isv))
    o = garbage(rng, (items, iso))
    x = np.arange(T) / (T - 1)
    for it in range(items):
        qv = q[it, :T * ldq].reshape(T, ldq)
        kv = k[it, :T * ldk].reshape(T, ldk)
        vv = vt[it, :w * ldvt].reshape(w, ldvt)
        for h in range(H):
            c = 64 * h
            qh = 0.05 * rng.standard_normal((T, 64))
            kh = rng.standard_normal((T, 64))
            if pattern == "dom32":
                kh[:, :32] = 0.0
                sp = enc_special(T, h)
                live = sp < T
                kh[sp[live], np.arange(32)[live]] = 1.0
                qh[:, :32] = 0.0
                qh[np.arange(T), enc_dom_index(T)] = 8.0
            else:
                pat = {"rising": -3 + 6 * x, "falling": 3 - 6 * x, "uniform": 0.05 * rng.standard_normal(T)}[pattern]
                kh[:, 0] = pat / 4.0
                qh[:, 0] = 4.0
            kh[:, 32] = 0.0
            kh[T - 1, 32] = 1.0
            probe = np.arange(T) % 16 == 5
            qh[probe] = 0.05 * rng.standard_normal((int(probe.sum()), 64))
            qh[probe, :33] = 0.0
            qh[probe, 32] = 8.0
            qv[:, c:c + 64] = qh
            kv[:, c:c + 64] = kh
            vv[c:c + 64, :T] = rng.standard_normal((64, T))
    return dict(q=_f16(q), k=_f16(k), vt=_f16(vt), o=_f16(o), T=T, H=H, items=items, pattern=pattern,
                ldq=ldq, ldk=ldk, ldvt=ldvt, ldo=ldo, isq=isq, isk=isk, isv=isv, iso=iso)


def enc_views(c, it, h):
    """float64 (Q [T][64], K [T][64], V^T [64][tpad]) of item it, head h"""
    T, w = c["T"], 64 * c["H"]
    s = slice(64 * h, 64 * h + 64)
    tpad = (T + 31) // 32 * 32
    q = c["q"][it, :T * c["ldq"]].reshape(T, -1)[:, s].astype(np.float64)
    k = c["k"][it, :T * c["ldk"]].reshape(T, -1)[:, s].astype(np.float64)
    vt = c["vt"][it, :w * c["ldvt"]].reshape(w, -1)[s, :tpad].astype(np.float64)
    return q, k, vt


def enc_pairs(c, subset=False):
    """(item, head) pairs; subset: first / last item x heads 0, 1, H - 1 (the host tests)"""
    its = sorted({0, c["items"] - 1}) if subset else range(c["items"])
    hs = sorted({0, min(1, c["H"] - 1), c["H"] - 1}) if subset else range(c["H"])
    return [(it, h) for it in its for h in hs]


def enc_ref(c, pairs, keys_of=None, v_of=None, rows=None):
    """{(item, head): (O [T][64], bound16 [T][64])}: softmax over the LIVE keys 0..T-1 (32-key tiles; the kernel's weights are
    rounded to fp16 for the second MFMA; one exponential per weight plus one running-max correction per tile: n_exp = ntiles).
    keys_of(k, vt, T) -> (k rows, v rows) replaces the key set (wrong answers); rows restricts the query rows."""
    T = c["T"]
    out = {}
    for it, h in pairs:
        q, k, vt = enc_views(c, it, h)
        if rows is not None:
            q = q[rows]
        kk, vv = (k, vt[:, :T].T) if keys_of is None else keys_of(k, vt, T)
        O, b32, _ = attn_block(q, kk, vv, a_steps=128, n_exp=(T + 31) // 32, p16=True)
        out[(it, h)] = (O, to16(O, b32))
    return out


def enc_wrong_leak_padded(c, pairs):
    """the first padded key taken for live: its K row is the clamped re-read of row T - 1, its V the V^T column T (None if T % 32 == 0)"""
    if c["T"] % 32 == 0:
        return None
    return enc_ref(c, pairs, keys_of=lambda k, vt, T: (np.vstack([k, k[T - 1:T]]), vt[:, :T + 1].T))


def enc_wrong_drop_last(c, pairs):
    """the last live key left out (the mask of the last tile off by one)"""
    return enc_ref(c, pairs, keys_of=lambda k, vt, T: (k[:T - 1], vt[:, :T - 1].T))


def enc_swap_pairs(c):
    """adjacent key pairs (j, j + 1) inside one tile whose exchange in V^T but not in K the case must notice: around every special key
    of "dom32" (both tiles), and the last two live keys (the probe rows) in every pattern"""
    T = c["T"]
    ps = {(T - 2, T - 1)} if (T - 2) // 32 == (T - 1) // 32 else set()
    if c["pattern"] == "dom32":
        for h in range(min(2, c["H"])):
            sp = enc_special(T, h)
            ps |= {(int(j), int(j) + 1) for j in sp[:-1] if j + 1 < T}
    return sorted(ps)


def enc_wrong_swap_v(c, pairs, pair):
    """keys pair[0] and pair[1] exchanged in V^T but not in K (the two key orders inside a tile disagreeing at one position)"""
    def keys_of(k, vt, T):
        v = vt[:, :T].T.copy()
        v[[pair[0], pair[1]]] = v[[pair[1], pair[0]]]
        return k, v
    return enc_ref(c, pairs, keys_of=keys_of)


def enc_emulate32(c, pairs):
    """float32 numpy in another association: scores and sums over the keys in reversed order, the weights rounded to fp16 for the
    numerator only, as the kernel's second MFMA sees them"""
    T = c["T"]
    out = {}
    for it, h in pairs:
        q, k, vt = (a.astype(np.float32) for a in enc_views(c, it, h))
        s = (q[:, ::-1] @ k[::-1, ::-1].T).astype(np.float32)
        p = np.exp(s - s.max(1, keepdims=True)).astype(np.float32)
        p16 = p.astype(np.float16).astype(np.float32)
        out[(it, h)] = ((p16 @ vt[:, :T].T[::-1]) / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float16)
    return out


def enc_excess(got, ref):
    return max(excess(got[key], ref[key][0], ref[key][1]) for key in ref)


def enc_unpack(c, o):
    """(dict (item, head) -> fp16 [T][64], mask of the bytes of `o` some thread owns) from the hook's O array"""
    T, w = c["T"], 64 * c["H"]
    owned = np.zeros(o.shape, bool)
    got = {}
    for it in range(c["items"]):
        ov = o[it, :T * c["ldo"]].reshape(T, -1)
        owned[it, :T * c["ldo"]].reshape(T, -1)[:, :w] = True
        for h in range(c["H"]):
            got[(it, h)] = ov[:, 64 * h:64 * h + 64]
    return got, owned


# ------------------------------------------------------------------ tile-packed cross K / V (the layout of the GEMM_CROSS_KV epilogue)
def pack_cross_k(K):
    """K [H][1536][64] -> the packed image [H * 48 * 2048]: per (head, 32-key tile) 2048 halfs, element ((s2 * 2 + kt2) * 64 + g * 16 + c)
    * 8 + e = K[key = tile * 32 + s2 * 16 + c][dim = kt2 * 32 + g * 8 + e] (gemm.hip, GEMM_CROSS_KV comment). Built as an index
    map from that formula."""
    K = np.asarray(K)
    H = K.shape[0]
    idx = np.arange(2048)
    e, lane, f = idx & 7, (idx >> 3) & 63, idx >> 9
    c, g, s2, kt2 = lane & 15, lane >> 4, f >> 1, f & 1
    key, dim = s2 * 16 + c, kt2 * 32 + g * 8 + e
    Kt = K.reshape(H, T_PAD // 32, 32, 64)
    return np.ascontiguousarray(Kt[:, :, key, dim]).reshape(-1)


def pack_cross_v(V):
    """V [H][1536][64] -> packed image: element (dt * 64 + g * 16 + c) * 8 + e = V[key = tile * 32 + (g * 4 + e if e < 4 else 16 + g * 4 +
    e - 4)][dim = dt * 16 + c]"""
    V = np.asarray(V)
    H = V.shape[0]
    idx = np.arange(2048)
    e, lane, dt = idx & 7, (idx >> 3) & 63, idx >> 9
    c, g = lane & 15, lane >> 4
    key = np.where(e < 4, g * 4 + e, 16 + g * 4 + e - 4)
    Vt = V.reshape(H, T_PAD // 32, 32, 64)
    return np.ascontiguousarray(Vt[:, :, key, dt * 16 + c]).reshape(-1)


def unpack_cross_k(img, H):
    """inverse of pack_cross_k, written independently as an axis permutation: the image is [H][tile][s2][kt2][g][c][e]"""
    a = np.asarray(img).reshape(H, T_PAD // 32, 2, 2, 4, 16, 8)
    return a.transpose(0, 1, 2, 5, 3, 4, 6).reshape(H, T_PAD, 64)          # key = (tile, s2, c), dim = (kt2, g, e)


def unpack_cross_v(img, H):
    """inverse of pack_cross_v: the image is [H][tile][dt][g][c][half][e4], key = (tile, half, g, e4), dim = (dt, c)"""
    a = np.asarray(img).reshape(H, T_PAD // 32, 4, 4, 16, 2, 4)
    return a.transpose(0, 1, 5, 3, 6, 2, 4).reshape(H, T_PAD, 64)


# ------------------------------------------------------------------ decode cross-attention (+ combine, + alignment scores)
XA_DOMS = (0, 191, 192, 1471, 1472, 1499)     # first key, both sides of a split edge, both sides of the last tile edge, last live key
# (H, R, groups, rows, n_items, pattern): R 1 / 4 / 5 / 15 / 16, groups 1 / 8 / 20, rows not a multiple of R, group_item with repeats
XA_CASES = [
    (6, 1, 1, 1, 2, "dom"), (6, 5, 1, 5, 2, "dom"), (12, 4, 8, 30, 3, "dom"), (20, 5, 20, 98, 4, "dom"), (6, 15, 8, 110, 3, "dom"),
    (6, 16, 1, 16, 2, "onesplit"), (12, 16, 8, 121, 2, "dom"), (20, 1, 20, 20, 3, "onesplit"), (6, 4, 20, 79, 5, "uniform"),
]


def xa_case(H, R, groups, rows, n_items, pattern, seed=0):
    """q [rows][ldq]; K / V [n_items][H][1536][64] and their packed images [n_items][item_stride]. Keys 1500..1535 of K hold +-1000
    (the kernel masks their scores; read as live they would outweigh every real key on about half the rows); of V zeros, as the engine's allocation guarantees (the slot's packed V is zeroed once
    and the GEMM epilogue never writes those keys), so a leaked padded key shows as a shrunken output. "dom": row r, head h has the
    dominant key XA_DOMS[(r + h) % 6] (dims 0..5 of K one-hot over them, q = 8 e); "onesplit": keys of split (r + h) % 8 score 100
    above the rest (every other split's exp(m - mmax) underflows in the combine); "uniform": near-flat scores. group_item is not the
    identity and repeats items."""
    rng = np.random.default_rng(seed * 100003 + H * 977 + R * 131 + groups * 17 + rows + ("dom", "onesplit", "uniform").index(pattern))
    w = 64 * H
    ldq, ldo = w + 8, w + 16
    item_stride = w * T_PAD + 64
    K = rng.standard_normal((n_items, H, T_PAD, 64))
    V = rng.standard_normal((n_items, H, T_PAD, 64))
    K[:, :, T_AUDIO:] = garbage(rng, (n_items, H, T_PAD - T_AUDIO, 64))
    V[:, :, T_AUDIO:] = 0.0
    q = garbage(rng, (rows, ldq))
    qh = 0.05 * rng.standard_normal((rows, H, 64))
    if pattern == "dom":
        K[:, :, :, :6] = 0.0
        for n, j in enumerate(XA_DOMS):
            K[:, :, j, n] = 1.0
        qh[:, :, :6] = 0.0
        for r in range(rows):
            for h in range(H):
                qh[r, h, (r + h) % 6] = 8.0
    elif pattern == "onesplit":
        K[:, :, :, :8] = 0.0
        for sp in range(XSPLIT):
            K[:, :, 192 * sp:192 * sp + 192, sp] = 12.5
        qh[:, :, :8] = 0.0
        for r in range(rows):
            for h in range(H):
                qh[r, h, (r + h) % 8] = 8.0
    q[:, :w] = qh.reshape(rows, w)
    K, V = _f16(K), _f16(V)
    kp = _f16(garbage(rng, (n_items, item_stride)))
    vp = _f16(garbage(rng, (n_items, item_stride)))
    for it in range(n_items):
        kp[it, :w * T_PAD] = pack_cross_k(K[it])
        vp[it, :w * T_PAD] = pack_cross_v(V[it])
    group_item = np.array([(3 * g + 1) % n_items for g in range(groups)], np.int32)
    return dict(q=_f16(q), K=K, V=V, kp=kp, vp=vp, item_stride=item_stride, n_items=n_items, H=H, R=R, groups=groups, rows=rows,
                group_item=group_item, ldq=ldq, ldo=ldo, pattern=pattern,
                part_o=_f16(garbage(rng, (groups, H, XSPLIT, 16, 64))), part_ml=garbage(rng, (groups, H, 16, XSPLIT, 2)).astype(np.float32),
                out=_f16(garbage(rng, (rows, ldo))), align_item=int(group_item[-1]), align_head=H - 1,
                align_out=garbage(rng, (rows, T_PAD)).astype(np.float32))


def xa_ref(c, item_of=None, nkeys=T_AUDIO, drop=None, swap=None, q=None, qb=None, dead_last=False):
    """dict of float64 references and bounds of one wlx_debug_dec_cross_attn call:
      part_o [groups][H][8][16][64]: softmax(q k^T) v over the live keys of each split of 192 keys (six 32-key tiles, one per wave, merged
        with one exponential each: n_exp = 2; weights rounded to fp16 for the second MFMA), fp16 — query lanes past R or past `rows`
        compute the group's first row again;
      part_m / part_l [groups][H][16][8]: the split's score maximum (bound: the score error em = 128 U32 A, two U32 per MFMA
        accumulation step) and sum of exp(s - m) (relative bound 2 eps_p + 2 em + 256 U32: eps_p of every term, the kernel's own
        maximum being off by <= em, 192 + 6 additions);
      out [rows][H * 64]: the whole softmax. The combine computes sum_sp w_sp o16_sp / sum_sp w_sp with w_sp = exp(m_sp - mmax) l_sp
        and o16_sp the fp16 partials: sum_sp f_sp b_sp (f_sp = the split's share of the mass, b_sp the bound of its partial, the
        second fp16 rounding included) + 2 ew sum_sp f_sp |o_sp| with ew = the relative bound of l + 2 em + 4 (Rm + 1) U32 (the
        exponential of m_sp - mmax, Rm = its range) + 16 U32 (eight products and additions, the division), then the fp16 rounding.
    Rm is clamped at 104 = 150 ln 2: below exp(-104) an fp32 value is under the smallest subnormal 2^-149, so __expf returns 0 (or a
    subnormal whose ABSOLUTE error is what matters: it is below 2^-149 times l_sp, nothing against the other splits' weights >= 1).
    The keyword arguments give the wrong answers (another item's K / V, a padded key taken for live, a key dropped, V rows swapped).
    q / qb (the fused LayerNorm + query projection + attention launch, tests/dec_gemv_kernel_ref.py): the query rows as float64 values
    the kernel's own fp16 query lies within qb of, element by element. A query off by dq moves score j by at most es_j = sum_d qb_d
    |k_jd|; with es = max_j es_j every weight p_j keeps its value up to a factor exp(+-2 es) against the others (its own shift and the
    maximum's), so m moves by <= es, l by the relative 2 es and O by 2 es S, S = sum_j p_j |v_j| / sum_j p_j (first order; SLACK
    covers exp(2 es) - 1 against 2 es for es <= 0.045 — (e^0.09 - 1) / 0.09 = 1.046 — which the cases keep). dead_last: that launch's query lanes past a group's live
    rows compute the group's LAST live row again, not its first."""
    H, R, G, rows = c["H"], c["R"], c["groups"], c["rows"]
    q64 = (c["q"] if q is None else q).astype(np.float64)
    po = np.zeros((G, H, XSPLIT, 16, 64))
    pob = np.zeros_like(po)
    pm = np.zeros((G, H, 16, XSPLIT))
    pmb, pl, plb = np.zeros_like(pm), np.zeros_like(pm), np.zeros_like(pm)
    out = np.zeros((rows, 64 * H))
    outb = np.zeros_like(out)
    for g in range(G):
        it = int(c["group_item"][g]) if item_of is None else item_of(g)
        dead = min(g * R + R, rows) - 1 if dead_last else g * R
        qr = np.array([g * R + cc if (cc < R and g * R + cc < rows) else dead for cc in range(16)])
        for h in range(H):
            k = c["K"][it, h].astype(np.float64)
            v = c["V"][it, h].astype(np.float64)
            if swap is not None:
                v = v.copy()
                v[[swap[0], swap[1]]] = v[[swap[1], swap[0]]]
            live = np.ones(T_PAD, bool)
            live[nkeys:] = False
            if drop is not None:
                live[drop] = False
            qq = q64[qr, 64 * h:64 * h + 64]
            mass = np.zeros((16, XSPLIT))
            for sp in range(XSPLIT):
                ks = np.arange(192 * sp, 192 * sp + 192)
                ks = ks[live[ks]]
                O, b32, s = attn_block(qq, k[ks], v[ks], a_steps=128, n_exp=2, p16=True)
                m = s.max(1)
                es = 0.0
                if qb is not None:
                    es = (qb[qr, 64 * h:64 * h + 64] @ np.abs(k[ks]).T).max(1)
                    pw = np.exp(s - m[:, None])
                    b32 = b32 + SLACK * 2 * es[:, None] * (pw @ np.abs(v[ks])) / pw.sum(1, keepdims=True)
                po[g, h, sp], pob[g, h, sp] = O, to16(O, b32)
                A = (np.abs(qq) @ np.abs(k[ks]).T).max(1)
                Rr = m - s.min(1)
                em = 128 * U32 * A
                pm[g, h, :, sp], pmb[g, h, :, sp] = m, SLACK * (em + es) + U32 * np.abs(m) + 1e-30
                l = np.exp(s - m[:, None]).sum(1)
                eps_p = U32 * (128 * A + 12 * (Rr + 1))
                pl[g, h, :, sp], plb[g, h, :, sp] = l, SLACK * l * (2 * eps_p + 2 * em + 256 * U32 + 2 * es)
                mass[:, sp] = l
            mmax = pm[g, h].max(1, keepdims=True)
            wgt = np.exp(pm[g, h] - mmax) * mass
            f = wgt / wgt.sum(1, keepdims=True)                       # [16][8]
            Rm = (mmax - pm[g, h]).max(1)
            ew = (plb[g, h] / pl[g, h]).max(1) + 2 * pmb[g, h].max(1) + (4 * (np.minimum(Rm, 104.0) + 1) + 16) * U32
            o = np.einsum("cs,scd->cd", f, po[g, h])
            b = np.einsum("cs,scd->cd", f, pob[g, h]) + SLACK * 2 * ew[:, None] * np.einsum("cs,scd->cd", f, np.abs(po[g, h]))
            n = min(R, rows - g * R)
            out[g * R:g * R + n, 64 * h:64 * h + 64] = o[:n]
            outb[g * R:g * R + n, 64 * h:64 * h + 64] = to16(o[:n], b[:n])
    return dict(part_o=(po, pob), part_m=(pm, pmb), part_l=(pl, plb), out=(out, outb))


def xa_align_ref(c, swap_halves=False):
    """(scores [rows][1536], bound): the raw 64-term dot products of head align_head with all 1536 padded keys of item align_item
    (two MFMAs: 2 U32 per accumulation step -> 128 U32 sum_d |q_d k_d|). swap_halves: the wrong answer with the two 16-key halves of
    every tile exchanged (the s2 index of the packed K read as the other half)."""
    h = c["align_head"]
    k = c["K"][c["align_item"], h].astype(np.float64)
    if swap_halves:
        k = k.reshape(-1, 2, 16, 64)[:, ::-1].reshape(T_PAD, 64)
    qq = c["q"][:, 64 * h:64 * h + 64].astype(np.float64)
    return qq @ k.T, SLACK * 128 * U32 * (np.abs(qq) @ np.abs(k).T) + 1e-30


def xa_excess(got, ref):
    """got: dict part_o / part_m / part_l / out -> worst excess over the four outputs"""
    return max(excess(got[n], ref[n][0], ref[n][1]) for n in ("part_o", "part_m", "part_l", "out"))


def xa_wrongs(c):
    """{name: reference dict of a broken kernel}"""
    w = {"neighbour_item": xa_ref(c, item_of=lambda g: (int(c["group_item"][g]) + 1) % c["n_items"]),
         "leak_padded_key": xa_ref(c, nkeys=T_AUDIO + 1),
         "drop_last_live_key": xa_ref(c, drop=T_AUDIO - 1)}
    if c["pattern"] == "dom":
        for a, b in ((0, 1), (190, 191), (192, 193), (1470, 1471), (1472, 1473), (1498, 1499)):
            w[f"swap_v_{a}_{b}"] = xa_ref(c, swap=(a, b))
    return w


def xa_emulate32(c):
    """float32 numpy, reversed key order, per split and combined as the kernels do (fp16 weights, fp16 partials)"""
    H, R, G, rows = c["H"], c["R"], c["groups"], c["rows"]
    q32 = c["q"].astype(np.float32)
    po = np.zeros((G, H, XSPLIT, 16, 64), np.float16)
    pm = np.zeros((G, H, 16, XSPLIT), np.float32)
    pl = np.zeros_like(pm)
    out = np.zeros((rows, 64 * H), np.float16)
    for g in range(G):
        it = int(c["group_item"][g])
        qr = np.array([g * R + cc if (cc < R and g * R + cc < rows) else g * R for cc in range(16)])
        for h in range(H):
            k = c["K"][it, h].astype(np.float32)
            v = c["V"][it, h].astype(np.float32)
            qq = q32[qr, 64 * h:64 * h + 64]
            for sp in range(XSPLIT):
                ks = np.arange(192 * sp, min(192 * sp + 192, T_AUDIO))[::-1]
                s = (qq[:, ::-1] @ k[ks][:, ::-1].T).astype(np.float32)
                m = s.max(1)
                p = np.exp(s - m[:, None]).astype(np.float32)
                l = p.sum(1, dtype=np.float32)
                po[g, h, sp] = ((p.astype(np.float16).astype(np.float32) @ v[ks]) / l[:, None]).astype(np.float16)
                pm[g, h, :, sp], pl[g, h, :, sp] = m, l
            wgt = (np.exp(pm[g, h] - pm[g, h].max(1, keepdims=True)) * pl[g, h]).astype(np.float32)
            o = np.einsum("cs,scd->cd", wgt[:, ::-1], po[g, h].astype(np.float32)[::-1]) / wgt.sum(1, dtype=np.float32)[:, None]
            n = min(R, rows - g * R)
            out[g * R:g * R + n, 64 * h:64 * h + 64] = o[:n].astype(np.float16)
    return dict(part_o=po, part_m=pm, part_l=pl, out=out)


# ------------------------------------------------------------------ decode self-attention over the KV cache
SA_POS = (0, 1, 31, 32, 33, 63, 64, 65, 447)
# (rows, H, ident, first position index): ident && rows <= 16 -> eight waves; ident && rows > 16 -> four; !ident -> table lookup, four.
# The 320-row cache is paired with H = 6 and positions <= 65 (a cache row then holds 66 positions: 16 MB per cache).
SA_CASES = [
    (1, 6, 1, 0), (1, 6, 1, 8), (1, 20, 1, 6), (5, 6, 1, 4), (16, 20, 1, 0), (16, 6, 1, 3),
    (17, 20, 1, 0), (40, 6, 1, 0), (320, 6, 1, 0),
    (1, 6, 0, 8), (5, 20, 0, 5), (17, 6, 0, 0), (40, 6, 0, 0), (320, 6, 0, 0),
]


def sa_case(rows, H, ident, p0, seed=0):
    """q [rows][ldq], caches [cache_rows][crs] with position p of a row at p * d, garbage past every row's filled positions and in
    the gap of crs. Row r sits at position SA_POS[(p0 + r) % 9] (<= 65 when rows = 320). Its history (ancestry row ancrow[r]: r
    itself, or a permutation for the table-lookup form) switches between the cache rows of its group of five at the block boundaries
    (64, 128, ...) and at random positions inside blocks. Scores rise gently towards the newest key (weight of the last key >= 1 / len)."""
    rng = np.random.default_rng(seed * 100003 + rows * 131 + H * 7 + ident * 3 + p0)
    d = 64 * H
    plist = [p for p in SA_POS if rows < 320 or p <= 65]
    pos = np.array([plist[(p0 + r) % len(plist)] for r in range(rows)], np.int32)
    npos = int(pos.max()) + 1
    cache_rows = rows + (0 if ident else 3)
    crs = (npos + 1) * d + 8
    ldq, ldo = 3 * d, d + 2
    ancrow = np.arange(rows, dtype=np.int32) if ident else rng.permutation(cache_rows)[:rows].astype(np.int32)
    anc = rng.integers(-30000, 30000, (cache_rows, T_TEXT)).astype(np.int16)         # entries past a row's history: never used
    # (the identity forms LOAD entries past the history — clamped to the row's 448 — but never use them as cache rows: out-of-range
    # garbage there, as in the engine's table)
    for r in range(rows):
        ln = int(pos[r]) + 1
        g0 = (int(ancrow[r]) // 5) * 5
        grp = [x for x in range(g0, g0 + 5) if x < cache_rows]
        cuts = sorted(set(range(64, ln, 64)) | {int(x) for x in rng.integers(1, max(ln, 2), size=max(1, ln // 40)) if x < ln})
        b, j = int(rng.integers(len(grp))), 0
        for cut in cuts + [ln]:
            anc[ancrow[r], j:cut] = grp[b]
            if len(grp) > 1:
                b = (b + 1 + int(rng.integers(len(grp) - 1))) % len(grp)
            j = cut
    # positions some history reads hold N(0, 1); every other position (one spare position behind the longest history included)
    # and the gap of the stride hold +-1000
    used = np.zeros((cache_rows, npos + 1), bool)
    for r in range(rows):
        ln = int(pos[r]) + 1
        used[anc[ancrow[r], :ln].astype(np.int64), np.arange(ln)] = True
    kc = garbage(rng, (cache_rows, crs))
    vc = garbage(rng, (cache_rows, crs))
    kn = rng.standard_normal((cache_rows, npos + 1, H, 64))
    kn[:, :, :, 0] = (np.arange(npos + 1) / 256.0)[None, :, None]
    vn = rng.standard_normal((cache_rows, npos + 1, H, 64))
    kv = kc[:, :(npos + 1) * d].reshape(cache_rows, npos + 1, H, 64)
    vv = vc[:, :(npos + 1) * d].reshape(cache_rows, npos + 1, H, 64)
    kv[used] = kn[used]
    vv[used] = vn[used]
    q = garbage(rng, (rows, ldq))
    qh = 0.2 * rng.standard_normal((rows, H, 64))
    qh[:, :, 0] = 2.0
    q[:, :d] = qh.reshape(rows, d)
    return dict(q=_f16(q), kc=_f16(kc), vc=_f16(vc), crs=crs, cache_rows=cache_rows, d=d, H=H, rows=rows, pos=pos, ancrow=ancrow,
                anc=anc, ident=ident, ldq=ldq, ldo=ldo, npos=npos, out=_f16(garbage(rng, (rows, ldo))))


def sa_ref(c, length_delta=0, late_switch=False):
    """(out [rows][H * 64], bound16): softmax over positions 0..pos[r] of the cache rows the ancestry names. The kernel works in fp32
    FMAs throughout (a_steps = 64: 8 FMAs and 3 butterfly additions per score are far below it; weights are NOT rounded to fp16),
    one exponential per weight plus one rescale per 64-position block and one per merged wave: n_exp = blocks + 2.
    Wrong answers: length_delta = +1 / -1 (the causal end off by one: one position too many — the garbage behind the history — or
    the newest key left out; rows whose history would be empty keep the right answer), late_switch (the first change of cache row
    in a row's history taken one position late)."""
    H, rows, d, npos = c["H"], c["rows"], c["d"], c["npos"]
    kcv, vcv = c["kc"].astype(np.float64), c["vc"].astype(np.float64)
    q64 = c["q"].astype(np.float64)
    out = np.zeros((rows, 64 * H))
    outb = np.zeros_like(out)
    for r in range(rows):
        ln = int(c["pos"][r]) + 1
        n = ln + length_delta
        if n < 1:
            n = ln
        ar = c["anc"][c["ancrow"][r]].astype(np.int64)[:ln]
        ar = np.concatenate([ar, np.full(max(n - ln, 0), ar[ln - 1])])      # (one position too many: from the newest key's cache row)
        if late_switch:
            sw = np.nonzero(ar[1:ln] != ar[:ln - 1])[0]
            if len(sw):
                ar[sw[0] + 1] = ar[sw[0]]
        p = np.arange(n)
        for h in range(H):
            off = (p * d + 64 * h)[:, None] + np.arange(64)[None, :]
            k = kcv[ar[:n, None], off]
            v = vcv[ar[:n, None], off]
            O, b32, _ = attn_block(q64[r:r + 1, 64 * h:64 * h + 64], k, v, a_steps=64, n_exp=(ln + 63) // 64 + 2, p16=False)
            out[r, 64 * h:64 * h + 64] = O[0]
            outb[r, 64 * h:64 * h + 64] = to16(O[0], b32[0])
    return out, outb


def sa_wrongs(c):
    """{name: out of a broken kernel} — the wrong answers that exist for the case (a history of one position has no newest key
    to drop and no switch)"""
    w = {"one_position_too_many": sa_ref(c, length_delta=+1)[0]}
    if (c["pos"] > 0).any():
        w["newest_key_dropped"] = sa_ref(c, length_delta=-1)[0]
    if any((np.diff(c["anc"][c["ancrow"][r]][:int(c["pos"][r]) + 1].astype(np.int64)) != 0).any() for r in range(c["rows"])):
        w["switch_one_late"] = sa_ref(c, late_switch=True)[0]
    return w


def sa_emulate32(c):
    H, rows, d = c["H"], c["rows"], c["d"]
    out = np.zeros((rows, 64 * H), np.float16)
    for r in range(rows):
        n = int(c["pos"][r]) + 1
        ar = c["anc"][c["ancrow"][r]].astype(np.int64)[:n][::-1]
        p = np.arange(n)[::-1]
        for h in range(H):
            off = (p * d + 64 * h)[:, None] + np.arange(64)[None, ::-1]
            k = c["kc"][ar[:, None], off].astype(np.float32)
            v = c["vc"][ar[:, None], off].astype(np.float32)
            s = k @ c["q"][r, 64 * h:64 * h + 64][::-1].astype(np.float32)
            pr = np.exp(s - s.max()).astype(np.float32)
            out[r, 64 * h:64 * h + 64] = ((pr @ v) / pr.sum(dtype=np.float32))[::-1].astype(np.float16)
    return out


# ------------------------------------------------------------------ the C-ABI hooks
def _u16(a):
    import ctypes as C
    return _ptr(a.view(np.uint16), C.c_uint16)


def run_ln(c, device=0, **over):
    """-> (rc, out16 fp16 [M * ldo], out32 float32 [M * ldo] or None, the +-1000 garbage out16 started as; out32 starts as the same
    values). `over` replaces hook arguments (refusal tests)."""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    a = dict(d=c["d"], M=c["M"], ldx=c["ldx"], ldo=c["ldo"])
    a.update(over)
    rng = np.random.default_rng(5)
    n_out = max(c["M"] * c["ldo"], a["M"] * a["ldo"]) if over else c["M"] * c["ldo"]
    o16 = _f16(garbage(rng, n_out))
    o32 = o16.astype(np.float32) if c["out32"] else None
    x = np.ascontiguousarray(c["x"], np.float32)
    rc = lib.wlx_debug_layernorm(device, _ptr(x, C.c_float), a["ldx"], _ptr(c["gamma"], C.c_float), _ptr(c["beta"], C.c_float), a["M"],
                                 a["d"], _u16(o16), _ptr(o32, C.c_float), a["ldo"])
    return rc, o16, o32, _f16(garbage(np.random.default_rng(5), n_out))


def run_enc(c, device=0, **over):
    """-> (rc, O fp16 [items][iso]) of one wlx_debug_attn_encoder call"""
    from whisperlive_amd import _lib
    lib = _lib.load()
    a = {n: c[n] for n in ("ldq", "isq", "ldk", "isk", "ldvt", "isv", "ldo", "iso", "T", "H", "items")}
    a.update(over)
    q, k, vt = (np.ascontiguousarray(c[n]) for n in ("q", "k", "vt"))
    o = np.ascontiguousarray(c["o"]).copy()
    rc = lib.wlx_debug_attn_encoder(device, _u16(q), a["ldq"], a["isq"], _u16(k), a["ldk"], a["isk"], _u16(vt), a["ldvt"], a["isv"],
                                    _u16(o), a["ldo"], a["iso"], a["T"], a["H"], a["items"])
    return rc, o


def run_xa(c, device=0, align=True, **over):
    """-> (rc, dict part_o / part_m / part_l / out / align) of one wlx_debug_dec_cross_attn call"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    a = {n: c[n] for n in ("ldq", "item_stride", "n_items", "H", "R", "groups", "rows", "ldo", "align_item", "align_head")}
    a.update(over)
    q, kp, vp = (np.ascontiguousarray(c[n]) for n in ("q", "kp", "vp"))
    gi = np.ascontiguousarray(over.get("group_item", c["group_item"]), np.int32)
    po, ml, out, al = (np.ascontiguousarray(c[n]).copy() for n in ("part_o", "part_ml", "out", "align_out"))
    rc = lib.wlx_debug_dec_cross_attn(device, _u16(q), a["ldq"], _u16(kp), _u16(vp), a["item_stride"], a["n_items"], a["H"], a["R"],
                                      a["groups"], a["rows"], _ptr(gi, C.c_int32), _u16(po), _ptr(ml, C.c_float), _u16(out), a["ldo"],
                                      a["align_item"], a["align_head"], _ptr(al if align else None, C.c_float))
    return rc, dict(part_o=po, part_m=ml[..., 0], part_l=ml[..., 1], out=out[:, :64 * c["H"]], out_full=out, align=al, part_ml=ml)


def run_sa(c, device=0, **over):
    """-> (rc, out fp16 [rows][ldo]) of one wlx_debug_dec_self_attn call"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    a = {n: c[n] for n in ("ldq", "crs", "cache_rows", "d", "H", "rows", "ident", "ldo")}
    a.update({k: v for k, v in over.items() if k in a})
    q, kc, vc = (np.ascontiguousarray(c[n]) for n in ("q", "kc", "vc"))
    pos = np.ascontiguousarray(over.get("pos", c["pos"]), np.int32)
    ancrow = np.ascontiguousarray(over.get("ancrow", c["ancrow"]), np.int32)
    anc = np.ascontiguousarray(over.get("anc", c["anc"]), np.int16)
    out = np.ascontiguousarray(c["out"]).copy()
    rc = lib.wlx_debug_dec_self_attn(device, _u16(q), a["ldq"], _u16(kc), _u16(vc), a["crs"], a["cache_rows"], a["d"], a["H"], a["rows"],
                                     _ptr(pos, C.c_int32), _ptr(ancrow, C.c_int32), _ptr(anc, C.c_int16), a["ident"], _u16(out), a["ldo"])
    return rc, out


# ------------------------------------------------------------------ encoder GEMM (launch_gemm: four kernels, six epilogues) + pack.hip
GEMM_TILES = {0: (64, 96), 1: (96, 96), 2: (128, 128), 3: (256, 256)}      # form -> (columns, rows) of a workgroup tile
E_ERF = 1.5e-7 + 32 * U32


def gelu64(x, tanh=False):
    import math
    if tanh:
        return 0.5 * x * (1 + np.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + np.vectorize(math.erf)(x / math.sqrt(2)))


def gemm_spec(mode, M, N, K, d=0, rpi=0, zbatch=1, lda=None, conv3_cin=0, KT=None, force=-1, name=""):
    return dict(mode=mode, M=M, N=N, K=K, d=d, rpi=rpi, zbatch=zbatch, lda=lda, conv3_cin=conv3_cin, KT=KT, force=force, name=name)


def _gemm_engine_cases():
    """the engine's own launches with launch_gemm's pick (force_form -1): per d the N = d / 3d / 4d / 2 d L and K = d / 4d launches at one
    window and at batched M, the two conv-as-GEMM launches (conv1: K = 3 n_mels in an even k-tile count, lda = n_mels, z-batched; conv2:
    K = 3 d at lda = 2 d)"""
    cs = []
    for d, nm in ((384, 80), (768, 80), (1280, 128)):
        kt1 = -(-(3 * nm) // 64) * 2
        cs += [gemm_spec(1, 3000, d, 3 * nm, lda=nm, conv3_cin=nm, KT=kt1, zbatch=2 if d == 384 else 1, name="conv1"),
               gemm_spec(2, 1500, d, 3 * d, lda=2 * d, conv3_cin=d, zbatch=3 if d == 384 else 1, name="conv2"),
               gemm_spec(4, 1500, 3 * d, d, d=d, rpi=1500, name="qkv"), gemm_spec(3, 1500, d, d, name="attn_out"),
               gemm_spec(1, 1500, 4 * d, d, name="fc1"), gemm_spec(3, 1500, d, 4 * d, name="fc2")]
    cs += [gemm_spec(5, 1500, 2 * 384 * 4, 384, d=384, rpi=1500, name="cross_kv_L4"),
           gemm_spec(5, 1500, 2 * 768 * 12, 768, d=768, rpi=1500, name="cross_kv_L12"),
           gemm_spec(4, 3000, 3 * 384, 384, d=384, rpi=1500, name="qkv_x2"), gemm_spec(4, 4500, 3 * 768, 768, d=768, rpi=1500, name="qkv_x3"),
           gemm_spec(1, 4500, 4 * 384, 384, name="fc1_x3"), gemm_spec(3, 7500, 384, 4 * 384, name="fc2_x5"),
           gemm_spec(5, 3000, 2 * 384 * 4, 384, d=384, rpi=1500, name="cross_kv_x2")]
    return cs


def _gemm_form_cases():
    """every (form, mode, epilogue, XCD remap) combination the launcher can produce, forced: d = 384 at one row of tiles (fewer than 16
    tiles or a count that is no multiple of 8: remap off), d = 768 at four rows of tiles (remap on); rows_per_item 128 (LDS-transposed
    epilogue for the fp16 modes) or 125 (& 3 != 0: direct). The large-M form has no remap (its own XCD-run tile list); with d = 384
    its scattering mode 5 runs the direct epilogue (d % 256 != 0)."""
    cs = []
    for form in (0, 1, 2):
        rows = GEMM_TILES[form][1]
        for mode in range(6):
            for rpi in ((128, 125) if mode in (0, 1, 4, 5) else (0,)):
                for remap in (0, 1):
                    d = 768 if remap else 384
                    M = 4 * rows - 5 if remap else rows - 6
                    N = 3 * d if mode == 4 else 2 * d
                    cs.append(gemm_spec(mode, M, N, 64, d=d if mode >= 4 else 0, rpi=rpi, force=form, name="f%d_remap%d" % (form, remap)))
    for mode in range(6):
        for rpi in ((128, 125) if mode in (0, 1, 4, 5) else (0,)):
            cs.append(gemm_spec(mode, 300, 3 * 768 if mode == 4 else 1536, 256, d=768 if mode >= 4 else 0, rpi=rpi, force=3, name="f3"))
    cs.append(gemm_spec(5, 300, 768 * 2, 256, d=384, rpi=128, force=3, name="f3_d384_direct"))
    # remap (a, b) = (1, 8) and a > 1 on the 64 x 96 tile; z-batched on the 96 x 96 tile; ragged last n-tile (N = 200) on the second form
    cs += [gemm_spec(0, 96, 1024, 64, force=0, name="remap_1_8"), gemm_spec(3, 192, 512, 64, force=0, name="remap_a2"),
           gemm_spec(1, 200, 384, 128, zbatch=3, force=1, name="z3"), gemm_spec(2, 100, 384, 128, zbatch=1, force=1, name="z1")]
    cs += [gemm_spec(m, 130, 200, 96, KT=4, force=f, name="ragged_n") for f in (0, 1, 2) for m in (0, 1, 2, 3)]
    return cs


GEMM_EDGE_MS = (1, 15, 16, 17, 95, 96, 97, 127, 128, 129, 255, 256, 257, 1500)
GEMM_ENGINE_CASES = _gemm_engine_cases()
GEMM_FORM_CASES = _gemm_form_cases()
# forced forms the launcher's contract refuses (-> the refusal tests): a scattering mode on a tile d is no multiple of, and the large-M
# form on N % 256, KT % 4, KT < 8, zbatch 3
GEMM_REFUSED = [gemm_spec(4, 100, 3 * 64, 64, d=64, rpi=100, force=1), gemm_spec(5, 100, 2 * 320, 64, d=320, rpi=100, force=2),
                gemm_spec(0, 300, 384, 256, force=3), gemm_spec(0, 300, 256, 192, force=3), gemm_spec(0, 300, 256, 128, force=3),
                gemm_spec(0, 300, 256, 256, zbatch=3, force=3), gemm_spec(0, 100, 256, 96, KT=3, force=0), gemm_spec(0, 100, 204, 64, force=0)]


def gemm_edge_case(M, form):
    """the same inputs for every form at one M (K = 256, d = 768), the mode cycling with M: the four forms must agree bit for bit"""
    mode = GEMM_EDGE_MS.index(M) % 6
    return gemm_spec(mode, M, 3 * 768 if mode == 4 else 1536, 256, d=768 if mode >= 4 else 0, rpi=128 if mode >= 4 else 0, force=form,
                     name="edge")


def gemm_case(s, seed=0):
    """inputs and garbage-filled destinations of one launch. A: N(0, 1) everywhere a row may be read (KT * 32 columns from its start;
    columns past K meet zero weights), W = N(0, 1) / sqrt(K) (smaller in the GELU modes), bias = 3 N(0, 1) (a column group shifted by 4 moves an output by ~4),
    pos N(0, 1), X prefilled with N(0, 1) on the rows the residual reads; strides wider than the rows, gaps and rows / items / keys past
    the end +-1000."""
    rng = np.random.default_rng(seed * 1000003 + s["mode"] * 7 + s["M"] * 13 + s["N"] * 3 + s["K"] + s["zbatch"])
    mode, M, N, K, Z, d = s["mode"], s["M"], s["N"], s["K"], s["zbatch"], s["d"]
    KT = s["KT"] or -(-K // 64) * 2
    lda = s["lda"] or KT * 32 + 8
    strideA = (M - 1) * lda + KT * 32 + 16 if Z > 1 else 0
    a_len = (Z - 1) * strideA + (M - 1) * lda + KT * 32
    c = dict(s, KT=KT, lda=lda, strideA=strideA, a_len=a_len)
    c["A"] = _f16(rng.standard_normal(a_len))
    # (GELU modes: the worst-case accumulation bound, 2 (K + 2) U32 sum |a w|, must stay below the ~3e-4 by which tanh-GELU differs
    # from erf-GELU, so their weights are small and the bias spreads x over the interesting range)
    wscale = 1 / (K * max(1.0, K / 256)) if mode in (1, 2) else 1 / np.sqrt(K)
    c["W"] = (rng.standard_normal((N, K)) * wscale).astype(np.float32)
    c["bias"] = (3 * rng.standard_normal(N)).astype(np.float32)
    c["pos"] = rng.standard_normal((M, N)).astype(np.float32) if mode == 2 else None
    c["qscale"] = 0.125
    rpi = s["rpi"]
    if mode in (0, 1):
        c["ldc"] = N + 8
        c["strideC"] = M * c["ldc"] + 24
        c["C"] = _f16(garbage(rng, (Z - 1) * c["strideC"] + M * c["ldc"] + 16))
    elif mode in (2, 3):
        c["ldx"] = N + 4
        c["strideX"] = M * c["ldx"] + 12
        X = garbage(rng, (Z - 1) * c["strideX"] + M * c["ldx"] + 8)
        if mode == 3:
            for z in range(Z):
                X[z * c["strideX"]:z * c["strideX"] + M * c["ldx"]].reshape(M, -1)[:, :N] = rng.standard_normal((M, N))
        c["X"] = X.astype(np.float32)
    else:
        items = -(-M // rpi)
        c["items"] = items
        if mode == 4:
            c["ldc"] = d + 8
            c["C"] = _f16(garbage(rng, M * c["ldc"] + 8))
            c["ldk"], c["ldvt"] = d + 16, (rpi + 3) // 4 * 4 + 8
            c["kis"], c["vis"] = rpi * c["ldk"] + 8, d * c["ldvt"] + 16
            c["kls"] = c["vls"] = 0
            c["Kout"] = _f16(garbage(rng, items * c["kis"]))
            c["Vt"] = _f16(garbage(rng, items * c["vis"]))
        else:
            L = N // (2 * d)
            c["L"] = L
            c["kis"] = c["vis"] = d * T_PAD + 8
            c["kls"] = c["vls"] = items * c["kis"] + 16
            c["Kout"] = _f16(garbage(rng, L * c["kls"]))
            c["Vt"] = _f16(garbage(rng, L * c["vls"]))
    return c


def gemm_rows(c):
    """A as the GEMM reads it: [zbatch][M][K] float64 (overlapping rows when lda < K: the conv windows)"""
    idx = (np.arange(c["zbatch"]) * c["strideA"])[:, None, None] + (np.arange(c["M"]) * c["lda"])[None, :, None] + np.arange(c["K"])[None, None, :]
    return c["A"].astype(np.float64)[idx]


def gemm_w16(c):
    """the fp16 weights as [N][K]: a conv weight [N][Cin][3] is read as k = j * Cin + ci"""
    W = c["W"]
    if c["conv3_cin"]:
        W = W.reshape(c["N"], c["conv3_cin"], 3).transpose(0, 2, 1).reshape(c["N"], c["K"])
    return W.astype(np.float16).astype(np.float64)


def acc_bound(absdot, K):
    """bound of an fp32 accumulation of K exact fp16 products in any association, absdot = sum_k |a_k w_k|: every accumulation step is
    charged 2 U32 since the rounding of the MFMA's internal additions is not documented (the derivation is gemm_logical's)"""
    return 2 * (K + 2) * U32 * absdot


def gemm_logical(c, wrong=None):
    """(values [Z][M][N] float64 the epilogue stores or adds, bound32 of their fp32 form, x0 or None).
    acc = A W^T: exact fp16 products, K fp32 accumulation steps (plus the zero-weight padding steps, which add exact zeros) charged
    2 U32 each since the rounding of the MFMA's internal additions is not documented: e32 = 2 (K + 2) U32 sum_k |a_k w_k| + U32 |bias|.
    GELU (modes 1, 2): |gelu'| <= 1.13 carries e32 through; erf_as is Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7) evaluated with one
    rcpf (1 ulp), one __expf (2 ulp) and five fp32 Horner steps whose coefficients (sum of |c_i| i < 12) amplify the relative error
    of t: E_ERF = 1.5e-7 + 32 U32 on erf, i.e. 0.5 |x| E_ERF on the result, plus 4 U32 (|gelu| + |x|) for the products.
    + pos / + residual: one more fp32 rounding of the sum (mode 3 adds acc + bias first: two). q: one rounding of the product by qscale.
    wrong: "bias_shift" (the bias of column group 16..31 read 4 columns on), "tanh_gelu", "garbage_tile" (a 64 x 64 tile never written),
    "qscale_on_k" (mode 4)."""
    rows, w = gemm_rows(c), gemm_w16(c)
    bias = c["bias"].astype(np.float64).copy()
    if wrong == "bias_shift":
        bias[16:32] = bias[20:36]
    x = rows @ w.T + bias
    e = acc_bound(np.abs(rows) @ np.abs(w).T, c["K"]) + U32 * np.abs(c["bias"].astype(np.float64))
    mode = c["mode"]
    x0 = None
    if mode in (1, 2):
        g = gelu64(x, tanh=wrong == "tanh_gelu")
        e = 1.13 * e + 0.5 * np.abs(x) * E_ERF + 4 * U32 * (np.abs(g) + np.abs(x))
        x = g
        if mode == 2:
            x = x + c["pos"].astype(np.float64)[None]
            e = e + U32 * np.abs(x)
    elif mode == 3:
        Z, M, N = x.shape
        x0 = np.stack([c["X"][z * c["strideX"]:z * c["strideX"] + M * c["ldx"]].reshape(M, -1)[:, :N] for z in range(Z)]).astype(np.float64)
        x = x0 + x
        e = e + 2 * U32 * (np.abs(x) + np.abs(x0))
    elif mode == 4:
        d = c["d"]
        x[..., :d] *= c["qscale"]
        e[..., :d] = e[..., :d] * c["qscale"] + U32 * np.abs(x[..., :d])
        if wrong == "qscale_on_k":
            x[..., d:2 * d] *= c["qscale"]
    if wrong == "garbage_tile":
        x[0, :64, :64] = 1000.0
    return x, SLACK * e + 1e-30


def gemm_check(c, out, wrong=None, vt_shift=0):
    """(worst excess over every destination element some thread owns, True when every other byte kept its bits). The placement is
    exact: each destination is read back through its documented layout — C / X rows, q rows, K rows per item, V^T [d][ldvt] per item,
    the packed cross K / V images through unpack_cross_k / unpack_cross_v — into the logical [M][N] result. vt_shift = 1: the wrong
    answer with every V^T element stored one time step late."""
    x, e = gemm_logical(c, wrong)
    mode, M, N, Z, d, rpi = c["mode"], c["M"], c["N"], c["zbatch"], c["d"], c["rpi"]
    worst, clean = 0.0, True
    bits = lambda a: a.view(np.uint16 if a.dtype == np.float16 else np.uint32)
    if mode in (0, 1, 2, 3):
        name, ld, st = ("C", c["ldc"], c["strideC"]) if mode < 2 else ("X", c["ldx"], c["strideX"])
        got, init = out[name], c[name]
        owned = np.zeros(got.shape, bool)
        for z in range(Z):
            v = got[z * st:z * st + M * ld].reshape(M, ld)[:, :N]
            owned[z * st:z * st + M * ld].reshape(M, ld)[:, :N] = True
            worst = max(worst, excess(v, x[z], to16(x[z], e[z]) if mode < 2 else e[z]))
        return worst, bool((bits(got)[~owned] == bits(init)[~owned]).all())
    x, e = x[0], e[0]
    items = c["items"]
    if mode == 4:
        got, init = out["C"], c["C"]
        owned = np.zeros(got.shape, bool)
        owned[:M * c["ldc"]].reshape(M, -1)[:, :d] = True
        worst = excess(got[:M * c["ldc"]].reshape(M, -1)[:, :d], x[:, :d], to16(x[:, :d], e[:, :d]))
        clean = bool((bits(got)[~owned] == bits(init)[~owned]).all())
        gk, gv = out["Kout"], out["Vt"]
        ok, ov = np.zeros(gk.shape, bool), np.zeros(gv.shape, bool)
        for it in range(items):
            tl = min(rpi, M - it * rpi)
            sl = slice(it * rpi, it * rpi + tl)
            kv = gk[it * c["kis"]:it * c["kis"] + tl * c["ldk"]].reshape(tl, -1)[:, :d]
            ok[it * c["kis"]:it * c["kis"] + tl * c["ldk"]].reshape(tl, -1)[:, :d] = True
            worst = max(worst, excess(kv, x[sl, d:2 * d], to16(x[sl, d:2 * d], e[sl, d:2 * d])))
            vv = gv[it * c["vis"]:it * c["vis"] + d * c["ldvt"]].reshape(d, -1)
            ov[it * c["vis"]:it * c["vis"] + d * c["ldvt"]].reshape(d, -1)[:, :tl] = True
            ref = x[sl, 2 * d:].T
            if vt_shift:
                ref = np.concatenate([np.full((d, 1), 1000.0), ref[:, :-1]], axis=1)
            worst = max(worst, excess(vv[:, :tl], ref, to16(ref, e[sl, 2 * d:].T)))
        clean = clean and bool((bits(gk)[~ok] == bits(c["Kout"])[~ok]).all()) and bool((bits(gv)[~ov] == bits(c["Vt"])[~ov]).all())
        return worst, clean
    H, L, img = d // 64, c["L"], d * T_PAD
    for name, unpack, part in (("Kout", unpack_cross_k, 0), ("Vt", unpack_cross_v, 1)):
        got, init = out[name], c[name]
        owned = np.zeros(got.shape, bool)
        for l in range(L):
            for it in range(items):
                o0 = l * c["kls"] + it * c["kis"]
                tl = min(rpi, M - it * rpi)
                g3, i3 = unpack(got[o0:o0 + img], H), unpack(init[o0:o0 + img], H)          # [H][1536][64]
                owned[o0:o0 + img] = True
                cols = slice(l * 2 * d + part * d, l * 2 * d + part * d + d)
                ref = x[it * rpi:it * rpi + tl, cols].reshape(tl, H, 64).transpose(1, 0, 2)
                eb = e[it * rpi:it * rpi + tl, cols].reshape(tl, H, 64).transpose(1, 0, 2)
                worst = max(worst, excess(g3[:, :tl], ref, to16(ref, eb)))
                clean = clean and bool((bits(np.ascontiguousarray(g3[:, tl:])) == bits(np.ascontiguousarray(i3[:, tl:]))).all())
        clean = clean and bool((bits(got)[~owned] == bits(init)[~owned]).all())
    return worst, clean


def gemm_place(c, x):
    """the destinations a correct kernel leaves for logical values x [Z][M][N] (fp16 / fp32 rounded), on top of the garbage: the inverse
    of gemm_check's reading, for the host tests"""
    mode, M, N, Z, d, rpi = c["mode"], c["M"], c["N"], c["zbatch"], c["d"], c["rpi"]
    out = {n: c[n].copy() for n in ("C", "X", "Kout", "Vt") if n in c}
    if mode < 4:
        name, ld, st = ("C", c["ldc"], c["strideC"]) if mode < 2 else ("X", c["ldx"], c["strideX"])
        for z in range(Z):
            out[name][z * st:z * st + M * ld].reshape(M, ld)[:, :N] = x[z]
        return out
    x = x[0]
    if mode == 4:
        out["C"][:M * c["ldc"]].reshape(M, -1)[:, :d] = x[:, :d]
        for it in range(c["items"]):
            tl = min(rpi, M - it * rpi)
            sl = slice(it * rpi, it * rpi + tl)
            out["Kout"][it * c["kis"]:it * c["kis"] + tl * c["ldk"]].reshape(tl, -1)[:, :d] = x[sl, d:2 * d]
            out["Vt"][it * c["vis"]:it * c["vis"] + d * c["ldvt"]].reshape(d, -1)[:, :tl] = x[sl, 2 * d:].T
        return out
    H, img = d // 64, d * T_PAD
    for name, pack, unpack, part in (("Kout", pack_cross_k, unpack_cross_k, 0), ("Vt", pack_cross_v, unpack_cross_v, 1)):
        for l in range(c["L"]):
            for it in range(c["items"]):
                o0 = l * c["kls"] + it * c["kis"]
                tl = min(rpi, M - it * rpi)
                full = unpack(out[name][o0:o0 + img], H).copy()
                cols = slice(l * 2 * d + part * d, l * 2 * d + part * d + d)
                full[:, :tl] = x[it * rpi:it * rpi + tl, cols].reshape(tl, H, 64).transpose(1, 0, 2)
                out[name][o0:o0 + img] = pack(full)
    return out


def gemm_emulate32(c):
    """float32 numpy with the K order reversed; erf from the math library"""
    rows, w = gemm_rows(c).astype(np.float32)[..., ::-1], gemm_w16(c).astype(np.float32)[:, ::-1]
    x = (rows @ w.T + c["bias"]).astype(np.float32)
    if c["mode"] in (1, 2):
        x = gelu64(x.astype(np.float64)).astype(np.float32)
        if c["mode"] == 2:
            x = x + c["pos"][None]
    elif c["mode"] == 3:
        x = gemm_logical(c)[0] - (gemm_rows(c) @ gemm_w16(c).T + c["bias"]) + x
    elif c["mode"] == 4:
        x[..., :c["d"]] *= np.float32(c["qscale"])
    return x.astype(np.float32)


def gemm_wrongs(c):
    w = ["bias_shift", "garbage_tile"]
    if c["mode"] in (1, 2):
        w.append("tanh_gelu")
    if c["mode"] == 4:
        w += ["qscale_on_k", "vt_shift"]
    return w


def gemm_combos():
    """{(form, mode, epi_lds, remap on)} launch_gemm's kernels can run, and the ones nobody can reach, with the reason"""
    reach, unreachable = set(), {}
    for form in range(4):
        for mode in range(6):
            for epi in (0, 1):
                for remap in (0, 1):
                    key = (form, mode, epi, remap)
                    if epi and mode in (2, 3):
                        unreachable[key] = "the fp32 modes store from registers: no LDS-transposed epilogue"
                    elif form == 3 and remap:
                        unreachable[key] = "the large-M form walks its own XCD-run tile list: no remap"
                    else:
                        reach.add(key)
    return reach, unreachable


def run_gemm(c, device=0, **over):
    """-> (rc, dict C / X / Kout / Vt of the copied-back destinations, (form, epi_lds, xcd_a, xcd_b))"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    a = _lib.wlx_debug_gemm_args()
    out = {n: c[n].copy() for n in ("C", "X", "Kout", "Vt") if n in c}
    vals = dict(zbatch=c["zbatch"], M=c["M"], N=c["N"], K=c["K"], KT=c["KT"], conv3_cin=c["conv3_cin"], mode=c["mode"], force_form=c["force"],
                d=c["d"], rows_per_item=c["rpi"], qscale=c["qscale"], lda=c["lda"], strideA=c["strideA"], a_len=c["a_len"],
                ldc=c.get("ldc", 0), strideC=c.get("strideC", 0), c_len=len(out["C"]) if "C" in out else 0,
                ldx=c.get("ldx", 0), strideX=c.get("strideX", 0), x_len=len(out["X"]) if "X" in out else 0,
                ldk=c.get("ldk", 0), kv_item_stride_k=c.get("kis", 0), kv_layer_stride_k=c.get("kls", 0), k_len=len(out["Kout"]) if "Kout" in out else 0,
                ldvt=c.get("ldvt", 0), kv_item_stride_v=c.get("vis", 0), kv_layer_stride_v=c.get("vls", 0), v_len=len(out["Vt"]) if "Vt" in out else 0)
    vals.update(over)
    for k, v in vals.items():
        setattr(a, k, v)
    ran = np.full(4, -1, np.int32)
    A, W = np.ascontiguousarray(c["A"]), np.ascontiguousarray(c["W"], np.float32)
    rc = lib.wlx_debug_gemm(device, C.byref(a), _u16(A), _ptr(W, C.c_float), _ptr(c["bias"], C.c_float), _ptr(c["pos"], C.c_float),
                            _u16(out["C"]) if "C" in out else None, _ptr(out.get("X"), C.c_float),
                            _u16(out["Kout"]) if "Kout" in out else None, _u16(out["Vt"]) if "Vt" in out else None, _ptr(ran, C.c_int32))
    return rc, out, tuple(int(v) for v in ran)
