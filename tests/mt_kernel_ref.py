"""float64 references of the translation engine's kernels (whisperlive_amd/csrc/mt.hip), their error bounds and the nearest
plausible wrong answers that the bounds must exclude. Inputs are the fp16-rounded (attention, embedding) or fp32 (top-k) values
the kernels see; everything is computed in float64 with numpy."""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32
U16 = 2.0 ** -11          # unit roundoff of fp16 (normal range)
SUB16 = 2.0 ** -25        # half the spacing of fp16 subnormals


# ------------------------------------------------------------------ attention
def key_rows(group, anc=None, ld_anc=0, tmax=0):
    """K / V row of every key of a group (q0, nq, k0, nk): k0 + j, or anc[q0][j] * tmax + j through the ancestry table"""
    q0, _, k0, nk = group
    j = np.arange(nk)
    if anc is None:
        return k0 + j
    return np.asarray(anc, np.int64).reshape(-1)[q0 * ld_anc + j] * tmax + j


def attn_ref(q, k, v, groups, heads, anc=None, ld_anc=0, tmax=0, rows_of=None):
    """softmax(q k^T) v per group and head in float64. q / k / v: fp16 arrays [rows][>= 64 heads]. Returns (out, scores):
    out[(row, h)] = float64 [64], scores[(row, h)] = float64 [nk]. rows_of(group) overrides the key rows (wrong answers)."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    out, scores = {}, {}
    for g in groups:
        q0, nq = g[0], g[1]
        kr = rows_of(g) if rows_of else key_rows(g, anc, ld_anc, tmax)
        for h in range(heads):
            c = slice(64 * h, 64 * h + 64)
            for i in range(q0, q0 + nq):
                s = k64[kr, c] @ q64[i, c]
                p = np.exp(s - s.max())
                out[(i, h)] = (p @ v64[kr, c]) / p.sum()
                scores[(i, h)] = s
    return out, scores


def attn_bound(q, k, v, groups, heads, anc=None, ld_anc=0, tmax=0):
    """per-element bound of |kernel - float64| (same keys as attn_ref). The kernel rounds its fp32 result to fp16:
    U16 |O| + SUB16, plus (1 + U16) times the fp32 error e32 of the value before rounding. e32 = 2 (eps_p + (nk + 2) U32) S with
    S = sum_j p_j |v_j| / sum_j p_j: a relative error eps_p of every weight p_j moves O by at most eps_p sum_j p_j |v_j - O| <=
    2 eps_p S, and the fp32 sums of nk terms in acc and l add (nk + 2) U32 S each. eps_p = U32 (64 A + 4 (R + 1) (T + 1)):
    the 64-term fp32 dot product of fp16 operands (exact products) with A = max_j sum_d |q_d k_jd|, and the __expf of the
    weight and of the T running-max corrections, each exact to 2 ulp of an argument of size <= R = max s - min s."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    ref, _ = attn_ref(q, k, v, groups, heads, anc, ld_anc, tmax)
    bound = {}
    for g in groups:
        q0, nq, _, nk = g
        kr = key_rows(g, anc, ld_anc, tmax)
        ntiles = (nk + 63) // 64
        for h in range(heads):
            c = slice(64 * h, 64 * h + 64)
            for i in range(q0, q0 + nq):
                s = k64[kr, c] @ q64[i, c]
                A = (np.abs(k64[kr, c]) @ np.abs(q64[i, c])).max()
                R = s.max() - s.min()
                p = np.exp(s - s.max())
                S = (p @ np.abs(v64[kr, c])) / p.sum()
                eps_p = U32 * (64 * A + 4 * (R + 1) * (ntiles + 1))
                e32 = 2 * (eps_p + (nk + 2) * U32) * S
                bound[(i, h)] = U16 * np.abs(ref[(i, h)]) + SUB16 + (1 + U16) * e32
    return bound


def attn_excess(got, ref, bound):
    """max over every row, head and dim of |got - ref| / bound (> 1: outside the bound)"""
    return max(float((np.abs(np.asarray(got[key], np.float64) - ref[key]) / bound[key]).max()) for key in ref)


def attn_wrong_drop_tile_end(q, k, v, groups, heads, anc=None, ld_anc=0, tmax=0):
    """the answer with the last key of the heaviest tile of each group left out (a tile loop's `live` bound off by one)"""
    q64, k64 = np.asarray(q, np.float64), np.asarray(k, np.float64)

    def rows_of(g):
        kr = key_rows(g, anc, ld_anc, tmax)
        nk = g[3]
        s = k64[kr, 0:64] @ q64[g[0], 0:64]
        p = np.exp(s - s.max())
        t = int(np.argmax([p[j0:j0 + 64].sum() for j0 in range(0, nk, 64)]))
        last = min(64 * t + 63, nk - 1)
        return kr[np.arange(nk) != last] if nk > 1 else kr
    return attn_ref(q, k, v, groups, heads, anc, ld_anc, tmax, rows_of=rows_of)[0]


def attn_wrong_neighbour_tile(q, k, v, groups, heads, anc, ld_anc, tmax, n_beams):
    """the answer with the keys of each group's heaviest tile gathered from the neighbouring beam's cache rows"""
    q64, k64 = np.asarray(q, np.float64), np.asarray(k, np.float64)
    a = np.asarray(anc, np.int64).reshape(-1)

    def rows_of(g):
        q0, _, _, nk = g
        j = np.arange(nk)
        beam = a[q0 * ld_anc + j]
        s = k64[beam * tmax + j, 0:64] @ q64[q0, 0:64]
        p = np.exp(s - s.max())
        t = int(np.argmax([p[j0:j0 + 64].sum() for j0 in range(0, nk, 64)]))
        tile = (j >= 64 * t) & (j < 64 * t + 64)
        beam = np.where(tile, (beam + 1) % n_beams, beam)
        return beam * tmax + j
    return attn_ref(q, k, v, groups, heads, anc, ld_anc, tmax, rows_of=rows_of)[0]


# ------------------------------------------------------------------ log-softmax + top-k
def logsumexp64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def topk_ref(logits, k, ban=None, nban=None, larger_index_on_tie=False, mask_bans_in_logz=False):
    """(val [rows][k] float64, idx [rows][k] int64): per row the k largest logits with the row's banned tokens excluded, by value
    descending and the smaller vocabulary index on a tie, as logit - logsumexp(ALL logits, banned included); -inf / -1 past the
    eligible tokens. The two flags give the nearest wrong answers: ties to the larger index, logZ over the unbanned logits."""
    x = np.asarray(logits, np.float64)
    rows, V = x.shape
    val = np.full((rows, k), -np.inf)
    idx = np.full((rows, k), -1, np.int64)
    for r in range(rows):
        keep = np.ones(V, bool)
        if nban is not None:
            b = np.asarray(ban[r][:nban[r]], np.int64)
            keep[b[(b >= 0) & (b < V)]] = False
        logz = logsumexp64(x[r][keep]) if mask_bans_in_logz and keep.any() else logsumexp64(x[r])
        cand = np.nonzero(keep)[0]
        order = np.lexsort((-cand if larger_index_on_tie else cand, -x[r][cand]))[:k]
        idx[r, :len(order)] = cand[order]
        val[r, :len(order)] = x[r][cand[order]] - logz
    return val, idx


def topk_bound(logits):
    """per-row bound of |kernel - float64| for the log-probabilities. The kernel takes fl(x - logZ) with logZ = M + __logf(Z),
    Z = sum over 64 chunks of s_c __expf(m_c - M), s_c = sum of __expf(x - m_c) over a chunk of cs = vocab / 64 logits (256
    threads, cs / 256 terms each, then 6 + 2 tree levels). Rounding of the subtraction and of M + log: 2 U32 (|x| + |logZ|);
    the sums: (cs / 256 + 8 + 64) U32; __expf to 2 ulp of arguments of size <= R = max x - min x: 4 U32 (R + 1); __logf: 4 U32
    (1 + |log Z|). Doubled for the second-order terms."""
    x = np.asarray(logits, np.float64)
    V = x.shape[1]
    cs = -(-V // 64)
    logz = logsumexp64(x)
    R = x.max(1) - x.min(1)
    amax = np.abs(x).max(1)
    lz = np.abs(logz - x.max(1))
    return 2 * U32 * (2 * (amax + np.abs(logz)) + cs / 256 + 72 + 4 * (R + 1) + 4 * (1 + lz))


# ------------------------------------------------------------------ embedding
def embed_ref(E, tok, pos, scale, sinpos):
    """scale * fp16(E)[tok] + sinpos[pos] in float64"""
    e = np.asarray(E, np.float32).astype(np.float16).astype(np.float64)
    return scale * e[np.asarray(tok)] + np.asarray(sinpos, np.float64)[np.asarray(pos)]


def embed_bound(E, tok, pos, scale, sinpos):
    """the kernel's fp32 scale * e + p: two roundings of at most U32 of |scale e| + |p| each"""
    e = np.asarray(E, np.float32).astype(np.float16).astype(np.float64)
    return 2 * U32 * (np.abs(scale * e[np.asarray(tok)]) + np.abs(np.asarray(sinpos, np.float64)[np.asarray(pos)])) + 1e-30


# ------------------------------------------------------------------ inputs shared by the GPU tests and the CPU guard tests
ATTN_NKS = (1, 2, 63, 64, 65, 127, 128, 129, 447, 448, 1000, 1024)
ATTN_PATTERNS = ("rising", "falling", "uniform", "dom0", "dom63", "dom64", "domlast")
# max_nq -> (heads, ldq, ldkv, ldo), the strides as multiples of / offsets to d = 64 heads: fused qkv rows (3d), cross K / V rows
# (2 d L, L = 3), odd widths; both templates (max_nq <= 4: one wave, else four)
ATTN_LAYOUTS = {1: (6, "3d", "3d", "d"), 4: (1, "d", "6d", "d"), 5: (16, "d+64", "d+8", "d+64"), 16: (6, "3d", "6d", "d+64")}
SENTINEL = np.float16(-777.0)


def _ld(spec, d):
    return {"d": d, "3d": 3 * d, "6d": 6 * d, "d+64": d + 64, "d+8": d + 8}[spec]


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def attn_tile_case(pattern, max_nq, seed=0):
    """one launch of every nk in ATTN_NKS (for which the pattern exists) as ragged groups over one packed K / V buffer, nq
    cycling through 1..max_nq, one spare row between groups (the sentinel rows of O). Scores follow the pattern along the
    keys: q_i = (4, small noise), k_j = (pattern_j / 4, noise), so s_j = pattern_j + O(0.3)."""
    heads, lq, lkv, lo = ATTN_LAYOUTS[max_nq]
    d = 64 * heads
    ldq, ldkv, ldo = _ld(lq, d), _ld(lkv, d), _ld(lo, d)
    rng = np.random.default_rng(seed * 1000 + max_nq * 10 + ATTN_PATTERNS.index(pattern))
    groups, q_rows, kv_rows = [], 0, 0
    nks = [nk for nk in ATTN_NKS if {"dom0": 0, "dom63": 63, "dom64": 64}.get(pattern, 0) < nk]
    # every nq of 1..max_nq at least once (the last wave of the four-wave kernel owns rows 12..15), nq = max_nq with nk >= 129
    pairs = [(1 + n % max_nq, nk) for n, nk in enumerate(nks)]
    big = [nk for nk in nks if nk >= 129]
    pairs += [(nq, big[i % len(big)]) for i, nq in enumerate(sorted(set(range(1, max_nq + 1)) - {p[0] for p in pairs}))]
    if not any(nq == max_nq and nk >= 129 for nq, nk in pairs):
        pairs.append((max_nq, big[-1]))
    for nq, nk in pairs:
        groups.append((q_rows + 1, nq, kv_rows, nk))
        q_rows += nq + 1
        kv_rows += nk
    q_rows += 1
    q = rng.uniform(-1000, 1000, (q_rows, ldq))              # columns past the heads: never read
    k = rng.uniform(-1000, 1000, (kv_rows, ldkv))
    v = rng.uniform(-1000, 1000, (kv_rows, ldkv))
    for (q0, nq, k0, nk) in groups:
        x = np.arange(nk) / max(nk - 1, 1)
        pat = {"rising": -3 + 6 * x, "falling": 3 - 6 * x, "uniform": 0.05 * rng.standard_normal(nk)}.get(pattern)
        if pat is None:
            pat = rng.uniform(-0.5, 0.5, nk)
            P = {"dom0": 0, "dom63": 63, "dom64": 64, "domlast": nk - 1}[pattern]
            pat[P] = 4.0
        for h in range(heads):
            c = 64 * h
            q[q0:q0 + nq, c:c + 64] = 0.05 * rng.standard_normal((nq, 64))
            q[q0:q0 + nq, c] = 4.0
            k[k0:k0 + nk, c:c + 64] = rng.standard_normal((nk, 64))
            k[k0:k0 + nk, c] = pat / 4.0
            v[k0:k0 + nk, c:c + 64] = rng.standard_normal((nk, 64))
    o = np.full((q_rows, ldo), SENTINEL, np.float16)
    return dict(q=_f16(q), k=_f16(k), v=_f16(v), o=o, groups=groups, max_nq=max_nq, heads=heads, anc=None, ld_anc=0, tmax=0)


def attn_ancestry_case(t1, seed=0, items=2, beams=5, heads=6, tmax=448):
    """decoder self-attention of items x beams one-row groups over a KV cache [rows][tmax][d] at step t1 - 1: every row's
    ancestry switches beams of its item at tile boundaries (64, 128, ...) and at random keys inside tiles"""
    d = 64 * heads
    rows = items * beams
    rng = np.random.default_rng(seed * 1000 + t1)
    anc = np.full((rows, tmax), -1, np.int32)
    for r in range(rows):
        item = r // beams
        cuts = sorted(set(range(64, t1, 64)) | set(int(c) for c in rng.integers(1, max(t1, 2), size=max(1, t1 // 40))))
        b, j = int(rng.integers(beams)), 0
        for c in cuts + [t1]:
            anc[r, j:c] = item * beams + b
            b = (b + 1 + int(rng.integers(beams - 1))) % beams
            j = c
        anc[r, t1:] = 10 ** 6                              # past nk: never read
    kc = rng.uniform(-1000, 1000, (rows * tmax, d))        # cache positions >= t1: never read
    vc = rng.uniform(-1000, 1000, (rows * tmax, d))
    for r in range(rows):
        kc[r * tmax:r * tmax + t1] = rng.standard_normal((t1, d))
        vc[r * tmax:r * tmax + t1] = rng.standard_normal((t1, d))
    q = 0.3 * rng.standard_normal((rows, 3 * d))           # near-uniform scores (|s| ~ 2)
    groups = [(r, 1, 0, t1) for r in range(rows)]
    o = np.full((rows, d), SENTINEL, np.float16)
    return dict(q=_f16(q), k=_f16(kc), v=_f16(vc), o=o, groups=groups, max_nq=1, heads=heads, anc=anc, ld_anc=tmax, tmax=tmax,
                n_rows=rows)


def attn_wrong_first_row_ancestry(c):
    """every group reads row 0's ancestry (anc[j] instead of anc[q0 * ld_anc + j])"""
    a = np.asarray(c["anc"], np.int64)
    return attn_ref(c["q"], c["k"], c["v"], c["groups"], c["heads"], rows_of=lambda g: a[0, :g[3]] * c["tmax"] + np.arange(g[3]))[0]


TOPK_VOCABS = (16, 80, 2112, 4000, 128112, 262144)
TOPK_KS = (1, 2, 10, 32)


def topk_case(vocab, k, seed=0):
    """logits [rows][vocab] with spreads from +-1 to +-80, ties placed within one thread's stride (i, i + 256), across the waves
    of a chunk (i, i + 64), across chunks (i, i + cs; i, i + 8 cs) and at the row maximum; bans on every other row that include the argmax,
    sit on chunk boundaries, repeat a token, and on row 7 (vocab <= 80) leave k - 1 tokens; rows with nban 0 between them"""
    rng = np.random.default_rng(seed * 100000 + vocab + k)
    rows = 80 if vocab <= 128112 else 16
    cs = -(-vocab // 64)
    spread = np.geomspace(1, 80, rows)
    x = (rng.uniform(-1, 1, (rows, vocab)) * spread[:, None]).astype(np.float32)
    nb_cap = 80
    ban = np.full((rows, nb_cap), -5, np.int32)
    nban = np.zeros(rows, np.int32)
    for r in range(rows):
        top = float(x[r].max())
        pairs = [(i, i + 256) for i in range(0, vocab - 256, max(1, vocab // 7))][:2]
        pairs += [(i, i + 64) for i in range(3, vocab - 64, max(1, vocab // 5))][:2]
        pairs += [(i, i + cs) for i in range(cs // 2, vocab - cs, max(1, vocab // 3))][:2]
        pairs += [(i, i + 8 * cs) for i in range(1, vocab - 8 * cs, max(1, vocab // 2))][:1]   # (one merge thread at k = 32)
        pairs += [(vocab - 1, 0)] if vocab > 1 else []
        for n, (a, b) in enumerate(pairs):
            val = top if (n == len(pairs) - 1 or r % 3 == 0) else top - 0.25 * spread[r] * (n + 1) / 8
            x[r, a] = x[r, b] = np.float32(val)
        if r % 2 == 1:
            am = int(np.argmax(x[r]))
            b = [am, am, cs - 1, cs, (5 * cs) % vocab, vocab - 1] + [int(t) for t in rng.integers(0, vocab, 4)]
            if r == 7 and vocab <= nb_cap:                 # k - 1 eligible tokens (none for k = 1)
                b = [int(t) for t in rng.permutation(vocab)[:vocab - min(k - 1, vocab)]]
            nban[r] = len(b)
            ban[r, :len(b)] = b
    return x, ban, nban, k


EMBED_CASES = ((160, 384, True), (2112, 1024, False))


def embed_case(vocab, d, scale_embedding, max_positions=1024, pad=1, seed=0):
    from .mt_oracle import sinusoidal_table   # (torch)
    rng = np.random.default_rng(seed + vocab)
    E = rng.standard_normal((vocab, d)).astype(np.float32)
    E[pad] = 0.0
    sinpos = sinusoidal_table(max_positions + 2, d, pad).numpy().astype(np.float32)
    tok = np.array([15, 16, 17, vocab - 1, pad, 0, 31, 32, 2, 1000 % vocab], np.int32)
    pos = np.array([2, 3, 4, 5, pad, max_positions + 1, pad, 1000, 2, 17], np.int32)
    scale = np.float32(np.sqrt(d)) if scale_embedding else np.float32(1.0)
    return E, tok, pos, scale, sinpos


# ------------------------------------------------------------------ the row kernels: KV-cache append and ReLU (bit-level, no tolerance)
# (d, rows, tmax, t, wide): d = 64 leaves 248 of the 256 threads idle, 1024 is half a trip, 2048 one trip exactly full, 2056 a second
# trip of one thread; one row and ten; a cache of one slot, of five and of the product's 448 with the first, a middle and the last
# slot; the fused buffer at its product stride 3 d and 8 halfs wider
KV_CASES = tuple((d, rows, tmax, t, wide) for d in (64, 1024, 2048, 2056) for rows in (1, 10)
                 for tmax, ts in ((1, (0,)), (5, (0, 2, 4)), (448, (0, 200, 447))) for t in ts for wide in (False, True))


def _finite_f16_bits(rng, shape):
    """seeded fp16 bit patterns of both signs without inf / NaN (exponent field below 31)"""
    return (rng.integers(0, 0x7c00, size=shape, dtype=np.uint16) | (rng.integers(0, 2, size=shape, dtype=np.uint16) << 15)).astype(np.uint16)


def kv_case(d, rows, tmax, t, wide, seed=0):
    """qkv fp16 [rows][ldqkv]: the K and V thirds seeded normal data with a scale per row and per third, the Q third and the padding
    columns +-1000; Kc / Vc [rows + 1][tmax][d] preset with seeded bit patterns (one spare cache row behind the last appended one)"""
    rng = np.random.default_rng(seed + d + 17 * rows + 31 * tmax + 7 * t + int(wide))
    ld = 3 * d + (8 if wide else 0)
    qkv = rng.choice([-1000.0, 1000.0], size=(rows, ld))
    scale = np.geomspace(0.5, 4.0, rows)[:, None]
    qkv[:, d:2 * d] = rng.standard_normal((rows, d)) * scale
    qkv[:, 2 * d:3 * d] = rng.standard_normal((rows, d)) * scale * 3.0
    cache_rows = rows + 1
    return dict(qkv=_f16(qkv).view(np.uint16), ldqkv=ld, rows=rows, d=d, cache_rows=cache_rows, tmax=tmax, t=t,
                kc=_finite_f16_bits(rng, (cache_rows, tmax, d)), vc=_finite_f16_bits(rng, (cache_rows, tmax, d)))


def kv_append_ref(c, swap=False, dt=0, dr=0, ld=None):
    """(Kc, Vc) uint16 after the append: slot t of cache row r = the K / V third of qkv row r for r < rows, everything else as preset.
    The wrong answers: K and V swapped, slot t + dt, cache row r + dr, the source rows taken at stride `ld` from the flat buffer."""
    d, rows, t = c["d"], c["rows"], c["t"] + dt
    kc, vc = c["kc"].copy(), c["vc"].copy()
    flat = c["qkv"].reshape(-1)
    ld = c["ldqkv"] if ld is None else ld
    for r in range(rows):
        k, v = flat[r * ld + d:r * ld + 2 * d], flat[r * ld + 2 * d:r * ld + 3 * d]
        kc[r + dr, t], vc[r + dr, t] = (v, k) if swap else (k, v)
    return kc, vc


def kv_wrong_answers(c):
    """{name: (Kc, Vc)} of every wrong answer that exists for the case (no slot t - 1 at t = 0, no narrower stride at ldqkv = 3 d,
    and at one row the stride does not matter)"""
    w = {"swap": kv_append_ref(c, swap=True), "row+1": kv_append_ref(c, dr=1)}
    if c["t"] > 0:
        w["t-1"] = kv_append_ref(c, dt=-1)
    if c["t"] + 1 < c["tmax"]:
        w["t+1"] = kv_append_ref(c, dt=1)
    if c["ldqkv"] > 3 * c["d"] and c["rows"] > 1:
        w["ld=3d"] = kv_append_ref(c, ld=3 * c["d"])
    return w


RELU_CASES = ((1, 8, 8), (3, 64, 64), (5, 4096, 4096), (7, 72, 136), (33, 248, 256))      # M N / 8 = 1, 24, 2560, 63, 1023 vectors
# -0.0 first (must come back as +0.0), +-inf, the smallest and the largest subnormal and normal of both signs, +0.0
RELU_SPECIALS = np.array([0x8000, 0x7c00, 0xfc00, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x8400, 0x7bff, 0xfbff, 0x0000], np.uint16)


def relu_case(M, N, ld, seed=0):
    """y uint16 [M][ld]: seeded normal values of both signs in every column, the padding columns N .. ld included (garbage there is
    negative half of the time: a ReLU over them would show); RELU_SPECIALS at the start of row 0 and ending on the last live column of
    the last row (N = 8 holds the first eight: -0.0, the infinities, the subnormals, the smallest positive normal). No NaN: the
    kernel's `v > 0 ? v : 0` maps NaN to 0 where torch.relu keeps it, and no product input is NaN (the FFN's GEMM output is finite)."""
    rng = np.random.default_rng(seed + M + N + ld)
    y = _f16(rng.standard_normal((M, ld)) * 3.0).view(np.uint16).copy()
    k = min(N, len(RELU_SPECIALS))
    y[M - 1, N - k:N] = RELU_SPECIALS[:k][::-1]
    y[0, :k] = RELU_SPECIALS[:k]
    return y


def relu_ref(y, N, keep_negative_zero=False):
    """bit-level ReLU of columns 0 .. N: a set sign bit gives +0.0 (0x0000), everything else (NaN is not among the inputs) is kept"""
    out = y.copy()
    live = out[:, :N]
    neg = (live & 0x8000) != 0
    if keep_negative_zero:
        neg &= live != 0x8000
    live[neg] = 0
    return out


# ------------------------------------------------------------------ the C-ABI hooks (wlx_mt_debug_attn / _topk / _embed / _kv_append / _relu)
def run_kv_append(c, device=0, **over):
    """-> (rc, Kc, Vc) uint16 of one launch_mt_kv_append through wlx_mt_debug_kv_append; `over` replaces scalar arguments (refusals)"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    a = dict(c)
    a.update(over)
    qkv = None if a["qkv"] is None else np.ascontiguousarray(a["qkv"])
    kc = None if a["kc"] is None else np.ascontiguousarray(a["kc"]).copy()
    vc = None if a["vc"] is None else np.ascontiguousarray(a["vc"]).copy()
    rc = lib.wlx_mt_debug_kv_append(device, _ptr(qkv, C.c_uint16), a["ldqkv"], a["rows"], a["d"], _ptr(kc, C.c_uint16), _ptr(vc, C.c_uint16),
                                    a["cache_rows"], a["tmax"], a["t"])
    return rc, kc, vc


def run_relu(y, N, ld=None, M=None, device=0):
    """-> (rc, y uint16 [M][ld]) of one launch_mt_relu_f16 through wlx_mt_debug_relu"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    out = None if y is None else np.ascontiguousarray(y).copy()
    rc = lib.wlx_mt_debug_relu(device, _ptr(out, C.c_uint16), (out.shape[1] if ld is None else ld), (out.shape[0] if M is None else M), N)
    return rc, out



def _ptr(a, t):
    import ctypes as C
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def run_attn(c, device=0):
    """-> (rc, O fp16 [rows][ldo]) of one launch_mt_attn through wlx_mt_debug_attn on the case dict `c`"""
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    q, k, v = (np.ascontiguousarray(c[n]) for n in ("q", "k", "v"))
    o = np.ascontiguousarray(c["o"]).copy()
    g = np.ascontiguousarray(np.asarray(c["groups"], np.int32).reshape(-1, 4))
    anc = None if c["anc"] is None else np.ascontiguousarray(c["anc"], np.int32)
    rc = lib.wlx_mt_debug_attn(device, _ptr(q.view(np.uint16), C.c_uint16), q.shape[1], q.shape[0],
                               _ptr(k.view(np.uint16), C.c_uint16), k.shape[1], _ptr(v.view(np.uint16), C.c_uint16), v.shape[1],
                               k.shape[0], _ptr(g, C.c_int32), len(g), c["max_nq"], c["heads"], _ptr(anc, C.c_int32), c["ld_anc"],
                               c["tmax"], _ptr(o.view(np.uint16), C.c_uint16), o.shape[1], o.shape[0])
    return rc, o


def run_topk(x, k, ban=None, nban=None, device=0):
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x, np.float32)
    rows, V = x.shape
    val = np.zeros((rows, k), np.float32)
    idx = np.zeros((rows, k), np.int32)
    ban = None if ban is None else np.ascontiguousarray(ban, np.int32)
    nban = None if nban is None else np.ascontiguousarray(nban, np.int32)
    rc = lib.wlx_mt_debug_topk(device, _ptr(x, C.c_float), rows, V, _ptr(ban, C.c_int32), _ptr(nban, C.c_int32),
                               0 if ban is None else ban.shape[1], k, _ptr(val, C.c_float), _ptr(idx, C.c_int32))
    return rc, val, idx


def run_embed(E, tok, pos, scale, sinpos, device=0):
    import ctypes as C

    from whisperlive_amd import _lib
    lib = _lib.load()
    E = np.ascontiguousarray(E, np.float32)
    sinpos = np.ascontiguousarray(sinpos, np.float32)
    tok, pos = np.ascontiguousarray(tok, np.int32), np.ascontiguousarray(pos, np.int32)
    x = np.zeros((len(tok), E.shape[1]), np.float32)
    rc = lib.wlx_mt_debug_embed(device, _ptr(E, C.c_float), E.shape[0], E.shape[1], _ptr(tok, C.c_int32), _ptr(pos, C.c_int32),
                                len(tok), float(scale), _ptr(sinpos, C.c_float), sinpos.shape[0], _ptr(x, C.c_float))
    return rc, x
