"""float64 references, case lists and derived bounds of the small softmax kernels of csrc/search.hip that produce the numbers the host
thresholds — token_prob_kernel (no_speech_prob), token_prob_rows_kernel (word probabilities of wlx_align / wlx_align_batch),
lang_probs_kernel (wlx_detect_language) — and the exact references of the data-movement kernels dec_embed_kernel, prep_window_kernel and
f32_to_f16_kernel. Host only (numpy); the run_* functions at the end call the wlx_debug_* hooks and are used by
tests/test_gpu_prob_kernels.py. tests/test_prob_kernel_ref.py shows on these references alone that every case separates the nearest
wrong kernels by more than its bound.

THE BOUND. All three kernels compute, in float32,   p_t = E(l_t - mx) / sum_i E(l_i - mx),   E = __expf, mx = the exact maximum of the
admitted logits (fmaxf is exact), the sum over the admitted ids i. With u = 2^-24 (half an ulp, the relative error of one rounding):

* E. hipcc's own header (lib/clang/<version>/include/__clang_hip_math.h) defines __expf(x) = __builtin_amdgcn_exp2f(log2e_f32 * x) with
  log2e_f32 = 0x1.715476p+0. Neither that header nor any HIP document installed with the toolchain states an accuracy for the
  instruction (v_exp_f32), so the figure is ASSUMED: EXP2_ULPS = 1 ulp = 2u relative, the accuracy the public CDNA instruction-set manuals
  give for V_EXP_F32. The argument x = l - mx is one float32 subtraction (u), the product with the constant one more rounding (u), the
  constant itself is off by KAPPA = |log2e_f32 - log2 e| / log2 e = 1.3e-8; an argument off by a relative d moves 2^y by |y| ln 2 d
  = |x| d. So   eps_E(x) = 2u EXP2_ULPS + |x| (2u + KAPPA)   — it grows with the distance from the maximum.
* The denominator's terms carry eps_E(x_i) each; the sum of positive terms is then off by at most their weighted mean
  sum_i e_i eps_E(x_i) / sum_i e_i, which the reference evaluates (far ids have a large eps_E and no weight).
* Summation. A thread adds its ceil(n / threads) strided terms in order: (ceil(n / threads) - 1) u; the wave butterfly is 6 additions
  deep: 6u; the waves' partial sums are added in order: `waves` u (16 for the 1024-thread kernels, 4 for lang_probs_kernel).
* The division (correctly rounded under hipcc's default, taken as 1 ulp = 2u) and the store: 3u.
With s the sum of these, |p_kernel - p| <= p s / (1 - s) (the usual bound of a product of (1 + eps)^(+-1) factors).
* Underflow. Terms below 2^-126 may be flushed by the instruction; against a sum >= 1 (the maximum contributes E(0) = 1) that is below
  2^-109 relative and is left out. A RESULT at or below FLOOR = 2^-125 may come out as 0, as a denormal or rounded: such elements get the
  absolute FLOOR added (p <= e_t, so the numerator is at least as large as the result: above the floor nothing is flushed).
* A target at -inf, or one the kernel does not admit, is exactly 0: bound 0.
* The beam search computes no_speech_prob itself when the prompt ends on start-of-transcript (search_scan3_kernel, then
  search_merge_update3_kernel), in two levels: a 256-thread workgroup per chunk of 2048 ids sums E(l_i - m_c) over its chunk's own
  maximum m_c — 8 terms per thread: 7u, the wave butterfly 6u, four waves added: 3u —, one wave then adds the chunks as
  s_c E(m_c - mx): the product u, the butterfly 6u. A term's two exponentials cover |l_i - m_c| + |m_c - mx| = |l_i - mx| between them,
  so they carry eps_E(l_i - mx) plus ONE more instruction error, 2u EXP2_ULPS. SCAN3_SUM_U = 7 + 6 + 3 + 1 + 6 + 2 EXP2_ULPS takes the
  place of the summation term; the numerator, the division and the floor are as above.
No constant here was fitted to what a kernel returned."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
EXP2_ULPS = 1.0                                   # ASSUMED accuracy of v_exp_f32, in ulps (see above)
LOG2E_F32 = float(np.float32(1.4426950408889634))  # 0x1.715476p+0, the constant of hipcc's __expf
KAPPA = abs(LOG2E_F32 - math.log2(math.e)) / math.log2(math.e)
FLOOR = 2.0 ** -125
PAD = 1000.0                                      # what the columns past V hold: a read past V is visible
FILL = 1000.0                                     # outputs are pre-filled with +-FILL
VOCABS = (2310, 51864, 51865, 51866)
ROWS = (1, 5, 17)
PATTERNS = ("gauss", "equal", "dominant", "argmax", "smallest", "third_inf", "target_inf")
LANG_NS = (1, 99, 100, 256)                       # 256 = WLX_LANG_MAX, the largest n the launch is given
LANG_MAX = 256
SR_THREADS, SR_WAVES = 1024, 16                   # token_prob_kernel, token_prob_rows_kernel
LP_THREADS, LP_WAVES = 256, 4                     # lang_probs_kernel
SCAN3_SUM_U = 7 + 6 + 3 + 1 + 6 + 2 * EXP2_ULPS   # search_scan3_kernel + search_merge_update3_kernel (see above), in units of u
GUARD = 64                                        # WLX_DEBUG_GUARD: words behind the last owned output word that travel with it
FRACS = (0.012, 0.02, 0.031, 0.045, 0.017, 0.026, 0.038)   # mass of a planted id: >= 1 %, neighbours in id and in row differ


def eot_of(V):
    """the end-of-text id of the Whisper layout scaled to V (tests/helpers.py token_ids_for: 50256 / 50257 for 51864 / 51865)"""
    return V - 1608


def ldl_of(V):
    return V + 11                                  # > V, odd: nothing in the kernels may lean on an aligned row


def eps_exp(x):
    return 2 * U * EXP2_ULPS + np.abs(x) * (2 * U + KAPPA)


def softmax_ref(buf, stride, rows, sel, targets, threads, waves, admit=None, row_map=None, sum_u=None):
    """p [rows][k] and its bound [rows][k]: row r is buf[row_map(r) * stride ...], the admitted ids are `sel` (an int: the prefix
    [0, sel); or an index array), `targets` [rows][k] the ids asked for; with admit = A a target outside [0, A) gives exactly 0, with
    admit = None the word at the target's place is read whatever it is (a mutant that reads a pad column gets the pad)."""
    buf = np.asarray(buf, np.float64)
    targets = np.asarray(targets, np.int64).reshape(rows, -1)
    p = np.zeros(targets.shape)
    b = np.zeros(targets.shape)
    n = sel if np.isscalar(sel) else len(sel)
    s_sum = ((math.ceil(n / threads) - 1 + 6 + waves) if sum_u is None else sum_u) * U + 3 * U
    for r in range(rows):
        base = (r if row_map is None else row_map(r)) * stride
        l = buf[base:base + sel] if np.isscalar(sel) else buf[base + np.asarray(sel, np.int64)]
        mx = l.max()
        with np.errstate(invalid="ignore", over="ignore"):
            x = mx - l
            e = np.exp(-x)
            S = e.sum()
            den = float(np.where(e > 0, e * eps_exp(np.where(e > 0, x, 0.0)), 0.0).sum() / S)
            for k, t in enumerate(targets[r]):
                if admit is not None and not (0 <= t < admit):
                    continue
                if base + t < 0 or base + t >= buf.size:
                    p[r, k] = np.nan                                   # (a mutant's read outside the buffer: no statement)
                    continue
                lt = buf[base + t]
                if lt == -np.inf:
                    continue
                xt = mx - lt
                p[r, k] = np.exp(-xt) / S
                s = float(eps_exp(xt)) + den + s_sum
                b[r, k] = p[r, k] * s / (1 - s) + (FLOOR if p[r, k] <= FLOOR else 0.0)
    return p, b


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (> 1: outside the bound); a zero bound asks for equality; inf when anything is not finite"""
    got, ref, bound = (np.asarray(a, np.float64).ravel() for a in (got, ref, bound))
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    z = bound == 0
    if (d[z] > 0).any():
        return float("inf")
    return float((d[~z] / bound[~z]).max()) if (~z).any() else 0.0


# ------------------------------------------------------------------ logits
def _lse(v):
    v = v[np.isfinite(v)]
    m = v.max()
    return m + math.log(np.exp(v - m).sum())


def plant(row, ids, r, among=None, first_frac=None):
    """give each of `ids` a stated share (FRACS, by row and place; the first one first_frac if given) of the final mass over `among`
    (default: the whole row)"""
    ids = list(dict.fromkeys(int(i) for i in ids))
    fr = [FRACS[(r + k) % len(FRACS)] for k in range(len(ids))]
    if first_frac is not None:
        fr[0] = first_frac
    rest = np.ones(row.size, bool) if among is None else np.isin(np.arange(row.size), among)
    rest[ids] = False
    L = _lse(row[rest]) if rest.any() and np.isfinite(row[rest]).any() else 0.0
    for i, f in zip(ids, fr):
        row[i] = L + math.log(f / (1 - sum(fr)))


def top_frac(r):
    """the share of an arg-max target: well above every other planted id, and another one in the neighbouring row"""
    return 0.3 + 0.05 * (r % 3)


def base_row(V, pattern, rng, r):
    if pattern == "equal":
        return np.full(V, r - 3.0)
    if pattern == "dominant":
        row = np.full(V, -80.0)
        row[(977 * (r + 1)) % (V - 1700)] = 80.0                       # (never one of the planted ids, which sit at the edges)
        return row
    row = rng.standard_normal(V) * 4.0
    if pattern == "third_inf":
        row[1::3] = -np.inf
    return row


def finish_row(row, pattern, target, r):
    """what a pattern does to its target once the shares are planted. "target_inf" takes every second row only, so that the
    neighbouring row answers something else than 0."""
    if pattern == "argmax":                        # no Gaussian outlier above the target (the planted neighbours sit ln(0.3 / 0.045) below it)
        over = row > row[target] - 1.0
        over[target] = False
        row[over] = row[target] - 1.0
    if pattern == "smallest":
        row[target] = row[np.isfinite(row)].min() - 1.0
    if pattern == "target_inf" and r % 2 == 0:
        row[target] = -np.inf


def _pack(rows_list, V):
    ldl = ldl_of(V)
    buf = np.full((len(rows_list), ldl), PAD, np.float32)
    for r, row in enumerate(rows_list):
        buf[r, :V] = row.astype(np.float32)
    return buf.ravel(), ldl


def case_list():
    """(V, rows, pattern): every vocabulary x every row count on Gaussian logits, every pattern x every vocabulary at 5 rows"""
    out = [(V, rows, "gauss") for V in VOCABS for rows in ROWS]
    out += [(V, 5, p) for V in VOCABS for p in PATTERNS if p != "gauss"]
    return out


TP_CASES = case_list()
TPR_CASES = case_list()
LP_CASES = ([(V, 5, "gauss", n) for V in VOCABS for n in LANG_NS] + [(51865, rows, "gauss", 99) for rows in (1, 17)] +
            [(51865, 5, p, n) for p in PATTERNS if p != "gauss" for n in (100, 256)] + [(2310, 17, "third_inf", 99)])


def tp_tok(V, rows, pattern):
    """the one id of a token_prob launch: the no-speech id of the layout, the first and the last id, taken in turn over the cases"""
    if pattern in ("smallest", "target_inf"):      # (a target without mass at V - 1 would BE the one-fewer mutant's id, and hide it)
        return V - 1503
    return (V - 1503, 0, V - 1)[(ROWS.index(rows) + PATTERNS.index(pattern)) % 3]


def tp_case(V, rows, pattern):
    tok = tp_tok(V, rows, pattern)
    rng = np.random.default_rng([V, rows, PATTERNS.index(pattern), 1])
    out = []
    for r in range(rows):
        row = base_row(V, pattern, rng, r)
        if pattern != "equal":
            ids = [tok] + [t for t in (tok - 1, tok + 1, V - 1, V - 2) if 0 <= t < V]
            plant(row, ids, r, first_frac=top_frac(r) if pattern == "argmax" else None)
            finish_row(row, pattern, tok, r)
        out.append(row)
    buf, ldl = _pack(out, V)
    return dict(V=V, rows=rows, pattern=pattern, tok=tok, buf=buf, ldl=ldl)


TPR_TARGETS = ("0", "vlim-1", "-1", "vlim", "V-1")


def tpr_targets(V, rows, k):
    vlim = eot_of(V)
    t = dict(zip(TPR_TARGETS, (0, vlim - 1, -1, vlim, V - 1)))
    return np.asarray([t[TPR_TARGETS[(r + k) % 5]] for r in range(rows)], np.int32)


def tpr_shifts(rows, pattern="gauss"):
    """the rotations of the five targets a case launches: one launch covers them from five rows on; all five where there is one row,
    and where a pattern shapes id 0 — every row then asks for the shaped id once"""
    return range(5) if rows < 5 or pattern != "gauss" else range(1)


def tpr_case(V, rows, pattern):
    vlim = eot_of(V)
    rng = np.random.default_rng([V, rows, PATTERNS.index(pattern), 2])
    out = []
    for r in range(rows):
        row = base_row(V, pattern, rng, r)
        if pattern != "equal":
            # both in-range targets with their neighbours, the last admitted id, the first id left out (end-of-text) and the last id
            plant(row, [0, vlim - 1, 1, vlim - 2, vlim, V - 1], r, first_frac=top_frac(r) if pattern == "argmax" else None)
            finish_row(row, pattern, 0, r)         # (the pattern's target is id 0: vlim - 1 keeps its share, it is the one-fewer mutant's id)
        out.append(row)
    buf, ldl = _pack(out, V)
    return dict(V=V, vlim=vlim, rows=rows, pattern=pattern, buf=buf, ldl=ldl)


def lp_case(V, rows, pattern, n):
    rng = np.random.default_rng([V, rows, PATTERNS.index(pattern), n, 3])
    perm = rng.permutation(np.arange(V - 1700, V))
    ids, extra = perm[:n].astype(np.int32), int(perm[n])              # unsorted, in the last 1700 columns; `extra`: the one-more-id mutant's
    assert (np.diff(ids) < 0).any() or n == 1
    out = []
    among = np.concatenate([ids, [extra]])
    for r in range(rows):
        row = base_row(V, pattern, rng, r)
        if pattern == "dominant":
            row[:] = -80.0
            row[ids[n // 2]] = 80.0
        if pattern != "equal":
            planted = [ids[0], ids[n - 1], extra] if n > 1 else [ids[0], extra]
            plant(row, planted, r, among=among, first_frac=top_frac(r) if pattern == "argmax" else None)
            if n > 1:
                finish_row(row, pattern, int(ids[0]), r)
        out.append(row)
    buf, ldl = _pack(out, V)
    return dict(V=V, rows=rows, pattern=pattern, n=n, ids=ids, extra=extra, buf=buf, ldl=ldl)


def tp_ref(c, **kw):
    a = dict(stride=c["ldl"], sel=c["V"], targets=np.full((c["rows"], 1), c["tok"]), admit=c["V"])
    a.update(kw)
    p, b = softmax_ref(c["buf"], a["stride"], c["rows"], a["sel"], a["targets"], SR_THREADS, SR_WAVES, a["admit"], a.get("row_map"))
    return p[:, 0], b[:, 0]


def tpr_ref(c, toks, **kw):
    a = dict(stride=c["ldl"], sel=c["vlim"], targets=np.asarray(toks).reshape(-1, 1), admit=c["vlim"])
    a.update(kw)
    p, b = softmax_ref(c["buf"], a["stride"], c["rows"], a["sel"], a["targets"], SR_THREADS, SR_WAVES, a["admit"], a.get("row_map"))
    return p[:, 0], b[:, 0]


def lp_ref(c, **kw):
    a = dict(stride=c["ldl"], sel=c["ids"], targets=np.tile(c["ids"], (c["rows"], 1)), admit=None)
    a.update(kw)
    return softmax_ref(c["buf"], a["stride"], c["rows"], a["sel"], a["targets"], LP_THREADS, LP_WAVES, a["admit"], a.get("row_map"))


def neighbour(rows):
    return lambda r: r + 1 if r + 1 < rows else r - 1


# ------------------------------------------------------------------ the exact kernels
def f16_bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def embed_ref(tok_emb16, pos_emb, tokens, pos):
    """x[r] = float32(tok_emb[tokens[r]]) + pos_emb[pos[r]]: the fp16 value is exact in float32, the sum is ONE float32 rounding"""
    return tok_emb16[tokens].astype(np.float32) + pos_emb[pos]


EMBED_CASES = [(rows, d) for rows in (1, 5, 64) for d in (384, 1280)]
EMBED_V, EMBED_NPOS = 2310, 448


def embed_case(rows, d):
    rng = np.random.default_rng([rows, d, 4])
    te = (rng.standard_normal((EMBED_V, d)) * 0.5).astype(np.float16)
    pe = (rng.standard_normal((EMBED_NPOS, d)) * 0.3).astype(np.float32)
    tokens = rng.integers(0, EMBED_V, rows).astype(np.int32)
    pos = rng.integers(0, EMBED_NPOS, rows).astype(np.int32)
    edge = [(0, 0), (EMBED_V - 1, 447), (0, 447), (EMBED_V - 1, 0), (EMBED_V - 1, 447)]     # first / last token and position; the last pair twice
    for r in range(min(rows, len(edge))):
        tokens[rows - 1 - r], pos[rows - 1 - r] = edge[r] if rows > 1 else (EMBED_V - 1, 447)
    if rows > 5:
        tokens[3] = tokens[9] = tokens[10]                             # duplicate tokens in a launch, at different positions
    return dict(rows=rows, d=d, te=te, pe=pe, tokens=tokens, pos=pos)


N_FRAMES = 3000
PREP_WINDOWS = ((0, 3000), (1000, 2700), (0, 1), (0, 31), (0, 33), (123, 2999))
PREP_CASES = [(nm, items, w0) for nm in (80, 128) for items, w0 in ((1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (3, 0), (3, 3))]


def prep_case(n_mels, items, w0):
    """items windows PREP_WINDOWS[w0 ...] (cyclic); the feature matrices [n_mels][ld] sit item_stride apart with item_stride larger
    than the matrix; values over the range the log-mel produces ((log10 + 4) / 4 clamped 8 decades below the maximum: about -1 .. 2)"""
    rng = np.random.default_rng([n_mels, items, w0, 5])
    wins = [PREP_WINDOWS[(w0 + i) % len(PREP_WINDOWS)] for i in range(items)]
    ld = 3704                                                          # >= seek + seg of every window, not a multiple of 32
    item_stride = n_mels * ld + 52
    feats = np.full(items * item_stride, 7.5, np.float32)              # (the gaps hold a value no window may show)
    for i in range(items):
        m = rng.uniform(-1.0, 2.0, (n_mels, ld)).astype(np.float32)
        m[:, ::97] = np.float32(2.0 ** -15) * rng.uniform(0.01, 1.0, m[:, ::97].shape).astype(np.float32)     # fp16 subnormals
        m[0, :8] = np.asarray([0.0, -0.0, 1.00048828125, 1.00146484375, -0.99951171875, 2.0, -1.0, 0.333251953125 + 2.0 ** -13], np.float32)  # ties
        feats[i * item_stride:i * item_stride + n_mels * ld] = m.ravel()
    stride_T = (N_FRAMES + 2) * n_mels + 64
    return dict(n_mels=n_mels, items=items, ld=ld, item_stride=item_stride, feats=feats, featT_stride=stride_T,
                seek=np.asarray([w[0] for w in wins], np.int32), seg=np.asarray([w[1] for w in wins], np.int32))


def prep_ref(c, init):
    """the expected bits of featT given its initial bits `init` (uint16 [items * featT_stride])"""
    out = init.copy()
    nm = c["n_mels"]
    for i in range(c["items"]):
        m = c["feats"][i * c["item_stride"]:i * c["item_stride"] + nm * c["ld"]].reshape(nm, c["ld"])
        w = np.zeros((N_FRAMES, nm), np.float16)
        sk, sg = int(c["seek"][i]), int(c["seg"][i])
        w[:sg] = m[:, sk:sk + sg].T.astype(np.float16)
        o = i * c["featT_stride"]
        out[o + nm:o + (N_FRAMES + 1) * nm] = w.view(np.uint16).ravel()
    return out


F16_NS = (1, 255, 256, 257)


def f16_values(n):
    """float32 values through the fp16 normal, subnormal and overflow ranges, ties and specials first"""
    rng = np.random.default_rng([n, 6])
    special = np.asarray([65504.0, 0.0, -0.0, 65519.9, 65520.0, -65520.0, 1e30, -1e30, np.inf, -np.inf, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                          2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 1.00048828125, 1.00146484375, 3.0 * 2.0 ** -25, 1e-10, -1e-10], np.float32)
    v = (np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-27, 18, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    k = min(n, special.size)
    v[:k] = special[:k]
    return v


# ------------------------------------------------------------------ the hooks
def _lib():
    from whisperlive_amd import _lib as L
    return L.load()


def _p(a, ct, name=None, null=()):
    """the array's address as a `ct` pointer; None (a null pointer) when the argument `name` is among `null`"""
    import ctypes as C
    return None if name in null else a.ctypes.data_as(C.POINTER(ct))


def _filled(n, dtype=np.float32):
    a = np.full(n, FILL, dtype)
    a[1::2] = -FILL
    return a


def run_tp(c, null=(), **over):
    """-> rc, out [rows + GUARD], its initial bytes; `over` replaces scalar arguments, `null` names pointers passed as null"""
    import ctypes as C
    a = dict(ldl=c["ldl"], V=c["V"], rows=c["rows"], tok=c["tok"])
    a.update(over)
    out = _filled(c["rows"] + GUARD)
    init = out.copy()
    rc = _lib().wlx_debug_token_prob(0, _p(c["buf"], C.c_float, "logits", null), a["ldl"], a["V"], a["rows"], a["tok"],
                                     _p(out, C.c_float, "out", null))
    return rc, out, init


def run_tpr(c, toks, null=(), **over):
    import ctypes as C
    a = dict(ldl=c["ldl"], vlim=c["vlim"], rows=c["rows"])
    a.update(over)
    toks = np.ascontiguousarray(toks, np.int32)
    out = _filled(c["rows"] + GUARD)
    init = out.copy()
    rc = _lib().wlx_debug_token_prob_rows(0, _p(c["buf"], C.c_float, "logits", null), a["ldl"], a["vlim"], a["rows"],
                                          _p(toks, C.c_int32, "toks", null), _p(out, C.c_float, "out", null))
    return rc, out, init


def run_lp(c, null=(), **over):
    import ctypes as C
    a = dict(ldl=c["ldl"], rows=c["rows"], n=c["n"])
    a.update({k: v for k, v in over.items() if k in a})
    ids = np.ascontiguousarray(over.get("ids", c["ids"]), np.int32)
    out = _filled(c["rows"] * c["n"] + GUARD)
    init = out.copy()
    rc = _lib().wlx_debug_lang_probs(0, _p(c["buf"], C.c_float, "logits", null), a["ldl"], a["rows"], _p(ids, C.c_int32, "ids", null),
                                     a["n"], _p(out, C.c_float, "probs", null))
    return rc, out, init


def run_embed(c, null=(), **over):
    import ctypes as C
    a = dict(vocab=EMBED_V, n_pos=EMBED_NPOS, d=c["d"], rows=c["rows"])
    a.update({k: v for k, v in over.items() if k in a})
    tokens = np.ascontiguousarray(over.get("tokens", c["tokens"]), np.int32)
    pos = np.ascontiguousarray(over.get("pos", c["pos"]), np.int32)
    x = _filled(c["rows"] * c["d"])
    intok = _filled(c["rows"] * 448, np.int32)
    init = (x.copy(), intok.copy())
    rc = _lib().wlx_debug_dec_embed(0, _p(c["te"].view(np.uint16), C.c_uint16, "tok_emb", null), a["vocab"],
                                    _p(c["pe"], C.c_float, "pos_emb", null), a["n_pos"], a["d"], _p(tokens, C.c_int32, "tokens", null),
                                    _p(pos, C.c_int32, "pos", null), a["rows"], _p(x, C.c_float, "x", null),
                                    _p(intok, C.c_int32, "intok", null))
    return rc, x, intok, init


def run_prep(c, null=(), **over):
    import ctypes as C
    a = dict(feats_len=c["feats"].size, ld=c["ld"], n_mels=c["n_mels"], item_stride=c["item_stride"], items=c["items"],
             featT_stride=c["featT_stride"])
    a.update({k: v for k, v in over.items() if k in a})
    seek = np.ascontiguousarray(over.get("seek", c["seek"]), np.int32)
    seg = np.ascontiguousarray(over.get("seg", c["seg"]), np.int32)
    out = _filled(c["items"] * c["featT_stride"], np.float16).view(np.uint16)
    init = out.copy()
    rc = _lib().wlx_debug_prep_windows(0, _p(c["feats"], C.c_float, "feats", null), a["feats_len"], a["ld"], a["n_mels"], a["item_stride"],
                                       a["items"], _p(seek, C.c_int32, "seek", null), _p(seg, C.c_int32, "seg", null),
                                       _p(out, C.c_uint16, "featT", null), a["featT_stride"])
    return rc, out, init


def run_f16(src, n, cap, alloc=None, null=()):
    import ctypes as C
    out = _filled(alloc or cap, np.float16).view(np.uint16)
    init = out.copy()
    rc = _lib().wlx_debug_f32_to_f16(0, _p(src, C.c_float, "src", null), n, _p(out, C.c_uint16, "dst", null), cap)
    return rc, out, init
