"""Host-only: on the float64 references of tests/prob_kernel_ref.py alone, every case of the GPU module separates the nearest wrong
kernels by MORE than the bound the GPU test grants — a kernel with one of these faults cannot pass tests/test_gpu_prob_kernels.py:
  the denominator with one more id / one fewer id; the denominator over V in place of vlim (word probabilities); normalisation over the
  whole row in place of the ids (language probabilities); the target id off by one; the row stride V in place of ldl; the neighbouring row.
The ids in question carry at least 1 % of the mass (asserted), so none of this hangs on the last digits. What a case cannot separate
by construction is named where it is left out:
  * "equal" is invariant under any permutation of ids and rows (its point is p = 1 / n): only the denominators and, where the row
    reaches the pad, the row stride move it; a list of one language id is p = 1 in whatever row;
  * a result that is exactly 0 (a target at -inf or one that is not admitted) stays 0 under every denominator;
  * with one row there is no neighbouring row and no stride."""
import numpy as np
import pytest

from . import prob_kernel_ref as R


def _separated(ref, bound, mut, rows=None):
    """per element: the mutant's answer lies outside the reference's bound (an unread place — nan — makes no statement)"""
    ok = np.abs(mut - ref) > bound
    ok &= ~np.isnan(mut)
    return ok if rows is None else ok[rows]


def test_constants():
    assert R.KAPPA < 2e-8 and R.LOG2E_F32 == float.fromhex("0x1.715476p+0")
    assert R.eps_exp(0.0) == 2 * R.U * R.EXP2_ULPS and R.eps_exp(160.0) < 3e-5
    assert min(R.FRACS) >= 0.01 and len(set(R.FRACS)) == len(R.FRACS)
    assert [R.eot_of(V) for V in (51864, 51865)] == [50256, 50257]
    for cases in (R.TP_CASES, R.TPR_CASES):
        assert {c[0] for c in cases} == set(R.VOCABS) and {c[1] for c in cases} == set(R.ROWS) and {c[2] for c in cases} == set(R.PATTERNS)
    assert {c[3] for c in R.LP_CASES} == set(R.LANG_NS) and {c[0] for c in R.LP_CASES} == set(R.VOCABS)
    assert {c[1] for c in R.LP_CASES} == set(R.ROWS) and {c[2] for c in R.LP_CASES} == set(R.PATTERNS)
    toks = {R.tp_tok(*c) - c[0] for c in R.TP_CASES}
    assert toks >= {-1503, -1} and 0 in {R.tp_tok(*c) for c in R.TP_CASES}


def _mass(c, r, ids, sel):
    row = c["buf"].reshape(c["rows"], c["ldl"])[r].astype(np.float64)
    l = row[:sel] if np.isscalar(sel) else row[np.asarray(sel)]
    e = np.exp(row[np.asarray(ids)] - l.max())
    return e / np.exp(l - l.max()).sum()


@pytest.mark.parametrize("case", R.TP_CASES, ids=lambda c: "V%d-r%d-%s" % c)
def test_token_prob_mutants(case):
    c = R.tp_case(*case)
    V, rows, pat, tok = c["V"], c["rows"], c["pattern"], c["tok"]
    ref, b = R.tp_ref(c)
    assert np.isfinite(ref).all() and (b >= 0).all()
    buf2 = c["buf"].reshape(rows, -1)
    assert (buf2[:, V:] == R.PAD).all() and c["ldl"] > V
    zero = ref == 0
    assert (zero == ((pat == "target_inf") & (np.arange(rows) % 2 == 0))).all() and (ref[~zero] > R.FLOOR).all()
    live = ~zero
    if pat == "equal":
        np.testing.assert_allclose(ref, 1.0 / V, rtol=1e-12)
    else:
        for r in range(rows):
            ids = [t for t in (tok - 1, tok + 1, V - 1) if 0 <= t < V and t != tok]
            assert (_mass(c, r, ids, V) >= 0.01).all(), (r, ids)
        if pat in ("gauss", "dominant", "third_inf", "argmax"):
            assert (ref >= 0.01).all()
    if pat == "argmax":
        assert all(int(np.argmax(buf2[r, :V])) == tok for r in range(rows))
    if pat == "smallest":
        assert all(buf2[r, tok] == buf2[r, :V][np.isfinite(buf2[r, :V])].min() for r in range(rows))
    assert _separated(ref, b, R.tp_ref(c, sel=V + 1)[0], live).all()         # one more id: the pad column (0 stays 0 under any denominator)
    assert _separated(ref, b, R.tp_ref(c, sel=V - 1)[0], live).all()         # one fewer id
    if pat != "equal":
        for dt in (-1, 1):
            if 0 <= tok + dt < V:
                assert _separated(ref, b, R.tp_ref(c, targets=np.full((rows, 1), tok + dt), admit=None)[0]).all(), dt
        if rows > 1:
            assert _separated(ref, b, R.tp_ref(c, row_map=R.neighbour(rows))[0]).all()
    if rows > 1:
        assert _separated(ref, b, R.tp_ref(c, stride=V, admit=None)[0], live & (np.arange(rows) > 0)).all()   # row 0 starts at the same word


@pytest.mark.parametrize("case", R.TPR_CASES, ids=lambda c: "V%d-r%d-%s" % c)
def test_token_prob_rows_mutants(case):
    c = R.tpr_case(*case)
    V, vlim, rows, pat = c["V"], c["vlim"], c["rows"], c["pattern"]
    seen = set()
    for k in R.tpr_shifts(rows, pat):
        toks = R.tpr_targets(V, rows, k)
        seen |= set(toks.tolist())
        ref, b = R.tpr_ref(c, toks)
        inr = (toks >= 0) & (toks < vlim)
        assert (ref[~inr] == 0).all() and (b[~inr] == 0).all()               # -1, vlim and V - 1: exactly 0
        live = inr & (ref > 0)
        assert (live == (inr & ~((pat == "target_inf") & (toks == 0) & (np.arange(rows) % 2 == 0)))).all() and (ref[live] > R.FLOOR).all()
        if pat == "equal":
            np.testing.assert_allclose(ref[inr], 1.0 / vlim, rtol=1e-12)
        else:
            for r in range(rows):
                assert (_mass(c, r, [1, vlim - 2, vlim - 1, vlim, V - 1], vlim) >= 0.01).all() or pat in ("smallest", "target_inf")
                assert (_mass(c, r, [1, vlim - 2, vlim, V - 1], vlim) >= 0.01).all()
        for sel in (vlim + 1, vlim - 1, V):                                   # one more id (end-of-text), one fewer, the whole vocabulary
            assert _separated(ref, b, R.tpr_ref(c, toks, sel=sel)[0], live).all(), sel
        if pat != "equal":
            up = R.tpr_ref(c, toks + 1)[0]
            dn = R.tpr_ref(c, toks - 1)[0]
            # every in-range target: both directions; -1 and vlim: the direction that lands on an admitted id (V - 1 has none: its
            # neighbours are no text either — what it pins is the admission test, through the exact 0)
            # (id 0 at -inf answers 0 like the id -1 below it: that row has the upward direction only)
            assert (_separated(ref, b, up, inr) & (_separated(ref, b, dn, inr) | ~live[inr])).all()
            inf0 = np.isneginf(c["buf"].reshape(rows, -1)[:, 0])                  # ("target_inf": id 0 answers 0 like the id below it)
            assert _separated(ref, b, up, (toks == -1) & ~inf0).all() and _separated(ref, b, dn, toks == vlim).all()
            if rows > 1:
                nb = R.tpr_ref(c, toks, row_map=R.neighbour(rows))[0]
                assert _separated(ref, b, nb, live).all()
        if rows > 1:
            st = R.tpr_ref(c, toks, stride=V)[0]
            assert _separated(ref, b, st, live & (np.arange(rows) > 0)).all()
    assert seen == {0, vlim - 1, -1, vlim, V - 1}


@pytest.mark.parametrize("case", R.LP_CASES, ids=lambda c: "V%d-r%d-%s-n%d" % c)
def test_lang_probs_mutants(case):
    c = R.lp_case(*case)
    V, rows, pat, n, ids = c["V"], c["rows"], c["pattern"], c["n"], c["ids"]
    assert ids.min() >= V - 1700 and ids.max() < V and len(set(ids.tolist())) == n and n <= R.LANG_MAX
    ref, b = R.lp_ref(c)
    assert np.isfinite(ref).all()
    np.testing.assert_allclose(ref.sum(1), 1.0, rtol=1e-12)
    live = ref > R.FLOOR                                                      # (below it the bound is the floor itself: no statement)
    assert live.any(1).all()
    if pat == "equal":
        np.testing.assert_allclose(ref, 1.0 / n, rtol=1e-12)
    else:
        for r in range(rows):
            assert (_mass(c, r, [ids[n - 1], c["extra"]], ids) >= 0.01).all()
    more = R.lp_ref(c, sel=np.concatenate([ids, [c["extra"]]]))[0]
    assert _separated(ref, b, more, live).all()
    if n > 1:
        fewer = R.lp_ref(c, sel=ids[:-1])[0]
        assert _separated(ref, b, fewer, live).all()
    whole = R.lp_ref(c, sel=V)[0]
    assert _separated(ref, b, whole, live).all()
    assert (1.0 - whole.sum(1) >= 0.01).all()                                 # the ids outside the list hold at least 1 % of the row
    if pat != "equal":
        for dt in (-1, 1):
            off = R.lp_ref(c, targets=np.tile(ids + dt, (rows, 1)))[0]
            assert _separated(ref, b, off).any(1).all(), dt                  # some element of every row
        if rows > 1 and n > 1:                                                # (a single id is p = 1 in every row)
            nb = R.lp_ref(c, row_map=R.neighbour(rows))[0]
            assert _separated(ref, b, nb).any(1).all()
    if rows > 1 and n > 1 and pat != "equal":                                 # (the ids sit far from the pad: equal rows stay equal)
        st = R.lp_ref(c, stride=V)[0]
        assert _separated(ref, b, st)[1:].any(1).all()


def test_bound_shape():
    """the bound grows with the distance from the maximum and with the terms per thread, and floors where float32 underflows"""
    V = 2310
    buf = np.full(R.ldl_of(V), R.PAD, np.float32)
    buf[:V] = -80.0
    buf[5] = 80.0
    buf[7] = 79.0
    p, b = R.softmax_ref(buf, R.ldl_of(V), 1, V, [[5, 7, 9]], R.SR_THREADS, R.SR_WAVES, admit=V)
    assert p[0, 2] < R.FLOOR and b[0, 2] >= R.FLOOR and b[0, 2] < 2 * R.FLOOR
    assert b[0, 1] / p[0, 1] > b[0, 0] / p[0, 0] > 0
    lo = (3 - 1 + 6 + 16 + 3 + 2) * R.U
    assert lo <= b[0, 0] / p[0, 0] < lo * 1.2
    p2, b2 = R.softmax_ref(buf, R.ldl_of(V), 1, V, [[5]], 64, 1, admit=V)
    assert b2[0, 0] > b[0, 0]
    p3, b3 = R.softmax_ref(buf, R.ldl_of(V), 1, V, [[5]], 1, 0, admit=V, sum_u=R.SCAN3_SUM_U)
    assert R.SCAN3_SUM_U == 25 and (25 + 3 + 2 + 2) * R.U < b3[0, 0] / p3[0, 0] < (25 + 3 + 2 + 3) * R.U    # + numerator 2u + denominator 2u .. 3u
    assert R.excess([0.0, 1.0], [0.0, 1.0], [0.0, 0.0]) == 0.0 and R.excess([1e-30], [0.0], [0.0]) == float("inf")
    assert R.excess([np.nan], [0.0], [1.0]) == float("inf")


def test_exact_references():
    c = R.embed_case(64, 384)
    assert c["tokens"][3] == c["tokens"][9] == c["tokens"][10] and {0, R.EMBED_V - 1} <= set(c["tokens"].tolist())
    assert {0, 447} <= set(c["pos"].tolist())
    x = R.embed_ref(c["te"], c["pe"], c["tokens"], c["pos"])
    assert x.dtype == np.float32 and x.shape == (64, 384)
    p = R.prep_case(80, 3, 3)
    init = np.full(3 * p["featT_stride"], 0x63D0, np.uint16)
    out = R.prep_ref(p, init)
    for i in range(3):
        w = out[i * p["featT_stride"]:(i + 1) * p["featT_stride"]]
        assert (w[:80] == 0x63D0).all() and (w[3001 * 80:] == 0x63D0).all()          # rows 0 and 3001, and the gap behind them
        seg = int(p["seg"][i])
        assert (w[(1 + seg) * 80:3001 * 80] == 0).all()                              # frames seg <= t < 3000 are zero
        assert (w[80:(1 + seg) * 80] != 0).any()
    assert p["item_stride"] > 80 * p["ld"] and [tuple(w) for w in zip(p["seek"], p["seg"])] == [(0, 31), (0, 33), (123, 2999)]
    with np.errstate(over="ignore"):
        v = R.f16_values(257)
        h = v.astype(np.float16)
    assert np.isinf(h[np.abs(v) >= 65520]).all() and h[0] == 65504 and (np.abs(h[np.isfinite(h)]) <= 65504).all()
    assert ((h != 0) & (np.abs(h) < 2.0 ** -14)).any() and np.isinf(h).any()
