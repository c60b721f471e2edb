"""CPU guard of tests/whisper_kernel_ref.py, for every case the GPU tests run (tests/test_gpu_whisper_kernels.py): the float64
reference is inside its own bound, an fp32 computation in another association stays inside it (the bound is not so tight that a
correct kernel fails), and every wrong answer that exists for the case leaves it on at least one element (the bound is not so loose
that a broken kernel passes). The packer and the unpacker of the tile-packed cross K / V invert each other. No hook is called."""
import numpy as np
import pytest

from . import whisper_kernel_ref as R


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("d", R.LN_DS)
def test_layernorm_bounds_hold_and_exclude_the_wrong_answers(d):
    for M in R.LN_MS:
        c = R.ln_case(d, M)
        x = c["x"][:, :d]
        ref = R.ln_ref(x, c["gamma"], c["beta"])
        e32, b16 = R.ln_bound(x, c["gamma"], c["beta"])
        assert R.excess(ref, ref, e32) == 0.0
        emu = R.ln_emulate32(x, c["gamma"], c["beta"])
        assert R.excess(emu, ref, e32) <= 1.0, (d, M)
        assert R.excess(emu.astype(np.float16), ref, b16) <= 1.0, (d, M)
        for wrong in (R.ln_wrong_mean_short, R.ln_wrong_eps_outside):
            bad = wrong(x, c["gamma"], c["beta"])
            assert R.excess(bad, ref, b16) > 1.0, (d, M, wrong.__name__)        # visible in the fp16 output alone


def test_layernorm_cases_hold_the_listed_rows():
    c = R.ln_case(768, 1500)
    x = c["x"][:, :768].astype(np.float64)
    assert (x[3] == x[3, 0]).all() and abs(x[2].mean() - 1e3) < 1 and x[2].std() < 0.02 and np.abs(x[4]).max() == 3e4
    assert (c["gamma"] == 0).any() and (c["gamma"] < 0).any()
    assert any(R.ln_case(d, M)["ldx"] > d for d, M in R.LN_CASES) and any(R.ln_case(d, 1)["out32"] for d in R.LN_DS)


# ------------------------------------------------------------------ encoder attention
@pytest.mark.parametrize("case", R.ENC_CASES, ids=lambda c: "T%d-H%d-x%d-%s" % c)
def test_encoder_attention_bounds_hold_and_exclude_the_wrong_answers(case):
    c = R.enc_case(*case)
    T = c["T"]
    pairs = R.enc_pairs(c, subset=True)
    ref = R.enc_ref(c, pairs)
    assert R.enc_excess({key: ref[key][0] for key in ref}, ref) == 0.0
    assert R.enc_excess(R.enc_emulate32(c, pairs), ref) <= 1.0
    for wrong in (R.enc_wrong_leak_padded, R.enc_wrong_drop_last):
        bad = wrong(c, pairs)
        if bad is None:
            assert T % 32 == 0 and wrong is R.enc_wrong_leak_padded       # no padded key exists
            continue
        assert R.enc_excess({key: bad[key][0] for key in bad}, ref) > 1.0, wrong.__name__
    swaps = R.enc_swap_pairs(c)
    assert swaps or (T - 2) // 32 != (T - 1) // 32
    hp = [(0, h) for h in range(min(2, c["H"]))]
    for a, b in swaps:
        rows = np.nonzero(np.isin(R.enc_dom_index(T), (a % 32, b % 32)) | (np.arange(T) % 16 == 5))[0]
        good = R.enc_ref(c, hp, rows=rows)
        bad = R.enc_ref(c, hp, rows=rows, keys_of=lambda k, vt, T_, a=a, b=b: (k, _swapped(vt[:, :T_].T, a, b)))
        assert R.enc_excess({key: bad[key][0] for key in bad}, good) > 1.0, (a, b)


def _swapped(v, a, b):
    v = v.copy()
    v[[a, b]] = v[[b, a]]
    return v


def test_encoder_attention_cases_cover_the_list():
    cs = R.ENC_CASES
    for H in (6, 12, 20):
        assert (1500, H, 1) in {c[:3] for c in cs} and (1500, H, 3) in {c[:3] for c in cs}
    nwg = lambda T, H, items: -(-T // (128 if items * T >= 4000 else 64)) * H * items
    assert any(nwg(*c[:3]) % 8 and c[2] * c[0] >= 4000 for c in cs) and any(nwg(*c[:3]) % 8 and c[2] * c[0] < 4000 for c in cs)
    assert {65, 127, 128, 129, 1472, 1473, 1499, 1501, 1535} <= {c[0] for c in cs}
    assert set(R.ENC_PATTERNS) == {c[3] for c in cs}
    # every position of an interior and of the last tile is the dominant key of some row
    c = R.enc_case(1500, 6, 1, "dom32")
    for h in (0, 1):
        q, k, _ = R.enc_views(c, 0, h)
        dom = np.argmax(q @ k.T, axis=1)
        want = R.enc_special(1500, h)
        assert set(want[want < 1500]) | {1499} <= set(dom)
    sw = R.enc_swap_pairs(c)
    assert all((j, j + 1) in sw for j in range(32, 63)) and all((j, j + 1) in sw for j in range(1472, 1499))


# ------------------------------------------------------------------ packed cross K / V
def test_cross_kv_packer_and_unpacker_invert_each_other():
    rng = np.random.default_rng(0)
    K = rng.standard_normal((3, R.T_PAD, 64)).astype(np.float16)
    assert (R.unpack_cross_k(R.pack_cross_k(K), 3) == K).all()
    assert (R.unpack_cross_v(R.pack_cross_v(K), 3) == K).all()
    # the documented element of each layout, spelled out once by hand: K[key 1499 = tile 46, s2 1, c 11][dim 45 = kt2 1, g 1, e 5]
    img = R.pack_cross_k(K)
    assert img[(2 * 48 + 46) * 2048 + ((1 * 2 + 1) * 64 + 1 * 16 + 11) * 8 + 5] == K[2, 1499, 45]
    # V[key 1499 = tile 46, 16 + g 2 * 4 + 3 -> e 7][dim 45 = dt 2, c 13]
    img = R.pack_cross_v(K)
    assert img[(2 * 48 + 46) * 2048 + (2 * 64 + 2 * 16 + 13) * 8 + 7] == K[2, 1499, 45]


# ------------------------------------------------------------------ decode cross-attention
@pytest.mark.parametrize("case", R.XA_CASES, ids=lambda c: "H%d-R%d-g%d-r%d-i%d-%s" % c)
def test_cross_attention_bounds_hold_and_exclude_the_wrong_answers(case):
    c = R.xa_case(*case)
    ref = R.xa_ref(c)
    assert R.xa_excess({n: ref[n][0] for n in ref}, ref) == 0.0
    assert R.xa_excess(R.xa_emulate32(c), ref) <= 1.0
    for name, bad in R.xa_wrongs(c).items():
        assert R.xa_excess({n: bad[n][0] for n in bad}, ref) > 1.0, name
    s, b = R.xa_align_ref(c)
    assert R.excess((c["q"][:, 64 * c["align_head"]:][:, :64].astype(np.float32)[:, ::-1]
                     @ c["K"][c["align_item"], c["align_head"]].astype(np.float32)[:, ::-1].T), s, b) <= 1.0
    assert R.excess(R.xa_align_ref(c, swap_halves=True)[0], s, b) > 1.0


def test_cross_attention_cases_cover_the_list():
    cs = R.XA_CASES
    assert {1, 4, 5, 15, 16} <= {c[1] for c in cs} and {1, 8, 20} <= {c[2] for c in cs} and {6, 12, 20} <= {c[0] for c in cs}
    assert any(c[3] % c[1] for c in cs)
    c = R.xa_case(*cs[3])
    gi = c["group_item"]
    assert (gi != np.arange(len(gi))).any() and len(set(gi)) < len(gi)
    assert (c["V"][:, :, R.T_AUDIO:] == 0).all() and np.isfinite(c["K"].astype(np.float32)).all()
    # all mass in one split: the other splits' weights underflow in the combine
    c = R.xa_case(*cs[5])
    ref = R.xa_ref(c)
    m = ref["part_m"][0][0, 0, 0]
    assert np.sort(m)[-1] - np.sort(m)[-2] > 88


# ------------------------------------------------------------------ decode self-attention
@pytest.mark.parametrize("case", R.SA_CASES, ids=lambda c: "r%d-H%d-ident%d-p%d" % c)
def test_self_attention_bounds_hold_and_exclude_the_wrong_answers(case):
    c = R.sa_case(*case)
    for n in ("kc", "vc"):
        assert c[n].nbytes <= 64 << 20
    ref, b = R.sa_ref(c)
    assert R.excess(ref, ref, b) == 0.0
    assert R.excess(R.sa_emulate32(c), ref, b) <= 1.0
    wrongs = R.sa_wrongs(c)
    assert "one_position_too_many" in wrongs and ("newest_key_dropped" in wrongs) == (int(c["pos"].max()) > 0)
    assert "switch_one_late" in wrongs or c["cache_rows"] == 1            # (one cache row: nothing to switch to)
    for name, bad in wrongs.items():
        assert R.excess(bad, ref, b) > 1.0, name


def test_self_attention_cases_cover_the_list():
    cs = R.SA_CASES
    assert {1, 5, 16, 17, 40, 320} <= {c[0] for c in cs} and {6, 20} <= {c[1] for c in cs}
    forms = {("ident8" if c[2] and c[0] <= 16 else "ident4" if c[2] else "table") for c in cs}
    assert forms == {"ident8", "ident4", "table"}
    seen = set()
    for case in cs:
        c = R.sa_case(*case)
        seen |= set(int(p) for p in c["pos"])
        if not case[2]:
            assert (c["ancrow"] != np.arange(c["rows"])).any() or c["rows"] == 1
    assert seen == set(R.SA_POS)
    c = R.sa_case(40, 6, 1, 0)
    r = int(np.argmax(c["pos"]))
    sw = np.nonzero(np.diff(c["anc"][r].astype(np.int64)[:448]))[0] + 1
    assert any(s % 64 == 0 for s in sw) and any(s % 64 for s in sw)       # switches at block boundaries and inside blocks


# ------------------------------------------------------------------ encoder GEMM
_GEMM_HOST = [s for s in R.GEMM_FORM_CASES if s["force"] in (0, 3)] + [s for s in R.GEMM_ENGINE_CASES if s["M"] * s["N"] * s["K"] < 2e9]


@pytest.mark.parametrize("n", range(len(_GEMM_HOST)))
def test_gemm_bounds_hold_and_exclude_the_wrong_answers(n):
    c = R.gemm_case(_GEMM_HOST[n])
    x, _ = R.gemm_logical(c)
    f16 = c["mode"] not in (2, 3)
    rnd = lambda v: v.astype(np.float16) if f16 else v.astype(np.float32)
    ex, clean = R.gemm_check(c, R.gemm_place(c, rnd(x)))
    assert ex <= 1.0 and clean                                    # the reference, rounded once, through packer and unpacker
    ex, clean = R.gemm_check(c, R.gemm_place(c, rnd(R.gemm_emulate32(c))))
    assert ex <= 1.0 and clean, ex
    good = R.gemm_place(c, rnd(x))
    for wrong in R.gemm_wrongs(c):
        if wrong == "vt_shift":
            assert R.gemm_check(c, good, vt_shift=1)[0] > 1.0
        else:
            assert R.gemm_check(c, good, wrong=wrong)[0] > 1.0, wrong


def test_gemm_case_lists_cover_the_launcher():
    reach, unreachable = R.gemm_combos()
    assert len(reach) + len(unreachable) == 4 * 6 * 2 * 2 and all(unreachable.values())
    forced = {(s["force"], s["mode"]) for s in R.GEMM_FORM_CASES}
    assert forced == {(f, m) for f in range(4) for m in range(6)}
    assert {s["M"] for s in R.GEMM_ENGINE_CASES} >= {1500, 3000, 4500, 7500}
    assert any(s["zbatch"] == 3 for s in R.GEMM_FORM_CASES) and any(s["N"] % 16 for s in R.GEMM_FORM_CASES)
