"""CPU guard of tests/dec_gemv_kernel_ref.py, for every case the GPU tests run (tests/test_gpu_dec_gemv_kernels.py): the float64
reference is inside its own bound, a float32 computation in another association stays inside it (the bound is not so tight that a
correct kernel fails), every wrong answer that exists for the case leaves it — excess > 1 on at least one element, or a byte outside
the documented layout changed — and the inputs make the wrong answers visible: every K slice, every slab and every k-tile carries a
share of every output far above the bound. No hook is called."""
import re
from pathlib import Path

import numpy as np
import pytest

from . import dec_gemv_kernel_ref as G
from . import whisper_kernel_ref as R

ROOT = Path(__file__).resolve().parents[1]
FAMILIES = sorted({G.family(s) for s in G.CASES})


@pytest.mark.parametrize("fam", FAMILIES)
def test_bounds_hold_and_exclude_the_wrong_answers(fam):
    seen = set()
    for s in (s for s in G.CASES if G.family(s) == fam):
        c = G.gv_case(s)
        ref = G.gv_logical(c)
        assert all(np.isfinite(b).all() and (b > 0).all() for _, b in ref.values()), G.spec_id(s)
        ex, per, clean = G.gv_check(c, G.gv_place(c, G.gv_emulate32(c)), ref)
        assert ex <= 1.0 and clean, (G.spec_id(s), per, clean)
        wrongs = G.gv_wrongs(c)
        if G.is_big(s):
            wrongs = wrongs[:1]
        for w in wrongs:
            ex, per, clean = G.gv_check(c, G.gv_wrong_arrays(c, w), ref)
            assert ex > 1.0 or not clean, (G.spec_id(s), w, per)
            if w not in ("dup_last_row", "kv_pos_plus1"):
                assert ex > 1.0, (G.spec_id(s), w, per)         # a value wrong shows in the values
            seen.add(w)
    want = {"in0_out4_xs1": {"slab_missing", "slab_twice", "ln_without_slabs", "qscale_on_k", "kv_pos_plus1"},
            "in1_out3_xs1": {"resid_slab_missing", "resid_slab_twice"}, "in1_out5_xs0": {"bias_both", "slab_swapped"},
            "in2_out3_xs0": {"drop_split"}, "in0_out2_xs0": {"ragged_clamped"}}.get(fam, set())
    assert want | {"drop_ktile", "dup_last_row"} <= seen, (fam, seen)


@pytest.mark.parametrize("fam", FAMILIES)
def test_case_inputs_make_the_wrong_answers_visible(fam):
    """every K slice and every slab holds a share of EVERY output at least four times the bound of that output, every k-tile on
    more than half of the outputs (a row's 32 products can cancel)"""
    for s in (s for s in G.CASES if G.family(s) == fam and not G.is_big(s)):
        c = G.gv_case(s)
        K, N, M = c["K"], c["N"], c["M"]
        h, _ = G.gv_rows(c)
        w = G.gv_w16(c)
        ref = G.gv_logical(c)
        # e: a bound of o = acc + bias per output, read back from the destination's bound (which only adds to it)
        if c["out"] == G.OUT_SLAB:
            v, b = ref["slab"]
            assert (np.abs(v) > 4 * b).all(), G.spec_id(s)      # each slice's own sum, bias or not
            e = b.max(0)
        elif c["out"] == G.OUT_QKV:
            e = np.concatenate([ref["Yh"][1] / c["qscale"], ref["K"][1], ref["V"][1]], axis=1)
        elif c["out"] in (G.OUT_F16, G.OUT_GELU):
            e = ref["Yh"][1] / c["qscale"]
        else:
            e = ref["Y" if c["out"] == G.OUT_F32 else "Xres"][1]
        for k0, k1 in ((0, K // 2), (K // 2, K)):
            assert (np.abs(h[:, k0:k1] @ w[:, k0:k1].T) > 4 * e).all(), (G.spec_id(s), k0)
        tiles = np.abs(np.einsum("mtk,ntk->tmn", h.reshape(M, K // 32, 32), w.reshape(N, K // 32, 32)))
        assert ((tiles > 4 * e[None]).mean((1, 2)) > 0.5).all(), G.spec_id(s)      # every k-tile, on most of the outputs
        if c["xs"] == G.X_SLABS:
            for sl in G._slabs(c):
                assert np.abs(sl).min() >= 0.25
            if c["out"] == G.OUT_RESID:
                assert ref["Xres"][1].max() < 0.25 / 4


def test_case_list_covers_what_the_issue_names():
    cs = G.CASES
    assert {s["K"] for s in cs if s["inm"] == G.IN_LN} == {384, 512, 768, 1024, 1280}
    assert {s["K"] for s in cs if s["out"] in (G.OUT_SLAB,)} == {1536, 2048, 3072, 4096, 5120}
    assert {1, 5, 8, 9, 16, 17, 32, 33, 48, 49, 60, 64, 65, 120, 320} <= {s["M"] for s in cs}
    assert {(s["K"], s["N"], s["M"]) for s in cs if s["out"] == G.OUT_GELU} >= {(1280, 5120, 16), (1280, 5120, 48)}
    voc = [s for s in cs if s["out"] == G.OUT_F32]
    assert {256, 265, 288, 51865} == {s["N"] for s in voc} and {0, 1} == {s["xs"] for s in voc}
    assert {(s["M"], s["K"]) for s in voc} >= {(65, 768), (49, 1280), (120, 768), (120, 1280), (5, 768), (60, 768)}
    assert any(s["busy"] for s in cs if s["inm"] == G.IN_F16 and s["out"] == G.OUT_RESID and s["M"] > 16)
    xat = {(s["Rq"], -(-s["M"] // s["Rq"])) for s in cs if s["inm"] == G.IN_XATTN}
    assert {1, 5, 16} == {r for r, _ in xat} and {1, 3} <= {g for _, g in xat} and all(s["M"] <= 16 for s in cs if s["inm"] == G.IN_XATTN)
    assert all(s["M"] <= G.MAX_ROWS for s in cs)


def test_case_names_cover_the_engines_instantiations():
    """every dec_gemv2_kernel / dec_vocab_kernel name of the recorded decode steps and of the pinned picks is some case's expected name
    (the GPU module asserts that the launches returned them)"""
    text = (ROOT / "tests" / "golden" / "decode_step_launches.json").read_text()
    want = set(re.findall(r"dec_(?:gemv2|vocab)_kernel<[^>]*>", text))
    from .test_gemv_picks import EXPECTED
    want |= set(EXPECTED.values())
    assert want - {s["name"] for s in G.CASES} == set()


@pytest.mark.parametrize("case", G.CQ_CASES, ids=lambda c: "R%d-g%d-r%d" % c)
def test_fused_query_cross_attention_reference(case):
    """a float32 query inside its bound gives partials inside theirs; the wrong answers of the fusion lie outside them"""
    c = G.cq_case(*case)
    ref, (q, qb) = G.cq_ref(c)
    es_max = max(float((qb[:, 64 * h:64 * h + 64] @ np.abs(c["K"][it, h].astype(np.float64)[:R.T_AUDIO]).T).max())
                 for it in range(c["n_items"]) for h in range(c["H"]))
    assert es_max <= 0.045, es_max                               # (the first-order treatment of the query's error: xa_ref)
    p = c["proj"]
    q16 = G.gv_emulate32(p)["Yh"]
    assert R.excess(q16, q, qb) <= 1.0
    c2 = dict(c, q=q16)
    emu = R.xa_emulate32(c2)                                    # (dead lanes: the group's first row; compared on the live lanes)
    live = G.cq_live(c)
    for n, sel in (("part_o", lambda a: a.transpose(0, 3, 1, 2, 4)[live]), ("part_m", lambda a: a.transpose(0, 2, 1, 3)[live]),
                   ("part_l", lambda a: a.transpose(0, 2, 1, 3)[live])):
        assert R.excess(sel(emu[n]), sel(ref[n][0]), sel(ref[n][1])) <= 1.0, n
    # the wrong answers of the fusion itself: the bias left out of the query, the query of the row below, one k-tile of the projection dropped
    qd = G.gv_logical(p, "drop_ktile")["Yh"][0]
    for name, qbad in (("no_bias", q - 0.125 * p["bias"].astype(np.float64)), ("row_below", np.roll(q, 1, axis=0)), ("drop_ktile", qd)):
        if name == "row_below" and c["rows"] == 1:
            continue
        bad = R.xa_ref(c, q=qbad, qb=qb, dead_last=True)
        assert max(R.excess(bad[n][0], ref[n][0], ref[n][1]) for n in ("part_o", "part_m", "part_l")) > 1.0, name
    other, _ = G.cq_ref(c, item_of=lambda g: (int(c["group_item"][g]) + 1) % c["n_items"])
    assert R.excess(other["part_o"][0], ref["part_o"][0], ref["part_o"][1]) > 1.0
    if case[2] < case[0] * case[1] or case[0] < 16:            # a dead lane exists: the two fallback rules differ
        first, _ = G.cq_ref(c, dead_last=False)
        if min(case[0], case[2] - (case[1] - 1) * case[0]) > 1:
            assert R.excess(first["part_o"][0], ref["part_o"][0], ref["part_o"][1]) > 1.0
