"""GPU tests of the decode GEMV chain and of the fused LayerNorm + query + cross-attention launch, one launch each, through the
wlx_debug_dec_gemv / wlx_debug_dec_cq_cross_attn hooks (csrc/kernel_hooks.hip): every projection of engine_decode.hip decoder_pass
with the parameter set the engine builds for it — QKV on plain, slab and embedding rows, attention output on plain and slab rows,
the cross-attention query, the split combine, the first MLP projection, the MLP output as RESID and as the two-slice SLAB form, the
vocabulary projection on plain and slab rows — at the smallest shapes that reach each launch rule (tests/dec_gemv_kernel_ref.py
CASES). Per case: rc == 0, everything finite, excess = max |got - float64 reference| / derived bound <= 1, every byte no thread owns
bit-identical to the +-1000 it was filled with (stride gaps, rows >= M, unaddressed cache rows and positions, the other slabs), and
the kernel name the launcher reports equals the one the case expects. tests/test_dec_gemv_kernel_ref.py shows on the host that the
nearest wrong answers fall outside the same bounds. The last test asserts that every dec_gemv2_kernel / dec_vocab_kernel
instantiation of tests/golden/decode_step_launches.json and of tests/test_gemv_picks.py EXPECTED was returned by a passing case.
Names of the pick sweep the engine never builds are out of scope: the split combine with more than one row tile (the engine runs
dec_xattn_combine_kernel + a plain projection above 16 rows), fp32 rows out with a bias, the first-generation dec_gemv_kernel."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

from . import dec_gemv_kernel_ref as G
from . import whisper_kernel_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
WLX_ERR_ARG = 1
_worst = {}
_names = set()
_ran = set()


def _record(family, case, ex):
    """the measured margin per family, for the record only (profiles/dec_gemv_kernel_tests_excess.txt); no bound reads it"""
    if ex > _worst.get(family, (-1.0, None))[0]:
        _worst[family] = (ex, case)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("WLX_EXCESS_OUT")
    if out and _worst:
        path = Path(out) / "dec_gemv_kernel_tests_excess.txt" if Path(out).is_dir() else ROOT / "profiles" / "dec_gemv_kernel_tests_excess.txt"
        with open(path, "w") as f:
            f.write("max over elements of |kernel - float64 reference| / derived bound, worst case per (IN, OUT, XS) family, from one run of\n"
                    "tests/test_gpu_dec_gemv_kernels.py on an MI355X. A record of the margin, not an input to any bound.\n")
            for fam in sorted(_worst):
                f.write("%-34s worst excess %.4f  at case %s\n" % (fam, _worst[fam][0], _worst[fam][1]))


def _same_bits(a, b, mask=None):
    a, b = G._bits(a), G._bits(b)
    return bool((a == b).all() if mask is None else (a[mask] == b[mask]).all())


def _run_check(s, c=None, arrays=None, fam=None):
    c = c or G.gv_case(s)
    rc, got, name = G.run_gemv(c, arrays=arrays)
    assert rc == 0, G.spec_id(s)
    ex, per, clean = G.gv_check(c, got)
    print("dec_gemv %s -> %s: excess %.4f %s" % (G.spec_id(s), name, ex, {k: round(v, 4) for k, v in per.items()}))
    _record(fam or G.family(s), G.spec_id(s) + " " + name, ex)
    assert ex <= 1.0, (G.spec_id(s), name, per)
    assert clean, (G.spec_id(s), name)
    if s["name"]:
        assert name == s["name"], (G.spec_id(s), name, s["name"])
    _names.add(name)
    _ran.add(G.spec_id(s))
    return c, got, name


GROUPS = sorted({(G.family(s), s["K"]) for s in G.CASES})


@pytest.mark.parametrize("fam,K", GROUPS, ids=lambda v: str(v))
def test_decode_projection(gpu, fam, K):
    for s in G.CASES:
        if G.family(s) == fam and s["K"] == K and not s["busy"]:
            _run_check(s)


def test_busy_device_row_tiles_give_the_same_bits(gpu):
    """dec_gemv.hip: two column tiles per workgroup under a busy device regroup the tiles, not any sum"""
    n = 0
    for s in G.CASES:
        if not s["busy"]:
            continue
        c, got, name = _run_check(s, fam=G.family(s) + "_busy")
        assert re.match(r"dec_gemv2_kernel<\d+, 1, 1, 3, 2, 1, 0>", name), name
        calm = dict(s, busy=0, name="")
        c0 = dict(c, busy=0)
        rc, got0, name0 = G.run_gemv(c0)
        assert rc == 0 and name0 != name and ", 3, 1, 1, 0>" in name0, (name0, name)
        assert all(_same_bits(got[k], got0[k]) for k in got), G.spec_id(calm)
        n += 1
    assert n >= 2


def test_vocabulary_rows_do_not_depend_on_the_rows_beside_them(gpu):
    """dec_vocab.hip: "A row's result does not depend on how many rows share the launch" — the same 5 rows alone and as rows 0..4 of 60"""
    s60 = G.spec(G.IN_LN, G.OUT_F32, G.X_PLAIN, 60, 768, 265, G.VOC % "24, 6, 4")
    c60, got60, _ = _run_check(s60)
    c5 = dict(c60, M=5, name=G.VOC % "24, 6, 1")
    rc, got5, name5 = G.run_gemv(c5)
    assert rc == 0 and name5 == c5["name"]
    ex, per, clean = G.gv_check(c5, got5)
    assert ex <= 1.0 and clean, per
    y60, y5 = (g["Y"].reshape(-1, c60["ldy"])[:5, :265] for g in (got60, got5))
    assert _same_bits(np.ascontiguousarray(y60), np.ascontiguousarray(y5))


def test_first_projection_reads_the_slabs_the_k_split_projection_writes(gpu):
    """producer and consumer tied without an engine: GEMV_OUT_SLAB at K = 3072, N = 768, 5 rows, then LayerNorm + QKV with xsrc = SLABS on
    the slab array it wrote (same row stride, same slab stride: the consumer's reference reads the producer's output)"""
    sp = G.spec(G.IN_F16, G.OUT_SLAB, G.X_PLAIN, 5, 3072, 768, G.G2 % "12, 1, 1, 5, 1, 1, 0")
    sc = G.spec(G.IN_LN, G.OUT_QKV, G.X_SLABS, 5, 768, 96, G.G2 % "4, 3, 0, 4, 1, 1, 1", d=32)
    cp, cc = G.gv_case(sp), G.gv_case(sc)
    assert cp["ldxres"] == cc["ldx"] and cp["slab_stride"] == cc["slab_stride"] and len(cp["slab"]) == len(cc["slab"])
    cp, gotp, _ = _run_check(sp, c=cp, fam="slab_pair_producer")
    cc["slab"] = gotp["slab"].copy()
    live = G._slabs(cc)
    assert all(np.isfinite(v).all() and np.abs(v).max() < 500 for v in live)          # (what the producer wrote, not the filler)
    _run_check(sc, c=cc, fam="slab_pair_consumer")


# ------------------------------------------------------------------ fused LayerNorm + query projection + cross-attention partials
def _sel(name, live):
    return (lambda a: a.transpose(0, 3, 1, 2, 4)[live]) if name == "part_o" else (lambda a: a.transpose(0, 2, 1, 3)[live])


@pytest.mark.parametrize("case", G.CQ_CASES, ids=lambda c: "R%d-g%d-r%d" % c)
def test_fused_query_cross_attention(gpu, case):
    c = G.cq_case(*case)
    rc, got = G.run_cq(c)
    assert rc == 0
    ref, (q, qb) = G.cq_ref(c)
    for n in ("part_o", "part_m", "part_l"):
        ex = R.excess(got[n], ref[n][0], ref[n][1])
        print("fused cq cross attention %s %s excess %.4f" % (case, n, ex))
        _record("dec_cq_cross_attn_" + n, case, ex)
        assert ex <= 1.0, (n, ex)
    # the unfused pair on the same inputs: LayerNorm + query projection (GEMV_OUT_F16), then dec_cross_attn_kernel
    p = c["proj"]
    rc, gq, name = G.run_gemv(p)
    assert rc == 0 and name == p["name"]
    q16 = gq["Yh"].reshape(-1, p["ldyh"])[:c["rows"], :G.CQ_D]
    exq = R.excess(q16, q, qb)
    _record("dec_cq_unfused_query", case, exq)
    assert exq <= 1.0
    c2 = dict(c, q=c["q"].copy())
    c2["q"][:, :G.CQ_D] = q16
    rc, un = R.run_xa(c2, align=False)
    assert rc == 0
    live = G.cq_live(c)
    for n in ("part_o", "part_m", "part_l"):
        sel = _sel(n, live)
        d = np.abs(sel(got[n]).astype(np.float64) - sel(un[n]).astype(np.float64))
        ex = float((d / (2 * sel(ref[n][1]))).max())
        print("fused against unfused %s %s: %.4f of the two bounds" % (case, n, ex))
        _record("dec_cq_fused_vs_unfused_" + n, case, ex)
        assert ex <= 1.0, (n, ex)


def test_fused_query_cross_attention_refusals(gpu):
    c = G.cq_case(5, 3, 13)
    bad_items = c["group_item"].copy()
    bad_items[1] = 3
    ld = c["proj"]["ldx"]
    overs = [dict(d=512), dict(d=1024), dict(H=6), dict(H=0), dict(R=0), dict(R=17), dict(rows=10), dict(rows=16), dict(groups=0),
             dict(ldx=ld + 2), dict(ldx=764), dict(item_stride=768 * R.T_PAD - 8), dict(item_stride=c["item_stride"] + 4),
             dict(group_item=bad_items), dict(n_items=0)]
    for over in overs:
        rc, got = G.run_cq(c, **over)
        assert rc == WLX_ERR_ARG, list(over)
        assert _same_bits(got["part_o"], c["part_o"]) and _same_bits(got["part_ml"], c["part_ml"])


# ------------------------------------------------------------------ refusals of wlx_debug_dec_gemv
def _refused(c, **over):
    rc, got, name = G.run_gemv(c, **over)
    assert rc == WLX_ERR_ARG, list(over)
    assert all(_same_bits(got[k], c[k]) for k in got), list(over)


def test_decode_projection_refusals(gpu):
    qkv = G.gv_case(G.spec(G.IN_LN, G.OUT_QKV, G.X_EMBED, 5, 768, 96, "", d=32))
    pos_hi, pos_lo, cache_hi, tok_hi = (qkv[n].copy() for n in ("row_pos", "row_pos", "row_cache", "emb_token"))
    pos_hi[2], pos_lo[1], cache_hi[3], tok_hi[0] = 448, -1, qkv["cache_rows"], 37
    pos_far = qkv["row_pos"].copy()
    pos_far[4] = qkv["npos"]
    for over in (dict(KT=23), dict(K=760, KT=24), dict(M=0), dict(M=321), dict(N=100), dict(d=24), dict(d=48), dict(ldx=770), dict(ldx=764),
                 dict(x_len=4 * 772 + 767), dict(ldyh=34), dict(ldyh=24), dict(yh_len=4 * 40 + 31), dict(cache_row_stride=qkv["crs"] + 2),
                 dict(cache_row_stride=16), dict(kc_len=qkv["crs"]), dict(vc_len=8), dict(row_pos=pos_hi), dict(row_pos=pos_lo),
                 dict(row_pos=pos_far), dict(row_cache=cache_hi), dict(emb_token=tok_hi), dict(intok_len=100), dict(pos_emb_len=768),
                 dict(bias=None), dict(gamma=None), dict(in_mode=3), dict(out_mode=6), dict(xsrc=3), dict(busy_device=2),
                 dict(out_mode=G.OUT_F16, N=96)):
        _refused(qkv, **over)
    for s in G.NOT_LEAN:                                                   # no lean kernel: the first-generation kernel knows no xsrc
        _refused(G.gv_case(s))
    res = G.gv_case(G.spec(G.IN_F16, G.OUT_RESID, G.X_SLABS, 5, 768, 64, ""))
    for over in (dict(ldxh=780), dict(ldxh=760), dict(xh_len=4 * 776 + 767), dict(ldxres=66), dict(ldxres=60), dict(xres_len=4 * 68 + 63),
                 dict(slab_stride=res["slab_stride"] + 2), dict(slab_stride=-4), dict(slab_len=res["slab_stride"] + 4 * 68 + 63),
                 dict(xsrc=G.X_EMBED), dict(K=736, KT=23, ldxh=744)):      # (the last: slab rows at a width without a lean kernel)
        _refused(res, **over)
    slab = G.gv_case(G.spec(G.IN_F16, G.OUT_SLAB, G.X_PLAIN, 5, 3072, 64, ""))
    for over in (dict(KTS=0), dict(KTS=32), dict(KTS=96), dict(slab_len=slab["slab_stride"] + 4 * 68 + 63), dict(ldxres=62)):
        _refused(slab, **over)
    xat = G.gv_case(G.spec(G.IN_XATTN, G.OUT_RESID, G.X_PLAIN, 13, 768, 64, "", Rq=5))
    for over in (dict(R=0), dict(R=17), dict(H=6), dict(R=4), dict(part_o_len=xat["part_o"].size - 1), dict(part_ml_len=xat["part_ml"].size - 1),
                 dict(xsrc=G.X_SLABS), dict(out_mode=G.OUT_F32)):
        _refused(xat, **over)
    voc = G.gv_case(G.spec(G.IN_LN, G.OUT_F32, G.X_SLABS, 5, 768, 265, ""))
    for over in (dict(M=17), dict(ldy=266), dict(ldy=264), dict(y_len=4 * 272 + 264), dict(K=1600, KT=50, ldx=1604)):
        _refused(voc, **over)


# ------------------------------------------------------------------ coverage (last: it reads what the tests above collected)
def test_every_engine_instantiation_was_launched(gpu):
    text = (ROOT / "tests" / "golden" / "decode_step_launches.json").read_text()
    want = set(re.findall(r"dec_(?:gemv2|vocab)_kernel<[^>]*>", text))
    from .test_gemv_picks import EXPECTED
    want |= set(EXPECTED.values())
    assert want - _names == set(), sorted(want - _names)
    assert {G.spec_id(s) for s in G.CASES} <= _ran                       # no case skipped
