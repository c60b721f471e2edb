"""GPU tests of the Whisper kernels one launch each, through the wlx_debug_layernorm / _attn_encoder / _dec_cross_attn /
_dec_self_attn hooks: LayerNorm (gemm.hip), the two encoder attention kernels (attention.hip), the decode cross-attention with
its combine and the alignment scores, and the three forms of the decode self-attention (decoder.hip). Every case of the lists of
tests/whisper_kernel_ref.py: rc == 0, everything finite, excess = max |got - float64 reference| / derived bound <= 1, and every
byte no thread owns bit-identical to the +-1000 it was filled with. tests/test_whisper_kernel_ref.py shows on the host that the
nearest wrong answers fall outside the same bounds. Refusal tests: every documented limit is WLX_ERR_ARG with the outputs
unchanged (the hooks return before anything is launched). wlx_debug_gemm runs launch_gemm / pack.hip the same way: the engine's
shapes on the launcher's pick, every form forced, form coverage and bit-identity across forms. The decode GEMV chain and the fused
dec_cq_cross_attn kernel have their own module of the same kind (tests/test_gpu_dec_gemv_kernels.py), and so have the softmax
kernels behind no_speech_prob, detect_language and the word probabilities with the data-movement kernels dec_embed, prep_window and
f32_to_f16 (tests/test_gpu_prob_kernels.py); the search of search.hip has token-exact injected-logits tests. Out of scope here:
log-mel and VAD, which are held to their oracles."""
import os

import numpy as np
import pytest

from . import whisper_kernel_ref as R

pytestmark = pytest.mark.gpu
WLX_ERR_ARG = 1
_worst = {}


def _record(family, case, ex):
    """the measured margin per family, for the record only (profiles/whisper_kernel_tests_excess.txt is the file a run with
    WLX_EXCESS_OUT set writes, header included); no bound reads it"""
    if ex > _worst.get(family, (-1.0, None))[0]:
        _worst[family] = (ex, case)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("WLX_EXCESS_OUT")
    if path and _worst:
        with open(path, "w") as f:
            f.write("max over elements of |kernel - float64 reference| / derived bound, worst case per family, from one run of\n"
                    "tests/test_gpu_whisper_kernels.py on an MI355X. A record of the margin, not an input to any bound.\n")
            for fam in sorted(_worst):
                f.write("%-28s worst excess %.4f  at case %s\n" % (fam, _worst[fam][0], _worst[fam][1]))


def _same_bits(a, b, mask=None):
    a, b = a.view(np.uint16 if a.dtype == np.float16 else np.uint32), b.view(np.uint16 if b.dtype == np.float16 else np.uint32)
    return bool((a == b).all() if mask is None else (a[mask] == b[mask]).all())


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("d", R.LN_DS)
def test_layernorm(gpu, d):
    for M in R.LN_MS:
        c = R.ln_case(d, M)
        rc, o16, o32, init = R.run_ln(c)
        assert rc == 0, (d, M)
        ld = c["ldo"]
        x = c["x"][:, :d]
        ref = R.ln_ref(x, c["gamma"], c["beta"])
        e32, b16 = R.ln_bound(x, c["gamma"], c["beta"])
        got = o16.reshape(M, ld)
        ex = R.excess(got[:, :d], ref, b16)
        print("layernorm d=%d M=%d excess %.4f" % (d, M, ex))
        _record("layernorm_f16", (d, M), ex)
        assert ex <= 1.0, (d, M, ex)
        assert _same_bits(got[:, d:], init.reshape(M, ld)[:, d:])
        if c["out32"]:
            g32 = o32.reshape(M, ld)
            ex32 = R.excess(g32[:, :d], ref, e32)
            print("layernorm d=%d M=%d float32 copy excess %.4f" % (d, M, ex32))
            _record("layernorm_f32_copy", (d, M), ex32)
            assert ex32 <= 1.0, (d, M, ex32)
            assert _same_bits(g32[:, :d].astype(np.float16), got[:, :d])          # the copy IS the value that was rounded
            assert _same_bits(g32[:, d:], init.astype(np.float32).reshape(M, ld)[:, d:])


def test_layernorm_refusals(gpu):
    c = R.ln_case(768, 5)
    assert c["out32"]
    for over in (dict(d=766), dict(d=2052), dict(d=0), dict(M=0), dict(ldx=764), dict(ldo=764), dict(ldx=770), dict(ldo=770)):
        rc, o16, o32, init = R.run_ln(c, **over)
        assert rc == WLX_ERR_ARG, over
        assert _same_bits(o16, init) and _same_bits(o32, init.astype(np.float32))


# ------------------------------------------------------------------ encoder attention
@pytest.mark.parametrize("case", R.ENC_CASES, ids=lambda c: "T%d-H%d-x%d-%s" % c)
def test_encoder_attention(gpu, case):
    c = R.enc_case(*case)
    rc, o = R.run_enc(c)
    assert rc == 0
    got, owned = R.enc_unpack(c, o)
    assert _same_bits(o, c["o"], ~owned)
    ref = R.enc_ref(c, R.enc_pairs(c))
    ex = R.enc_excess(got, ref)
    print("encoder attention %s excess %.4f" % (case, ex))
    _record("attn_encoder_%dwaves" % (8 if c["items"] * c["T"] >= 4000 else 4), case, ex)
    assert ex <= 1.0, ex


def test_encoder_attention_refusals(gpu):
    c = R.enc_case(129, 3, 1, "uniform")
    overs = [dict(T=64), dict(T=1), dict(ldvt=c["ldvt"] - 16), dict(ldvt=c["ldvt"] + 4), dict(ldq=c["ldq"] + 4), dict(ldk=64 * 3 - 8),
             dict(ldo=c["ldo"] + 2), dict(isq=c["isq"] + 4), dict(isk=129 * c["ldk"] - 8), dict(H=0), dict(items=0), dict(H=65)]
    for over in overs:
        rc, o = R.run_enc(c, **over)
        assert rc == WLX_ERR_ARG, over
        assert _same_bits(o, c["o"])
    for case in R.ENC_REFUSED:
        rc, o = R.run_enc(R.enc_case(*case))
        assert rc == WLX_ERR_ARG, case


# ------------------------------------------------------------------ decode cross-attention, combine, alignment scores
@pytest.mark.parametrize("case", R.XA_CASES, ids=lambda c: "H%d-R%d-g%d-r%d-i%d-%s" % c)
def test_cross_attention(gpu, case):
    c = R.xa_case(*case)
    rc, got = R.run_xa(c)
    assert rc == 0
    ref = R.xa_ref(c)
    for n in ("part_o", "part_m", "part_l", "out"):
        ex = R.excess(got[n], ref[n][0], ref[n][1])
        print("cross attention %s %s excess %.4f" % (case, n, ex))
        _record("dec_cross_attn_" + n, case, ex)
        assert ex <= 1.0, (n, ex)
    assert _same_bits(got["out_full"][:, 64 * c["H"]:], c["out"][:, 64 * c["H"]:])
    s, b = R.xa_align_ref(c)
    ex = R.excess(got["align"], s, b)
    print("alignment scores %s excess %.4f" % (case, ex))
    _record("dec_align_scores", case, ex)
    assert ex <= 1.0, ex


def test_cross_attention_refusals(gpu):
    c = R.xa_case(6, 4, 8, 30, 3, "uniform")
    bad_items = c["group_item"].copy()
    bad_items[3] = 3
    overs = [dict(R=0), dict(R=17), dict(rows=28), dict(rows=33), dict(groups=0), dict(ldq=c["ldq"] + 4), dict(ldo=64 * 6 - 8),
             dict(item_stride=6 * 64 * R.T_PAD - 8), dict(item_stride=c["item_stride"] + 4), dict(group_item=bad_items), dict(H=0),
             dict(align_head=6), dict(align_item=3), dict(n_items=0)]
    for over in overs:
        rc, got = R.run_xa(c, **over)
        assert rc == WLX_ERR_ARG, over
        assert _same_bits(got["out_full"], c["out"]) and _same_bits(got["part_o"], c["part_o"])
        assert _same_bits(got["part_ml"], c["part_ml"]) and _same_bits(got["align"], c["align_out"])


# ------------------------------------------------------------------ decode self-attention
@pytest.mark.parametrize("case", R.SA_CASES, ids=lambda c: "r%d-H%d-ident%d-p%d" % c)
def test_self_attention(gpu, case):
    c = R.sa_case(*case)
    rc, out = R.run_sa(c)
    assert rc == 0
    w = 64 * c["H"]
    ref, b = R.sa_ref(c)
    ex = R.excess(out[:, :w], ref, b)
    form = "ident_8waves" if c["ident"] and c["rows"] <= 16 else "ident_4waves" if c["ident"] else "table_4waves"
    print("self attention %s (%s) excess %.4f" % (case, form, ex))
    _record("dec_self_attn_" + form, case, ex)
    assert ex <= 1.0, ex
    assert _same_bits(out[:, w:], c["out"][:, w:])


def test_self_attention_refusals(gpu):
    c = R.sa_case(5, 6, 0, 5)
    assert (c["ancrow"] != np.arange(5)).any()
    pos_hi, pos_lo = c["pos"].copy(), c["pos"].copy()
    pos_hi[2], pos_lo[1] = 448, -1
    anc_bad = c["anc"].copy()
    anc_bad[c["ancrow"][0], 0] = c["cache_rows"]
    ancrow_bad = c["ancrow"].copy()
    ancrow_bad[4] = c["cache_rows"]
    overs = [dict(ident=1), dict(pos=pos_hi), dict(pos=pos_lo), dict(anc=anc_bad), dict(ancrow=ancrow_bad), dict(d=c["d"] - 8),
             dict(d=c["d"] + 4), dict(ldq=c["ldq"] + 4), dict(ldo=c["d"] - 2), dict(crs=c["crs"] - 2 * c["d"]), dict(crs=c["crs"] + 4),
             dict(cache_rows=0), dict(H=0), dict(rows=0)]
    for over in overs:
        rc, out = R.run_sa(c, **over)
        assert rc == WLX_ERR_ARG, list(over)
        assert _same_bits(out, c["out"])


# ------------------------------------------------------------------ encoder GEMM (launch_gemm, pack.hip)
_seen = set()


def _gemm_run_check(spec, family):
    c = R.gemm_case(spec)
    rc, out, ran = R.run_gemm(c)
    assert rc == 0, spec
    ex, clean = R.gemm_check(c, out)
    print("gemm %s mode %d M %d N %d K %d z %d -> form %d epi_lds %d xcd %d x %d: excess %.4f" % (
        spec["name"], spec["mode"], spec["M"], spec["N"], spec["K"], spec["zbatch"], *ran, ex))
    _record(family, (spec["name"], spec["mode"], spec["M"], spec["N"], spec["K"], ran), ex)
    assert ex <= 1.0, (spec, ran, ex)
    assert clean, (spec, ran)
    _seen.add((ran[0], spec["mode"], ran[1], int(ran[2] > 0)))
    return c, out, ran


@pytest.mark.parametrize("n", range(len(R.GEMM_ENGINE_CASES)))
def test_gemm_engine_shapes_on_the_launchers_pick(gpu, n):
    _gemm_run_check(R.GEMM_ENGINE_CASES[n], "gemm_engine_shapes")


def test_gemm_every_form_mode_epilogue_and_remap(gpu):
    for spec in R.GEMM_FORM_CASES:
        c, out, ran = _gemm_run_check(spec, "gemm_forced_form_%d" % spec["force"])
        assert ran[0] == spec["force"]
        if spec["name"] == "remap_1_8":
            assert ran[2:] == (1, 8)
        if spec["name"] == "remap_a2":
            assert ran[2] > 1
        if spec["name"].endswith("remap0") or spec["name"] in ("z3", "f3"):
            assert ran[2:] == (0, 0)
        if spec["name"].endswith("remap1"):
            assert ran[2] > 0
        if spec["name"] == "f3_d384_direct":
            assert ran[1] == 0
    reach, unreachable = R.gemm_combos()
    assert reach - _seen == set(), sorted(reach - _seen)
    assert not (_seen & set(unreachable))


@pytest.mark.parametrize("M", R.GEMM_EDGE_MS)
def test_gemm_forms_agree_bit_for_bit_at_tile_edges(gpu, M):
    """gemm.hip: "Results do not depend on the shape (same products, same K order)" — the three second-form tiles and the large-M
    form on the same inputs"""
    outs = []
    for form in range(4):
        c, out, ran = _gemm_run_check(R.gemm_edge_case(M, form), "gemm_edge_rows_form_%d" % form)
        outs.append(out)
    for form in (1, 2, 3):
        for name in outs[0]:
            assert _same_bits(outs[form][name], outs[0][name]), (M, form, name)


def test_gemm_refusals(gpu):
    for spec in R.GEMM_REFUSED:
        c = R.gemm_case(spec)
        rc, out, ran = R.run_gemm(c)
        assert rc == WLX_ERR_ARG, spec
        assert all(_same_bits(out[n], c[n]) for n in out)
    c = R.gemm_case(R.gemm_spec(4, 100, 3 * 128, 64, d=128, rpi=100, force=0))
    for over in (dict(mode=6), dict(force_form=4), dict(lda=c["lda"] + 4), dict(a_len=c["a_len"] - 8), dict(ldc=c["ldc"] + 4),
                 dict(c_len=len(c["C"]) - 64), dict(k_len=len(c["Kout"]) - 64), dict(v_len=len(c["Vt"]) - 64), dict(ldvt=96),
                 dict(ldk=120), dict(zbatch=2), dict(d=96), dict(rows_per_item=0), dict(KT=3)):
        rc, out, ran = R.run_gemm(c, **over)
        assert rc == WLX_ERR_ARG, over
        assert all(_same_bits(out[n], c[n]) for n in out)


def test_cross_attention_reads_what_the_cross_kv_gemm_writes(gpu):
    """producer and consumer tied without an engine: the packed K / V images of wlx_debug_gemm mode 5 (LDS-transposed epilogue on the
    second form, and the large-M form) go straight into wlx_debug_dec_cross_attn; the reference attends to the float64 K / V of the GEMM
    rounded to fp16 as the GEMM's own output is (read back through the unpacker, whose agreement with the GEMM reference was checked
    above to the GEMM bound)"""
    for force in (0, 3):
        d, H = 384, 6
        g = R.gemm_case(R.gemm_spec(5, 3000, 2 * d, 256, d=d, rpi=1500, force=force, name="ckv_for_attn"))
        rc, out, ran = R.run_gemm(g)
        assert rc == 0
        ex, clean = R.gemm_check(g, out)
        assert ex <= 1.0 and clean
        c = R.xa_case(H, 5, 8, 38, 2, "uniform")
        c["item_stride"] = g["kis"]
        c["kp"] = out["Kout"][:2 * g["kis"]].reshape(2, -1).copy()
        c["vp"] = out["Vt"][:2 * g["vis"]].reshape(2, -1).copy()
        for it in range(2):
            c["K"][it] = R.unpack_cross_k(c["kp"][it, :d * R.T_PAD], H)
            c["V"][it] = R.unpack_cross_v(c["vp"][it, :d * R.T_PAD], H)
            c["vp"][it, :d * R.T_PAD] = R.pack_cross_v(np.where(np.arange(R.T_PAD)[None, :, None] < R.T_AUDIO, c["V"][it], 0))
            c["V"][it][:, R.T_AUDIO:] = 0              # (the engine's V padding is zero; the hook's destination was garbage-filled)
        rc, got = R.run_xa(c)
        assert rc == 0
        ref = R.xa_ref(c)
        for n in ("part_o", "part_m", "part_l", "out"):
            ex = R.excess(got[n], ref[n][0], ref[n][1])
            print("cross attention on the GEMM's packed output (form %d) %s excess %.4f" % (force, n, ex))
            _record("dec_cross_attn_from_gemm_" + n, force, ex)
            assert ex <= 1.0, (n, ex)
