"""GPU tests of dec_gemv2_kernel's argument head (csrc/dec_gemv_internal.h GemvHead), one launch each through wlx_debug_dec_gemv
against tests/dec_gemv_kernel_ref.py: every input form — LayerNorm rows, rows + slabs, embedding rows, fp16 rows (plain residual, slab
residual, K-split output), split combine — at d_model 512 and 768 and at the row counts where the head is read another way:
  1, 5   one stream's step: every first-trip address comes from the head, the row offset of the chunk rebase is 0;
  17     the first shape with 16-row tiles folded into blockIdx.x: the head's row base, the late rebase of the struct's pointers and
         the chunk fields read through the kernel-argument pointer must follow the tile;
  49     prompt prefill, two grid.z chunks of 48 rows.
Per case, as tests/test_gpu_dec_gemv_kernels.py: rc == 0, excess = max |got - float64 reference| / derived bound <= 1, and every byte
no thread owns bit-identical to the sentinel it was filled with (rows >= M, stride gaps, the other slabs, unaddressed cache rows).
Slab rows and the split combine above one row tile, and embedding rows above 48, run as row tiles of the lean kernel too (the split combine
above 32 rows on the first-generation kernel): the same checks. d_model 512 with fewer than five slab / embedding rows has no
instantiation and must be refused. d_model 128, the width of the test models, reaches dec_gemv2_kernel only without a LayerNorm (its LayerNorm rows are units of 256
columns: those forms run on the first-generation kernel); the last test runs the plain-row forms there, and 512 is the smallest
width every form of the head can be tested at.
dec_gemv2_kernel does not read the done flag (decoder.hip: a step past the finish only rewrites scratch), so there is no done case."""
import pytest

from . import dec_gemv_kernel_ref as G

pytestmark = pytest.mark.gpu
WLX_ERR_ARG = 1

# (label, in, out, xs, N, d, K or None = both widths)
FORMS = [
    ("ln_rows", G.IN_LN, G.OUT_GELU, G.X_PLAIN, 128, 0, None),
    ("ln_rows_qkv", G.IN_LN, G.OUT_QKV, G.X_PLAIN, 96, 32, None),
    ("rows_slabs", G.IN_LN, G.OUT_QKV, G.X_SLABS, 96, 32, None),
    ("embedding_rows", G.IN_LN, G.OUT_QKV, G.X_EMBED, 96, 32, None),
    ("f16_rows", G.IN_F16, G.OUT_RESID, G.X_PLAIN, 64, 0, None),
    ("f16_rows_slab_residual", G.IN_F16, G.OUT_RESID, G.X_SLABS, 64, 0, None),
    ("f16_rows_k_split", G.IN_F16, G.OUT_SLAB, G.X_PLAIN, 64, 0, 3072),
    ("split_combine", G.IN_XATTN, G.OUT_RESID, G.X_PLAIN, 64, 0, None),
]
ROWS = (1, 5, 17, 49)


def _refused(inm, xs, M, K):
    """tests/dec_gemv_kernel_ref.py NOT_LEAN: d_model 512 with fewer than five slab / embedding rows has no instantiation, and the
    first-generation kernel knows neither source"""
    return inm == G.IN_LN and xs != G.X_PLAIN and K == 512 and M < 5


CASES = [(lab, inm, out, xs, M, K, N, d) for lab, inm, out, xs, N, d, k in FORMS for K in ((k,) if k else (512, 768)) for M in ROWS]


@pytest.mark.parametrize("lab,inm,out,xs,M,K,N,d", CASES, ids=lambda v: str(v))
def test_head_follows_form_and_row_chunk(gpu, lab, inm, out, xs, M, K, N, d):
    s = G.spec(inm, out, xs, M, K, N, "", d=d, Rq=(M if M <= 16 else 5))
    c = G.gv_case(s)
    rc, got, name = G.run_gemv(c)
    if _refused(inm, xs, M, K):
        assert rc == WLX_ERR_ARG, (G.spec_id(s), rc, name)
        return
    assert rc == 0, G.spec_id(s)
    # (the split combine above 32 rows is the first-generation kernel's: the engine combines batched rows in a launch of their own)
    assert name.startswith("dec_gemv_kernel<" if (inm == G.IN_XATTN and M > 32) else "dec_gemv2_kernel<"), (G.spec_id(s), name)
    ex, per, clean = G.gv_check(c, got)
    print("argument head %s %s -> %s: excess %.4f" % (lab, G.spec_id(s), name, ex))
    assert ex <= 1.0, (G.spec_id(s), name, per)
    assert clean, (G.spec_id(s), name)


def test_d_model_128(gpu):
    """the width of the test models: its LayerNorm-fronted forms run on the first-generation kernel (no head), the others on the lean one; the same bounds"""
    for lab, inm, out, xs, N, d, k in FORMS:
        if k or xs != G.X_PLAIN:
            continue
        s = G.spec(inm, out, xs, 5, 128, N, "", d=d, Rq=5)
        c = G.gv_case(s)
        rc, got, name = G.run_gemv(c)
        # (LayerNorm rows are units of 256 columns: first-generation kernel; fp16 rows and the split combine split K = 128 as any other)
        assert rc == 0 and name.startswith("dec_gemv_kernel<" if inm == G.IN_LN else "dec_gemv2_kernel<"), (lab, rc, name)
        ex, per, clean = G.gv_check(c, got)
        assert ex <= 1.0 and clean, (lab, name, per)
