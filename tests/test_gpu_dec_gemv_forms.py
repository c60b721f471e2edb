"""GPU tests of the decode projection forms of one stream's step (csrc/dec_gemv.hip dec_gemv2_kernel), one launch each through
wlx_debug_dec_gemv, bit for bit against arrays recorded from the library BEFORE the bodies of the fp16-rows-in forms were re-ordered
(tests/golden/dec_gemv_forms_before_reorder.npz): the staging helper's unit index by a rounded reciprocal, the B fragments of a
staged one-chunk wave as LDS reads inside the staged branch (MFMAs wait weight by weight), and the K-split form's bias zeroed in the
epilogue instead of behind the weight request. Same values into the same arithmetic in the same order: every in / out array of a
launch — what the kernel owns, and every byte around it — must keep the recorded bits.

d_model 768, rows 1 (one live row), 5 (the headline's odd row count, two row trips of the LayerNorm-fronted form) and 16 (a full
tile) of:
  mlp1   LayerNorm + first MLP projection + GELU          <6, 3, 0, 1, 1, 1, 0>
  slab   K-split MLP output projection, BOTH K slices     <12, 1, 1, 5, 1, 1, 0>   (grid.y = 2: slice 0 adds the bias, slice 1 must not)
  xattn  cross-attention output projection, split combine <6, 1, 2, 3, 1, 1, 0>   (partials: see _xattn_partials)
  sao    self-attention output projection, rows + slabs   <12, 1, 1, 3, 1, 1, 1>   (the other staged fp16-rows-in form of the step)
The float64 reference and its bounds are checked for the same launches too (tests/dec_gemv_kernel_ref.py), so a recorded array cannot
pin a wrong answer."""
from pathlib import Path

import numpy as np
import pytest

from . import dec_gemv_kernel_ref as G

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "dec_gemv_forms_before_reorder.npz"
ROWS = [1, 5, 16]
FORMS = {
    "mlp1": (G.IN_LN, G.OUT_GELU, G.X_PLAIN, 768, 128, "6, 3, 0, 1, 1, 1, 0"),
    "slab": (G.IN_F16, G.OUT_SLAB, G.X_PLAIN, 3072, 64, "12, 1, 1, 5, 1, 1, 0"),
    "xattn": (G.IN_XATTN, G.OUT_RESID, G.X_PLAIN, 768, 64, "6, 1, 2, 3, 1, 1, 0"),
    "sao": (G.IN_F16, G.OUT_RESID, G.X_SLABS, 768, 64, "12, 1, 1, 3, 1, 1, 1"),
}
_runs = {}


def _xattn_partials(c):
    """the (m, l) pairs of the split combine, per (row, head): even heads — split 3's maximum dominates (m = 40 above the others:
    their weights exp(-40) vanish against it in fp32 sums of eight); odd heads — all eight maxima EQUAL (every weight is exp(0) l)"""
    ml = c["part_ml"]
    H = ml.shape[1]
    for h in range(H):
        if h % 2 == 0:
            ml[:, h, :, 3, 0] = ml[:, h, :, :, 0].max(-1) + 40.0
        else:
            ml[:, h, :, :, 0] = ml[:, h, :, :1, 0]
    c["part_ml"] = ml.astype(np.float32)


def case(form, M):
    inm, out, xs, K, N, name = FORMS[form]
    Rq = (16 if M == 16 else min(M, 5)) if inm == G.IN_XATTN else 5
    c = G.gv_case(G.spec(inm, out, xs, M, K, N, G.G2 % name, Rq=Rq))
    if inm == G.IN_XATTN:
        _xattn_partials(c)
    return c


def run(form, M):
    """one launch per case, shared by the tests that read it"""
    if (form, M) not in _runs:
        c = case(form, M)
        rc, got, name = G.run_gemv(c)
        assert rc == 0
        _runs[(form, M)] = (c, got, name)
    return _runs[(form, M)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]).ravel()


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_form_runs_its_instantiation_inside_the_bounds(gpu, form, M):
    c, got, name = run(form, M)
    assert name == c["name"]
    worst, per, clean = G.gv_check(c, got)
    print("forms %s rows %d excess %s" % (form, M, {k: round(float(v), 4) for k, v in per.items()}))
    assert clean and worst <= 1.0, (form, M, per, clean)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_form_equals_the_recorded_arrays_bit_for_bit(gpu, form, M):
    c, got, _ = run(form, M)
    with np.load(GOLDEN) as z:
        names = [n for n in z.files if n.startswith("%s_rows%d_" % (form, M))]
        assert names, (form, M)
        for n in names:
            arr = n.split("_", 2)[2]
            assert z[n].dtype in (np.uint16, np.uint32)
            assert np.array_equal(bits(got[arr]), z[n]), (form, M, arr)


def test_slab_case_has_both_k_slices_and_xattn_case_both_kinds_of_maxima():
    """what the cases are for (no launch): two K slices with a non-zero bias, dominated and equal maxima among the partials"""
    c = case("slab", 5)
    assert c["KTS"] * 2 == c["KT"] and G.KS == 2 and np.abs(c["bias"]).min() > 0
    ml = case("xattn", 5)["part_ml"]
    m = ml[..., 0]
    assert (np.sort(m[:, 0::2], -1)[..., -1] - np.sort(m[:, 0::2], -1)[..., -2] >= 40.0 - 1e-3).all()
    assert (m[:, 1::2].max(-1) == m[:, 1::2].min(-1)).all()
