"""GPU tests of the front of the fused LayerNorm + query + cross-attention launch (csrc/decoder.hip dec_cq_cross_attn_kernel), one launch
each through wlx_debug_dec_cq_cross_attn, against the float64 reference of tests/dec_gemv_kernel_ref.py with the bounds of
tests/test_gpu_dec_gemv_kernels.py (excess = max |got - reference| / derived bound <= 1). The front is where the launch's requests are
ordered: the group's item is requested first and waited for in front of K / V only, the gamma / beta exchange and the first trip's
LayerNorm run behind the weight requests and in front of K / V's. Rows 1 (wave 0 alone holds a row), 5, 6 (the last one-trip count),
7 (the first second trip) and 16 (a full tile) in one group; two groups on two DIFFERENT items with a short last group (the
group_item path). The last test holds the partials of rows 5 and 7 bit for bit against arrays recorded from the library before the
requests were re-ordered (tests/golden/cq_cross_attn_front_before_reorder.npz): same values into the same arithmetic."""
from pathlib import Path

import numpy as np
import pytest

from . import dec_gemv_kernel_ref as G
from . import whisper_kernel_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "cq_cross_attn_front_before_reorder.npz"
ONE_GROUP_ROWS = [1, 5, 6, 7, 16]
_runs = {}


def _case(Rq, groups, rows, items=None):
    c = G.cq_case(Rq, groups, rows)
    if items is not None:
        c["group_item"] = np.array(items, np.int32)
    return c


def _run(key, c):
    """one launch per case, shared by the tests that read it"""
    if key not in _runs:
        rc, got = G.run_cq(c)
        assert rc == 0
        _runs[key] = got
    return _runs[key]


def _check(c, got, tag):
    ref, _ = G.cq_ref(c)
    for n in ("part_o", "part_m", "part_l"):
        ex = R.excess(got[n], ref[n][0], ref[n][1])
        print("cq front %s %s excess %.4f" % (tag, n, ex))
        assert ex <= 1.0, (tag, n, ex)


@pytest.mark.parametrize("rows", ONE_GROUP_ROWS)
def test_one_group_rows(gpu, rows):
    c = _case(rows, 1, rows)
    _check(c, _run(("one", rows), c), "rows %d" % rows)


@pytest.mark.parametrize("Rq,rows,items", [(5, 8, (2, 0)), (7, 9, (0, 2))], ids=["R5-rows8", "R7-rows9"])
def test_two_groups_on_two_items_last_group_short(gpu, Rq, rows, items):
    c = _case(Rq, 2, rows, items)
    assert c["n_items"] > max(items) and items[0] != items[1] and rows % Rq
    _check(c, _run(("two", Rq, rows), c), "R %d rows %d items %s" % (Rq, rows, items))
    # the group table is read: the same launch with the two items swapped gives other partials
    c2 = _case(Rq, 2, rows, items[::-1])
    rc, got2 = G.run_cq(c2)
    assert rc == 0
    _check(c2, got2, "R %d rows %d items %s" % (Rq, rows, items[::-1]))
    assert not np.array_equal(got2["part_ml"], _runs[("two", Rq, rows)]["part_ml"])


@pytest.mark.parametrize("rows", [5, 7])
def test_partials_equal_the_recorded_ones_bit_for_bit(gpu, rows):
    c = _case(rows, 1, rows)
    got = _run(("one", rows), c)
    with np.load(GOLDEN) as z:
        po, ml = z["part_o_rows%d" % rows], z["part_ml_rows%d" % rows]
    assert po.dtype == np.uint16 and ml.dtype == np.uint32
    assert np.array_equal(np.ascontiguousarray(got["part_o"]).view(np.uint16).reshape(po.shape), po)
    assert np.array_equal(np.ascontiguousarray(got["part_ml"]).view(np.uint32).reshape(ml.shape), ml)
