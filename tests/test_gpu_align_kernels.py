"""GPU tests (-m gpu) of word alignment's post-processing kernels (csrc/align.hip) through their hooks, no engine:

* wlx_debug_dtw against oracle.alignment.dtw, element for element. Integer-valued matrices (entries in {-2, -1, 0}: exact in float32
  and full of ties, so they pin the tie rule) and seeded Gaussian ones; one add per cell, so the path has to be identical.
* wlx_debug_align_post's cost matrix against a float64 numpy restatement (below, with oracle.alignment.median_filter): absolute 2e-5.
  A plain float32 numpy restatement stays within 4e-7 of float64 on these inputs (|x| <= 1.1); the factor of 50 is room for the
  hardware exp and another summation order, far below the 1e-3 scale at which paths move.
* the path wlx_debug_align_post returns is exactly oracle.alignment.dtw of the cost matrix it returned.
* shapes the launchers do not serve are refused (WLX_ERR_ARG) with the outputs unchanged."""
import ctypes as C

import numpy as np
import pytest

from oracle import alignment as oal

pytestmark = pytest.mark.gpu

ROW = 1536
N_SOT = 3


@pytest.fixture(scope="module")
def lib(gpu):
    from whisperlive_amd import _lib
    return _lib.load()


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def run_dtw(lib, mats, path_stride=None, sentinel=-7):
    """-> (rc, [(ti, fi)] per matrix, raw output arrays)"""
    n = len(mats)
    N = np.asarray([m.shape[0] for m in mats], dtype=np.int32)
    M = np.asarray([m.shape[1] for m in mats], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.float32).ravel() for m in mats]))
    ps = int((N + M).max()) + 3 if path_stride is None else path_stride
    ti = np.full((n, ps), sentinel, dtype=np.int32)
    fi = np.full((n, ps), sentinel, dtype=np.int32)
    npth = np.full(n, sentinel, dtype=np.int32)
    rc = lib.wlx_debug_dtw(0, _f32(x), n, _i32(N), _i32(M), _i32(ti), _i32(fi), ps, _i32(npth))
    paths = [(ti[e, : npth[e]].copy(), fi[e, : npth[e]].copy()) for e in range(n)] if rc == 0 else None
    return rc, paths, (ti, fi, npth)


def make_matrix(kind, N, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        return rng.integers(-2, 1, size=(N, M)).astype(np.float32)
    return rng.standard_normal((N, M)).astype(np.float32)


DTW_SHAPES = [(2, 1), (2, 2), (1, 5), (3, 64), (63, 65), (64, 64), (65, 129), (130, 1500), (445, 1500)]
_dtw_ref_cache = {}


def dtw_ref(kind, N, M):
    """the definition's path of the seeded matrix of this kind and shape (computed once: 445 x 1500 takes the Python loop seconds)"""
    key = (kind, N, M)
    if key not in _dtw_ref_cache:
        x = make_matrix(kind, N, M, seed=1000 * N + M)
        _dtw_ref_cache[key] = (x, oal.dtw(x))
    return _dtw_ref_cache[key]


@pytest.mark.parametrize("kind", ["ties", "gauss"])
@pytest.mark.parametrize("shape", DTW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtw_is_the_definition_element_for_element(lib, kind, shape):
    x, (rti, rfi) = dtw_ref(kind, *shape)
    rc, paths, (ti, fi, npth) = run_dtw(lib, [x])
    assert rc == 0, lib.wlx_last_error()
    assert npth[0] == len(rti)
    np.testing.assert_array_equal(paths[0][0], rti)
    np.testing.assert_array_equal(paths[0][1], rfi)
    assert (ti[0, npth[0]:] == -7).all() and (fi[0, npth[0]:] == -7).all()       # nothing written past the path


@pytest.mark.parametrize("kind", ["ties", "gauss"])
def test_dtw_ragged_launch_equals_single_launches(lib, kind):
    shapes = [s for s in DTW_SHAPES if s[0] > 1]
    assert len(shapes) == 8
    mats = [dtw_ref(kind, *s)[0] for s in shapes]
    rc, ragged, _ = run_dtw(lib, mats)
    assert rc == 0, lib.wlx_last_error()
    for m, got, s in zip(mats, ragged, shapes):
        rc1, single, _ = run_dtw(lib, [m])
        assert rc1 == 0
        np.testing.assert_array_equal(got[0], single[0][0], err_msg=str(s))
        np.testing.assert_array_equal(got[1], single[0][1], err_msg=str(s))
        rti, rfi = dtw_ref(kind, *s)[1]
        np.testing.assert_array_equal(got[0], rti, err_msg=str(s))
        np.testing.assert_array_equal(got[1], rfi, err_msg=str(s))


# ---- cost matrix
def cost_ref64(scores, nf, mw):
    """float64 restatement of oracle.alignment.align's matrix, negated: scores [heads, n_tok, ROW] -> [n_tok - 1 - N_SOT, nf]"""
    s = scores[:, :, :nf].astype(np.float64)
    w = np.exp(s - s.max(axis=-1, keepdims=True))
    w /= w.sum(axis=-1, keepdims=True)
    mean, std = w.mean(axis=1, keepdims=True), w.std(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (w - mean) / std
    z = oal.median_filter(z, mw)
    return -(z.mean(axis=0)[N_SOT:-1])


def run_post(lib, entries, mw, n_heads, path_stride=None, n_sot=N_SOT, sentinel=-7):
    """entries = [(scores [heads, n_tok, ROW], nf)] -> (rc, [cost [N, nf]], [(ti, fi)], raw outputs)"""
    n = len(entries)
    n_tok = np.asarray([s.shape[1] for s, _ in entries], dtype=np.int32)
    nf = np.asarray([f for _, f in entries], dtype=np.int32)
    scores = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.float32).ravel() for s, _ in entries]))
    Ns = np.maximum(n_tok - 1 - n_sot, 0)
    sizes = [int(a) * max(int(b), 0) for a, b in zip(Ns, nf)]
    cost = np.full(max(1, sum(sizes)), float(sentinel), dtype=np.float32)
    ps = int((Ns + np.clip(nf, 0, 1500)).max()) + 3 if path_stride is None else path_stride
    ti = np.full((n, ps), sentinel, dtype=np.int32)
    fi = np.full((n, ps), sentinel, dtype=np.int32)
    npth = np.full(n, sentinel, dtype=np.int32)
    rc = lib.wlx_debug_align_post(0, _f32(scores), n, n_heads, _i32(n_tok), n_sot, _i32(nf), mw, _f32(cost), _i32(ti), _i32(fi), ps, _i32(npth))
    if rc != 0:
        return rc, None, None, (cost, ti, fi, npth)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    mats = [cost[offs[e]: offs[e + 1]].reshape(int(Ns[e]), int(nf[e])) for e in range(n)]
    paths = [(ti[e, : npth[e]].copy(), fi[e, : npth[e]].copy()) for e in range(n)]
    return rc, mats, paths, (cost, ti, fi, npth)


def make_scores(heads, n_tok, nf, std, seed):
    rng = np.random.default_rng(seed)
    s = (std * rng.standard_normal((heads, n_tok, ROW))).astype(np.float32)
    s[:, :, nf:] = np.nan           # the 1536-float rows of the capture kernel: frames past nf are never read
    return s


POST_CASES = [(1, 6, 1, 7), (1, 6, 3, 7), (1, 6, 4, 7), (3, 7, 33, 3), (6, 12, 75, 7), (2, 9, 65, 1), (2, 9, 65, 15), (10, 40, 700, 7),
              (6, 130, 1500, 7)]


@pytest.mark.parametrize("std", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("case", POST_CASES, ids=lambda c: "h%d_t%d_f%d_m%d" % c)
def test_cost_matrix_against_float64_and_path_against_its_own_matrix(lib, case, std):
    heads, n_tok, nf, mw = case
    scores = make_scores(heads, n_tok, nf, std, seed=heads * 100000 + n_tok * 1000 + nf + mw + int(std))
    rc, mats, paths, _ = run_post(lib, [(scores, nf)], mw, heads)
    assert rc == 0, lib.wlx_last_error()
    ref = cost_ref64(scores, nf, mw)
    got = mats[0]
    assert got.shape == ref.shape
    if nf == 1:                     # a zero std under the division: NaN in both, nothing else is asserted
        np.testing.assert_allclose(got, ref, atol=2e-5, rtol=0, equal_nan=True)
        return
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("align cost", case, "std", std, "max abs error vs float64", err, "max |x|", float(np.abs(ref).max()))
    assert np.isfinite(got).all()
    assert err <= 2e-5
    rti, rfi = oal.dtw(got)         # exact: the path is the DTW of the float32 matrix the device computed
    np.testing.assert_array_equal(paths[0][0], rti)
    np.testing.assert_array_equal(paths[0][1], rfi)


def test_cost_matrix_ragged_launch_equals_single_launches(lib):
    cases = [(4, 6, 3), (4, 7, 33), (4, 12, 75), (4, 9, 65), (4, 40, 700), (4, 70, 1500)]
    entries = [(make_scores(h, t, f, 2.0, seed=t), f) for h, t, f in cases]
    rc, mats, paths, _ = run_post(lib, entries, 7, 4)
    assert rc == 0, lib.wlx_last_error()
    for e, ent in enumerate(entries):
        rc1, m1, p1, _ = run_post(lib, [ent], 7, 4)
        assert rc1 == 0
        np.testing.assert_array_equal(mats[e].view(np.uint32), m1[0].view(np.uint32))
        np.testing.assert_array_equal(paths[e][0], p1[0][0])
        np.testing.assert_array_equal(paths[e][1], p1[0][1])


def _unchanged(raw, sentinel=-7):
    return all((np.asarray(a) == sentinel).all() for a in raw)


@pytest.mark.parametrize("what", ["even width", "width 17", "n = 65", "nf = 0", "nf = 1501", "n_tok < n_sot + 3", "path_stride too small"])
def test_align_post_refusals_leave_the_outputs_alone(lib, what):
    from whisperlive_amd._lib import ERR_ARG
    heads, n_tok, nf, mw, n, ps = 2, 8, 40, 7, 1, None
    if what == "even width":
        mw = 6
    elif what == "width 17":
        mw = 17
    elif what == "n = 65":
        n = 65
    elif what == "nf = 0":
        nf = 0
    elif what == "nf = 1501":
        nf = 1501
    elif what == "n_tok < n_sot + 3":
        n_tok = N_SOT + 2
    else:
        ps = (n_tok - 1 - N_SOT) + nf - 1
    s = np.zeros((heads, n_tok, ROW), dtype=np.float32)
    rc, _, _, raw = run_post(lib, [(s, nf)] * n, mw, heads, path_stride=ps)
    assert rc == ERR_ARG, (what, rc)
    assert _unchanged(raw), what


def test_dtw_refusals_leave_the_outputs_alone(lib):
    from whisperlive_amd._lib import ERR_ARG
    x = np.zeros((4, 9), dtype=np.float32)
    for mats, ps in (([x] * 65, None), ([x], 4 + 9 - 1), ([np.zeros((449, 3), dtype=np.float32)], None),
                     ([np.zeros((3, 1501), dtype=np.float32)], None)):
        rc, _, raw = run_dtw(lib, mats, path_stride=ps)
        assert rc == ERR_ARG
        assert _unchanged(raw)
