"""CPU test of tests/vad_kernel_ref.py, before anything runs on a GPU: every wrong variant of a stage leaves the stage's derived bound
on the case named here, the float32 run of the restatement stays inside the bound on EVERY case (so the bound is a statement about
float32 arithmetic), the W_hh factor of the second weight family is admitted, and the references agree with oracle/silero_vad.py."""
import numpy as np
import pytest

from oracle import silero_vad as sv
from . import vad_kernel_ref as R

# the case on which each wrong variant is shown to leave the bound
FE_CAUGHT = {"no_b_hh": (1, "speech"), "tail_off_by_one": (0, "nyquist"), "nyquist_dropped": (1, "nyquist"), "conv3_tap0": (1, "dc"),
             "conv2_shifted": (1, "dc"), "context_zero": (3, "speech"), "context_from_neighbour": (3, "fullscale")}
LSTM_CAUGHT = {"gate_order_iofg": ("base", "sat100", "ragged"), "whh_quarters": ("scaled", "gauss", "one"),
               "no_reset": ("base", "gauss", "table")}
OUT_CAUGHT = {"no_relu": (1, 0), "copy1": (1, 4)}


def _packed(c):
    return np.concatenate([it[1] for it in c["items"]]), np.concatenate([it[2] for it in c["items"]])


def test_every_wrong_variant_is_listed():
    assert set(FE_CAUGHT) == set(R.FE_WRONGS) and set(LSTM_CAUGHT) == set(R.LSTM_WRONGS) and set(OUT_CAUGHT) == set(R.OUT_WRONGS)
    assert all(c in R.FE_CASES for c in FE_CAUGHT.values()) and all(c in R.LSTM_CASES for c in LSTM_CAUGHT.values())
    assert all(c in R.OUT_CASES for c in OUT_CAUGHT.values())


def test_case_lists_cover_what_they_promise():
    ns = {n for counts, _ in R.FE_SHAPES for n in counts}
    assert ns == {1, 63, 511, 512, 513, 2047, 2048, 2049}
    assert {e for _, ex in R.FE_SHAPES for e in ex} == {0, 1, 4}
    assert {1, 3, 4, 5} <= {R.windows_of(n, e) for counts, ex in R.FE_SHAPES for n, e in zip(counts, ex)}
    assert {T for ts in R.LSTM_TS.values() for T in ts} == {1, 2, 3, 65} and len(R.LSTM_TS["table"]) == 64
    assert {T for T, _ in R.OUT_CASES} == {1, 3, 4, 5}


@pytest.mark.parametrize("case", R.FE_CASES, ids=lambda c: "s%d-%s" % c)
def test_frontend_float32_run_is_inside_the_bound(case):
    c = R.fe_case(*case)
    ref, b = R.fe_ref(c)
    assert ref.shape == (sum(c["T"]), 512) and np.isfinite(ref).all() and np.isfinite(b).all() and (b > 0).all()
    f32, _ = R.fe_ref(c, np.float32)
    ex = R.excess(f32, ref, b)
    print("frontend %s float32 excess %.4f, largest bound %.3g" % (case, ex, b.max()))
    assert ex <= 1.0
    # a window that is all zeros, context included, gives the row of silence
    sil, _ = R.fe_silence_row()
    for r in R.fe_silent_rows(c):
        assert np.abs(ref[r] - sil[0]).max() < 1e-12


def test_frontend_reference_is_the_oracle():
    c = R.fe_case(2, "speech")
    w = R.weights()
    ref, _ = R.fe_ref(c)
    row = 0
    for x, e in zip(R.fe_items(c), c["extras"]):
        T = R.windows_of(x.shape[0], e)
        feats = sv.encode_windows(w, sv.frame_windows(np.pad(x, (0, T * 512 - x.shape[0]))))
        want = feats @ w["lstm_w_ih"].astype(np.float64).T + w["lstm_b_ih"].astype(np.float64) + w["lstm_b_hh"].astype(np.float64)
        assert np.abs(ref[row:row + T] - want).max() < 1e-10
        row += T


@pytest.mark.parametrize("variant", R.FE_WRONGS)
def test_frontend_wrong_variant_leaves_the_bound(variant):
    case = FE_CAUGHT[variant]
    c = R.fe_case(*case)
    ref, b = R.fe_ref(c)
    ex = R.excess(R.fe_ref(c, variant=variant)[0], ref, b)
    print("frontend %s on %s: excess %.3g" % (variant, case, ex))
    assert ex > 1.0


@pytest.mark.parametrize("case", R.LSTM_CASES, ids=lambda c: "%s-%s-%s" % c)
def test_lstm_float32_run_is_inside_the_bound(case):
    ref, b = _packed(R.lstm_case(*case))
    assert np.isfinite(ref).all() and np.isfinite(b).all() and (b > 0).all()
    ex = R.excess(R.lstm_wrong(*case, None, np.float32), ref, b)
    print("lstm %s float32 excess %.4f, largest bound %.3g" % (case, ex, b.max()))
    assert ex <= 1.0


def test_lstm_reference_is_the_oracle_and_reaches_the_regimes():
    w = R.weights()
    gx, hs, _ = R.lstm_item_ref("base", "gauss", 65, 1)
    h = np.zeros(128)
    c = np.zeros(128)
    whh = w["lstm_w_hh"].astype(np.float64)
    for t in range(65):
        g = gx[t].astype(np.float64) + whh @ h
        i, f, gg, o = sv._sigmoid(g[:128]), sv._sigmoid(g[128:256]), np.tanh(g[256:384]), sv._sigmoid(g[384:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        assert np.abs(hs[t] - h).max() < 1e-13
    # "climb": c passes 44.4 (E(2c) = inf in float32) and h follows o
    gx, hs, _ = R.lstm_item_ref("base", "climb", 65, 1)
    _, _, (_, c_end) = R.lstm_ref(w, gx, want_bound=False)
    assert c_end.min() > 60
    assert np.abs(hs[50:] - sv._sigmoid(gx[50:, 384:].astype(np.float64) + hs[49:-1] @ whh[384:].T)).max() < 1e-12
    # "small_c": c stays near 1e-3; "sat100": every gate is 0 or 1 within the floor
    gx, hs, _ = R.lstm_item_ref("base", "small_c", 65, 1)
    assert 0 < np.abs(hs).max() < 2e-3
    gx, hs, _ = R.lstm_item_ref("base", "sat100", 65, 1)
    assert np.isin(np.round(hs, 6), np.round(np.tanh(np.arange(-65, 66)), 6)).all()


@pytest.mark.parametrize("variant", R.LSTM_WRONGS)
def test_lstm_wrong_variant_leaves_the_bound(variant):
    case = LSTM_CAUGHT[variant]
    ref, b = _packed(R.lstm_case(*case))
    ex = R.excess(R.lstm_wrong(*case, variant), ref, b)
    print("lstm %s on %s: excess %.3g" % (variant, case, ex))
    assert ex > 1.0


def test_whh_scale_is_admitted():
    """the factor of the second family: at the LAST of 65 steps the bound still separates the variants that act through W_hh, and the
    largest bound of the family's T = 65 items is below BOUND_TO_SIGNAL_MAX (h lies in (-1, 1))"""
    assert R.WHH_SCALE > 1
    worst = 0.0
    for case in R.LSTM_CASES:
        fam, pattern, ts = case
        if fam != "scaled" or ts == "table":
            continue
        k = R.LSTM_TS[ts].index(65)
        _, ref, b = R.lstm_case(*case)["items"][k]
        worst = max(worst, float(b.max()))
        if pattern == "gauss":
            lo = sum(R.LSTM_TS[ts][:k])
            for variant in ("gate_order_iofg", "whh_quarters"):
                wrong = R.lstm_wrong(fam, pattern, ts, variant)[lo + 64]
                ex = R.excess(wrong, ref[64], b[64])
                print("scaled %s %s at step 64: excess %.3g" % (ts, variant, ex))
                assert ex > 1.0
    print("W_hh x %g: largest bound of the T = 65 items %.3g (signal scale 1)" % (R.WHH_SCALE, worst))
    assert worst <= R.BOUND_TO_SIGNAL_MAX


@pytest.mark.parametrize("case", R.OUT_CASES, ids=lambda c: "T%d-r%d" % c)
def test_out_float32_run_is_inside_the_bound(case):
    c = R.out_case(*case)
    ref, b = R.out_ref(c)
    assert np.isfinite(ref).all() and (b > 0).all()
    assert R.excess(R.out_ref(c, np.float32)[0], ref, b) <= 1.0
    hs = c["hs"].reshape(c["T"], 128, 4)
    assert (hs[:, :, 0] < 0).any() and (hs[:, :, 1] != hs[:, :, 0]).all()      # negative entries; the copies differ


def test_out_cases_reach_the_stated_preactivations():
    w = R.weights()
    seen = set()
    for case in R.OUT_CASES:
        c = R.out_case(*case)
        x = np.maximum(c["hs"].reshape(c["T"], 128, 4)[:, :, 0].astype(np.float64), 0) @ w["out_w"].astype(np.float64) + float(w["out_b"][0])
        for t in range(c["T"]):
            want = R.OUT_TARGETS[(case[1] + t) % 6]
            if want is not None:
                assert abs(x[t] - want) < 1e-4
                seen.add(want)
    assert seen == {0.0, 20.0, -20.0, 100.0, -100.0}


@pytest.mark.parametrize("variant", R.OUT_WRONGS)
def test_out_wrong_variant_leaves_the_bound(variant):
    case = OUT_CAUGHT[variant]
    c = R.out_case(*case)
    ref, b = R.out_ref(c)
    ex = R.excess(R.out_ref(c, variant=variant)[0], ref, b)
    print("out %s on %s: excess %.3g" % (variant, case, ex))
    assert ex > 1.0
