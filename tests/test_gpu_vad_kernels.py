"""GPU tests (-m gpu) of the three Silero VAD kernels of csrc/vad.hip, one launch each through the wlx_vad_debug_frontend / _lstm / _out
hooks on the weights as wlx_vad_create repacked them, against the float64 references under the bounds derived in
tests/vad_kernel_ref.py (tests/test_vad_kernel_ref.py shows on the host that every wrong variant leaves them). Every case: rc == 0,
everything finite, excess = max |got - ref| / bound <= 1, the canary rows and the WLX_DEBUG_GUARD words behind the items' own rows keep
their +-1000 fill, an item's rows have the same bits alone and inside the ragged launch, and in hs the four copies of a unit are
bit-equal. The wiring test chains the three hooks and asks for the bits of wlx_vad_probs_batch; one end-to-end clip runs the second
weight family against oracle/silero_vad.py; every refusal is WLX_ERR_ARG with the output unchanged."""
import os

import numpy as np
import pytest

from oracle import silero_vad as sv
from . import vad_kernel_ref as R

pytestmark = pytest.mark.gpu
WLX_ERR_ARG = 1
CANARY_ROWS = 2
E2E_SEED, E2E_MARGIN = 17, 8.0
_worst = {}


def _record(stage, case, ex):
    """the measured margin per stage, for the record only (profiles/vad_kernel_tests_excess.txt is the file a run with WLX_EXCESS_OUT set
    writes, header included); no bound reads it"""
    if ex > _worst.get(stage, (-1.0, None))[0]:
        _worst[stage] = (ex, case)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("WLX_EXCESS_OUT")
    if path and _worst:
        with open(path, "w") as f:
            f.write("max over elements of |kernel - float64 reference| / derived bound, worst case per stage, from one run of\n"
                    "tests/test_gpu_vad_kernels.py on an MI355X. A record of the margin, not an input to any bound.\n")
            for stage in sorted(_worst):
                f.write("%-28s worst excess %.4f  at case %s\n" % (stage, _worst[stage][0], _worst[stage][1]))


@pytest.fixture(scope="module")
def models(gpu):
    ms = {f: R.make_model(f) for f in R.LSTM_FAMILIES}
    yield ms
    for m in ms.values():
        m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


@pytest.mark.parametrize("case", R.FE_CASES, ids=lambda c: "s%d-%s" % c)
def test_frontend(models, case):
    m = models["base"]
    c = R.fe_case(*case)
    rows = sum(c["T"])
    rc, out, init = R.run_frontend(m, c["pcm"], c["counts"], c["extras"], rows + CANARY_ROWS)
    assert rc == 0
    gx = out[:rows * 512].reshape(rows, 512)
    ref, b = R.fe_ref(c)
    ex = R.excess(gx, ref, b)
    print("frontend %s excess %.4f" % (case, ex))
    _record("frontend", case, ex)
    assert np.isfinite(gx).all() and ex <= 1.0, ex
    assert _same(out[rows * 512:], init[rows * 512:])                       # the canary rows and the guard words
    silent = R.fe_silent_rows(c)
    assert all(_same(gx[r], gx[silent[0]]) for r in silent)                 # every all-zero window gives the same row
    row, start = 0, 0
    for n, e, T in zip(c["counts"], c["extras"], c["T"]):                   # the item alone: a launch of one item
        rc, one, init1 = R.run_frontend(m, c["pcm"][start:start + n], [n], [e], T + CANARY_ROWS)
        assert rc == 0 and _same(one[:T * 512], out[row * 512:(row + T) * 512]), (n, e)
        assert _same(one[T * 512:], init1[T * 512:])
        row, start = row + T, start + n


@pytest.mark.parametrize("case", R.LSTM_CASES, ids=lambda c: "%s-%s-%s" % c)
def test_lstm(models, case):
    m = models[case[0]]
    c = R.lstm_case(*case)
    Ts = c["Ts"]
    rows = sum(Ts)
    gx = np.concatenate([it[0] for it in c["items"]])
    rc, out, init = R.run_lstm(m, gx, Ts, rows + CANARY_ROWS)
    assert rc == 0
    hs = out[:rows * 512].reshape(rows, 128, 4)
    assert all(_same(hs[:, :, k], hs[:, :, 0]) for k in (1, 2, 3))          # the four copies of a unit
    ref = np.concatenate([it[1] for it in c["items"]])
    b = np.concatenate([it[2] for it in c["items"]])
    ex = R.excess(hs[:, :, 0], ref, b)
    print("lstm %s excess %.4f" % (case, ex))
    _record("lstm", case, ex)
    assert np.isfinite(hs).all() and ex <= 1.0, ex
    assert _same(out[rows * 512:], init[rows * 512:])
    row = 0
    for (g, _, _), T in zip(c["items"], Ts):
        rc, one, init1 = R.run_lstm(m, g, [T], T + CANARY_ROWS)
        assert rc == 0 and _same(one[:T * 512], out[row * 512:(row + T) * 512]), row
        assert _same(one[T * 512:], init1[T * 512:])
        row += T


@pytest.mark.parametrize("case", R.OUT_CASES, ids=lambda c: "T%d-r%d" % c)
def test_out(models, case):
    c = R.out_case(*case)
    T = c["T"]
    rc, out, init = R.run_out(models["base"], c["hs"], T, T + 3)
    assert rc == 0
    ref, b = R.out_ref(c)
    ex = R.excess(out[:T], ref, b)
    print("out %s excess %.4f" % (case, ex))
    _record("out", case, ex)
    assert np.isfinite(out[:T]).all() and ex <= 1.0, ex
    assert _same(out[T:], init[T:])


def test_the_pass_is_the_three_hooks_chained(models):
    """wlx_vad_probs_batch on a ragged set has the bits of the three launches run one by one on the same inputs"""
    from whisperlive_amd.synthetic import speech_like_pcm
    m = models["base"]
    src = speech_like_pcm(1.0, seed=23)
    counts = [1, 513, 2049, 512, 700]
    clips = [src[31 * i: 31 * i + n].copy() for i, n in enumerate(counts)]
    want = np.concatenate(m.probs_many(clips))
    extras = [1 if n % 512 == 0 else 0 for n in counts]                     # probs_many pads to the NEXT multiple of 512
    Ts = [R.windows_of(n, e) for n, e in zip(counts, extras)]
    rows = sum(Ts)
    assert want.shape == (rows,)
    rc, gx, _ = R.run_frontend(m, np.concatenate(clips), counts, extras, rows)
    assert rc == 0
    rc, hs, _ = R.run_lstm(m, gx[:rows * 512], Ts, rows)
    assert rc == 0
    rc, probs, _ = R.run_out(m, hs[:rows * 512], rows, rows)
    assert rc == 0
    assert _same(probs[:rows], want)


def test_scaled_family_end_to_end_against_the_oracle(models):
    """the whole pass with W_hh x WHH_SCALE on 3 s of speech-like audio. The tolerance is the oracle's own float32-versus-float64 gap on
    this clip times E2E_MARGIN = 8 (the kernels add in other orders than numpy's float32 sums, whose error is one sample of the same
    distribution, not its maximum), plus 2^-24: the oracle rounds its float64 probabilities to float32."""
    from whisperlive_amd.synthetic import speech_like_pcm
    w = R.weights("scaled")
    x = speech_like_pcm(3.0, seed=E2E_SEED)[:48000 - 512 + 100]
    padded = np.pad(x, (0, 512 - x.shape[0] % 512))
    assert padded.shape[0] <= 48000
    p64 = sv.speech_probs(w, padded)
    gap = float(np.abs(sv.speech_probs(w, padded, np.float32).astype(np.float64) - p64).max())
    print("oracle float32 / float64 gap %.3g" % gap)
    assert 0 < gap <= 1e-4                     # (a clip on which the gap is larger is no yardstick: take another seed, never a wider margin)
    got = models["scaled"](padded)
    err = float(np.abs(got.astype(np.float64) - p64).max())
    print("end to end: error %.3g, tolerance %.3g" % (err, E2E_MARGIN * gap + 2.0 ** -24))
    _record("end_to_end_scaled", E2E_SEED, err / (E2E_MARGIN * gap + 2.0 ** -24))
    assert got.shape == p64.shape and np.isfinite(got).all()
    assert err <= E2E_MARGIN * gap + 2.0 ** -24


# ------------------------------------------------------------------ refusals: WLX_ERR_ARG, nothing written
def test_frontend_refusals_write_nothing(models):
    m = models["base"]
    pcm = np.zeros(4096, np.float32)
    ok = dict(pcm=pcm, counts=[1000, 513], extras=[0, 1], cap=5)
    cases = {
        "n = 0": dict(n=0), "n = 65": dict(counts=[10] * 65, extras=[0] * 65, cap=100), "cap one short": dict(cap=4), "cap = 0": dict(cap=0),
        "cap = -1": dict(cap=-1), "negative count": dict(counts=[1000, -1]),
        "extra = 5": dict(extras=[0, 5], cap=16), "extra = -1": dict(extras=[-1, 0], cap=16),
        "null pcm": dict(null=("pcm",)), "null counts": dict(null=("counts",)), "null gx": dict(null=("gx",)), "null object": dict(null=("v",)),
    }
    for name, kw in cases.items():
        a = dict(ok)
        a.update(kw)
        rc, out, init = R.run_frontend(m, a.pop("pcm"), a.pop("counts"), a.pop("extras"), a.pop("cap"), **a)
        assert rc == WLX_ERR_ARG, name
        assert _same(out, init), name
    rc, out, init = R.run_frontend(m, pcm, ok["counts"], None, 4)            # null extras: none; 2 + 2 windows fit
    assert rc == 0 and not _same(out[:4 * 512], init[:4 * 512]) and _same(out[4 * 512:], init[4 * 512:])
    rc, out, init = R.run_frontend(m, pcm, [0, 0], [0, 0], 1)                # no window: nothing is launched
    assert rc == 0 and _same(out, init)


def test_lstm_refusals_write_nothing(models):
    m = models["base"]
    gx = np.zeros((5, 512), np.float32)
    ok = dict(Ts=[2, 3], cap=5)
    cases = {
        "n = 0": dict(n=0), "n = 65": dict(Ts=[0] * 65, cap=100), "cap one short": dict(cap=4), "cap = 0": dict(cap=0),
        "negative count": dict(Ts=[2, -1]), "null gx": dict(null=("gx",)), "null T": dict(null=("T",)), "null hs": dict(null=("hs",)),
        "null object": dict(null=("v",)),
    }
    for name, kw in cases.items():
        a = dict(ok)
        a.update(kw)
        rc, out, init = R.run_lstm(m, gx, a.pop("Ts"), a.pop("cap"), **a)
        assert rc == WLX_ERR_ARG, name
        assert _same(out, init), name
    rc, out, init = R.run_lstm(m, gx, [2, 0, 3], 5)                          # an item without a window takes no part
    assert rc == 0 and _same(out[5 * 512:], init[5 * 512:]) and np.isfinite(out[:5 * 512]).all()


def test_out_refusals_write_nothing(models):
    m = models["base"]
    hs = np.zeros((4, 512), np.float32)
    for name, kw in {"cap one short": dict(T=4, cap=3), "cap = 0": dict(T=0, cap=0), "negative count": dict(T=-1, cap=4),
                     "null hs": dict(T=4, cap=4, null=("hs",)), "null probs": dict(T=4, cap=4, null=("probs",)),
                     "null object": dict(T=4, cap=4, null=("v",))}.items():
        rc, out, init = R.run_out(m, hs, kw["T"], kw["cap"], kw.get("null", ()))
        assert rc == WLX_ERR_ARG, name
        assert _same(out, init), name
    rc, out, init = R.run_out(m, hs, 0, 4)
    assert rc == 0 and _same(out, init)
