"""GPU tests (-m gpu) of the kernels that produce the numbers the host thresholds, one launch each through the wlx_debug_token_prob /
_token_prob_rows / _lang_probs hooks: token_prob_kernel (no_speech_prob), token_prob_rows_kernel (word probabilities) and
lang_probs_kernel (detect_language) of search.hip, against the float64 softmax under the bound derived in tests/prob_kernel_ref.py
(tests/test_prob_kernel_ref.py shows on the host that one id more or fewer in the denominator, the wrong id set, a target off by one,
the wrong row stride and the neighbouring row all fall outside it). Every case: rc == 0, everything finite, excess = max |got - ref| /
bound <= 1, every output word no thread owns keeps its +-1000 fill (the hooks carry WLX_DEBUG_GUARD = 64 words behind the last owned
one in and out); rows are padded to ldl > V with +1000, so a read past V shows.
The data-movement kernels dec_embed_kernel, prep_window_kernel and f32_to_f16_kernel are compared bit for bit with numpy. Refusals:
every documented limit is WLX_ERR_ARG with the outputs unchanged. The last three tests tie the kernels to the engine's row and id
arithmetic on the tiny random-weight engine: the probabilities the product calls return against the float64 softmax of the engine's
own logits."""
import os

import numpy as np
import pytest

from . import prob_kernel_ref as R

pytestmark = pytest.mark.gpu
WLX_ERR_ARG = 1
_worst = {}


def _record(family, case, ex):
    """the measured margin per family, for the record only (profiles/prob_kernel_tests_excess.txt is the file a run with
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
                    "tests/test_gpu_prob_kernels.py on an MI355X. A record of the margin, not an input to any bound.\n")
            for fam in sorted(_worst):
                f.write("%-28s worst excess %.4f  at case %s\n" % (fam, _worst[fam][0], _worst[fam][1]))


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(a, b):
    return bool((_bits(np.ascontiguousarray(a)) == _bits(np.ascontiguousarray(b))).all())


# ------------------------------------------------------------------ the three softmax kernels
@pytest.mark.parametrize("case", R.TP_CASES, ids=lambda c: "V%d-r%d-%s" % c)
def test_token_prob(gpu, case):
    c = R.tp_case(*case)
    rc, out, init = R.run_tp(c)
    assert rc == 0
    ref, b = R.tp_ref(c)
    ex = R.excess(out[:c["rows"]], ref, b)
    print("token_prob %s tok %d excess %.4f" % (case, c["tok"], ex))
    _record("token_prob", case, ex)
    assert np.isfinite(out).all() and ex <= 1.0, ex
    assert out.size == c["rows"] + R.GUARD and _same_bits(out[c["rows"]:], init[c["rows"]:])


@pytest.mark.parametrize("case", R.TPR_CASES, ids=lambda c: "V%d-r%d-%s" % c)
def test_token_prob_rows(gpu, case):
    c = R.tpr_case(*case)
    for k in R.tpr_shifts(c["rows"], c["pattern"]):
        toks = R.tpr_targets(c["V"], c["rows"], k)
        rc, out, init = R.run_tpr(c, toks)
        assert rc == 0
        ref, b = R.tpr_ref(c, toks)
        rows = c["rows"]
        ex = R.excess(out[:rows], ref, b)
        print("token_prob_rows %s targets %s excess %.4f" % (case, toks[:5].tolist(), ex))
        _record("token_prob_rows", case + (k,), ex)
        assert np.isfinite(out).all() and ex <= 1.0, ex
        outside = (toks < 0) | (toks >= c["vlim"])
        assert (_bits(out[:rows][outside]) == 0).all()                        # -1, vlim and V - 1: exactly +0
        assert out.size == rows + R.GUARD and _same_bits(out[rows:], init[rows:])


@pytest.mark.parametrize("case", R.LP_CASES, ids=lambda c: "V%d-r%d-%s-n%d" % c)
def test_lang_probs(gpu, case):
    c = R.lp_case(*case)
    rc, out, init = R.run_lp(c)
    assert rc == 0
    ref, b = R.lp_ref(c)
    owned = c["rows"] * c["n"]
    ex = R.excess(out[:owned], ref, b)
    print("lang_probs %s excess %.4f" % (case, ex))
    _record("lang_probs", case, ex)
    assert np.isfinite(out).all() and ex <= 1.0, ex
    assert out.size == owned + R.GUARD and _same_bits(out[owned:], init[owned:])


def test_prob_refusals(gpu):
    big = (1 << 20) + 1
    c = R.tp_case(2310, 5, "gauss")
    for over in (dict(rows=0), dict(rows=65536), dict(tok=-1), dict(tok=2310), dict(ldl=2309), dict(V=0), dict(V=big, ldl=big, tok=0),
                 dict(rows=65535, ldl=1 << 13), dict(ldl=(1 << 28) + 1, rows=1), dict(null=("logits",)), dict(null=("out",))):
        rc, out, init = R.run_tp(c, **over)
        assert rc == WLX_ERR_ARG, over
        assert _same_bits(out, init)
    c = R.tpr_case(2310, 5, "gauss")
    toks = R.tpr_targets(2310, 5, 0)
    for over in (dict(rows=0), dict(rows=65536), dict(ldl=c["vlim"] - 1), dict(vlim=0), dict(vlim=big, ldl=big), dict(rows=65535, ldl=1 << 13),
                 dict(null=("logits",)), dict(null=("toks",)), dict(null=("out",))):
        rc, out, init = R.run_tpr(c, toks, **over)
        assert rc == WLX_ERR_ARG, over
        assert _same_bits(out, init)
    c = R.lp_case(2310, 5, "gauss", 99)
    lo, hi = c["ids"].copy(), c["ids"].copy()
    lo[7], hi[98] = -1, c["ldl"]
    for over in (dict(rows=0), dict(rows=65536), dict(n=0), dict(n=R.LANG_MAX + 1, ids=np.arange(R.LANG_MAX + 1)), dict(ids=lo), dict(ids=hi),
                 dict(ldl=0), dict(rows=65535, ldl=1 << 13), dict(null=("logits",)), dict(null=("ids",)), dict(null=("probs",))):
        rc, out, init = R.run_lp(c, **over)
        assert rc == WLX_ERR_ARG, list(over)
        assert _same_bits(out, init)


# ------------------------------------------------------------------ the exact kernels
@pytest.mark.parametrize("case", R.EMBED_CASES, ids=lambda c: "r%d-d%d" % c)
def test_dec_embed(gpu, case):
    c = R.embed_case(*case)
    rc, x, intok, (x0, intok0) = R.run_embed(c)
    assert rc == 0
    assert _same_bits(x.reshape(c["rows"], c["d"]), R.embed_ref(c["te"], c["pe"], c["tokens"], c["pos"]))
    want = intok0.reshape(c["rows"], 448).copy()
    want[np.arange(c["rows"]), c["pos"]] = c["tokens"]                        # the token each cache row was fed, and nothing else
    assert (intok.reshape(c["rows"], 448) == want).all()


def test_dec_embed_refusals(gpu):
    c = R.embed_case(5, 384)
    tk, ps = c["tokens"].copy(), c["pos"].copy()
    tk[2], ps[4] = R.EMBED_V, -1
    nulls = [dict(null=(n,)) for n in ("tok_emb", "pos_emb", "tokens", "pos", "x", "intok")]
    for over in [dict(d=382), dict(d=0), dict(d=8196), dict(rows=0), dict(rows=65536), dict(vocab=0), dict(vocab=(1 << 20) + 1),
                 dict(vocab=1 << 20, d=384), dict(n_pos=449), dict(n_pos=0), dict(n_pos=447), dict(vocab=R.EMBED_V - 1), dict(tokens=tk),
                 dict(pos=ps)] + nulls:
        rc, x, intok, (x0, intok0) = R.run_embed(c, **over)
        assert rc == WLX_ERR_ARG, list(over)
        assert _same_bits(x, x0) and (intok == intok0).all()


@pytest.mark.parametrize("case", R.PREP_CASES, ids=lambda c: "m%d-x%d-w%d" % c)
def test_prep_windows(gpu, case):
    c = R.prep_case(*case)
    rc, out, init = R.run_prep(c)
    assert rc == 0
    want = R.prep_ref(c, init)
    assert (out == want).all(), int((out != want).sum())
    nm = c["n_mels"]
    for i in range(c["items"]):
        w, w0 = (a[i * c["featT_stride"]:(i + 1) * c["featT_stride"]] for a in (out, init))
        assert (w[:nm] == w0[:nm]).all() and (w[3001 * nm:] == w0[3001 * nm:]).all()         # rows 0 and 3001 keep their fill
        assert (w[(1 + int(c["seg"][i])) * nm:3001 * nm] == 0).all()                           # frames seg <= t < 3000 are +0


def test_prep_windows_refusals(gpu):
    c = R.prep_case(80, 3, 3)
    sk, sg, sg2 = c["seek"].copy(), c["seg"].copy(), c["seg"].copy()
    sk[1], sg[0], sg2[2] = -1, 3001, c["ld"] - 122
    nulls = [dict(null=(n,)) for n in ("feats", "seek", "seg", "featT")]
    for over in [dict(n_mels=0), dict(n_mels=129), dict(items=0), dict(items=65), dict(seek=sk), dict(seg=sg), dict(seg=sg2),
                 dict(featT_stride=3002 * 80 - 1), dict(featT_stride=(1 << 28) // 3 + 1), dict(feats_len=c["feats"].size - c["ld"]),
                 dict(feats_len=(1 << 28) + 1), dict(ld=0), dict(ld=(1 << 28) + 1), dict(item_stride=-1), dict(item_stride=(1 << 28) + 1)] + nulls:
        rc, out, init = R.run_prep(c, **over)
        assert rc == WLX_ERR_ARG, list(over)
        assert (out == init).all()


@pytest.mark.parametrize("n", R.F16_NS)
def test_f32_to_f16(gpu, n):
    """fp16(float32) as numpy.float16: round to nearest even through the normal and subnormal ranges; past the fp16 range +-inf (from
    65520 on), which is also what the engine relies on: a token embedding outside fp16 must not come back as a finite value"""
    v = R.f16_values(n)
    cap = n + 3
    rc, out, init = R.run_f16(v, n, cap)
    assert rc == 0
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).view(np.uint16)
    assert (out[:n] == want).all(), np.flatnonzero(out[:n] != want)[:8]
    assert (out[n:] == init[n:]).all()


def test_f32_to_f16_refusals(gpu):
    v = R.f16_values(257)
    for n, cap, null in ((0, 8, ()), (-1, 8, ()), (257, 256, ()), ((1 << 28) + 1, (1 << 28) + 1, ()), (257, (1 << 28) + 1, ()), (257, 260, ("src",)),
                         (257, 260, ("dst",))):
        rc, out, init = R.run_f16(v, n, cap, alloc=300, null=null)
        assert rc == WLX_ERR_ARG, (n, cap, null)
        assert (out == init).all()


# ------------------------------------------------------------------ wiring: the product calls on the tiny random-weight engine
LANG = dict(threads=R.LP_THREADS, waves=R.LP_WAVES)          # lang_probs_kernel
TOKEN = dict(threads=R.SR_THREADS, waves=R.SR_WAVES)         # token_prob_kernel, token_prob_rows_kernel
SCAN3 = dict(threads=1, waves=0, sum_u=R.SCAN3_SUM_U)        # the beam search's own two-level sum (tests/prob_kernel_ref.py)


@pytest.fixture(scope="module")
def tiny(gpu):
    from tests import helpers as H
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    spec = H.TINY_EN
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7))
    yield spec, eng, H.token_ids_for(spec.vocab), H
    eng.close()


def _pcm(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1730 * t + 1.0) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def _soft(logits, sel, targets, kernel):
    """the float64 softmax of the engine's own logits rows and the bound of the kernel that computed the product's number"""
    logits = np.ascontiguousarray(logits, np.float32)
    return R.softmax_ref(logits.ravel(), logits.shape[1], logits.shape[0], sel, targets, admit=None, **kernel)


@pytest.mark.parametrize("batch", [1, 3])
def test_detect_language_is_the_softmax_of_the_slots_own_rows(tiny, batch):
    """Slot.detect_language against the float64 softmax over lang_ids of the slot's own logits rows, read back straight after: the row
    of every item and the id set, without network noise"""
    spec, eng, ids, H = tiny
    slot = eng.create_slot(batch, 5)
    try:
        Ts = [slot.logmel(_pcm((3 + b) * 16000, 8 + b), item=b) for b in range(batch)]
        slot.encode(batch, seek=[0] * batch, seg=[t - 1 for t in Ts])
        lang = np.random.default_rng(batch).permutation(np.arange(ids.sot + 1, ids.sot + 100))
        got = slot.detect_language(batch, ids.sot, lang)
        lg = slot.debug_logits(batch)
        ref, b = _soft(lg, lang, np.tile(lang, (batch, 1)), LANG)
        ex = R.excess(got, ref, b)
        print("detect_language batch %d excess %.4f" % (batch, ex))
        _record("wiring_detect_language", batch, ex)
        assert ex <= 1.0, ex
        if batch > 1:
            assert not np.array_equal(got[0], got[1])
    finally:
        slot.close()


def _logits_noise(slot, prompt, sot, monkeypatch):
    """the teacher-forced logits of `prompt`, and max |dl| between logits sets of the same input that came through different pass
    shapes (each of them is checked against the float64 oracle in tests/test_gpu_parity.py): the prompt prefilled 48 rows at a time and
    16 at a time, and the row of [sot] alone from a decode step (wlx_detect_language's pass) and from a prefill"""
    a = slot.debug_decode_logits(prompt)
    monkeypatch.setenv("WLX_PREFILL_ROWS", "16")
    b = slot.debug_decode_logits(prompt)
    monkeypatch.delenv("WLX_PREFILL_ROWS")
    slot.detect_language(1, sot, [sot + 1])
    step = slot.debug_logits(1)[0].astype(np.float64)
    pre = slot.debug_decode_logits([sot])[0]
    return a, max(float(np.abs(a.astype(np.float64) - b).max()), float(np.abs(step - pre).max()))


@pytest.mark.parametrize("n_prev,chunk", [(0, None), (100, None), (20, "16")], ids=["sot_last", "behind_100", "row_5_of_the_second_chunk"])
def test_no_speech_prob_is_the_softmax_of_the_sot_row(tiny, n_prev, chunk, monkeypatch):
    """no_speech_prob of a generate against the float64 softmax of the start-of-transcript row of wlx_debug_decode_logits on the same
    prompt, under the bound of the kernel that computes it:
      * the prompt ends on start-of-transcript: the beam search of the first step (search_scan3 + search_merge_update3);
      * start-of-transcript behind start-of-previous and 100 previous-text tokens: the one-pass prefill projects that one row and
        token_prob_kernel reads it;
      * behind 20 previous-text tokens with the prefill cut into 16-row chunks: token_prob_kernel on row nsp_index - c0 = 21 - 16 of the
        second chunk's logits.
    Those logits may come from another pass shape than the generate's, so they need not be bit-identical: a logit off by dl moves p
    by at most a relative exp(2 max |dl|) - 1 (numerator and denominator by exp(+-dl) each), with max |dl| measured between passes
    of different shapes and added to the kernel bound."""
    spec, eng, ids, H = tiny
    slot = eng.create_slot(1, 5)
    try:
        T = slot.logmel(_pcm(5 * 16000, 4))
        slot.encode(1, seek=[0], seg=[T - 1])
        prev = np.random.default_rng(5).integers(300, 20000, size=n_prev).tolist()
        sot_prev = ids.timestamp_begin - 3
        prompt = ([sot_prev] + prev if n_prev else []) + [ids.sot] + ([ids.sot + 1, ids.sot + 2] if n_prev else [])
        sot_at = prompt.index(ids.sot)
        lg, dl = _logits_noise(slot, prompt, ids.sot, monkeypatch)
        if chunk:
            monkeypatch.setenv("WLX_PREFILL_ROWS", chunk)
            assert sot_at > int(chunk) and len(prompt) - 1 <= 48
            lg = slot.debug_decode_logits(prompt)                             # (the rows as this chunking computes them)
        res = slot.generate([prompt], H.engine_ids(ids), beam_size=5, max_length=len(prompt) + 6, suppress_tokens=H.default_suppress(ids))[0]
        kernel = TOKEN if n_prev else SCAN3
        ref, b = _soft(lg[sot_at:sot_at + 1], spec.vocab, [[ids.no_speech]], kernel)
        bound = b[0, 0] + ref[0, 0] * np.expm1(2 * dl)
        err = abs(res.no_speech_prob - ref[0, 0])
        print("no_speech_prob n_prev %d chunk %s: got %.9g ref %.9g max|dl| %.3g kernel bound %.3g + logits %.3g, excess %.4f" % (
            n_prev, chunk, res.no_speech_prob, ref[0, 0], dl, b[0, 0], ref[0, 0] * np.expm1(2 * dl), err / bound))
        _record("wiring_no_speech_prob", (n_prev, chunk), err / bound)
        assert err <= bound, (err, bound)
        beside = [abs(_soft(lg[r:r + 1], spec.vocab, [[ids.no_speech]], kernel)[0][0, 0] - ref[0, 0])
                  for r in (sot_at - 1, sot_at + 1) if 0 <= r < len(prompt)]
        assert not beside or min(beside) > bound                              # the rows next to it answer something else
    finally:
        slot.close()


def test_align_word_probabilities_are_the_softmax_below_eot(tiny, monkeypatch):
    """text_token_probs of wlx_align on a 12-token text against the float64 softmax over [0, eot) of the teacher-forced rows of
    wlx_debug_decode_logits, under the same rule as above"""
    spec, eng, ids, H = tiny
    slot = eng.create_slot(1, 5)
    try:
        T = slot.logmel(_pcm(8 * 16000, 12))
        slot.encode(1, seek=[0], seg=[T - 1])
        text = np.random.default_rng(12).integers(300, ids.eot - 1, size=12).tolist()
        tokens = [ids.sot, ids.no_timestamps] + text + [ids.eot]
        heads = [(l, h) for l in range(spec.dec_layers // 2, spec.dec_layers) for h in range(spec.n_heads)]
        _, _, probs = slot.align(tokens, 1, T - 1, heads, ids.eot, median_filter_width=7)
        lg, dl = _logits_noise(slot, tokens, ids.sot, monkeypatch)
        rows = lg[1:1 + len(text)]                                            # row n_sot + i predicts text token i
        ref, b = _soft(rows, ids.eot, np.asarray(text).reshape(-1, 1), TOKEN)
        bound = b[:, 0] + ref[:, 0] * np.expm1(2 * dl)
        ex = float((np.abs(probs - ref[:, 0]) / bound).max())
        print("align word probabilities: max|dl| %.3g, excess %.4f" % (dl, ex))
        _record("wiring_align_probs", len(text), ex)
        assert ex <= 1.0, ex
        whole = _soft(rows, spec.vocab, np.asarray(text).reshape(-1, 1), TOKEN)[0][:, 0]
        shifted = _soft(lg[2:2 + len(text)], ids.eot, np.asarray(text).reshape(-1, 1), TOKEN)[0][:, 0]
        assert (np.abs(whole - ref[:, 0]) > bound).all() and (np.abs(shifted - ref[:, 0]) > bound).any()
    finally:
        slot.close()
