"""GPU (-m gpu): the production search launches (search.hip: search_scan3_kernel + search_merge_update3_kernel in beam mode,
search_rows_kernel + search_update_kernel when sampling) on INJECTED logits, through wlx_debug_search_batch — beam widths 6 .. 16 and
several items in one call — against oracle/decoding.py: tokens exact, scores at rtol = atol = 1e-3. The cases and their oracle answers
are tests/search_cases.py; tests/test_search_cases_host.py shows that every deciding pair of scores in them is more than 1e-3 apart,
so no mismatch here is a near-tie.

Two engines: the micro model (vocabulary 2310: one text and one timestamp scan chunk) and a two-layer model with the multilingual
vocabulary (51865: 26 scan chunks, the last text chunk ragged). No encode: the search never touches the network."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import search_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import WhisperSpec
    from whisperlive_amd.weights import random_weights
    full = WhisperSpec(n_mels=80, d_model=768, n_heads=12, enc_layers=1, dec_layers=2, ffn=3072, vocab=SC.VOCAB["full"])
    assert H.MICRO.vocab == SC.VOCAB["micro"]
    engs = {"micro": HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3)), "full": HipWhisperEngine(full, random_weights(full, seed=11))}
    yield engs
    for e in engs.values():
        e.close()


def _names(*prefixes, vocab=None):
    return sorted(n for n, c in SC.CASES.items() if n.startswith(prefixes) and (vocab is None or c.vocab == vocab))


def _run(slot, name, lg=None):
    c = SC.CASES[name]
    lg = c.logits() if lg is None else lg
    return slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)


def _check(got, name):
    """every item: the hypotheses returned, in order, token for token; scores to 1e-3 (sampling rows: as sets, they finish in any order)"""
    c, ref = SC.CASES[name], SC.answer(name).results
    assert len(got) == len(ref) == c.items
    sampling = c.kw.get("sampling_temperature", 0.0) > 0 or c.kw["beam_size"] <= 1
    for b, (g, r) in enumerate(zip(got, ref)):
        keep = [i for i, s in enumerate(r.scores) if np.isfinite(s)]
        rs, rq = [r.scores[i] for i in keep], [r.sequences_ids[i] for i in keep]
        print(name, "item", b, "gpu", g.scores[:3], "oracle", rs[:3], "tokens", len(rq[0]) if rq else None)
        if sampling:
            assert sorted(map(tuple, g.sequences_ids)) == sorted(map(tuple, rq)), (name, b, g.sequences_ids, rq)
            np.testing.assert_allclose(sorted(g.scores), sorted(rs), rtol=1e-3, atol=1e-3)
        else:
            assert g.sequences_ids == rq, (name, b, g.sequences_ids, rq)
            np.testing.assert_allclose(g.scores, rs, rtol=1e-3, atol=1e-3)


# ---- a. beam widths, one item
@pytest.mark.parametrize("name", _names("beam6-", "beam7-", "beam8-", "beam9-", "beam12-", "beam16-gauss", "beam16-quant", "beam16-patience2-"))
def test_wide_beam_equals_oracle(engines, name):
    """6: the last width of one merge trip and three list quads; 7: a second trip (fresh loads into the wave's list again) and a fourth
    quad; 8: the last with 2 * beam <= 16; 9: the first whose four wave lists need the second candidate register of the scan's merge;
    12 with six allowed ids at the first step: exhausted lists; 16: 32 candidates per row, 128 wave-list entries, and with patience 2 the
    whole hypothesis store (16 returned)."""
    c = SC.CASES[name]
    slot = engines[c.vocab].create_slot(1, 16)
    try:
        _check(_run(slot, name), name)
    finally:
        slot.close()


# ---- b. several items, beam mode
@pytest.mark.parametrize("name", _names("batch"))
def test_batched_beam_equals_oracle_and_singles(engines, name):
    """Prompts of 1 / 4 / 9 tokens (per-item plen, position and last step), an item that ends at the second step while the others run
    (item_done, the done word only with the last item), one that runs into max_length; the option cases walk the history through
    rows that are not item 0's. Every item equals the oracle, and — the same kernels on the same rows — debug_search of its rows alone,
    bit for bit."""
    c = SC.CASES[name]
    eng = engines[c.vocab]
    slot, one = eng.create_slot(c.items, 16), eng.create_slot(1, 16)
    try:
        lg = c.logits()
        got = _run(slot, name, lg)
        _check(got, name)
        for b in range(c.items):
            alone = one.debug_search(c.item_logits(lg, b), c.prompts[b], H.engine_ids(c.ids), **c.gen_kw)
            assert alone.sequences_ids == got[b].sequences_ids, (name, b)
            assert alone.scores == got[b].scores, (name, b, alone.scores, got[b].scores)
    finally:
        slot.close()
        one.close()


# ---- c. several items, sampling pair
@pytest.mark.parametrize("name", _names("sample3x5", "greedy4"))
def test_batched_sampling_equals_oracle(engines, name):
    """search_rows_kernel + search_update_kernel with rows that are not item 0's: the draw is keyed on (row, position) with the row counted
    over the whole call (the oracle's row_base = b * R); the same call twice gives the same bits; items 0 and 1 of the sampling case have
    the same logits and prompt and draw different sequences."""
    c = SC.CASES[name]
    slot = engines[c.vocab].create_slot(c.items, 16)
    try:
        lg = c.logits()
        got = _run(slot, name, lg)
        _check(got, name)
        again = _run(slot, name, lg)
        assert [(g.sequences_ids, g.scores) for g in again] == [(g.sequences_ids, g.scores) for g in got]
        if c.same_as:
            assert sorted(map(tuple, got[0].sequences_ids)) != sorted(map(tuple, got[1].sequences_ids))
    finally:
        slot.close()


# ---- d. state between calls on one slot
@pytest.mark.parametrize("order", [
    ("batch5x5-micro", "batch2x5-micro", "batch5x5-micro"),                 # the per-item words of a wider call must not leak into a narrower one, and back
    ("beam16-gauss-micro", "batch3x5-micro", "beam16-patience2-micro"),     # 16 rows per item, then 5, then a full hypothesis store
    ("batch3x5-micro", "sample3x5-micro", "batch3x5-keep-blank"),           # the sampling pair between two beam calls (row_done, rule state)
    ("batch3x8-full", "greedy4-full", "batch2x16-full"),
])
def test_calls_on_one_slot_do_not_see_each_other(engines, order):
    slot = engines[SC.CASES[order[0]].vocab].create_slot(5, 16)
    try:
        for name in order:
            _check(_run(slot, name), name)
    finally:
        slot.close()


# ---- e. refusals
def _raw(slot, lg, steps, batch, pr, pl, stride, o, toks, nt, sc):
    from whisperlive_amd.engine import _f32p, _i32p
    p = lambda a, f: None if a is None else f(a)
    return slot.lib.wlx_debug_search_batch(slot.engine._h, slot.sid, p(lg, _f32p), steps, batch, p(pr, _i32p), p(pl, _i32p), stride,
                                           None if o is None else C.byref(o), p(toks, _i32p), 448, p(nt, _i32p), p(sc, _f32p))


def test_refusals_leave_outputs_and_slot_untouched(engines):
    """null arguments, batch < 1 or above the slot's items, steps < 1, and what generate itself refuses (rows, prompt length, a token outside
    the vocabulary): WLX_ERR_ARG, the three output arrays as they were, and a valid call right after gives the oracle's answer."""
    from whisperlive_amd import _lib
    name = "batch2x5-micro"
    c = SC.CASES[name]
    slot = engines["micro"].create_slot(2, 5)
    try:
        lg = c.logits()
        o, keep = slot._opts(H.engine_ids(c.ids), **dict(dict(beam_size=5, patience=1.0, num_hypotheses=1, length_penalty=1.0, repetition_penalty=1.0,
                                                               no_repeat_ngram_size=0, max_length=448, suppress_blank=True, suppress_tokens=(),
                                                               max_initial_timestamp_index=50, sampling_topk=0, sampling_temperature=0.0, seed=0), **c.gen_kw))
        stride = max(c.plens)
        pr = np.zeros((2, stride), dtype=np.int32)
        for i, p in enumerate(c.prompts):
            pr[i, :len(p)] = p
        pl = np.asarray(c.plens, dtype=np.int32)
        toks = np.full((2, 1, 448), -7, dtype=np.int32); nt = np.full((2, 1), -7, dtype=np.int32); sc = np.full((2, 1), -7.0, dtype=np.float32)
        good = dict(lg=lg, steps=lg.shape[0], batch=2, pr=pr, pl=pl, stride=stride, o=o, toks=toks, nt=nt, sc=sc)
        wide = slot._opts(H.engine_ids(c.ids), **dict(dict(beam_size=6, patience=1.0, num_hypotheses=1, length_penalty=1.0, repetition_penalty=1.0,
                                                           no_repeat_ngram_size=0, max_length=c.kw["max_length"], suppress_blank=True, suppress_tokens=(),
                                                           max_initial_timestamp_index=50, sampling_topk=0, sampling_temperature=0.0, seed=0)))[0]
        long_pl = pl.copy(); long_pl[1] = c.kw["max_length"]
        bad_tok = pr.copy(); bad_tok[1, 0] = c.V
        bad = [dict(lg=None), dict(pr=None), dict(pl=None), dict(o=None), dict(toks=None), dict(nt=None), dict(sc=None),
               dict(batch=0), dict(batch=-1), dict(batch=3), dict(steps=0), dict(steps=-2),
               dict(o=wide),                     # six rows per item on a slot of five
               dict(pl=long_pl), dict(pl=np.asarray([1, 0], dtype=np.int32)), dict(pr=bad_tok)]
        for change in bad:
            rc = _raw(slot, **dict(good, **change))
            assert rc == _lib.ERR_ARG, (list(change), rc)
            assert (toks == -7).all() and (nt == -7).all() and (sc == -7.0).all(), list(change)
            _check(_run(slot, name, lg), name)
        assert _raw(slot, **good) == 0 and nt[0, 0] == len(SC.answer(name).results[0].sequences_ids[0])
    finally:
        slot.close()


def test_patience_beyond_the_hypothesis_limit_is_refused(engines):
    """beam 16 with patience 2.5 waits for round(16 * 2.5) = 40 finished hypotheses; the engine ranks up to 32 asked for (plus what the last step
    adds). With a store of 32 and no check the search ran on and returned other hypotheses than the oracle (its 3rd score -0.909 against
    -0.861): the options are refused, with the limit in the message, outputs untouched; patience 2.0 on the same slot right after is exact."""
    from whisperlive_amd import _lib
    c = SC.CASES["beam16-patience2.5-micro"]
    assert SC.answer(c.name).n_hyps[0] >= 40                       # the oracle does collect them: the case is a real request
    slot = engines["micro"].create_slot(1, 16)
    try:
        with pytest.raises(_lib.WlxError) as ei:
            _run(slot, c.name)
        assert ei.value.code == _lib.ERR_ARG and "32" in str(ei.value) and "40" in str(ei.value), str(ei.value)
        lg = c.logits()
        d = dict(beam_size=5, patience=1.0, num_hypotheses=1, length_penalty=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, max_length=448,
                 suppress_blank=True, suppress_tokens=(), max_initial_timestamp_index=50, sampling_topk=0, sampling_temperature=0.0, seed=0)
        o, keep = slot._opts(H.engine_ids(c.ids), **dict(d, **c.gen_kw))
        pr, pl = np.asarray(c.prompts, dtype=np.int32), np.asarray(c.plens, dtype=np.int32)
        toks = np.full((1, 16, 448), -7, dtype=np.int32); nt = np.full((1, 16), -7, dtype=np.int32); sc = np.full((1, 16), -7.0, dtype=np.float32)
        assert _raw(slot, lg, lg.shape[0], 1, pr, pl, 1, o, toks, nt, sc) == _lib.ERR_ARG
        assert (toks == -7).all() and (nt == -7).all() and (sc == -7.0).all()
        _check(_run(slot, "beam16-patience2-micro"), "beam16-patience2-micro")
    finally:
        slot.close()
