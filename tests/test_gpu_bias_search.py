"""GPU (-m gpu): keyword boosting inside the production search launches, on INJECTED logits through wlx_debug_search_batch with a bias table
installed on the slot (Slot.set_bias), against oracle.decoding.generate driven by a test-side LogitsProvider that tracks every row's
automaton state through `parents` and adds the bias with biasing.BiasTable.bias_row. Tokens exact, scores at the tolerance of
tests/test_gpu_search_batch.py (rtol = atol = 1e-3); every case's deciding scores are more than that apart in the oracle (asserted here).
Boost and values are exact in float32. The cases reuse the seeded logits of tests/search_cases.py."""
import numpy as np
import pytest

from oracle import decoding as odec
from tests import helpers as H
from tests import search_cases as SC
from whisperlive_amd import biasing as B

pytestmark = pytest.mark.gpu

V = SC.VOCAB["micro"]
IDS = SC.token_ids(V)
BOOST = 16.0                 # against logits of sigma 4 (the best of 2310 draws sits near 14): a boosted token competes, it does not always win
PHRASES = [[31, 57, 123], [57, 300], [31, 57], [411]]     # overlap (31 57 then 300 completes `57 300`), a prefix of another, a single token
LOGIT_BIAS = {640: 4.0, 57: -2.0, IDS.timestamp_begin + 3: 2.0, IDS.eot: -0.5}


def table():
    return B.compile_bias(PHRASES, BOOST, LOGIT_BIAS, vocab=V, eot=IDS.eot)


class BiasedLogits(odec.InjectedLogits):
    """injected logits + the bias of each row's node: the node follows `parents`. `sot_last`: row 0 of the first step stays raw, as the
    row that defines no_speech_prob inside the search does in wlx_generate; the injected-logits hook runs no prefill and marks no such
    row, so the cases here pass False (the untouched row is tests/test_gpu_bias_kernel.py's and tests/test_gpu_keyword_bias.py's)"""

    def __init__(self, logits, tab, sot_last=False):
        super().__init__(logits)
        self.tab, self.sot_last, self.states = tab, sot_last, None
        self.visited, self.ts_resets = set(), 0

    def step(self, tokens, parents):
        first = self.states is None
        if first:
            self.states = [0] * len(tokens)
        else:
            new = [self.tab.next_state(self.states[p], t) for p, t in zip(parents, tokens)]
            self.ts_resets += sum(1 for p, t in zip(parents, tokens) if self.states[p] != 0 and t >= IDS.timestamp_begin)
            self.states = new
        self.visited.update(self.states)
        out = np.array(super().step(tokens, parents), dtype=np.float32, copy=True)
        for r, s in enumerate(self.states):
            if not (first and self.sot_last and r == 0):
                self.tab.bias_row(out[r], s)
        return out


def oracle_answer(c, lg, tab):
    res, margin, provs = [], float("inf"), []
    o = c.opts()
    beam_mode = not (o.sampling_temperature > 0 or o.beam_size <= 1)
    for b, prompt in enumerate(c.prompts):
        w = SC._Watch(c.R, max(1, o.num_hypotheses), c.ids.eot) if beam_mode else None
        prov = BiasedLogits(c.item_logits(lg, b), tab)
        res.append(odec.generate(prov, prompt, o, row_base=b * c.R, observer=w))
        provs.append(prov)
        if w is not None:
            margin = min(margin, w.margin)
    return res, margin, provs


def check(got, ref, sampling):
    for b, (g, r) in enumerate(zip(got, ref)):
        keep = [i for i, s in enumerate(r.scores) if np.isfinite(s)]
        rs, rq = [r.scores[i] for i in keep], [r.sequences_ids[i] for i in keep]
        print("item", b, "gpu", g.scores[:3], "oracle", rs[:3], "tokens", rq[0] if rq else None)
        if sampling:
            assert sorted(map(tuple, g.sequences_ids)) == sorted(map(tuple, rq)), (b, g.sequences_ids, rq)
            np.testing.assert_allclose(sorted(g.scores), sorted(rs), rtol=1e-3, atol=1e-3)
        else:
            assert g.sequences_ids == rq, (b, g.sequences_ids, rq)
            np.testing.assert_allclose(g.scores, rs, rtol=1e-3, atol=1e-3)


# the lift of the planted phrase per case: where the first value (6.0) left two deciding scores of the biased oracle closer than
# SC.MARGIN another one was taken (scanned in steps of 0.5), the margin never widened
LIFT = {"batch3x5-micro": 5.5, "batch5x5-micro": 5.5, "batch2x5-micro": 5.5}


def planted(c, lg):
    """the case's logits with a phrase planted along the way: from the second step on the phrase tokens are lifted so that some beams walk
    `31 57` and split into `123` / `300`, and one step favours a timestamp behind `31` (a timestamp in the middle of a phrase)"""
    lg = lg.copy()
    lg[1:, :, 31] += np.float32(LIFT.get(c.name, 6.0))
    lg[2:, :, [57, 123, 300]] += 3.0
    if lg.shape[0] > 4:
        lg[3, :, IDS.timestamp_begin + 5:IDS.timestamp_begin + 9] += 12.0
    return lg


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    assert H.MICRO.vocab == V
    e = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3))
    yield e
    e.close()


# name, what it is for
BEAM_CASES = ["batch3x5-micro",          # 3 items, prompts of 1 / 4 / 9 tokens, one ends at the second step, one runs into max_length: 15 rows, two steps per graph
              "batch5x5-micro",          # 25 rows: more than 16, one step per graph
              "beam6-gauss-micro",       # one item, six beams
              "batch3x5-length-penalty0"]


@pytest.mark.parametrize("name", BEAM_CASES)
def test_biased_beam_search_equals_the_biased_oracle(eng, name):
    c = SC.CASES[name]
    tab = table()
    lg = planted(c, c.logits())
    ref, margin, provs = oracle_answer(c, lg, tab)
    assert margin > SC.MARGIN, (name, margin)
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_bias(tab)
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(got, ref, sampling=False)
        # the bias changes the answer (this test fails without the feature), states beyond the root were walked
        assert any(r.sequences_ids != p.sequences_ids for r, p in zip(ref, plain)), name
        assert any(len(p.visited) > 2 for p in provs), [p.visited for p in provs]
        # cleared: the slot answers like one that never had a table, bit for bit
        slot.clear_bias()
        fresh = eng.create_slot(c.items, 16)
        try:
            a = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
            b = fresh.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
            assert [(x.sequences_ids, x.scores) for x in a] == [(x.sequences_ids, x.scores) for x in b]
            check(a, plain, sampling=False)
        finally:
            fresh.close()
    finally:
        slot.close()


def test_state_follows_the_beam_reordering_and_a_timestamp_resets_it(eng):
    """the oracle's trace of the first beam case shows what the case is for: a row whose parent is another row while that parent sits in a
    non-root node, and a timestamp fed behind a partial match"""
    c = SC.CASES["batch3x5-micro"]
    tab = table()

    class Spy(BiasedLogits):
        moved = 0

        def step(self, tokens, parents):
            if self.states is not None:
                Spy.moved += sum(1 for r, p in enumerate(parents) if p != r and self.states[p] != 0)
            return super().step(tokens, parents)

    lg = planted(c, c.logits())
    o = c.opts()
    resets = 0
    for b, prompt in enumerate(c.prompts):
        prov = Spy(c.item_logits(lg, b), tab)
        odec.generate(prov, prompt, o, row_base=b * c.R)
        resets += prov.ts_resets
    assert Spy.moved > 0 and resets > 0, (Spy.moved, resets)


@pytest.mark.parametrize("name", ["sample3x5-micro", "greedy4-micro"])
def test_biased_sampling_equals_the_biased_oracle(eng, name):
    """T > 0 with a seed (and the greedy rows): search_rows_kernel reads the biased row; the same call twice gives the same bits"""
    c = SC.CASES[name]
    tab = table()
    lg = planted(c, c.logits())
    ref, _, provs = oracle_answer(c, lg, tab)
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_bias(tab)
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(got, ref, sampling=True)
        again = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        assert [(g.sequences_ids, g.scores) for g in again] == [(g.sequences_ids, g.scores) for g in got]
        assert any(sorted(map(tuple, r.sequences_ids)) != sorted(map(tuple, p.sequences_ids)) for r, p in zip(ref, plain)), name
    finally:
        slot.close()


def test_a_second_table_on_the_same_slot_and_a_refused_one(eng):
    """set, clear, set another: each call answers like the oracle under ITS table; a table the library refuses leaves the installed one"""
    from whisperlive_amd import _lib
    c = SC.CASES["batch2x5-micro"]
    lg = planted(c, c.logits())
    t1 = table()
    t2 = B.compile_bias([[123, 31], [300]], 2.0, {31: -4.0}, vocab=V, eot=IDS.eot)
    slot = eng.create_slot(c.items, 5)
    try:
        for tab in (t1, t2, t1):
            ref, margin, _ = oracle_answer(c, lg, tab)
            assert margin > SC.MARGIN, margin
            slot.set_bias(tab)
            check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), ref, sampling=False)
            slot.clear_bias()
        slot.set_bias(t1)
        bad = B.compile_bias([[1, 2]], 0.5, {}, vocab=V, eot=IDS.eot)
        bad.edge_tok = bad.edge_tok.copy(); bad.edge_tok[0] = V
        with pytest.raises(_lib.WlxError) as ei:
            slot.set_bias(bad)
        assert ei.value.code == _lib.ERR_ARG and "vocabulary" in str(ei.value)
        ref, _, _ = oracle_answer(c, lg, t1)
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), ref, sampling=False)
    finally:
        slot.close()
