"""GPU (-m gpu): the grammar launch inside the production search launches, on INJECTED logits through wlx_debug_search_batch with a grammar
installed on the slot (Slot.set_grammar), against oracle.decoding.generate driven by a test-side LogitsProvider that tracks every row's DFA
state through `parents` and masks the row with tests/grammar_ref.py, step by step. Tokens exact, scores at the tolerance of
tests/test_gpu_search_batch.py (rtol = atol = 1e-3); every beam case's deciding scores are more than that apart in the oracle (asserted
here). The cases reuse the seeded logits of tests/search_cases.py: beam 5 in a batch of 3 and of 5 rows-per-graph shapes, one item of six
beams, sampling at a temperature, and greedy rows (beam 1).

The grammar is wide on purpose — every state allows at least twelve text tokens — so that a step always has 2 x beam finite candidates
and no hypothesis with a score of -inf (whose tokens only a tie-break decides) enters a beam."""
import numpy as np
import pytest

from oracle import decoding as odec
from tests import grammar_ref as GR
from tests import helpers as H
from tests import search_cases as SC
from whisperlive_amd import grammar as G

pytestmark = pytest.mark.gpu

V = SC.VOCAB["micro"]
IDS = SC.token_ids(V)
FIRST = list(range(300, 316))                   # sixteen first tokens; none is in tests/search_cases.py suppress_list, none is the blank
SECOND = list(range(400, 412))


def phrases():
    """`a b` for every first token a and twelve second tokens b (shifted per a), the first four `a` alone as well (a phrase that is a
    prefix of others: after it the next phrase may start or this one go on), and `300 400 500+k` (a third token)"""
    out = [[a, b + (a % 3)] for a in FIRST for b in SECOND]
    out += [[a] for a in FIRST[:4]]
    out += [[300, 400, 500 + k] for k in range(12)]
    return out


def grammar():
    g = G.compile_grammar(None, phrases(), vocab=V, eot=IDS.eot)
    assert min(int(g.edge_off[n + 1] - g.edge_off[n]) for n in range(g.n_states)) >= 12
    return g


class MaskedLogits(odec.InjectedLogits):
    """injected logits under the grammar: each row's state follows `parents`, the row is masked with grammar_ref.mask_row"""

    def __init__(self, logits, g, plen):
        super().__init__(logits)
        self.g, self.plen, self.states, self.pos = g, plen, None, plen - 1
        self.visited, self.moved, self.kept_over_ts = set(), 0, 0

    def step(self, tokens, parents):
        if self.states is None:
            self.states = [0] * len(tokens)
        else:
            self.pos += 1
            self.moved += sum(1 for r, p in enumerate(parents) if p != r and self.states[p] != 0)
            self.kept_over_ts += sum(1 for p, t in zip(parents, tokens) if self.states[p] != 0 and t >= IDS.timestamp_begin)
            self.states = [GR.next_state(self.g, self.states[p], int(t), self.pos, self.plen) for p, t in zip(parents, tokens)]
        self.visited.update(self.states)
        out = np.array(super().step(tokens, parents), dtype=np.float32, copy=True)
        for r, s in enumerate(self.states):
            GR.mask_row(self.g, out[r], s)
        return out


def oracle_answer(c, lg, g):
    res, margin, provs = [], float("inf"), []
    o = c.opts()
    beam_mode = not (o.sampling_temperature > 0 or o.beam_size <= 1)
    for b, prompt in enumerate(c.prompts):
        w = SC._Watch(c.R, max(1, o.num_hypotheses), c.ids.eot) if beam_mode else None
        prov = MaskedLogits(c.item_logits(lg, b), g, len(prompt))
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


# the top of the ramp over the first tokens per case: where the first value (3.0) left two deciding scores of the masked oracle closer than
# SC.MARGIN another one was taken (scanned in steps of 0.5 on the oracle alone)
LIFT = {"batch3x5-micro": 3.5, "batch5x5-micro": 3.5, "beam6-gauss-micro": 4.0}


def planted(c, lg):
    """the case's logits with the grammar's tokens lifted a little, unevenly, so that the beams spread over several first tokens, some walk
    `300 400` into its third token, and one step favours a timestamp behind a first token (a timestamp in the middle of a phrase)"""
    lg = lg.copy()
    lg[:, :, FIRST] += np.linspace(1.0, LIFT.get(c.name, 3.0), len(FIRST), dtype=np.float32)
    lg[1:, :, 400:416] += 2.0
    lg[2:, :, 500:512] += 2.5
    if lg.shape[0] > 4:
        lg[3, :, IDS.timestamp_begin + 5:IDS.timestamp_begin + 9] += 12.0
    return lg


def conforms(g, seqs, budget=None):
    """every hypothesis is a string of the language — or, where it ran into the step budget (no end-of-text was reached), the beginning of one"""
    for s in seqs:
        text = [t for t in s if t < IDS.eot]
        if G.accepts(g, text):
            continue
        state = 0
        for t in text:
            state = g.step(state, t)
            if state < 0:
                return False
        if budget is None or len(s) < budget:
            return False
    return True


def budgets(c):
    return [c.kw["max_length"] - len(p) for p in c.prompts]


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    assert H.MICRO.vocab == V
    e = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3))
    yield e
    e.close()


BEAM_CASES = ["batch3x5-micro",          # 3 items, prompts of 1 / 4 / 9 tokens: 15 rows, two steps per graph
              "batch5x5-micro",          # 25 rows: more than 16, one step per graph
              "beam6-gauss-micro"]       # one item, six beams


@pytest.mark.parametrize("name", BEAM_CASES)
def test_beam_search_under_a_grammar_equals_the_masked_oracle(eng, name):
    c = SC.CASES[name]
    g = grammar()
    lg = planted(c, c.logits())
    ref, margin, provs = oracle_answer(c, lg, g)
    assert margin > SC.MARGIN, (name, margin)
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
    # what the case is for: the oracle's answer is in the language and the unconstrained one is not; states beyond the start state were
    # walked; a row's parent was ANOTHER row while that parent sat inside a phrase (the beam re-ordered), a timestamp kept a state
    assert all(conforms(g, r.sequences_ids, n) for r, n in zip(ref, budgets(c))) and not all(conforms(g, p.sequences_ids, n) for p, n in zip(plain, budgets(c)))
    assert any(len(p.visited) > 2 for p in provs) and sum(p.moved for p in provs) > 0
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_grammar(g)
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(got, ref, sampling=False)
        assert all(conforms(g, x.sequences_ids, n) for x, n in zip(got, budgets(c)))
        # cleared: the slot answers like one that never had a grammar, bit for bit
        slot.clear_grammar()
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


def test_a_timestamp_in_the_middle_of_a_phrase_keeps_the_state():
    """(CPU side of the first beam case: the oracle's trace shows a timestamp fed behind a partial match, and the phrase goes on after it)"""
    c = SC.CASES["batch3x5-micro"]
    _ref, _margin, provs = oracle_answer(c, planted(c, c.logits()), grammar())
    assert sum(p.kept_over_ts for p in provs) > 0


@pytest.mark.parametrize("name", ["sample3x5-micro", "greedy4-micro"])
def test_sampling_under_a_grammar_equals_the_masked_oracle(eng, name):
    """T > 0 with a seed, and the greedy rows (beam 1): search_rows_kernel reads the masked row; the same call twice gives the same bits"""
    c = SC.CASES[name]
    g = grammar()
    lg = planted(c, c.logits())
    ref, _, _provs = oracle_answer(c, lg, g)
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
    assert all(conforms(g, r.sequences_ids, n) for r, n in zip(ref, budgets(c))) and not all(conforms(g, p.sequences_ids, n) for p, n in zip(plain, budgets(c)))
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_grammar(g)
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(got, ref, sampling=True)
        assert all(conforms(g, x.sequences_ids, n) for x, n in zip(got, budgets(c)))
        again = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        assert [(x.sequences_ids, x.scores) for x in again] == [(x.sequences_ids, x.scores) for x in got]
    finally:
        slot.close()


def test_a_second_grammar_a_keyword_table_and_a_refused_grammar_on_one_slot(eng):
    """set, set another, a keyword table in between (one mode at a time: the last set call decides), a refused table: each call answers
    like the oracle under what is installed"""
    from whisperlive_amd import _lib
    from whisperlive_amd import biasing as B
    c = SC.CASES["batch2x5-micro"]
    lg = planted(c, c.logits())
    g1 = grammar()
    g2 = G.compile_grammar(None, [[a, b] for a in FIRST[4:] for b in range(400, 414)], vocab=V, eot=IDS.eot)
    slot = eng.create_slot(c.items, 5)
    try:
        for g in (g1, g2, g1):
            ref, margin, _ = oracle_answer(c, lg, g)
            assert margin > SC.MARGIN, margin
            slot.set_grammar(g)
            check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), ref, sampling=False)
        ref1, _, _ = oracle_answer(c, lg, g1)
        # a keyword table takes the slot out of grammar mode; an empty one adds nothing: the unconstrained answer
        plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
        slot.set_bias(B.compile_bias([[5, 6]], 0.0, {}, vocab=V, eot=IDS.eot))
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), plain, sampling=False)
        slot.clear_grammar()                                            # (not in grammar mode: the table stays)
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), plain, sampling=False)
        slot.set_grammar(g1)
        bad = G.compile_grammar(None, [[1, 2]], vocab=V, eot=IDS.eot)
        bad.edge_tok = bad.edge_tok.copy(); bad.edge_tok[0] = IDS.eot
        with pytest.raises(_lib.WlxError) as ei:
            slot.set_grammar(bad)
        assert ei.value.code == _lib.ERR_ARG and "text token" in str(ei.value)
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), ref1, sampling=False)
        # a call whose end-of-text is not the grammar's is refused
        other = H.engine_ids(c.ids)
        other.eot = c.ids.eot - 1
        with pytest.raises(_lib.WlxError) as ei:
            slot.debug_search_batch(lg, c.prompts, other, **c.gen_kw)
        assert ei.value.code == _lib.ERR_ARG and "end-of-text" in str(ei.value)
    finally:
        slot.close()
