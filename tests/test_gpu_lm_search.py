"""GPU (-m gpu): n-gram language-model fusion inside the production search launches, on INJECTED logits through wlx_debug_search_batch with
a model set on the slot (Slot.set_lm), against oracle.decoding.generate driven by a test-side LogitsProvider that tracks every row's
context state through `parents` and applies lm.NgramLM.fuse_row (float64). Tokens exact, scores at the tolerance of
tests/test_gpu_search_batch.py (rtol = atol = 1e-3); every beam case's deciding scores are more than that apart in the oracle (asserted
here). The cases reuse the seeded logits of tests/search_cases.py."""
import numpy as np
import pytest

from oracle import decoding as odec
from tests import helpers as H
from tests import search_cases as SC
from tests.test_gpu_bias_search import check
from whisperlive_amd import lm as L

pytestmark = pytest.mark.gpu

V = SC.VOCAB["micro"]
IDS = SC.token_ids(V)
WEIGHT = 1.0                 # against logits of sigma 4: a token the model knows gains several units on one it does not
CORPUS = [[31, 57, 123], [31, 57, 123, 640], [57, 300], [57, 300, 31], [31, 57], [411], [411, 31, 57, 300], [640, 640, 31]]


def model():
    return L.NgramLM.from_corpus(CORPUS, None, order=3, eot=IDS.eot, vocab=V)


class FusedLogits(odec.InjectedLogits):
    """injected logits fused with the model in each row's context: the context follows `parents`"""

    def __init__(self, logits, lm):
        super().__init__(logits)
        self.lm, self.states, self.visited, self.moved = lm, None, set(), 0

    def step(self, tokens, parents):
        if self.states is None:
            self.states = [self.lm.start_state] * len(tokens)
        else:
            self.moved += sum(1 for r, p in enumerate(parents) if p != r and self.states[p] != self.states[r])
            self.states = [self.lm.next_state(self.states[p], t) for p, t in zip(parents, tokens)]
        self.visited.update(self.states)
        raw = np.asarray(super().step(tokens, parents), dtype=np.float32)
        return np.stack([self.lm.fuse_row(raw[r], s, WEIGHT) for r, s in enumerate(self.states)]).astype(np.float32)


def oracle_answer(c, lg, lm):
    res, margin, provs = [], float("inf"), []
    o = c.opts()
    beam_mode = not (o.sampling_temperature > 0 or o.beam_size <= 1)
    for b, prompt in enumerate(c.prompts):
        w = SC._Watch(c.R, max(1, o.num_hypotheses), c.ids.eot) if beam_mode else None
        prov = FusedLogits(c.item_logits(lg, b), lm)
        res.append(odec.generate(prov, prompt, o, row_base=b * c.R, observer=w))
        provs.append(prov)
        if w is not None:
            margin = min(margin, w.margin)
    return res, margin, provs


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    assert H.MICRO.vocab == V
    e = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3))
    yield e
    e.close()


@pytest.mark.parametrize("name", ["batch3x5-micro", "sample3x5-micro"])
def test_fused_search_equals_the_fused_oracle(eng, name):
    c = SC.CASES[name]
    lm, lg = model(), c.logits()
    sampling = name.startswith("sample")
    ref, margin, provs = oracle_answer(c, lg, lm)
    if not sampling:
        assert margin > SC.MARGIN, (name, margin)
        assert any(p.moved > 0 for p in provs)                  # a row took its context from ANOTHER row: the state follows the re-ordering
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R) for b, p in enumerate(c.prompts)]
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_lm(lm, WEIGHT)
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(got, ref, sampling=sampling)
        # the fusion changes the answer (this test fails without the feature), contexts beyond the start were walked
        key = (lambda r: sorted(map(tuple, r.sequences_ids))) if sampling else (lambda r: r.sequences_ids)
        assert any(key(r) != key(p) for r, p in zip(ref, plain)), name
        assert any(len(p.visited) > 2 for p in provs), [p.visited for p in provs]
        # cleared: the slot answers like one that never had a model, bit for bit; the engine then lets the model go
        slot.clear_lm()
        a = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        check(a, plain, sampling=sampling)
        eng.destroy_lm(lm)
    finally:
        slot.close()
