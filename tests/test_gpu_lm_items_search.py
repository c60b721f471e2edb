"""GPU (-m gpu): a language model per item in the search. On INJECTED logits a group of 3 items under [A, none, B] yields,
item by item, the tokens and scores (bit for bit: the same arithmetic) of that item ALONE under set_lm of its entry; then other selections
on the same slot, over the states the last left. A real decode does the same through CAPTURED step graphs, replayed under another pool."""
import struct

import pytest

from oracle import logmel as olm
from tests import helpers as H
from tests import search_cases as SC
from tests.test_gpu_lm_search import CORPUS, IDS, V, eng  # noqa: F401  (the module's engine fixture)
from whisperlive_amd import lm as L

pytestmark = pytest.mark.gpu
A = L.NgramLM.from_corpus(CORPUS, None, order=3, eot=IDS.eot, vocab=V)
B = L.NgramLM.from_corpus([c[::-1] for c in CORPUS], None, order=1, eot=IDS.eot, vocab=V)
ENTRY = {"A": (A, 1.0), "B": (B, 0.6), "A2": (A, 0.25), None: None}       # two models, one of them at two weights
SELECTIONS = (["A", None, "B"], ["B", "A2", None], ["A2", "A", "B"])      # permuted on the pool as it is, then the pool grown


def answers(results):
    return [(r.sequences_ids, struct.pack("%df" % len(r.scores), *r.scores)) for r in results]


@pytest.mark.parametrize("route", ["injected", "decode"])
def test_a_group_under_a_selection_equals_each_entry_on_its_own(eng, route):
    c = SC.CASES["batch3x5-micro"]
    ids = H.engine_ids(c.ids)
    slot = eng.create_slot(c.items, 16 if route == "injected" else 5)
    try:
        if route == "injected":                 # the reference: every item ALONE, a batch of one
            lg = c.logits()
            group = lambda: answers(slot.debug_search_batch(lg, c.prompts, ids, **c.gen_kw))
            ref = lambda: [answers(slot.debug_search_batch(c.item_logits(lg, b), [c.prompts[b]], ids, **c.gen_kw))[0] for b in range(c.items)]
        else:                                   # captured step graphs; the reference: the same batch, the same launch list on the same rows
            slot.encode(1, seek=[0], seg=[slot.logmel(olm.speech_like_pcm(4.0, seed=11)) - 1])
            kw = dict(beam_size=5, max_length=1 + 10, suppress_tokens=[ids.sot], enc_items=[0, 0, 0])
            group = ref = lambda: answers(slot.generate([[ids.sot]] * 3, ids, **kw))
        single = {}
        for name, entry in ENTRY.items():
            L.install(slot, entry)
            single[name] = ref()
        names = list(ENTRY)
        assert all(single[x] != single[y] for i, x in enumerate(names) for y in names[i + 1:])      # a wrong entry shows
        lset = L.LmSet()
        for sel in SELECTIONS:                  # every later selection finds the states another model left behind
            slot.select_lms(L.install_items(slot, [ENTRY[x] for x in sel], lset))
            assert slot._lm is lset and len(lset.models) == 2
            assert group() == [single[x][b] for b, x in enumerate(sel)], sel
        L.install(slot, None)
        assert group() == single[None]
    finally:
        slot.close()
