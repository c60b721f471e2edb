"""GPU (-m gpu): a grammar per item inside the production search launches. Injected logits through wlx_debug_search_batch with a
grammar SET on the slot (Slot.set_grammars) and a selection (Slot.select_grammars): the item under table A is bit-identical, in tokens
and scores, to the same logits decoded alone (sampling: in its own rows, see `alone`) on a slot that holds A through wlx_grammar_set;
the item without a table to a slot without a grammar. What the single-grammar decode itself answers is the subject of
tests/test_gpu_grammar_search.py, whose grammar, planted logits and seeded cases are reused. The micro vocabulary: 2310 ids, two tiles."""
import numpy as np
import pytest

from tests import helpers as H
from tests import search_cases as SC
from tests.test_gpu_grammar_search import FIRST, IDS, V, budgets, conforms, eng, grammar, planted  # noqa: F401  (eng: the module's engine fixture)
from whisperlive_amd import _lib
from whisperlive_amd import grammar as G

pytestmark = pytest.mark.gpu


def bits(results):
    return [(r.sequences_ids, [np.float32(s).tobytes() for s in r.scores]) for r in results]


def alone(eng, c, lg, b, g, sampling):
    """item b of the case on a fresh slot under `g` through wlx_grammar_set, or under none. Beam mode: the item decoded ALONE. Sampling
    mode: the sampler's random stream is keyed by the decoder row, so the reference there is the whole batch on that slot, item b of it."""
    slot = eng.create_slot(c.items if sampling else 1, 16)
    try:
        if g is not None:
            slot.set_grammar(g)
        if sampling:
            return slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)[b]
        return slot.debug_search_batch(c.item_logits(lg, b), [c.prompts[b]], H.engine_ids(c.ids), **c.gen_kw)[0]
    finally:
        slot.close()


@pytest.mark.parametrize("name,sampling", [("batch3x5-micro", False), ("sample3x5-micro", True)])
def test_a_none_b_in_one_batch(eng, name, sampling):
    c = SC.CASES[name]
    lg = planted(c, c.logits())
    ga, gb = grammar(), G.compile_grammar(None, [[a, b] for a in FIRST[4:] for b in range(400, 414)], vocab=V, eot=IDS.eot)
    run = lambda: slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
    slot = eng.create_slot(c.items, 16)
    try:
        with pytest.raises(_lib.WlxError) as ei:                 # a selection needs a set
            slot.select_grammars([0, 0, 0])
        assert ei.value.code == _lib.ERR_STATE
        slot.set_grammars(G.GrammarSet([ga, gb]))
        plain = run()                                            # a new set: every item deselected
        assert bits(plain) == bits([alone(eng, c, lg, b, None, sampling) for b in range(3)])
        for sel in ([0, -1, 1], [1, 0, -1]):                     # (the second: re-selected, nothing uploaded again)
            slot.select_grammars(sel)
            got = run()
            for b, t in enumerate(sel):
                g = (ga, gb)[t] if t >= 0 else None
                assert bits([got[b]]) == bits([alone(eng, c, lg, b, g, sampling)]), (name, sel, b)
                assert g is None or conforms(g, got[b].sequences_ids, budgets(c)[b])             # in the item's own language
            assert any(bits([got[b]]) != bits([plain[b]]) for b, t in enumerate(sel) if t >= 0)     # the tables change the answer
        slot.select_grammars([0])
        with pytest.raises(_lib.WlxError) as ei:                 # a generate wider than the selection
            run()
        assert ei.value.code == _lib.ERR_STATE
        slot.clear_grammar()                                     # wlx_grammar_clear clears this mode too
        assert bits(run()) == bits(plain)
    finally:
        slot.close()
