"""GPU (-m gpu): per-item keyword boosting inside the production search launches. Injected logits through wlx_debug_search_batch with a
table SET installed on the slot (Slot.set_bias_items) and a selection (Slot.select_bias): the item under table A is bit-identical, in
tokens and scores, to the same logits decoded alone (sampling: in its own rows, see `alone`) on a slot that holds A's CLOSED form through wlx_bias_set; the item without a table to
an unbiased slot; all of them equal oracle.decoding.generate behind the states-tracking provider of tests/test_gpu_bias_search.py. The
injected-logits loop launches eagerly; the captured step graphs (two steps per graph for <= 16 rows on a lone slot, one step above) are
covered by the real decodes at the end, on a random-weights engine. The cases reuse the seeded logits of tests/search_cases.py."""
import numpy as np
import pytest

from oracle import decoding as odec
from tests import helpers as H
from tests import search_cases as SC
from tests.test_gpu_bias_search import BOOST, LOGIT_BIAS, PHRASES, BiasedLogits, check, planted
from whisperlive_amd import _lib
from whisperlive_amd import biasing as B

pytestmark = pytest.mark.gpu

V = SC.VOCAB["micro"]
IDS = SC.token_ids(V)
SPEC_A = (PHRASES, BOOST, LOGIT_BIAS)
SPEC_B = ([[123, 31], [300], [31, 640]], 12.0, {31: -1.0, 57: 2.0})


def forms(spec):
    return B.compile_compact(*spec, vocab=V, eot=IDS.eot), B.compile_bias(*spec, vocab=V, eot=IDS.eot)


def bits(results):
    return [(r.sequences_ids, [np.float32(s).tobytes() for s in r.scores]) for r in results]


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    assert H.MICRO.vocab == V
    e = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3))
    yield e
    e.close()


def alone(eng, c, lg, b, closed, sampling=False):
    """item b of the case on a fresh slot under `closed` through wlx_bias_set, or unbiased. Beam mode: the item decoded ALONE. Sampling
    mode: the sampler's random stream is keyed by the decoder row (the oracle's `row_base`), so an item decoded alone in rows 0 .. R - 1
    draws other numbers than in its rows of the batch: the reference there is the whole batch on the single-table slot, item b of it."""
    slot = eng.create_slot(c.items if sampling else 1, 16)
    try:
        if closed is not None:
            slot.set_bias(closed)
        if sampling:
            return slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)[b]
        return slot.debug_search_batch(c.item_logits(lg, b), [c.prompts[b]], H.engine_ids(c.ids), **c.gen_kw)[0]
    finally:
        slot.close()


def oracle_item(c, lg, b, closed):
    prov = BiasedLogits(c.item_logits(lg, b), closed) if closed is not None else odec.InjectedLogits(c.item_logits(lg, b))
    o = c.opts()
    beam_mode = not (o.sampling_temperature > 0 or o.beam_size <= 1)
    w = SC._Watch(c.R, max(1, o.num_hypotheses), c.ids.eot) if beam_mode else None
    res = odec.generate(prov, c.prompts[b], o, row_base=b * c.R, observer=w)
    assert w is None or w.margin > SC.MARGIN, (c.name, b, w.margin)       # the deciding scores are further apart than the tolerance
    return res


@pytest.mark.parametrize("name,sampling", [("batch3x5-micro", False), ("sample3x5-micro", True)])
def test_a_none_b_in_one_batch(eng, name, sampling):
    c = SC.CASES[name]
    lg = planted(c, c.logits())
    (ca, xa), (cb, xb) = forms(SPEC_A), forms(SPEC_B)
    bset = B.BiasSet([ca, cb])
    slot = eng.create_slot(c.items, 16)
    try:
        slot.set_bias_items(bset)
        slot.select_bias([0, -1, 1])
        got = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        closed = [xa, None, xb]
        for b in range(3):
            assert bits([got[b]]) == bits([alone(eng, c, lg, b, closed[b], sampling)]), (name, b)
        check(got, [oracle_item(c, lg, b, closed[b]) for b in range(3)], sampling=sampling)
        plain = [oracle_item(c, lg, b, None) for b in range(3)]
        key = (lambda r: sorted(map(tuple, r.sequences_ids))) if sampling else (lambda r: r.sequences_ids)
        assert key(got[0]) != key(plain[0]) or key(got[2]) != key(plain[2])        # the tables change the answer
        # ---- re-select on the same slot, nothing uploaded again: (B, A, none)
        slot.select_bias([1, 0, -1])
        again = slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        closed = [xb, xa, None]
        for b in range(3):
            assert bits([again[b]]) == bits([alone(eng, c, lg, b, closed[b], sampling)]), (name, b)
    finally:
        slot.close()


def test_set_items_then_single_table_then_clear_equal_fresh_slots(eng):
    c = SC.CASES["batch2x5-micro"]
    lg = planted(c, c.logits())
    (ca, xa), (cb, xb) = forms(SPEC_A), forms(SPEC_B)
    run = lambda s: bits(s.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw))

    def fresh(prepare):
        s = eng.create_slot(c.items, 5)
        try:
            prepare(s)
            return run(s)
        finally:
            s.close()

    slot = eng.create_slot(c.items, 5)
    try:
        slot.set_bias_items(B.BiasSet([ca, cb]))
        slot.select_bias([1, 0])
        per_item = run(slot)
        assert per_item == [fresh(lambda s: s.set_bias(xb))[0], fresh(lambda s: s.set_bias(xa))[1]]
        slot.set_bias(xb)                                        # back to single-table mode: every item under B
        assert run(slot) == fresh(lambda s: s.set_bias(xb))
        with pytest.raises(_lib.WlxError) as ei:                 # a selection needs a set
            slot.select_bias([0, 0])
        assert ei.value.code == _lib.ERR_STATE
        slot.clear_bias()
        assert run(slot) == fresh(lambda s: None)
        slot.set_bias_items(B.BiasSet([ca]))                     # a new set starts with every item deselected
        assert run(slot) == fresh(lambda s: None)
        slot.clear_bias()
        assert run(slot) == fresh(lambda s: None)
    finally:
        slot.close()


def test_refusals(eng):
    c = SC.CASES["batch2x5-micro"]
    lg = c.logits()
    ca, _ = forms(SPEC_A)
    slot = eng.create_slot(c.items, 5)
    try:
        with pytest.raises(_lib.WlxError) as ei:
            slot.select_bias([0])
        assert ei.value.code == _lib.ERR_STATE
        slot.set_bias_items(B.BiasSet([ca]))
        slot.select_bias([0])
        with pytest.raises(_lib.WlxError) as ei:                 # a generate wider than the selection
            slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
        assert ei.value.code == _lib.ERR_STATE and "selection" in str(ei.value)
        for bad in ([1, 0], [-2, 0], [0, 0, 0]):
            with pytest.raises(_lib.WlxError) as ei:
                slot.select_bias(bad)
            assert ei.value.code == _lib.ERR_ARG
        # a refused set leaves the installed one whole
        broken = B.compile_compact(*SPEC_A, vocab=V, eot=IDS.eot)
        broken.edge_tok = broken.edge_tok.copy(); broken.edge_tok[0] = V
        with pytest.raises(_lib.WlxError) as ei:
            slot.set_bias_items(B.BiasSet([broken]))
        assert ei.value.code == _lib.ERR_ARG and "vocabulary" in str(ei.value)
        slot.select_bias([0, -1])
        slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw)
    finally:
        slot.close()


@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("items", [3, 5])
def test_real_decodes_through_the_step_graphs(gpu, items, sampling):
    """a random-weights engine with ONE live slot: 15 rows decode with two steps per captured graph, 25 rows with one; beam search and
    sampling (T = 0.6, seeded, five hypotheses per item). A two-table set with one table selected for every item equals wlx_bias_set of
    that table's closed form bit for bit; (A, none, B, A, none) equals, item by item, the all-A, the cleared and the all-B decode of the
    same batch; graphs captured in one mode are not replayed in another (the modes alternate on one slot)."""
    from oracle import logmel as olm
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    ids = H.token_ids_for(V)
    text = [t for t in range(20, 400)]
    spec_a = ([[t] for t in text[::8]] + [[text[1], text[2]]], 6.0, {text[4]: 3.0})       # 48 first tokens: about 2500 edges closed
    spec_b = ([[t, t + 1] for t in text[3::11]] + [[text[5]]], 4.0, {text[9]: -2.0})
    (ca, xa), (cb, xb) = ((B.compile_compact(*sp, vocab=V, eot=ids.eot), B.compile_bias(*sp, vocab=V, eot=ids.eot)) for sp in (spec_a, spec_b))
    kw = dict(max_length=1 + 8, suppress_tokens=H.default_suppress(ids))
    kw.update(dict(beam_size=1, num_hypotheses=5, sampling_temperature=0.6, sampling_topk=0, seed=1234) if sampling else dict(beam_size=5))
    e = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=5))
    try:
        slot = e.create_slot(items, 5)
        Ts = [slot.logmel(olm.speech_like_pcm(2.0 + 0.5 * i, seed=40 + i), item=i) for i in range(items)]
        slot.encode(items, seek=[0] * items, seg=[t - 1 for t in Ts])
        run = lambda: bits(slot.generate([[ids.sot]] * items, H.engine_ids(ids), **kw))
        plain = run()
        slot.set_bias(xa)
        single_a = run()
        slot.set_bias(xb)
        single_b = run()
        assert single_a != plain and single_b != plain and single_a != single_b
        slot.set_bias_items(B.BiasSet([ca, cb]))
        slot.select_bias([0] * items)
        assert run() == single_a
        slot.select_bias([1] * items)
        assert run() == single_b
        sel = [(0, -1, 1, 0, -1)[i] for i in range(items)]
        slot.select_bias(sel)
        mixed = run()
        assert mixed == [{0: single_a, 1: single_b, -1: plain}[sel[i]][i] for i in range(items)]
        slot.clear_bias()
        assert run() == plain
        slot.close()
    finally:
        e.close()
