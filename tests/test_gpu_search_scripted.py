"""GPU (-m gpu): the production search launches (search.hip: search_scan3_kernel + search_merge_update3_kernel in beam mode,
search_rows_kernel + search_update_kernel for greedy / sampling rows) on the SCRIPTED logits of tests/search_scripts.py, through
wlx_debug_search / wlx_debug_search_batch. Every case steers the search into one corner of one token rule; what comes back is held to three
things that do not depend on each other:

* the oracle (oracle/decoding.py): every returned hypothesis, token for token and in order;
* the case itself: a legal script comes back verbatim, an illegal one does not, and the positions / counts / orders the case names hold;
* `violations`: no returned sequence breaks a rule (a predicate on the sequence alone), and the scores equal `score_f64`, the float64 sum of
  log-probabilities under the float64 restatement of the rules.

Score tolerance: the oracle's own float32 scores differ from `score_f64` by at most 1.58e-6 over all cases and returned hypotheses
(ORACLE_SCORE_ERR = 1.6e-6, held by tests/test_search_scripts_host.py); the device sums in another order and uses __expf / __logf and is
allowed 8 x that, 1.28e-5 absolute (measured on MI355X: 1.58e-6 over 116 scores) — 78 x tighter than the 1e-3 * max(1, |score|) of the random-logits tests, which caps it for large scores.
tests/test_search_scripts_host.py shows that every deciding pair of scores in every case is more than 1e-3 apart, so no mismatch here is a
near-tie.

One engine and one slot per vocabulary: the micro model (2310 ids: one text and one timestamp scan chunk) and a two-layer model with the
multilingual vocabulary (51865: 25 text chunks, the last one ragged, and one timestamp chunk). No encode: the search never touches the
network."""
import numpy as np
import pytest

from tests import helpers as H
from tests import search_cases as SC
from tests import search_scripts as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slots(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import WhisperSpec
    from whisperlive_amd.weights import random_weights
    full = WhisperSpec(n_mels=80, d_model=768, n_heads=12, enc_layers=1, dec_layers=2, ffn=3072, vocab=SC.VOCAB["full"])
    assert H.MICRO.vocab == SC.VOCAB["micro"]
    engs = {"micro": HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3)), "full": HipWhisperEngine(full, random_weights(full, seed=11))}
    out = {"micro": engs["micro"].create_slot(3, 5), "full": engs["full"].create_slot(1, 5)}
    yield out
    for s in out.values():
        s.close()
    for e in engs.values():
        e.close()


def _solo(slot, s, lg=None):
    return slot.debug_search(s.logits() if lg is None else lg, s.prompt, H.engine_ids(s.ids), **s.gen_kw)


def _check(s, got):
    ref = SS.answer(s.name).result
    o, lg = s.opts(), s.logits()
    print(s.name, "gpu", got.sequences_ids[0], got.scores[:3], "oracle", ref.scores[:3])
    assert got.sequences_ids == ref.sequences_ids, (s.name, got.sequences_ids, ref.sequences_ids)
    assert SS.expectation_failures(s, got.sequences_ids) == []
    worst = 0.0
    for seq, sc in zip(got.sequences_ids, got.scores):
        assert SS.violations(seq, s.ids, o, s.apply_ts) == [], (s.name, seq)
        want = SS.score_f64(seq, SS.ended_on_eot(s, seq), lg[:, 0], o, s.apply_ts)
        worst = max(worst, abs(sc - want))
        print("   score", sc, "float64", want, "diff", abs(sc - want), "allowed", SS.device_tol(want))
        assert abs(sc - want) <= SS.device_tol(want), (s.name, seq, sc, want)
    return worst


@pytest.mark.parametrize("name", sorted(SS.SCRIPTS))
def test_scripted_search(slots, name):
    s = SS.SCRIPTS[name]
    _check(s, _solo(slots[s.vocab], s))


def test_patience_halves_round_up_on_the_device(slots):
    """beam * patience = 4.5, 2.5, 12.5 stop after 5, 3, 13 finished hypotheses (one finishes per step): the longest returned hypothesis has that
    many tokens, and with five asked for beam 5 / patience 0.5 returns three"""
    for name, stop in (("finish-beam3-patience1.5", 5), ("finish-beam5-patience0.5", 3), ("finish-beam5-patience2.5", 13)):
        s = SS.SCRIPTS[name]
        got = _solo(slots["micro"], s)
        assert max(len(q) for q in got.sequences_ids) == stop == SS.answer(name).n_hyps, (name, got.sequences_ids)
        assert len(got.sequences_ids) == min(stop, s.gen_kw["num_hypotheses"])


@pytest.mark.parametrize("name", sorted(SS.BATCHES))
def test_batched_items_equal_their_solo_runs(slots, name):
    """three items with different scripts and prompts of 1 / 4 / 9 tokens in one call, one of which ends many steps before the others: every
    item is the oracle's answer and its own solo run, scores bit for bit"""
    items = [SS.SCRIPTS[n] for n in SS.BATCHES[name]]
    slot = slots["micro"]
    R, V = items[0].R, items[0].V
    kw = items[0].gen_kw
    assert all(s.gen_kw == kw and s.R == R for s in items)
    steps = max(s.max_new for s in items)
    lg = np.zeros((steps, len(items) * R, V), dtype=np.float32)
    for b, s in enumerate(items):
        lg[:s.max_new, b * R:(b + 1) * R] = s.logits()
    got = slot.debug_search_batch(lg, [s.prompt for s in items], H.engine_ids(items[0].ids), **kw)
    assert len(got) == len(items)
    for s, g in zip(items, got):
        _check(s, g)
        alone = _solo(slot, s)
        assert alone.sequences_ids == g.sequences_ids, s.name
        assert alone.scores == g.scores, (s.name, alone.scores, g.scores)
