"""The injected-logits cases of tests/search_cases.py, on the oracle alone (no GPU): every case has the property it was built for, and
its deciding scores are more than 1e-3 apart, so tests/test_gpu_search_batch.py can ask for exact tokens."""
import numpy as np
import pytest

from oracle import decoding as odec
from tests import helpers as H
from tests import search_cases as SC


def test_ids_and_suppress_list_are_the_helpers():
    for v in SC.VOCAB.values():
        assert SC.token_ids(v) == H.token_ids_for(v)
        assert SC.suppress_list(SC.token_ids(v)) == H.default_suppress(H.token_ids_for(v))


def test_case_sizes_stay_inside_the_budget():
    """at most 16 steps x 48 rows at the full vocabulary, 32 steps at the micro one"""
    for c in SC.CASES.values():
        assert c.items * c.R <= 48 and c.steps <= (16 if c.vocab == "full" else 32), c.name
        assert all(1 <= n < c.kw["max_length"] for n in c.plens), c.name


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_deciding_scores_are_separated(name):
    """Beam cases: wherever the order of two scores from different beam rows decides the result — the last merged candidate kept against the
    first dropped, the last candidate that may finish against the next, the beams that go on (their order is their row) and the first one
    left out, the finished hypotheses returned and the first one left out — the two differ by more than 1e-3."""
    a = SC.answer(name)
    c = SC.CASES[name]
    if c.kw.get("sampling_temperature", 0.0) > 0 or c.kw["beam_size"] <= 1:
        assert a.margin == float("inf")                   # rows on their own: nothing is ranked across rows
    else:
        assert a.margin > SC.MARGIN, (name, a.margin, a.where)
    assert all(r.sequences_ids for r in a.results), name


def test_observer_changes_no_result():
    c = SC.CASES["batch3x8-micro"]
    lg = c.logits()
    seen = []
    for b, p in enumerate(c.prompts):
        plain = odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R)
        watched = odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, c.opts(), row_base=b * c.R, observer=seen.append)
        assert plain == watched == SC.answer(c.name).results[b]
    assert seen and "hyps" in seen[-1] and len(seen[0]["cands"]) == c.R * 2 * c.R


@pytest.mark.parametrize("name", sorted(n for n in SC.CASES if n.startswith(("batch", "greedy4"))))
def test_items_of_a_batch_end_at_different_steps(name):
    a = SC.answer(name)
    c = SC.CASES[name]
    steps = [r.steps for r in a.results]
    assert len(set(steps)) >= min(len(steps), 3), steps
    assert min(steps) in (1, 2), steps                                    # the first item to end: at the first or second step
    by_budget = [b for b, r in enumerate(a.results) if r.steps == a.max_new[b]]
    assert by_budget and max(steps) in [steps[b] for b in by_budget], steps   # the item that ends last runs into max_length
    assert len(set(c.plens)) >= min(c.items, 3) and set(c.plens) <= {1, 2, 4, 9}, c.plens
    b = by_budget[0]                                                      # ended by max_length, not by end-of-text: its best has every token
    assert len(a.results[b].sequences_ids[0]) == a.max_new[b]


@pytest.mark.parametrize("vocab", ["micro", "full"])
def test_first_step_offers_fewer_ids_than_candidates(vocab):
    name = f"beam12-initial-ts5-{vocab}"
    assert SC.first_step_allowed(name) == 6 < 2 * SC.CASES[name].R


@pytest.mark.parametrize("vocab", ["micro", "full"])
def test_patience_two_fills_the_hypothesis_store(vocab):
    a = SC.answer(f"beam16-patience2-{vocab}")
    assert a.n_hyps[0] >= 32 and len(a.results[0].sequences_ids) == 16
    assert a.results[0].steps < a.max_new[0]                                                    # ended by the count, not by the step budget


def test_patience_two_and_a_half_asks_for_more_than_the_store():
    a = SC.answer("beam16-patience2.5-micro")
    assert a.n_hyps[0] >= 40 and a.results[0].steps < a.max_new[0]


@pytest.mark.parametrize("vocab", ["micro", "full"])
def test_sampling_draws_differ_between_items_with_equal_logits(vocab):
    c = SC.CASES[f"sample3x5-{vocab}"]
    lg = c.logits()
    assert np.array_equal(c.item_logits(lg, 0), c.item_logits(lg, 1)) and c.prompts[0] == c.prompts[1]
    a = SC.answer(c.name)
    assert sorted(map(tuple, a.results[0].sequences_ids)) != sorted(map(tuple, a.results[1].sequences_ids))
    # ... only through the row key of the draw: with item 0's row_base the second item repeats the first
    again = odec.generate(odec.InjectedLogits(c.item_logits(lg, 1)), c.prompts[1], c.opts(), row_base=0)
    assert again == a.results[0]
    assert len({tuple(s) for s in a.results[0].sequences_ids}) > 1                              # rows of one item differ too


def test_penalty_cases_act_on_repetitions():
    """the repetition penalty / the n-gram ban change the result of their case (the history is read, not just carried)"""
    for name, off in (("batch3x5-repetition-penalty", dict(repetition_penalty=1.0)), ("batch3x5-no-repeat-ngram", dict(no_repeat_ngram_size=0))):
        c = SC.CASES[name]
        lg = c.logits()
        o = odec.GenOptions(ids=c.ids, **dict(c.gen_kw, **off))
        plain = odec.generate(odec.InjectedLogits(c.item_logits(lg, 0)), c.prompts[0], o)
        assert plain.sequences_ids != SC.answer(name).results[0].sequences_ids, name             # item 0: the one that runs its whole budget
