"""The scripted searches of tests/search_scripts.py on the CPU (no GPU): the oracle walks every script where the case says it must, the
float64 restatement of the rules (`rules_f64`, `score_f64`) and the predicate on output sequences (`violations`) agree with
oracle/decoding.py at every row the oracle processed, and every decision of every case is more than 1e-3 apart, so
tests/test_gpu_search_scripted.py can ask the device for exact tokens."""
import types

import numpy as np
import pytest

from oracle import decoding as odec
from tests import search_cases as SC
from tests import search_scripts as SS

ALL = sorted(SS.SCRIPTS)


def test_the_table_has_every_family():
    fam = lambda p: [n for n in ALL if n.startswith(p)]
    assert len(fam("legal-")) >= 7 and len(fam("illegal-")) >= 12 and len(fam("norules-")) >= 6 and len(fam("ngram")) >= 9 and len(fam("penalty")) >= 6
    assert len(fam("finish-")) >= 7 and len(fam("full-")) >= 8 and len(fam("mass-")) >= 2
    assert len([n for n in ALL if n.endswith("-greedy")]) >= 6 and len([n for n in ALL if n.endswith("-topk1")]) >= 6
    for s in SS.SCRIPTS.values():
        assert s.max_new <= (12 if s.vocab == "full" else 20), s.name
        assert s.expect in ("verbatim", None) and s.R <= 5
    assert SS.MARGIN == SC.MARGIN == 1e-3
    for items in SS.BATCHES.values():
        ss = [SS.SCRIPTS[n] for n in items]
        assert [s.plen for s in ss] == [1, 4, 9] and len({s.gen_kw["max_length"] for s in ss}) == 1 and len({tuple(s.script) for s in ss}) == 3
        steps = [SS.answer(s.name).result.steps for s in ss]
        assert min(steps) <= 4 and max(steps) - min(steps) >= 6, steps            # one item ends many steps ahead of the others


def test_scripted_logits_shape_and_boosts():
    ids = SC.token_ids(2310)
    lg = SS.scripted_logits([900, 100], 5, 2310, ids, 8.0, seed=1)
    plain = np.random.default_rng(1).standard_normal((3, 1, 2310), dtype=np.float32)
    assert lg.shape == (3, 5, 2310) and lg.dtype == np.float32
    d = lg - plain
    assert (d[0, :, 900] == np.float32(plain[0, 0, 900] + np.float32(8.0)) - plain[0, 0, 900]).all() and d[1, 0, 100] > 7.9 and d[2, 0, ids.eot] > 7.9
    d[0, :, 900] = d[1, :, 100] = d[2, :, ids.eot] = 0
    assert not d.any()                                                            # every row is the same noise, nothing else is touched
    other = SS.scripted_logits([900, 100], 5, 2310, ids, 8.0, seed=1, identical_rows=False)
    assert not np.array_equal(other[0, 0], other[0, 1])


@pytest.mark.parametrize("name", ALL)
def test_oracle_walks_the_script(name):
    """"verbatim" cases come back as scripted, the others do not; the position-wise expectations, the number of hypotheses returned and finished
    and the order the case was built for hold; no returned hypothesis breaks a rule (`violations` sees the sequence alone)."""
    s, a = SS.SCRIPTS[name], SS.answer(name)
    assert SS.expectation_failures(s, a.result.sequences_ids) == []
    if s.n_finished is not None:
        assert a.n_hyps == s.n_finished, (name, a.n_hyps)
    o = s.opts()
    for seq in a.result.sequences_ids:
        assert SS.violations(seq, s.ids, o, s.apply_ts) == [], (name, seq)


@pytest.mark.parametrize("name", ALL)
def test_rules_f64_masks_what_the_oracle_masks(name):
    """at every (step, row) the oracle processed, with that row's history: the same ids are masked, the log-sum-exp agrees to float32 rounding
    (a few ulp of a value below 32: 1e-5), and the timestamp-mass rule is never within 1e-3 of its threshold (the side is not in doubt)"""
    s, a = SS.SCRIPTS[name], SS.answer(name)
    o, lg = s.opts(), s.logits()
    assert a.seen
    for t, r, h in a.seen:
        v64, lse64, gap = SS._rules(lg[t, r], h, o, s.apply_ts)
        v32, lse32, _ = odec.process_logits(lg[t, r], h, o, s.apply_ts)
        assert np.array_equal(np.isfinite(v64), np.isfinite(v32)), (name, t, r, h, np.flatnonzero(np.isfinite(v64) != np.isfinite(v32))[:10])
        assert abs(lse64 - float(lse32)) <= 1e-5, (name, t, r, lse64, lse32)
        assert gap is None or abs(gap) > SS.MARGIN, (name, t, r, gap)
        again, lse_again = SS.rules_f64(lg[t, r], h, o, s.apply_ts)
        assert lse_again == lse64 and np.array_equal(again, v64)


def test_oracle_scores_equal_score_f64():
    """every returned hypothesis of every case: the oracle's float32 score against the float64 sum, within ORACLE_SCORE_ERR (the measured
    largest difference, 1.58e-6: what the device's allowance of 8 x is taken from)"""
    worst, where = 0.0, ""
    for name in ALL:
        s, a = SS.SCRIPTS[name], SS.answer(name)
        o, lg = s.opts(), s.logits()
        assert np.array_equal(lg[:, 0], lg[:, -1])                                # identical rows: what score_f64 needs
        for seq, sc in zip(a.result.sequences_ids, a.result.scores):
            d = abs(sc - SS.score_f64(seq, SS.ended_on_eot(s, seq), lg[:, 0], o, s.apply_ts))
            if d > worst:
                worst, where = d, name
    print("largest |oracle float32 score - score_f64|:", worst, where)
    assert worst <= SS.ORACLE_SCORE_ERR, (worst, where)
    assert worst >= SS.ORACLE_SCORE_ERR / 2                                      # the constant is the measurement, not a loose bound
    assert SS.DEVICE_SCORE_TOL == 8 * SS.ORACLE_SCORE_ERR and SS.device_tol(0.3) == SS.DEVICE_SCORE_TOL < 1e-3 and SS.device_tol(1e6) == SS.DEVICE_SCORE_TOL


@pytest.mark.parametrize("name", ALL)
def test_deciding_scores_are_separated(name):
    """Through the oracle's observer (tests/search_cases.py _Watch): neighbours among the kept candidates, the last kept candidate and the
    first dropped one, the hypotheses returned and the first left out differ by more than 1e-3. No case is exempt; rows on their own
    (greedy / sampling) rank nothing across rows."""
    s, a = SS.SCRIPTS[name], SS.answer(name)
    if s.beam_mode:
        assert a.margin > SS.MARGIN, (name, a.margin, a.where)
    else:
        assert a.margin == float("inf")


@pytest.mark.parametrize("beam,patience,stop", [(3, 1.5, 5), (5, 0.5, 3), (5, 2.5, 13), (5, 1.0, 5), (16, 2.0, 32), (2, 0.2, 1)])
def test_patience_rounds_halves_up_like_the_engine(beam, patience, stop):
    """beam * patience halves: 4.5 -> 5, 2.5 -> 3, 12.5 -> 13 (std::lround in the engine; Python's round() gave 4, 2, 12). The search stops at the
    step that brings the finished hypotheses to that count: with one hypothesis finishing per step, the count itself."""
    s = SS.SCRIPTS["finish-beam5-patience2.5"]
    ids, V = s.ids, s.V
    script = [ids.timestamp_begin] + [100 + i for i in range(2 * stop + 2)] if stop > 16 else s.script
    lg = SS.scripted_logits(script, beam, V, ids, SS.GAP, seed=11)
    for t in range(1, len(script)):
        lg[t, :, ids.eot] = lg[t, :, script[t]] - np.float32(4.0)
    o = odec.GenOptions(ids=ids, beam_size=beam, patience=patience, num_hypotheses=1, max_length=1 + len(script) + 1, suppress_tokens=SC.suppress_list(ids))
    seen = []
    res = odec.generate(odec.InjectedLogits(lg), [ids.sot], o, observer=seen.append)
    n = len(seen[-1]["hyps"])
    assert res.steps < len(script)                                                # ended by the count
    assert stop <= n < stop + beam and n - stop < 2, (n, stop)                    # (a wide beam may finish two in its last step)


# ---- violations itself
def _o(**kw):
    ids = SC.token_ids(2310)
    d = dict(suppress_tokens=SC.suppress_list(ids), suppress_blank=True, no_repeat_ngram_size=0, max_initial_timestamp_index=50)
    d.update(kw)
    return ids, types.SimpleNamespace(ids=ids, **d)


TB = 809
BAD = [
    ("not a timestamp", [100, 101], {}, True),
    ("past max_initial_timestamp_index", [TB + 51, 100], {}, True),
    ("past max_initial_timestamp_index", [TB + 1, 100], dict(max_initial_timestamp_index=0), True),
    ("decreases", [TB, 100, TB + 9, TB + 9, 101, TB + 8], {}, True),
    ("not strictly greater after text", [TB, 100, TB + 7, TB + 7, 101, TB + 7], {}, True),
    ("not strictly greater after text", [TB + 4, 100, TB + 4], {}, True),
    ("three timestamps in a row", [TB, 100, TB + 7, TB + 7, TB + 9], {}, True),
    ("directly after the opening timestamp", [TB, TB + 1, 100], {}, True),
    ("after a single timestamp that follows text", [TB, 100, TB + 7, 101], {}, True),
    ("suppressed id 14", [TB, 100, 14], {}, True),
    ("suppressed id 14", [100, 14], {}, False),
    ("<|notimestamps|>", [TB, 808, 100], {}, True),
    ("blank or end-of-text first", [220, 100], {}, False),
    ("blank or end-of-text first", [702, 100], {}, False),
    ("1-gram (100,)", [100, 101, 100], dict(no_repeat_ngram_size=1), False),
    ("2-gram (100, 101)", [100, 101, 102, 100, 101], dict(no_repeat_ngram_size=2), False),
    ("3-gram (100, 816, 816)", [TB, 100, 816, 816, 100, 816, 816], dict(no_repeat_ngram_size=3), False),
]


@pytest.mark.parametrize("what,seq,kw,apply_ts", BAD, ids=[f"{i}-{b[0][:24]}" for i, b in enumerate(BAD)])
def test_violations_reports_each_kind(what, seq, kw, apply_ts):
    ids, o = _o(**kw)
    got = SS.violations(seq, ids, o, apply_ts)
    assert len(got) == 1 and what in got[0], got


def test_violations_passes_what_is_legal():
    ids, o = _o()
    for seq in ([], [TB], [TB, 100, TB + 7, TB + 7, 101, TB + 8, TB + 8], [TB + 50, 100, TB + 51], [TB, 100, TB + 1500, TB + 1500], [TB, 100, TB + 3, TB + 9, 101],
                [TB, 703 + 1, 100], [TB, 100, TB + 7, 704, 101]):           # (704: a special id between end-of-text and the timestamps is no text)
        assert SS.violations(seq, ids, o, True) == [], seq
    for seq in ([100, 101, 100, 101], [TB + 9, TB + 3, TB + 3, TB + 3, 100], [808], [TB + 51]):
        assert SS.violations(seq, ids, o, False) == [], seq
    ids, o = _o(suppress_blank=False)
    assert SS.violations([220], ids, o, False) == []
    ids, o = _o(no_repeat_ngram_size=3)
    assert SS.violations([100, 101, 102, 103, 101, 102, 104, 100, 101], ids, o, False) == []
    ids, o = _o(max_initial_timestamp_index=-1)
    assert SS.violations([TB + 900, 100], ids, o, True) == []


def test_rules_f64_by_hand():
    """three rows small enough to read: the pair rule, the strict increase after text, the mass rule on both sides"""
    ids = odec.TokenIds(sot=5, eot=4, no_timestamps=7, timestamp_begin=8, no_speech=6, blank=0)
    o = types.SimpleNamespace(ids=ids, suppress_tokens=[1], suppress_blank=True, no_repeat_ngram_size=0, repetition_penalty=1.0, max_initial_timestamp_index=1)
    row = np.zeros(12)
    row[2] = 5.0
    alive = lambda h, r=row: np.flatnonzero(np.isfinite(SS.rules_f64(r, h, o, True)[0])).tolist()
    assert alive([]) == [8, 9]                                  # first: timestamps up to index 1
    assert alive([8]) == [0, 2, 3, 4, 5, 6]                     # after the opening timestamp: no timestamp, not <|notimestamps|>, not the suppressed id
    assert alive([8, 2]) == [0, 2, 3, 4, 5, 6, 9, 10, 11]       # 8 is not strictly greater; mass: log(3 * e^0) = 1.1 < 5 -> text stays ...
    quiet = np.zeros(12)
    assert alive([8, 2], quiet) == [9, 10, 11]                  # ... and with flat text, three timestamps outweigh every single text id
    assert alive([8, 2, 9], quiet) == [9, 10, 11]               # one timestamp after text: its partner (9 may repeat) or the end; 4 (eot) is text for the mass rule
    assert alive([8, 2, 9, 9], quiet) == [0, 2, 3, 4, 5, 6]     # pair closed: no timestamp
    v, lse = SS.rules_f64(row, [8], o, True)
    assert abs(lse - np.log(np.exp(5.0) + 5.0)) < 1e-12
