"""CPU tests of the n-gram language-model fusion's host side (whisperlive_amd/lm.py): a counted model sums to one in every
context, an ARPA model scores and moves like a brute-force dictionary backoff scorer, the bindings against include/wlx_lm.h, the
mode-exclusivity refusals on the scripted engine of tests/fakes.py, and the caps."""
import math
import os
import re

import numpy as np
import pytest

from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd import lm as L
from whisperlive_amd.tokenizer import synthetic_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN10 = math.log(10.0)
EOT = 12
ARPA = """\\data\\
ngram 1=7
ngram 2=5
ngram 3=3

\\1-grams:
-1.0 <unk>
-99 <s> -0.5
-0.9 </s>
-0.7 1 -0.4
-0.8 2 -0.3
-1.1 3 -0.2
-1.3 5

\\2-grams:
-0.3 <s> 1 -0.25
-0.6 1 2 -0.35
-0.5 2 3
-0.4 2 </s>
-0.9 3 1

\\3-grams:
-0.2 <s> 1 2
-0.1 1 2 3
-0.45 1 2 </s>

\\end\\
"""
B = L.BOS
# the same file as dictionaries, log10: P[context + (word,)], BOW[context]
P = {(12,): -0.9, (1,): -0.7, (2,): -0.8, (3,): -1.1, (5,): -1.3, (B, 1): -0.3, (1, 2): -0.6, (2, 3): -0.5, (2, 12): -0.4, (3, 1): -0.9,
     (B, 1, 2): -0.2, (1, 2, 3): -0.1, (1, 2, 12): -0.45}
BOW = {(B,): -0.5, (1,): -0.4, (2,): -0.3, (3,): -0.2, (B, 1): -0.25, (1, 2): -0.35}
UNSEEN = [t for t in range(EOT + 1) if (t,) not in P]           # they share the <unk> mass of 10^-1


def brute(hist, w):
    if not hist:
        return P[(w,)] * LN10 if (w,) in P else math.log(0.1 / len(UNSEEN))
    if hist + (w,) in P:
        return P[hist + (w,)] * LN10
    return BOW.get(hist, 0.0) * LN10 + brute(hist[1:], w)


@pytest.mark.parametrize("hist", [[], [1], [1, 2], [1, 2, 3], [5], [4], [2, 3], [1, 2, 3, 1], [3, 1, 2], [1, 13, 2, 14]])
def test_an_arpa_model_scores_and_moves_like_a_dictionary_backoff_scorer(hist):
    m = L.NgramLM.from_arpa(ARPA, eot=EOT, vocab=16)
    state = m.start_state
    for t in hist:
        state = m.next_state(state, t)
    text = tuple(t for t in hist if t < EOT)                    # ids >= eot are transparent
    want = [brute(((B,) + text)[-2:], w) for w in range(EOT + 1)]
    assert np.allclose(m.score_row(state), want, rtol=0, atol=2e-6), (hist, state)


def test_every_context_of_a_counted_model_sums_to_one():
    rng = np.random.default_rng(0)
    texts = [[int(t) for t in rng.integers(0, 9, size=int(rng.integers(1, 9)))] for _ in range(40)]
    for order in (1, 2, 3, 5):
        m = L.NgramLM.from_corpus(texts, None, order=order, eot=EOT, vocab=20)
        assert m.order == order and (order == 1) == (m.n_states == 1)
        for s in range(m.n_states):
            assert abs(np.exp(m.score_row(s)).sum() - 1.0) < 2e-6, (order, s)
    # fuse_row keeps the mass of A and everything behind eot
    row = rng.standard_normal(20) * 4
    row[3] = -np.inf
    out = m.fuse_row(row, m.start_state, 0.7)
    assert np.isclose(np.exp(out[:EOT + 1]).sum(), np.exp(row[:EOT + 1]).sum()) and out[3] == -np.inf and (out[EOT + 1:] == row[EOT + 1:]).all()
    assert not np.allclose(out[:3], row[:3])
    # a tokenizer's strings count like its token lists
    tk = synthetic_tokenizer(2310)
    from whisperlive_amd.tokenizer import Tokenizer
    t = Tokenizer(tk, True, task="transcribe", language="en")
    a = L.NgramLM.from_corpus(["ab ab", "ba"], t, order=2)
    b = L.NgramLM.from_corpus([t.encode("ab ab"), t.encode("ba")], None, order=2, eot=t.eot)
    assert a.eot == t.eot and all(np.array_equal(x, y) for x, y in zip(a.packed(), b.packed()))


def test_the_bindings_are_the_functions_of_wlx_lm_h():
    text = open(os.path.join(ROOT, "include", "wlx_lm.h")).read()
    assert re.findall(r"^int32_t\s+(wlx_\w+)\(", text, flags=re.M) == _lib.EXPORTS_LM
    assert '#include "wlx_lm.h"' in open(os.path.join(ROOT, "include", "wlx.h")).read()
    for name, value in (("ORDER", _lib.LM_MAX_ORDER), ("STATES", _lib.LM_MAX_STATES), ("EDGES", _lib.LM_MAX_EDGES), ("VOCAB", _lib.LM_MAX_VOCAB),
                        ("MODELS", _lib.LM_MAX_MODELS)):
        assert eval(re.search(rf"#define WLX_LM_MAX_{name} (.+)", text).group(1)) == value


class LmSlot(FakeSlot):
    def set_lm(self, lm, weight):
        self.calls.append(("set_lm", lm, weight))

    def clear_lm(self):
        self.calls.append(("clear_lm",))


class LmEngine(FakeEngine):
    slot_type = LmSlot


def test_one_mode_at_a_time_and_the_scope_reaches_the_slot():
    from whisperlive_amd.transcriber import WhisperModelHIP
    eng = LmEngine()
    eng.default_tokens = [50, 51]
    m = WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(2310))
    lm = L.NgramLM.from_corpus([[5, 6, 7]], None, order=2, eot=m.token_ids.eot, vocab=m.spec.vocab)
    pcm, kw = np.zeros(16000, np.float32), dict(language="en", temperature=0.0, vad_filter=False)
    slot = m._slot()
    m.transcribe(pcm, **kw, lm=lm, lm_weight=0.5)
    m.transcribe(pcm, **kw, lm=lm, lm_weight=0.5)               # the same model and weight again: set once
    m.transcribe(pcm, **kw)
    calls = [c for c in slot.calls if c[0] in ("set_lm", "clear_lm", "generate")]
    assert [c[0] for c in calls] == ["set_lm", "generate", "generate", "clear_lm", "generate"] and calls[0][1:] == (lm, 0.5)
    with m.language_model(lm) as v:
        assert v == (lm, L.DEFAULT_WEIGHT)
    for extra in (dict(keywords=[[5, 6]]), dict(logit_bias={5: 1.0}), dict(grammar=[[5]]), dict(grammar_pattern="a+")):
        with pytest.raises(ValueError, match="out of scope"):
            m.transcribe(pcm, **kw, lm=lm, **extra)
    with m.keyword_bias(phrases=[[5, 6]]):
        with pytest.raises(ValueError, match="language model together with keyword boosting is out of scope"):
            m.language_model(lm)
    with m.grammar(phrases=[[5]]):
        with pytest.raises(ValueError, match="language model together with a grammar is out of scope"):
            m.language_model(lm)
    with m.language_model(lm):
        with m.grammar(pattern="a+"):
            with pytest.raises(ValueError, match="language model together with a grammar is out of scope"):
                m.transcribe(pcm, **kw)
    with pytest.raises(ValueError, match="per file or per item is out of scope"):
        m.language_model([lm, lm])
    with pytest.raises(ValueError, match="weight"):
        m.language_model(lm, 0.0)
    with pytest.raises(ValueError, match="end-of-text"):
        m.language_model(L.NgramLM.from_arpa(ARPA, eot=EOT))
    with pytest.raises(ValueError, match="word-level ARPA"):
        L.NgramLM.from_arpa(ARPA.replace("-0.9 3 1", "-0.9 3 hello"), eot=EOT)


@pytest.mark.parametrize("name, build", [
    ("order", lambda: L.NgramLM.from_corpus([[1, 2]], None, order=6, eot=EOT)),
    ("vocab", lambda: L.NgramLM.from_corpus([[1, 2]], None, order=2, eot=EOT, vocab=_lib.LM_MAX_VOCAB + 1)),
    ("states", lambda: L.NgramLM(16, EOT, 2, 0, np.zeros(_lib.LM_MAX_STATES + 2), np.zeros(_lib.LM_MAX_STATES + 1),
                                 np.zeros(_lib.LM_MAX_STATES + 1), [], [], [], np.zeros(16), np.zeros(16))),
    ("edges", lambda: L.NgramLM(16, EOT, 2, 0, [0, 0, _lib.LM_MAX_EDGES + 1], [0, 0], [0, 0], np.zeros(_lib.LM_MAX_EDGES + 1, np.int32),
                                np.zeros(_lib.LM_MAX_EDGES + 1, np.float32), np.zeros(_lib.LM_MAX_EDGES + 1, np.int32), np.zeros(16), np.zeros(16))),
])
def test_each_cap_is_refused_by_name(name, build):
    with pytest.raises(ValueError, match=name):
        build()
