"""GPU (-m gpu): regular-expression grammars end to end. On the seeded MICRO model with the synthetic tokenizer (text tokens
are the 256 single bytes and ` w<id>`), through WhisperModelHIP: under `grammar_pattern` the text of every window fully matches the
pattern — beam search, sampling at a temperature, and a batched transcribe_many of three files — and every avg_logprob is finite, while
the same calls without the pattern leave the language (asserted: the test cannot pass on a lucky seed). Out of the scope the model
answers like a fresh one, token for token. On injected logits (the wlx_debug_search hooks, as tests/test_gpu_grammar_search.py drives
them) the device's tokens and scores equal the oracle search run on logits masked by a Python loop over the tokens' bytes."""
import itertools

import numpy as np
import pytest

from oracle import decoding as odec
from tests import helpers as H
from tests import search_cases as SC
from tests.test_gpu_grammar_search import budgets, check, planted
from whisperlive_amd import pattern as P
from whisperlive_amd.tokenizer import synthetic_tokenizer

pytestmark = pytest.mark.gpu

V = H.MICRO.vocab
IDS = SC.token_ids(V)
# Random weights never reach end-of-text inside a step budget, so the pattern is one whose every reachable state accepts (a window cut
# at its budget is still a string of the language, as in tests/test_gpu_grammar.py): words whose number starts with 3, 4 or 5. The
# only way into a state that does not accept is the lone space token, which the default suppress list removes.
REGEX = r"( w[3-5][0-9]*)+"
# a window here is one whole decode: no timestamps (with them the transcriber cuts a window at its last timestamp pair and decodes the rest
# again from the start state; random weights put timestamps anywhere, so they are suppressed outright)
NO_TS = dict(without_timestamps=True, suppress_tokens=[-1] + list(range(IDS.timestamp_begin, V)))
KW = dict(language="en", vad_filter=False, condition_on_previous_text=False, no_speech_threshold=None, log_prob_threshold=None,
          compression_ratio_threshold=None, max_new_tokens=24, **NO_TS)
MODES = {"beam": dict(beam_size=5, temperature=0.0), "sampling": dict(beam_size=1, best_of=2, temperature=0.7)}


@pytest.fixture(scope="module")
def vocab():
    tk = synthetic_tokenizer(V)
    off, by = P.token_bytes(tk, IDS.eot)
    return tk, off, [bytes(by[off[t]:off[t + 1]]) for t in range(IDS.eot)]


def _model(seed=3):
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights
    return WhisperModelHIP("rand", weights=random_weights(H.MICRO, seed=seed), spec=H.MICRO, hf_tokenizer=synthetic_tokenizer(V), max_batch=4,
                           multilingual=False)


@pytest.fixture(scope="module")
def model(gpu):
    m = _model()
    yield m
    m.close()
    m.engine.close()


@pytest.fixture(scope="module")
def clips():
    from oracle.logmel import speech_like_pcm
    return [speech_like_pcm(3.0 + b, seed=200 + b) for b in range(3)]


def windows(segments, words):
    """the text of each window as bytes: the text tokens of the segments that share a seek"""
    return [b"".join(words[t] for s in grp for t in s.tokens if t < IDS.eot) for _seek, grp in itertools.groupby(segments, key=lambda s: s.seek)]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_window_fully_matches_the_pattern(model, clips, vocab, mode):
    _tk, _off, words = vocab
    pat = P.compile_pattern(REGEX)
    plain = [list(model.transcribe(c, **KW, **MODES[mode])[0]) for c in clips]
    got = [list(model.transcribe(c, **KW, **MODES[mode], grammar_pattern=REGEX)[0]) for c in clips]
    for segs, raw in zip(got, plain):
        texts = windows(segs, words)
        print(mode, "pattern", texts, "plain", windows(raw, words))
        assert texts and all(pat.accepts(t) for t in texts), texts
        assert all(np.isfinite(s.avg_logprob) for s in segs)
    assert any(not pat.accepts(t) for raw in plain for t in windows(raw, words))          # without the pattern the model leaves the language
    assert P.current() is None
    # out of the scope the slot's step is the launch list of a slot that never had a pattern: a fresh model answers the same, token for token
    after = [list(model.transcribe(c, **KW, **MODES["beam"])[0]) for c in clips]
    fresh = _model()
    try:
        ref = [list(fresh.transcribe(c, **KW, **MODES["beam"])[0]) for c in clips]
    finally:
        fresh.close()
        fresh.engine.close()
    assert [[s.tokens for s in f] for f in after] == [[s.tokens for s in f] for f in ref]


def test_three_files_as_one_batched_job(model, clips, vocab):
    from whisperlive_amd.batched import BatchedInferencePipeline
    _tk, _off, words = vocab
    pat = P.compile_pattern(REGEX)
    pipe = BatchedInferencePipeline(model)
    kw = dict(batch_size=2, language="en", beam_size=5, temperature=0.0, vad_filter=False, **NO_TS)
    many = pipe.transcribe_many(clips, **kw, grammar_pattern=REGEX)
    plain = pipe.transcribe_many(clips, **kw)
    assert len(many) == 3
    for segs, _info in many:
        assert not isinstance(segs, Exception), segs
        assert segs and all(pat.accepts(t) for t in windows(segs, words)) and all(np.isfinite(s.avg_logprob) for s in segs)
    assert any(not pat.accepts(t) for segs, _ in plain for t in windows(segs, words))
    one, _info = pipe.transcribe(clips[0], **kw, grammar_pattern=REGEX)
    assert [s.tokens for s in one] == [s.tokens for s in many[0][0]]
    assert P.current() is None


EXCLUDED = {"keywords": dict(keywords=[" w300"]), "phrases": dict(grammar=[" w300"]), "per item": dict(grammar_pattern=[REGEX, REGEX, REGEX])}


@pytest.mark.parametrize("what", sorted(EXCLUDED))
def test_what_is_out_of_scope_is_a_value_error(model, clips, what):
    from whisperlive_amd.batched import BatchedInferencePipeline
    kw = dict({"grammar_pattern": REGEX}, **EXCLUDED[what])
    with pytest.raises(ValueError, match="out of scope"):
        BatchedInferencePipeline(model).transcribe_many(clips, batch_size=2, language="en", vad_filter=False, **kw)
    if what != "per item":
        with pytest.raises(ValueError, match="out of scope"):
            model.transcribe(clips[0], **KW, **kw)
    with pytest.raises(ValueError, match="out of scope"):
        model.grammar(phrases=[" w300"], pattern=REGEX)


# ---------------------------------------------------------------------------------------------------- injected logits
class MaskedLogits(odec.InjectedLogits):
    """injected logits under the pattern: each row's state follows `parents` over the fed token's bytes; a text token keeps its logit iff
    it has bytes and they can be walked from the row's state, end-of-text iff the state accepts"""

    def __init__(self, logits, pat, words, plen):
        super().__init__(logits)
        self.pat, self.words, self.plen, self.states, self.pos = pat, words, plen, None, plen - 1

    def next_state(self, ps, tok):
        if self.pos < self.plen or tok >= IDS.eot:
            return 0 if self.pos < self.plen else ps
        return max(self.pat.step(ps, self.words[tok]), 0) if self.words[tok] else 0

    def step(self, tokens, parents):
        if self.states is None:
            self.states = [0] * len(tokens)
        else:
            self.pos += 1
            self.states = [self.next_state(self.states[p], int(t)) for p, t in zip(parents, tokens)]
        out = np.array(super().step(tokens, parents), dtype=np.float32, copy=True)
        for r, s in enumerate(self.states):
            for t in range(IDS.eot):
                if not self.words[t] or self.pat.step(s, self.words[t]) < 0:
                    out[r, t] = -np.inf
            if not self.pat.accept[s]:
                out[r, IDS.eot] = -np.inf
        return out


def test_beam_search_under_a_pattern_equals_the_masked_oracle(gpu, vocab):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    _tk, off, words = vocab
    c = SC.CASES["batch3x5-micro"]
    pat = P.compile_pattern(REGEX)                              # wide: every state allows dozens of ` w<id>` tokens (the planted ones among them)
    lg = planted(c, c.logits())
    o, ref, margin = c.opts(), [], float("inf")
    for b, prompt in enumerate(c.prompts):
        w = SC._Watch(c.R, max(1, o.num_hypotheses), c.ids.eot)
        ref.append(odec.generate(MaskedLogits(c.item_logits(lg, b), pat, words, len(prompt)), prompt, o, row_base=b * c.R, observer=w))
        margin = min(margin, w.margin)
    assert margin > SC.MARGIN, margin
    text = lambda seq: b"".join(words[t] for t in seq if t < IDS.eot)
    full = lambda res, n: all(pat.accepts(text(s)) or len(s) >= n for s in res.sequences_ids)
    plain = [odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), p, o, row_base=b * c.R) for b, p in enumerate(c.prompts)]
    assert all(full(r, n) for r, n in zip(ref, budgets(c))) and not all(full(r, n) for r, n in zip(plain, budgets(c)))
    eng = HipWhisperEngine(H.MICRO, random_weights(H.MICRO, seed=3))
    slot = eng.create_slot(c.items, 16)
    try:
        eng.set_pattern_vocab(IDS.eot, off, np.frombuffer(b"".join(words), np.uint8))
        slot.set_pattern(pat)
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), ref, sampling=False)
        slot.clear_pattern()                                    # cleared: the unconstrained answer again
        check(slot.debug_search_batch(lg, c.prompts, H.engine_ids(c.ids), **c.gen_kw), plain, sampling=False)
    finally:
        slot.close()
        eng.close()
