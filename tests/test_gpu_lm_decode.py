"""GPU (-m gpu): n-gram language-model fusion end to end. On the seeded MICRO model with the synthetic tokenizer, through
WhisperModelHIP.transcribe(lm=, lm_weight=): the fused call's tokens differ from the unfused call's and equal a second fused call's;
out of the scope the same slot — whose step graphs were captured before the model came — answers like it did before, bit for bit; the
batched pipeline and transcribe_many decode one file like transcribe's scope does."""
import pytest

from tests import helpers as H
from tests import search_cases as SC
from whisperlive_amd import lm as L
from whisperlive_amd.tokenizer import synthetic_tokenizer

pytestmark = pytest.mark.gpu

V = H.MICRO.vocab
IDS = SC.token_ids(V)
KW = dict(language="en", vad_filter=False, condition_on_previous_text=False, no_speech_threshold=None, log_prob_threshold=None,
          compression_ratio_threshold=None, max_new_tokens=16, beam_size=5, temperature=0.0)
# random weights know no language: a handful of words the model makes 6 nats likelier each, at a weight that outweighs the logits' spread
CORPUS = [[300, 301, 302], [300, 301, 303], [301, 302, 300, 301], [304, 300], [302, 305, 301]]
WEIGHT = 4.0


@pytest.fixture(scope="module")
def model(gpu):
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights
    m = WhisperModelHIP("rand", weights=random_weights(H.MICRO, seed=3), spec=H.MICRO, hf_tokenizer=synthetic_tokenizer(V), max_batch=4,
                        multilingual=False)
    yield m
    m.close()
    m.engine.close()


def answer(segments):
    return [(s.tokens, s.avg_logprob) for s in segments]


def test_the_fusion_acts_repeats_and_leaves_with_its_scope(model):
    from oracle.logmel import speech_like_pcm
    from whisperlive_amd.batched import BatchedInferencePipeline
    clip = speech_like_pcm(3.0, seed=200)
    lm = L.NgramLM.from_corpus(CORPUS, None, order=3, eot=IDS.eot, vocab=V)
    plain = answer(model.transcribe(clip, **KW)[0])             # (captures the slot's step graphs without the launch)
    fused = answer(model.transcribe(clip, **KW, lm=lm, lm_weight=WEIGHT)[0])
    again = answer(model.transcribe(clip, **KW, lm=lm, lm_weight=WEIGHT)[0])
    print("plain", plain, "fused", fused)
    assert [t for t, _ in fused] != [t for t, _ in plain] and fused == again
    assert any(t in (300, 301, 302) for toks, _ in fused for t in toks)
    assert L.current() is None
    assert answer(model.transcribe(clip, **KW)[0]) == plain     # the graphs captured before the model came, replayed: bit for bit
    with model.language_model(lm, WEIGHT):
        assert answer(model.transcribe(clip, **KW)[0]) == fused
    # the batched routes take the same model: one file through the pipeline and as a job of one
    pipe = BatchedInferencePipeline(model)
    kw = dict(batch_size=2, language="en", beam_size=5, temperature=0.0, vad_filter=False)
    one, _ = pipe.transcribe(clip, **kw, lm=lm, lm_weight=WEIGHT)
    many = pipe.transcribe_many([clip], **kw, lm=lm, lm_weight=WEIGHT)
    raw, _ = pipe.transcribe(clip, **kw)
    assert [s.tokens for s in one] == [s.tokens for s in many[0][0]] != [s.tokens for s in raw]
    with pytest.raises(ValueError, match="out of scope"):
        pipe.transcribe_many([clip], **kw, lm=[lm])
