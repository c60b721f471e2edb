"""GPU (-m gpu): grammar-constrained decoding end to end. On the seeded tiny.en model of the parity tests, through wlx_generate_ex
(Slot.generate): with a grammar installed the text tokens of every returned hypothesis are a string of the language — beam 5, beam 1 and
sampling at temperature 1.0, with and without timestamps, one item and a batch of 3 — and the same windows decoded without one are not,
which is what fails on an engine without the feature. On the TRAINED checkpoint tests/golden/trained_tiny (a word of its language is one
token, 300 + w, spelled " w30x"), through WhisperModelHIP: a grammar of the transcript's words plus distractors reproduces the pinned
transcript, a grammar of distractors alone yields distractors, and one POST with `grammar` fields answers like transcribe(grammar=).

Every state of the tiny.en grammar accepts (each first token is a phrase of its own and the start of two-token phrases), so a hypothesis
that runs into the step budget is still a string of the language and `accepts` holds without an exception for it."""
import http.client
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.golden.make_trained_tiny import utterance
from tests.test_gpu_keyword_bias import KW, WordTokenizer, _tokens, _wav
from whisperlive_amd import grammar as G

pytestmark = pytest.mark.gpu

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_tiny")
FIRST = list(range(1000, 1016))
SECOND = list(range(2000, 2012))
STEPS = 12


@pytest.fixture(scope="module")
def tiny(gpu):
    from oracle.logmel import speech_like_pcm
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    spec = H.TINY_EN
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7))
    ids = H.token_ids_for(spec.vocab)
    g = G.compile_grammar(None, [[a] for a in FIRST] + [[a, b] for a in FIRST for b in SECOND], vocab=spec.vocab, eot=ids.eot)
    assert g.n_states == 17 and np.all(g.accept == 1)
    clips = [speech_like_pcm(4.0 + b, seed=100 + b) for b in range(3)]

    def encoded(slot, n):
        T = [slot.logmel(clips[b], item=b) for b in range(n)]
        slot.encode(n, seek=[0] * n, seg=[t - 1 for t in T])

    yield dict(eng=eng, ids=ids, eids=H.engine_ids(ids), g=g, encoded=encoded, sup=H.default_suppress(ids))
    eng.close()


MODES = {"beam5": dict(beam_size=5, num_hypotheses=5), "beam1": dict(beam_size=1),
         "sampling": dict(beam_size=1, num_hypotheses=3, sampling_temperature=1.0, sampling_topk=0, seed=11)}


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("timestamps", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_hypothesis_is_in_the_language(tiny, mode, timestamps, batch):
    ids, g = tiny["ids"], tiny["g"]
    prompt = [ids.sot] if timestamps else [ids.sot, ids.no_timestamps]
    kw = dict(MODES[mode], max_length=len(prompt) + STEPS, suppress_tokens=tiny["sup"])
    slot = tiny["eng"].create_slot(batch, 5)
    try:
        tiny["encoded"](slot, batch)
        plain = slot.generate([prompt] * batch, tiny["eids"], **kw)
        slot.set_grammar(g)
        got = slot.generate([prompt] * batch, tiny["eids"], **kw)
        text = lambda seq: [t for t in seq if t < ids.eot]
        for b in range(batch):
            assert got[b].sequences_ids and all(np.isfinite(got[b].scores)), (b, got[b].scores)
            for seq in got[b].sequences_ids:
                assert G.accepts(g, seq), (mode, timestamps, b, seq)
            print(mode, timestamps, b, "grammar", got[b].sequences_ids[0], "plain", plain[b].sequences_ids[0])
        # the same windows without a grammar leave the language (random weights: the first text token is none of sixteen in 50000)
        assert all(text(p.sequences_ids[0]) and not G.accepts(g, p.sequences_ids[0]) for p in plain), [p.sequences_ids[0] for p in plain]
        # no_speech_prob is defined by the raw row: the same bits with and without a grammar
        assert [x.no_speech_prob for x in got] == [p.no_speech_prob for p in plain]
        # cleared: tokens, scores and no_speech_prob are those of the decode this slot made on the same encoder output before it ever had a
        # grammar, bit for bit. (Against a SECOND slot that never had one the comparison is made on injected logits, bit for bit, in
        # tests/test_gpu_grammar_search.py: two slots that encode the same audio each for themselves differ in the fifth digit of a score
        # on this model with no grammar anywhere, so a second slot here would compare encoders, not the launch list.)
        slot.clear_grammar()
        after = slot.generate([prompt] * batch, tiny["eids"], **kw)
        assert [(x.sequences_ids, x.scores, x.no_speech_prob) for x in after] == [(x.sequences_ids, x.scores, x.no_speech_prob) for x in plain]
    finally:
        slot.close()


def test_a_generate_with_another_end_of_text_is_refused(tiny):
    from whisperlive_amd import _lib
    from whisperlive_amd.engine import TokenIds
    ids = tiny["ids"]
    slot = tiny["eng"].create_slot(1, 5)
    try:
        tiny["encoded"](slot, 1)
        slot.set_grammar(tiny["g"])
        other = TokenIds(ids.sot, ids.eot - 1, ids.no_timestamps, ids.timestamp_begin, ids.no_speech, ids.blank)
        with pytest.raises(_lib.WlxError) as ei:
            slot.generate([[ids.sot]], other, beam_size=5, max_length=4)
        assert ei.value.code == _lib.ERR_ARG and "end-of-text" in str(ei.value)
    finally:
        slot.close()


# ---------------------------------------------------------------------------------------------------- the trained checkpoint
@pytest.fixture(scope="module")
def trained(gpu):
    import tokenizers
    from whisperlive_amd.transcriber import WhisperModelHIP
    tok = WordTokenizer(tokenizers.Tokenizer.from_file(os.path.join(DIR, "tokenizer.json")))
    model = WhisperModelHIP(DIR, device="cuda", device_index=0, hf_tokenizer=tok, max_batch=4)
    with open(os.path.join(DIR, "expected.json")) as f:
        exp = json.load(f)
    case = exp["cases"][0]
    pcm, _ws = utterance(case["seed"])
    truth = [t for t in case["truth_tokens"] if t < exp["timestamp_begin"]]
    yield dict(model=model, pcm=pcm, truth=truth, words=exp["word_token_ids"])
    model.close()
    model.engine.close()


DISTRACTORS = [[320], [321, 322], [323, 324, 325]]          # token lists: no word of the fixture's language


def test_the_transcripts_phrases_plus_distractors_transcribe_at_word_error_rate_0(trained):
    m, pcm, truth = trained["model"], trained["pcm"], trained["truth"]
    plain, _ = m.transcribe(pcm, **KW)
    assert _tokens(m, plain) == truth                                           # expected.json's transcript
    words = [f"w{t}" for t in sorted(set(truth))]
    g = m.compile_grammar(words + DISTRACTORS)
    segs, _ = m.transcribe(pcm, **KW, grammar=words + DISTRACTORS)
    got = _tokens(m, segs)
    assert got == truth and G.accepts(g, got)                                   # word error rate 0
    assert [s.no_speech_prob for s in segs] == [s.no_speech_prob for s in plain]
    # the context manager is the same scope; two-word phrases of the transcript: the window's transcript is a string of THAT language. It
    # is not the whole utterance: under this list the beam search closes the window behind the second pair (`... w301 w300 <|2.00|>`),
    # and oracle.decoding.generate on the CPU, fed the same model's logits masked by tests/grammar_ref.py, returns exactly that
    # hypothesis too — what a hard mask does to a beam search that counts masked end-of-text candidates, not the kernel
    pairs = [f"w{a} w{b}" for a, b in zip(truth[0::2], truth[1::2])] + ([f"w{truth[-1]}"] if len(truth) % 2 else [])
    with m.grammar(phrases=pairs + DISTRACTORS) as g2:
        segs2, _ = m.transcribe(pcm, **KW)
    print("pairs", pairs, [s.tokens for s in segs2], "plain", [s.tokens for s in plain])
    got2 = _tokens(m, segs2)
    assert G.accepts(g2, truth) and G.accepts(g2, got2) and len(got2) >= 4 and got2 == truth[:len(got2)], got2
    # distractors alone: the transcript is a sequence of distractors and nothing else
    gd = m.compile_grammar(DISTRACTORS)
    with m.grammar(phrases=DISTRACTORS):
        segs3, _ = m.transcribe(pcm, **KW)
    got3 = _tokens(m, segs3)
    print("distractors alone", [s.tokens for s in segs3])
    assert G.accepts(gd, got3) and not set(got3) & set(trained["words"]), got3
    # repeat=False: one phrase or nothing
    segs4, _ = m.transcribe(pcm, **KW, grammar=words, grammar_repeat=False)
    assert len(_tokens(m, segs4)) <= 1 and G.accepts(m.compile_grammar(words, False), _tokens(m, segs4))
    # out of the scope the thread decodes unconstrained again, bit for bit
    after, _ = m.transcribe(pcm, **KW)
    assert _tokens(m, after) == truth and [s.avg_logprob for s in after] == [s.avg_logprob for s in plain]
    with pytest.raises(ValueError, match="one of them"):
        m.transcribe(pcm, **KW, grammar=words, keywords=[[300]])


def test_the_batched_pipeline_transcribe_many_and_the_file_endpoint(trained):
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.rest import ROUTE, RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    m, pcm, truth = trained["model"], trained["pcm"], trained["truth"]
    clip = pcm[:int(16000 * (0.5 + 0.5 * len(truth) + 0.5))]
    pipe = BatchedInferencePipeline(m)
    bkw = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, without_timestamps=False, batch_size=2)
    gd = m.compile_grammar(DISTRACTORS)
    with m.grammar(phrases=DISTRACTORS):
        got = _tokens(m, list(pipe.transcribe(clip, **bkw)[0]))                 # (the segments arrive lazily: drawn inside the scope)
    assert G.accepts(gd, got), got
    many = pipe.transcribe_many([clip, clip], batch_size=2, language="en", beam_size=5, temperature=0.0, vad_filter=False,
                                without_timestamps=False, grammar=DISTRACTORS)
    for segs, _info in many:
        assert not isinstance(segs, Exception), segs
        assert _tokens(m, segs) == got
    assert G.current() is None
    words = [f"w{t}" for t in sorted(set(truth))]
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "trained", model_factory=lambda model, device_index, **kw: m).start()
    try:
        b = "grBoundary"

        def post(fields):
            body = b"".join([f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="u.wav"\r\nContent-Type: audio/wav\r\n\r\n'.encode(),
                             _wav(clip)] + [f'\r\n--{b}\r\nContent-Disposition: form-data; name="{k}"\r\n\r\n{v}'.encode() for k, v in fields]
                            + [f"\r\n--{b}--\r\n".encode()])
            c = http.client.HTTPConnection("127.0.0.1", server.port, timeout=120)
            c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
            r = c.getresponse()
            out = (r.status, json.loads(r.read()))
            c.close()
            return out

        two = words[:2]
        st, ans = post([("response_format", "verbose_json")] + [("grammar", w) for w in two])
        assert st == 200, ans
        ref, _ = m.transcribe(_wav(clip), temperature=0.0, vad_filter=False, grammar=two)
        assert [s["tokens"] for s in ans["segments"]] == [s.tokens for s in ref]
        assert G.accepts(m.compile_grammar(two), [t for s in ans["segments"] for t in s["tokens"]])
        st, err = post([("grammar", words[0]), ("keywords", words[1])])
        assert st == 400 and "keywords" in err["error"]
    finally:
        server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
