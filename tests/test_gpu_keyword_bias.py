"""GPU (-m gpu): keyword boosting end to end on the TRAINED checkpoint tests/golden/trained_tiny (a word of its language is one token,
300 + w, spelled " w30x"): a phrase `first word, substitute` with a large exact boost makes the substitute appear where the unbiased
transcript — the one expected.json pins — has another word; through keyword_bias, transcribe(keywords=), BatchedInferencePipeline,
transcribe_many and one POST with `keywords`. The fixture's BPE cannot re-encode " w30x" into the word's token (it spells it in bytes), so the
tokenizer the model is built with maps exactly those spellings back to their ids — the role a real vocabulary plays for real words."""
import http.client
import io
import json
import os
import re
import wave

import numpy as np
import pytest

from tests.golden.make_trained_tiny import utterance

pytestmark = pytest.mark.gpu

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_tiny")
KW = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, condition_on_previous_text=False,
          compression_ratio_threshold=None, log_prob_threshold=None, no_speech_threshold=None)
BOOST = 64.0


class WordTokenizer:
    """tokenizers.Tokenizer with `encode` of a text made of the fixture's words (" w302 w309") answering the words' own token ids"""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def encode(self, text, add_special_tokens=False):
        if re.fullmatch(r"( ?w3\d\d)+", text):
            ids = [int(w[1:]) for w in text.split()]
            return type("Encoding", (), {"ids": ids})()
        return self._inner.encode(text, add_special_tokens=add_special_tokens)


def _expected():
    with open(os.path.join(DIR, "expected.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def setup(gpu):
    import tokenizers
    from whisperlive_amd.transcriber import WhisperModelHIP
    tok = WordTokenizer(tokenizers.Tokenizer.from_file(os.path.join(DIR, "tokenizer.json")))
    model = WhisperModelHIP(DIR, device="cuda", device_index=0, hf_tokenizer=tok, max_batch=4)
    exp = _expected()
    case = exp["cases"][0]
    pcm, ws = utterance(case["seed"])
    truth = [t for t in case["truth_tokens"] if t < exp["timestamp_begin"]]
    sub = next(t for t in exp["word_token_ids"] if t not in truth[:3])        # a word the utterance does not have at its start
    yield dict(model=model, pcm=pcm, truth=truth, sub=sub, phrase=f"w{truth[0]} w{sub}")
    model.close()
    model.engine.close()


def _tokens(model, segs):
    return [t for s in segs for t in s.tokens if t < model.token_ids.eot]


def _wav(pcm):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(pcm, -1, 1) * 32767).astype("<i2").tobytes())
    return buf.getvalue()


def test_a_boosted_phrase_puts_its_word_where_the_unbiased_transcript_has_another(setup):
    m, pcm, truth, sub = setup["model"], setup["pcm"], setup["truth"], setup["sub"]
    plain, _ = m.transcribe(pcm, **KW)
    assert _tokens(m, plain) == truth                                           # expected.json's transcript
    # the phrase's first word is boosted in every state (no revocation): the token list takes exactly that back, so only the second word moves
    lb = {truth[0]: -BOOST}
    with m.keyword_bias(phrases=[setup["phrase"]], boost=BOOST, logit_bias=lb):
        biased, _ = m.transcribe(pcm, **KW)
    got = _tokens(m, biased)
    assert got[0] == truth[0] and got[1] == sub != truth[1], (got, truth)
    # the same through the arguments of transcribe, and with the phrase as token ids
    direct, _ = m.transcribe(pcm, **KW, keywords=[[truth[0], sub]], keywords_boost=BOOST, logit_bias=lb)
    assert _tokens(m, direct) == got and [s.avg_logprob for s in direct] == [s.avg_logprob for s in biased]
    # no_speech_prob is defined by the raw row: bit-identical with and without a table; the scores are those of the biased rows
    assert [s.no_speech_prob for s in biased] == [s.no_speech_prob for s in plain]
    assert biased[0].avg_logprob != plain[0].avg_logprob
    # out of the scope the thread decodes unbiased again, bit for bit
    after, _ = m.transcribe(pcm, **KW)
    assert _tokens(m, after) == truth and [s.avg_logprob for s in after] == [s.avg_logprob for s in plain]


def test_an_empty_table_reproduces_the_pinned_transcript(setup):
    m = setup["model"]
    exp = _expected()
    with m.keyword_bias(phrases=[], logit_bias={}):
        for c in exp["cases"][:3]:
            pcm, _ws = utterance(c["seed"])
            segs, _ = m.transcribe(pcm, **KW)
            assert _tokens(m, segs) == [t for t in c["truth_tokens"] if t < exp["timestamp_begin"]]


def test_set_clear_set_on_one_slot_reuses_the_graphs_and_equals_fresh_slots(setup):
    """three tables in turn on the thread's slot (the captured step graphs of the first biased call serve the others: the table lives at fixed
    addresses); each result equals that of a model whose slot never saw another table"""
    from whisperlive_amd.transcriber import WhisperModelHIP
    m, pcm, truth, sub = setup["model"], setup["pcm"], setup["truth"], setup["sub"]
    other = next(t for t in _expected()["word_token_ids"] if t not in (sub, truth[0], truth[1]))
    tables = [dict(phrases=[[truth[0], sub]], boost=BOOST, logit_bias={truth[0]: -BOOST}), None,
              dict(phrases=[[truth[0], other]], boost=BOOST, logit_bias={truth[0]: -BOOST})]

    def run(model, t):
        if t is None:
            return model.transcribe(pcm, **KW)[0]
        with model.keyword_bias(**t):
            return model.transcribe(pcm, **KW)[0]

    slot = m._slot()
    same = []
    for t in tables + tables[:1]:
        same.append(run(m, t))
        assert m._slot() is slot
    for t, got in zip(tables + tables[:1], same):
        f2 = WhisperModelHIP(DIR, device="cuda", device_index=0, engine=m.engine, hf_tokenizer=m.hf_tokenizer)      # a slot of its own
        try:
            ref = run(f2, t)
            assert _tokens(m, got) == _tokens(m, ref) and [s.avg_logprob for s in got] == [s.avg_logprob for s in ref], t
        finally:
            f2.close()
    assert _tokens(m, same[0])[1] == sub and _tokens(m, same[1]) == truth and _tokens(m, same[2])[1] == other and _tokens(m, same[3])[1] == sub


def test_batched_pipeline_transcribe_many_and_the_file_endpoint(setup):
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.rest import ROUTE, RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    m, pcm, truth, sub = setup["model"], setup["pcm"], setup["truth"], setup["sub"]
    n = int(16000 * (0.5 + 0.5 * len(truth) + 0.5))
    clip = pcm[:n]
    pipe = BatchedInferencePipeline(m)
    bkw = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, without_timestamps=False, batch_size=2)
    plain = list(pipe.transcribe(clip, **bkw)[0])
    words = [t for t in _tokens(m, plain) if 300 <= t < 310]
    assert words == truth
    lb = {truth[0]: -BOOST}
    with m.keyword_bias(phrases=[setup["phrase"]], boost=BOOST, logit_bias=lb):
        biased = list(pipe.transcribe(clip, **bkw)[0])                          # (the segments arrive lazily: drawn inside the scope)
        many = pipe.transcribe_many([clip, clip], batch_size=2, language="en", beam_size=5, temperature=0.0, vad_filter=False,
                                    without_timestamps=False)
    got = [t for t in _tokens(m, biased) if 300 <= t < 310]
    assert got[0] == truth[0] and got[1] == sub, (got, truth)
    for segs, info in many:
        assert not isinstance(segs, Exception), segs
        w = [t for t in _tokens(m, segs) if 300 <= t < 310]
        assert w[0] == truth[0] and w[1] == sub, w
    # one POST with `keywords`: the root's boost of the first word is not taken back here, so the table is the phrase alone and the
    # endpoint's answer equals a direct call under the same table
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "trained", model_factory=lambda model, device_index, **kw: m).start()
    try:
        b = "kwBoundary"

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

        st, unb = post([("response_format", "verbose_json")])
        assert st == 200, unb
        st, ans = post([("response_format", "verbose_json"), ("keywords", setup["phrase"]), ("keywords_boost", str(BOOST))])
        assert st == 200, ans
        with m.keyword_bias(phrases=[setup["phrase"]], boost=BOOST):
            ref, _ = m.transcribe(_wav(clip), temperature=0.0, vad_filter=False)
        assert [s["tokens"] for s in ans["segments"]] == [s.tokens for s in ref]
        assert ans["text"] != unb["text"] and f"w{sub}" in ans["text"], (ans["text"], unb["text"])
        st, err = post([("keywords", setup["phrase"]), ("keywords_boost", "nan")])
        assert st == 400 and "keywords_boost" in err["error"]
    finally:
        server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
