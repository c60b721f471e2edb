"""GPU (-m gpu): keyword boosting per file, end to end on the TRAINED checkpoint of tests/test_gpu_keyword_bias.py (a word is one token,
300 + w): one transcribe_many job over three files with the keyword lists (X, none, Y) and a batch_size that puts all three into ONE
decode group — each file's transcript is the one its own list gives it alone, and a substitute word appears only in its own file; a
refused list costs only its file; a list the closed form refuses decodes through compact=True; two uploads with different `keywords`
pooled into one job of the file endpoint against the same uploads sent alone; two live sessions with different keywords in one batch of
the batch worker against each on its own slot."""
import http.client
import json
import os
import threading
from unittest.mock import MagicMock

import pytest

from tests.golden.make_trained_tiny import utterance
from tests.test_gpu_keyword_bias import BOOST, DIR, WordTokenizer, _expected, _tokens, _wav

pytestmark = pytest.mark.gpu

BKW = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, without_timestamps=False)


@pytest.fixture(scope="module")
def setup(gpu):
    import tokenizers
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.transcriber import WhisperModelHIP
    tok = WordTokenizer(tokenizers.Tokenizer.from_file(os.path.join(DIR, "tokenizer.json")))
    model = WhisperModelHIP(DIR, device="cuda", device_index=0, hf_tokenizer=tok, max_batch=8)
    exp = _expected()
    case = exp["cases"][0]
    pcm, _ws = utterance(case["seed"])
    truth = [t for t in case["truth_tokens"] if t < exp["timestamp_begin"]]
    clip = pcm[:int(16000 * (0.5 + 0.5 * len(truth) + 0.5))]
    spare = [t for t in exp["word_token_ids"] if t not in truth[:3]]
    yield dict(model=model, pipe=BatchedInferencePipeline(model), clip=clip, truth=truth, x=spare[0], y=spare[1])
    model.close()
    model.engine.close()


def _words(m, segs):
    return [t for t in _tokens(m, segs) if 300 <= t < 310]


def test_three_files_with_their_own_lists_in_one_decode_group(setup):
    m, pipe, clip, truth, x, y = (setup[k] for k in ("model", "pipe", "clip", "truth", "x", "y"))
    lists = [[[truth[0], x]], None, [[truth[0], y]]]
    lb = {truth[0]: -BOOST}                       # (the root's boost of the first word is taken back: only the second word moves)
    many = pipe.transcribe_many([clip, clip, clip], batch_size=3, keywords=lists, keywords_boost=BOOST, logit_bias=[lb, None, lb], **BKW)
    alone = []
    for kws in lists:
        if kws is None:
            alone.append(list(pipe.transcribe(clip, batch_size=3, **BKW)[0]))
        else:
            with m.keyword_bias(phrases=kws, boost=BOOST, logit_bias=lb):
                alone.append(list(pipe.transcribe(clip, batch_size=3, **BKW)[0]))
    for (segs, info), ref in zip(many, alone):
        assert not isinstance(segs, Exception), segs
        assert _tokens(m, segs) == _tokens(m, ref)
        assert [s.avg_logprob for s in segs] == pytest.approx([s.avg_logprob for s in ref], abs=1e-3)
    w = [_words(m, segs) for segs, _ in many]
    assert w[1] == truth and w[0][:2] == [truth[0], x] and w[2][:2] == [truth[0], y]
    # a substitute appears only in its own file (the utterance may have the same word further on: the place it was put is the second word)
    assert w[1][1] not in (x, y) and w[0][1] != y and w[2][1] != x
    # the next job on the same slot, without keywords: unbiased again
    again = pipe.transcribe_many([clip, clip], batch_size=3, **BKW)
    assert [_words(m, segs) for segs, _ in again] == [truth, truth]


def test_a_refused_list_costs_only_its_file(setup):
    m, pipe, clip, truth, x = (setup[k] for k in ("model", "pipe", "clip", "truth", "x"))
    bad = [[m.token_ids.eot + 1]]                 # a special token in a phrase
    many = pipe.transcribe_many([clip, clip], batch_size=3, keywords=[bad, [[truth[0], x]]], keywords_boost=BOOST,
                                logit_bias={truth[0]: -BOOST}, **BKW)
    assert isinstance(many[0][0], ValueError) and many[0][1] is None and "special or timestamp" in str(many[0][0])
    assert _words(m, many[1][0])[:2] == [truth[0], x]
    with pytest.raises(ValueError, match="special or timestamp"):
        pipe.transcribe_many([clip, clip], batch_size=3, on_error="raise", keywords=[bad, None], **BKW)


def test_a_list_the_closed_form_refuses_decodes_compact(setup):
    m, clip, truth, x = (setup[k] for k in ("model", "clip", "truth", "x"))
    filler = [[t] for t in range(10, 290)]        # 280 first tokens: the closed form needs 283 x 281 edges
    lb = {t: -BOOST for t in range(10, 290)}      # ... each boosted in every state: the token list takes exactly that back
    lb[truth[0]] = -BOOST
    kw = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, condition_on_previous_text=False,
              compression_ratio_threshold=None, log_prob_threshold=None, no_speech_threshold=None)
    with pytest.raises(ValueError, match="edges"):
        m.transcribe(clip, **kw, keywords=filler + [[truth[0], x]], keywords_boost=BOOST, logit_bias=lb)
    segs, _ = m.transcribe(clip, **kw, keywords=filler + [[truth[0], x]], keywords_boost=BOOST, logit_bias=lb, keywords_compact=True)
    small, _ = m.transcribe(clip, **kw, keywords=[[truth[0], x]], keywords_boost=BOOST, logit_bias={truth[0]: -BOOST})
    assert _words(m, segs)[:2] == [truth[0], x] and _tokens(m, segs) == _tokens(m, small)
    plain, _ = m.transcribe(clip, **kw)
    assert _words(m, plain) == truth


def _post(port, data, keywords):
    from whisperlive_amd.rest import ROUTE
    b = "kwItems"
    fields = [("language", "en"), ("response_format", "verbose_json"), ("keywords", keywords), ("keywords_boost", str(BOOST))]
    body = b"".join([f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="u.wav"\r\nContent-Type: audio/wav\r\n\r\n'.encode(), data]
                    + [f'\r\n--{b}\r\nContent-Disposition: form-data; name="{k}"\r\n\r\n{v}'.encode() for k, v in fields] + [f"\r\n--{b}--\r\n".encode()])
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
    r = c.getresponse()
    raw = r.read()
    c.close()
    assert r.status == 200, raw
    return raw


def test_two_pooled_uploads_with_different_keywords_equal_the_unpooled_responses(setup, monkeypatch):
    """the same two uploads, each with its own `keywords`, to a server without the batch window (each decoded in its request's thread
    under its closed-form table) and to one with it (ONE iter_many job, each file under its own compact table): the response bodies are
    byte-identical. Both servers' transcribers hold the same number of items, so a row is computed by the same launches."""
    from whisperlive_amd import many_files, vad
    from whisperlive_amd.rest import RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.transcriber import WhisperModelHIP
    m, clip, truth, x, y = (setup[k] for k in ("model", "clip", "truth", "x", "y"))
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    models = []

    def factory(model, device_index, max_batch=1):
        models.append(WhisperModelHIP(DIR, device="cuda", device_index=0, engine=m.engine, hf_tokenizer=m.hf_tokenizer, max_batch=4, vad_model=gate))
        return models[-1]

    jobs = []
    real = many_files.iter_many
    monkeypatch.setattr(many_files, "iter_many", lambda pipe, audios, **kw: (jobs.append((len(audios), kw.get("keywords"))), real(pipe, audios, **kw))[1])
    data = _wav(clip)
    kws = [f"w{truth[0]} w{x}", f"w{truth[0]} w{y}"]
    saved = dict(ServeClientHIP.MODELS)
    answers = {}
    try:
        for window in (0, 300):
            ServeClientHIP.MODELS.clear()
            server = RestServer("127.0.0.1", 0, "trained", model_factory=factory, file_batch_size=2, file_batch_window_ms=window).start()
            try:
                if window == 0:
                    answers[0] = [_post(server.port, data, k) for k in kws]
                    assert jobs == []
                else:
                    got = [None, None]
                    ts = [threading.Thread(target=lambda i=i: got.__setitem__(i, _post(server.port, data, kws[i]))) for i in range(2)]
                    [t.start() for t in ts]
                    [t.join(120) for t in ts]
                    answers[300] = got
                    assert [j[0] for j in jobs] == [2] and sorted(map(repr, jobs[0][1])) == sorted(repr([k]) for k in kws), jobs
            finally:
                server.shutdown()
        for i, (alone, pooled) in enumerate(zip(answers[0], answers[300])):
            print("upload", i, "alone", alone[:400], "pooled", None if pooled is None else pooled[:400])
            assert pooled == alone, i
        texts = [json.loads(a)["text"] for a in answers[300]]
        # (the form fields carry no logit_bias, so the root's boost of the phrase's first word is not taken back, as in
        # tests/test_gpu_keyword_bias.py: that word floods the text and the substitute follows it somewhere — in its own upload's text)
        assert f"w{x}" in texts[0].split() and f"w{y}" in texts[1].split() and texts[0] != texts[1]
    finally:
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        for mm in models:
            mm.close()
        gate.close()


def test_two_live_sessions_with_different_keywords_share_a_worker_batch(setup):
    """two sessions whose first messages carried different `keywords`: through the batch worker both chunks are ONE batch
    (_process_multi, an item_scope of the two sessions' tables), and each session's text is what it gets on its own slot in its own
    thread (no worker: the single-table route under its table)"""
    from whisperlive_amd.batching import BatchInferenceWorker
    from whisperlive_amd.serve_client import ServeClientHIP
    m, clip, truth, x, y = (setup[k] for k in ("model", "clip", "truth", "x", "y"))
    kws = [[f"w{truth[0]} w{x}"], [f"w{truth[0]} w{y}"]]
    saved = ServeClientHIP.BATCH_WORKER, dict(ServeClientHIP.BATCH_WORKERS)
    ServeClientHIP.BATCH_WORKERS.clear()
    worker = BatchInferenceWorker(m, max_batch_size=4, batch_window_ms=400, wait_when_idle=True)
    batches, real = [], worker._process_multi
    worker._process_multi = lambda batch: (batches.append([r.bias_table for r in batch]), real(batch))[1]
    worker.start()
    try:
        cs = [ServeClientHIP(MagicMock(), client_uid=f"kw{i}", model="small.en", transcriber=m, start_thread=False, use_vad=False,
                             keywords=kws[i], keywords_boost=BOOST) for i in range(2)]
        assert all(c._bias is not None and c._bias.table.phrases == [(truth[0], w)] for c, w in zip(cs, (x, y)))
        # A first message carries no logit_bias, so the phrase's first word, boosted in every state, would flood the text and push both
        # routes into their sampling fallbacks (random, and seeded differently). The sessions' tables are therefore replaced by the same
        # phrases WITH the token-list entry that takes the root's boost back, as the transcribe_many case above does: greedy-free decodes
        # at temperature 0 that the two routes can be compared on.
        for c, w in zip(cs, (x, y)):
            c._bias = m.keyword_bias(phrases=[[truth[0], w]], boost=BOOST, logit_bias={truth[0]: -BOOST})
        ServeClientHIP.BATCH_WORKER = worker
        outs = [None, None]
        ts = [threading.Thread(target=lambda i=i: outs.__setitem__(i, cs[i].transcribe_audio(clip))) for i in range(2)]
        [t.start() for t in ts]
        [t.join(60) for t in ts]
        assert len(batches) == 1 and len(batches[0]) == 2 and all(t is not None for t in batches[0]), batches
        ServeClientHIP.BATCH_WORKER = None
        direct = [c.transcribe_audio(clip) for c in cs]
        words = lambda res: " ".join(s.text.strip() for s in res).split()
        print("worker", [words(o) for o in outs], "direct", [words(d) for d in direct])
        for o, d in zip(outs, direct):
            assert o and words(o) == words(d)
        assert words(outs[0])[:2] == [f"w{truth[0]}", f"w{x}"] and words(outs[1])[:2] == [f"w{truth[0]}", f"w{y}"]
        assert all(s.temperature == 0.0 for o in outs + direct for s in o)
    finally:
        ServeClientHIP.BATCH_WORKER = saved[0]
        ServeClientHIP.BATCH_WORKERS.update(saved[1])
        worker.stop()
