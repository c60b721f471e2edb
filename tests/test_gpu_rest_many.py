"""GPU: the file endpoint started with a file batch window pools three concurrent uploads (A: 16-bit WAV, B: FLAC, C: a short WAV) into ONE
iter_many job, and answers each request what the same upload gets when it is sent alone to a server without the window."""
import http.client
import json
import threading

import pytest

from tests import batched_common as BC
from tests import helpers as H
from tests import test_gpu_many_files as MANY

pytestmark = pytest.mark.gpu


def _post(port, data: bytes) -> dict:
    from whisperlive_amd.rest import ROUTE
    b = "gpuRESTmany"
    body = b"".join([
        f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="a.wav"\r\nContent-Type: audio/wav\r\n\r\n'.encode(), data,
        f'\r\n--{b}\r\nContent-Disposition: form-data; name="language"\r\n\r\nen'.encode(),
        f'\r\n--{b}\r\nContent-Disposition: form-data; name="response_format"\r\n\r\nverbose_json\r\n--{b}--\r\n'.encode()])
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
    r = c.getresponse()
    got = json.loads(r.read())
    c.close()
    assert r.status == 200, got
    return got


def test_three_concurrent_uploads_are_one_job_and_each_gets_its_own_answer(gpu, monkeypatch):
    from whisperlive_amd import many_files, vad
    from whisperlive_amd.rest import RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    weights = H.peaked_weights(spec, 5)
    made, models = [], []

    def factory(model, device_index, max_batch=1):
        made.append(max_batch)
        models.append(WhisperModelHIP("peaked", weights=weights, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab),
                                      max_batch=max_batch, vad_model=gate))
        # both servers' model ends a decode after MAX_NEW tokens behind the two prompt tokens, the length the peaked weights are searched
        # for (batched_common): the endpoint has no max_new_tokens field, and a 448-token decode of seeded weights runs into near ties,
        # where two transcribers of different max_batch (4 alone, 8 pooled) may part by a rounding
        models[-1].max_length = 2 + BC.MAX_NEW
        return models[-1]

    jobs = []
    real = many_files.iter_many
    monkeypatch.setattr(many_files, "iter_many", lambda pipe, audios, **kw: (jobs.append(len(audios)), real(pipe, audios, **kw))[1])

    f = MANY._files()
    qc, _ = MANY._quantized(f["C"])
    uploads = [f["A"], f["B"], MANY._wav16(qc)]
    saved = dict(ServeClientHIP.MODELS)
    try:
        answers = {}
        for window in (0, 200):                       # the same uploads: alone on a server without the window, then pooled
            ServeClientHIP.MODELS.clear()
            server = RestServer("127.0.0.1", 0, "peaked", model_factory=factory, file_batch_size=4, file_batch_window_ms=window).start()
            try:
                if window == 0:
                    answers[0] = [_post(server.port, data) for data in uploads]
                    assert server.batcher is None and jobs == []
                else:
                    got = [None] * 3
                    threads = [threading.Thread(target=lambda i=i: got.__setitem__(i, _post(server.port, uploads[i]))) for i in range(3)]
                    for t in threads:
                        t.start()
                    for t in threads:
                        t.join(120)
                    answers[200] = got
                    assert jobs == [3] and server.batcher.jobs == 1                       # ONE job of three files, not three pipeline runs
            finally:
                server.shutdown()
        assert made == [4, 8]                          # N chunks per step; with the window, a wave of N files behind them
        for alone, pooled in zip(answers[0], answers[200]):
            assert pooled is not None and alone["segments"]
            print("segments", len(alone["segments"]), len(pooled["segments"]),
                  [(a["start"], a["end"], a["tokens"] == p["tokens"]) for a, p in zip(alone["segments"], pooled["segments"])])
            assert (pooled["text"], pooled["duration"], pooled["language"]) == (alone["text"], alone["duration"], alone["language"])
            key = ("id", "seek", "start", "end", "text", "tokens", "temperature", "compression_ratio")
            assert [[s[k] for k in key] for s in pooled["segments"]] == [[s[k] for k in key] for s in alone["segments"]]
            for p, a in zip(pooled["segments"], alone["segments"]):
                assert abs(p["avg_logprob"] - a["avg_logprob"]) <= 2e-3 * abs(a["avg_logprob"]) + 1e-3      # the decode suites' score bound
                # ... and their bound on no_speech_prob of one prompt in two batch shapes (tests/test_gpu_lean_family.py)
                assert abs(p["no_speech_prob"] - a["no_speech_prob"]) <= 1e-5 + 2e-2 * a["no_speech_prob"]
        assert [a["duration"] for a in answers[0]] == [16.0, 16.0, 8.2]
    finally:
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        for m in models:
            m.close()
            m.engine.close()
        gate.close()
