"""GPU: a real tiny.en engine (peaked weights) behind RestServer — the endpoint's verbose_json answer for a FLAC upload equals a
direct transcribe(path, word_timestamps=True) on the same transcriber."""
import http.client
import json
import os

import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

JFK = os.path.join(os.path.dirname(__file__), "golden", "jfk_head.flac")


def test_verbose_json_with_words_equals_direct_transcribe(gpu):
    from whisperlive_amd.rest import ROUTE, RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab))
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "peaked", model_factory=lambda model, device_index: hip).start()
    try:
        with open(JFK, "rb") as f:
            data = f.read()
        b = "gpuRESTboundary"
        body = b"".join([
            f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="jfk_head.flac"\r\nContent-Type: audio/flac\r\n\r\n'.encode(),
            data, f'\r\n--{b}\r\nContent-Disposition: form-data; name="response_format"\r\n\r\nverbose_json'.encode(),
            f'\r\n--{b}\r\nContent-Disposition: form-data; name="timestamp_granularities"\r\n\r\nword\r\n--{b}--\r\n'.encode()])
        c = http.client.HTTPConnection("127.0.0.1", server.port, timeout=120)
        c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
        r = c.getresponse()
        got = json.loads(r.read())
        c.close()
        assert r.status == 200, got
        segs, info = hip.transcribe(JFK, temperature=0.0, vad_filter=False, word_timestamps=True)
        segs = list(segs)
        assert segs and got["task"] == "transcribe" and got["language"] == info.language and got["duration"] == info.duration
        assert got["text"] == " ".join(s.text.strip() for s in segs)
        assert len(got["segments"]) == len(segs)
        for g, s in zip(got["segments"], segs):
            assert (g["id"], g["seek"], g["start"], g["end"], g["text"], g["tokens"]) == (s.id, s.seek, s.start, s.end, s.text.strip(), s.tokens)
            assert (g["temperature"], g["avg_logprob"], g["compression_ratio"], g["no_speech_prob"]) == \
                (s.temperature, s.avg_logprob, s.compression_ratio, s.no_speech_prob)
            assert g["words"] == [{"word": w.word, "start": w.start, "end": w.end, "probability": w.probability} for w in s.words]
    finally:
        server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        hip.close()
        hip.engine.close()
