"""GPU: POST /v1/audio/transcriptions with multichannel=true answers the pipeline's multichannel segments, each with its channel;
without the field the answer is what the multichannel=False pipeline gives, as before."""
import http.client
import json

import numpy as np
import pytest

from oracle import logmel as olm
from tests import batched_common as BC
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _post(port, data: bytes, extra=()) -> dict:
    from whisperlive_amd.rest import ROUTE
    b = "gpuRESTmultichannel"
    fields = [("language", "en"), ("response_format", "verbose_json")] + list(extra)
    body = f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="a.wav"\r\nContent-Type: audio/wav\r\n\r\n'.encode() + data
    for k, v in fields:
        body += f'\r\n--{b}\r\nContent-Disposition: form-data; name="{k}"\r\n\r\n{v}'.encode()
    body += f"\r\n--{b}--\r\n".encode()
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
    r = c.getresponse()
    got = json.loads(r.read())
    c.close()
    assert r.status == 200, got
    return got


def test_rest_multichannel_field(gpu):
    from whisperlive_amd import vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.rest import RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)

    def factory(model, device_index, max_batch=1):
        return WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab),
                               max_batch=max_batch, vad_model=gate)

    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "peaked", model_factory=factory, file_batch_size=4).start()
    hip = None
    try:
        a = BC.audio16()[: 8 * BC.SR]
        b = olm.speech_like_pcm(8.0, seed=4321).astype(np.float32)
        wav = BC.wav_bytes(np.stack([a, b], axis=1), BC.SR)
        kw = dict(language="en", temperature=0.0, vad_filter=True)
        got = _post(server.port, wav, [("multichannel", "true")])
        hip = ServeClientHIP.MODELS[0]
        segs, info = BatchedInferencePipeline(hip).transcribe(wav, batch_size=2, multichannel=True, **kw)   # min(4, max_batch 4 - 2 channels)
        segs = list(segs)
        assert segs and {s.channel for s in segs} == {0, 1} and got["duration"] == info.duration
        assert [(g["id"], g["channel"], g["seek"], g["start"], g["end"], g["tokens"]) for g in got["segments"]] == \
            [(s.id, s.channel, s.seek, s.start, s.end, s.tokens) for s in segs]
        assert got["text"] == "\n".join(s.text.strip() for s in segs)
        plain = _post(server.port, wav)                                  # without the field: the down-mix route, unchanged
        segs, info = BatchedInferencePipeline(hip).transcribe(wav, batch_size=4, multichannel=False, **kw)
        segs = list(segs)
        assert segs and plain["text"] == " ".join(s.text.strip() for s in segs) and plain["duration"] == info.duration
        assert all("channel" not in g for g in plain["segments"])
        assert [(g["id"], g["seek"], g["start"], g["end"], g["tokens"]) for g in plain["segments"]] == \
            [(s.id, s.seek, s.start, s.end, s.tokens) for s in segs]
    finally:
        server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        if hip is not None:
            hip.close()
            hip.engine.close()
        gate.close()
