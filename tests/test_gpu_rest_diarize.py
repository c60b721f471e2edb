"""GPU: POST /v1/audio/transcriptions with diarize=true — the transcription as without the field, then offline diarization
(file_diarization.FileDiarizer on wlx_spk_diarize_pcm) of the audio it left in the slot: a speaker on every segment and word, the list
of speakers in the answer; a multichannel upload gets one diarization per channel. A small seeded speaker engine stands in for the
checkpoint (embedder_factory)."""
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
    b = "gpuRESTdiarize"
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


def test_rest_diarize_field(gpu):
    from whisperlive_amd import spk_weights, vad
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    from whisperlive_amd.rest import RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    sspec = spk_weights.SpkSpec(n_mels=16, planes=32, blocks=(1, 1, 1, 1), embed_dim=32, max_seconds=6)
    embedder = SpeakerEmbedderHIP(sspec, spk_weights.fold(spk_weights.random_weights(sspec, seed=11), sspec), device=0)

    def factory(model, device_index, max_batch=1):
        return WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab),
                               max_batch=max_batch, vad_model=gate)

    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "peaked", model_factory=factory, file_batch_size=4,
                        embedder_factory=lambda path, device_index: embedder).start()
    try:
        a = BC.audio16()[: 8 * BC.SR]
        b = olm.speech_like_pcm(8.0, seed=4321).astype(np.float32)
        mono = BC.wav_bytes(a[:, None], BC.SR)
        words = [("timestamp_granularities", "word")]
        plain = _post(server.port, mono, words)
        got = _post(server.port, mono, words + [("diarize", "true"), ("max_speakers", "2")])
        assert plain["segments"] and "speakers" not in plain and all("speaker" not in g for g in plain["segments"])
        assert got["text"] == plain["text"] and 1 <= len(got["speakers"]) <= 2
        assert all(s.startswith("SPEAKER_") for s in got["speakers"])
        for g, p in zip(got["segments"], plain["segments"]):
            assert g["speaker"] in got["speakers"] and g["words"] and all(w["speaker"] in got["speakers"] for w in g["words"])
            assert (g["id"], g["start"], g["end"], g["tokens"]) == (p["id"], p["start"], p["end"], p["tokens"])
            assert [(w["word"], w["start"], w["end"]) for w in g["words"]] == [(w["word"], w["start"], w["end"]) for w in p["words"]]
        assert len(got["segments"]) == len(plain["segments"])
        # two channels: one diarization each, the speakers carry their channel
        stereo = BC.wav_bytes(np.stack([a, b], axis=1), BC.SR)
        plain = _post(server.port, stereo, [("multichannel", "true")])
        got = _post(server.port, stereo, [("multichannel", "true"), ("diarize", "true")])
        assert got["text"] == plain["text"] and {g["channel"] for g in got["segments"]} == {0, 1}
        assert got["speakers"] and all(s.startswith(("CH0_SPEAKER_", "CH1_SPEAKER_")) for s in got["speakers"])
        for g in got["segments"]:
            assert g["speaker"] in got["speakers"] and g["speaker"].startswith(f"CH{g['channel']}_")
    finally:
        server.shutdown()
        hip = ServeClientHIP.MODELS.get(0)
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        if hip is not None:
            hip.close()
            hip.engine.close()
        embedder.close()
        gate.close()
