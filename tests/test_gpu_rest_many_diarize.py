"""GPU: the file endpoint with a file batch window pools three concurrent `diarize=true` uploads into ONE iter_many job — whose wave is
diarized by one wlx_spk_diarize_many call while its files are still resident — and answers each request the speakers the same upload
gets when it is sent alone to a server without the window (the per-file route: wlx_spk_diarize_pcm on what the transcription left in
the slot). A small seeded speaker engine stands in for the checkpoint (embedder_factory)."""
import http.client
import json
import threading

import pytest

from tests import batched_common as BC
from tests import helpers as H
from tests import test_gpu_many_files as MANY

pytestmark = pytest.mark.gpu


def _post(port, data: bytes, cap: int) -> dict:
    from whisperlive_amd.rest import ROUTE
    b = "gpuRESTmanyDiarize"
    body = f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="a.wav"\r\nContent-Type: audio/wav\r\n\r\n'.encode() + data
    for k, v in (("language", "en"), ("response_format", "verbose_json"), ("diarize", "true"), ("max_speakers", str(cap))):
        body += f'\r\n--{b}\r\nContent-Disposition: form-data; name="{k}"\r\n\r\n{v}'.encode()
    body += f"\r\n--{b}--\r\n".encode()
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
    r = c.getresponse()
    got = json.loads(r.read())
    c.close()
    assert r.status == 200, got
    return got


def test_three_pooled_diarize_uploads_get_the_speakers_of_the_unpooled_route(gpu):
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
    weights = H.peaked_weights(spec, 5)
    models, waves = [], []

    def factory(model, device_index, max_batch=1):
        models.append(WhisperModelHIP("peaked", weights=weights, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab),
                                      max_batch=max_batch, vad_model=gate))
        models[-1].max_length = 2 + BC.MAX_NEW          # (tests/test_gpu_rest_many.py says why)
        return models[-1]

    real = embedder.diarize_many
    embedder.diarize_many = lambda *a, **k: (waves.append((list(a[1]), list(a[4]))), real(*a, **k))[1]
    f = MANY._files()
    qc, _ = MANY._quantized(f["C"])
    uploads, caps = [f["A"], f["B"], MANY._wav16(qc)], [2, 0, 3]
    saved = dict(ServeClientHIP.MODELS)
    try:
        answers = {}
        for window in (0, 200):                         # the same uploads: alone on a server without the window, then pooled
            ServeClientHIP.MODELS.clear()
            server = RestServer("127.0.0.1", 0, "peaked", model_factory=factory, file_batch_size=4, file_batch_window_ms=window,
                                embedder_factory=lambda path, device_index: embedder).start()
            try:
                if window == 0:
                    answers[0] = [_post(server.port, data, cap) for data, cap in zip(uploads, caps)]
                    assert server.batcher is None and waves == []
                else:
                    got = [None] * 3
                    threads = [threading.Thread(target=lambda i=i: got.__setitem__(i, _post(server.port, uploads[i], caps[i]))) for i in range(3)]
                    for t in threads:
                        t.start()
                    for t in threads:
                        t.join(120)
                    answers[200] = got
                    assert server.batcher.jobs == 1 and len(waves) == 1                      # ONE job, ONE diarize_many call for its wave
                    assert sorted(waves[0][0]) == [4, 5, 6] and sorted(waves[0][1]) == sorted(caps)
            finally:
                server.shutdown()
        for alone, pooled, cap in zip(answers[0], answers[200], caps):
            assert pooled is not None and alone["segments"] and alone["speakers"] and (cap == 0 or len(alone["speakers"]) <= cap)
            print("speakers", alone["speakers"], [g["speaker"] for g in alone["segments"]])
            assert pooled["speakers"] == alone["speakers"] and pooled["text"] == alone["text"]
            assert [(g["id"], g["start"], g["end"], g["speaker"]) for g in pooled["segments"]] == \
                   [(g["id"], g["start"], g["end"], g["speaker"]) for g in alone["segments"]]
    finally:
        del embedder.diarize_many
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        for m in models:
            m.close()
            m.engine.close()
        embedder.close()
        gate.close()
