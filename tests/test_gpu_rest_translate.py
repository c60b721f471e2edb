"""GPU: one upload of the short fixture through a running RestServer with a real tiny.en engine (peaked weights) and the seeded
fixture-size translation model saved as a checkpoint directory: verbose_json carries per segment the translation
HipTranslator.translate gives for that segment's text, srt carries the same strings, and a request without target_language is
answered as by a server without a translation model."""
import http.client
import json
import os
import shutil

import numpy as np
import pytest

from tests import helpers as H
from whisperlive_amd.mt_weights import MTSpec, random_mt_weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
JFK = os.path.join(HERE, "golden", "jfk_head.flac")
GOLD = json.load(open(os.path.join(HERE, "golden", "mt_golden.json")))
FIX = MTSpec(**GOLD["spec"])


def _post(port, fields, data):
    from whisperlive_amd.rest import ROUTE
    b = "gpuRESTtranslate"
    body = f'--{b}\r\nContent-Disposition: form-data; name="file"; filename="jfk_head.flac"\r\nContent-Type: audio/flac\r\n\r\n'.encode() + data
    for k, v in fields.items():
        body += f'\r\n--{b}\r\nContent-Disposition: form-data; name="{k}"\r\n\r\n{v}'.encode()
    body += f"\r\n--{b}--\r\n".encode()
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={b}"})
    r = c.getresponse()
    out = r.status, r.read()
    c.close()
    return out


def test_upload_with_target_language(gpu, tmp_path):
    from safetensors.numpy import save_file

    from whisperlive_amd import translation as tr
    from whisperlive_amd.rest import RestServer
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    d = tmp_path / "small100-seeded"
    d.mkdir()
    json.dump(FIX.hf_config(), open(d / "config.json", "w"))
    json.dump({"num_beams": 5, "max_length": 40, "early_stopping": True}, open(d / "generation_config.json", "w"))
    w = random_mt_weights(FIX, seed=GOLD["seed"], peaked=GOLD["peaked"])
    save_file({k: np.ascontiguousarray(v) for k, v in w.items()}, str(d / "model.safetensors"))
    for f in ("vocab.json", "sentencepiece.bpe.model", "tokenizer_config.json"):
        shutil.copy(os.path.join(HERE, "golden", "mt_tok", f), d / f)

    spec = H.TINY_EN
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab))
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server = RestServer("127.0.0.1", 0, "peaked", model_factory=lambda model, device_index: hip, translation_model=str(d)).start()
    plain_server = RestServer("127.0.0.1", 0, "peaked", model_factory=lambda model, device_index: hip).start()
    try:
        with open(JFK, "rb") as f:
            data = f.read()
        st, body = _post(server.port, {"response_format": "verbose_json", "target_language": "de"}, data)
        got = json.loads(body)
        assert st == 200, got
        ref = tr.shared_translator(str(d), 0)
        assert isinstance(ref.engine, tr.HipMTEngine)
        assert got["target_language"] == "de" and got["segments"]
        for seg in got["segments"]:
            assert seg["translation"] == ref.translate([seg["text"]], "de")[0].strip(), seg
        assert any(seg["translation"] for seg in got["segments"])
        assert got["translation"] == " ".join(seg["translation"] for seg in got["segments"])
        st, srt = _post(server.port, {"response_format": "srt", "target_language": "de"}, data)
        from whisperlive_amd.rest import _stamp
        want = "\n".join(f"{i}\n{_stamp(seg['start']).replace('.', ',')} --> {_stamp(seg['end']).replace('.', ',')}\n{seg['translation']}\n"
                         for i, seg in enumerate(got["segments"], 1))
        assert st == 200 and srt.decode() == want
        # without the field: the bytes of a server that has no translation model
        for fmt in ("verbose_json", "json", "srt"):
            a = _post(server.port, {"response_format": fmt}, data)
            b = _post(plain_server.port, {"response_format": fmt}, data)
            assert a == b and a[0] == 200, fmt
        plain = json.loads(_post(server.port, {"response_format": "verbose_json"}, data)[1])
        assert "translation" not in plain and "target_language" not in plain
        assert [{k: v for k, v in seg.items() if k != "translation"} for seg in got["segments"]] == plain["segments"]
        st, body = _post(server.port, {"target_language": "xx"}, data)
        assert st == 400 and "xx" in json.loads(body)["error"]
    finally:
        server.shutdown()
        plain_server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
        shared = tr._shared.pop((str(d), 0), None)
        if shared is not None:
            shared.close()
        hip.close()
        hip.engine.close()
