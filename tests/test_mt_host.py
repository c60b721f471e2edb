"""CPU tests of the translation feature: the torch restatement (tests/mt_oracle.py) against transformers' recording, the
sentencepiece tokenizer against M2M100Tokenizer's recording, generation-option resolution, checkpoint loading, the C-ABI
symbols, ServeClientTranslation with a fake translator and the server wiring of `enable_translation`."""
from __future__ import annotations

import ctypes
import json
import os
import queue
import threading

import numpy as np
import pytest
import torch

from whisperlive_amd.mt_weights import MTGenOptions, MTSpec, generation_options, layer_names, load_mt_dir, random_mt_weights

from .mt_oracle import M2M100Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "mt_golden.json")))
ARR = np.load(os.path.join(HERE, "golden", "mt_golden.npz"))
TOK = os.path.join(HERE, "golden", "mt_tok")
FIX = MTSpec(**GOLD["spec"])


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))


@pytest.fixture(scope="module")
def orc():
    return M2M100Oracle(FIX, random_mt_weights(FIX, seed=GOLD["seed"], peaked=GOLD["peaked"]))


def test_oracle_encoder_and_logits_match_transformers(orc):
    for i in (0, 4):
        e = orc.encode(GOLD["sources"][i]).numpy()
        ref = ARR[f"enc_{i}"]
        assert rel_rms(e[:len(ref)], ref) <= 1e-5
    src = GOLD["sources"][GOLD["tf_source"]]
    lg = orc.decode_logits(orc.encode(src), GOLD["tf_decoder"]).numpy()
    assert rel_rms(lg[GOLD["tf_rows"]], ARR["tf_logits"]) <= 1e-5


@pytest.mark.parametrize("case", [c["name"] for c in GOLD["cases"]])
def test_oracle_generate_matches_transformers(orc, case):
    c = next(x for x in GOLD["cases"] if x["name"] == case)
    o = MTGenOptions(num_beams=c["num_beams"], max_length=c["max_length"], early_stopping=c["early_stopping"],
                     length_penalty=c["length_penalty"], no_repeat_ngram_size=c.get("no_repeat_ngram_size", 0),
                     forced_eos_token_id=c.get("forced_eos_token_id"))
    toks, scores = orc.generate(GOLD["sources"], o)
    for i, r in enumerate(c["results"]):
        s = r["sequence"][1:]
        if FIX.eos_id in s:
            s = s[:s.index(FIX.eos_id)]
        assert toks[i] == s, (case, i)
        if r["score"] is not None:
            assert abs(scores[i] - r["score"]) <= 1e-4, (case, i)


def test_golden_exercises_every_search_rule():
    names = {c["name"]: c for c in GOLD["cases"]}
    assert {1, 5} <= {c["num_beams"] for c in GOLD["cases"]}
    assert {True, False, "never"} <= {c["early_stopping"] for c in GOLD["cases"]}
    assert any(c["length_penalty"] != 1.0 for c in GOLD["cases"])
    assert all(len(r["sequence"]) == 6 for r in names["beam4_maxlen"]["results"])           # runs to max_length
    assert os.path.getsize(os.path.join(HERE, "golden", "mt_golden.npz")) + os.path.getsize(os.path.join(HERE, "golden", "mt_golden.json")) < 100_000


def test_tokenizer_matches_m2m100_tokenizer_recording():
    from whisperlive_amd.mt_tokenizer import M2M100SPTokenizer
    g = json.load(open(os.path.join(TOK, "tok_golden.json"), encoding="utf-8"))
    tok = M2M100SPTokenizer(TOK)
    for c in g["encode"]:
        assert tok.encode_source(c["text"], c["tgt_lang"]) == c["ids"], c["text"]
    for c in g["decode"]:
        assert tok.decode(c["ids"]) == c["text"], c["ids"]


def test_language_codes_from_checkpoint_files(tmp_path):
    from whisperlive_amd.mt_tokenizer import M2M100SPTokenizer, fairseq_language_codes
    fairseq = fairseq_language_codes(None)
    assert fairseq[:3] == ["af", "am", "ar"] and len(fairseq) == 100
    for f in ("vocab.json", "sentencepiece.bpe.model"):
        (tmp_path / f).write_bytes(open(os.path.join(TOK, f), "rb").read())
    n = len(json.load(open(tmp_path / "vocab.json")))
    # a complete list in the checkpoint's own order is taken as it stands
    mine = fairseq[::-1]
    json.dump({"additional_special_tokens": [f"__{c}__" for c in mine]}, open(tmp_path / "tokenizer_config.json", "w"))
    tok = M2M100SPTokenizer(str(tmp_path))
    assert tok.lang_id("zu") == n and tok.lang_id("af") == n + 99
    assert tok.encode_source("Hello", "fr")[0] == n + mine.index("fr") and tok.encode_source("Hello", "fr")[-1] == 2
    # a partial (or repeating) list would shift the ids after a gap: ignored, the fairseq order holds
    for partial in (["__zz__", "__fr__", "__en__"], [f"__{c}__" for c in fairseq[:99]] + ["__af__"]):
        json.dump({"additional_special_tokens": partial}, open(tmp_path / "tokenizer_config.json", "w"))
        tok = M2M100SPTokenizer(str(tmp_path))
        assert tok.lang_id("fr") == n + fairseq.index("fr") and "zz" not in tok.lang_code_to_id


def test_fixture_tokenizer_needs_no_transformers(monkeypatch):
    """the fixture checkpoint carries the full code list, so the tokenizer (as the GPU tests and the server use it) never
    imports transformers"""
    import sys
    from whisperlive_amd.mt_tokenizer import M2M100SPTokenizer
    monkeypatch.setitem(sys.modules, "transformers", None)
    tok = M2M100SPTokenizer(TOK)
    g = json.load(open(os.path.join(TOK, "tok_golden.json"), encoding="utf-8"))
    assert all(tok.encode_source(c["text"], c["tgt_lang"]) == c["ids"] for c in g["encode"])


def test_generation_option_resolution(tmp_path):
    assert generation_options(config={}) == MTGenOptions(1, 20, False, 1.0, 0, None)
    # config.json only: transformers takes its generation keys
    cfg = {"num_beams": 5, "max_length": 200, "early_stopping": True, "d_model": 1024}
    o = generation_options(config=cfg)
    assert (o.num_beams, o.max_length, o.early_stopping) == (5, 200, True)
    # generation_config.json present: it wins, and config.json's generation keys are not consulted
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    json.dump({"num_beams": 4, "length_penalty": 0.8, "forced_eos_token_id": 2}, open(tmp_path / "generation_config.json", "w"))
    o = generation_options(str(tmp_path))
    assert o == MTGenOptions(4, 20, False, 0.8, 0, 2)
    assert generation_options(config={"early_stopping": "never"}).early_stopping_code() == 2
    with pytest.raises(ValueError, match="448"):
        generation_options(config={"max_length": 449})


def test_spec_and_weights_from_save_pretrained_dir(tmp_path):
    transformers = pytest.importorskip("transformers")
    spec = MTSpec(d_model=128, n_heads=2, enc_layers=1, dec_layers=1, ffn=256, vocab=160)
    w = random_mt_weights(spec, seed=1)
    model = transformers.M2M100ForConditionalGeneration(transformers.M2M100Config(**spec.hf_config()))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    for safe, fn in ((True, "model.safetensors"), (False, "pytorch_model.bin")):
        d = tmp_path / fn
        model.save_pretrained(str(d), safe_serialization=safe) if safe else None
        if not safe:
            d.mkdir()
            json.dump(spec.hf_config(), open(d / "config.json", "w"))
            torch.save({k: torch.from_numpy(v) for k, v in w.items() if k != "model.shared.weight"} |
                       {"model.encoder.embed_tokens.weight": torch.from_numpy(w["model.shared.weight"])}, d / fn)
        got_spec, got = load_mt_dir(str(d))
        assert got_spec == spec
        assert set(got) == set(layer_names(spec))
        for k in got:
            np.testing.assert_array_equal(got[k], w[k])


def test_random_weights_are_reproducible():
    a = random_mt_weights(FIX, seed=4, peaked=True)
    b = random_mt_weights(FIX, seed=4, peaked=True)
    assert set(a) == set(layer_names(FIX)) and all(np.array_equal(a[k], b[k]) for k in a)


def test_abi_declares_translation_entry_points():
    from whisperlive_amd import _lib
    path = _lib.build()
    lib = ctypes.CDLL(str(path))
    for s in ("wlx_mt_create", "wlx_mt_destroy", "wlx_mt_slot_create", "wlx_mt_slot_destroy", "wlx_mt_translate",
              "wlx_mt_debug_encode", "wlx_mt_debug_decode_logits", "wlx_mt_debug_timings"):
        assert hasattr(lib, s) and s in _lib.EXPORTS
    assert {"mt.hip", "mt_engine.hip"} <= set(_lib.SOURCES)
    assert ctypes.sizeof(_lib.wlx_mt_spec) == 11 * 4 and ctypes.sizeof(_lib.wlx_mt_gen_opts) == 6 * 4


def test_engine_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from whisperlive_amd._lib import WlxError
    from whisperlive_amd.translation import HipMTEngine
    with pytest.raises(WlxError):
        HipMTEngine(FIX, random_mt_weights(FIX, seed=0))


# ---------------------------------------------------------------- ServeClientTranslation
class FakeWS:
    def __init__(self, fail=False):
        self.sent, self.fail = [], fail

    def send(self, m):
        if self.fail:
            raise ConnectionError("closed")
        self.sent.append(json.loads(m))


def run_client(segs, translator, n=2, **kw):
    from whisperlive_amd.translation import ServeClientTranslation
    q, ws = queue.Queue(), FakeWS()
    c = ServeClientTranslation("u1", ws, q, target_language="es", send_last_n_segments=n, translator=translator, **kw)
    th = threading.Thread(target=c.speech_to_text, daemon=True)
    th.start()
    for s in segs:
        q.put(s)
    q.join()
    c.cleanup()
    th.join(5)
    assert not th.is_alive()
    return c, ws


def seg(i, done=True, text=None):
    return {"start": f"{i:.3f}", "end": f"{i + 1:.3f}", "text": text or f"text {i}", "completed": done}


def test_translation_client_message_shape_last_n_and_skip():
    calls = []

    def fake(texts, lang):
        calls.append((list(texts), lang))
        return [t.upper() for t in texts]
    c, ws = run_client([seg(0), seg(1, done=False), seg(2), seg(3)], fake, n=2)
    assert [x[0] for x in calls] == [["text 0"], ["text 2"], ["text 3"]] and all(x[1] == "es" for x in calls)
    assert len(ws.sent) == 3 and all(set(m) == {"uid", "translated_segments"} and m["uid"] == "u1" for m in ws.sent)
    last = ws.sent[-1]["translated_segments"]
    assert [s["text"] for s in last] == ["TEXT 2", "TEXT 3"]
    assert last[0] == {"start": "2.000", "end": "3.000", "text": "TEXT 2", "completed": True, "target_language": "es"}
    assert [s["text"] for s in ws.sent[0]["translated_segments"]] == ["TEXT 0"]


def test_translation_client_falls_back_to_original_text_on_error():
    def boom(texts, lang):
        raise RuntimeError("engine down")
    _, ws = run_client([seg(0, text="keep me")], boom)
    assert ws.sent[-1]["translated_segments"][0]["text"] == "keep me"


def test_translation_client_target_language_and_cleanup():
    from whisperlive_amd.translation import ServeClientTranslation
    q = queue.Queue()
    c = ServeClientTranslation("u", FakeWS(), q, translator=lambda t, l: [l + ":" + x for x in t])
    c.set_target_language("ja")
    assert c.translate_text("hi") == "ja:hi" and c.translate_text("  ") == "  "
    th = threading.Thread(target=c.speech_to_text, daemon=True)
    th.start()
    c.cleanup()
    th.join(5)
    assert not th.is_alive() and c.exit


# ---------------------------------------------------------------- server wiring
class _WS:
    def __init__(self):
        self.sent = []

    def send(self, m):
        self.sent.append(json.loads(m))

    def close(self):
        pass


class _Tx:
    pass


def _server(monkeypatch, resolved):
    from whisperlive_amd import artifacts
    from whisperlive_amd import server as srv
    monkeypatch.setattr(artifacts, "resolve_translation_model", lambda name=None, **k: resolved)
    s = srv.TranscriptionServer()
    s.client_manager = srv.ClientManager()
    s.model_factory = lambda model, dev: _Tx()
    return s


def test_server_wires_translation_when_a_model_resolves(monkeypatch, tmp_path):
    from whisperlive_amd import server as srv
    from whisperlive_amd import translation as tr
    s = _server(monkeypatch, str(tmp_path))
    monkeypatch.setattr(tr, "shared_translator", lambda d, dev: (lambda texts, lang: [f"[{lang}] {t}" for t in texts]))
    ws = _WS()
    s.initialize_client(ws, {"uid": "a", "language": "en", "task": "transcribe", "model": "mt-host-test",
                             "enable_translation": True, "target_language": "it"}, None, None, False)
    c = s.client_manager.get_client(ws)
    try:
        assert c.translation_queue is not None and c.translation_thread.daemon and c.translation_thread.is_alive()
        assert c.translation_client.model_name == str(tmp_path) and c.translation_client.target_language == "it"
        c.translation_queue.put(seg(0, text="ciao"))
        c.translation_queue.join()
        msg = [m for m in ws.sent if "translated_segments" in m]
        assert msg and msg[-1]["translated_segments"][0]["text"] == "[it] ciao"
    finally:
        s.cleanup(ws)
        srv.ServeClientHIP.MODELS.pop((0, "mt-host-test"), None)
    assert not c.translation_thread.is_alive()


def test_server_keeps_warning_without_a_model(monkeypatch, caplog):
    from whisperlive_amd import server as srv
    s = _server(monkeypatch, None)
    ws = _WS()
    with caplog.at_level("WARNING"):
        s.initialize_client(ws, {"uid": "b", "language": "en", "task": "transcribe", "model": "mt-host-test2",
                                 "enable_translation": True}, None, None, False)
    c = s.client_manager.get_client(ws)
    try:
        assert "enable_translation: the translation side-channel is not part of this server; ignored" in caplog.text
        assert c.translation_queue is None and not hasattr(c, "translation_client")
    finally:
        s.cleanup(ws)
        srv.ServeClientHIP.MODELS.pop((0, "mt-host-test2"), None)


def test_resolve_translation_model_never_downloads_when_disallowed(monkeypatch, tmp_path):
    from whisperlive_amd import artifacts
    calls = []
    monkeypatch.setenv("WLX_NO_DOWNLOAD", "1")
    monkeypatch.delenv("WLX_MODEL_ROOT", raising=False)
    assert artifacts.resolve_translation_model("alirezamsh/small100", snapshot=lambda r, c, local: calls.append(local)) is None
    assert calls == [True]
    d = tmp_path / "m"
    d.mkdir()
    for f in ("config.json", "model.safetensors", "vocab.json", "sentencepiece.bpe.model"):
        (d / f).write_text("{}")
    assert artifacts.resolve_translation_model(str(d)) == str(d)
    monkeypatch.setenv("WLX_MODEL_ROOT", str(tmp_path))
    assert artifacts.resolve_translation_model("m") == str(d)
