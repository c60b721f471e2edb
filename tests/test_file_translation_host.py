"""CPU: translated transcripts of the file routes on scripted parts — file_translation.translate_segments, the target_language
option of BatchedInferencePipeline.transcribe / transcribe_many (scripted engine of tests/fakes.py), the REST endpoint's renderings
with and without the field (scripted transcriber of tests/test_rest.py; the bodies without the field are the ones that module
writes out for the parent's handler), the 400s, and the binding of wlx_mt_translate_many against the header."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import file_translation as FT
from whisperlive_amd.types import Segment, Word

from .test_rest import FILE, TEXT, Served, _clean_model_cache, _segments, _verbose  # noqa: F401  (the fixture is autouse here too)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ScriptedTranslator:
    """records its calls; "translates" by tagging: deterministic, and different for every text and language"""

    def __init__(self, codes=("de", "fr", "ja")):
        self.calls = []
        self.tokenizer = self      # check_target_language reads tokenizer.lang_id
        self.codes = set(codes)

    def lang_id(self, code):
        if code not in self.codes:
            raise KeyError(code)
        return 1

    def translate_many(self, texts, lang):
        self.calls.append((list(texts), lang))
        return [f"<{lang}>{t}</{lang}>" for t in texts]


def _segs():
    a, b = _segments()
    empty = Segment(id=3, seek=3000, start=3727.125, end=3727.5, text="   ", tokens=[], avg_logprob=0.0, compression_ratio=0.0,
                    no_speech_prob=0.5, temperature=0.0, words=[], channel=1)
    b = dataclasses.replace(b, channel=0)
    b.speaker = "SPEAKER_01"           # (labels ride on the objects of some routes)
    return [a, b, empty]


# ------------------------------------------------------------------------------------------------- translate_segments
def test_translate_segments_adds_translation_and_keeps_everything_else():
    tr = ScriptedTranslator()
    src = _segs()
    before = [dataclasses.asdict(s) for s in src]
    out = FT.translate_segments(iter(src), tr, "de")
    assert [dataclasses.asdict(s) for s in src] == before and not any(hasattr(s, "translation") for s in src)      # inputs untouched
    assert [dataclasses.asdict(s) for s in out] == before                      # ids, times, words, channel, tokens, ...
    assert out[1].speaker == "SPEAKER_01" and out[1].channel == 0 and out[0].words == src[0].words
    assert [s.translation for s in out] == ["<de>Hello there.</de>", "<de>Über  uns</de>", "   "]
    # one call per file, the empty text not sent
    assert tr.calls == [(["Hello there.", "Über  uns"], "de")]


def test_translate_segments_without_a_language_or_without_text():
    tr = ScriptedTranslator()
    src = _segs()
    assert FT.translate_segments(src, tr, None) == src and tr.calls == []
    out = FT.translate_segments([src[2]], tr, "de")
    assert out[0].translation == "   " and tr.calls == []        # nothing to send: no call at all
    assert FT.translate_segments([], tr, "de") == [] and FT.translate_segments(None, tr, "de") == []
    with pytest.raises(ValueError, match="needs a translator"):
        FT.translate_segments(src, None, "de")


def test_translators_of_three_kinds_and_a_short_answer():
    class OnlyTranslate:
        def translate(self, texts, lang):
            return [t.upper() for t in texts]
    assert [s.translation for s in FT.translate_segments(_segs()[:1], OnlyTranslate(), "de")] == ["HELLO THERE."]
    assert [s.translation for s in FT.translate_segments(_segs()[:1], lambda t, lang: [lang + ":" + x for x in t], "fr")] == ["fr:Hello there."]
    with pytest.raises(RuntimeError, match="returned 1 texts for 2"):
        FT.translate_segments(_segs(), lambda t, lang: t[:1], "de")
    with pytest.raises(TypeError):
        FT.translate_segments(_segs(), object(), "de")


def test_check_target_language():
    tr = ScriptedTranslator()
    FT.check_target_language(tr, "de")
    with pytest.raises(ValueError, match="'xx' is not a language"):
        FT.check_target_language(tr, "xx")
    for bad in ("", "  ", None, 5):
        with pytest.raises(ValueError):
            FT.check_target_language(tr, bad)
    FT.check_target_language(lambda t, lang: t, "xx")          # a bare callable has no code table to ask


def test_hip_translator_translate_many_skips_empty_texts_and_makes_one_engine_call():
    from whisperlive_amd.mt_weights import MTGenOptions
    from whisperlive_amd.translation import HipTranslator

    class Tok:
        def encode_source(self, text, lang):
            return [7] + [ord(c) for c in text] + [2]

        def decode(self, ids):
            return "".join(chr(i) for i in ids)

    class Eng:
        max_batch, max_src = 2, 6
        calls = []

        def translate_ids_many(self, srcs, opts):
            self.calls.append([list(s) for s in srcs])
            return [s[1:-1][::-1] for s in srcs], [0.0] * len(srcs)
    tr = HipTranslator(None, engine=Eng(), tokenizer=Tok(), options=MTGenOptions())
    out = tr.translate_many(["abc", "", "  ", "de", "abcdefgh", None], "de")
    assert out == ["cba", "", "  ", "ed", "dcba", None]
    # ONE call for more texts than max_batch; a source longer than max_src is cut to it, its last token kept
    assert Eng.calls == [[[7, 97, 98, 99, 2], [7, 100, 101, 2], [7, 97, 98, 99, 100, 2]]]


# ------------------------------------------------------------------------------------------------- the batched pipeline
SR = 16000
CLIPS = [{"start": 0, "end": SR}, {"start": SR, "end": 2 * SR}]
PIPE_KW = dict(language="en", vad_filter=False, clip_timestamps=CLIPS, chunk_length=1)


def _pipeline(max_batch=3, many=False):
    from tests import test_batched_pipeline_host as one_file
    from tests import test_many_files_host as many_files
    return (many_files if many else one_file)._model(max_batch=max_batch)


def test_pipeline_transcribe_with_and_without_target_language():
    from whisperlive_amd.batched import BatchedInferencePipeline
    hip, _eng = _pipeline()
    audio = np.zeros(2 * SR, np.float32)
    kw = dict(PIPE_KW, batch_size=2)
    plain, info = BatchedInferencePipeline(hip).transcribe(audio, **kw)
    plain = list(plain)
    assert plain and not any(hasattr(s, "translation") for s in plain)
    tr = ScriptedTranslator()
    got, info2 = BatchedInferencePipeline(hip).transcribe(audio, target_language="fr", translator=tr, **kw)
    assert isinstance(got, list) and got == plain and info2.duration == info.duration          # (dataclass equality: every field)
    assert [s.translation for s in got] == [f"<fr>{s.text.strip()}</fr>" for s in plain]
    assert len(tr.calls) == 1
    with pytest.raises(ValueError, match="not a language"):
        BatchedInferencePipeline(hip).transcribe(audio, target_language="xx", translator=tr, **kw)
    calls = len(_eng.slots[0].calls)
    with pytest.raises(ValueError, match="needs a translator"):
        BatchedInferencePipeline(hip).transcribe(audio, target_language="fr", **kw)
    assert len(_eng.slots[0].calls) == calls          # refused before the file is touched


def test_transcribe_many_takes_target_language_per_file():
    from whisperlive_amd.batched import BatchedInferencePipeline
    hip, _eng = _pipeline(max_batch=6, many=True)
    audios = [np.full(2 * SR, 0.1 * (i + 1), np.float32) for i in range(3)]
    kw = dict(PIPE_KW)
    pipe = BatchedInferencePipeline(hip)
    plain = pipe.transcribe_many(audios, batch_size=3, **kw)
    assert pipe.transcribe_many(audios, batch_size=3, target_language=None, translator=None, **kw) == plain
    tr = ScriptedTranslator()
    got = pipe.transcribe_many(audios, batch_size=3, target_language=["de", None, "ja"], translator=tr, **kw)
    assert [g[0] for g in got] == [p[0] for p in plain]
    for (segs, _info), lang in zip(got, ("de", None, "ja")):
        if lang is None:
            assert not any(hasattr(s, "translation") for s in segs)
        else:
            assert [s.translation for s in segs] == [f"<{lang}>{s.text.strip()}</{lang}>" for s in segs]
    assert [c[1] for c in tr.calls] == ["de", "ja"]              # one call per translated file
    one = pipe.transcribe_many(audios, batch_size=3, target_language="fr", translator=tr, **kw)
    assert all(s.translation.startswith("<fr>") for segs, _ in one for s in segs)
    by_iter = sorted(pipe.iter_many(audios, batch_size=3, target_language="fr", translator=tr, **kw), key=lambda x: x[0])
    assert [x[1] for x in by_iter] == [g[0] for g in one]
    with pytest.raises(ValueError, match="a list of 2 entries for 3 files"):
        pipe.transcribe_many(audios, batch_size=3, target_language=["de", "fr"], translator=tr, **kw)
    with pytest.raises(ValueError, match="not a language"):
        pipe.transcribe_many(audios, batch_size=3, target_language=["de", "xx", None], translator=tr, **kw)


# ------------------------------------------------------------------------------------------------- the REST endpoint
TR_TEXT = "<de>Hello there.</de> <de>Über  uns</de>"


def _served(**kw):
    tr = ScriptedTranslator()
    made = []

    def factory(model, device_index):
        made.append((model, device_index))
        return tr
    s = Served(translation_model="some/small100", translator_factory=factory, **kw)
    s.tr, s.tr_made = tr, made
    return s


def test_rest_renders_the_translation_in_every_format():
    with _served() as s:
        lang = ("target_language", "de")
        st, h, body = s.post([FILE, ("response_format", "text"), lang])
        assert st == 200 and h["content-type"] == "text/plain; charset=utf-8" and body == TR_TEXT.encode("utf-8")
        st, h, body = s.post([FILE, lang])
        assert st == 200 and body == ('{"text":"' + TEXT + '","translation":"' + TR_TEXT + '"}').encode("utf-8")
        st, _, body = s.post([FILE, ("response_format", "srt"), lang])
        assert st == 200 and body.decode() == ("1\n00:00:00,250 --> 00:00:00,999\n<de>Hello there.</de>\n\n"
                                               "2\n01:02:05,500 --> 01:02:07,125\n<de>Über  uns</de>\n")
        st, _, body = s.post([FILE, ("response_format", "vtt"), lang])
        assert st == 200 and body.decode() == ("00:00:00.250 --> 00:00:00.999\n<de>Hello there.</de>\n\n"
                                               "01:02:05.500 --> 01:02:07.125\n<de>Über  uns</de>\n")
        st, _, body = s.post([FILE, ("response_format", "verbose_json"), ("language", "de"), ("timestamp_granularities[]", "word"), lang])
        want = _verbose(True)
        want["target_language"], want["translation"] = "de", TR_TEXT
        for seg, t in zip(want["segments"], ("<de>Hello there.</de>", "<de>Über  uns</de>")):
            seg["translation"] = t                 # the words (and their times) stay the source's
        assert st == 200 and json.loads(body) == want
        assert [c[1] for c in s.tr.calls] == ["de"] * 5 and all(c[0] == ["Hello there.", "Über  uns"] for c in s.tr.calls)      # one job per file
        assert s.tr_made[0] == ("some/small100", 0)


def test_rest_without_the_field_answers_byte_for_byte_as_before():
    """the expectations tests/test_rest.py writes out for the parent's handler, from a server WITH a translation model"""
    with _served() as s:
        st, h, body = s.post([FILE, ("response_format", "text")])
        assert st == 200 and h["content-type"] == "text/plain; charset=utf-8" and body == TEXT.encode("utf-8")
        st, h, body = s.post([FILE])
        assert st == 200 and h["content-type"] == "application/json" and body == ('{"text":"' + TEXT + '"}').encode("utf-8")
        st, _, body = s.post([FILE, ("response_format", "srt")])
        assert body.decode() == "1\n00:00:00,250 --> 00:00:00,999\nHello there.\n\n2\n01:02:05,500 --> 01:02:07,125\nÜber  uns\n"
        st, _, body = s.post([FILE, ("response_format", "vtt")])
        assert body.decode() == "00:00:00.250 --> 00:00:00.999\nHello there.\n\n01:02:05.500 --> 01:02:07.125\nÜber  uns\n"
        st, _, body = s.post([FILE, ("response_format", "verbose_json"), ("language", "de"), ("timestamp_granularities[]", "word")])
        assert st == 200 and body == R_json(_verbose(True))
        st, _, body = s.post([FILE, ("target_language", "  ")])          # an empty field is no field
        assert st == 200 and body == ('{"text":"' + TEXT + '"}').encode("utf-8")
        assert s.tr.calls == [] and s.tr_made == []


def R_json(obj) -> bytes:
    from whisperlive_amd.rest import _json_bytes
    return _json_bytes(obj)


def test_rest_400s():
    with Served() as s:            # no model configured
        st, _, body = s.post([FILE, ("target_language", "de")])
        assert st == 400 and "no translation model" in json.loads(body)["error"] and "--translation_model" in json.loads(body)["error"]
        assert s.t.calls == []                               # refused before the file is decoded
        st, _, body = s.post([FILE, ("target_language", "de"), ("stream", "true")])
        assert st == 400 and "no translation model" in json.loads(body)["error"]
    with _served() as s:           # an unknown language code
        st, _, body = s.post([FILE, ("target_language", "xx")])
        assert st == 400 and "'xx' is not a language" in json.loads(body)["error"]
        assert s.t.calls == [] and s.tr.calls == []


def test_rest_stream_emits_the_translations_in_one_final_event():
    with _served() as s:
        st, h, body = s.post([FILE, ("stream", "true"), ("target_language", "ja")])
        assert st == 200 and h["content-type"].startswith("text/event-stream")
        events = [e[len("data: "):] for e in body.decode().split("\n\n") if e]
        assert events[-1] == "[DONE]" and len(events) == 4
        assert [json.loads(e)["text"] for e in events[:2]] == ["Hello there.", "Über  uns"]
        assert json.loads(events[2]) == {"target_language": "ja", "translations": [{"id": 1, "translation": "<ja>Hello there.</ja>"},
                                                                                  {"id": 2, "translation": "<ja>Über  uns</ja>"}]}
        plain = s.post([FILE, ("stream", "true")])[2].decode()
        assert plain == "\n\n".join("data: " + e for e in events[:2] + ["[DONE]"]) + "\n\n"
        assert len(s.tr.calls) == 1


def test_rest_translation_with_the_pooled_route():
    """FileBatcher (file_batch_window_ms > 0): the upload is transcribed in a pooled job and translated in its own request thread"""
    from tests.test_rest import ScriptedTranscriber

    class Pipe:
        def __init__(self, t):
            self.t = t

        def iter_many(self, audios, **kw):
            for i, _a in enumerate(audios):
                segs, info = self.t.transcribe(_a)
                yield i, list(segs), info
    t = ScriptedTranscriber()
    with _served(transcriber=t, file_batch_size=2, file_batch_window_ms=1, pipeline_factory=lambda tr: Pipe(tr),
                 model_factory=lambda model, device_index, **kw: t) as s:
        st, _, body = s.post([FILE, ("target_language", "fr")])
        assert st == 200 and json.loads(body) == {"text": TEXT, "translation": "<fr>Hello there.</fr> <fr>Über  uns</fr>"}
        st, _, body = s.post([FILE])
        assert st == 200 and body == ('{"text":"' + TEXT + '"}').encode("utf-8")


# ------------------------------------------------------------------------------------------------- the binding
def _header_prototype(name):
    src = open(os.path.join(ROOT, "include", "wlx.h"), encoding="utf-8").read()
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, name
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        arg = arg.strip()
        ptr = "*" in arg
        base = re.sub(r"\bconst\b", "", arg).replace("*", " ").split()[0]
        out.append((base, ptr))
    return out


@pytest.mark.parametrize("name", ["wlx_mt_translate_many", "wlx_mt_debug_search"])
def test_the_new_entry_points_are_bound_with_the_headers_prototypes(name):
    _lib.build()
    lib = _lib.load()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ctype = {("int32_t", False): C.c_int32, ("int32_t", True): i32p, ("float", True): f32p, ("wlx_mt", True): C.c_void_p,
             ("wlx_mt_gen_opts", True): C.POINTER(_lib.wlx_mt_gen_opts)}
    want = [ctype[a] for a in _header_prototype(name)]
    fn = getattr(lib, name)
    assert list(fn.argtypes) == want and fn.restype is C.c_int32
    assert name in _lib.EXPORTS and "mt_search.hip" in _lib.SOURCES
    assert _lib.MT_MANY_MAX == int(re.search(r"#define WLX_MT_MANY_MAX (\d+)", open(os.path.join(ROOT, "include", "wlx.h")).read()).group(1))
    assert lib.wlx_abi_version() == 1
