"""CPU, loopback only: the OpenAI-style endpoint (whisperlive_amd/rest.py) over a scripted transcriber handed in through
model_factory. Expected bodies are written out as the reference's handler (whisper_live/server.py:733-859) produces them."""
import http.client
import json
import logging
import socket
import struct
import threading

import numpy as np
import pytest

from whisperlive_amd import rest as R
from whisperlive_amd.types import Segment, TranscriptionInfo, TranscriptionOptions, Word

WAV = b"RIFF" + struct.pack("<I", 36 + 8) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + \
    struct.pack("<I", 8) + b"\x00\x01" * 4


def _segments():
    return [
        Segment(id=1, seek=0, start=0.25, end=0.9994, text=" Hello there.", tokens=[50364, 2425, 456, 13], avg_logprob=-0.25,
                compression_ratio=0.75, no_speech_prob=0.0625, temperature=0.0,
                words=[Word(0.25, 0.5, " Hello", 0.875), Word(0.5, 0.9994, " there.", 0.5)]),
        Segment(id=2, seek=3000, start=3725.5, end=3727.125, text=" Über  uns ", tokens=[7, 8], avg_logprob=-0.5,
                compression_ratio=1.5, no_speech_prob=0.125, temperature=0.2, words=[Word(3725.5, 3727.125, " Über", 0.25)]),
    ]


class ScriptedTranscriber:
    """records every transcribe call and the slot it ran on; a pool of slots like WhisperModelHIP's (one per calling thread)"""

    def __init__(self, segments=None, fail=None, barrier=None, lazy_fail_after=None):
        self.segments, self.fail, self.barrier, self.lazy_fail_after = segments, fail, barrier, lazy_fail_after
        self.calls, self.lock = [], threading.Lock()
        self.slots, self.in_use, self.released = [], {}, 0
        self._tls = threading.local()

    def _slot(self):
        s = getattr(self._tls, "slot", None)
        if s is None:
            with self.lock:
                s = next((x for x in self.slots if x not in self.in_use.values()), None)
                if s is None:
                    s = len(self.slots)
                    self.slots.append(s)
                self.in_use[threading.get_ident()] = s
            self._tls.slot = s
        return s

    def release_slot(self):
        with self.lock:
            self.in_use.pop(threading.get_ident(), None)
            self.released += 1
        self._tls.slot = None

    def transcribe(self, audio, **kw):
        slot = self._slot()
        with self.lock:
            self.calls.append((audio, kw, slot))
        if self.barrier is not None:
            self.barrier.wait(timeout=10)
        if self.fail is not None:
            raise self.fail
        segs = _segments() if self.segments is None else self.segments
        info = TranscriptionInfo(language=kw.get("language") or "en", language_probability=1.0, duration=3727.125,
                                 duration_after_vad=3727.125, all_language_probs=None,
                                 transcription_options=TranscriptionOptions(), vad_options=None)
        if self.lazy_fail_after is not None:
            def gen():
                for s in segs[: self.lazy_fail_after]:
                    yield s
                raise RuntimeError("decoder fell over")
            return gen(), info
        return segs, info


@pytest.fixture(autouse=True)
def _clean_model_cache():
    from whisperlive_amd.serve_client import ServeClientHIP
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    yield
    ServeClientHIP.MODELS.clear()
    ServeClientHIP.MODELS.update(saved)


class Served:
    def __init__(self, transcriber=None, **kw):
        from whisperlive_amd.serve_client import ServeClientHIP
        ServeClientHIP.MODELS.clear()              # (the cache is process-wide: each server of a test starts from an empty one)
        self.t = transcriber or ScriptedTranscriber()
        self.made = []

        def factory(model, device_index):
            self.made.append((model, device_index))
            return self.t
        kw.setdefault("model_factory", factory)
        self.server = R.RestServer("127.0.0.1", 0, "tiny.en", **kw).start()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.server.shutdown()

    def request(self, method, path, body=None, headers=None):
        c = http.client.HTTPConnection("127.0.0.1", self.server.port, timeout=10)
        try:
            c.request(method, path, body=body, headers=headers or {})
            r = c.getresponse()
            return r.status, dict((k.lower(), v) for k, v in r.getheaders()), r.read()
        finally:
            c.close()

    def post(self, fields, boundary="XbOuNdArY", headers=None, quoted=False, path=R.ROUTE):
        body = multipart(fields, boundary)
        b = f'"{boundary}"' if quoted else boundary
        h = {"Content-Type": f"multipart/form-data; boundary={b}"}
        h.update(headers or {})
        return self.request("POST", path, body, h)


def multipart(fields, boundary="XbOuNdArY"):
    """fields: list of (name, value) with value str, or (filename, bytes)"""
    out = b""
    for name, value in fields:
        out += b"--" + boundary.encode() + b"\r\n"
        if isinstance(value, tuple):
            out += f'Content-Disposition: form-data; name="{name}"; filename="{value[0]}"\r\n'.encode()
            out += b"Content-Type: application/octet-stream\r\n\r\n" + value[1] + b"\r\n"
        else:
            out += f'Content-Disposition: form-data; name="{name}"\r\n\r\n'.encode() + value.encode() + b"\r\n"
    return out + b"--" + boundary.encode() + b"--\r\n"


FILE = ("file", ("a.wav", WAV))
TEXT = "Hello there. Über  uns"


# ---------------------------------------------------------------------------------------------------------- formats
def test_text_and_json_byte_for_byte():
    with Served() as s:
        st, h, body = s.post([FILE, ("response_format", "text")])
        assert st == 200 and h["content-type"] == "text/plain; charset=utf-8" and body == TEXT.encode("utf-8")
        st, h, body = s.post([FILE])
        assert st == 200 and h["content-type"] == "application/json" and body == ('{"text":"' + TEXT + '"}').encode("utf-8")
        audio, kw, _ = s.t.calls[0]
        assert audio == WAV
        assert kw == dict(language=None, initial_prompt=None, temperature=0.0, vad_filter=False, word_timestamps=False, hotwords=None)
        assert s.made == [("tiny.en", 0)]                     # ONE transcriber for both requests: the GPU's shared one


def test_srt_and_vtt_above_an_hour_and_below_a_second():
    with Served() as s:
        st, _, body = s.post([FILE, ("response_format", "srt")])
        assert st == 200 and body.decode() == ("1\n00:00:00,250 --> 00:00:00,999\nHello there.\n\n"
                                               "2\n01:02:05,500 --> 01:02:07,125\nÜber  uns\n")
        st, _, body = s.post([FILE, ("response_format", "vtt")])
        assert st == 200 and body.decode() == ("00:00:00.250 --> 00:00:00.999\nHello there.\n\n"
                                               "01:02:05.500 --> 01:02:07.125\nÜber  uns\n")


def _verbose(words: bool, speakers=None):
    segs = []
    for i, g in enumerate(_segments()):
        d = {"id": g.id, "seek": g.seek, "start": g.start, "end": g.end, "text": g.text.strip(), "tokens": g.tokens,
             "temperature": g.temperature, "avg_logprob": g.avg_logprob, "compression_ratio": g.compression_ratio,
             "no_speech_prob": g.no_speech_prob}
        if speakers and i in speakers:
            d["speaker"] = speakers[i]
        if words:
            d["words"] = [{"word": w.word, "start": w.start, "end": w.end, "probability": w.probability} for w in g.words]
        segs.append(d)
    return {"task": "transcribe", "language": "de", "duration": 3727.125, "text": TEXT, "segments": segs}


def test_verbose_json_with_and_without_word_granularity():
    with Served() as s:
        st, h, body = s.post([FILE, ("response_format", "verbose_json"), ("language", "de"), ("prompt", "Hallo"),
                              ("temperature", "0.2"), ("hotwords", "uns")])
        want = json.dumps(_verbose(False), ensure_ascii=False, separators=(",", ":")).encode("utf-8")
        assert st == 200 and h["content-type"] == "application/json" and body == want
        assert list(json.loads(body)["segments"][0]) == ["id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob",
                                                         "compression_ratio", "no_speech_prob"]
        assert s.t.calls[0][1] == dict(language="de", initial_prompt="Hallo", temperature=0.2, vad_filter=False,
                                       word_timestamps=False, hotwords="uns")
        st, _, body = s.post([FILE, ("response_format", "verbose_json"), ("language", "de"),
                              ("timestamp_granularities", "segment, word")])
        assert st == 200 and body == json.dumps(_verbose(True), ensure_ascii=False, separators=(",", ":")).encode("utf-8")
        assert s.t.calls[1][1]["word_timestamps"] is True
        # repeated fields, and the bracketed spelling some clients use
        st, _, body = s.post([FILE, ("response_format", "verbose_json"), ("language", "de"), ("timestamp_granularities[]", "segment"),
                              ("timestamp_granularities[]", "word")])
        assert st == 200 and json.loads(body) == _verbose(True) and s.t.calls[2][1]["word_timestamps"] is True


def test_ignored_parameters_and_model_name_are_warned_about(caplog):
    with Served() as s, caplog.at_level(logging.WARNING):
        st, _, _ = s.post([FILE, ("chunking_strategy", "auto"), ("include", "logprobs"), ("include", "x"), ("model", "gpt-4o-transcribe")])
        assert st == 200
    msgs = [r.getMessage() for r in caplog.records]
    assert "Unsupported OpenAI params ignored: chunking_strategy='auto', include=['logprobs', 'x']" in msgs
    assert "Model 'gpt-4o-transcribe' requested; using 'tiny.en' as fallback." in msgs


# ---------------------------------------------------------------------------------------------------------- statuses
def test_400s():
    with Served() as s:
        st, _, body = s.post([FILE, ("response_format", "yaml")])
        assert st == 400 and body == b'{"error":"Unsupported response_format. Supported: [\'json\', \'text\', \'srt\', \'verbose_json\', \'vtt\']"}'
        st, _, body = s.post([("response_format", "json")])
        assert st == 400 and b"file" in body                                        # no file
        st, _, body = s.post([("file", ("a.mp3", b"ID3\x03" + b"\x00" * 64))])
        assert st == 400 and b"neither WAV nor FLAC" in body                         # undecodable
        st, _, body = s.post([("file", ("a.wav", b""))])
        assert st == 400 and b"neither WAV nor FLAC" in body                         # an empty file parses, and is no audio
        st, _, _ = s.request("POST", R.ROUTE, b"--x\r\nrubbish", {"Content-Type": "multipart/form-data; boundary=x"})
        assert st == 400
        st, _, _ = s.request("POST", R.ROUTE, b"{}", {"Content-Type": "application/json"})
        assert st == 400
        st, _, _ = s.request("POST", R.ROUTE, multipart([FILE])[:-20], {"Content-Type": "multipart/form-data; boundary=XbOuNdArY"})
        assert st == 400                                                             # no closing boundary
        st, _, _ = s.post([FILE, ("temperature", "warm")])
        assert st == 400
        assert s.t.calls == []


def test_401_429_413_404_405_500():
    with Served(api_key="sekret") as s:
        assert s.post([FILE])[0] == 401
        st, _, body = s.post([FILE], headers={"Authorization": "Bearer wrong"})
        assert st == 401 and body == b'{"error":"Invalid or missing API key"}'
        assert s.post([FILE], headers={"Authorization": "Bearer sekret"})[0] == 200
    with Served(rate_limit_rpm=2) as s:
        assert [s.post([FILE])[0] for _ in range(3)] == [200, 200, 429]
        assert s.post([FILE])[2] == b'{"error":"Rate limit exceeded"}'
    with Served(max_body_bytes=1000) as s:
        st, _, body = s.post([("file", ("a.wav", WAV + b"\x00" * 2000))])
        assert st == 413 and s.t.calls == []
        assert s.post([FILE])[0] == 200
    with Served(ScriptedTranscriber(fail=RuntimeError("HBM on fire"))) as s:
        st, _, body = s.post([FILE])
        assert st == 500 and body == b'{"error":"HBM on fire"}'
        assert s.t.released == 1                                                     # the slot goes back on the failure path too
        assert s.request("GET", "/v1/models")[0] == 404
        assert s.request("POST", "/v1/audio/translations", b"")[0] == 404
        assert s.request("GET", R.ROUTE)[0] == 405
        assert s.request("DELETE", R.ROUTE)[0] == 405


# ---------------------------------------------------------------------------------------------------------- multipart
def test_early_answers_reach_a_client_that_is_still_uploading():
    """401 / 413 are decided from the headers: the unread upload is read and dropped first, so the client sees the status and not
    a reset connection; a client that sent `Expect: 100-continue` is answered before it has sent a byte of the body"""
    big = multipart([("file", ("a.wav", WAV + bytes(4 << 20)))])
    ctype = {"Content-Type": "multipart/form-data; boundary=XbOuNdArY"}
    with Served(api_key="k") as s:
        st, _, body = s.request("POST", R.ROUTE, big, ctype)
        assert st == 401 and json.loads(body) == {"error": "Invalid or missing API key"}
    with Served(max_body_bytes=1 << 20) as s:
        st, _, body = s.request("POST", R.ROUTE, big, ctype)
        assert st == 413
        small = multipart([FILE, ("response_format", "text")])
        head = ("POST " + R.ROUTE + " HTTP/1.1\r\nHost: x\r\nContent-Type: " + ctype["Content-Type"] + "\r\nExpect: 100-continue\r\n")

        def talk(length, body):
            with socket.create_connection(("127.0.0.1", s.server.port), timeout=10) as c:
                c.sendall((head + f"Content-Length: {length}\r\n\r\n").encode())
                first = c.recv(65536)
                if first.startswith(b"HTTP/1.1 100"):
                    c.sendall(body)
                    first = b""
                while True:
                    chunk = c.recv(65536)
                    if not chunk:
                        return first
                    first += chunk

        answer = talk(len(big), None)                          # over the limit: refused with nothing uploaded
        assert answer.split(b" ", 2)[1] == b"413"
        answer = talk(len(small), small)                       # within it: 100 Continue, then the ordinary answer
        assert answer.split(b" ", 2)[1] == b"200" and answer.endswith(TEXT.encode("utf-8"))


def test_multipart_edge_cases():
    nasty = WAV + b"\r\n--XbOuNdAr\r\n--XbOuNdArYz\r\nContent-Disposition: form-data; name=\"response_format\"\r\n\r\nsrt\r\n--XbOuNdArY_\r\n"
    with Served() as s:
        st, _, body = s.post([("file", ("a.wav", nasty)), ("response_format", "text")], quoted=True)
        assert st == 200 and body == TEXT.encode() and s.t.calls[0][0] == nasty
    parts = R.parse_multipart(multipart([("a", "1"), ("a", "2,3"), ("b", ("f.bin", b"")), ("c", "")]), 'multipart/form-data; boundary="XbOuNdArY"')
    assert [(p.name, p.filename, p.data) for p in parts] == [("a", None, b"1"), ("a", None, b"2,3"), ("b", "f.bin", b""), ("c", None, b"")]
    assert R.normalize_form_list(["1", "2, 3", " ", ""]) == ["1", "2", "3"]
    # a preamble, bare LF inside content, and blanks behind the boundary
    body = b"preamble\r\n--b \r\nContent-Disposition: form-data; name=x\r\n\r\nl1\nl2\r\n--b--\r\nepilogue"
    assert [(p.name, p.data) for p in R.parse_multipart(body, "multipart/form-data; charset=utf-8; boundary=b")] == [("x", b"l1\nl2")]
    for bad in ("text/plain", "multipart/form-data", "multipart/form-data; boundary="):
        with pytest.raises(ValueError):
            R.parse_multipart(body, bad)


# ---------------------------------------------------------------------------------------------------------- streaming
def test_sse_framing_done_and_mid_stream_error():
    with Served() as s:
        st, h, body = s.post([FILE, ("stream", "true"), ("timestamp_granularities", "word"), ("response_format", "nonsense")])
        assert st == 200 and h["content-type"].startswith("text/event-stream")
        segs = _segments()
        ev = [{"id": g.id, "start": g.start, "end": g.end, "text": g.text.strip(),
               "words": [{"word": w.word, "start": w.start, "end": w.end, "probability": w.probability} for w in g.words]} for g in segs]
        assert body.decode() == "".join(f"data: {json.dumps(e)}\n\n" for e in ev) + "data: [DONE]\n\n"
        assert "hotwords" not in s.t.calls[0][1] and s.t.calls[0][1]["word_timestamps"] is True
    with Served(ScriptedTranscriber(lazy_fail_after=1)) as s:
        st, _, body = s.post([FILE, ("stream", "1")])
        first = {"id": 1, "start": 0.25, "end": 0.9994, "text": "Hello there."}
        assert st == 200 and body.decode() == f"data: {json.dumps(first)}\n\n" + 'data: {"error": "decoder fell over"}\n\n'
        assert s.t.released == 1


# ---------------------------------------------------------------------------------------------------------- speakers
class FakeEmbedder:
    """unit vectors by the sign of the audio's mean; None under 0.3 s, as the HIP embedder"""

    def __call__(self, pcm, sample_rate=16000):
        pcm = np.asarray(pcm, dtype=np.float32)
        if pcm.shape[0] < 4800:
            return None
        return np.array([1.0, 0.0], np.float32) if pcm.mean() >= 0 else np.array([0.0, 1.0], np.float32)


def _wav16(samples: np.ndarray) -> bytes:
    d = (np.clip(samples, -1, 1) * 32767).astype("<i2").tobytes()
    return b"RIFF" + struct.pack("<I", 36 + len(d)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + \
        struct.pack("<I", len(d)) + d


def test_known_speakers_validation_and_labels():
    made = []

    def embedders(path, device_index):
        made.append((path, device_index))
        return FakeEmbedder()
    segs = [Segment(1, 0, 0.0, 1.0, " a", [1], -0.1, 1.0, 0.0, None, 0.0), Segment(2, 0, 1.0, 2.0, " b", [2], -0.1, 1.0, 0.0, None, 0.0),
            Segment(3, 0, 2.0, 2.0, " c", [3], -0.1, 1.0, 0.0, None, 0.0)]
    audio = np.concatenate([np.full(16000, 0.5, np.float32), np.full(16000, -0.5, np.float32)])
    pos, neg = _wav16(np.full(8000, 0.25, np.float32)), _wav16(np.full(8000, -0.25, np.float32))
    base = [("file", ("a.wav", _wav16(audio))), ("response_format", "verbose_json")]
    with Served(ScriptedTranscriber(segments=segs), embedder_factory=embedders) as s:
        st, _, body = s.post(base + [("known_speaker_references", ("p.wav", pos))])
        assert st == 400 and body == b'{"error":"known_speaker_references requires matching known_speaker_names"}'
        st, _, body = s.post(base + [("known_speaker_names", "ann,bob"), ("known_speaker_references", ("p.wav", pos))])
        assert st == 400 and body == b'{"error":"known_speaker_names and known_speaker_references must have the same length"}'
        st, _, body = s.post(base + [("known_speaker_names", "ann"), ("known_speaker_references", ("p.wav", _wav16(np.zeros(100, np.float32))))])
        assert st == 400 and body == b'{"error":"known_speaker_references for \'ann\' is too short"}'
        st, _, body = s.post(base + [("known_speaker_names", "ann"), ("known_speaker_names", "bob"),
                                     ("known_speaker_references", ("p.wav", pos)), ("known_speaker_references", ("n.wav", neg))])
        assert st == 200
        got = json.loads(body)["segments"]
        assert [g.get("speaker") for g in got] == ["ann", "bob", None]            # (the empty third segment gets no label)
        assert made and made[-1][1] == 0
        assert all("speaker" not in g for g in json.loads(s.post(base)[2])["segments"])
    with Served(ScriptedTranscriber(segments=segs), diarization_model="/nonexistent/wespeaker.bin") as s:
        st, _, body = s.post(base + [("known_speaker_names", "ann"), ("known_speaker_references", ("p.wav", pos))])
        assert st == 400 and b"no speaker-embedding checkpoint" in body


# ---------------------------------------------------------------------------------------------------------- CORS
def test_cors_preflight_and_simple_headers():
    with Served(cors_origins="https://a.example, https://b.example") as s:
        st, h, body = s.request("OPTIONS", R.ROUTE, headers={"Origin": "https://b.example", "Access-Control-Request-Method": "POST",
                                                              "Access-Control-Request-Headers": "authorization, content-type"})
        assert st == 200 and body == b"OK"
        assert h["access-control-allow-origin"] == "https://b.example" and h["access-control-allow-credentials"] == "true"
        assert "POST" in h["access-control-allow-methods"] and h["access-control-allow-headers"] == "authorization, content-type"
        assert h["access-control-max-age"] == "600" and h["vary"] == "Origin"
        st, h, _ = s.request("OPTIONS", R.ROUTE, headers={"Origin": "https://evil.example", "Access-Control-Request-Method": "POST"})
        assert st == 400 and "access-control-allow-origin" not in h
        st, h, _ = s.post([FILE], headers={"Origin": "https://a.example"})
        assert st == 200 and h["access-control-allow-origin"] == "https://a.example"
        st, h, _ = s.post([FILE], headers={"Origin": "https://evil.example"})
        assert st == 200 and "access-control-allow-origin" not in h
        assert "access-control-allow-origin" not in s.post([FILE])[1]


# ---------------------------------------------------------------------------------------------------------- concurrency
def test_four_concurrent_requests_each_on_a_slot_of_its_own_and_devices_rotate():
    t = ScriptedTranscriber(barrier=threading.Barrier(4))
    with Served(t, devices=[0, 1]) as s:
        out = [None] * 4

        def go(i):
            out[i] = s.post([FILE, ("response_format", "text")])[0]
        th = [threading.Thread(target=go, args=(i,)) for i in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join(15)
        assert out == [200] * 4
        assert sorted(c[2] for c in t.calls) == [0, 1, 2, 3]          # four requests in flight at once: four slots
        assert t.released == 4 and not t.in_use
        assert sorted(s.made) == [("tiny.en", 0), ("tiny.en", 1)]      # one transcriber per GPU, requests alternate
        t.barrier = None
        assert s.post([FILE])[0] == 200 and t.calls[-1][2] == 0        # a handed-back slot is reused


def test_shares_the_websocket_servers_model_cache():
    from whisperlive_amd.serve_client import ServeClientHIP
    shared = ScriptedTranscriber()
    with Served() as s:
        ServeClientHIP.MODELS[0] = shared                              # what a single_model session of GPU 0 left there
        assert s.post([FILE])[0] == 200
        assert s.made == [] and len(shared.calls) == 1


def test_shutdown_leaves_no_thread_behind():
    before = set(threading.enumerate())
    s = Served()
    assert s.post([FILE])[0] == 200
    assert any(t.name == "wlx-rest" for t in threading.enumerate())
    s.server.shutdown()
    assert set(threading.enumerate()) <= before
    s.server.shutdown()                                                # idempotent
    with pytest.raises(OSError):
        s.post([FILE])


def test_enable_rest_on_the_websocket_server_still_raises():
    """the endpoint is a module of its own; TranscriptionServer.run(enable_rest=True) is wired to it in a later change"""
    from whisperlive_amd.server import TranscriptionServer
    with pytest.raises(NotImplementedError):
        TranscriptionServer().run("127.0.0.1", port=0, enable_rest=True)


def test_metrics_helper_is_a_no_op_without_prometheus():
    from whisperlive_amd import metrics
    metrics.track_rest_request(endpoint="transcriptions", status=200)
    metrics.track_rest_request("transcriptions", 500)
