"""CPU tests of wire-format live sessions (the protocol keys sample_rate / channels / audio_format of the first JSON message): the
server hands such a session its packets unconverted, the session resamples them — here on the host, the engine being a fake — and
everything behind the buffer sees 16 kHz. Sessions with the default options never reach the new code."""
import json
import threading
import time
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests import resample_kernel_ref as R
from whisperlive_amd import stream_resample as SR
from whisperlive_amd import ws
from whisperlive_amd.serve_client import ServeClientBase, ServeClientHIP
from whisperlive_amd.server import TranscriptionServer


class RecordingTranscriber:
    """a fake engine: records the PCM it is handed, answers one segment over the whole chunk"""

    def __init__(self):
        self.calls = []

    def transcribe(self, audio, **kw):
        self.calls.append(audio.copy())
        dur = audio.shape[0] / 16000.0
        return ([SimpleNamespace(start=0.0, end=dur, text=f" n{len(self.calls)}", no_speech_prob=0.0, words=None)],
                SimpleNamespace(language="en", language_probability=0.99))


@pytest.fixture
def running_server():
    started = []

    def start(**kw):
        srv, ready = TranscriptionServer(), threading.Event()
        kw.setdefault("model_factory", lambda model, dev: RecordingTranscriber())
        t = threading.Thread(target=srv.run, args=("127.0.0.1",), kwargs=dict(port=0, ready=ready, **kw), daemon=True)
        t.start()
        assert ready.wait(10)
        started.append((srv, t))
        return srv

    ServeClientHIP.MODELS.clear()
    yield start
    for srv, t in started:
        srv.shutdown()
        t.join(5)
    ServeClientHIP.MODELS.clear()


OPTS = dict(uid="u1", language="en", task="transcribe", model="small.en", use_vad=False, send_last_n_segments=10,
            no_speech_thresh=0.45, clip_audio=False, same_output_threshold=10)


def mulaw_encode(x):
    table = SR.decode_mulaw(np.arange(256, dtype=np.uint8)).astype(np.float64)
    return np.abs(np.asarray(x, np.float64)[:, None] * 32768.0 - table[None, :]).argmin(axis=1).astype(np.uint8)


def oracle(codes, rate=8000):
    """the host oracle of the whole stream: scipy.signal.resample_poly of the decoded samples"""
    return R.scipy_ref(SR.decode_samples(codes, SR.WIRE_FORMATS["mulaw"][0]), *R.ratio(rate)).astype(np.float32)


def _wait(cond, seconds=10.0):
    deadline = time.time() + seconds
    while not cond() and time.time() < deadline:
        time.sleep(0.01)
    return cond()


def test_e2e_8khz_mulaw_session_is_resampled_to_the_16khz_timeline(running_server):
    srv = running_server(single_model=True)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, sample_rate=8000, audio_format="mulaw")))
    assert json.loads(c.recv(timeout=10.0))["message"] == "SERVER_READY"
    codes = mulaw_encode(0.5 * R.speech_like(16000, 8000, seed=3))                 # 2 s
    want = oracle(codes)
    assert want.shape[0] == 32000                                                  # ceil(16000 * up / down)
    for i in range(0, codes.shape[0], 160):                                        # 20 ms packets
        c.send(codes[i: i + 160].tobytes())
    assert _wait(lambda: len(srv.client_manager.clients) == 1)
    client = next(iter(srv.client_manager.clients.values()))
    assert SR.stream_count(8000, 16000) == 32000 - 20                              # the filter's look-ahead is still to come
    assert _wait(lambda: client.frames_np is not None and client.frames_np.shape[0] == 32000 - 20)
    msg = json.loads(c.recv(timeout=10.0))
    assert msg["segments"] and float(msg["segments"][0]["end"]) <= 2.0             # seconds of 16 kHz audio
    c.send(b"END_OF_AUDIO")
    with pytest.raises(ws.ConnectionClosed):
        for _ in range(200):
            c.recv(timeout=5.0)
    assert _wait(lambda: not srv.client_manager.clients) and not srv.audio_formats and not srv.wire_sessions
    # the flush completed the buffer to the one-shot length; it equals the oracle of the whole stream
    assert client._wire.closed and client.frames_np.shape[0] == 32000
    assert np.abs(client.frames_np - want).max() <= R.RESAMPLE_ATOL / 4
    assert client.frames_offset == 0.0 and 0.0 <= client.timestamp_offset <= 2.0
    audio = ServeClientHIP.MODELS[0].calls[0]                                      # what the engine was handed: 16 kHz PCM from sample 0
    assert audio.dtype == np.float32 and audio.shape[0] >= 16000 and np.array_equal(audio, client.frames_np[: audio.shape[0]])


def test_offsets_of_a_wire_session_are_on_the_16khz_timeline_across_trims():
    class Short(ServeClientHIP):
        MAX_BUFFER_DURATION_S, BUFFER_TRIM_DURATION_S = 2, 1

    c = Short(MagicMock(), client_uid="u", model=None, transcriber=RecordingTranscriber(), use_vad=False, start_thread=False)
    c.set_wire_format("mulaw", 1, 8000)
    codes = mulaw_encode(0.5 * R.speech_like(5 * 8000, 8000, seed=4))
    want = oracle(codes)
    for i in range(0, codes.shape[0], 160):
        c.add_wire_frames(codes[i: i + 160].tobytes())
    c.add_wire_frames(b"", flush=True)
    assert c._ring is False                                                        # no engine behind the transcriber: the host resampler
    assert c.frames_offset >= 2.0 and c.timestamp_offset == c.frames_offset        # trims of one 16 kHz second each
    first = int(round(c.frames_offset * 16000))
    assert first + c.frames_np.shape[0] == want.shape[0] == 80000
    assert np.abs(c.frames_np - want[first:]).max() <= R.RESAMPLE_ATOL / 4
    n = c.frames_np.shape[0]
    c.add_wire_frames(codes[:160].tobytes())                                       # after the flush the stream is closed
    assert c.frames_np.shape[0] == n


def test_default_sessions_never_touch_the_wire_code(running_server, monkeypatch):
    touched = []
    monkeypatch.setattr(ServeClientBase, "set_wire_format", lambda self, *a, **k: touched.append("set_wire_format"))
    monkeypatch.setattr(ServeClientBase, "add_wire_frames", lambda self, *a, **k: touched.append("add_wire_frames"))
    monkeypatch.setattr(SR, "check_format", lambda *a, **k: touched.append("check_format"))
    monkeypatch.setattr(SR.StreamResampler, "__init__", lambda self, *a, **k: touched.append("StreamResampler"))
    monkeypatch.setattr(TranscriptionServer, "process_wire_frames", lambda self, w: touched.append("process_wire_frames"))
    srv = running_server(single_model=True)
    for extra in ({}, dict(sample_rate=16000, channels=1, audio_format="int16")):
        c = ws.connect(f"ws://127.0.0.1:{srv.port}")
        c.send(json.dumps(dict(OPTS, **extra)))
        assert json.loads(c.recv(timeout=10.0))["message"] == "SERVER_READY"
        pcm = 0.1 * np.sin(np.arange(2 * 16000) * 0.05)
        c.send((pcm * 32767).astype(np.int16).tobytes() if extra else pcm.astype(np.float32).tobytes())
        assert json.loads(c.recv(timeout=10.0))["segments"]
        c.send(b"END_OF_AUDIO")
        with pytest.raises(ws.ConnectionClosed):
            for _ in range(200):
                c.recv(timeout=5.0)
        assert _wait(lambda: not srv.client_manager.clients)
    assert not touched and not srv.wire_sessions


@pytest.mark.parametrize("extra", [dict(sample_rate=44101), dict(channels=0), dict(channels=9), dict(sample_rate=8000, channels="2"),
                                   dict(audio_format="mulaw", sample_rate=7999)])
def test_unserved_wire_formats_get_the_error_message_and_are_closed(running_server, extra):
    srv = running_server(single_model=True)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, **extra)))
    msg = json.loads(c.recv(timeout=10.0))
    assert msg["uid"] == "u1" and msg["status"] == "ERROR" and "Unsupported" in msg["message"]
    with pytest.raises(ws.ConnectionClosed):
        c.recv(timeout=5.0)
    assert not srv.client_manager.clients and not srv.audio_formats and not srv.wire_sessions and not ServeClientHIP.MODELS


def test_a_packet_that_is_not_whole_frames_ends_the_session_with_an_error(running_server):
    srv = running_server(single_model=True)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, sample_rate=8000, channels=2, audio_format="alaw")))
    assert json.loads(c.recv(timeout=10.0))["message"] == "SERVER_READY"
    c.send(bytes(321))                                                             # 160 and a half stereo frames
    msg = json.loads(c.recv(timeout=10.0))
    assert msg["status"] == "ERROR" and "whole number" in msg["message"]
    with pytest.raises(ws.ConnectionClosed):
        for _ in range(50):
            c.recv(timeout=5.0)
    assert _wait(lambda: not srv.client_manager.clients) and not srv.wire_sessions
