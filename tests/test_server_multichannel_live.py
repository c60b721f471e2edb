"""CPU tests of live MULTICHANNEL sessions (first message: multichannel true, channels >= 2): one socket fans out into one
ServeClientHIP per channel, every message carries its channel, the host route takes over from a failing ring group without a gap, the
refusals come at connection time, and sessions that do not ask for it never reach the new code. The engine is a fake."""
import json
import threading
import time
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests import resample_kernel_ref as R
from whisperlive_amd import serve_client as SC
from whisperlive_amd import stream_resample as SR
from whisperlive_amd import ws
from whisperlive_amd.serve_client import MultichannelSession, ServeClientBase, ServeClientHIP
from whisperlive_amd.server import TranscriptionServer


class RecordingTranscriber:
    """a fake engine: records the PCM it is handed, answers one segment over the whole chunk"""

    def __init__(self, engine=None):
        self.calls = []
        if engine is not None:
            self.engine = engine

    def transcribe(self, audio, **kw):
        self.calls.append(np.asarray(audio).copy())
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
STEREO = dict(multichannel=True, channels=2, sample_rate=48000, audio_format="int16")


def _wait(cond, seconds=10.0):
    deadline = time.time() + seconds
    while not cond() and time.time() < deadline:
        time.sleep(0.01)
    return cond()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stereo(n=24000, channels=2, rate=48000):
    return np.ascontiguousarray(R.multichannel(n, rate, channels, R.S16))


def cuttings(n):
    rng = np.random.default_rng(5)
    rand = np.sort(np.concatenate((rng.integers(0, n + 1, 12), [0, n])))
    return {"one_packet": [0, n], "short_packets": list(range(0, 40)) + list(range(40, n, 997)) + [n],
            "random_with_empty": np.sort(np.concatenate((rand, rand[::3]))).tolist()}


def per_channel_oracle(x, edges, name="int16", rate=48000):
    """one StreamResampler per channel over that channel's column, same cutting, then a flush"""
    out = []
    for c in range(x.shape[1]):
        r = SR.StreamResampler(name, 1, rate)
        parts = [r.feed(np.ascontiguousarray(x[a:b, c])) for a, b in zip(edges[:-1], edges[1:])] + [r.flush()]
        out.append(np.concatenate(parts))
    return out


def session(websocket=None, engine=None, channels=2, name="int16", rate=48000):
    websocket = websocket or MagicMock()

    def make_child(c, sock):
        return ServeClientHIP(sock, client_uid="u", model=None, transcriber=RecordingTranscriber(engine), use_vad=False, start_thread=False)
    return MultichannelSession(websocket, "u", name, channels, rate, make_child), websocket


# ------------------------------------------------------------------------------------------------ fan-out
@pytest.mark.parametrize("cut", ["one_packet", "short_packets", "random_with_empty"])
def test_each_child_gets_its_own_channel_resampled(cut):
    x = stereo(9000, channels=3)
    edges = cuttings(x.shape[0])[cut]
    s, sock = session(channels=3)
    assert json.loads(sock.send.call_args_list[0][0][0]) == {"uid": "u", "message": "SERVER_READY", "backend": "faster_whisper", "channels": 3}
    assert sock.send.call_count == 1                                               # the children's own SERVER_READY is not forwarded
    for a, b in zip(edges[:-1], edges[1:]):
        s.add_wire_frames(x[a:b].tobytes())
    before = [ch.frames_np.shape[0] for ch in s.children]
    assert before == [SR.stream_count(48000, x.shape[0])] * 3
    s.add_wire_frames(b"", flush=True)
    want = per_channel_oracle(x, edges)
    for c, ch in enumerate(s.children):
        assert ch._ring is False and s._group is False                             # no engine behind the transcriber: the host route
        assert ch.frames_np.shape[0] == 3000 and np.array_equal(bits(ch.frames_np), bits(want[c])), c
    assert not np.array_equal(bits(want[0]), bits(want[1]))
    n = s.children[0].frames_np.shape[0]
    s.add_wire_frames(x[:10].tobytes())                                            # after the flush the stream is closed
    assert s.children[0].frames_np.shape[0] == n
    with pytest.raises(ValueError):
        session(channels=1)
    s.cleanup()
    assert all(ch.exit for ch in s.children)


def test_every_message_of_a_child_carries_its_channel_and_the_sessions_uid():
    s, sock = session()
    sock.send.reset_mock()
    s.children[1].send_transcription_to_client([{"start": "0.000", "end": "1.000", "text": " a", "completed": True}])
    s.children[0].set_language(SimpleNamespace(language="de", language_probability=0.9))
    s.children[1].websocket.send(json.dumps({"uid": "u", "status": "WARNING", "message": "x"}))
    msgs = [json.loads(c[0][0]) for c in sock.send.call_args_list]
    assert [m["channel"] for m in msgs] == [1, 0, 1] and all(m["uid"] == "u" for m in msgs)
    assert msgs[0]["segments"][0]["text"] == " a" and msgs[1]["language"] == "de"
    s.disconnect()
    assert json.loads(sock.send.call_args_list[-1][0][0]) == {"uid": "u", "message": "DISCONNECT"}


def test_e2e_stereo_session_fans_out_and_end_of_audio_flushes(running_server):
    srv = running_server(single_model=True)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, **STEREO)))
    ready = json.loads(c.recv(timeout=10.0))
    assert ready["message"] == "SERVER_READY" and ready["channels"] == 2 and "channel" not in ready
    x = stereo(2 * 48000)                                                          # 2 s
    for i in range(0, x.shape[0], 4096):
        c.send(x[i: i + 4096].tobytes())
    assert _wait(lambda: len(srv.client_manager.clients) == 1)
    sess = next(iter(srv.client_manager.clients.values()))
    assert isinstance(sess, MultichannelSession) and srv.client_manager.slots_in_use() == 2
    assert _wait(lambda: all(ch.frames_np is not None and ch.frames_np.shape[0] == SR.stream_count(48000, x.shape[0]) for ch in sess.children))
    seen = set()
    for _ in range(40):
        msg = json.loads(c.recv(timeout=10.0))
        assert msg["uid"] == "u1" and msg["channel"] in (0, 1) and msg["segments"]
        seen.add(msg["channel"])
        if seen == {0, 1}:
            break
    assert seen == {0, 1}
    c.send(b"END_OF_AUDIO")
    deadline = time.time() + 30                                                    # (two fake engines answer at once: many messages)
    with pytest.raises(ws.ConnectionClosed):
        while time.time() < deadline:
            msg = c.recv(timeout=5.0)
            assert "channel" in json.loads(msg)
    assert _wait(lambda: not srv.client_manager.clients) and not srv.audio_formats and not srv.wire_sessions
    edges = list(range(0, x.shape[0], 4096)) + [x.shape[0]]
    want = per_channel_oracle(x, edges)
    for k, ch in enumerate(sess.children):
        assert sess._wire.closed and ch.frames_np.shape[0] == 32000 and np.array_equal(bits(ch.frames_np), bits(want[k]))
        assert ch.exit
    # each child handed ITS channel to the engine, from sample 0
    calls = ServeClientHIP.MODELS[0].calls
    heads = {bytes(bits(a[:16000])) for a in calls}
    assert {bytes(bits(w[:16000])) for w in want} <= heads


# ------------------------------------------------------------------------------------------------ the switch to the host route
class ScriptedGroup:
    """a ring group that computes on the host and fails at packet `fail_at`"""

    def __init__(self, name, channels, rate, fail_at):
        self.host, self.fail_at, self.calls, self.resident, self.closed = SR.ChannelStreamResamplers(name, channels, rate), fail_at, 0, 0, False
        self.lanes = [MagicMock() for _ in range(channels)]

    def lane(self, c):
        return self.lanes[c]

    def append_frames(self, raw, flush=False):
        self.calls += 1
        if self.calls - 1 == self.fail_at:
            raise RuntimeError("group lost")
        new = self.host.feed(raw, flush)
        self.resident += new[0].shape[0]
        return np.stack(new), 0, 0, self.resident

    def close(self):
        self.closed = True


@pytest.mark.parametrize("fail_at", [0, 1, 7, 25])
def test_host_route_takes_over_from_a_failing_group_without_a_gap_or_a_repeat(fail_at, monkeypatch):
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    x = stereo(30000)
    edges = list(range(0, x.shape[0], 1000)) + [x.shape[0]]
    made = []

    def create_ring_group(code, channels, rate):
        made.append(ScriptedGroup(SR._BY_CODE[code][0], channels, rate, fail_at))
        return made[-1]
    s, _ = session(engine=SimpleNamespace(create_ring_group=create_ring_group))
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        s.add_wire_frames(x[a:b].tobytes())
        if k < fail_at:
            assert s._group is made[0] and all(ch._ring is made[0].lanes[c] for c, ch in enumerate(s.children))
    s.add_wire_frames(b"", flush=True)
    assert len(made) == 1 and made[0].calls == fail_at + 1 and s._group is False and all(ch._ring is False for ch in s.children)
    all_host, _ = session()
    for a, b in zip(edges[:-1], edges[1:]):
        all_host.add_wire_frames(x[a:b].tobytes())
    all_host.add_wire_frames(b"", flush=True)
    for ch, ref in zip(s.children, all_host.children):
        assert ch.frames_np.shape[0] == 10000 and np.array_equal(bits(ch.frames_np), bits(ref.frames_np))
    for lane in made[0].lanes:
        lane.close.assert_called()
    assert not made[0].closed                                                      # the group itself goes behind the last child's thread
    s.cleanup()
    assert made[0].closed


def test_a_healthy_group_is_used_for_every_packet_and_no_ring_with_the_switch_off(monkeypatch):
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    x = stereo(8000)
    made = []

    def create_ring_group(code, channels, rate):
        made.append(ScriptedGroup(SR._BY_CODE[code][0], channels, rate, -1))
        return made[-1]
    eng = SimpleNamespace(create_ring_group=create_ring_group)
    s, _ = session(engine=eng)
    for a in range(0, 8000, 1000):
        s.add_wire_frames(x[a:a + 1000].tobytes())
    s.add_wire_frames(b"", flush=True)
    assert made[0].calls == 9 and s._wire.J == 8000 == made[0].host.J and s._wire.M == made[0].host.M    # the host states kept in step
    want = per_channel_oracle(x, list(range(0, 8001, 1000)))
    for c, ch in enumerate(s.children):
        assert ch._ring is made[0].lanes[c] and np.array_equal(bits(ch.frames_np), bits(want[c]))
    s.cleanup()
    assert made[0].closed and all(ch._ring is False for ch in s.children)
    monkeypatch.setenv("WLX_PCM_RING", "0")
    s, _ = session(engine=eng)
    s.add_wire_frames(x[:1000].tobytes())
    assert len(made) == 1 and s._group is False


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("extra,word", [
    (dict(STEREO, channels=1), "channels >= 2"),
    (dict(multichannel=True, sample_rate=48000, audio_format="int16"), "channels >= 2"),
    (dict(STEREO, channels="2"), "channels >= 2"),
    (dict(STEREO, channels=9), "Unsupported channels"),
    (dict(STEREO, sample_rate=44101), "Unsupported sample_rate"),
    (dict(STEREO, audio_format="opus"), "Unsupported audio_format"),
    (dict(STEREO, channels=3), "free slots"),
    (dict(STEREO, enable_diarization=True), "enable_diarization"),
    (dict(STEREO, enable_translation=True), "enable_translation"),
])
def test_connection_time_refusals_get_the_error_message_and_a_closed_socket(running_server, extra, word):
    srv = running_server(single_model=True, max_clients=2)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, **extra)))
    msg = json.loads(c.recv(timeout=10.0))
    assert msg["uid"] == "u1" and msg["status"] == "ERROR" and word in msg["message"], msg
    with pytest.raises(ws.ConnectionClosed):
        c.recv(timeout=5.0)
    assert not srv.client_manager.clients and not srv.audio_formats and not srv.wire_sessions and not ServeClientHIP.MODELS


def test_a_multichannel_session_counts_one_slot_per_channel(running_server):
    srv = running_server(single_model=True, max_clients=3)
    a = ws.connect(f"ws://127.0.0.1:{srv.port}")
    a.send(json.dumps(dict(OPTS, **STEREO)))
    assert json.loads(a.recv(timeout=10.0))["message"] == "SERVER_READY"
    assert _wait(lambda: srv.client_manager.free_slots() == 1)
    b = ws.connect(f"ws://127.0.0.1:{srv.port}")
    b.send(json.dumps(dict(OPTS, uid="u2", **STEREO)))                             # two channels, one free slot
    msg = json.loads(b.recv(timeout=10.0))
    assert msg["uid"] == "u2" and msg["status"] == "ERROR" and "free slots" in msg["message"]
    d = ws.connect(f"ws://127.0.0.1:{srv.port}")
    d.send(json.dumps(dict(OPTS, uid="u3")))                                       # a plain session still fits
    assert json.loads(d.recv(timeout=10.0))["message"] == "SERVER_READY"
    assert _wait(lambda: srv.client_manager.free_slots() == 0)
    e = ws.connect(f"ws://127.0.0.1:{srv.port}")
    e.send(json.dumps(dict(OPTS, uid="u4")))                                       # ... and then the server is full
    assert json.loads(e.recv(timeout=10.0))["status"] == "WAIT"
    a.send(b"END_OF_AUDIO")
    assert _wait(lambda: srv.client_manager.free_slots() == 2)                     # a disconnect gives every channel's slot back


def test_a_packet_that_is_not_whole_frames_is_refused_when_it_arrives(running_server):
    srv = running_server(single_model=True)
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(dict(OPTS, **STEREO)))
    assert json.loads(c.recv(timeout=10.0))["message"] == "SERVER_READY"
    c.send(bytes(4 * 100 + 2))                                                     # 100 and a half stereo int16 frames
    msg = json.loads(c.recv(timeout=10.0))
    assert msg["status"] == "ERROR" and "whole number" in msg["message"]
    until = time.time() + 30
    with pytest.raises(ws.ConnectionClosed):
        while time.time() < until:
            c.recv(timeout=5.0)
    assert _wait(lambda: not srv.client_manager.clients) and not srv.wire_sessions


# ------------------------------------------------------------------------------------------------ everyone else
def test_sessions_without_multichannel_take_the_routes_they_took(running_server, monkeypatch):
    touched, reached = [], []
    monkeypatch.setattr(TranscriptionServer, "open_multichannel", lambda self, *a, **k: touched.append("open_multichannel"))
    monkeypatch.setattr(MultichannelSession, "__init__", lambda self, *a, **k: touched.append("MultichannelSession"))
    monkeypatch.setattr(SR.ChannelStreamResamplers, "__init__", lambda self, *a, **k: touched.append("ChannelStreamResamplers"))
    monkeypatch.setattr(SC._ChannelSocket, "__init__", lambda self, *a, **k: touched.append("_ChannelSocket"))
    monkeypatch.setattr(ServeClientBase, "take_wire_samples", lambda self, *a, **k: touched.append("take_wire_samples"))
    for name in ("add_frames", "add_wire_frames"):
        inner = getattr(ServeClientBase, name)

        def wrapped(self, *a, _inner=inner, _name=name, **k):
            reached.append((_name, type(self).__name__))
            return _inner(self, *a, **k)
        monkeypatch.setattr(ServeClientBase, name, wrapped)
    groups = []
    eng = SimpleNamespace(create_ring_group=lambda *a, **k: groups.append(a))
    srv = running_server(single_model=True, model_factory=lambda model, dev: RecordingTranscriber(eng))
    cases = ({}, dict(multichannel=False), dict(multichannel=False, **{k: v for k, v in STEREO.items() if k != "multichannel"}),
             dict(sample_rate=8000, audio_format="mulaw"), dict(multichannel="true"))
    for extra in cases:
        wire = "sample_rate" in extra
        c = ws.connect(f"ws://127.0.0.1:{srv.port}")
        c.send(json.dumps(dict(OPTS, **extra)))
        assert json.loads(c.recv(timeout=10.0)) == {"uid": "u1", "message": "SERVER_READY", "backend": "faster_whisper"}
        if not wire:
            c.send((0.1 * np.sin(np.arange(2 * 16000) * 0.05)).astype(np.float32).tobytes())
        elif extra.get("channels") == 2:
            c.send(stereo(2 * 48000).tobytes())
        else:
            c.send(bytes(2 * 8000))
        msg = json.loads(c.recv(timeout=10.0))
        assert msg["segments"] and "channel" not in msg
        assert _wait(lambda: len(srv.client_manager.clients) == 1)
        client = next(iter(srv.client_manager.clients.values()))
        assert type(client) is ServeClientHIP and (client._wire is not None) == wire
        c.send(b"END_OF_AUDIO")
        until = time.time() + 30
        with pytest.raises(ws.ConnectionClosed):
            while time.time() < until:
                c.recv(timeout=5.0)
        assert _wait(lambda: not srv.client_manager.clients)
    assert not touched and not groups
    data = [r for r in reached]
    assert [n for n, _ in data if n == "add_frames"] == ["add_frames"] * 3
    # a wire session: one data packet, then the flush of END_OF_AUDIO
    assert [n for n, _ in data if n == "add_wire_frames"] == ["add_wire_frames"] * 4
    assert all(t == "ServeClientHIP" for _, t in data)
