"""GPU tests (-m gpu) of live multichannel sessions on a real engine (seeded peaked tiny.en weights): int16 48 kHz stereo with
different content per channel goes through a MultichannelSession as packets; each channel's segments — text and times, completed and
in progress — equal those of a mono wire-format session fed that channel alone with the same packet cutting; every message carries
its channel; with WLX_PCM_RING=0 the host route is taken and still yields per-channel segments.

The comparison drives the transcription loop's body from the test's thread at fixed points of the stream (the loop itself runs
whenever its thread is scheduled, which no two runs repeat); a last test lets the threads run and checks slots and teardown."""
import json
import time
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R

pytestmark = pytest.mark.gpu

RATE, SECONDS, PACKET = 48000, 5, 4096
STEP_EVERY = 18                                                                    # packets between two passes of the loop body (~1.5 s)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def hip(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    m = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab))
    yield m
    m.close()
    m.engine.close()


@pytest.fixture(scope="module")
def stereo():
    return np.ascontiguousarray(R.multichannel(SECONDS * RATE, RATE, 2, R.S16))    # another seed and gain per channel


def child_of(hip, sock, start_thread=False):
    from whisperlive_amd.serve_client import ServeClientHIP
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=hip, use_vad=False, same_output_threshold=1, no_speech_thresh=1.0,
                       start_thread=start_thread)
    if not start_thread:
        c._wake.set()                                                              # driven from the test: the loop's pauses end at once
    return c


def loop_body(c):
    """one pass of ServeClientBase.speech_to_text's body"""
    if c.frames_np is None:
        return
    chunk, duration = c.get_audio_chunk_for_processing()
    if duration < 1.0:
        return
    result = c.transcribe_audio(chunk.copy())
    if result is None or c.language is None:
        c.timestamp_offset += duration
        return
    c.handle_transcription_output(result, duration)


def drive(feed, sessions, x):
    """the stream in packets of PACKET frames; a pass of the loop body for every session every STEP_EVERY packets and four behind the flush"""
    for k, a in enumerate(range(0, x.shape[0], PACKET)):
        feed(x[a:a + PACKET].tobytes(), False)
        if k % STEP_EVERY == STEP_EVERY - 1:
            for c in sessions:
                loop_body(c)
    feed(b"", True)
    for _ in range(4):
        for c in sessions:
            loop_body(c)


def segment_messages(sock):
    return [json.loads(a[0][0]) for a in sock.send.call_args_list if "segments" in json.loads(a[0][0])]


@pytest.fixture(scope="module")
def mono_runs(hip, stereo):
    """per channel: a mono wire-format session fed that channel alone with the same cutting -> (session, its segment messages)"""
    out = []
    for c in range(2):
        sock = MagicMock()
        s = child_of(hip, sock)
        s.set_wire_format("int16", 1, RATE)
        col = np.ascontiguousarray(stereo[:, c])
        drive(lambda raw, fl, s=s: s.add_wire_frames(raw, fl), [s], col)
        assert s._ring, "the mono session ran on its device ring"
        s._ring.close()
        s._ring = False
        out.append((s, segment_messages(sock)))
    return out


def multichannel_run(hip, stereo):
    from whisperlive_amd.serve_client import MultichannelSession
    sock = MagicMock()
    sess = MultichannelSession(sock, "u", "int16", 2, RATE, lambda c, s: child_of(hip, s))
    drive(sess.add_wire_frames, sess.children, stereo)
    return sess, sock


def test_each_channel_equals_the_mono_session_fed_that_channel(hip, stereo, mono_runs, monkeypatch):
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    sess, sock = multichannel_run(hip, stereo)
    try:
        assert sess._group and all(ch._ring is sess._group.lane(c) for c, ch in enumerate(sess.children))     # the device route, to the end
        assert sess._group.state() == (0, SECONDS * 16000)
        msgs = [json.loads(a[0][0]) for a in sock.send.call_args_list]
        assert msgs[0] == {"uid": "u", "message": "SERVER_READY", "backend": "faster_whisper", "channels": 2}
        assert all(m["uid"] == "u" and m["channel"] in (0, 1) for m in msgs[1:])  # every message of a child carries its channel
        for c, (mono, mono_msgs) in enumerate(mono_runs):
            ch = sess.children[c]
            assert np.array_equal(bits(ch.frames_np), bits(mono.frames_np)), c
            assert (ch.frames_offset, ch.timestamp_offset) == (mono.frames_offset, mono.timestamp_offset), c
            got = [m for m in segment_messages(sock) if m["channel"] == c]
            print(f"channel {c}: {len(got)} segment messages, {len(ch.transcript)} completed segments, offset {ch.timestamp_offset:.3f}")
            assert len(got) >= 2 and len(ch.transcript) >= 1, c
            assert ch.transcript == mono.transcript and ch.text == mono.text, c   # completed segments: text and times
            assert [dict(m, channel=c) for m in mono_msgs] == got, c              # ... and everything sent on the way
        assert not np.array_equal(bits(sess.children[0].frames_np), bits(sess.children[1].frames_np))          # different content per channel
    finally:
        sess.cleanup()
    assert sess._released and sess._group is False and all(ch._ring is False for ch in sess.children)


def test_with_the_ring_switched_off_the_host_route_yields_per_channel_segments(hip, stereo, mono_runs, monkeypatch):
    monkeypatch.setenv("WLX_PCM_RING", "0")
    sess, sock = multichannel_run(hip, stereo)
    try:
        assert sess._group is False and all(ch._ring is False for ch in sess.children)
        for c, (mono, _) in enumerate(mono_runs):
            ch = sess.children[c]
            got = [m for m in segment_messages(sock) if m["channel"] == c]
            assert got and all(m["segments"] for m in got), c
            assert ch.frames_np.shape == mono.frames_np.shape
            err = float(np.abs(ch.frames_np.astype(np.float64) - mono.frames_np.astype(np.float64)).max())
            print(f"channel {c}: host route against the device route, max abs {err:.3e}")
            assert err <= R.RESAMPLE_ATOL                                          # the bound of the mono stream form's host half
    finally:
        sess.cleanup()


def test_threads_take_a_slot_each_and_a_disconnect_releases_everything(hip, stereo, monkeypatch):
    from whisperlive_amd.serve_client import MultichannelSession
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    sock = MagicMock()
    sess = MultichannelSession(sock, "u", "int16", 2, RATE, lambda c, s: child_of(hip, s, start_thread=True))
    x = stereo[:2 * RATE]
    for a in range(0, x.shape[0], PACKET):
        sess.add_wire_frames(x[a:a + PACKET].tobytes())
    group = sess._group
    assert group
    deadline = time.time() + 20
    while time.time() < deadline and {m["channel"] for m in segment_messages(sock)} != {0, 1}:
        time.sleep(0.02)
    assert {m["channel"] for m in segment_messages(sock)} == {0, 1}
    live = [s for s in hip._slots if s._owner is not None and s._owner.is_alive()]
    assert len({id(s) for s in live}) >= 2                                         # one engine slot per child thread
    sess.add_wire_frames(b"", flush=True)
    sess.cleanup()
    for ch in sess.children:
        ch.trans_thread.join(timeout=20)
        assert not ch.trans_thread.is_alive()
    assert sess._released and group._h is None and all(ch._ring is False for ch in sess.children)
