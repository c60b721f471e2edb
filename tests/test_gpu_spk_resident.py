"""GPU tests (-m gpu) of speaker embedding on device-resident audio: wlx_spk_embed_pcm_batch on ranges of a slot item's PCM and
wlx_spk_embed_ring_batch on absolute positions of a PCM ring, each row against the upload of the same samples as a batch of one
(wlx_spk_embed), bit for bit: a row depends neither on where its samples lie nor on the other rows; the refusals, a concurrent
ring writer, and the file endpoint's labelling helper on the audio a transcription left resident."""
from __future__ import annotations

import ctypes as C
import io
import threading
import wave
from types import SimpleNamespace

import numpy as np
import pytest

from tests import helpers as H
from whisperlive_amd import _lib, spk_weights
from whisperlive_amd.diarization import SpeakerDiarizer, SpeakerEmbedderHIP
from whisperlive_amd.engine import ResidentPcm

from .test_gpu_diarization import SPEC, WEIGHT_SEED, _widest_gap_threshold

pytestmark = pytest.mark.gpu

E = SPEC.embed_dim
N = 6 * 16000                # samples resident in the slot
SENTINEL = 7.0
# (start, n): the shortest range; an odd start with one sample short of another frame; a range twice; one overlapping it; one that ends
# exactly at the resident count
RANGES = [(0, 4800), (37, 4800 + 159), (1000, 16000), (1000, 16000), (8000, 20000), (N - 30000, 30000)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def spk():
    w = spk_weights.fold(spk_weights.random_weights(SPEC, seed=WEIGHT_SEED), SPEC)
    e = SpeakerEmbedderHIP(SPEC, w, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


@pytest.fixture(scope="module")
def noise():
    return (np.random.default_rng(2024).standard_normal(N) * 0.1).astype(np.float32)


@pytest.fixture(scope="module")
def slot(eng, noise):
    s = eng.create_slot(2, 5)
    s.pcm_put(noise)                 # item 0; item 1 holds nothing
    yield s
    s.close()


@pytest.fixture(scope="module")
def alone(spk, slot):
    """wlx_spk_embed of every range of RANGES on the samples wlx_pcm_get returns, computed once before any resident call"""
    pcm = slot.pcm()
    assert pcm.shape[0] == N
    return {r: spk.embed(pcm[r[0]:r[0] + r[1]]) for r in set(RANGES)}


def raw_pcm(spk, slot, item, ranges, n=None, out=None, status=None):
    """-> (rc, out, status) of one wlx_spk_embed_pcm_batch call; out / status prefilled with the sentinels unless given"""
    starts = np.array([a for a, _ in ranges], dtype=np.int64)
    counts = np.array([c for _, c in ranges], dtype=np.int64)
    n = len(ranges) if n is None else n
    rows = max(len(ranges), n, 1)
    out = np.full((rows, E), SENTINEL, np.float32) if out is None else out
    status = np.full(rows, -1, np.int32) if status is None else status
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    rc = spk.lib.wlx_spk_embed_pcm_batch(spk.h, slot.engine._h, slot.sid, item, starts.ctypes.data_as(i64p), counts.ctypes.data_as(i64p), n,
                                         out.ctypes.data_as(f32p), status.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, status


def raw_ring(spk, ring, ranges):
    starts = np.array([a for a, _ in ranges], dtype=np.int64)
    counts = np.array([c for _, c in ranges], dtype=np.int64)
    out, status = np.full((len(ranges), E), SENTINEL, np.float32), np.full(len(ranges), -1, np.int32)
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    rc = spk.lib.wlx_spk_embed_ring_batch(spk.h, ring._h, starts.ctypes.data_as(i64p), counts.ctypes.data_as(i64p), len(ranges),
                                          out.ctypes.data_as(f32p), status.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, status


def test_slot_rows_equal_single_embeds(spk, slot, alone):
    rc, out, st = raw_pcm(spk, slot, 0, RANGES)
    assert rc == 0 and (st == 0).all()
    for i, r in enumerate(RANGES):
        assert (_bits(out[i]) == _bits(alone[r])).all(), f"range {r} differs from wlx_spk_embed on the same samples"
    fb, nn = spk.timings()                                    # this pass was the last one
    assert fb > 0 and nn > 0
    # the same ranges in reversed order: the same rows
    rc, rev, st = raw_pcm(spk, slot, 0, RANGES[::-1])
    assert rc == 0 and (st == 0).all() and (_bits(rev[::-1]) == _bits(out)).all()
    # the resident audio was only read
    assert np.array_equal(slot.pcm(), slot.pcm()) and slot.pcm_count() == N
    # the Python face: one embedding per range, the same bits
    got = spk.embed_resident(slot, 0, RANGES + [(5, 100)])
    assert got[-1] is None and all((_bits(g) == _bits(alone[r])).all() for g, r in zip(got, RANGES))


def test_short_ranges(spk, slot, alone):
    ranges = [RANGES[2], (0, 4799), RANGES[4]]
    rc, out, st = raw_pcm(spk, slot, 0, ranges)
    assert rc == 0 and st.tolist() == [0, _lib.ERR_TOO_SHORT, 0]
    assert (out[1] == 0).all() and (_bits(out[0]) == _bits(alone[ranges[0]])).all() and (_bits(out[2]) == _bits(alone[ranges[2]])).all()
    before = spk.timings()
    rc, out, st = raw_pcm(spk, slot, 0, [(0, 4799), (N - 10, 10), (N, 0)])
    assert rc == 0 and (st == _lib.ERR_TOO_SHORT).all() and (out == 0).all()
    assert spk.timings() == before                            # nothing was launched


def test_slot_refusals_write_nothing(spk, slot, alone):
    cap = SPEC.max_seconds * 16000
    assert 8 * N > cap >= N
    cases = [
        ("one sample past the resident count", 0, [(N - 4800 + 1, 4800)], None, _lib.ERR_STATE),
        ("no PCM resident in the item", 1, [(0, 4800)], None, _lib.ERR_STATE),
        ("item outside the slot", 2, [(0, 4800)], None, _lib.ERR_ARG),
        ("negative item", -1, [(0, 4800)], None, _lib.ERR_ARG),
        ("sum over max_seconds", 0, [(0, N)] * 8, None, _lib.ERR_ARG),
        ("negative start", 0, [(0, 4800), (-1, 4800)], None, _lib.ERR_ARG),
        ("negative count", 0, [(0, -1)], None, _lib.ERR_ARG),
        ("n = 0", 0, [(0, 4800)], 0, _lib.ERR_ARG),
        ("n = 65", 0, [(0, 4800)] * 65, 65, _lib.ERR_ARG),
        ("a start that would overflow", 0, [(2 ** 63 - 1, 4800)], None, _lib.ERR_STATE),
    ]
    for what, item, ranges, n, want in cases:
        rc, out, st = raw_pcm(spk, slot, item, ranges, n=n)
        assert rc == want, (what, rc)
        assert (out == SENTINEL).all() and (st == -1).all(), what
    # null pointers
    f32p, i64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    a, c = np.array([0], np.int64), np.array([4800], np.int64)
    out, st = np.full((1, E), SENTINEL, np.float32), np.full(1, -1, np.int32)
    full = [spk.h, slot.engine._h, slot.sid, 0, a.ctypes.data_as(i64p), c.ctypes.data_as(i64p), 1, out.ctypes.data_as(f32p), st.ctypes.data_as(i32p)]
    for k in (0, 1, 4, 5, 7, 8):
        args = list(full)
        args[k] = None
        assert spk.lib.wlx_spk_embed_pcm_batch(*args) == _lib.ERR_ARG, k
        assert (out == SENTINEL).all() and (st == -1).all()
    # the engine still works, and so does the slot
    rc, out, st = raw_pcm(spk, slot, 0, RANGES[:3])
    assert rc == 0 and all((_bits(out[i]) == _bits(alone[r])).all() for i, r in enumerate(RANGES[:3]))


def test_after_the_device_resampler(spk, eng):
    """frames at 44.1 kHz stereo S16 through wlx_pcm_put_frames, embedded right behind it (the engine's stream waits for the slot's)"""
    rng = np.random.default_rng(5)
    frames = np.clip(rng.standard_normal((44100 * 2, 2)) * 6000, -32768, 32767).astype(np.int16)
    s = eng.create_slot(1, 5)
    try:
        n = s.put_frames(frames, 44100)
        assert 31000 < n < 33000
        ranges = [(0, 4800), (11, 20000), (n - 9000, 9000)]
        rc, out, st = raw_pcm(spk, s, 0, ranges)
        assert rc == 0 and (st == 0).all()
        pcm = s.pcm()
        for i, (a, c) in enumerate(ranges):
            assert (_bits(out[i]) == _bits(spk.embed(pcm[a:a + c]))).all(), (a, c)
    finally:
        s.close()


def test_ring_rows_equal_single_embeds(spk, eng):
    rng = np.random.default_rng(6)
    ring = eng.create_ring()
    try:
        host = (rng.standard_normal(48000) * 0.1).astype(np.float32)
        assert ring.append(host, max_resident=40000, trim=16000) == (0, 0, 48000)
        more = (rng.standard_normal(8000) * 0.1).astype(np.float32)
        dropped, base, resident = ring.append(more, max_resident=40000, trim=16000)       # over the cap: one trim
        assert (dropped, base, resident) == (16000, 16000, 40000)
        host = np.concatenate([host, more])                # host[p] = stream position p
        # the first resident sample, a range across the old end of the buffer (where the appended packet begins), the last sample
        ranges = [(16000, 4800), (16001, 9000), (44000, 10000), (56000 - 4800, 4800), (20000, 4799)]
        rc, out, st = raw_ring(spk, ring, ranges)
        assert rc == 0 and st.tolist() == [0, 0, 0, 0, _lib.ERR_TOO_SHORT] and (out[4] == 0).all()
        for i, (a, c) in enumerate(ranges[:4]):
            assert (_bits(out[i]) == _bits(spk.embed(host[a:a + c]))).all(), (a, c)
        got = spk.embed_ring(ring, ranges)
        assert got[4] is None and all((_bits(g) == _bits(out[i])).all() for i, g in enumerate(got[:4]))
        for what, bad in (("starts below base", [(15999, 4800)]), ("ends past the resident end", [(56000 - 4800 + 1, 4800)]),
                          ("trimmed away entirely", [(0, 4800)])):
            rc, out, st = raw_ring(spk, ring, [ranges[0]] + bad)
            assert rc == _lib.ERR_STATE, what
            assert (out == SENTINEL).all() and (st == -1).all(), what
        rc, out, st = raw_ring(spk, ring, [(-1, 4800)])
        assert rc == _lib.ERR_ARG and (out == SENTINEL).all()
        assert ring.state() == (16000, 40000)
    finally:
        ring.close()


def test_ring_reader_against_a_concurrent_writer(spk, eng):
    """a second thread appends (no trim) while this one embeds ranges that were resident before it started"""
    rng = np.random.default_rng(8)
    ring = eng.create_ring(capacity_samples=64000)            # the appends outgrow it: the buffer is re-allocated under the reader's feet
    errs = []
    try:
        host = (rng.standard_normal(32000) * 0.1).astype(np.float32)
        ring.append(host, max_resident=0)
        ranges = [(0, 4800), (3000, 12000), (32000 - 8000, 8000)]
        want = [spk.embed(host[a:a + c]) for a, c in ranges]
        packets = [(rng.standard_normal(4096) * 0.1).astype(np.float32) for _ in range(24)]

        def writer():
            try:
                for p in packets:
                    ring.append(p, max_resident=0)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = threading.Thread(target=writer)
        th.start()
        rounds = 0
        while rounds < 3 or (th.is_alive() and rounds < 50):
            rc, out, st = raw_ring(spk, ring, ranges)
            assert rc == 0 and (st == 0).all()
            assert all((_bits(out[i]) == _bits(w)).all() for i, w in enumerate(want)), rounds
            rounds += 1
        th.join(30)
        assert not th.is_alive() and not errs, errs
        assert ring.state() == (0, 32000 + 24 * 4096)
    finally:
        ring.close()


def _coloured(kind, n, seed):
    x = np.random.default_rng(seed).standard_normal(n + 64)
    if kind:                                                  # the second "speaker": low-passed and gated at 7 Hz
        x = np.convolve(x, np.ones(24) / 24.0, mode="same") * 4.0 * (0.6 + 0.4 * np.sign(np.sin(2 * np.pi * 7.0 * np.arange(n + 64) / 32000.0)))
    return (0.1 * x[:n]).astype(np.float32)


def test_file_labels_come_from_the_resident_audio(spk, eng, monkeypatch):
    """a file through WhisperModelHIP.transcribe, then speaker_labels_for_segments on what it left in the slot: the labels of
    identify_speakers on the wlx_pcm_get slices, the file not decoded again"""
    from whisperlive_amd import audio_io, rest
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    piece = 48000                                             # 1.5 s per turn at 32 kHz, two noise colours alternating
    pcm32k = np.concatenate([_coloured(i % 2, piece, 70 + i) for i in range(6)])
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(32000)
        w.writeframes((np.clip(pcm32k, -1, 1) * 32767).astype(np.int16).tobytes())
    data = buf.getvalue()
    calls = []
    real_load = audio_io.load_audio
    monkeypatch.setattr(audio_io, "load_audio", lambda *a, **k: (calls.append(1), real_load(*a, **k))[1])
    m = WhisperModelHIP("rand", engine=eng, hf_tokenizer=synthetic_tokenizer(H.TINY_EN.vocab))
    try:
        segs, _info = m.transcribe(data, language="en", temperature=0.0, max_new_tokens=4, vad_filter=False)
        list(segs or [])
        handle = m.resident_file_audio()
        assert isinstance(handle, ResidentPcm) and handle.item == 0 and abs(handle.n_samples - 9 * 16000) <= 1
        host = handle.slot.pcm()
        assert host.shape[0] == handle.n_samples
        # one segment per turn, one too short, one empty, one past the file
        spans = [(i * 1.5, (i + 1) * 1.5) for i in range(6)] + [(1.0, 1.2), (2.0, 2.0), (9.5, 10.0)]
        segments = [SimpleNamespace(start=a, end=b) for a, b in spans]
        slices = [host[int(a * 16000):min(len(host), int(b * 16000))] for a, b in spans[:7]]
        thr, _ = _widest_gap_threshold([spk.embed(s) for s in slices[:6]])
        want = SpeakerDiarizer(similarity_threshold=thr, embedder=spk).identify_speakers(slices)
        print("labels on the host slices:", want)
        assert want[6] is None and all(want[:6])
        dev = SpeakerDiarizer(similarity_threshold=thr, embedder=spk)
        got = rest.speaker_labels_for_segments(segments, lambda: audio_io.load_audio(data), dev, resident=handle)
        assert got == {i: lab for i, lab in enumerate(want) if lab}
        assert not calls, "the file was decoded again for labelling"
        # without the handle the same call decodes the file (today's route)
        again = SpeakerDiarizer(similarity_threshold=thr, embedder=spk)
        rest.speaker_labels_for_segments(segments, lambda: audio_io.load_audio(data), again, resident=None)
        assert len(calls) == 1
        m.release_slot()
        assert m.resident_file_audio() is None               # a released slot may be refilled by another request
    finally:
        m.close()
