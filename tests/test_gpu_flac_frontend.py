"""GPU: the FLAC front end on the product path (Slot.put_flac, transcribe(file), BatchedInferencePipeline.transcribe(file)): what it
leaves resident is BIT-IDENTICAL to put_frames(read_flac(file)), so everything behind it computes what it computed before."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

from . import flac_writer as W

pytestmark = pytest.mark.gpu

JFK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_head.flac")


@pytest.fixture(scope="module")
def engine(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7), device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def jfk():
    from whisperlive_amd import audio_io
    with open(JFK, "rb") as f:
        data = f.read()
    frames, rate = audio_io.read_flac(data)
    return data, frames, rate


def _synthetic(rate, ch, n, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    x = np.sin(6.2831853 * t * rng.uniform(200, 900, size=(1, ch)) / rate) * 9000 + rng.randint(-300, 300, size=(n, ch))
    pcm = np.round(x).astype(np.int64)
    return W.encode_stream(pcm, rate, 16, W.split_blocks(n, 1152), subframe={"type": "fixed", "order": 2, "k": 9},
                           assignment=W.MID_SIDE if ch == 2 else W.INDEPENDENT)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _both(engine, data, frames, rate):
    """-> (pcm, features) after put_flac and after put_frames(read_flac), each on a slot of its own"""
    out = []
    for route in ("flac", "frames"):
        s = engine.create_slot(1, 5)
        try:
            if route == "flac":
                n, info = s.put_flac(data)
                assert (info.sample_rate, info.channels, info.total_samples, info.served) == (rate, frames.shape[1], frames.shape[0], 1)
            else:
                n = s.put_frames(frames, rate)
            pcm = s.pcm()
            assert pcm.shape[0] == n
            s.logmel_resident()
            out.append((pcm, s.features()))
        finally:
            s.close()
    return out


def test_put_flac_of_a_real_file_is_bit_identical_to_put_frames_of_read_flac(engine, jfk):
    data, frames, rate = jfk
    (a, fa), (b, fb) = _both(engine, data, frames, rate)
    assert a.shape == b.shape == (53499,) and np.array_equal(_bits(a), _bits(b))                 # 44.1 kHz stereo: resampled
    assert fa.shape == fb.shape and np.array_equal(_bits(fa), _bits(fb))                         # ... and logmel_resident after it


@pytest.mark.parametrize("rate,ch,n", [(16000, 1, 9000), (8000, 2, 7001)], ids=["16k_mono_copy", "8k_stereo_upsample"])
def test_put_flac_of_synthetic_streams_is_bit_identical(engine, rate, ch, n):
    from whisperlive_amd import audio_io
    data = _synthetic(rate, ch, n, seed=rate + ch)
    frames, sr = audio_io.read_flac(data)
    assert sr == rate and frames.shape == (n, ch)
    (a, fa), (b, fb) = _both(engine, data, frames, rate)
    assert a.shape == b.shape == (n * 16000 // rate if (n * 16000) % rate == 0 else n * 16000 // rate + 1,)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(fa), _bits(fb))


def _put_flac_rc(engine, s, data):
    from whisperlive_amd import _lib
    n = C.c_int64(-1)
    info = _lib.wlx_flac_info()
    return engine.lib.wlx_pcm_put_flac(engine._h, s.sid, 0, data, len(data), C.byref(info), C.byref(n)), n.value


def test_refused_and_damaged_streams_leave_the_resident_pcm_alone(engine):
    from whisperlive_amd import _lib
    s = engine.create_slot(1, 5)
    try:
        before = np.linspace(-1, 1, 5000, dtype=np.float32)
        s.pcm_put(before)
        rng = np.random.RandomState(2)
        wide = W.encode_stream(rng.randint(-(1 << 31), 1 << 31, size=(300, 2)).astype(np.int64), 16000, 32, [200, 100])
        rc, n = _put_flac_rc(engine, s, wide)
        assert rc == _lib.ERR_ARG and n == -1                              # a 32-bit stream: refused, nothing launched
        assert np.array_equal(_bits(s.pcm()), _bits(before))
        good = bytearray(_synthetic(16000, 1, 3000, seed=4))
        good[len(good) // 2] ^= 0x20                                       # a frame body byte: the HOST index finds the CRC-16 wrong
        rc, n = _put_flac_rc(engine, s, bytes(good))
        assert rc == _lib.ERR_DATA and n == -1
        assert np.array_equal(_bits(s.pcm()), _bits(before))
        with pytest.raises(_lib.WlxError) as ei:
            s.put_flac(bytes(good))
        assert ei.value.code == _lib.ERR_DATA
    finally:
        s.close()


def test_a_second_larger_put_flac_on_the_same_slot_grows_the_scratch(engine, jfk):
    from whisperlive_amd import audio_io
    data, frames, rate = jfk
    small = _synthetic(16000, 1, 2000, seed=9)
    s = engine.create_slot(1, 5)
    ref = engine.create_slot(1, 5)
    try:
        n0, _ = s.put_flac(small)
        assert n0 == 2000
        n1, _ = s.put_flac(data)
        ref.put_frames(frames, rate)
        assert n1 == 53499 and np.array_equal(_bits(s.pcm()), _bits(ref.pcm()))
        n2, _ = s.put_flac(small)                                          # ... and a smaller one after it
        ref.put_frames(audio_io.read_flac(small)[0], 16000)
        assert n2 == 2000 and np.array_equal(_bits(s.pcm()), _bits(ref.pcm()))
    finally:
        s.close()
        ref.close()


@pytest.fixture(scope="module")
def peaked(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=2)
    yield hip
    hip.close()
    hip.engine.close()


KW = dict(language="en", temperature=0.0, max_new_tokens=24, vad_filter=False, compression_ratio_threshold=None,
          log_prob_threshold=None, no_speech_threshold=None)


def _without_put_flac(monkeypatch):
    """the route of before: read_flac on the host, put_frames on the device"""
    from whisperlive_amd import engine as E
    monkeypatch.setattr(E.Slot, "put_flac", property(), raising=True)


def test_transcribe_of_a_flac_file_equals_the_put_frames_route(peaked, jfk, monkeypatch):
    from whisperlive_amd import engine as E
    calls = []
    real = E.Slot.put_flac
    monkeypatch.setattr(E.Slot, "put_flac", lambda self, data, item=0: (calls.append(len(data)), real(self, data, item))[1])
    a, ai = peaked.transcribe(JFK, **KW)
    a = list(a)
    na = peaked.resident_file_audio().n_samples
    assert calls == [len(jfk[0])]
    _without_put_flac(monkeypatch)
    b, bi = peaked.transcribe(JFK, **KW)
    b = list(b)
    assert a and [(s.tokens, s.seek, s.start, s.end) for s in a] == [(s.tokens, s.seek, s.start, s.end) for s in b]
    assert ai.duration == bi.duration and na == peaked.resident_file_audio().n_samples == 53499


def test_batched_transcribe_of_flac_bytes_equals_the_put_frames_route(peaked, jfk, monkeypatch):
    from whisperlive_amd.batched import BatchedInferencePipeline
    data = jfk[0]
    kw = dict(language="en", clip_timestamps=[{"start": 0, "end": 25000}, {"start": 26000, "end": 53000}], chunk_length=2, vad_filter=False,
              batch_size=2)
    p = BatchedInferencePipeline(peaked)
    a, ai = p.transcribe(data, **kw)
    a = list(a)
    na = peaked.resident_file_audio().n_samples
    _without_put_flac(monkeypatch)
    b, bi = p.transcribe(data, **{**kw, "clip_timestamps": [dict(c) for c in kw["clip_timestamps"]]})
    b = list(b)
    assert len(a) == 2 and [(s.tokens, s.seek, s.start, s.end) for s in a] == [(s.tokens, s.seek, s.start, s.end) for s in b]
    assert ai.duration == bi.duration and na == peaked.resident_file_audio().n_samples == 53499
