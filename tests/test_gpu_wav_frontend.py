"""GPU: the telephony WAV front end on the product path (Slot.put_wav / put_wav_split, transcribe(file), multichannel=True): what it leaves
resident is BIT-IDENTICAL to put_frames(read_wav(file)), so everything behind it computes what it computed before."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

from . import wav_writer as W

pytestmark = pytest.mark.gpu

JFK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_16k.npz")
TAGS = {"mulaw": W.TAG_MULAW, "alaw": W.TAG_ALAW, "ima": W.TAG_IMA, "ms": W.TAG_MS}


@pytest.fixture(scope="module")
def engine(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7), device=0)
    yield eng
    eng.close()


def _file(kind, rate, ch, seconds, seed=0, **kw):
    """a file of about `seconds`: G.711 of speech-like audio; ADPCM of seeded random nibbles (every clamp, no slow encoder)"""
    n = int(rate * seconds) + 3
    if kind in ("mulaw", "alaw"):
        return W.write_g711(W.speech_like(n, ch, seed=seed, rate=rate), rate, TAGS[kind], extensible=(kind == "alaw"))
    ba = 256 * ch
    spb = (W.ima_samples_per_block if kind == "ima" else W.ms_samples_per_block)(ba, ch)
    return W.random_adpcm(TAGS[kind], n // spb + 1, ch, ba, rate=rate, seed=seed, **kw)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("rate,seconds", [(8000, 3), (11025, 1), (16000, 2), (44100, 1)])
@pytest.mark.parametrize("kind", sorted(TAGS))
def test_put_wav_is_bit_identical_to_put_frames_of_read_wav_mono_mix_and_split(engine, kind, rate, seconds):
    from whisperlive_amd import audio_io
    data = _file(kind, rate, 2, seconds, seed=rate % 97)
    frames, sr = audio_io.read_wav(data)
    assert sr == rate and frames.shape[1] == 2
    s = engine.create_slot(3, 5)
    ref = engine.create_slot(1, 5)
    try:
        n, info = s.put_wav(data)
        assert (info.sample_rate, info.channels, info.n_frames, info.served) == (rate, 2, frames.shape[0], 1)
        assert n == ref.put_frames(frames, rate)
        mix = s.pcm()
        assert mix.shape[0] == n and np.array_equal(_bits(mix), _bits(ref.pcm()))
        s.logmel_resident()
        ref.logmel_resident()
        assert np.array_equal(_bits(s.features()), _bits(ref.features()))                      # ... and logmel_resident after it
        n2, _ = s.put_wav_split(data, 1)
        for c in range(2):
            assert ref.put_frames(np.ascontiguousarray(frames[:, c:c + 1]), rate) == n2
            assert np.array_equal(_bits(s.pcm(1 + c)), _bits(ref.pcm()))
        assert np.array_equal(_bits(s.pcm(0)), _bits(mix))                                     # item 0 is not one of the split's
    finally:
        s.close()
        ref.close()


@pytest.mark.parametrize("kind", ["ima", "ms"])
def test_a_file_cut_by_fact_inside_a_block(engine, kind):
    from whisperlive_amd import audio_io
    data = _file(kind, 8000, 1, 1, seed=3, fact=7777, partial=100)
    frames, _ = audio_io.read_wav(data)
    assert frames.shape == (7777, 1)
    s = engine.create_slot(1, 5)
    ref = engine.create_slot(1, 5)
    try:
        n, info = s.put_wav(data)
        assert info.n_frames == 7777 and n == ref.put_frames(frames, 8000) == 15554
        assert np.array_equal(_bits(s.pcm()), _bits(ref.pcm()))
    finally:
        s.close()
        ref.close()


def _put_wav_rc(engine, slot, data, split=False):
    from whisperlive_amd import _lib
    n = C.c_int64(-1)
    fn = slot.lib.wlx_pcm_put_wav_split if split else slot.lib.wlx_pcm_put_wav
    return fn(engine._h, slot.sid, 0, data, len(data), None, C.byref(n)), n.value


def test_refused_and_damaged_files_leave_the_resident_pcm_alone(engine):
    from whisperlive_amd import _lib
    s = engine.create_slot(2, 5)
    try:
        before = np.linspace(-1, 1, 5000, dtype=np.float32)
        s.pcm_put(before)
        s.pcm_put(before[::-1].copy(), 1)
        odd_rate = W.random_adpcm(W.TAG_IMA, 20, 1, 256, rate=44101)
        pcm16 = W.container(1, 1, 8000, 16, 2, bytes(2000))
        three = W.random_adpcm(W.TAG_MS, 20, 3, 96)                          # three channels into a slot of two items
        for data, split in ((odd_rate, False), (pcm16, False), (three, True)):
            rc, n = _put_wav_rc(engine, s, data, split)
            assert rc == _lib.ERR_ARG and n == -1                             # refused, nothing launched
        damaged = bytearray(W.random_adpcm(W.TAG_IMA, 20, 1, 256))
        damaged[damaged.index(b"data") + 8 + 5 * 256 + 2] = 120
        rc, n = _put_wav_rc(engine, s, bytes(damaged))
        assert rc == _lib.ERR_DATA and n == -1
        with pytest.raises(_lib.WlxError) as ei:
            s.put_wav(bytes(damaged))
        assert ei.value.code == _lib.ERR_DATA
        assert np.array_equal(_bits(s.pcm()), _bits(before)) and np.array_equal(_bits(s.pcm(1)), _bits(before[::-1]))
    finally:
        s.close()


def test_g711_across_a_staging_block_seam(engine):
    """one mono file just over one 8 MB staging block (the resample tests' block-shrinking hook refuses the 8-bit codes, as
    wlx_pcm_put_frames does): the outputs around the seam need input bytes of both blocks"""
    from whisperlive_amd import audio_io
    rng = np.random.RandomState(1)
    n = (8 << 20) + 12345
    data = W.container(W.TAG_MULAW, 1, 8000, 8, 1, rng.randint(0, 256, size=n).astype(np.uint8).tobytes())
    frames, _ = audio_io.read_wav(data)
    s = engine.create_slot(1, 5)
    ref = engine.create_slot(1, 5)
    try:
        got_n, _ = s.put_wav(data)
        assert got_n == ref.put_frames(frames, 8000) == 2 * n
        assert np.array_equal(_bits(s.pcm()), _bits(ref.pcm()))
    finally:
        s.close()
        ref.close()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def peaked(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=4)
    yield hip
    hip.close()
    hip.engine.close()


KW = dict(language="en", temperature=0.0, max_new_tokens=24, vad_filter=False, compression_ratio_threshold=None,
          log_prob_threshold=None, no_speech_threshold=None)


def _key(segs):
    return [(s.tokens, s.seek, s.start, s.end) for s in segs]


@pytest.mark.parametrize("kind", ["mulaw", "ima"])
def test_transcribe_of_a_telephony_file_equals_transcribe_of_the_host_decoded_waveform(peaked, kind, tmp_path, monkeypatch):
    from whisperlive_amd import audio_io
    from whisperlive_amd import engine as E
    jfk = np.load(JFK)["pcm"][:6 * 16000]
    pcm = np.clip(np.round(jfk.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    data = W.write_g711(pcm, 16000, W.TAG_MULAW) if kind == "mulaw" else W.write_ima(pcm, 16000, 512, fact=True)
    path = tmp_path / f"jfk_{kind}.wav"
    path.write_bytes(data)
    calls = []
    real = E.Slot.put_wav
    monkeypatch.setattr(E.Slot, "put_wav", lambda self, d, item=0: (calls.append(len(d)), real(self, d, item))[1])
    a, ai = peaked.transcribe(str(path), **KW)
    a = list(a)
    assert calls == [len(data)] and peaked.resident_file_audio().n_samples == 6 * 16000
    wave, sr = audio_io.read_wav(data)
    assert sr == 16000 and wave.shape == (6 * 16000, 1)
    b, bi = peaked.transcribe(wave[:, 0].copy(), **KW)
    b = list(b)
    assert a and _key(a) == _key(b) and ai.duration == bi.duration == 6.0


def test_multichannel_of_a_stereo_ms_adpcm_file_equals_the_two_mono_runs(peaked):
    from whisperlive_amd import audio_io
    from whisperlive_amd.batched import BatchedInferencePipeline
    pcm = W.speech_like(5 * 8000, 2, seed=21)
    stereo = W.write_ms(pcm, 8000, 256, fact=True)
    monos = [W.write_ms(pcm[:, c:c + 1], 8000, 128, fact=True, predictors=[c]) for c in range(2)]
    whole, _ = audio_io.read_wav(stereo)
    for c in range(2):
        assert np.array_equal(audio_io.read_wav(monos[c])[0][:, 0], whole[:, c])          # the mono files hold the stereo file's channels
    kw = dict(language="en", clip_timestamps=[{"start": 0, "end": 30000}, {"start": 40000, "end": 72000}], chunk_length=2, vad_filter=False,
              batch_size=1)
    p = BatchedInferencePipeline(peaked)
    fresh = lambda: {**kw, "clip_timestamps": [dict(c) for c in kw["clip_timestamps"]]}
    segs, info = p.transcribe(stereo, multichannel=True, **fresh())
    segs = list(segs)
    assert info.duration == 5.0 and sorted({s.channel for s in segs}) == [0, 1]
    for c in range(2):
        mono, _ = p.transcribe(monos[c], **fresh())
        assert _key([s for s in segs if s.channel == c]) == _key(list(mono))
