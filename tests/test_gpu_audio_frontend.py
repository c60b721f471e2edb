"""GPU: the file path's device front end on the product path (Slot.put_frames / Slot.pcm / transcribe(path)), tiny.en shapes."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

from oracle import decoding as odec
from oracle import model as omodel
from oracle.provider import NetProvider
from tests import helpers as H
from tests import resample_kernel_ref as R

pytestmark = pytest.mark.gpu

JFK = os.path.join(os.path.dirname(__file__), "golden", "jfk_head.flac")
NOISE_AMP = 0.02            # the amplitude the other suites perturb the oracle's logits with (tests/helpers.py check_decode)


def _wav_bytes(frames: np.ndarray, rate: int) -> bytes:
    """float32 WAVE (format tag 3) of [n, ch] frames"""
    x = np.ascontiguousarray(frames, dtype="<f4")
    ch = x.shape[1]
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", x.nbytes) + x.tobytes()
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module")
def engine(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7), device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def clip():
    """2.0 s of 44.1 kHz stereo, the channels carrying different signals"""
    return R.multichannel(2 * 44100, 44100, 2, R.F32) * np.float32(0.5)


def test_put_frames_matches_load_audio_and_feeds_logmel_resident(engine, clip):
    from whisperlive_amd.audio_io import load_audio
    a, b = engine.create_slot(1, 5), engine.create_slot(1, 5)
    try:
        n = a.put_frames(clip, 44100)
        pcm = a.pcm()
        want = load_audio(_wav_bytes(clip, 44100))
        assert n == pcm.shape[0] == want.shape[0] == 32000
        err = float(np.abs(pcm.astype(np.float64) - want.astype(np.float64)).max())
        print(f"put_frames vs load_audio: max abs {err:.3e}")
        assert err <= R.RESAMPLE_ATOL
        T = a.logmel_resident()
        assert T == b.logmel(pcm)
        assert np.array_equal(a.features().view(np.uint32), b.features().view(np.uint32))
    finally:
        a.close()
        b.close()


def test_int16_frames_and_16k_mono_float_is_pcm_put(engine):
    s = engine.create_slot(1, 5)
    try:
        x = R.multichannel(16000, 16000, 1, R.F32)
        assert s.put_frames(x, 16000) == 16000
        assert np.array_equal(s.pcm(), x[:, 0])                       # convert + down-mix only: bit-identical to wlx_pcm_put
        q = R.multichannel(48000, 48000, 2, R.S16)
        assert s.put_frames(q, 48000) == 16000
        want = R.scipy_ref(R.mono_f32(q), 1, 3)
        assert np.abs(s.pcm() - want).max() <= R.RESAMPLE_ATOL
    finally:
        s.close()


def test_steep_rate_file_takes_the_device_route(engine):
    """176.4 kHz (40 / 441) is served with a smaller tile: the same check as at 44.1 kHz, with the steep rates' bound"""
    from whisperlive_amd.audio_io import load_audio
    from whisperlive_amd.engine import resample_supported
    x = R.multichannel(176400 // 2, 176400, 2, R.F32) * np.float32(0.5)
    s = engine.create_slot(1, 5)
    try:
        assert resample_supported(176400, 2)
        assert s.put_frames(x, 176400) == 8000
        want = load_audio(_wav_bytes(x, 176400))
        err = float(np.abs(s.pcm().astype(np.float64) - want.astype(np.float64)).max())
        print(f"put_frames vs load_audio at 176400 Hz: max abs {err:.3e}")
        assert err <= R.RESAMPLE_ATOL_STEEP
    finally:
        s.close()


def test_put_frames_on_item_1_leaves_item_0(engine, clip):
    s = engine.create_slot(2, 5)
    try:
        other = R.multichannel(48000, 48000, 1, R.F32)
        s.put_frames(other, 48000, item=0)
        s.logmel_resident(item=0)
        before = s.features(item=0).copy()
        pcm0 = s.pcm(item=0).copy()
        s.put_frames(clip, 44100, item=1)
        s.logmel_resident(item=1)
        assert s.features(item=1).shape[1] == 32000 // 160 + 1
        assert np.array_equal(s.features(item=0), before) and np.array_equal(s.pcm(item=0), pcm0)
    finally:
        s.close()


def test_output_over_an_hour_is_refused_before_the_frames_are_read(engine):
    from whisperlive_amd import _lib
    s = engine.create_slot(1, 5)
    try:
        tiny = np.zeros(16, np.float32)                               # shape-only: the call must refuse before it reads n_frames samples
        n_out = C.c_int64(-1)
        n_frames = 8000 * 3600 + 1                                    # at 8 kHz: 2 n_frames = 3600 s + 2 samples of output
        rc = engine.lib.wlx_pcm_put_frames(engine._h, s.sid, 0, tiny.ctypes.data_as(C.c_void_p), n_frames, 1, _lib.PCM_F32, 8000,
                                           C.byref(n_out))
        assert rc == _lib.ERR_ARG and n_out.value == -1
        rc = engine.lib.wlx_pcm_put_frames(engine._h, s.sid, 0, tiny.ctypes.data_as(C.c_void_p), 16, 1, _lib.PCM_F32, 44101, C.byref(n_out))
        assert rc == _lib.ERR_ARG                                     # a ratio the device does not serve
        assert s.pcm().shape[0] == 0                                  # nothing became resident
    finally:
        s.close()


def _conditioned_model(path):
    """tiny.en on peaked weights, the first seed (5, 6, ...) whose first-window decode of the clip is well conditioned by
    H.decode_is_well_conditioned; -> (model, seed)"""
    from whisperlive_amd.audio_io import load_audio
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from oracle import logmel as olm
    spec = H.TINY_EN
    pcm = load_audio(path)
    feats = olm.pad_or_trim(olm.log_mel_spectrogram(pcm, spec.n_mels)[:, :-1])[None]
    ids = H.token_ids_for(spec.vocab)
    for seed in (5, 6, 7, 8):
        w = H.peaked_weights(spec, seed)
        oracle = omodel.WhisperOracle(H.oracle_spec(spec), H.f16_weights(w))
        enc = oracle.encode(feats)
        opts = odec.GenOptions(ids=ids, beam_size=5, patience=1.0, max_length=1 + 24, suppress_tokens=H.default_suppress(ids))
        ref = odec.generate(NetProvider(oracle, enc), [ids.sot], opts)
        if H.decode_is_well_conditioned(oracle, enc, [ids.sot], opts, ref, NOISE_AMP):
            return WhisperModelHIP("peaked", weights=w, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab)), seed
    raise AssertionError("no well-conditioned seed among 5..8")


@pytest.fixture(scope="module")
def conditioned(gpu):
    hip, seed = _conditioned_model(JFK)
    print("peaked seed used:", seed)
    yield hip
    hip.close()
    hip.engine.close()


KW = dict(language="en", temperature=0.0, max_new_tokens=24, vad_filter=False, compression_ratio_threshold=None,
          log_prob_threshold=None, no_speech_threshold=None)


def test_transcribe_path_equals_transcribe_of_load_audio(conditioned):
    from whisperlive_amd.audio_io import load_audio
    hip = conditioned
    a, ai = hip.transcribe(JFK, **KW)
    b, bi = hip.transcribe(load_audio(JFK), **KW)
    a, b = list(a), list(b)
    assert a and [s.tokens for s in a] == [s.tokens for s in b]
    assert [(s.seek, s.start, s.end) for s in a] == [(s.seek, s.start, s.end) for s in b]
    assert ai.duration == bi.duration and ai.language == bi.language == "en"
    with open(JFK, "rb") as f:
        c, _ = hip.transcribe(io.BytesIO(f.read()), **KW)
    assert [s.tokens for s in c] == [s.tokens for s in a]


def test_refused_rate_keeps_the_host_route(conditioned, monkeypatch):
    """a file at a rate the device front end refuses (44101 Hz: 16000 / 44101 does not reduce) is resampled on the host as
    load_audio does, so transcribe(file) IS transcribe(load_audio(file)) — when Python knows the rate is refused, and when only
    the library does (its WLX_ERR_ARG refusal launches nothing and is answered with the host route, not raised)"""
    from whisperlive_amd import engine as E
    from whisperlive_amd.audio_io import load_audio, read_audio
    hip = conditioned
    frames, rate = read_audio(JFK)
    assert rate == 44100
    wav = _wav_bytes(frames, 44101)                                  # the same samples, labelled one hertz off
    calls = []
    real = E.Slot.put_frames
    monkeypatch.setattr(E.Slot, "put_frames", lambda self, fr, sr, item=0: (calls.append(sr), real(self, fr, sr, item))[1])

    def run(src):
        segs, info = hip.transcribe(src, **KW)
        return [(s.tokens, s.seek, s.start, s.end) for s in segs], info.duration

    want = run(load_audio(wav))
    assert want[0]
    assert run(wav) == want and calls == []                          # Python knew: the device was not asked
    monkeypatch.setattr(E, "resample_supported", lambda sr, ch=1: True)
    assert run(wav) == want and calls == [44101]                     # the library refused: same answer
    assert run(JFK)[0] and calls == [44101, 44100]                   # ... and a served file still takes the device route
