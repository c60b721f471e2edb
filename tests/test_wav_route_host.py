"""CPU: where transcribe(file), BatchedInferencePipeline.transcribe(file) and multichannel=True send a telephony WAV file (G.711, IMA /
MS ADPCM), on scripted slots in the style of tests/fakes.py: to Slot.put_wav / put_wav_split when the probe says the device route
serves the file; back to read_audio + put_frames when the library refuses it (WLX_ERR_ARG) or the probe says unserved; a ValueError
when the file is damaged (WLX_ERR_DATA, from the probe or from the call); and the route of before for PCM files and on a slot
without the front end. The probe (wlx_wav_probe) is host-only and runs for real."""
import numpy as np
import pytest

from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

from . import wav_writer as W

SR = 16000
PCM = W.speech_like(2 * 8000, 2, seed=1)
FILES = {
    "mulaw": W.write_g711(PCM[:, :1], 8000, W.TAG_MULAW),
    "alaw": W.write_g711(PCM[:, :1], 8000, W.TAG_ALAW, extensible=True),
    "ima": W.random_adpcm(W.TAG_IMA, 32, 1, 256, seed=3),
    "ms": W.random_adpcm(W.TAG_MS, 32, 1, 256, seed=4),
}


def _error(code):
    e = _lib.WlxError(f"libwlx error {code}: scripted")
    e.code = code
    return e


class FrontEndSlot(FakeSlot):
    """FakeSlot with the device front end's methods, scripted: wav_error = the wlx_status put_wav fails with"""
    wav_error = None

    def put_wav(self, data, item=0):
        self.calls.append(("put_wav", bytes(data[:4]), item))
        if self.wav_error:
            raise _error(self.wav_error)
        self._pcm = np.zeros(2 * SR, np.float32)
        return self._pcm.shape[0], None

    def put_wav_split(self, data, first_item=0):
        self.calls.append(("put_wav_split", bytes(data[:4]), first_item))
        if self.wav_error:
            raise _error(self.wav_error)
        self.sources = [first_item, first_item + 1]
        return 2 * SR, None

    def put_frames(self, frames, sample_rate, item=0):
        self.calls.append(("put_frames", tuple(np.asarray(frames).shape), sample_rate))
        self._pcm = np.zeros(np.asarray(frames).shape[0], np.float32)
        return self._pcm.shape[0]

    def put_frames_split(self, frames, rate, first_item=0):
        self.calls.append(("put_frames_split", tuple(np.asarray(frames).shape), rate))
        return np.asarray(frames).shape[0] * 16000 // rate

    def pcm_put(self, pcm, item=0):
        self.calls.append(("pcm_put", item, len(pcm)))
        self._pcm = np.asarray(pcm)

    def pcm(self, item=0):
        return self._pcm

    def pcm_count(self, item=0):
        return self._pcm.shape[0]

    def logmel_resident(self, item=0):
        self.calls.append(("logmel_resident", item))
        self._frames[item] = (self._pcm.shape[0] + 160) // 160
        return self._frames[item]

    def logmel_chunks(self, chunks, src_item=0, first_item=0):
        self.calls.append(("logmel_chunks", len(chunks)))
        for i, c in enumerate(chunks):
            self._frames[first_item + i] = (sum(b - a for a, b in c) + 160) // 160
        return [self._frames[first_item + i] for i in range(len(chunks))]


class FrontEndEngine(FakeEngine):
    slot_type = FrontEndSlot
    wav_error = None

    def create_slot(self, max_batch=1, rows=5):
        s = self.slot_type(self, max_batch, rows)
        s.wav_error = self.wav_error
        s._enc_generation = 0
        self.slots.append(s)
        return s


class NoWavSlot(FrontEndSlot):
    put_wav = property()                        # hasattr(slot, "put_wav") is False: the front end of before
    put_wav_split = property()


def _model(engine, max_batch=2):
    engine.spec = WhisperSpec(80, 128, 2, 1, 1, 512, 2310)
    engine.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=engine, hf_tokenizer=synthetic_tokenizer(engine.spec.vocab), max_batch=max_batch)


KW = dict(language="en", vad_filter=False)
CLIP = [{"start": 0, "end": SR}]


def _single(hip, data):
    segs, info = hip.transcribe(data, **KW)
    return list(segs), info


def _batched(hip, data):
    segs, info = BatchedInferencePipeline(hip).transcribe(data, clip_timestamps=CLIP, batch_size=1, **KW)
    return list(segs), info


def _multi(hip, data):
    segs, info = BatchedInferencePipeline(hip).transcribe(data, clip_timestamps=CLIP, batch_size=1, multichannel=True, **KW)
    return list(segs), info


def _names(eng):
    keep = ("put_wav", "put_wav_split", "put_frames", "put_frames_split", "pcm_put", "logmel")
    return [c[0] for s in eng.slots for c in s.calls if c[0] in keep]


@pytest.mark.parametrize("kind", sorted(FILES))
@pytest.mark.parametrize("run", [_single, _batched])
def test_a_served_telephony_file_goes_to_put_wav(run, kind):
    eng = FrontEndEngine()
    _segs, info = run(_model(eng), FILES[kind])
    assert _names(eng) == ["put_wav"] and info.duration == 2.0


@pytest.mark.parametrize("run", [_single, _batched])
def test_a_refused_file_falls_back_to_read_audio_and_put_frames(run):
    eng = FrontEndEngine()
    eng.wav_error = _lib.ERR_ARG
    run(_model(eng), FILES["mulaw"])
    assert _names(eng) == ["put_wav", "put_frames"]
    assert [c for s in eng.slots for c in s.calls if c[0] == "put_frames"] == [("put_frames", (2 * 8000, 1), 8000)]


@pytest.mark.parametrize("run", [_single, _batched])
def test_a_file_the_call_finds_damaged_is_a_value_error(run):
    eng = FrontEndEngine()
    eng.wav_error = _lib.ERR_DATA
    with pytest.raises(ValueError, match="damaged WAV stream"):
        run(_model(eng), FILES["ima"])
    assert _names(eng) == ["put_wav"]


@pytest.mark.parametrize("run", [_single, _batched, _multi])
def test_a_file_the_probe_finds_damaged_is_a_value_error_before_any_call(run):
    data = bytearray(W.random_adpcm(W.TAG_IMA, 8, 2, 72, seed=1))
    data[data.index(b"data") + 8 + 72 + 2] = 200
    eng = FrontEndEngine()
    with pytest.raises(ValueError, match="damaged WAV stream"):
        run(_model(eng, 4), bytes(data))
    assert _names(eng) == []


@pytest.mark.parametrize("run", [_single, _batched])
def test_any_other_library_error_is_raised(run):
    eng = FrontEndEngine()
    eng.wav_error = 2                             # WLX_ERR_HIP
    with pytest.raises(_lib.WlxError):
        run(_model(eng), FILES["ms"])


@pytest.mark.parametrize("run", [_single, _batched])
def test_pcm_files_and_slots_without_put_wav_take_the_route_of_before(run):
    s16 = W.container(1, 1, 8000, 16, 2, PCM[:, :1].astype("<i2").tobytes())
    eng = FrontEndEngine()
    run(_model(eng), s16)
    assert _names(eng) == ["put_frames"]
    eng = FrontEndEngine()
    eng.slot_type = NoWavSlot
    run(_model(eng), FILES["ima"])
    assert _names(eng) == ["put_frames"]


@pytest.mark.parametrize("run", [_single, _batched])
def test_an_unserved_telephony_file_is_decoded_on_the_host(run):
    """44101 Hz: the probe says unserved, read_audio decodes the ADPCM, and the resampler's own refusal sends it to the host resample"""
    eng = FrontEndEngine()
    _segs, info = run(_model(eng), W.random_adpcm(W.TAG_MS, 64, 1, 256, rate=44101, seed=5))
    assert "put_wav" not in _names(eng) and "put_frames" not in _names(eng)
    assert abs(info.duration - 64 * 500 / 44101) < 1e-3


def test_a_slot_without_any_front_end_decodes_and_resamples_on_the_host():
    eng = FakeEngine()
    _segs, info = _single(_model(eng), FILES["alaw"])
    assert _names(eng) == ["logmel"] and info.duration == 2.0


def test_multichannel_sends_a_served_stereo_file_to_put_wav_split():
    eng = FrontEndEngine()
    segs, _info = _multi(_model(eng, 4), W.write_ms(PCM, 8000, 256))
    assert _names(eng) == ["put_wav_split"] and eng.slots[0].calls[0] == ("put_wav_split", b"RIFF", 2)
    assert sorted({s.channel for s in segs}) == [0, 1]


def test_multichannel_decodes_an_unserved_layout_with_read_audio_and_splits_the_frames():
    eng = FrontEndEngine()
    eng.slot_type = NoWavSlot
    _multi(_model(eng, 4), W.write_g711(PCM, 8000, W.TAG_MULAW))
    assert _names(eng) == ["put_frames_split"]
    assert eng.slots[0].calls[0] == ("put_frames_split", (2 * 8000, 2), 8000)


def test_multichannel_turns_the_calls_errors_into_value_errors():
    for code, text in ((_lib.ERR_DATA, "damaged WAV stream"), (_lib.ERR_ARG, "refused the audio")):
        eng = FrontEndEngine()
        eng.wav_error = code
        with pytest.raises(ValueError, match=text):
            _multi(_model(eng, 4), W.write_ima(PCM, 8000, 256))
