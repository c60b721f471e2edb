"""CPU: where transcribe(file) and BatchedInferencePipeline.transcribe(file) send a FLAC file, on scripted slots (tests/fakes.py): to
Slot.put_flac when the slot has one; back to read_audio + put_frames when the library refuses the stream (WLX_ERR_ARG); a ValueError
when it finds the stream damaged (WLX_ERR_DATA); and the route of before on a slot without the front end."""
import numpy as np
import pytest

from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

from . import flac_writer as W

SR = 16000


def _flac(seconds=2, rate=16000):
    rng = np.random.RandomState(0)
    pcm = rng.randint(-2000, 2000, size=(seconds * rate, 1)).astype(np.int64)
    return W.encode_stream(pcm, rate, 16, W.split_blocks(pcm.shape[0], 4096), subframe={"type": "fixed", "order": 0, "k": 10})


def _error(code):
    e = _lib.WlxError(f"libwlx error {code}: scripted")
    e.code = code
    return e


class FrontEndSlot(FakeSlot):
    """FakeSlot with the device front end's methods, scripted: flac_error = the wlx_status put_flac fails with"""
    flac_error = None

    def put_flac(self, data, item=0):
        self.calls.append(("put_flac", bytes(data[:4]), item))
        if self.flac_error:
            raise _error(self.flac_error)
        self._pcm = np.zeros(2 * SR, np.float32)
        return self._pcm.shape[0], None

    def put_frames(self, frames, sample_rate, item=0):
        self.calls.append(("put_frames", tuple(np.asarray(frames).shape), sample_rate))
        self._pcm = np.zeros(np.asarray(frames).shape[0], np.float32)
        return self._pcm.shape[0]

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
        return [(sum(b - a for a, b in c) + 160) // 160 for c in chunks]


class FrontEndEngine(FakeEngine):
    slot_type = FrontEndSlot
    flac_error = None

    def create_slot(self, max_batch=1, rows=5):
        s = self.slot_type(self, max_batch, rows)
        s.flac_error = self.flac_error
        s._enc_generation = 0
        self.slots.append(s)
        return s


class NoFlacSlot(FrontEndSlot):
    put_flac = property()                       # hasattr(slot, "put_flac") is False: the front end of before


def _model(engine):
    engine.spec = WhisperSpec(80, 128, 2, 1, 1, 512, 2310)
    engine.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=engine, hf_tokenizer=synthetic_tokenizer(engine.spec.vocab), max_batch=2)


KW = dict(language="en", vad_filter=False)


def _single(hip, data):
    segs, info = hip.transcribe(data, **KW)
    return list(segs), info


def _batched(hip, data):
    segs, info = BatchedInferencePipeline(hip).transcribe(data, clip_timestamps=[{"start": 0, "end": SR}], batch_size=1, **KW)
    return list(segs), info


def _names(eng):
    return [c[0] for s in eng.slots for c in s.calls if c[0] in ("put_flac", "put_frames", "pcm_put", "logmel")]


@pytest.mark.parametrize("run", [_single, _batched])
def test_flac_bytes_go_to_put_flac(run):
    eng = FrontEndEngine()
    _segs, info = run(_model(eng), _flac())
    assert _names(eng) == ["put_flac"] and info.duration == 2.0


@pytest.mark.parametrize("run", [_single, _batched])
def test_a_refused_stream_falls_back_to_read_audio_and_put_frames(run):
    eng = FrontEndEngine()
    eng.flac_error = _lib.ERR_ARG
    _segs, info = run(_model(eng), _flac())
    assert _names(eng) == ["put_flac", "put_frames"] and info.duration == 2.0
    assert [c for s in eng.slots for c in s.calls if c[0] == "put_frames"] == [("put_frames", (2 * SR, 1), 16000)]


@pytest.mark.parametrize("run", [_single, _batched])
def test_a_damaged_stream_is_the_value_error_of_the_python_decoder(run):
    eng = FrontEndEngine()
    eng.flac_error = _lib.ERR_DATA
    with pytest.raises(ValueError):
        run(_model(eng), _flac())
    assert _names(eng) == ["put_flac"]


@pytest.mark.parametrize("run", [_single, _batched])
def test_any_other_library_error_is_raised(run):
    eng = FrontEndEngine()
    eng.flac_error = 2                            # WLX_ERR_HIP
    with pytest.raises(_lib.WlxError):
        run(_model(eng), _flac())


@pytest.mark.parametrize("run", [_single, _batched])
def test_a_slot_without_put_flac_takes_the_route_of_before(run):
    eng = FrontEndEngine()
    eng.slot_type = NoFlacSlot
    run(_model(eng), _flac())
    assert _names(eng) == ["put_frames"]


def test_a_slot_without_any_front_end_decodes_and_resamples_on_the_host():
    eng = FakeEngine()
    _segs, info = _single(_model(eng), _flac(rate=8000))
    assert _names(eng) == ["logmel"] and info.duration == 2.0
