"""Host side of the batched VAD gate (no GPU): how BatchInferenceWorker._process_multi drives a transcriber's
`encode_audio_batch_gated` and falls back to the per-request gate, the arithmetic of SileroHIPModel.probs_many / probs_pcm_many against
a stub library, and the binding table."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests.fakes import FakeEngine
from whisperlive_amd import _lib, vad
from whisperlive_amd.batching import BatchInferenceWorker, BatchRequest
from whisperlive_amd.tokenizer import Tokenizer, synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

V = 2310


class GatedModel(WhisperModelHIP):
    """a transcriber with a scripted batched front half: records its calls; `mode` = "ok" (every gated item keeps half its samples,
    an empty audio counts 0), "none" (refusal) or "raise" """
    mode = "ok"

    def encode_audio_batch_gated(self, audios, options_list):
        self.gated_calls.append((list(audios), list(options_list)))
        if self.mode == "none":
            return None
        if self.mode == "raise":
            raise RuntimeError("front half broke")
        counts = [(len(a) // 2 if o is not None else len(a)) for a, o in zip(audios, options_list)]
        return self.encode_audio_batch([a[:c] for a, c in zip(audios, counts) if c]), counts


def make(cls=GatedModel, mode="ok"):
    eng = FakeEngine()
    m = cls("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(V), max_batch=8, vad_model=vad.EnergyGateModel())
    m.gated_calls, m.mode = [], mode
    tk = Tokenizer(m.hf_tokenizer, False)
    eng.default_tokens = [tk.timestamp_begin] + tk.encode(" fine") + [tk.timestamp_begin + 40]
    return m, eng


def requests():
    loud = (0.1 * np.sin(np.arange(32000) * 0.05)).astype(np.float32)
    return [BatchRequest(audio=loud, use_vad=True),
            BatchRequest(audio=loud[:16000], use_vad=False),
            BatchRequest(audio=loud[:24000], use_vad=True, vad_parameters={"threshold": 0.4, "speech_pad_ms": 30})]


def test_one_call_per_batch_with_none_options_for_ungated_requests():
    m, eng = make()
    reqs = requests()
    BatchInferenceWorker(m, max_batch_size=8)._process_multi(reqs)
    assert all(r.future.is_set() and r.error is None for r in reqs)
    assert len(m.gated_calls) == 1
    audios, opts = m.gated_calls[0]
    assert [len(a) for a in audios] == [32000, 16000, 24000]
    assert opts[0] == vad.VadOptions() and opts[1] is None and opts[2] == vad.VadOptions(threshold=0.4, speech_pad_ms=30)
    # the durations are the gated counts, and nothing was gated or encoded a second time
    assert [r.info.duration_after_vad for r in reqs] == [1.0, 1.0, 0.75]
    assert [c[0] for c in eng.slots[0].calls] == ["logmel", "logmel", "logmel", "encode", "generate"]
    assert [r.result[0].text for r in reqs] == ["fine"] * 3


def test_count_zero_is_an_empty_result_and_takes_no_encoder_item():
    m, eng = make()
    reqs = requests() + [BatchRequest(audio=np.zeros(0, np.float32), use_vad=False)]
    BatchInferenceWorker(m, max_batch_size=8)._process_multi(reqs)
    assert reqs[3].future.is_set() and reqs[3].error is None and reqs[3].result == [] and reqs[3].info.duration == 0.0
    assert all(r.error is None and r.result for r in reqs[:3])
    assert [c for c in eng.slots[0].calls if c[0] == "encode"][0][1] == 3


def test_bad_vad_parameters_are_that_request_s_error_alone():
    m, _ = make()
    reqs = requests()
    reqs[1] = BatchRequest(audio=reqs[1].audio, use_vad=True, vad_parameters={"no_such_option": 1})
    BatchInferenceWorker(m, max_batch_size=8)._process_multi(reqs)
    assert isinstance(reqs[1].error, TypeError) and reqs[1].future.is_set() and reqs[1].result is None
    assert reqs[0].error is None and reqs[2].error is None and reqs[0].result and reqs[2].result
    assert len(m.gated_calls) == 1 and len(m.gated_calls[0][0]) == 2          # the refused request is not in the batch


@pytest.mark.parametrize("mode", ["none", "raise"])
def test_refusal_or_exception_falls_back_to_the_per_request_gate(mode):
    m, eng = make(mode=mode)
    reqs = requests()
    reqs.append(BatchRequest(audio=reqs[0].audio, use_vad=True, vad_parameters={"no_such_option": 1}))
    BatchInferenceWorker(m, max_batch_size=8)._process_multi(reqs)
    assert all(r.future.is_set() for r in reqs)
    assert all(r.error is None and r.result for r in reqs[:3]) and isinstance(reqs[3].error, TypeError)
    assert len(m.gated_calls) == 1
    # today's route: the energy gate per request on the host, then encode_audio_batch over what it kept
    want = [len(np.concatenate(vad.collect_chunks(r.audio, vad.get_speech_timestamps(
        r.audio, vad.VadOptions(**(r.vad_parameters or {})), model=m.vad_model))[0])) if r.use_vad else len(r.audio) for r in reqs[:3]]
    assert [c[2] for c in eng.slots[0].calls if c[0] == "logmel"] == want
    assert [r.info.duration_after_vad for r in reqs[:3]] == [n / 16000 for n in want]


def test_a_gate_that_is_not_the_silero_network_never_takes_the_batched_route():
    m, eng = make(cls=WhisperModelHIP)                      # the real method, an EnergyGateModel gate, no resident-PCM entry points
    opts = [vad.VadOptions(), None]
    audios = [np.ones(4000, np.float32), np.ones(3000, np.float32)]
    assert m.speech_timestamps_batch(audios, [vad.VadOptions()] * 2) is None
    assert m.encode_audio_batch_gated(audios, opts) is None
    assert m.encode_audio_batch_gated(audios, [None, None]) is None           # (FakeSlot has no pcm_put: not a device slot)
    assert not eng.slots or not eng.slots[0].calls                            # nothing was launched on the way to the refusal
    reqs = requests()
    BatchInferenceWorker(m, max_batch_size=8)._process_multi(reqs)
    assert all(r.error is None and r.result for r in reqs)


def test_a_mock_transcriber_does_not_grow_the_attribute():
    from unittest.mock import MagicMock
    w = BatchInferenceWorker(MagicMock(), max_batch_size=4)
    assert w._gate_batch([BatchRequest(audio=np.zeros(10, np.float32))]) is None


# ---- SileroHIPModel.probs_many / probs_pcm_many against a stub library -------------------------------------------------
class StubLib:
    """records every batch call and answers row i with T_i copies of (index of the item in the whole list)"""

    def __init__(self):
        self.calls = []
        self.seen = 0

    def _serve(self, cnt, extra, n, probs, cap, nw, ms):
        counts = [cnt[i] for i in range(n)]
        ex = [extra[i] for i in range(n)]
        T = [-(-c // 512) + e for c, e in zip(counts, ex)]
        assert sum(T) == cap
        k = 0
        for i, t in enumerate(T):
            nw[i] = t
            for _ in range(t):
                probs[k] = float(self.seen + i)
                k += 1
        self.seen += n
        C.cast(ms, C.POINTER(C.c_float))[0] = 0.25
        return counts, ex

    def wlx_vad_probs_batch(self, handle, pcm, cnt, extra, n, probs, cap, nw, ms):
        counts, ex = self._serve(cnt, extra, n, probs, cap, nw, ms)
        self.calls.append(("batch", counts, ex, [pcm[j] for j in range(sum(counts))]))
        return 0

    def wlx_vad_probs_pcm_batch(self, handle, eng, sid, first_item, cnt, extra, n, probs, cap, nw, ms):
        counts, ex = self._serve(cnt, extra, n, probs, cap, nw, ms)
        self.calls.append(("pcm", eng, sid, first_item, counts, ex))
        return 0


def stub_model():
    m = vad.SileroHIPModel.__new__(vad.SileroHIPModel)
    m._lib, m.lib, m.handle, m.device, m.last_device_ms = _lib, StubLib(), C.c_void_p(1), 0, 0.0
    return m


def test_probs_many_extra_windows_and_packing():
    m = stub_model()
    lens = [1, 511, 512, 513, 1024, 0]
    audios = [np.full(n, i + 1, np.float32) for i, n in enumerate(lens)]
    rows = m.probs_many(audios)
    (kind, counts, extra, flat), = m.lib.calls
    assert kind == "batch" and counts == lens
    assert extra == [0, 0, 1, 0, 1, 1]                          # a whole zero window when n is a multiple of 512 (0 included)
    assert flat == np.concatenate(audios).tolist()              # back to back, unpadded
    assert [r.tolist() for r in rows] == [[0.0], [1.0], [2.0, 2.0], [3.0, 3.0], [4.0] * 3, [5.0]]
    assert [len(r) for r in rows] == [n // 512 + 1 for n in lens]
    assert m.last_device_ms == 0.25
    assert m.probs_many([]) == []


def test_lists_longer_than_the_table_are_split_into_consecutive_calls():
    m = stub_model()
    lens = [(7 * i) % 40 + 1 for i in range(130)]
    audios = [np.full(n, i, np.float32) for i, n in enumerate(lens)]
    rows = m.probs_many(audios)
    assert [len(c[1]) for c in m.lib.calls] == [64, 64, 2]
    assert [c[3] for c in m.lib.calls] == [np.concatenate(audios[a:a + 64]).tolist() for a in (0, 64, 128)]   # each call reads its own segments
    assert [r.tolist() for r in rows] == [[float(i)] for i in range(130)]
    assert m.last_device_ms == 0.75
    slot = SimpleNamespace(engine=SimpleNamespace(_h="engine"), sid=3)
    m2 = stub_model()
    rows = m2.probs_pcm_many(slot, [600] * 70, first_item=2)
    assert [(c[0], c[1], c[2], c[3], len(c[4])) for c in m2.lib.calls] == [("pcm", "engine", 3, 2, 64), ("pcm", "engine", 3, 66, 6)]
    assert all(c[5] == [0] * len(c[4]) for c in m2.lib.calls)
    assert [r.tolist() for r in rows] == [[float(i)] * 2 for i in range(70)]


def test_get_speech_timestamps_many_segments_every_row(monkeypatch):
    m = stub_model()
    monkeypatch.setattr(m, "probs_many", lambda audios: [np.full(len(a) // 512 + 1, p, np.float32) for a, p in zip(audios, (0.9, 0.1))])
    seen = []
    monkeypatch.setattr(vad, "speech_segments_from_probs_native", lambda p, n, o, sr=16000: seen.append((p.tolist(), n, o, sr)) or [len(seen)])
    o = vad.VadOptions(threshold=0.3)
    out = vad.get_speech_timestamps_many([np.zeros(1000, np.float32), np.zeros(512, np.float32)], [o, None], m)
    assert out == [[1], [2]]
    assert seen[0][1:] == (1000, o, 16000) and seen[1][1:] == (512, vad.VadOptions(), 16000) and len(seen[1][0]) == 2


# ---- binding table ---------------------------------------------------------------------------------------------------
def test_exports_and_the_table_width_mirror_the_header():
    assert {"wlx_vad_probs_batch", "wlx_vad_probs_pcm_batch"} <= set(_lib.EXPORTS)
    hdr = (Path(_lib.PKG_DIR).parent / "include" / "wlx.h").read_text()
    assert int(re.search(r"#define\s+WLX_VAD_MAX_BATCH\s+(\d+)", hdr).group(1)) == _lib.VAD_MAX_BATCH == 64
    assert re.search(r"int32_t\s+wlx_vad_probs_batch\(wlx_vad\* v, const float\* pcm, const int64_t\* n_samples", hdr)
    assert re.search(r"int32_t\s+wlx_vad_probs_pcm_batch\(wlx_vad\* v, wlx_engine\* e, int32_t slot, int32_t first_item", hdr)
