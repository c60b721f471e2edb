"""CPU: the host side of wlx_pcm_put_many — the header and its ctypes mirror, batched._put_audio_many and iter_many(wave_put=True) on
scripted slots (tests/fakes.py), the REST flag, and csrc/put_many_plan.h under the host sanitizers (tests/put_many_plan_check.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

from tests.fakes import FrontEndEngine, FrontEndSlot
from whisperlive_amd import _lib as L
from whisperlive_amd import batched as B
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

from . import flac_writer as FW
from . import wav_writer as WW

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = next((c for c in (shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
SR = 16000
KW = dict(language="en", vad_filter=False, clip_timestamps=[{"start": 0, "end": SR}])


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_entry_point_and_both_structs():
    with open(os.path.join(ROOT, "include", "wlx.h")) as f:
        h = f.read()
    assert "#define WLX_ABI_VERSION 1" in h or re.search(r"WLX_ABI_VERSION\s+1\b", h)
    for name, value in (("WLX_PUT_PCM", 0), ("WLX_PUT_FRAMES", 1), ("WLX_PUT_FLAC", 2), ("WLX_PUT_WAV", 3), ("WLX_PUT_MANY_MAX", 64)):
        assert re.search(rf"#define {name}\s+{value}\b", h), name
    flat = " ".join(h.split())
    assert ("typedef struct { int32_t kind; const void* data; int64_t n; /* samples | frames | bytes */ int32_t channels, sample_format, "
            "sample_rate; /* WLX_PUT_FRAMES only */ } wlx_put_entry;") in flat
    assert "typedef struct { int32_t status; int64_t n_out; } wlx_put_result;" in flat
    assert ("int32_t wlx_pcm_put_many(wlx_engine* e, int32_t slot, int32_t first_item, int32_t n, const wlx_put_entry* entries, "
            "wlx_put_result* results);") in flat
    for hook in ("wlx_debug_resample_many", "wlx_debug_flac_decode_many", "wlx_debug_put_many_budget"):
        assert f"int32_t {hook}(" in h and hook in L.EXPORTS
    assert "wlx_pcm_put_many" in L.EXPORTS and "put_many.hip" in L.SOURCES
    assert (L.PUT_PCM, L.PUT_FRAMES, L.PUT_FLAC, L.PUT_WAV, L.PUT_MANY_MAX) == (0, 1, 2, 3, 64)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_ctypes_structs_match_the_headers_sizes(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "wlx.h"\nint main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(wlx_put_entry), offsetof(wlx_put_entry, data), offsetof(wlx_put_entry, n), offsetof(wlx_put_entry, channels), "
                   "offsetof(wlx_put_entry, sample_rate), sizeof(wlx_put_result), offsetof(wlx_put_result, n_out), "
                   "offsetof(wlx_put_entry, sample_format)); }\n")
    exe = tmp_path / "sizes"
    build = subprocess.run([CXX, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E, R = L.wlx_put_entry, L.wlx_put_result
    assert got == [C.sizeof(E), E.data.offset, E.n.offset, E.channels.offset, E.sample_rate.offset, C.sizeof(R), R.n_out.offset,
                   E.sample_format.offset]
    assert C.sizeof(E) == 40 and C.sizeof(R) == 16


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_sub_batch_packing_tile_prefix_and_status_verdict_under_the_sanitizers(tmp_path):
    exe = tmp_path / "put_many_plan_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "put_many_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr[-3000:])
    assert run.returncode == 0 and "put_many_plan_check: 0 failures" in run.stdout, (run.stdout, run.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- scripted slots
class ManySlot(FrontEndSlot):
    """FrontEndSlot with the single-file routes and put_many, scripted: `verdict(kind, data)` -> None (served), L.ERR_ARG or L.ERR_DATA"""
    verdict = staticmethod(lambda kind, data: None)

    def _single(self, name, n, item):
        self.calls.append((name, item, n))
        self.resident[item] = np.zeros(n, np.float32)
        return n

    def put_flac(self, data, item=0):
        return self._single("put_flac", 2 * SR, item), None

    def put_wav(self, data, item=0):
        return self._single("put_wav", SR, item), None

    def put_frames(self, frames, rate, item=0):
        return self._single("put_frames", int(np.asarray(frames).shape[0]) * SR // rate, item)

    def put_many(self, entries, first_item=0, with_info=False):
        out = []
        for at in range(0, len(entries), L.PUT_MANY_MAX):          # as engine.Slot.put_many cuts them
            part = entries[at:at + L.PUT_MANY_MAX]
            self.calls.append(("put_many", first_item + at, [e[0] for e in part]))
            for k, e in enumerate(part):
                code = self.verdict(e[0], e[1])
                if code is not None:
                    err = L.WlxError(f"scripted {code}")
                    err.code = code
                    out.append(err)
                    continue
                n = {"pcm": lambda: len(e[1]), "frames": lambda: e[1].shape[0] * SR // e[2], "flac": lambda: 2 * SR, "wav": lambda: SR}[e[0]]()
                self.resident[first_item + at + k] = np.zeros(n, np.float32)
                out.append((n, None))
        return out


class ManyEngine(FrontEndEngine):
    slot_type = ManySlot


class _Model:
    class feature_extractor:
        sampling_rate = SR


def _flac(seconds=2, seed=0):
    pcm = np.random.RandomState(seed).randint(-2000, 2000, size=(seconds * SR, 1)).astype(np.int64)
    return FW.encode_stream(pcm, SR, 16, FW.split_blocks(pcm.shape[0], 4096), subframe={"type": "fixed", "order": 0, "k": 10})


def _wav16(n=SR, rate=SR, ch=1):
    return WW.container(1, ch, rate, 16, 2 * ch, np.zeros((n, ch), "<i2").tobytes())


def _slot(verdict=None):
    s = ManyEngine().create_slot(80, 5)
    if not hasattr(s, "lock"):
        s.lock = threading.Lock()
    if verdict:
        s.verdict = verdict
    return s


def test_the_kind_of_each_file_is_the_one_put_audio_chooses():
    s = _slot()
    mulaw = WW.write_g711(WW.speech_like(8000, 1), 8000, WW.TAG_MULAW)
    wave = np.zeros(SR // 2, np.float32)
    odd = _wav16(4410, 44101)                                      # a rate the resampler does not serve: the host route, alone
    audios = [_flac(1), mulaw, _wav16(SR, 44100, 2), wave, odd, np.zeros(0, np.float32)]
    out = B._put_audio_many(_Model, s, audios, list(range(10, 16)))
    puts = [c for c in s.calls if c[0].startswith("put") or c[0] == "pcm_put"]
    assert puts[0] == ("put_many", 10, ["flac", "wav", "frames", "pcm"])
    assert puts[1:] == [("pcm_put", 14, 1600)]                     # the odd rate: resampled on the host, uploaded as a waveform
    assert [o[0] for o in out] == [2 * SR, SR, SR * SR // 44100, SR // 2, 1600, 0]
    assert all(o[2] for o in out) and out[3][1] is wave and callable(out[0][1])


def test_a_refused_entry_falls_back_alone_and_a_damaged_one_costs_only_itself():
    flac_a, flac_b = _flac(1, 1), _flac(1, 2)
    s = _slot(lambda kind, data: L.ERR_ARG if data is flac_a else L.ERR_DATA if data is flac_b else None)
    wave = np.zeros(SR, np.float32)
    out = B._put_audio_many(_Model, s, [wave, flac_a, flac_b, wave], [4, 5, 6, 7])
    puts = [c for c in s.calls if c[0].startswith("put") or c[0] == "pcm_put"]
    assert puts == [("put_many", 4, ["pcm", "flac", "flac", "pcm"]), ("put_flac", 5, 2 * SR)]      # the refused file took its own route
    assert out[0][0] == out[3][0] == SR and out[1][0] == 2 * SR
    assert isinstance(out[2], ValueError) and "damaged FLAC stream" in str(out[2])


def test_more_than_64_entries_are_cut_into_calls_and_runs_follow_the_items():
    s = _slot()
    waves = [np.zeros(160 + k, np.float32) for k in range(70)]
    out = B._put_audio_many(_Model, s, waves, list(range(70)))
    assert [(c[1], len(c[2])) for c in s.calls if c[0] == "put_many"] == [(0, 64), (64, 6)]
    assert [o[0] for o in out] == [160 + k for k in range(70)]
    s = _slot()
    B._put_audio_many(_Model, s, waves[:4], [3, 4, 8, 9])          # items that are not neighbours: one call per run
    assert [(c[1], len(c[2])) for c in s.calls if c[0] == "put_many"] == [(3, 2), (8, 2)]


def test_engine_slot_put_many_cuts_more_than_64_entries_into_calls():
    from whisperlive_amd import engine as E
    seen = []

    class Lib:
        @staticmethod
        def wlx_pcm_put_many(h, sid, first, n, arr, res):
            seen.append((first, n, [arr[k].kind for k in range(n)][:2], arr[0].n))
            for k in range(n):
                res[k].status, res[k].n_out = (L.ERR_ARG, 0) if first + k == 65 else (0, arr[k].n)
            return 0

    s = E.Slot.__new__(E.Slot)
    s.engine, s.sid, s.lib, s.pcm_longest = type("Eng", (), {"_h": None})(), 0, Lib, 480000
    out = s.put_many([("pcm", np.zeros(500000 + k, np.float32)) for k in range(66)], first_item=0)
    assert [x[:2] for x in seen] == [(0, 64), (64, 2)] and seen[1][3] == 500064
    assert out[0] == (500000, None) and isinstance(out[65], L.WlxError) and out[65].code == L.ERR_ARG and out[64] == (500064, None)
    assert s.pcm_longest == 500065                                 # `_grew` as the single routes: the request, served or not
    with pytest.raises(ValueError):
        s.put_many([("mp3", b"")])


# ---------------------------------------------------------------------------------------------------------------- the job
def _model(engine_type, max_batch=6):
    eng = engine_type(WhisperSpec(80, 128, 2, 1, 1, 512, 2310))
    eng.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(eng.spec.vocab), max_batch=max_batch), eng


def _puts(eng):
    return [c[:2] for c in eng.slots[0].calls if c[0].startswith("put") or c[0] == "pcm_put"]


def test_wave_put_makes_one_put_many_per_wave_and_the_same_results():
    audios = [np.full(SR + 160 * i, 0.01, np.float32) for i in range(5)]
    hip, eng = _model(ManyEngine, max_batch=4)
    got = list(BatchedInferencePipeline(hip).iter_many(audios, batch_size=2, wave_put=True, **KW))
    assert _puts(eng) == [("put_many", 2)] * 3                     # waves of two, two and one file, behind the group's two items
    assert [c[2] for c in eng.slots[0].calls if c[0] == "put_many"] == [["pcm", "pcm"], ["pcm", "pcm"], ["pcm"]]
    hip2, eng2 = _model(ManyEngine, max_batch=4)
    want = list(BatchedInferencePipeline(hip2).iter_many(audios, batch_size=2, **KW))
    assert _puts(eng2) == [("pcm_put", 2), ("pcm_put", 3), ("pcm_put", 2), ("pcm_put", 3), ("pcm_put", 2)]     # the default: today's sequence
    assert [g[0] for g in got] == [w[0] for w in want] == [0, 1, 2, 3, 4]
    for g, w in zip(got, want):
        assert [(s.id, s.tokens, s.start, s.end, s.text) for s in g[1]] == [(s.id, s.tokens, s.start, s.end, s.text) for s in w[1]]
        assert g[2].duration == w[2].duration


def test_a_slot_without_put_many_keeps_the_per_file_puts():
    audios = [np.full(SR + 160 * i, 0.01, np.float32) for i in range(3)]
    hip, eng = _model(FrontEndEngine, max_batch=4)
    got = BatchedInferencePipeline(hip).transcribe_many(audios, batch_size=2, wave_put=True, **KW)
    assert _puts(eng) == [("pcm_put", 2), ("pcm_put", 3), ("pcm_put", 2)] and all(len(segs) == 1 for segs, _ in got)


def test_a_damaged_file_of_a_wave_put_costs_only_itself_and_raise_raises():
    good, bad = _flac(2, seed=1), _flac(2, seed=2)
    hip, eng = _model(ManyEngine)
    eng.slot_type.verdict = staticmethod(lambda kind, data: L.ERR_DATA if data is bad else None)
    try:
        pipe = BatchedInferencePipeline(hip)
        got = list(pipe.iter_many([good, bad, good], batch_size=2, wave_put=True, **KW))
        assert [g[0] for g in got] == [0, 1, 2] and isinstance(got[1][1], ValueError) and got[1][2] is None
        assert len(got[0][1]) == len(got[2][1]) == 1
        with pytest.raises(ValueError):
            list(pipe.iter_many([good, bad, good], batch_size=2, wave_put=True, on_error="raise", **KW))
    finally:
        eng.slot_type.verdict = staticmethod(lambda kind, data: None)


def test_the_rest_flag_reaches_the_job(monkeypatch):
    from whisperlive_amd import rest
    made = []

    class Recorder:
        def __init__(self, *a, **kw):
            made.append(kw)

        def serve_forever(self):
            pass

    monkeypatch.setattr(rest, "RestServer", Recorder)
    rest.main(["--port", "0", "--file_batch_size", "4", "--file_batch_window_ms", "200", "--file_batch_wave_put"])
    rest.main(["--port", "0", "--file_batch_size", "4", "--file_batch_window_ms", "200"])
    assert [kw["file_batch_wave_put"] for kw in made] == [True, False]
    seen = []

    class Pipe:
        def iter_many(self, audios, **kw):
            seen.append(kw.get("wave_put", "absent"))
            return iter([(i, [], object()) for i in range(len(audios))])

    for flag in (True, False):
        b = rest.FileBatcher(lambda t: Pipe(), 2, 0.0, wave_put=flag)
        try:
            b.submit(object(), b"x", {"language": None, "initial_prompt": None, "hotwords": None}, {})
        finally:
            b.close()
    assert seen == [True, "absent"]                                # off: the call of before, keyword for keyword
