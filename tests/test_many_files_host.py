"""CPU: the host logic of BatchedInferencePipeline.transcribe_many (whisperlive_amd/many_files.py) on scripted slots (tests/fakes.py),
and the REST batcher that pools concurrent uploads into its jobs (rest.FileBatcher) on a scripted pipeline."""
import inspect
import json
import os
import threading

import numpy as np
import pytest

from tests.fakes import FrontEndEngine
from whisperlive_amd import many_files as MF
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

from . import flac_writer as W

SR = 16000
KW = dict(language="en", vad_filter=False, clip_timestamps=[{"start": 0, "end": SR}])


def _model(max_batch=6):
    eng = FrontEndEngine(WhisperSpec(80, 128, 2, 1, 1, 512, 2310))
    eng.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(eng.spec.vocab), max_batch=max_batch), eng


def _flac(seconds=2, seed=0):
    pcm = np.random.RandomState(seed).randint(-2000, 2000, size=(seconds * SR, 1)).astype(np.int64)
    return W.encode_stream(pcm, SR, 16, W.split_blocks(pcm.shape[0], 4096), subframe={"type": "fixed", "order": 0, "k": 10})


# ---------------------------------------------------------------------------------------------------------------- waves
def test_a_wave_holds_max_batch_minus_batch_size_files_in_input_order():
    assert MF.plan_waves([10, 30, 20, 50, 40, 60, 5], batch_size=4, max_batch=7) == [[0, 1, 2], [3, 4, 5], [6]]
    assert MF.plan_waves([], 4, 8) == []


def test_the_byte_budget_closes_a_wave_early_and_an_oversized_file_runs_alone():
    # (files + batch_size) x longest x 4 bytes against a budget of 4000: two files of 100 samples with batch_size 2 are 1600, a third
    # makes 2000; a file of 300 would make the wave (3 + 2) x 300 x 4 = 6000
    assert MF.plan_waves([100, 100, 300, 100], 2, 10, budget=4000) == [[0, 1], [2], [3]]
    # a file that alone passes the budget is a wave of one, and the order is kept around it
    assert MF.plan_waves([10, 5000, 10, 10], 2, 10, budget=4000) == [[0], [1], [2, 3]]
    assert MF.WAVE_PCM_BUDGET == 4 << 30


def test_a_wave_is_closed_where_its_rows_would_pass_what_the_chunk_gather_addresses():
    hour = 3600 * SR                                    # 57.6e6 samples: 37 rows of it are 2.13e9 <= 2^31 - 1, 38 are not
    waves = MF.plan_waves([hour] * 40, 2, 64, budget=1 << 60)
    assert [len(w) for w in waves] == [37, 3]


def test_a_batch_size_that_leaves_no_room_is_refused_in_the_words_of_check_batch():
    hip, _ = _model(max_batch=4)
    with pytest.raises(ValueError, match=r"batch_size 4 exceeds max_batch 4 - 1 file = 3 .*max_batch >= 5 or lower batch_size"):
        BatchedInferencePipeline(hip).transcribe_many([np.zeros(SR, np.float32)], batch_size=4, **KW)


def test_resident_samples_reads_the_header():
    assert MF.resident_samples(np.zeros(1234, np.float32)) == 1234
    assert MF.resident_samples(_flac(2)) == 2 * SR
    assert MF.resident_samples(b"RIFFxxxxWAVEjunk") is None and MF.resident_samples(b"") is None       # the header does not say
    unknown = bytearray(_flac(2))
    unknown[21] &= 0xF0
    unknown[22:26] = b"\0\0\0\0"                       # STREAMINFO total_samples = 0, as streaming encoders write it
    assert MF.resident_samples(bytes(unknown)) is None


def test_a_file_of_unknown_length_runs_as_a_wave_of_one():
    assert MF.plan_waves([10, None, 10, 10], 2, 10) == [[0], [1], [2, 3]]
    assert MF.plan_waves([None, None], 2, 10) == [[0], [1]]


def test_a_long_file_keeps_the_rows_long_for_the_waves_behind_it():
    """the slot's rows never shrink: after a 50-minute file (48e6 samples a row) 48 voicemails are 48 x 48e6 = 2.3e9 > 2^31 - 1 apart,
    though their own wave would be 48 x 480000; at most 44 rows of 48e6 fit"""
    long, short = 50 * 60 * SR, 20 * SR
    waves = MF.plan_waves([long] + [short] * 48, 12, 60)
    assert [i for w in waves for i in w] == list(range(49)) and waves[0][0] == 0
    for w in waves:
        assert MF.source_rows_addressable(len(w), long) and len(w) <= 44
    assert [len(w) for w in MF.plan_waves([short] * 48, 12, 60)] == [48]                       # a fresh slot takes them as one wave
    assert [len(w) for w in MF.plan_waves([short] * 48, 12, 60, stride=long)] == [44, 4]       # a slot that held the long file does not
    assert MF.next_wave([short] * 48, 44, 12, 60, stride=long) == [44, 45, 46, 47]


def test_the_job_sizes_its_waves_from_what_the_slot_already_holds():
    hip, eng = _model(max_batch=60)
    slot = hip._slot()
    slot.pcm_longest = 50 * 60 * SR                      # an earlier call on this thread's slot put a 50-minute file there
    audios = [np.zeros(SR, np.float32)] * 48
    got = list(BatchedInferencePipeline(hip).iter_many(audios, batch_size=12, **KW))
    assert [g[0] for g in got] == list(range(48)) and all(g[2] is not None for g in got)
    items = [x[1] for x in slot.calls if x[0] == "pcm_put"]
    assert items == list(range(12, 56)) + list(range(12, 16))                                  # waves of 44 and 4 files
    for x in slot.calls:
        if x[0] == "logmel_chunks":
            assert MF.source_rows_addressable(max(x[2]) - min(x[2]) + 1, slot.pcm_longest)


def test_a_file_every_route_refuses_costs_only_itself():
    from whisperlive_amd import _lib
    hip, eng = _model()
    slot = hip._slot()
    real = slot.pcm_put

    def pcm_put(pcm, item=0):
        if len(pcm) > 3 * SR:
            e = _lib.WlxError(f"libwlx error {_lib.ERR_ARG}: audio chunk too long")
            e.code = _lib.ERR_ARG
            raise e
        if len(pcm) == 2 * SR + 1:
            e = _lib.WlxError("libwlx error 2: scripted")
            e.code = 2
            raise e
        return real(pcm, item=item)

    slot.pcm_put = pcm_put
    pipe = BatchedInferencePipeline(hip)
    out = pipe.transcribe_many([np.zeros(SR, np.float32), np.zeros(4 * SR, np.float32), np.zeros(SR, np.float32)], batch_size=2, **KW)
    assert len(out[0][0]) == 1 and len(out[2][0]) == 1
    assert isinstance(out[1][0], ValueError) and "refused" in str(out[1][0]) and out[1][1] is None
    with pytest.raises(ValueError, match="refused"):
        pipe.transcribe_many([np.zeros(SR, np.float32), np.zeros(4 * SR, np.float32)], batch_size=2, on_error="raise", **KW)
    with pytest.raises(_lib.WlxError):                   # any other device error is the job's
        pipe.transcribe_many([np.zeros(SR, np.float32), np.zeros(2 * SR + 1, np.float32)], batch_size=2, **KW)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_per_file_keyword_lists():
    a = dict(language=["en", "de", None], initial_prompt="hello", hotwords=None, prefix=None, clip_timestamps=[{"start": 0, "end": 5}], task="x")
    per = MF.per_file_arguments(a, 3)
    assert [p["language"] for p in per] == ["en", "de", None] and {p["initial_prompt"] for p in per} == {"hello"}
    assert all(p["clip_timestamps"] == [{"start": 0, "end": 5}] for p in per)           # a list of clips is one value, for every file
    per = MF.per_file_arguments({**a, "clip_timestamps": [[{"start": 0, "end": 5}], None, []], "initial_prompt": [1, 2, 3]}, 3)
    assert [p["clip_timestamps"] for p in per] == [[{"start": 0, "end": 5}], None, []]
    assert all(p["initial_prompt"] == [1, 2, 3] for p in per)                            # token ids: one prompt


@pytest.mark.parametrize("name", ["language", "initial_prompt", "hotwords", "prefix", "clip_timestamps"])
def test_a_per_file_list_of_the_wrong_length_is_a_value_error(name):
    hip, _ = _model()
    value = {"clip_timestamps": [[{"start": 0, "end": SR}]] * 2}.get(name, ["a", "b"])
    with pytest.raises(ValueError, match=f"{name}: a list of 2 entries for 3 files"):
        BatchedInferencePipeline(hip).transcribe_many([np.zeros(SR, np.float32)] * 3, batch_size=2, **{**KW, name: value})


def test_multichannel_is_refused():
    hip, _ = _model()
    with pytest.raises(ValueError, match="multichannel=True is not part of this route"):
        BatchedInferencePipeline(hip).iter_many([np.zeros((SR, 2), np.float32)], batch_size=2, multichannel=True, **KW)


def test_the_transcribe_signature_is_the_golden_one():
    with open(os.path.join(os.path.dirname(__file__), "golden", "batched_transcribe_signature.json")) as f:
        want = [tuple(x) for x in json.load(f)]
    sig = inspect.signature(BatchedInferencePipeline.transcribe)
    got = [(name, "<required>" if p.default is p.empty else p.default) for name, p in list(sig.parameters.items())[1:]]
    assert [g[0] for g in got] == [w[0] for w in want]
    for (n, g), (_n, w) in zip(got, want):
        assert g == w and type(g) is type(w), n
    # ... and the job's own entry points take the files, then keywords only
    for name in ("transcribe_many", "iter_many"):
        params = list(inspect.signature(getattr(BatchedInferencePipeline, name)).parameters.values())
        assert [p.name for p in params] == ["self", "audios", "batch_size", "on_error", "kwargs"]
        assert params[2].kind == params[3].kind == inspect.Parameter.KEYWORD_ONLY and (params[2].default, params[3].default) == (8, "return")


# ---------------------------------------------------------------------------------------------------------------- a job
def test_files_go_into_their_own_items_and_groups_mix_files():
    hip, eng = _model(max_batch=6)
    a, b, c = (np.full(2 * SR, 0.1 * (i + 1), np.float32) for i in range(3))
    clips = [{"start": 0, "end": SR}, {"start": SR, "end": 2 * SR}]
    out = BatchedInferencePipeline(hip).transcribe_many([a, b, c], batch_size=3, language="en", vad_filter=False, clip_timestamps=clips,
                                                        chunk_length=1)
    calls = eng.slots[0].calls
    assert [x for x in calls if x[0] == "pcm_put"] == [("pcm_put", 3, 2 * SR), ("pcm_put", 4, 2 * SR), ("pcm_put", 5, 2 * SR)]
    assert [x[2] for x in calls if x[0] == "logmel_chunks"] == [[3, 3, 4], [4, 5, 5]]            # six chunks in (file, start) order
    assert [x[0] for x in calls if x[0] in ("pcm_put", "logmel_chunks", "encode")] == ["pcm_put"] * 3 + ["logmel_chunks", "encode"] * 2
    for segs, info in out:
        assert [s.id for s in segs] == [1, 2] and [s.tokens for s in segs] == [[300, 301, 302]] * 2
        assert [(s.start, s.end) for s in segs] == [(0.0, 1.0), (1.0, 2.0)]
        assert info.duration == 2.0 and info.duration_after_vad == 2.0 and info.language == "en"


def test_more_files_than_a_wave_holds_come_back_in_input_order():
    hip, eng = _model(max_batch=4)
    audios = [np.zeros(SR + 160 * i, np.float32) for i in range(5)]
    got = list(BatchedInferencePipeline(hip).iter_many(audios, batch_size=2, **KW))
    assert [g[0] for g in got] == [0, 1, 2, 3, 4]
    assert [g[2].duration for g in got] == [(SR + 160 * i) / SR for i in range(5)]
    assert [x[1] for x in eng.slots[0].calls if x[0] == "pcm_put"] == [2, 3, 2, 3, 2]              # waves of two files, behind the group


def test_a_file_without_clips_yields_no_segments():
    hip, _ = _model()
    out = BatchedInferencePipeline(hip).transcribe_many(
        [np.zeros(SR, np.float32), np.zeros(SR, np.float32)], batch_size=2, language="en", vad_filter=False,
        clip_timestamps=[[{"start": 0, "end": SR}], [{"start": 5, "end": 5}]])
    assert len(out[0][0]) == 1 and out[1][0] == [] and out[1][1].duration_after_vad == 0 and out[1][1].duration == 1.0


def test_a_truncated_flac_costs_only_its_own_file():
    hip, _ = _model()
    good, bad = _flac(2, seed=1), _flac(2, seed=2)
    bad = bad[: len(bad) // 2]
    pipe = BatchedInferencePipeline(hip)
    got = list(pipe.iter_many([good, bad, good], batch_size=2, **KW))
    assert [g[0] for g in got] == [0, 1, 2]
    assert isinstance(got[1][1], ValueError) and got[1][2] is None
    single, info = pipe.transcribe(good, batch_size=2, **KW)
    single = list(single)
    for i in (0, 2):
        assert [(s.id, s.tokens, s.start, s.end, s.text) for s in got[i][1]] == [(s.id, s.tokens, s.start, s.end, s.text) for s in single]
        assert got[i][2].duration == info.duration == 2.0
    with pytest.raises(ValueError):
        list(pipe.iter_many([good, bad, good], batch_size=2, on_error="raise", **KW))


def test_an_unreadable_path_costs_only_its_own_file(tmp_path):
    hip, _ = _model()
    out = BatchedInferencePipeline(hip).transcribe_many([np.zeros(SR, np.float32), str(tmp_path / "missing.wav")], batch_size=2, **KW)
    assert len(out[0][0]) == 1 and isinstance(out[1][0], OSError) and out[1][1] is None


# ---------------------------------------------------------------------------------------------------------------- the REST batcher
class _Pipeline:
    """scripted pipeline: records every job; `gate` (an Event) holds a job until the test lets it go"""

    def __init__(self, log, gate=None):
        self.log, self.gate = log, gate

    def iter_many(self, audios, **kw):
        self.log.append((list(audios), kw))
        if self.gate is not None:
            self.gate.wait(10)
        for i, data in enumerate(audios):
            if data == b"bad":
                yield i, ValueError("damaged"), None
            else:
                yield i, [data.decode()], {"language": kw["language"][i]}


def _submit_all(batcher, uploads):
    """every upload from its own thread -> results (or the exception raised) in upload order"""
    out = [None] * len(uploads)

    def one(i, data, per_file, shared):
        try:
            out[i] = batcher.submit("transcriber", data, per_file, shared)
        except Exception as e:  # noqa: BLE001
            out[i] = e

    threads = [threading.Thread(target=one, args=(i, *u)) for i, u in enumerate(uploads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(20)
    return out


def _per_file(language):
    return dict(language=language, initial_prompt=None, hotwords=None)


def test_uploads_with_equal_options_inside_the_window_form_one_job():
    from whisperlive_amd.rest import FileBatcher
    log = []
    # the window closes as soon as batch_size uploads of one key wait: nothing here waits for a timer
    b = FileBatcher(lambda tr: _Pipeline(log), batch_size=3, window_s=30.0)
    try:
        shared = dict(temperature=0.0, word_timestamps=False)
        got = _submit_all(b, [(b"a", _per_file("en"), shared), (b"bad", _per_file("de"), shared), (b"c", _per_file(None), dict(shared))])
    finally:
        b.close()
    assert b.jobs == 1 and len(log) == 1
    audios, kw = log[0]
    assert sorted(audios) == [b"a", b"bad", b"c"] and kw["batch_size"] == 3 and kw["vad_filter"] is True
    assert sorted(kw["language"], key=str) == sorted(["en", "de", None], key=str) and kw["temperature"] == 0.0
    assert got[0] == (["a"], {"language": "en"}) and got[2] == (["c"], {"language": None})      # each request from its own result
    assert isinstance(got[1], ValueError)                                                      # ... or its own error


def test_different_beam_sizes_form_two_jobs():
    from whisperlive_amd.rest import FileBatcher
    log = []
    b = FileBatcher(lambda tr: _Pipeline(log), batch_size=2, window_s=30.0)
    try:
        got = _submit_all(b, [(b"a", _per_file("en"), dict(beam_size=5)), (b"b", _per_file("en"), dict(beam_size=1)),
                              (b"c", _per_file("en"), dict(beam_size=5)), (b"d", _per_file("en"), dict(beam_size=1))])
    finally:
        b.close()
    assert b.jobs == 2
    assert sorted((sorted(audios), kw["beam_size"]) for audios, kw in log) == [([b"a", b"c"], 5), ([b"b", b"d"], 1)]
    assert [g[0] for g in got] == [["a"], ["b"], ["c"], ["d"]]


class _Transcriber:
    max_batch = 8

    def release_slot(self):
        pass


def _server(**kw):
    from whisperlive_amd.rest import RestServer
    log = []

    class Pipe(_Pipeline):
        def transcribe(self, data, **k):
            self.log.append(("transcribe", data, k))
            return [], None

    return RestServer("127.0.0.1", 0, "fake", model_factory=lambda m, d, **k: _Transcriber(), pipeline_factory=lambda tr: Pipe(log), **kw), log


def test_window_zero_never_constructs_the_worker():
    server, _ = _server(file_batch_size=4)
    assert server.batcher is None and server.file_batch_window_ms == 0
    assert not [t for t in threading.enumerate() if t.name == "wlx-rest-batcher"]
    with pytest.raises(ValueError, match="file_batch_window_ms needs file_batch_size"):
        _server(file_batch_size=0, file_batch_window_ms=50)


def test_a_refused_constructor_leaves_no_worker_behind():
    with pytest.raises(ValueError, match="devices"):
        _server(file_batch_size=4, file_batch_window_ms=50, devices=[-1])
    assert not [t for t in threading.enumerate() if t.name == "wlx-rest-batcher"]
    server, _ = _server(file_batch_size=4, file_batch_window_ms=50, devices=[0, 1])         # one worker per GPU
    try:
        assert len([t for t in threading.enumerate() if t.name == "wlx-rest-batcher"]) == 2 and server.batcher is server._batchers[0]
    finally:
        server.shutdown()
    assert not [t for t in threading.enumerate() if t.name == "wlx-rest-batcher"]


def test_the_command_line_carries_both_flags(monkeypatch):
    from whisperlive_amd import rest
    made = []

    class Recorder:
        def __init__(self, *a, **kw):
            made.append((a, kw))

        def serve_forever(self):
            pass

    monkeypatch.setattr(rest, "RestServer", Recorder)
    rest.main(["--port", "0", "--file_batch_size", "4", "--file_batch_window_ms", "200"])
    rest.main(["--port", "0", "--file_batch_size", "4"])
    assert [(kw["file_batch_size"], kw["file_batch_window_ms"]) for _a, kw in made] == [(4, 200), (4, 0)]


def test_a_streamed_request_bypasses_the_worker():
    import http.client
    from whisperlive_amd.rest import ROUTE
    from whisperlive_amd.serve_client import ServeClientHIP
    server, log = _server(file_batch_size=2, file_batch_window_ms=30000)
    saved = dict(ServeClientHIP.MODELS)
    ServeClientHIP.MODELS.clear()
    server.start()
    try:
        bd = "hostmany"
        body = (f'--{bd}\r\nContent-Disposition: form-data; name="file"; filename="a.wav"\r\n\r\n'.encode() + b"RIFFdata"
                + f'\r\n--{bd}\r\nContent-Disposition: form-data; name="stream"\r\n\r\ntrue\r\n--{bd}--\r\n'.encode())
        c = http.client.HTTPConnection("127.0.0.1", server.port, timeout=20)
        c.request("POST", ROUTE, body, {"Content-Type": f"multipart/form-data; boundary={bd}"})
        r = c.getresponse()
        text = r.read().decode()
        c.close()
        assert r.status == 200 and "[DONE]" in text
        assert [x[0] for x in log] == ["transcribe"] and server.batcher.jobs == 0          # the pipeline alone, not a pooled job
    finally:
        server.shutdown()
        ServeClientHIP.MODELS.clear()
        ServeClientHIP.MODELS.update(saved)
