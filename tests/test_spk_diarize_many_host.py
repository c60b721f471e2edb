"""CPU: the host side of diarizing a wave of files in one call — diarization.plan_diarize_many on each cap, FileDiarizer.diarize_many on
a scripted embedder with and without the wave call, BatchedInferencePipeline.transcribe_many(diarize=...) on the scripted slots of
tests/fakes.py, and the REST batcher, which now takes a `diarize=true` upload and still leaves one with known speakers out."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from tests.fakes import FrontEndEngine
from tests.test_rest import FILE, Served, _clean_model_cache, _segments, _verbose  # noqa: F401  (the fixture is autouse)
from whisperlive_amd import _lib
from whisperlive_amd import file_diarization as FD
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.diarization import plan_diarize_many
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP
from whisperlive_amd.types import TranscriptionInfo, TranscriptionOptions

SR = 16000


# ------------------------------------------------------------------------------------------------------------ the plan
def test_plan_on_the_file_cap():
    assert plan_diarize_many([3] * 64) == [list(range(64))]                                   # the boundary itself
    assert plan_diarize_many([3] * 65) == [list(range(64)), [64]]                             # one past it
    assert plan_diarize_many([3] * 130, max_files=64) == [list(range(64)), list(range(64, 128)), [128, 129]]
    assert plan_diarize_many([]) == []
    assert _lib.SPK_MANY_MAX_FILES == 64 and _lib.SPK_MANY_MAX_ROWS == 8192 and _lib.SPK_MANY_MAX_CELLS == 4 * 2048 * 2048


def test_plan_on_the_row_cap():
    assert plan_diarize_many([2048] * 4) == [[0, 1, 2, 3]]                                    # 8192 windows: the boundary
    assert plan_diarize_many([2048] * 4 + [1]) == [[0, 1, 2, 3], [4]]                         # one window past it
    assert plan_diarize_many([2048, 2048, 2048, 2047, 1, 1]) == [[0, 1, 2, 3, 4], [5]]
    # short windows count as rows, not as cells
    assert plan_diarize_many([2048] * 5, [0] * 5) == [[0, 1, 2, 3], [4]]
    assert plan_diarize_many([10, 10, 10], max_rows=20) == [[0, 1], [2]] and plan_diarize_many([10, 10, 1], max_rows=21) == [[0, 1, 2]]


def test_plan_on_the_matrix_cap():
    # 3^2 + 4^2 = 25: the boundary, and one float past it
    assert plan_diarize_many([3, 4, 1], max_cells=26) == [[0, 1, 2]]
    assert plan_diarize_many([3, 4], max_cells=25) == [[0, 1]] and plan_diarize_many([3, 4], max_cells=24) == [[0], [1]]
    assert plan_diarize_many([5, 5], [3, 4], max_cells=25) == [[0, 1]]                        # the windows that take part, squared
    # under the library's own caps the rows close a call no later than the matrices do: four files at the cap are both boundaries
    assert plan_diarize_many([2048] * 8) == [[0, 1, 2, 3], [4, 5, 6, 7]]


def test_plan_keeps_the_order_and_refuses_what_fits_no_call():
    calls = plan_diarize_many([1500, 900, 2048, 7, 2048, 2048, 2048, 3, 1])
    assert [f for c in calls for f in c] == list(range(9)) and all(c == list(range(c[0], c[-1] + 1)) for c in calls)
    assert all(sum([1500, 900, 2048, 7, 2048, 2048, 2048, 3, 1][f] for f in c) <= 8192 for c in calls)
    for bad in ([2049], [3, -1]):
        with pytest.raises(ValueError):
            plan_diarize_many(bad)
    with pytest.raises(ValueError):
        plan_diarize_many([3, 3], [3, 4])                                                     # more take part than there are
    with pytest.raises(ValueError):
        plan_diarize_many([3, 3], [3])


# ------------------------------------------------------------------------------------------------------------ FileDiarizer
def script_labels(windows, boundaries, cap):
    """the label of a window is the number of boundaries at or before its centre, renumbered by first appearance; a cap of K folds
    the labels from K on into K - 1"""
    raw = [sum((s + n / 2.0) / SR >= b for b in boundaries) if n >= 4800 else -1 for s, n in windows]
    if cap:
        raw = [min(r, cap - 1) for r in raw]
    order = []
    for r in raw:
        if r >= 0 and r not in order:
            order.append(r)
    return np.array([order.index(r) if r >= 0 else -1 for r in raw], np.int32), np.eye(8, dtype=np.float32)[: len(order)]


class OneByOne:
    """diarize_resident alone, boundaries per item"""

    def __init__(self, boundaries):
        self.boundaries, self.calls = boundaries, []

    def diarize_resident(self, slot, item, windows, threshold, max_clusters=0):
        self.calls.append(("one", item, len(windows), max_clusters))
        return script_labels(windows, self.boundaries[item], max_clusters)


class Wave(OneByOne):
    """the same with the wave call"""

    def diarize_many(self, slot, items, windows_per_file, thresholds, max_clusters=0):
        caps = [max_clusters] * len(items) if np.isscalar(max_clusters) else list(max_clusters)
        self.calls.append(("many", list(items), [len(w) for w in windows_per_file], caps))
        return [script_labels(w, self.boundaries[i], c) for i, w, c in zip(items, windows_per_file, caps)]


def test_file_diarizer_many_equals_the_loop():
    slot = object()
    residents = [SimpleNamespace(slot=slot, item=i, n_samples=n * SR) for i, n in ((4, 10), (5, 6), (6, 20), (7, 3))]
    spans = [[(0.0, 6.0), (7.0, 12.0)], [(0.5, 5.5)], [], [(1.0, 1.1)]]          # past the end, plain, no span, a span with no window
    boundaries = {4: [4.0, 8.5], 5: [2.0], 6: [], 7: []}
    wave, loop = Wave(boundaries), OneByOne(boundaries)
    d_wave, d_loop = FD.FileDiarizer(wave, max_speakers=4), FD.FileDiarizer(loop, max_speakers=4)
    want = [d_loop.diarize(r, s) for r, s in zip(residents, spans)]
    assert FD.speakers_in_order(want[0]) == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_02"] and want[2] == [] and want[3] == []
    assert d_wave.diarize_many(residents, spans) == want
    assert [c[0] for c in wave.calls] == ["many"] and wave.calls[0][1] == [4, 5] and wave.calls[0][3] == [4, 4]      # ONE call, the files with windows
    assert d_loop.diarize_many(residents, spans) == want                                       # no wave call on the embedder: the loop
    # a cap per file in place of the diarizer's own
    capped = d_wave.diarize_many(residents, spans, max_speakers=[2, None, 0, 0])
    assert wave.calls[-1][3] == [2, 4] and FD.speakers_in_order(capped[0]) == ["SPEAKER_00", "SPEAKER_01"] and capped[1] == want[1]
    assert d_loop.diarize_many(residents, spans, max_speakers=[2, None, 0, 0]) == capped
    # known speakers name the clusters, as in diarize
    known = {"ann": np.eye(8, dtype=np.float32)[1] * 2}
    assert d_wave.diarize_many(residents, spans, known=known) == [d_loop.diarize(r, s, known=known) for r, s in zip(residents, spans)]
    # a file over the device's window cap keeps the host route of cluster_windows; the others still share the wave call
    d_wave.window_s, d_wave.hop_s = 0.3, 0.009
    huge = [SimpleNamespace(slot=slot, item=6, n_samples=20 * SR), residents[1]]
    n = len(d_wave.windows_of(huge[0], [(0.0, 20.0)]))
    assert n > _lib.SPK_CLUSTER_MAX
    wave.calls.clear()
    wave.embed_resident = lambda s, i, ranges: [np.eye(8, dtype=np.float32)[0] for _ in ranges]
    got = d_wave.diarize_many(huge, [[(0.0, 20.0)], [(0.5, 5.5)]])
    assert [c[0] for c in wave.calls] == ["many"] and wave.calls[0][1] == [5] and [t[2] for t in got[0]] == ["SPEAKER_00"]
    # the switch for a case where the wave call does not pay
    d_wave.window_s, d_wave.hop_s, d_wave.many_on_device = 1.5, 0.75, False
    wave.calls.clear()
    assert d_wave.diarize_many(residents, spans) == want and [c[0] for c in wave.calls] == ["one", "one"]
    with pytest.raises(ValueError):
        d_wave.diarize_many(residents, spans[:2])


# ------------------------------------------------------------------------------------------------------------ transcribe_many
def _model(max_batch=6):
    eng = FrontEndEngine(WhisperSpec(80, 128, 2, 1, 1, 512, 2310))
    eng.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(eng.spec.vocab), max_batch=max_batch), eng


CLIPS = [{"start": 0, "end": SR}, {"start": SR, "end": 2 * SR}]
KW = dict(language="en", vad_filter=False, clip_timestamps=CLIPS, chunk_length=1)


class ByItem(Wave):
    """every item changes speaker at 1.0 s"""

    def __init__(self):
        super().__init__(None)
        self.boundaries = type("B", (), {"__getitem__": lambda s, i: [1.0]})()


def test_transcribe_many_puts_speakers_on_segments():
    hip, eng = _model(max_batch=4)
    emb = ByItem()
    pipe = BatchedInferencePipeline(hip)
    pipe.file_diarizer = FD.FileDiarizer(emb)                       # what diarize=True stands for
    audios = [np.full(2 * SR, 0.1 * (i + 1), np.float32) for i in range(5)]
    plain = pipe.transcribe_many(audios, batch_size=2, **KW)
    seen = []
    for index, segments, info in pipe.iter_many(audios, batch_size=2, diarize=True, **KW):
        seen.append((index, len([c for c in emb.calls if c[0] == "many"]), len([c for c in eng.slots[0].calls if c[0] == "encode"])))
        assert [s.speaker for s in segments] == ["SPEAKER_00", "SPEAKER_01"] and info.speakers == ["SPEAKER_00", "SPEAKER_01"]
        want = plain[index][0]                                       # nothing else changed
        assert [(s.id, s.start, s.end, s.text, s.tokens) for s in segments] == [(s.id, s.start, s.end, s.text, s.tokens) for s in want]
    # waves of two files: input order, each wave behind its last decode group and its ONE diarize_many call
    assert [x[0] for x in seen] == [0, 1, 2, 3, 4] and [x[1] for x in seen] == [1, 1, 2, 2, 3]
    assert seen[0][2] == seen[1][2] and seen[2][2] == seen[3][2] and seen[1][2] < seen[2][2] < seen[4][2]
    many = [c for c in emb.calls if c[0] == "many"]
    assert [c[1] for c in many] == [[2, 3], [2, 3], [2]] and not [c for c in emb.calls if c[0] == "one"]      # the files' items, behind the group's
    assert not hasattr(plain[0][0][0], "speaker")                   # without diarize nothing is added


def test_words_take_the_turn_they_overlap_and_the_segment_the_speaker_of_most_of_them():
    """the labelling step of a wave on segments with word times (the scripted slots align nothing): `.speaker` on every word by
    file_diarization.label_segments, as rest.diarize_file_segments answers for one file"""
    from whisperlive_amd import many_files as MF
    from whisperlive_amd.types import Segment, Word
    seg = lambda a, b, words: Segment(1, 0, a, b, "x", [1], 0.0, 1.0, 0.0, words=words)
    segments = [seg(0.0, 2.0, [Word(0.1, 0.6, " a", 1.0), Word(1.2, 1.9, " b", 1.0), Word(1.9, 1.9, " c", 1.0)]), seg(2.5, 3.5, None)]
    f = MF._File(0, {}, None, 3, FD.FileDiarizer(ByItem()), None)
    f.segments, f.n_samples, f.info = segments, 4 * SR, SimpleNamespace()
    MF._speakers(SimpleNamespace(), [f])
    assert [w.speaker for w in segments[0].words] == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_01"]      # (a word of no duration: its segment's)
    assert segments[0].speaker == "SPEAKER_01" and segments[1].speaker == "SPEAKER_01" and f.info.speakers == ["SPEAKER_00", "SPEAKER_01"]
    turns = f.diarizer.diarize(SimpleNamespace(slot=None, item=3, n_samples=4 * SR), FD.merge_spans(segments))
    assert FD.label_segments(segments, turns)[0] == [s.speaker for s in segments]


def test_transcribe_many_max_speakers_per_file_and_a_failed_file(tmp_path):
    hip, eng = _model(max_batch=6)
    emb = ByItem()
    pipe = BatchedInferencePipeline(hip)
    d = FD.FileDiarizer(emb, max_speakers=0)
    audios = [np.zeros(2 * SR, np.float32), str(tmp_path / "missing.wav"), np.zeros(2 * SR, np.float32), np.zeros(2 * SR, np.float32)]
    got = list(pipe.iter_many(audios, batch_size=2, diarize=d, max_speakers=[1, 0, None, 2], **KW))
    assert [g[0] for g in got] == [0, 1, 2, 3]
    assert isinstance(got[1][1], OSError) and got[1][2] is None     # the failed file still yields (index, exception, None)
    assert [s.speaker for s in got[0][1]] == ["SPEAKER_00", "SPEAKER_00"] and got[0][2].speakers == ["SPEAKER_00"]          # capped at one
    assert [s.speaker for s in got[2][1]] == ["SPEAKER_00", "SPEAKER_01"] and [s.speaker for s in got[3][1]] == ["SPEAKER_00", "SPEAKER_01"]
    assert [c for c in emb.calls if c[0] == "many"][0][3] == [1, 0, 2]
    # a list per file: only the named files are diarized, the wave still leaves together
    emb.calls.clear()
    got = pipe.transcribe_many(audios[:1] + audios[2:], batch_size=2, diarize=[False, d, False], **KW)
    assert not hasattr(got[0][0][0], "speaker") and [s.speaker for s in got[1][0]] == ["SPEAKER_00", "SPEAKER_01"]
    assert [c[1] for c in emb.calls] == [[3]]
    # an embedder without the wave call: the loop, the same speakers
    loop = OneByOne(emb.boundaries)
    got = pipe.transcribe_many(audios[2:], batch_size=2, diarize=FD.FileDiarizer(loop), **KW)
    assert [[s.speaker for s in g[0]] for g in got] == [["SPEAKER_00", "SPEAKER_01"]] * 2 and [c[0] for c in loop.calls] == ["one", "one"]
    for bad in (dict(diarize=[d]), dict(diarize=d, max_speakers=[1]), dict(diarize=d, max_speakers=-1), dict(diarize="yes")):
        with pytest.raises(ValueError):
            pipe.transcribe_many(audios[2:], batch_size=2, **bad, **KW)


# ------------------------------------------------------------------------------------------------------------ the REST batcher
class _Transcriber:
    def __init__(self):
        self.released = 0

    def release_slot(self):
        self.released += 1

    def transcribe(self, data, **kw):
        return _segments(), _info(kw.get("language") or "en")

    def resident_file_audio(self, channel=None):
        return SimpleNamespace(slot="slot", item=0, n_samples=3728 * SR)


def _info(language="de"):
    return TranscriptionInfo(language=language, language_probability=1.0, duration=3727.125, duration_after_vad=3727.125,
                             all_language_probs=None, transcription_options=TranscriptionOptions(), vad_options=None)


class _Pipeline:
    """iter_many labels its files through the diarizers it is handed, on a resident handle of its own; transcribe is the unpooled route"""
    log: list = []

    def __init__(self, transcriber):
        self.t = transcriber

    def transcribe(self, data, **kw):
        self.log.append(("transcribe", kw))
        return _segments(), _info(kw.get("language") or "en")

    def iter_many(self, audios, **kw):
        self.log.append(("iter_many", len(audios), kw))
        for i in range(len(audios)):
            segments, info = _segments(), _info(kw["language"][i] or "en")
            d = kw.get("diarize", [False] * len(audios))[i]
            if d:
                turns = d.diarize_many([self.t.resident_file_audio()], [FD.merge_spans(segments)], max_speakers=[kw["max_speakers"][i]])[0]
                per_seg, per_word = FD.label_segments(segments, turns)
                for seg, who, words in zip(segments, per_seg, per_word):
                    seg.speaker = who
                    for w, ww in zip(seg.words, words):
                        w.speaker = ww
                info.speakers = FD.speakers_in_order(turns)
            yield i, segments, info


def test_the_batcher_takes_a_diarize_request_and_leaves_known_speakers_out():
    emb = Wave({0: [100.0]})
    _Pipeline.log = []
    base = [FILE, ("response_format", "verbose_json"), ("language", "de"), ("timestamp_granularities", "word")]
    kw = dict(embedder_factory=lambda path, device: emb, model_factory=lambda model, device, max_batch=1: _Transcriber(), pipeline_factory=_Pipeline)
    with Served(**kw) as s:                                          # the unpooled answer: the yardstick, byte for byte
        st, _, unpooled = s.post(base + [("diarize", "true"), ("max_speakers", "3")])
        assert st == 200 and json.loads(unpooled)["speakers"] == ["SPEAKER_00", "SPEAKER_01"]
    emb.calls.clear()
    _Pipeline.log = []
    with Served(file_batch_size=2, file_batch_window_ms=5, **kw) as s:
        st, _, body = s.post(base + [("diarize", "true"), ("max_speakers", "3")])
        assert st == 200 and s.server.batcher.jobs == 1 and body == unpooled
        name, n, job = _Pipeline.log[-1]
        assert name == "iter_many" and n == 1 and job["max_speakers"] == [3] and isinstance(job["diarize"][0], FD.FileDiarizer)
        assert emb.calls[-1][0] == "many" and emb.calls[-1][3] == [3]
        got = json.loads(body)
        assert [g["speaker"] for g in got["segments"]] == ["SPEAKER_00", "SPEAKER_01"]
        assert [[w["speaker"] for w in g["words"]] for g in got["segments"]] == [["SPEAKER_00", "SPEAKER_00"], ["SPEAKER_01"]]
        # a second request shares the GPU's pooled diarizer: one diarize_many job per wave needs one diarizer
        assert s.post(base + [("diarize", "true")])[0] == 200 and _Pipeline.log[-1][2]["diarize"][0] is job["diarize"][0]
        assert _Pipeline.log[-1][2]["max_speakers"] == [0] and s.server.batcher.jobs == 2
        # without diarize the job carries neither keyword, and the answer is today's
        st, _, body = s.post(base)
        assert st == 200 and "diarize" not in _Pipeline.log[-1][2] and json.loads(body) == _verbose(True) and s.server.batcher.jobs == 3
        # known speakers: not pooled, with or without diarize
        for extra in ([("known_speaker_names", "ann")], [("known_speaker_names", "ann"), ("diarize", "true")]):
            st, _, body = s.post(base + extra)
            assert st == 200 and _Pipeline.log[-1][0] == "transcribe" and s.server.batcher.jobs == 3
