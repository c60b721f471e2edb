"""Host logic of multichannel transcription (no GPU): pooling, ordering and ids, the batch check, the language channel, the REST
renderings and form parsing, Segment's new last field, and the bindings of the four new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from whisperlive_amd import multichannel as M
from whisperlive_amd.types import Segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seg(start, channel, text="x", **kw):
    return Segment(id=0, seek=0, start=start, end=start + 1.0, text=text, tokens=[1], avg_logprob=-0.1, compression_ratio=1.0,
                   no_speech_prob=0.0, channel=channel, **kw)


def test_pooling_is_in_channel_then_start_order():
    per = [([[(0, 10)], [(20, 30), (30, 35)]], [{"start_time": 0.0}, {"start_time": 1.0}]),
           ([], []),
           ([[(5, 9)]], [{"start_time": 0.0}])]
    ranges, meta, channels = M.pool_chunks(per)
    assert ranges == [[(0, 10)], [(20, 30), (30, 35)], [(5, 9)]] and channels == [0, 0, 2]
    assert meta == [{"start_time": 0.0}, {"start_time": 1.0}, {"start_time": 0.0}]


def test_segments_are_sorted_by_start_then_channel_and_numbered():
    segs = [_seg(0.0, 0, "a0"), _seg(2.5, 0, "a1"), _seg(0.0, 1, "b0"), _seg(1.0, 1, "b1"), _seg(2.5, 1, "b2")]
    out = M.order_segments(segs)
    assert [(s.text, s.id) for s in out] == [("a0", 1), ("b0", 2), ("b1", 3), ("a1", 4), ("b2", 5)]


def test_batch_check_names_both_numbers():
    M.check_batch(6, 8, 2)
    with pytest.raises(ValueError, match=r"batch_size 7 .*max_batch 8 - 2 channels"):
        M.check_batch(7, 8, 2)
    with pytest.raises(ValueError, match=r"batch_size 1 .*max_batch 2 - 2 channels"):
        M.check_batch(1, 2, 2)


def test_language_channel_is_the_one_with_most_speech_lowest_on_a_tie():
    assert M.language_channel([10, 30, 20]) == 1
    assert M.language_channel([30, 30, 5]) == 0
    assert M.language_channel([0, 7, 7]) == 1
    assert M.language_channel([0, 0]) == 0


def test_waveform_shapes():
    assert M.parse_waveform(np.zeros(5, np.float32)).shape == (5, 1)
    assert M.parse_waveform(np.zeros((5, 2), np.float32)).shape == (5, 2)
    with pytest.raises(ValueError, match="3-dimensional"):
        M.parse_waveform(np.zeros((5, 2, 2), np.float32))


def test_segment_without_channel_compares_as_before():
    kw = dict(id=1, seek=0, start=0.0, end=1.0, text="x", tokens=[1, 2], avg_logprob=-0.5, compression_ratio=1.0, no_speech_prob=0.1)
    assert Segment(**kw) == Segment(**kw, words=None, temperature=None) and Segment(**kw).channel is None
    assert Segment(1, 0, 0.0, 1.0, "x", [1, 2], -0.5, 1.0, 0.1, None, 0.0) == Segment(**kw, temperature=0.0)      # positional use is unchanged
    assert Segment(**kw, channel=1) != Segment(**kw)
    assert [f for f in Segment.__dataclass_fields__][-1] == "channel"


# ---------------------------------------------------------------------------------------------------------- REST
def test_rest_renderings():
    from whisperlive_amd import rest
    mono = [_seg(0.0, None, " hello "), _seg(1.5, None, "world")]
    multi = [_seg(0.0, 0, " hello "), _seg(0.0, 1, "hi"), _seg(1.5, 0, "world")]
    assert rest.render_text(mono) == "hello world" and rest.render_text(multi, True) == "hello\nhi\nworld"
    assert rest.render_subtitles(mono, "srt") == "1\n00:00:00,000 --> 00:00:01,000\nhello\n\n2\n00:00:01,500 --> 00:00:02,500\nworld\n"
    assert rest.render_subtitles(multi, "srt").splitlines()[2::4] == ["[ch 0] hello", "[ch 1] hi", "[ch 0] world"]
    assert rest.render_subtitles(multi, "vtt").splitlines()[1::3] == ["[ch 0] hello", "[ch 1] hi", "[ch 0] world"]
    assert rest.render_subtitles(mono, "vtt").splitlines()[1::3] == ["hello", "world"]


def test_rest_boolean_field_and_channel_count():
    from tests import batched_common as BC
    from tests import flac_writer as W
    from whisperlive_amd import rest
    for v in ("true", "1", " Yes "):
        assert rest.parse_bool_field(v, "multichannel") is True
    for v in ("false", "0", "", None):
        assert rest.parse_bool_field(v, "multichannel") is False
    with pytest.raises(rest._HttpError) as ei:
        rest.parse_bool_field("maybe", "multichannel")
    assert ei.value.status == 400 and ei.value.payload == {"error": "multichannel must be a boolean"}
    assert rest.file_channels(BC.wav_bytes(np.zeros((10, 3), np.float32), 16000)) == 3
    assert rest.file_channels(W.encode_stream(np.zeros((32, 2), np.int64), 16000, 16, [32])) == 2
    assert rest.file_channels(b"nonsense") == 0


class _StubTranscriber:
    """stands in for the shared transcriber: records what BatchedInferencePipeline.transcribe is asked"""
    max_batch = 4


def test_rest_transcribe_file_serves_multichannel_through_the_pipeline(monkeypatch):
    from tests import batched_common as BC
    from whisperlive_amd import batched, rest
    asked = []

    def fake(self, data, **kw):
        asked.append(kw)
        if kw.get("language") == "refuse":
            raise ValueError("44101 Hz: no host route")
        return iter([_seg(0.0, 1)]), None

    monkeypatch.setattr(batched.BatchedInferencePipeline, "transcribe", fake)
    server = rest.RestServer.__new__(rest.RestServer)
    server.file_batch_size = 8
    wav = BC.wav_bytes(np.zeros((10, 2), np.float32), 16000)
    segs, _ = server.transcribe_file(_StubTranscriber(), wav, multichannel=True, language="en")
    assert [s.channel for s in segs] == [1]
    assert asked == [dict(vad_filter=True, batch_size=2, multichannel=True, language="en")]      # min(8, max_batch 4 - 2 channels)
    with pytest.raises(rest._HttpError) as ei:                                                     # C + 1 items do not fit
        server.transcribe_file(_StubTranscriber(), BC.wav_bytes(np.zeros((10, 4), np.float32), 16000), multichannel=True)
    assert ei.value.status == 400 and "4 channels" in ei.value.payload["error"] and "holds 4" in ei.value.payload["error"]
    with pytest.raises(rest._HttpError) as ei:                                                     # no host route: a 400, not a 500
        server.transcribe_file(_StubTranscriber(), wav, multichannel=True, language="refuse")
    assert ei.value.status == 400 and "no host route" in ei.value.payload["error"]
    server.transcribe_file(_StubTranscriber(), wav, language="en")                                # without the field: as before
    assert asked[-1] == dict(vad_filter=True, batch_size=8, language="en")


def test_speaker_labels_are_read_per_channel():
    from whisperlive_amd import rest

    class Resident:
        def __init__(self, ch):
            self.ch, self.n_samples = ch, 16000 * 10

    class Diarizer:
        calls = []

        def identify_speakers_resident(self, resident, ranges):
            self.calls.append((resident.ch, list(ranges)))
            return [f"spk{resident.ch}"] * len(ranges)

    segs = [_seg(0.0, 0), _seg(0.5, 1), _seg(2.0, 0)]
    d = Diarizer()
    labels = rest.speaker_labels_per_channel(segs, d, lambda ch: Resident(ch))
    assert labels == {0: "spk0", 1: "spk1", 2: "spk0"}
    assert d.calls == [(0, [(0, 16000), (32000, 16000)]), (1, [(8000, 16000)])]                   # one call per channel


# ---------------------------------------------------------------------------------------------------------- bindings
def _header_prototype(name):
    src = open(os.path.join(ROOT, "include", "wlx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int32_t\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


CTYPE = {"wlx_engine*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const void*": C.c_void_p,
         "int64_t*": C.POINTER(C.c_int64), "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32),
         "int32_t*": C.POINTER(C.c_int32), "float*": C.POINTER(C.c_float)}


@pytest.mark.parametrize("name", ["wlx_pcm_put_frames_split", "wlx_pcm_put_flac_split", "wlx_logmel_chunks_multi",
                                  "wlx_debug_resample_split"])
def test_the_new_symbols_are_bound_with_the_headers_signatures(name):
    from whisperlive_amd import _lib
    assert name in _lib.EXPORTS
    lib = _lib.load()
    want = []
    for arg in _header_prototype(name):
        typ = arg.rsplit(" ", 1)[0].replace(" *", "*")
        want.append(C.POINTER(_lib.wlx_flac_info) if typ == "wlx_flac_info*" else CTYPE[typ])
    fn = getattr(lib, name)
    assert list(fn.argtypes) == want and fn.restype is C.c_int32


# ---------------------------------------------------------------------------------------------------------- the pipeline on a scripted slot
def test_source_rows_stay_addressable_for_everything_the_front_end_serves():
    assert M.source_rows_addressable(8, 3600 * 16000)                      # 8 channels of an hour: 4.6e8 samples
    assert M.source_rows_addressable(37, 3600 * 16000) and not M.source_rows_addressable(38, 3600 * 16000)
    assert M.source_rows_addressable(4473, 1) and not M.source_rows_addressable(4474, 1)          # rows are whole 30 s windows


def _split_engine():
    from tests.fakes import FakeEngine, FakeSlot
    from whisperlive_amd.specs import WhisperSpec

    class SplitSlot(FakeSlot):
        """the device front end's methods, scripted; a log-mel group that reaches a source item is the bug this guards against"""

        def put_frames_split(self, frames, rate, first_item=0):
            self.calls.append(("put_frames_split", np.asarray(frames).shape, rate, first_item))
            self.sources = list(range(first_item, first_item + np.asarray(frames).shape[1]))
            return np.asarray(frames).shape[0]

        def pcm(self, item=0):
            raise AssertionError("nothing here needs the host copy")

        def logmel_chunks(self, chunks, src_item=0, first_item=0):
            assert first_item + len(chunks) <= min(self.sources), "a destination item overlaps a source"
            self.calls.append(("logmel_chunks", len(chunks), list(src_item), first_item))
            for i, c in enumerate(chunks):
                self._frames[first_item + i] = (sum(b - a for a, b in c) + 160) // 160
            return [self._frames[first_item + i] for i in range(len(chunks))]

    class SplitEngine(FakeEngine):
        def create_slot(self, max_batch=1, rows=5):
            s = SplitSlot(self, max_batch, rows)
            s._enc_generation = 0
            self.slots.append(s)
            return s

    return SplitEngine(WhisperSpec(80, 128, 2, 1, 1, 512, 2409))


def test_language_detection_reads_a_channel_with_more_chunks_than_fit_in_front_of_the_sources():
    """max_batch 4, stereo: two items are left for a group, and the language channel has ten chunks — the detection's log-mel
    launches go out two chunks at a time (groups of batch_size), never over a source item"""
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    eng = _split_engine()
    eng.default_tokens = [300, 301, 302]
    eng.lang_index = 3
    hip = WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(eng.spec.vocab), max_batch=4, multilingual=True)
    sr = 16000
    clips = [{"start": i * 3 * sr, "end": i * 3 * sr + 2 * sr} for i in range(10)]
    audio = np.zeros((30 * sr, 2), np.float32)
    segs, info = BatchedInferencePipeline(hip).transcribe(audio, clip_timestamps=clips, chunk_length=2, vad_filter=False, batch_size=2,
                                                          multichannel=True)
    calls = eng.slots[0].calls
    detect = [c for c in calls[: [c[0] for c in calls].index("detect_language")] if c[0] == "logmel_chunks"]
    # a tie in speech: channel 0 (item 2) is read; ten chunks of 200 frames are fewer than the 3000 the vote asks for, so all are read
    assert detect == [("logmel_chunks", 2, [2, 2], 0)] * 5
    assert info.language == hip._base_tokenizer.language_token_ids()[3][0] and info.language_probability > 0.5
    segs = list(segs)
    assert len(segs) == 20 and [s.channel for s in segs] == [0, 1] * 10 and [s.id for s in segs] == list(range(1, 21))
    decode = [c for c in calls if c[0] == "logmel_chunks"][5:]
    assert [c[2] for c in decode] == [[2, 2]] * 5 + [[3, 3]] * 5 and all(c[3] == 0 for c in decode)


def test_rest_refuses_multichannel_with_stream():
    import http.client
    from tests import test_rest as TR
    with TR.Served() as s:
        st, _, body = s.post([TR.FILE, ("stream", "true"), ("multichannel", "true")])
        assert st == 400 and b"multichannel cannot be combined with stream" in body
        st, _, body = s.post([TR.FILE, ("multichannel", "perhaps")])
        assert st == 400 and b"multichannel must be a boolean" in body
        assert s.t.calls == []
