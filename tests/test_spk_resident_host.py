"""CPU tests of the resident speaker-labelling route: SpeakerDiarizer.identify_speakers_resident against identify_speakers on the same
embeddings, the REST labelling helper's choice between the resident and the host route, the segment-to-range clamping, and the
bindings of wlx_spk_embed_pcm_batch / wlx_spk_embed_ring_batch against include/wlx.h."""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from whisperlive_amd import _lib, rest
from whisperlive_amd.diarization import SpeakerDiarizer
from whisperlive_amd.engine import ResidentPcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(v):
    v = np.asarray(v, dtype=np.float32)
    return v / np.linalg.norm(v)


# the embedding of a range / segment is looked up by its length: one table serves both routes
A, B, D = _unit([1, 0, 0, 0]), _unit([0, 1, 0, 0]), _unit([0, 0, 1, 0])
TABLE = {16000: A, 16001: B, 16002: _unit([0.9, 0.1, 0, 0]), 16003: None, 16004: D, 16005: _unit([0.1, 0.9, 0, 0]), 16006: _unit([0, 0, 0, 1])}
LENGTHS = [16000, 16001, 16002, 16003, 16004, 16005, 16006, 16000]


class FakeEmbedder:
    """records every call; it has no resident entry points, as an embedder from before them"""

    def __init__(self):
        self.calls = []

    def __call__(self, pcm, sample_rate=16000):
        self.calls.append(("embed", len(pcm)))
        return TABLE[len(pcm)]

    def embed_many(self, pcms, sample_rate=16000):
        self.calls.append(("embed_many", [len(p) for p in pcms]))
        return [TABLE[len(p)] for p in pcms]


class ResidentEmbedder(FakeEmbedder):
    def embed_resident(self, slot, item, ranges):
        self.calls.append(("embed_resident", slot, item, list(ranges)))
        return [TABLE.get(n) if n >= 4800 else None for _, n in ranges]

    def embed_ring(self, ring, ranges):
        self.calls.append(("embed_ring", ring, list(ranges)))
        return [TABLE.get(n) if n >= 4800 else None for _, n in ranges]


@pytest.mark.parametrize("kw", [{}, {"max_speakers": 2}, {"speaker_names": ["ann", "bob"]}])
@pytest.mark.parametrize("source", ["slot", "ring"])
def test_resident_labels_equal_identify_speakers(kw, source):
    """a None in the middle, the speaker cap and speaker_names: the labels and the centroids of the host route, in order"""
    host = SpeakerDiarizer(embedder=FakeEmbedder(), **kw)
    want = host.identify_speakers([np.zeros(n, np.float32) for n in LENGTHS])
    assert want[3] is None and len(set(want) - {None}) >= 2
    if "max_speakers" in kw:
        assert len(set(want) - {None}) == 2
    if "speaker_names" in kw:
        assert want[0] == "ann" and want[1] == "bob" and "SPEAKER_02" in want
    emb = ResidentEmbedder()
    dev = SpeakerDiarizer(embedder=emb, **kw)
    ranges = [(100 * i, n) for i, n in enumerate(LENGTHS)]
    slot, ring = object(), object()
    src = ResidentPcm(slot, 3, 10 ** 6) if source == "slot" else ring
    assert dev.supports_resident(src)
    assert dev.identify_speakers_resident(src, ranges) == want
    assert emb.calls == ([("embed_resident", slot, 3, ranges)] if source == "slot" else [("embed_ring", ring, ranges)])    # one call, all ranges
    assert list(dev.speakers) == list(host.speakers)
    for k in host.speakers:
        assert (dev.speakers[k] == host.speakers[k]).all()


def test_short_range_gets_no_label_and_old_embedder_is_not_supported():
    dev = SpeakerDiarizer(embedder=ResidentEmbedder())
    assert dev.identify_speakers_resident(ResidentPcm(object(), 0, 10 ** 6), [(0, 4799), (0, 16000), (5, 0)]) == [None, "SPEAKER_00", None]
    old = SpeakerDiarizer(embedder=FakeEmbedder())
    assert not old.supports_resident(ResidentPcm(object(), 0, 10 ** 6)) and not old.supports_resident(object())
    assert not dev.supports_resident(None)


def _segments(*spans):
    return [SimpleNamespace(start=a, end=b) for a, b in spans]


def test_segment_ranges_are_clamped_to_the_file():
    segs = _segments((0.0, 1.0), (1.0, 1.0), (2.5, 2.0), (-1.0, 0.5), (9.5, 12.0), (10.0, 11.0), (11.0, 12.0), (0.00001, 0.00002))
    got = rest.segment_sample_ranges(segs, 160000)
    # empty, reversed, starting at the end of the file, past it, and rounding to nothing: no range
    assert got == [(0, 0, 16000), (3, 0, 8000), (4, 152000, 160000)]
    assert rest.segment_sample_ranges(segs, 0) == []


def test_rest_helper_takes_the_resident_route_when_it_can():
    segs = _segments((0.0, 1.0), (1.0, 1.0), (1.0, 1.0 + 16001 / 16000), (50.0, 60.0))
    handle = ResidentPcm(object(), 0, 16000 * 3)
    host_audio = np.zeros(16000 * 3, np.float32)
    loads = []

    def load():
        loads.append(1)
        return host_audio

    # resident: the embedder reads the slot, the host audio is never asked for
    emb = ResidentEmbedder()
    got = rest.speaker_labels_for_segments(segs, load, SpeakerDiarizer(embedder=emb), resident=handle)
    assert got == {0: "SPEAKER_00", 2: "SPEAKER_01"} and not loads
    assert emb.calls == [("embed_resident", handle.slot, 0, [(0, 16000), (16000, 16001)])]
    # no handle: today's route, on the waveform
    emb = ResidentEmbedder()
    assert rest.speaker_labels_for_segments(segs, load, SpeakerDiarizer(embedder=emb), resident=None) == got and len(loads) == 1
    assert emb.calls == [("embed_many", [16000, 16001])]
    # an embedder without the entry point: today's route although the audio is resident
    emb = FakeEmbedder()
    assert rest.speaker_labels_for_segments(segs, host_audio, SpeakerDiarizer(embedder=emb), resident=handle) == got
    assert emb.calls == [("embed_many", [16000, 16001])]
    # a diarizer that only labels one segment at a time
    one = SimpleNamespace(identify_speaker=lambda pcm, sr: "S%d" % len(pcm))
    assert rest.speaker_labels_for_segments(segs, host_audio, one, resident=handle) == {0: "S16000", 2: "S16001"}
    # nothing to read at all
    assert rest.speaker_labels_for_segments(segs, None, SpeakerDiarizer(embedder=emb)) == {}
    assert rest.speaker_labels_for_segments(segs, host_audio, None, resident=handle) == {}


def test_rest_helper_falls_back_when_the_resident_audio_is_gone():
    class Evicted(ResidentEmbedder):
        def embed_resident(self, slot, item, ranges):
            raise _lib.WlxError("item 0: no PCM resident")

    segs = _segments((0.0, 1.0))
    emb = Evicted()
    d = SpeakerDiarizer(embedder=emb)
    got = rest.speaker_labels_for_segments(segs, lambda: np.zeros(32000, np.float32), d, resident=ResidentPcm(object(), 0, 32000))
    assert got == {0: "SPEAKER_00"} and emb.calls == [("embed_many", [16000])] and len(d.speakers) == 1


def test_transcriber_handle_is_dropped_with_the_slot():
    """WhisperModelHIP.resident_file_audio: only while the thread keeps the slot and the item holds the file"""
    import threading
    from whisperlive_amd.transcriber import WhisperModelHIP
    m = WhisperModelHIP.__new__(WhisperModelHIP)
    m._tls, m._slots_lock = threading.local(), threading.Lock()
    count = {"n": 1000}
    slot = SimpleNamespace(sid=0, lock=threading.Lock(), pcm_count=lambda item=0: count["n"], _owner=None)
    assert m.resident_file_audio() is None
    m._tls.slot, m._tls.file_audio = slot, ResidentPcm(slot, 0, 1000)
    assert m.resident_file_audio() is m._tls.file_audio
    count["n"] = 999                                  # the item was overwritten
    assert m.resident_file_audio() is None
    count["n"] = 1000
    shared = {"resident": False}                      # the batched pipeline evicted its source item
    m._tls.file_audio = ResidentPcm(slot, 0, 1000, shared)
    assert m.resident_file_audio() is None
    shared["resident"] = True
    assert m.resident_file_audio() is not None
    m._tls.slot = SimpleNamespace(sid=1)              # the thread's slot was replaced by a wider one
    assert m.resident_file_audio() is None
    m._tls.slot = slot
    m.release_slot()
    assert m.resident_file_audio() is None and m._tls.slot is None


# ------------------------------------------------------------------------------------------------ bindings against the header
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "wlx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _argtype(decl):
    """'const int64_t* starts' -> POINTER(c_int64); opaque handles are void pointers in the binding"""
    decl = decl.replace("const ", "")
    base, ptr = re.match(r"(\w+)\s*(\**)", decl).groups()
    if base.startswith("wlx_"):
        assert ptr == "*"
        return C.c_void_p
    return C.POINTER(_CTYPES[base]) if ptr else _CTYPES[base]


@pytest.mark.parametrize("name,n_args", [("wlx_spk_embed_pcm_batch", 9), ("wlx_spk_embed_ring_batch", 7)])
def test_bindings_match_the_header(name, n_args):
    ret, args = _prototype(name)
    assert ret == "int32_t" and len(args) == n_args
    assert name in _lib.EXPORTS

    _lib.build()
    lib = _lib.load()           # (no GPU needed: loading declares the prototypes and reads the ABI version)
    fn = getattr(lib, name)
    assert list(fn.argtypes) == [_argtype(a) for a in args] and fn.restype is C.c_int32


# ------------------------------------------------------------------------------------------------ the streaming speaker step
class _Diar:
    def __init__(self, resident=True, fail=False):
        self.calls, self.resident, self.fail = [], resident, fail

    def supports_resident(self, source):
        return self.resident

    def identify_speakers_resident(self, source, ranges):
        self.calls.append(("ring", source, list(ranges)))
        if self.fail:
            raise _lib.WlxError("range is not resident")
        return ["R"]

    def identify_speaker(self, pcm, sr):
        self.calls.append(("host", len(pcm), float(pcm[0]) if len(pcm) else None))
        return "H"


def _session(diar, ring):
    from whisperlive_amd.serve_client import ServeClientHIP
    c = ServeClientHIP(None, model=None, diarization=diar)
    c.frames_np = np.arange(16000 * 10, dtype=np.float32)
    c.frames_offset, c.timestamp_offset = 30.0, 32.0          # 30 s trimmed away, 2 s of the buffer committed
    c._ring = ring
    return c


def test_streaming_step_reads_the_ring_at_absolute_positions():
    seg = SimpleNamespace(start=1.0, end=3.5)
    ring = object()
    d = _Diar()
    assert _session(d, ring)._identify_speaker(seg) == "R"
    # buffer offsets 48000 .. 88000 of a buffer that starts at stream position 480000
    assert d.calls == [("ring", ring, [(480000 + 48000, 40000)])]
    # the end is clamped to what the buffer holds, as the host slice is
    d = _Diar()
    assert _session(d, ring)._identify_speaker(SimpleNamespace(start=7.0, end=9.0)) == "R"
    assert d.calls == [("ring", ring, [(480000 + 144000, 16000)])]
    # under 0.3 s: no label, no call
    d = _Diar()
    assert _session(d, ring)._identify_speaker(SimpleNamespace(start=1.0, end=1.2)) is None and d.calls == []


def test_streaming_step_keeps_the_host_slice_when_it_must():
    seg = SimpleNamespace(start=1.0, end=3.5)
    for d, ring in ((_Diar(), False), (_Diar(), None), (_Diar(resident=False), object())):
        assert _session(d, ring)._identify_speaker(seg) == "H"
        assert d.calls == [("host", 40000, 48000.0)]
    d = _Diar(fail=True)                                       # trimmed away between the snapshot and the call
    ring = object()
    assert _session(d, ring)._identify_speaker(seg) == "H"
    assert d.calls == [("ring", ring, [(528000, 40000)]), ("host", 40000, 48000.0)]
    old = SimpleNamespace(identify_speaker=lambda pcm, sr: "OLD")          # a diarizer from before the resident route
    assert _session(old, object())._identify_speaker(seg) == "OLD"
