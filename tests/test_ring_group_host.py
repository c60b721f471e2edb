"""CPU tests of the ring group's host side: the ctypes prototypes of every wlx_ring_group_* entry of include/wlx.h, the argument
checks of engine.PcmRingGroup (made before the library is asked for anything), and the per-channel host resampler."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd import stream_resample as SR
from whisperlive_amd.engine import HipWhisperEngine, PcmRing, PcmRingGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wlx_ring_group_create", "wlx_ring_group_destroy", "wlx_ring_group_lane", "wlx_ring_group_append_frames")


def test_header_declares_the_group_and_the_binding_has_a_prototype_for_each_entry():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(wlx_ring_group_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(ENTRIES)
    assert all(name in _lib.EXPORTS for name in ENTRIES)
    _lib.build()
    lib = _lib.load()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    assert lib.wlx_ring_group_create.argtypes == [vp, i64, i32, i32, i32, C.POINTER(vp)]
    assert lib.wlx_ring_group_lane.argtypes == [vp, i32, C.POINTER(vp)]
    assert lib.wlx_ring_group_append_frames.argtypes == [vp, vp, i64, i32, i64, i64, f32p, i64, i64p, i64p, i64p, i64p]
    # the group's append takes what the ring's takes, argument for argument
    assert lib.wlx_ring_group_append_frames.argtypes == lib.wlx_ring_append_frames.argtypes
    assert lib.wlx_ring_group_destroy.argtypes == [vp] and lib.wlx_ring_group_destroy.restype is None
    for name in ("wlx_ring_group_create", "wlx_ring_group_lane", "wlx_ring_group_append_frames"):
        assert getattr(lib, name).restype is i32


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.wlx_ring_group_create(None, 0, _lib.PCM_S16, 2, 48000, C.byref(h)) == _lib.ERR_ARG and not h.value
    assert lib.wlx_ring_group_lane(None, 0, C.byref(h)) == _lib.ERR_ARG
    assert lib.wlx_ring_group_append_frames(None, None, 0, 0, 0, 0, None, 0, None, None, None, None) == _lib.ERR_ARG
    lib.wlx_ring_group_destroy(None)                                               # like free(NULL)
    assert b"wlx_ring_group_append_frames" in lib.wlx_last_error()


class NoLibrary:
    """an engine whose library must not be reached: the checks come first"""
    device = 0

    @property
    def lib(self):
        raise AssertionError("the library was asked before the arguments were checked")


@pytest.mark.parametrize("args", [
    (_lib.PCM_S16, 0, 48000), (_lib.PCM_S16, 9, 48000), (_lib.PCM_S16, True, 48000), (_lib.PCM_S16, "2", 48000), (_lib.PCM_S16, 2.0, 48000),
    (2, 2, 48000), (6, 2, 48000), ("int16", 2, 48000),
    (_lib.PCM_S16, 2, 44101), (_lib.PCM_S16, 2, 0), (_lib.PCM_S16, 2, -8000), (_lib.PCM_S16, 2, "48000"), (_lib.PCM_MULAW, 2, 7999),
])
def test_group_argument_checks(args):
    with pytest.raises(ValueError):
        PcmRingGroup(NoLibrary(), *args)
    with pytest.raises(ValueError):
        PcmRingGroup(NoLibrary(), _lib.PCM_S16, 2, 48000, capacity_samples=-1)


def test_engine_offers_the_group_and_a_lane_is_a_ring():
    assert callable(HipWhisperEngine.create_ring_group)
    from whisperlive_amd.engine import _PcmRingLane
    assert issubclass(_PcmRingLane, PcmRing)
    assert (PcmRingGroup.MAX_RESIDENT, PcmRingGroup.TRIM) == (PcmRing.MAX_RESIDENT, PcmRing.TRIM)


def test_the_host_route_is_one_stream_resampler_per_channel():
    x = np.ascontiguousarray(R.multichannel(5000, 44100, 3, R.F32))
    host = SR.ChannelStreamResamplers("float32", 3, 44100)
    edges = [0, 1, 1, 40, 2000, 2000, 4999, 5000]
    parts = [host.feed(x[a:b].tobytes()) for a, b in zip(edges[:-1], edges[1:])] + [host.feed(b"", flush=True)]
    assert host.closed and host.J == 5000 and host.M == SR.stream_count(44100, 5000, True)
    for c in range(3):
        mono = SR.StreamResampler("float32", 1, 44100)
        want = np.concatenate([mono.feed(np.ascontiguousarray(x[a:b, c])) for a, b in zip(edges[:-1], edges[1:])] + [mono.flush()])
        got = np.concatenate([p[c] for p in parts])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # ... which is scipy's resample_poly of that channel alone: no mean over the channels
        ref = R.scipy_ref(x[:, c], *R.ratio(44100)).astype(np.float32)
        assert np.abs(got - ref).max() <= R.RESAMPLE_ATOL / 4
    # advance keeps the book without computing
    book = SR.ChannelStreamResamplers("float32", 3, 44100)
    assert [book.advance(x[a:b]) for a, b in zip(edges[:-1], edges[1:])] == [p[0].shape[0] for p in parts[:-1]]
    assert (book.J, book.M) == (5000, SR.stream_count(44100, 5000))
    with pytest.raises(ValueError):
        book.frames(bytes(13))
    with pytest.raises(ValueError):
        SR.ChannelStreamResamplers("float32", 9, 44100)
