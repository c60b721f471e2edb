"""GPU tests (-m gpu) of the VAD gate over a slot item's resident PCM (include/wlx.h wlx_vad_probs_pcm): the same pass as the upload
path and the ring path (each a batch of one) on the same samples, bit for bit, wherever the samples lie; ordered behind the slot's
stream; nothing of the VAD object's PCM buffers involved."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd._lib import WlxError
from whisperlive_amd.synthetic import energy_following_vad_weights, speech_like_pcm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


@pytest.fixture(scope="module")
def vm(gpu):
    from whisperlive_amd import vad
    m = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def resident(eng):
    pcm = speech_like_pcm(3.0, seed=21)[:48000]
    slot = eng.create_slot(2, 5)
    slot.pcm_put(pcm, item=1)
    ring = eng.create_ring()
    ring.append(pcm)                                                  # the same samples at stream positions 0 ...
    yield slot, pcm, ring
    ring.close()
    slot.close()


def raw_probs(vm, x=None, ring=None, slot=None, start=0, n=0, extra=0):
    """one of the three single entry points with an explicit extra_zero_windows (the Python wrappers choose it themselves)"""
    if x is not None:
        x = np.ascontiguousarray(x, np.float32)
        n, extra = x.shape[0], 0
    cap = -(-n // 512) + extra
    probs, nw = np.full(cap + 1, -7.0, np.float32), C.c_int32(-1)
    out = probs.ctypes.data_as(C.POINTER(C.c_float))
    if x is not None:
        rc = vm.lib.wlx_vad_probs(vm.handle, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], out, cap, C.byref(nw), None)
    elif ring is not None:
        rc = vm.lib.wlx_vad_probs_resident(vm.handle, ring._h, start, n, extra, out, cap, C.byref(nw), None)
    else:
        rc = vm.lib.wlx_vad_probs_pcm(vm.handle, slot.engine._h, slot.sid, 1, start, n, extra, out, cap, C.byref(nw), None)
    assert rc == 0 and nw.value == cap and probs[cap] == -7.0
    return probs[:cap]


@pytest.mark.parametrize("start", [0, 777])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 2560, 40000])
def test_gate_on_resident_pcm_equals_gate_on_the_upload(vm, resident, n, start):
    from whisperlive_amd import vad
    slot, pcm, ring = resident
    x = pcm[start:start + n]
    want = vm(np.pad(x, (0, vad.WINDOW - n % vad.WINDOW)))            # a whole zero window when n is a multiple of 512
    got = vm.probs_pcm(slot, start, n, item=1)
    assert got.shape == want.shape == (n // 512 + 1,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the three single entry points are one pass: with no and with the most extra zero windows they agree bit for bit on the same
    # samples (the upload has no such argument: it is given the zeros)
    for extra in (0, 4):
        up = raw_probs(vm, x=np.pad(x, (0, 512 * (-(-n // 512) + extra) - n)))
        assert up.shape == (-(-n // 512) + extra,)
        assert np.array_equal(up.view(np.uint32), raw_probs(vm, ring=ring, start=start, n=n, extra=extra).view(np.uint32)), extra
        assert np.array_equal(up.view(np.uint32), raw_probs(vm, slot=slot, start=start, n=n, extra=extra).view(np.uint32)), extra
    if start == 0:
        opt = vad.VadOptions(threshold=0.5)
        assert vad.get_speech_timestamps_pcm(slot, n, opt, model=vm, item=1) == vad.get_speech_timestamps(x, opt, model=vm)


def test_gate_right_behind_put_frames_sees_the_resampled_audio(eng, vm):
    """put_frames returns with the resample launches possibly still in flight on the slot's stream; the gate runs on the VAD
    object's stream and has to wait for them (an event, not the null stream)"""
    from whisperlive_amd import vad
    clip = R.multichannel(3 * 44100, 44100, 2, R.F32) * np.float32(0.5)
    slot = eng.create_slot(1, 5)
    try:
        n = slot.put_frames(clip, 44100)
        got = vm.probs_pcm(slot, 0, n)
        pcm = slot.pcm()
        assert pcm.shape[0] == n == 48000
        want = vm(np.pad(pcm, (0, vad.WINDOW - n % vad.WINDOW)))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        slot.close()


def test_span_outside_the_resident_samples_is_a_state_error(vm, resident):
    slot, pcm, _ = resident
    for start, n, item in ((47000, 1001, 1), (0, 48001, 1), (0, 16, 0)):         # item 0 holds nothing
        with pytest.raises(WlxError, match="not resident") as ei:
            vm.probs_pcm(slot, start, n, item=item)
        assert ei.value.code == _lib.ERR_STATE


def test_a_fresh_vad_object_gates_a_long_item_without_having_seen_it(eng):
    """The library exposes no buffer sizes. What this shows: a VAD object whose own PCM buffers (device and pinned, 64 s at creation)
    have never held more than 512 samples gates a 2-million-sample (125 s) item — twice what those buffers hold — so the samples are
    read from the slot and only the per-window buffers grew; the probabilities equal the upload path's on another object."""
    from whisperlive_amd import vad
    n = 2_000_000
    pcm = np.tile(speech_like_pcm(5.0, seed=4)[:80000], 25)
    assert pcm.shape[0] == n
    fresh = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    other = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    slot = eng.create_slot(1, 5)
    try:
        fresh(np.zeros(512, np.float32))
        slot.pcm_put(pcm)
        got = fresh.probs_pcm(slot, 0, n)
        want = other(np.pad(pcm, (0, vad.WINDOW - n % vad.WINDOW)))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        slot.close(); fresh.close(); other.close()
