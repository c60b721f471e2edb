"""GPU test (-m gpu) of two DIFFERENT readers of one slot item back to back behind one asynchronous writer (csrc/engine.h PcmLease):
put_frames returns with its resample launches possibly still in flight on the slot's stream, the VAD gate and the speaker engine then
read the item from streams of their own, in either order, and a refused call between them disturbs neither. Each reader equals its
upload route on the samples wlx_pcm_get returns, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_kernel_ref as R
from whisperlive_amd import _lib, vad
from whisperlive_amd.synthetic import energy_following_vad_weights

from .test_gpu_spk_resident import E, SENTINEL, eng, raw_pcm, spk  # noqa: F401  (eng and spk are that module's fixtures)

pytestmark = pytest.mark.gpu

RATE, SECONDS = 48000, 2
RANGES = [(0, 16000), (8000, 16000)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vm(gpu):
    m = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    yield m
    m.close()


def _refused_gate(vm, slot, item, n):
    """wlx_vad_probs_pcm on [0, n) -> (rc, the output array)"""
    cap = n // 512 + 2
    probs, nw = np.full(cap, SENTINEL, np.float32), C.c_int32(-1)
    rc = vm.lib.wlx_vad_probs_pcm(vm.handle, slot.engine._h, slot.sid, item, 0, n, 0, probs.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                  C.byref(nw), None)
    return rc, probs


def test_two_readers_back_to_back_behind_one_put_frames(eng, spk, vm):  # noqa: F811
    clip = R.multichannel(SECONDS * RATE, RATE, 2, R.F32) * np.float32(0.5)
    other = np.ascontiguousarray(clip[::-1, ::-1]) * np.float32(0.8)         # a different signal for item 1
    n = SECONDS * 16000
    slot = eng.create_slot(2, 5)
    try:
        # item 0: the gate first, a refused speaker call (one sample past the resident count), then the speaker engine
        assert slot.put_frames(clip, RATE, item=0) == n
        probs0 = vm.probs_pcm(slot, 0, n, item=0)
        rc, out, st = raw_pcm(spk, slot, 0, [RANGES[0], (n - 16000 + 1, 16000)])
        assert rc == _lib.ERR_STATE and (out == SENTINEL).all() and (st == -1).all()
        emb0 = spk.embed_resident(slot, 0, RANGES)
        # item 1: the opposite order on a fresh put_frames, a refused gate call between the two
        assert slot.put_frames(other, RATE, item=1) == n
        emb1 = spk.embed_resident(slot, 1, RANGES)
        rc, probs = _refused_gate(vm, slot, 1, n + 1)
        assert rc == _lib.ERR_STATE and (probs == SENTINEL).all()
        probs1 = vm.probs_pcm(slot, 0, n, item=1)
        # the upload routes on what the items hold (read only now: wlx_pcm_get waits for the slot's stream)
        assert slot.pcm_count(0) == slot.pcm_count(1) == n
        pcm0, pcm1 = slot.pcm(0), slot.pcm(1)
        assert not np.array_equal(pcm0, pcm1)
        for item, (pcm, probs, emb) in enumerate(((pcm0, probs0, emb0), (pcm1, probs1, emb1))):
            want = vm(np.pad(pcm, (0, vad.WINDOW - n % vad.WINDOW)))
            assert probs.shape == want.shape and np.array_equal(_bits(probs), _bits(want)), item
            for (a, c), got in zip(RANGES, emb):
                assert got is not None and got.shape == (E,) and np.array_equal(_bits(got), _bits(spk.embed(pcm[a:a + c]))), (item, a, c)
    finally:
        slot.close()
