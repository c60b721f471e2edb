"""GPU tests (-m gpu) of the ragged-batch VAD gate (include/wlx.h wlx_vad_probs_batch / wlx_vad_probs_pcm_batch): a row of a batch does
not depend on its neighbours, its position or the table's fill — it is compared with the same item as a batch of ONE (which is what the
single entry points run) through .view(np.uint32), no tolerance; the absolute reference is oracle/silero_vad.py; and the batch worker's
front half built on it (WhisperModelHIP.encode_audio_batch_gated) produces the
features, encoder outputs and results of the per-request host gate."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd._lib import WlxError
from whisperlive_amd.synthetic import energy_following_vad_weights, speech_like_pcm

pytestmark = pytest.mark.gpu

RAGGED = [1, 511, 512, 513, 2047, 2048, 2049, 40000, 1536]      # 1 window; n % 512 == 0 (+1 zero window); 3, 4, 5 windows round the 4-window group


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def padded(x):
    return np.pad(np.asarray(x, np.float32), (0, 512 - x.shape[0] % 512))      # get_speech_timestamps' rule: to the NEXT multiple


@pytest.fixture(scope="module")
def vm(gpu):
    from whisperlive_amd import vad
    m = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


@pytest.fixture(scope="module")
def ragged(vm):
    """the ragged set and the row of each item on its own (wlx_vad_probs: a batch of one), computed once"""
    src = speech_like_pcm(3.0, seed=77)
    clips = [src[37 * i: 37 * i + n].copy() for i, n in enumerate(RAGGED)]
    return clips, [vm(padded(x)) for x in clips]


def test_ragged_batch_equals_singles_in_any_order(vm, ragged):
    clips, want = ragged
    got = vm.probs_many(clips)
    assert [g.shape[0] for g in got] == [n // 512 + 1 for n in RAGGED]
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (i, RAGGED[i])
        assert same(vm.probs_many([clips[i]])[0], w), (i, RAGGED[i])        # the batch entry point with one item
    for order in (list(range(len(clips)))[::-1], np.random.default_rng(5).permutation(len(clips)).tolist()):
        got = vm.probs_many([clips[i] for i in order])
        for k, i in enumerate(order):
            assert same(got[k], want[i]), (order, k)


def test_every_item_starts_from_a_zero_state(vm):
    loud = speech_like_pcm(1.0, seed=9)[:12000]
    silent = np.zeros(3000, np.float32)
    a, b, c = vm.probs_many([loud, silent, loud])
    assert same(a, c) and same(a, vm(padded(loud)))
    assert same(b, vm(padded(silent)))


def test_a_full_table_and_a_list_split_in_two_calls(vm):
    rng = np.random.default_rng(64)
    src = speech_like_pcm(2.0, seed=3)
    clips = [src[k: k + int(n)].copy() for k, n in zip(rng.integers(0, 16000, 65), rng.integers(600, 1601, 65))]
    want = [vm(padded(x)) for x in clips]
    got = vm.probs_many(clips[:64])                 # one call, every table entry in use
    assert len(got) == 64 and all(same(g, w) for g, w in zip(got, want))
    got = vm.probs_many(clips)                      # 64 + 1
    assert len(got) == 65 and all(same(g, w) for g, w in zip(got, want))


def test_short_batch_after_a_long_one_reads_nothing_stale(vm, ragged):
    clips, want = ragged
    long_ = clips[RAGGED.index(40000)]
    assert same(vm.probs_many([long_, long_[:20000]])[0], want[RAGGED.index(40000)])
    ones = [clips[0], clips[1], speech_like_pcm(1.0, seed=2)[4000:4300]]
    got = vm.probs_many(ones)
    assert all(g.shape == (1,) and same(g, vm(padded(x))) for g, x in zip(got, ones))


def test_ragged_batch_against_the_restatement(gpu):
    """the network itself: random Silero-shaped weights against oracle/silero_vad.py within the 2e-5 of tests/test_vad_model.py"""
    from oracle import silero_vad as sv
    from whisperlive_amd import vad
    w = sv.random_weights(3)
    m = vad.SileroHIPModel(w, device=0)
    try:
        src = speech_like_pcm(2.0, seed=11)
        clips = [src[100 * i: 100 * i + n] for i, n in enumerate([513, 5000, 1, 2048, 16000])]
        for x, g in zip(clips, m.probs_many(clips)):
            want = sv.speech_probs(w, padded(x))
            assert g.shape == want.shape and np.abs(g - want).max() < 2e-5, np.abs(g - want).max()
    finally:
        m.close()


@pytest.mark.parametrize("opt", [dict(threshold=0.5), dict(threshold=0.6, min_silence_duration_ms=200, speech_pad_ms=60, min_speech_duration_ms=100)])
def test_segmentation_of_a_batch_equals_per_item(vm, opt):
    from whisperlive_amd import vad
    clips = [speech_like_pcm(s, seed=30 + i)[: int(s * 16000)] for i, s in enumerate((1.0, 4.0, 2.56, 6.0))] + [np.zeros(5000, np.float32)]
    opts = [vad.VadOptions(**opt)] * len(clips)
    got = vad.get_speech_timestamps_many(clips, opts, vm)
    assert got == [vad.get_speech_timestamps(x, o, model=vm) for x, o in zip(clips, opts)]
    assert any(got)


def _raw(vm, pcm, counts, extra, n, cap, probs, nw, handle="vm"):
    f32p, i64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return vm.lib.wlx_vad_probs_batch(vm.handle if handle == "vm" else None, ptr(pcm, f32p), ptr(counts, i64p), ptr(extra, i32p), n,
                                      ptr(probs, f32p), cap, ptr(nw, i32p), None)


def test_refusals_write_nothing(vm):
    pcm = speech_like_pcm(1.0, seed=1)
    c2 = np.asarray([1000, 513], np.int64)                # 2 + 2 windows
    big = np.full(65, 10, np.int64)
    e0, e5 = np.zeros(2, np.int32), np.asarray([0, 5], np.int32)
    cases = {
        "n = 0": dict(counts=c2, extra=e0, n=0, cap=8),
        "n = 65": dict(counts=big, extra=np.zeros(65, np.int32), n=65, cap=100),
        "cap one short": dict(counts=c2, extra=e0, n=2, cap=3),
        "negative count": dict(counts=np.asarray([1000, -1], np.int64), extra=e0, n=2, cap=8),
        "extra = 5": dict(counts=c2, extra=e5, n=2, cap=16),
        "extra = -1": dict(counts=c2, extra=np.asarray([-1, 0], np.int32), n=2, cap=16),
        "null pcm": dict(pcm=None, counts=c2, extra=e0, n=2, cap=8),
        "null counts": dict(counts=None, extra=e0, n=2, cap=8),
        "null probs": dict(counts=c2, extra=e0, n=2, cap=8, probs=None),
        "null n_windows": dict(counts=c2, extra=e0, n=2, cap=8, nw=None),
        "null object": dict(counts=c2, extra=e0, n=2, cap=8, handle=None),
    }
    for name, kw in cases.items():
        probs, nw = np.full(128, -7.0, np.float32), np.full(65, -7, np.int32)
        args = dict(pcm=pcm, probs=probs, nw=nw)
        args.update(kw)
        assert _raw(vm, **args) == _lib.ERR_ARG, name
        assert (probs == -7.0).all() and (nw == -7).all(), name
    # the same arguments with room for the 4 windows are served
    probs, nw = np.full(128, -7.0, np.float32), np.full(65, -7, np.int32)
    assert _raw(vm, pcm, c2, None, 2, 4, probs, nw) == 0
    assert nw[:2].tolist() == [2, 2] and (nw[2:] == -7).all() and (probs[4:] == -7.0).all()
    assert same(probs[:2], vm(pcm[:1000])) and same(probs[2:4], vm(pcm[1000:1513]))


def test_all_empty_items_launch_nothing(vm):
    probs, nw = np.full(8, -7.0, np.float32), np.full(3, -7, np.int32)
    assert _raw(vm, np.zeros(1, np.float32), np.zeros(3, np.int64), None, 3, 0, probs, nw) == 0
    assert nw.tolist() == [0, 0, 0] and (probs == -7.0).all()
    # an empty item between two others takes no part
    pcm = speech_like_pcm(1.0, seed=6)
    probs, nw = np.full(8, -7.0, np.float32), np.full(3, -7, np.int32)
    assert _raw(vm, pcm, np.asarray([700, 0, 300], np.int64), None, 3, 3, probs, nw) == 0
    assert nw.tolist() == [2, 0, 1]
    assert same(probs[:2], vm(pcm[:700])) and same(probs[2:3], vm(pcm[700:1000]))


# ---- resident form ----------------------------------------------------------------------------------------------------
def test_gate_over_resident_items_equals_per_item_and_the_upload(vm, eng):
    src = speech_like_pcm(3.0, seed=21)
    lens = [40000, 513, 2048, 1]
    slot = eng.create_slot(4, 5)
    try:
        for i, n in enumerate(lens):
            slot.pcm_put(src[11 * i: 11 * i + n], item=i)
        got = vm.probs_pcm_many(slot, lens)
        for i, n in enumerate(lens):
            x = src[11 * i: 11 * i + n]
            assert same(got[i], vm.probs_pcm(slot, 0, n, item=i)), i
            assert same(got[i], vm(padded(x))), i
        up = vm.probs_many([src[11 * i: 11 * i + n] for i, n in enumerate(lens)])
        assert all(same(a, b) for a, b in zip(got, up))
        # a prefix of what is resident, from the second item on
        sub = vm.probs_pcm_many(slot, [500, 1024], first_item=1)
        assert same(sub[0], vm(padded(src[11: 511]))) and same(sub[1], vm(padded(src[22: 22 + 1024])))
        with pytest.raises(WlxError) as ei:                    # items 3 and 4: one past the slot
            vm.probs_pcm_many(slot, [1, 1], first_item=3)
        assert ei.value.code == _lib.ERR_ARG
    finally:
        slot.close()


def test_gate_right_behind_put_frames_waits_for_the_resampler(vm, eng):
    clip = R.multichannel(3 * 44100, 44100, 2, R.F32) * np.float32(0.5)
    other = speech_like_pcm(1.0, seed=8)[:9000]
    slot = eng.create_slot(2, 5)
    try:
        slot.pcm_put(other, item=1)
        n = slot.put_frames(clip, 44100, item=0)
        got = vm.probs_pcm_many(slot, [n, other.shape[0]])
        pcm = slot.pcm(0)
        assert pcm.shape[0] == n == 48000
        assert same(got[0], vm(padded(pcm))) and same(got[1], vm(padded(other)))
    finally:
        slot.close()


def test_item_without_pcm_is_a_state_error_and_other_devices_are_refused(vm, eng):
    import torch
    from whisperlive_amd import vad
    slot = eng.create_slot(2, 5)
    try:
        slot.pcm_put(speech_like_pcm(1.0, seed=8)[:1000], item=0)
        with pytest.raises(WlxError, match="not resident") as ei:
            vm.probs_pcm_many(slot, [16, 16])
        assert ei.value.code == _lib.ERR_STATE
        with pytest.raises(WlxError, match="not resident"):
            vm.probs_pcm_many(slot, [1001])
        if torch.cuda.device_count() > 1:
            far = vad.SileroHIPModel(energy_following_vad_weights(3), device=1)
            try:
                with pytest.raises(WlxError) as ei:
                    far.probs_pcm_many(slot, [16])
                assert ei.value.code == _lib.ERR_ARG
            finally:
                far.close()
    finally:
        slot.close()


# ---- the worker's front half ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker_case(eng, vm):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    hip = WhisperModelHIP("rand", engine=eng, hf_tokenizer=synthetic_tokenizer(H.TINY_EN.vocab), max_batch=6, vad_model=vm)
    hip.max_length = 24                                   # random weights never emit end-of-text: keep the decode short
    secs = (4.0, 9.0, 3.0, 2.0, 4.0)
    audios = [speech_like_pcm(s, seed=60 + i)[: int(s * 16000)] for i, s in enumerate(secs)]
    audios[0] = np.concatenate([audios[0][:16000], np.zeros(40000, np.float32), audios[0][16000:24000]])      # 2.5 s of silence inside
    audios[2] = np.zeros(48000, np.float32)               # all silent: the gate finds nothing and the whole audio is kept
    use_vad = [True, True, True, False, True]
    params = [None, None, None, None, dict(threshold=0.6, min_silence_duration_ms=200, speech_pad_ms=60)]
    yield hip, audios, use_vad, params
    hip.close()


def test_gated_front_half_equals_the_host_gate_route(worker_case, vm):
    from whisperlive_amd import vad
    hip, audios, use_vad, params = worker_case
    opts = [vad.VadOptions(**(p or {})) if u else None for u, p in zip(use_vad, params)]
    host = []
    for a, o in zip(audios, opts):
        chunks = vad.get_speech_timestamps(a, o, model=vm) if o is not None else []
        host.append(np.concatenate(vad.collect_chunks(a, chunks)[0]) if chunks else a)
    assert host[0].shape[0] < audios[0].shape[0] and host[2].shape[0] == 48000 and host[3] is audios[3]     # the gate really cuts
    assert host[4].shape[0] != audios[4].shape[0]
    enc = hip.encode_audio_batch(host)
    slot = enc.slot
    want_f = [slot.features(i).copy() for i in range(5)]
    want_e = [slot.encoder_output(i).copy() for i in range(5)]
    got = hip.encode_audio_batch_gated(audios, opts)
    assert got is not None
    enc2, counts = got
    assert enc2.slot is slot and enc2.batch == 5 and enc2.generation == enc.generation + 1
    assert counts == [h.shape[0] for h in host]
    for i in range(5):
        assert same(slot.features(i), want_f[i]), i
        assert same(slot.encoder_output(i), want_e[i]), i


def test_worker_results_equal_with_and_without_the_batched_route(worker_case, monkeypatch):
    from whisperlive_amd.batching import BatchInferenceWorker, BatchRequest
    from whisperlive_amd.transcriber import WhisperModelHIP
    hip, audios, use_vad, params = worker_case

    def run():
        w = BatchInferenceWorker(hip, max_batch_size=6, batch_window_ms=10)
        w.TEMPERATURES = (0.0,)
        reqs = [BatchRequest(audio=a, language="en", use_vad=u, vad_parameters=p) for a, u, p in zip(audios, use_vad, params)]
        w._process_multi(reqs)
        assert all(r.future.is_set() and r.error is None for r in reqs), [r.error for r in reqs]
        return [([(s.text, s.tokens, s.start, s.end) for s in r.result], r.info.duration, r.info.duration_after_vad) for r in reqs]

    calls = []
    real = WhisperModelHIP.encode_audio_batch_gated
    monkeypatch.setattr(WhisperModelHIP, "encode_audio_batch_gated", lambda self, a, o: calls.append(len(a)) or real(self, a, o))
    batched = run()
    assert calls == [5]
    monkeypatch.delattr(WhisperModelHIP, "encode_audio_batch_gated")
    per_request = run()
    assert batched == per_request
    assert any(segs for segs, _, _ in batched)
    assert batched[0][2] < 4.0 and batched[2][2] == 3.0 and batched[3][2] == 2.0
