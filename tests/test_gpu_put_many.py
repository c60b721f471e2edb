"""GPU: wlx_pcm_put_many on the product path (Slot.put_many, transcribe_many(wave_put=True)): a wave of files of every route goes up in
one call, and every item holds BIT for BIT what the single-file route of its kind leaves (Slot.put_frames / put_flac / put_wav /
pcm_put into a reference slot), `logmel_resident` after it included; a refused or damaged entry costs only itself."""
import ctypes as C

import numpy as np
import pytest

from tests import batched_common as BC
from tests import helpers as H

from . import flac_writer as FW
from . import wav_writer as WW
from .put_many_cases import broken_frame_stream, flac_stream

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engine(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    eng = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7), device=0)
    yield eng
    eng.close()


def _adpcm(tag, rate, seconds, seed):
    spb = (WW.ima_samples_per_block if tag == WW.TAG_IMA else WW.ms_samples_per_block)(256, 1)
    return WW.random_adpcm(tag, int(rate * seconds) // spb + 1, 1, 256, rate=rate, seed=seed)


def _entries(scale=1.0):
    """the eight entries of the issue's call, about `scale` x 0.5 s each -> [(put_many entry, single route as (method, args))]"""
    rng = np.random.RandomState(int(scale * 100))
    n441 = int(22050 * scale)
    s16 = rng.randint(-20000, 20000, size=(n441, 2)).astype(np.int16)                       # what a 44.1 kHz stereo S16 WAV holds
    f16, _ = flac_stream(max(2, int(2 * scale)), 4096, 16, 1, 21)
    f441, _ = flac_stream(max(2, int(5 * scale)), 4096, 24, 2, 22, assignment=FW.MID_SIDE, rate=44100)
    mulaw = WW.write_g711(WW.speech_like(int(4000 * scale) + 3, 1, seed=1), 8000, WW.TAG_MULAW)
    alaw = WW.write_g711(WW.speech_like(int(4000 * scale) + 5, 2, seed=2), 8000, WW.TAG_ALAW, extensible=True)
    ima = _adpcm(WW.TAG_IMA, 8000, 0.5 * scale, 3)
    ms = _adpcm(WW.TAG_MS, 11025, 0.5 * scale, 4)
    wave = (rng.standard_normal(int(9000 * scale) + 1) * 0.1).astype(np.float32)
    return [(("frames", s16, 44100), ("put_frames", (s16, 44100))), (("flac", f16), ("put_flac", (f16,))),
            (("flac", f441), ("put_flac", (f441,))), (("wav", mulaw), ("put_wav", (mulaw,))), (("wav", alaw), ("put_wav", (alaw,))),
            (("wav", ima), ("put_wav", (ima,))), (("wav", ms), ("put_wav", (ms,))), (("pcm", wave), ("pcm_put", (wave,)))]


def _reference(ref, route):
    """the single route into the reference slot -> (pcm bits, feature bits)"""
    getattr(ref, route[0])(*route[1])
    pcm = ref.pcm()
    ref.logmel_resident()
    return _bits(pcm), _bits(ref.features())


def _check_items(s, ref, pairs, results, first):
    for k, ((_ent, route), r) in enumerate(zip(pairs, results)):
        assert isinstance(r, tuple), (k, r)
        want_pcm, want_feat = _reference(ref, route)
        got = s.pcm(first + k)
        assert r[0] == got.shape[0] == want_pcm.shape[0] and np.array_equal(_bits(got), want_pcm), k
        s.logmel_resident(first + k)
        assert np.array_equal(_bits(s.features(first + k)), want_feat), k


def _budget(lib, bytes_):
    prev, nb = C.c_int64(0), C.c_int32(0)
    assert lib.wlx_debug_put_many_budget(bytes_, C.byref(prev), C.byref(nb)) == 0
    return prev.value, nb.value


def test_one_call_of_every_route_equals_the_single_routes_and_touches_nothing_else(engine):
    s, ref = engine.create_slot(12, 5), engine.create_slot(1, 5)
    try:
        keep = np.linspace(-1, 1, 7001, dtype=np.float32)
        s.pcm_put(keep, 0)
        s.pcm_put(keep[::-1].copy(), 9)
        pairs = _entries()
        results = s.put_many([p[0] for p in pairs], first_item=1, with_info=True)
        assert results[1][1].sample_rate == 16000 and results[2][1].channels == 2 and results[3][1].format_tag == WW.TAG_MULAW
        assert results[0][1] is None and results[7][1] is None
        _check_items(s, ref, pairs, results, 1)
        assert _budget(s.lib, 0)[1] == 1                                                   # one sub-batch under the default budget
        assert np.array_equal(_bits(s.pcm(0)), _bits(keep)) and np.array_equal(_bits(s.pcm(9)), _bits(keep[::-1]))
        assert s.pcm_count(10) == 0 and s.pcm_count(11) == 0
        # ---- a second call with shorter files into the same items: nothing of the first call's scratch shows
        short = _entries(0.4)
        results = s.put_many([p[0] for p in short], first_item=1)
        _check_items(s, ref, short, results, 1)
    finally:
        s.close()
        ref.close()


def _flac_need(lib, data):
    """the scratch share of a FLAC entry as csrc/put_many.hip counts it (include/wlx.h: file bytes, frame table, status words, planes, frames)"""
    from whisperlive_amd import _lib as L
    info = L.wlx_flac_info()
    assert lib.wlx_flac_probe(data, len(data), C.byref(info)) == 0
    up = lambda v: (v + 255) & ~255                                                         # noqa: E731
    ns4 = info.total_samples * info.channels * 4
    return 512 + up(info.n_frames * 32) + up(info.n_frames * 4) + up(len(data)) + 2 * up(ns4)


def test_a_budget_that_forces_three_sub_batches_gives_the_same_items(engine):
    s, ref = engine.create_slot(9, 5), engine.create_slot(1, 5)
    pairs = _entries()
    pairs = [pairs[0], pairs[2]] + pairs[3:] + [pairs[1]]           # frames | the 44.1 kHz FLAC | everything else
    need = _flac_need(s.lib, pairs[1][0][1])
    prev, _ = _budget(s.lib, need)                                  # the large FLAC fits alone, and with nothing beside it
    try:
        results = s.put_many([p[0] for p in pairs], first_item=0)
        assert _budget(s.lib, 0)[1] == 3
        _check_items(s, ref, pairs, results, 0)
        # ... and one byte less refuses that entry alone: its item stays as it was, the others are exact
        _budget(s.lib, need - 1)
        before = _bits(s.pcm(1))
        results = s.put_many([p[0] for p in pairs], first_item=0)
        from whisperlive_amd import _lib as L
        assert isinstance(results[1], L.WlxError) and results[1].code == L.ERR_ARG
        assert np.array_equal(_bits(s.pcm(1)), before)
        for k in (0, 2, 7):
            assert isinstance(results[k], tuple) and np.array_equal(_bits(s.pcm(k)), _reference(ref, pairs[k][1])[0])
    finally:
        _budget(s.lib, -1)
        assert _budget(s.lib, 0)[0] == prev
        s.close()
        ref.close()


def test_a_frame_that_fails_on_the_device_and_a_refused_rate_cost_only_themselves(engine):
    from whisperlive_amd import _lib as L
    s, ref = engine.create_slot(6, 5), engine.create_slot(1, 5)
    try:
        old = (np.arange(5000, dtype=np.float32) / 5000.0)
        for item in range(5):
            s.pcm_put(old + item, item)
        pairs = _entries(0.4)
        bad, _pcm = broken_frame_stream()
        odd = np.zeros((4410, 1), np.float32)
        entries = [pairs[1][0], ("flac", bad), pairs[3][0], ("frames", odd, 44101), pairs[7][0]]
        results = s.put_many(entries, first_item=0)
        assert isinstance(results[1], L.WlxError) and results[1].code == L.ERR_DATA
        assert s.pcm_count(1) == 0                                                          # the damaged entry's item holds nothing
        assert isinstance(results[3], L.WlxError) and results[3].code == L.ERR_ARG
        assert np.array_equal(_bits(s.pcm(3)), _bits(old + 3))                              # the refused entry's item is as it was
        for k in (0, 2, 4):
            route = (pairs[1][1], None, pairs[3][1], None, pairs[7][1])[k]
            assert isinstance(results[k], tuple) and np.array_equal(_bits(s.pcm(k)), _reference(ref, route)[0])
        # a stream the HOST index finds damaged: answered before any launch, the item as it was
        torn = bytearray(pairs[1][0][1])
        torn[len(torn) // 2] ^= 0x20
        results = s.put_many([("flac", bytes(torn)), pairs[3][0]], first_item=3)
        assert isinstance(results[0], L.WlxError) and results[0].code == L.ERR_DATA
        assert np.array_equal(_bits(s.pcm(3)), _bits(old + 3)) and isinstance(results[1], tuple)
    finally:
        s.close()
        ref.close()


def test_a_bad_count_or_first_item_refuses_the_call_and_changes_nothing(engine):
    from whisperlive_amd import _lib as L
    s = engine.create_slot(3, 5)
    try:
        old = np.linspace(-1, 1, 3000, dtype=np.float32)
        for item in range(3):
            s.pcm_put(old * (item + 1), item)
        wave = np.ones(100, np.float32)
        arr, res = (L.wlx_put_entry * 65)(), (L.wlx_put_result * 65)()
        for k in range(65):
            arr[k].kind, arr[k].data, arr[k].n = L.PUT_PCM, wave.ctypes.data, 100
        call = lambda first, n, a=arr, r=res: s.lib.wlx_pcm_put_many(engine._h, s.sid, first, n, a, r)      # noqa: E731
        assert call(0, 0) == L.ERR_ARG and call(0, 65) == L.ERR_ARG and call(-1, 1) == L.ERR_ARG and call(2, 2) == L.ERR_ARG
        assert call(0, 1, None) == L.ERR_ARG and call(0, 1, arr, None) == L.ERR_ARG
        for item in range(3):
            assert np.array_equal(_bits(s.pcm(item)), _bits(old * (item + 1)))
        with pytest.raises(L.WlxError):
            s.put_many([("pcm", wave)] * 2, first_item=2)
        assert call(2, 1) == 0 and res[0].status == 0 and res[0].n_out == 100 and np.array_equal(s.pcm(2), wave)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the job
def test_transcribe_many_with_wave_put_equals_the_default(gpu, monkeypatch):
    from whisperlive_amd import engine as E
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from .test_gpu_many_files import BATCH, CLIPS, KW, _files
    spec = H.TINY_EN
    f = _files()
    files = [f["A"], f["B"], f["C"]]                                 # a 16-bit WAV (frames), a FLAC file, a waveform
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=8)
    calls = []
    real = E.Slot.put_many
    monkeypatch.setattr(E.Slot, "put_many", lambda self, entries, **kw: calls.append([e[0] for e in entries]) or real(self, entries, **kw))
    try:
        kw = dict(clip_timestamps=[[dict(c) for c in cl] for cl in CLIPS], chunk_length=BC.CHUNK_LENGTH, vad_filter=False, batch_size=BATCH, **KW)
        want = BatchedInferencePipeline(hip).transcribe_many(files, **kw)
        assert calls == []
        got = BatchedInferencePipeline(hip).transcribe_many(files, wave_put=True, **kw)
        assert calls == [["frames", "flac", "pcm"]]                  # the wave went up in one call
        assert len(got) == len(want) == 3
        for (gs, gi), (ws, wi) in zip(got, want):
            assert len(gs) == len(ws) and ws
            for g, w in zip(gs, ws):
                assert (g.tokens, g.seek, g.start, g.end, g.id, g.text) == (w.tokens, w.seek, w.start, w.end, w.id, w.text)
            assert (gi.duration, gi.language, gi.duration_after_vad) == (wi.duration, wi.language, wi.duration_after_vad)
    finally:
        hip.close()
        hip.engine.close()
