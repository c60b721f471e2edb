"""GPU tests (-m gpu) of the live path's stream resampler (include/wlx.h wlx_ring_set_format / wlx_ring_append_frames; test hook
wlx_debug_resample_stream): ANY cutting of a stream into packets followed by a flush is BIT-IDENTICAL to the one-shot resample of
the concatenated frames (wlx_debug_resample), the 8-bit wire formats equal the one-shot fed their host-decoded values, a ring with a
format keeps the buffer rule and holds what it returned, and a session over a real ring stays sample for sample with it — and with
the host fallback when the ring goes away mid-stream."""
import ctypes as C
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd import stream_resample as SR
from whisperlive_amd._lib import WlxError

pytestmark = pytest.mark.gpu

FILL = np.float32(-7.25)
_DT = {_lib.PCM_F32: np.float32, _lib.PCM_S16: np.int16}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def planner(rate, J, flush):
    n = C.c_int64(-1)
    assert _lib.load().wlx_resample_stream_count(rate, J, flush, C.byref(n)) == 0
    return n.value


def run_stream(frames, fmt, rate, cuts, flush, extra=5):
    """wlx_debug_resample_stream on [n, ch] wire frames -> (rc, out buffer pre-filled with FILL, n_out, per-call counts)"""
    lib = _lib.load()
    x = np.ascontiguousarray(frames, dtype=_DT.get(fmt, np.uint8))
    n, ch = x.shape
    cap = planner(rate, n, 1) + extra
    out = np.full(cap, FILL, np.float32)
    cu = np.asarray(cuts, dtype=np.int64)
    counts = np.full(cu.shape[0] + 1 + (1 if flush == 1 else 0), -1, np.int64)
    n_out = C.c_int64(-1)
    i64p = C.POINTER(C.c_int64)
    rc = lib.wlx_debug_resample_stream(0, x.ctypes.data_as(C.c_void_p), n, ch, fmt, rate, cu.ctypes.data_as(i64p), cu.shape[0], flush,
                                       out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n_out), counts.ctypes.data_as(i64p))
    return rc, out, n_out.value, counts


def cut_patterns(n, rate, seed):
    """name -> (cuts, flush mode of the hook)"""
    rng = np.random.default_rng(seed)
    short = max(1, R.reach(*R.ratio(rate)) - 1)
    rand = np.sort(rng.integers(0, n + 1, 24))
    return {
        "one_packet": ([], 1),
        "one_frame_packets": (list(range(1, 65)), 1),
        "all_shorter_than_reach": (list(range(short, n, short)), 1),
        "random_with_empty": (np.sort(np.concatenate((rand, rand[::4], [0, n]))).tolist(), 1),
        "flush_with_data": (rand[::3].tolist(), 2),
    }


def check_against_one_shot(frames, fmt, rate, want, seed):
    """every cut pattern of `frames` against the one-shot result `want` (float32 [out_len])"""
    n = frames.shape[0]
    total = want.shape[0]
    assert total == planner(rate, n, 1)
    for name, (cuts, flush) in cut_patterns(n, rate, seed).items():
        rc, out, n_out, counts = run_stream(frames, fmt, rate, cuts, flush)
        assert rc == 0, (name, _lib.load().wlx_last_error())
        assert n_out == total and np.array_equal(bits(out[:total]), bits(want)), name
        assert np.array_equal(bits(out[total:]), bits(np.full(5, FILL))), name              # floats past *n_out come back unchanged
        # before the flush every call completes exactly the outputs the planner gives for the frames seen so far
        edges = list(cuts) + [n]
        data_calls = len(edges) if flush == 1 else len(edges) - 1
        cum = np.cumsum(counts)
        assert [int(c) for c in cum[:data_calls]] == [planner(rate, int(j), 0) for j in edges[:data_calls]], name
        assert int(cum[-1]) == total and np.all(counts >= 0), name
    # no flush at all: what has been emitted is the one-shot's prefix, and nothing past it is written
    cuts, _ = cut_patterns(n, rate, seed)["random_with_empty"]
    rc, out, n_out, counts = run_stream(frames, fmt, rate, cuts, 0)
    assert rc == 0 and n_out == planner(rate, n, 0) == int(counts.sum()) <= total
    assert np.array_equal(bits(out[:n_out]), bits(want[:n_out])) and np.array_equal(bits(out[n_out:]), bits(np.full(out.shape[0] - n_out, FILL)))


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", [R.F32, R.S16])
@pytest.mark.parametrize("rate", [8000, 48000, 44100, 11025, 16000])
def test_any_cutting_then_flush_is_bit_identical_to_the_one_shot(gpu, rate, fmt, channels):
    n = 3000 + (rate // 25 + 997 * channels + 389 * fmt) % 3000
    frames = R.multichannel(n, rate, channels, fmt)
    rc, ref, n_ref = R.run_hook(frames, rate)
    assert rc == 0 and n_ref == R.out_len(n, *R.ratio(rate))
    check_against_one_shot(frames, fmt, rate, ref[:n_ref], seed=rate + channels)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [8000, 16000])
@pytest.mark.parametrize("name", ["mulaw", "alaw", "uint8"])
def test_eight_bit_formats_equal_the_one_shot_of_their_decoded_values(gpu, name, rate, channels):
    code = SR.WIRE_FORMATS[name][0]
    n = 3000 + 211 * channels + rate // 100
    rng = np.random.default_rng(code * 100 + channels)
    frames = rng.integers(0, 256, (n, channels), dtype=np.uint8)
    frames[:256, 0] = np.arange(256)                                              # every code at least once
    decoded = SR.decode_samples(frames, code)                                     # exact in float32
    rc, ref, n_ref = R.run_hook(decoded, rate)
    assert rc == 0
    check_against_one_shot(frames, code, rate, ref[:n_ref], seed=code)


def test_hook_refusals_happen_before_any_launch(gpu):
    x = np.zeros((100, 1), np.int16)
    i64p = C.POINTER(C.c_int64)

    def call(fmt=R.S16, rate=8000, cuts=(), cap=205, channels=1):
        out, n, cu = np.full(cap, FILL, np.float32), C.c_int64(-1), np.asarray(cuts, dtype=np.int64)
        rc = _lib.load().wlx_debug_resample_stream(0, x.ctypes.data_as(C.c_void_p), 100, channels, fmt, rate, cu.ctypes.data_as(i64p),
                                                   cu.shape[0], 1, out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), None)
        return rc, bool(np.all(out == FILL))

    assert call() == (0, False)
    for kw in (dict(rate=44101), dict(fmt=2), dict(fmt=6), dict(channels=0), dict(channels=9), dict(cuts=[50, 40]), dict(cuts=[101]),
               dict(cap=199)):                                                     # 200 outputs: a buffer below the planner's total
        assert call(**kw) == (_lib.ERR_ARG, True), kw


# ------------------------------------------------------------------------------------------------ the ring
@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


class HostBuffer:
    """the buffer rule of ServeClientBase.add_frames with the cap and trim the test passes per call"""

    def __init__(self, max_resident, trim):
        self.buf, self.base, self.max_resident, self.trim = np.zeros(0, np.float32), 0, max_resident, trim

    def add(self, pkt):
        dropped = 0
        if self.buf.shape[0] > self.max_resident:
            dropped = min(self.trim, self.buf.shape[0])
            self.buf = self.buf[dropped:]
            self.base += dropped
        self.buf = np.concatenate((self.buf, pkt))
        return dropped


def same_logmel(ring, slot, one, base, resident, host):
    T = slot.logmel_ring(ring, [(base, base + resident)])
    assert one.logmel(host) == T
    return np.array_equal(slot.features(), one.features())


def test_ring_with_a_format_keeps_the_buffer_rule_and_holds_what_it_returned(eng):
    rate, ch = 48000, 2
    sizes = [4096, 1, 0, 777, 3000, 50, 6000, 4096, 10, 9000, 0, 4096, 333, 12000, 4096, 7, 5000]
    frames = R.multichannel(sum(sizes), rate, ch, R.S16)
    rc, ref, n_ref = R.run_hook(frames, rate)
    assert rc == 0
    ring, slot, one = eng.create_ring(), eng.create_slot(1, 5), eng.create_slot(1, 5)
    host, got, drops, pos = HostBuffer(3000, 2000), [], 0, 0
    try:
        ring.set_format(R.S16, ch, rate)
        with pytest.raises(WlxError) as ei:                                        # a second format: refused, nothing changes
            ring.set_format(R.S16, 1, 8000)
        assert ei.value.code == _lib.ERR_STATE
        with pytest.raises(WlxError) as ei:                                        # the plain append is not for this ring
            ring.append(np.zeros(16, np.float32))
        assert ei.value.code == _lib.ERR_STATE and ring.state() == (0, 0)
        for i, n in enumerate(sizes):
            pkt = frames[pos: pos + n]
            pos += n
            last = i == len(sizes) - 1
            if i == 4:
                # room for fewer samples than the packet completes: refused before any launch, the ring as it was
                before, small, k = ring.state(), np.full(3, FILL, np.float32), C.c_int64(-1)
                rc = ring.lib.wlx_ring_append_frames(ring._h, pkt.ctypes.data_as(C.c_void_p), n, 0, 3000, 2000,
                                                     small.ctypes.data_as(C.POINTER(C.c_float)), 3, C.byref(k), None, None, None)
                assert rc == _lib.ERR_ARG and ring.state() == before and np.all(small == FILL)
            new, dropped, base, resident = ring.append_frames(pkt.tobytes() if i % 2 else pkt, flush=last, max_resident=3000, trim=2000)
            want_drop = host.add(new)
            drops += 1 if dropped else 0
            assert (dropped, base, resident) == (want_drop, host.base, host.buf.shape[0]) and ring.state() == (base, resident), i
            assert new.shape[0] == planner(rate, pos, 1 if last else 0) - sum(g.shape[0] for g in got), i
            got.append(new)
            if (dropped or i % 4 == 3 or last) and resident >= 400:
                assert same_logmel(ring, slot, one, base, resident, host.buf), ("packet", i)
        assert drops >= 3                                                          # the trim rule fired several times
        assert np.array_equal(bits(np.concatenate(got)), bits(ref[:n_ref]))        # what the calls returned IS the one-shot
        with pytest.raises(WlxError) as ei:                                        # the stream is closed
            ring.append_frames(frames[:4])
        assert ei.value.code == _lib.ERR_STATE and ring.state() == (host.base, host.buf.shape[0])
    finally:
        slot.close(); one.close(); ring.close()


def test_ring_without_a_format_is_as_before_and_takes_no_format_after_an_append(eng):
    ring, slot, one = eng.create_ring(), eng.create_slot(1, 5), eng.create_slot(1, 5)
    try:
        pcm = R.speech_like(5000, 16000).astype(np.float32)
        assert ring.append(pcm[:2000]) == (0, 0, 2000) and ring.append(pcm[2000:]) == (0, 0, 5000)
        assert same_logmel(ring, slot, one, 0, 5000, pcm)
        with pytest.raises(WlxError) as ei:
            ring.set_format(R.S16, 1, 8000)
        assert ei.value.code == _lib.ERR_STATE
        k = C.c_int64(-1)
        assert ring.lib.wlx_ring_append_frames(ring._h, pcm.ctypes.data_as(C.c_void_p), 10, 0, 0, 0, None, 0, C.byref(k), None, None, None) == _lib.ERR_STATE
        assert ring.append(pcm[:100]) == (0, 0, 5100)
        fresh = eng.create_ring()
        try:
            for bad in ((2, 1, 8000), (R.S16, 0, 8000), (R.S16, 9, 8000), (R.S16, 1, 44101)):
                with pytest.raises(WlxError) as ei:
                    fresh.set_format(*bad)
                assert ei.value.code == _lib.ERR_ARG
            fresh.set_format(_lib.PCM_ALAW, 1, 8000)                               # a refusal changed nothing: the ring still takes one
        finally:
            fresh.close()
    finally:
        slot.close(); one.close(); ring.close()


# ------------------------------------------------------------------------------------------------ the session
def mulaw_encode(x):
    """nearest mu-law code of float samples in [-1, 1) (a search over the 256 decoded values: the test needs no encoder of its own)"""
    table = SR.decode_mulaw(np.arange(256, dtype=np.uint8)).astype(np.float64)
    return np.abs(np.asarray(x, np.float64)[:, None] * 32768.0 - table[None, :]).argmin(axis=1).astype(np.uint8)


def make_session(eng):
    from whisperlive_amd.serve_client import ServeClientHIP
    tr = SimpleNamespace(engine=eng, transcribe=lambda audio, **kw: ([], SimpleNamespace(language="en", language_probability=0.99)))
    c = ServeClientHIP(MagicMock(), client_uid="u", model=None, transcriber=tr, use_vad=False, start_thread=False)
    c.set_wire_format("mulaw", 1, 8000)
    return c


@pytest.fixture(scope="module")
def phone_call():
    codes = mulaw_encode(0.5 * R.speech_like(16000, 8000, seed=9))                 # 2 s at 8 kHz
    rc, ref, n_ref = R.run_hook(SR.decode_samples(codes[:, None], _lib.PCM_MULAW), 8000)
    assert rc == 0 and n_ref == 32000
    return codes, ref[:n_ref]


def test_session_over_a_real_ring_stays_sample_for_sample_with_it(eng, phone_call, monkeypatch):
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    codes, ref = phone_call
    c = make_session(eng)
    slot, one = eng.create_slot(1, 5), eng.create_slot(1, 5)
    try:
        for i in range(0, codes.shape[0], 160):                                    # 20 ms packets
            c.add_wire_frames(codes[i: i + 160].tobytes())
        ring = c._ring
        assert ring and c.frames_np.shape[0] == planner(8000, 16000, 0) < 32000
        c.add_wire_frames(b"", flush=True)
        assert c._ring is ring and ring.state() == (0, 32000) and c.frames_np.shape[0] == 32000
        assert same_logmel(ring, slot, one, 0, 32000, c.frames_np)                 # frames_np == the ring's content
        assert np.array_equal(bits(c.frames_np), bits(ref))                        # ... == the one-shot of the whole stream
        assert (c._wire.J, c._wire.M, c.frames_offset, c.timestamp_offset) == (16000, 32000, 0.0, 0.0)
    finally:
        slot.close(); one.close(); c.on_transcription_thread_exit()


def test_host_fallback_takes_over_mid_stream_without_a_gap(eng, phone_call, monkeypatch):
    monkeypatch.delenv("WLX_PCM_RING", raising=False)
    codes, ref = phone_call
    c = make_session(eng)
    try:
        for i in range(0, 8000, 160):
            c.add_wire_frames(codes[i: i + 160].tobytes())
        assert c._ring
        on_device = c.frames_np.shape[0]
        assert on_device == planner(8000, 8000, 0) and np.array_equal(bits(c.frames_np), bits(ref[:on_device]))

        def broken(*a, **k):
            raise RuntimeError("ring lost")
        monkeypatch.setattr(c._ring, "append_frames", broken)
        for i in range(8000, codes.shape[0], 160):
            c.add_wire_frames(codes[i: i + 160].tobytes())
        c.add_wire_frames(b"", flush=True)
        assert c._ring is False and c.frames_np.shape[0] == 32000
        assert np.array_equal(bits(c.frames_np[:on_device]), bits(ref[:on_device]))   # nothing emitted is revised
        # the host half is float64 arithmetic == scipy's; RESAMPLE_ATOL is the bound of the device kernel against scipy
        err = float(np.abs(c.frames_np.astype(np.float64) - ref.astype(np.float64)).max())
        print(f"host fallback against the one-shot: max abs {err:.3e}")
        assert err <= R.RESAMPLE_ATOL
    finally:
        c.on_transcription_thread_exit()
