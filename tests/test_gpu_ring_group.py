"""GPU tests (-m gpu) of the ring group of live multichannel sessions (include/wlx.h wlx_ring_group_create / _lane / _append_frames /
_destroy): for any cutting of an interleaved stream into packets followed by a flush, lane c is BIT-IDENTICAL to a mono ring given
wlx_ring_set_format(fmt, 1, rate) and fed channel c's frames with the same cutting — dropped / base / resident agree at every packet,
across trims and a growth — hence to the one-shot resample of that channel; a lane is a full ring for the log-mel front end and the
VAD gate; refusals change nothing; the per-channel host oracle agrees within the bound of the mono stream form."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import resample_kernel_ref as R
from whisperlive_amd import _lib
from whisperlive_amd import stream_resample as SR
from whisperlive_amd._lib import WlxError

pytestmark = pytest.mark.gpu

FILL = np.float32(-7.25)
# (wire format, rate, channels): the issue's table; the last is the convert-only path (16 kHz in)
CASES = [("mulaw", 8000, 2), ("alaw", 8000, 8), ("int16", 48000, 2), ("float32", 44100, 3), ("uint8", 16000, 2)]
IDS = [f"{f}-{r}-{c}" for f, r, c in CASES]
CUTTINGS = ["one_packet", "one_frame_packets", "all_shorter_than_reach", "random_with_empty"]
TILE = 1024                                                                        # outputs per workgroup at every rate of the table


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stream_of(name, rate, channels, n=None):
    """seeded [n, channels] wire frames, n = 3 * reach + tile + 37 input frames unless the test says otherwise"""
    code, dt = SR.WIRE_FORMATS[name]
    n = 3 * R.reach(*R.ratio(rate)) + TILE + 37 if n is None else n
    if dt == np.uint8:
        x = np.random.default_rng(code * 1000 + channels).integers(0, 256, (n, channels), dtype=np.uint8)
        x[:256, 0] = np.arange(256)                                                # every code at least once
        return code, x
    return code, np.ascontiguousarray(R.multichannel(n, rate, channels, R.S16 if name == "int16" else R.F32))


def packets_of(n, rate, cutting, seed):
    """-> list of (a, b, flush): the packets [a, b) of the stream, the flush on the last packet or as an empty call behind the data"""
    rng = np.random.default_rng(seed)
    short = max(1, R.reach(*R.ratio(rate)) - 1)
    if cutting == "one_packet":
        edges, empty_flush = [0, n], False
    elif cutting == "one_frame_packets":
        edges, empty_flush = list(range(0, 41)) + [n], True
    elif cutting == "all_shorter_than_reach":
        edges, empty_flush = list(range(0, n, short)) + [n], False
    else:
        rand = np.sort(rng.integers(0, n + 1, 24))
        edges, empty_flush = np.sort(np.concatenate((rand, rand[::4], [0, 0, n]))).tolist(), True
    pk = [(int(a), int(b), False) for a, b in zip(edges[:-1], edges[1:])]
    if empty_flush:
        return pk + [(n, n, True)]
    return pk[:-1] + [(pk[-1][0], pk[-1][1], True)]


@pytest.fixture(scope="module")
def eng(gpu):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    e = HipWhisperEngine(H.TINY_EN, random_weights(H.TINY_EN, seed=7))
    yield e
    e.close()


def run_both(eng, code, rate, x, packets, max_resident=0, trim=0, capacity=0):
    """the group over the interleaved stream and C mono rings over its columns, packet by packet with the same cutting;
    asserts dropped / base / resident equal at every packet -> (group lanes' concatenated new_out, mono rings' same, trims seen)"""
    ch = x.shape[1]
    group = eng.create_ring_group(code, ch, rate, capacity)
    monos = [eng.create_ring(capacity) for _ in range(ch)]
    got, want, trims = [[] for _ in range(ch)], [[] for _ in range(ch)], 0
    try:
        for r in monos:
            r.set_format(code, 1, rate)
        for i, (a, b, fl) in enumerate(packets):
            new, dropped, base, resident = group.append_frames(x[a:b], flush=fl, max_resident=max_resident, trim=trim)
            assert new.shape[0] == ch
            trims += 1 if dropped else 0
            for c in range(ch):
                m_new, m_dropped, m_base, m_resident = monos[c].append_frames(np.ascontiguousarray(x[a:b, c]), flush=fl,
                                                                              max_resident=max_resident, trim=trim)
                assert (dropped, base, resident) == (m_dropped, m_base, m_resident), (i, c)
                assert group.lane(c).state() == (base, resident) == monos[c].state(), (i, c)
                assert new[c].shape == m_new.shape, (i, c)
                got[c].append(new[c].copy())
                want[c].append(m_new)
        return [np.concatenate(g) for g in got], [np.concatenate(w) for w in want], trims, group, monos
    except BaseException:
        group.close()
        for r in monos:
            r.close()
        raise


def close_all(group, monos):
    group.close()
    for r in monos:
        r.close()


def one_shot(eng, name, code, rate, x):
    """per channel, the one-shot resample: item c of wlx_pcm_put_frames_split for F32 / S16, wlx_debug_resample of the host-decoded
    channel for the 8-bit formats (every decoded value is exact in float32)"""
    ch = x.shape[1]
    if name in ("int16", "float32"):
        slot = eng.create_slot(ch, 5)
        try:
            slot.put_frames_split(x, rate)
            return [slot.pcm(c) for c in range(ch)]
        finally:
            slot.close()
    out = []
    for c in range(ch):
        rc, ref, n_ref = R.run_hook(SR.decode_samples(x[:, c:c + 1], code), rate)
        assert rc == 0
        out.append(ref[:n_ref].copy())
    return out


@pytest.mark.parametrize("cutting", CUTTINGS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lane_is_bit_identical_to_a_mono_ring_fed_that_channel(eng, case, cutting):
    name, rate, ch = case
    code, x = stream_of(name, rate, ch)
    n = x.shape[0]
    got, want, _, group, monos = run_both(eng, code, rate, x, packets_of(n, rate, cutting, seed=rate + ch))
    try:
        total = R.out_len(n, *R.ratio(rate))
        for c in range(ch):
            assert got[c].shape[0] == total and np.array_equal(bits(got[c]), bits(want[c])), c
        if cutting == "random_with_empty":                                         # one cutting per case: also the one-shot
            for c, ref in enumerate(one_shot(eng, name, code, rate, x)):
                assert ref.shape[0] == total and np.array_equal(bits(got[c]), bits(ref)), c
    finally:
        close_all(group, monos)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_trims_and_growth_keep_the_lanes_in_step_with_the_mono_rings(eng, case):
    """max_resident = 4000, trim = 2000. A stream of 3 * reach + tile + 37 input frames is 416 .. 2254 samples at 16 kHz and can never
    exceed 4000 resident, so THIS test runs the same cases on a longer stream — the input of 9000 samples at 16 kHz, plus 37 frames —
    in packets of about 600 samples: the rule fires at least twice inside it."""
    name, rate, ch = case
    up, down = R.ratio(rate)
    code, x = stream_of(name, rate, ch, n=9000 * down // up + 37)
    n = x.shape[0]
    total = R.out_len(n, up, down)
    step = max(1, 600 * rate // 16000)
    packets = [(a, min(n, a + step), False) for a in range(0, n, step)] + [(n, n, True)]
    got, want, trims, group, monos = run_both(eng, code, rate, x, packets, max_resident=4000, trim=2000)
    try:
        assert trims >= 2
        for c in range(ch):
            assert np.array_equal(bits(got[c]), bits(want[c])), c
    finally:
        close_all(group, monos)
    # a group (and mono rings) created smaller than the stream: the growth path runs, nothing resident is lost
    got, want, _, group, monos = run_both(eng, code, rate, x, packets, capacity=700)
    try:
        slot, one = eng.create_slot(1, 5), eng.create_slot(1, 5)
        try:
            for c in range(ch):
                assert np.array_equal(bits(got[c]), bits(want[c])), c
                assert group.lane(c).state() == (0, total)
            c = ch - 1                                                             # what the grown lane HOLDS is what it returned
            T = slot.logmel_ring(group.lane(c), [(0, total)])
            assert one.logmel(got[c]) == T and np.array_equal(bits(slot.features()), bits(one.features()))
        finally:
            slot.close(); one.close()
    finally:
        close_all(group, monos)


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_a_lane_is_a_full_ring_for_the_logmel_front_end_and_the_vad_gate(eng, case):
    from oracle import silero_vad as sv
    from whisperlive_amd.vad import SileroHIPModel
    name, rate, ch = case
    code, x = stream_of(name, rate, ch)
    n = x.shape[0]
    packets = packets_of(n, rate, "all_shorter_than_reach", seed=3)
    got, want, _, group, monos = run_both(eng, code, rate, x, packets)
    vad = SileroHIPModel(sv.random_weights(0), device=0)
    slot, one = eng.create_slot(1, 5), eng.create_slot(1, 5)
    try:
        total = got[0].shape[0]
        ranges = [(17, total // 3), (total // 2 + 5, total - 11)]
        for c in range(ch):
            lane = group.lane(c)
            assert slot.logmel_ring(lane, ranges) == one.logmel_ring(monos[c], ranges)
            assert np.array_equal(bits(slot.features()), bits(one.features())), c
            a, b = vad.probs_resident(lane, 5, total - 9), vad.probs_resident(monos[c], 5, total - 9)
            assert a.shape == b.shape and a.shape[0] >= 1 and np.array_equal(bits(a), bits(b)), c
        assert not np.array_equal(bits(got[0]), bits(got[1]))                      # the channels carry different signals
    finally:
        slot.close(); one.close(); close_all(group, monos)


def test_refusals_change_nothing(eng):
    lib = _lib.load()
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    # creation: a bad channel count, format or rate is WLX_ERR_ARG and nothing is created
    for fmt, ch, rate in ((_lib.PCM_S16, 0, 48000), (_lib.PCM_S16, 9, 48000), (2, 2, 48000), (6, 2, 48000), (_lib.PCM_S16, 2, 44101),
                          (_lib.PCM_MULAW, 2, 0)):
        h = C.c_void_p()
        assert lib.wlx_ring_group_create(eng._h, 0, fmt, ch, rate, C.byref(h)) == _lib.ERR_ARG and not h.value, (fmt, ch, rate)
    code, x = stream_of("int16", 48000, 2)
    group = eng.create_ring_group(code, 2, 48000)
    try:
        new, dropped, base, resident = group.append_frames(x[:3000])
        state, held = (base, resident), [n.copy() for n in new]
        assert resident == new.shape[1] > 0

        def unchanged():
            slot, one = eng.create_slot(1, 5), eng.create_slot(1, 5)
            try:
                for c in range(2):
                    assert group.lane(c).state() == state
                    T = slot.logmel_ring(group.lane(c), [(0, resident)])
                    assert one.logmel(held[c]) == T and np.array_equal(bits(slot.features()), bits(one.features()))
            finally:
                slot.close(); one.close()

        # a lane index out of range
        for c in (-1, 2):
            h = C.c_void_p()
            assert lib.wlx_ring_group_lane(group._h, c, C.byref(h)) == _lib.ERR_ARG and not h.value
            with pytest.raises(IndexError):
                group.lane(c)
        # room for fewer samples than the packet completes: refused before anything is enqueued
        small, k = np.full((2, 3), FILL, np.float32), C.c_int64(-1)
        pkt = np.ascontiguousarray(x[3000:3600])
        rc = lib.wlx_ring_group_append_frames(group._h, pkt.ctypes.data_as(C.c_void_p), 600, 0, 0, 0, small.ctypes.data_as(f32p), 3,
                                              C.byref(k), None, None, None)
        assert rc == _lib.ERR_ARG and np.all(small == FILL)
        unchanged()
        # the writers of a plain ring refuse a lane; destroying a lane does nothing
        lane = group.lane(1)
        z = np.zeros(16, np.float32)
        assert lib.wlx_ring_append(lane._h, z.ctypes.data_as(f32p), 16, 0, 0, None, None, None) == _lib.ERR_STATE
        assert lib.wlx_ring_set_format(lane._h, _lib.PCM_S16, 1, 48000) == _lib.ERR_STATE
        assert lib.wlx_ring_append_frames(lane._h, pkt.ctypes.data_as(C.c_void_p), 10, 0, 0, 0, None, 0, C.byref(k), None, None, None) == _lib.ERR_STATE
        for call in (lambda: lane.append(z), lambda: lane.set_format(_lib.PCM_S16, 1, 48000), lambda: lane.append_frames(pkt[:10, 0].copy())):
            with pytest.raises(WlxError) as ei:
                call()
            assert ei.value.code == _lib.ERR_STATE
        lib.wlx_ring_destroy(lane._h)
        unchanged()
        # the packet that was refused goes through afterwards, as if nothing had happened: the stream state did not move either
        new2, _, _, resident2 = group.append_frames(pkt, flush=True)
        mono = eng.create_ring()
        try:
            mono.set_format(code, 1, 48000)
            a = mono.append_frames(np.ascontiguousarray(x[:3000, 1]))[0]
            b = mono.append_frames(np.ascontiguousarray(x[3000:3600, 1]), flush=True)[0]
            assert np.array_equal(bits(held[1]), bits(a)) and np.array_equal(bits(new2[1]), bits(b))
        finally:
            mono.close()
        # an append after the flush
        state, held = (0, resident2), [np.concatenate((held[c], new2[c])) for c in range(2)]
        resident = resident2
        with pytest.raises(WlxError) as ei:
            group.append_frames(pkt)
        assert ei.value.code == _lib.ERR_STATE
        with pytest.raises(WlxError) as ei:
            group.append_frames(b"", flush=True)
        assert ei.value.code == _lib.ERR_STATE
        unchanged()
    finally:
        group.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_per_channel_host_oracle_agrees_with_the_device(eng, case):
    name, rate, ch = case
    code, x = stream_of(name, rate, ch)
    n = x.shape[0]
    packets = packets_of(n, rate, "random_with_empty", seed=11)
    got, _, _, group, monos = run_both(eng, code, rate, x, packets)
    close_all(group, monos)
    host = SR.ChannelStreamResamplers(name, ch, rate)
    parts = [host.feed(np.ascontiguousarray(x[a:b]), fl) for a, b, fl in packets]
    assert host.closed and host.J == n and host.M == got[0].shape[0]
    for c in range(ch):
        h = np.concatenate([p[c] for p in parts])
        err = float(np.abs(h.astype(np.float64) - got[c].astype(np.float64)).max())
        print(f"{name} {rate} Hz channel {c}: host oracle against the device, max abs {err:.3e}")
        # the bound tests/test_gpu_stream_resample.py uses for the mono stream form's host half: each lane is that arithmetic
        assert h.shape == got[c].shape and err <= R.RESAMPLE_ATOL, c
