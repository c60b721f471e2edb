"""Timing of the FLAC front end (Slot.put_flac: csrc/flac.hip) against the route it replaces (audio_io.read_audio on the host, then
Slot.put_frames), on ONE file: --seconds (default 600) of 44.1 kHz 16-bit stereo FLAC written by tests/flac_writer.py from noise plus
tones (mid/side, FIXED order 2, Rice parameter from the first block's residuals: not a trivial bitstream), 4096-sample blocks.
  device:  wall time of put_flac, median of 5; of the last call the host index + CRC time, and the HIP-event times of the upload, of
           flac_frames_kernel, flac_finish_kernel and the resample launch (wlx_debug_flac_timings); the same for tests/golden/jfk_head.flac.
           Then put_frames on the SAME samples (what read_audio would have returned), once: the device half of the parent route.
  --host-decode: the host half of the parent route alone, read_audio on the same file, once (it takes minutes; needs no device).
usage: python scripts/flac_time.py [--seconds S] > profiles/flac_time.txt ;  python scripts/flac_time.py --host-decode >> profiles/flac_time.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
RATE, BLOCK = 44100, 4096


def make_file(seconds):
    from tests import flac_writer as W
    rng = np.random.RandomState(11)
    n = seconds * RATE
    t = np.arange(n) / RATE
    cols = [0.35 * np.sin(2 * np.pi * (180 + 90 * c) * t) + 0.2 * np.sin(2 * np.pi * (1700 + 400 * c) * t) + 0.03 * rng.standard_normal(n)
            for c in range(2)]
    pcm = np.round(np.stack(cols, axis=1) * 32767).astype(np.int64)
    first = pcm[:BLOCK]
    res = np.concatenate([((first[:, 0] + first[:, 1]) >> 1), first[:, 0] - first[:, 1]])
    res = res[2:] - 2 * res[1:-1] + res[:-2]
    k = max(0, int(np.log2(max(1.0, np.abs(res).mean()))))
    t0 = time.perf_counter()
    data = W.encode_stream(pcm, RATE, 16, W.split_blocks(n, BLOCK), assignment=W.MID_SIDE, subframe={"type": "fixed", "order": 2, "k": k})
    return data, pcm, k, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--host-decode", action="store_true")
    a = ap.parse_args()
    data, pcm, k, wsec = make_file(a.seconds)
    head = (f"file: {a.seconds} s, 44.1 kHz x 2 x 16 bit, {len(data) / 1e6:.1f} MB of FLAC ({pcm.size * 2 / 1e6:.1f} MB of PCM), "
            f"{-(-pcm.shape[0] // BLOCK)} frames of {BLOCK}, Rice k = {k} (written in {wsec:.0f} s)")
    if a.host_decode:
        from whisperlive_amd import audio_io
        t0 = time.perf_counter()
        frames, sr = audio_io.read_audio(data)
        dt = time.perf_counter() - t0
        assert sr == RATE and np.array_equal(np.round(frames.astype(np.float64) * 32768).astype(np.int64), pcm)
        print(head)
        print(f"parent route, host half: audio_io.read_audio (read_flac, MD5 verified) {dt:.1f} s = {a.seconds / dt:.2f} x real time, once, one CPU thread")
        return
    import ctypes as C
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    spec = SPECS["tiny.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = eng.create_slot(1, 5)
    print(head)

    def timed(blob, label):
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            n, info = slot.put_flac(blob)
            walls.append((time.perf_counter() - t0) * 1e3)
        ms = (C.c_float * 5)()
        from whisperlive_amd._lib import check
        check(eng.lib.wlx_debug_flac_timings(eng._h, slot.sid, ms))
        print(f"{label}: put_flac wall median of 5 {np.median(walls):.2f} ms (all: {', '.join(f'{w:.2f}' for w in walls)}) -> {n} samples resident; "
              f"last call: host index + CRC {ms[0]:.2f} ms, upload {ms[1]:.2f} ms, flac_frames_kernel {ms[2]:.2f} ms, flac_finish_kernel {ms[3]:.3f} ms, "
              f"resample_kernel {ms[4]:.3f} ms")
        return n
    try:
        n = timed(data, "device route")
        frames = (pcm / 32768.0).astype(np.float32)              # what read_audio returns for this file (tests/test_flac_writer.py)
        t0 = time.perf_counter()
        m = slot.put_frames(frames, RATE)
        dt = (time.perf_counter() - t0) * 1e3
        assert m == n
        print(f"parent route, device half: put_frames of the decoded float32 frames {dt:.2f} ms, once (the host half, read_audio, is timed by --host-decode)")
        with open(os.path.join("tests", "golden", "jfk_head.flac"), "rb") as f:
            timed(f.read(), "jfk_head.flac (3.34 s, 24 bit stereo, 32 frames of 4608; parent: read_flac 1.3-1.4 s)")
    finally:
        slot.close()
        eng.close()


if __name__ == "__main__":
    main()
