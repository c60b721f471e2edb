"""Timing of the telephony WAV front end (Slot.put_wav: csrc/adpcm.hip) against the route it replaces (audio_io.read_wav on the host,
then Slot.put_frames of the decoded float32 frames), on ONE file per format: --seconds (default 600) of 8 kHz stereo as G.711 mu-law,
G.711 A-law, IMA ADPCM and MS ADPCM (block_align 512: 256 bytes per channel). The payloads are seeded random codes / nibbles behind valid
block headers (tests/wav_writer.py random_adpcm): the decode cost of these formats does not depend on the content.
  device route: wall time of put_wav, 2 warm-up calls, then 9 calls; the two routes ALTERNATE call by call so that both see the same
                machine, and the median and the whole list are printed.
  host route:   read_wav (host decode, one CPU thread; median of 3) + put_frames (device half; alternated with put_wav as above).
Before anything is timed the two routes' resident PCM is compared bit for bit.
usage: python scripts/wav_time.py [--seconds S] > profiles/telephony_wav_time.txt"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
RATE, CH, BLOCK = 8000, 2, 512


def make_file(kind, seconds):
    from tests import wav_writer as W
    n = seconds * RATE
    if kind in ("mulaw", "alaw"):
        rng = np.random.RandomState(3)
        tag = W.TAG_MULAW if kind == "mulaw" else W.TAG_ALAW
        return W.container(tag, CH, RATE, 8, CH, rng.randint(0, 256, size=n * CH).astype(np.uint8).tobytes(), fmt_extra=b"\0\0")
    tag = W.TAG_IMA if kind == "ima" else W.TAG_MS
    spb = (W.ima_samples_per_block if kind == "ima" else W.ms_samples_per_block)(BLOCK, CH)
    return W.random_adpcm(tag, -(-n // spb), CH, BLOCK, rate=RATE, seed=5, fact=n)


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    a = ap.parse_args()
    from whisperlive_amd import audio_io
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    spec = SPECS["tiny.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    dev, ref = eng.create_slot(1, 5), eng.create_slot(1, 5)
    print(f"scripts/wav_time.py on one MI355X: {a.seconds} s of {RATE} Hz x {CH} channels per format; wall times in ms, host decode on one CPU thread")
    try:
        for kind in ("mulaw", "alaw", "ima", "ms"):
            data = make_file(kind, a.seconds)
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                frames, sr = audio_io.read_wav(data)
                host.append((time.perf_counter() - t0) * 1e3)
            assert sr == RATE and frames.shape == (a.seconds * RATE, CH)
            n, info = dev.put_wav(data)
            assert ref.put_frames(frames, sr) == n
            same = np.array_equal(dev.pcm().view(np.uint32), ref.pcm().view(np.uint32))
            dev.put_wav(data); ref.put_frames(frames, sr)                                       # second warm-up of both
            tw, tf = [], []
            for _ in range(9):
                t0 = time.perf_counter(); dev.put_wav(data); tw.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); ref.put_frames(frames, sr); tf.append((time.perf_counter() - t0) * 1e3)
            fmt = lambda xs: ", ".join(f"{x:.2f}" for x in xs)
            print(f"\n{kind}: file {len(data) / 1e6:.2f} MB (decoded float32 frames {frames.nbytes / 1e6:.1f} MB), block_align {info.block_align}, "
                  f"{n} samples resident, routes bit-identical: {same}")
            print(f"  device route: put_wav median of 9 {med(tw):.2f} ms (all: {fmt(tw)})")
            print(f"  host route:   read_wav median of 3 {med(host):.1f} ms (all: {fmt(host)}) + put_frames median of 9 {med(tf):.2f} ms (all: {fmt(tf)})"
                  f" = {med(host) + med(tf):.1f} ms -> {(med(host) + med(tf)) / med(tw):.1f} x the device route")
    finally:
        dev.close(); ref.close(); eng.close()


if __name__ == "__main__":
    main()
