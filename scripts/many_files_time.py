#!/usr/bin/env python
"""An archive of short recordings: (a) what a user does today — a loop of BatchedInferencePipeline.transcribe over the files — against
(b) ONE BatchedInferencePipeline.transcribe_many job whose decode groups mix files, on the same process, model and slot.

The files: --files (default 48) synthetic recordings of --seconds (default 20) each (oracle.logmel.speech_like_pcm, a seed per file),
half of them 8 kHz G.711 mu-law WAV, half 16 kHz 16-bit FLAC, alternating. scripts/longform_time.py's conventions: seeded weights, beam 5,
the seeded energy-following gate, exactly --max-new-tokens tokens per chunk (the end-of-text token is suppressed). Shapes: tiny.en and
small.en. Both legs decode --batch (default 12) chunks per step on a transcriber of max_batch = batch + files (one wave).

Per shape one warm-up of each leg, then --pairs (default 3) ALTERNATING pairs (loop, job, loop, job, ...): wall time of each leg, segments
consumed; the ratio of the medians; and the share of the job's wave spent before its first decode (puts + gate + language:
pipe.many_timing). Before anything is timed the two legs' tokens are compared file by file.
usage: python scripts/many_files_time.py [--files 48] [--seconds 20] [--batch 12] [--pairs 3] > profiles/many_files_time.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_files(n, seconds):
    from scipy.signal import resample_poly

    from oracle.logmel import speech_like_pcm
    from tests import flac_writer as W
    from tests import wav_writer as WW
    files = []
    for i in range(n):
        x = speech_like_pcm(float(seconds), seed=100 + i).astype(np.float64)
        if i % 2 == 0:
            q = np.clip(np.round(resample_poly(x, 1, 2) * 32767.0), -32768, 32767).astype(np.int16)
            files.append(WW.write_g711(q[:, None], 8000, WW.TAG_MULAW))
        else:
            q = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int64)
            files.append(W.encode_stream(q[:, None], 16000, 16, W.split_blocks(q.shape[0], 4096), subframe={"type": "fixed", "order": 2, "k": 11}))
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--models", default="tiny.en,small.en")
    a = ap.parse_args()

    from whisperlive_amd import engine as E, vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights

    files = make_files(a.files, a.seconds)
    print(f"scripts/many_files_time.py on one MI355X: {a.files} files of {a.seconds:g} s (8 kHz G.711 mu-law WAV and 16 kHz FLAC, alternating; "
          f"{sum(len(f) for f in files) / 1e6:.2f} MB in all), batch_size {a.batch}, beam 5, {a.max_new_tokens} forced tokens per chunk, the gate on; "
          f"wall times in seconds, {a.pairs} alternating pairs after one warm-up of each leg", flush=True)
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    for name in [m for m in a.models.split(",") if m]:
        spec = SPECS[name]
        eng = E.HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
        hip = WhisperModelHIP(name, engine=eng, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=a.batch + a.files, vad_model=gate)
        pipe = BatchedInferencePipeline(hip)
        kw = dict(language="en", temperature=0.0, beam_size=5, max_new_tokens=a.max_new_tokens, without_timestamps=True, vad_filter=True,
                  suppress_tokens=[-1, hip._base_tokenizer.eot], batch_size=a.batch)

        def loop():
            t0 = time.perf_counter()
            out = []
            for f in files:
                segs, info = pipe.transcribe(f, **kw)
                out.append((list(segs), info))
            return time.perf_counter() - t0, out

        def job():
            t0 = time.perf_counter()
            out = pipe.transcribe_many(files, **kw)
            return time.perf_counter() - t0, out

        try:
            _, want = loop()
            _, got = job()
            chunks = sum(len(s) for s, _ in want)
            same = all([x.tokens for x in g[0]] == [x.tokens for x in w[0]] and [(x.start, x.end) for x in g[0]] == [(x.start, x.end) for x in w[0]]
                       for g, w in zip(got, want))
            tl, tj, front = [], [], []
            for _ in range(a.pairs):
                tl.append(loop()[0])
                tj.append(job()[0])
                front.append(pipe.many_timing["front_s"] / pipe.many_timing["total_s"])
            fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)
            ml, mj = float(np.median(tl)), float(np.median(tj))
            audio_s = a.files * a.seconds
            print(f"\n{name}: {chunks} segments in all, {pipe.many_timing['waves']} wave(s); tokens and times of the two legs equal file by file: {same}")
            print(f"  loop of transcribe:  {fmt(tl)}   p50 {ml:.4f}  ({audio_s / ml:.0f} x real time)")
            print(f"  transcribe_many job: {fmt(tj)}   p50 {mj:.4f}  ({audio_s / mj:.0f} x real time)")
            print(f"  job / loop = {mj / ml:.3f} (loop / job = {ml / mj:.2f} x)")
            print(f"  share of the job's wave before its first decode (puts + gate + language): {fmt(front)}   p50 {float(np.median(front)):.3f}")
        finally:
            hip.close()
            eng.close()
    gate.close()


if __name__ == "__main__":
    main()
