#!/usr/bin/env python
"""The front of a many-files job: one put per file (today's default, `batched._put_audio` in a loop) against ONE Slot.put_many call per
wave (wlx_pcm_put_many: one wait), on the same process, model and slot.

The workload is scripts/many_files_time.py's: --files (default 48) synthetic recordings of --seconds (default 20), half 8 kHz G.711
mu-law WAV, half 16 kHz 16-bit FLAC, alternating; --batch (default 12) chunks per decode step, one wave; seeded weights, beam 5, the
seeded energy-following gate, --max-new-tokens forced tokens per chunk. Shapes: tiny.en and small.en.

Per shape, after one warm-up of each leg, --pairs (default 5) ALTERNATING pairs of
  (1) the front alone: the loop of `_put_audio` over the wave's files, then `_put_audio_many` of the same files into the same items
      (wall time; each leg ends in the wait of its last put, so the clock covers finished work). --front-reps (default 5) repeats per
      pair are summed, because one front is a few milliseconds;
  (2) the whole job: transcribe_many() (the default = the code of before this option) then transcribe_many(wave_put=True);
and the split of the DEFAULT job's front into puts, gate and language + the rest (clips, tokenizers), from clocks around
many_files._put_audio / _gate / _languages. Before anything is timed, the resident PCM of every item after the two fronts is compared
bit for bit, and the two jobs' tokens and times file by file.
usage: python scripts/put_many_time.py [--files 48] [--seconds 20] [--batch 12] [--pairs 5] > profiles/put_many_time.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.many_files_time import make_files      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--front-reps", type=int, default=5)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--models", default="tiny.en,small.en")
    a = ap.parse_args()

    from whisperlive_amd import batched as B, engine as E, many_files as MF, vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights

    files = make_files(a.files, a.seconds)
    items = [a.batch + k for k in range(a.files)]
    print(f"scripts/put_many_time.py on one MI355X: {a.files} files of {a.seconds:g} s (8 kHz G.711 mu-law WAV and 16 kHz FLAC, alternating; "
          f"{sum(len(f) for f in files) / 1e6:.2f} MB in all), batch_size {a.batch}, beam 5, {a.max_new_tokens} forced tokens per chunk, the gate on; "
          f"wall times in seconds, {a.pairs} alternating pairs after one warm-up of each leg", flush=True)
    fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)             # noqa: E731
    p50 = lambda xs: float(np.median(xs))                         # noqa: E731
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)

    # clocks around the three stages of the default front (many_files looks the names up at call time)
    split = {"puts": 0.0, "gate": 0.0, "language": 0.0}

    def clocked(name, fn):
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                split[name] += time.perf_counter() - t0
        return run
    MF._put_audio = clocked("puts", MF._put_audio)
    MF._put_audio_many = clocked("puts", MF._put_audio_many)
    MF._gate = clocked("gate", MF._gate)
    MF._languages = clocked("language", MF._languages)

    for name in [m for m in a.models.split(",") if m]:
        spec = SPECS[name]
        eng = E.HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
        hip = WhisperModelHIP(name, engine=eng, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=a.batch + a.files, vad_model=gate)
        pipe = BatchedInferencePipeline(hip)
        kw = dict(language="en", temperature=0.0, beam_size=5, max_new_tokens=a.max_new_tokens, without_timestamps=True, vad_filter=True,
                  suppress_tokens=[-1, hip._base_tokenizer.eot], batch_size=a.batch)
        slot = hip._slot(rows=5)

        def front_loop(reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                for f, item in zip(files, items):
                    B._put_audio(hip, slot, f, item)
            return time.perf_counter() - t0

        def front_many(reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                out = B._put_audio_many(hip, slot, files, items)
                assert not any(isinstance(o, Exception) for o in out)
            return time.perf_counter() - t0

        def job(**extra):
            for k in split:
                split[k] = 0.0
            t0 = time.perf_counter()
            out = pipe.transcribe_many(files, **kw, **extra)
            return time.perf_counter() - t0, out, dict(split), dict(pipe.many_timing)

        try:
            front_loop(1)
            want_pcm = [slot.pcm(i).view(np.uint32).copy() for i in items]
            for i in items:
                slot.pcm_put(np.zeros(16, np.float32), i)
            front_many(1)
            same_pcm = all(np.array_equal(slot.pcm(i).view(np.uint32), w) for i, w in zip(items, want_pcm))
            _, want, _, _ = job()
            _, got, _, _ = job(wave_put=True)
            same = all([x.tokens for x in g[0]] == [x.tokens for x in w[0]] and [(x.start, x.end) for x in g[0]] == [(x.start, x.end) for x in w[0]]
                       for g, w in zip(got, want))
            fl, fm, jl, jm, parts, fronts_d, fronts_w = [], [], [], [], [], [], []
            for _ in range(a.pairs):
                fl.append(front_loop(a.front_reps) / a.front_reps)
                fm.append(front_many(a.front_reps) / a.front_reps)
                t, _, sp, tm = job()
                jl.append(t); parts.append(sp); fronts_d.append(tm["front_s"])
                t, _, _, tm = job(wave_put=True)
                jm.append(t); fronts_w.append(tm["front_s"])
            audio_s = a.files * a.seconds
            print(f"\n{name}: resident PCM of all {a.files} items equal bit for bit after the two fronts: {same_pcm}; "
                  f"tokens and times of the two jobs equal file by file: {same}")
            print(f"  front alone, loop of _put_audio ({a.files} puts, {a.files} waits):  {fmt(fl)}   p50 {p50(fl):.4f}")
            print(f"  front alone, _put_audio_many (1 call, 1 wait):           {fmt(fm)}   p50 {p50(fm):.4f}")
            print(f"  put_many / loop = {p50(fm) / p50(fl):.3f} (loop / put_many = {p50(fl) / p50(fm):.2f} x)")
            print(f"  whole job, default (per-file puts):  {fmt(jl)}   p50 {p50(jl):.4f}  ({audio_s / p50(jl):.0f} x real time)")
            print(f"  whole job, wave_put=True:            {fmt(jm)}   p50 {p50(jm):.4f}  ({audio_s / p50(jm):.0f} x real time)")
            print(f"  wave_put / default = {p50(jm) / p50(jl):.3f}")
            print(f"  front of the job (before the first decode), default:  {fmt(fronts_d)}   p50 {p50(fronts_d):.4f}")
            print(f"  front of the job (before the first decode), wave_put: {fmt(fronts_w)}   p50 {p50(fronts_w):.4f}")
            for k in ("puts", "gate", "language"):
                xs = [p[k] for p in parts]
                print(f"  default front, {k:9s}: {fmt(xs)}   p50 {p50(xs):.4f}  ({100 * p50(xs) / p50(fronts_d):.0f} % of the front)")
            rest = [f - sum(p.values()) for f, p in zip(fronts_d, parts)]
            print(f"  default front, the rest : {fmt(rest)}   p50 {p50(rest):.4f}  (clips, tokenizers, options)")
        finally:
            hip.close()
            eng.close()
    gate.close()


if __name__ == "__main__":
    main()
