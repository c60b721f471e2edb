"""Timing of the HIP M2M100 translation engine at small100's dimensions (d_model 1024, 16 heads, 12 + 3 layers, FFN 4096, vocabulary
128112) on seeded weights, device times from the engine's HIP events (wlx_mt_debug_timings):
  * per-call latency for 1 and 8 segments of 16 / 64 source tokens, beam 5, 31 decode steps (max_length 32; the seeded weights do
    not finish early), split into encoder pass and decode loop, and the decode time per step;
  * p50 of an ASR window (Whisper-small.en, 30 s, log-mel + encoder + beam-5 decode of 64 tokens) with and without a concurrent
    translation stream on its own slot.
usage: python scripts/mt_time.py [--mt-only]   (--mt-only: the translation calls alone, e.g. under rocprofv3 --kernel-trace --stats)"""
import dataclasses
import sys
import threading
import time

import numpy as np

sys.path.insert(0, ".")
from oracle import logmel as olm          # synthetic PCM generator only
from whisperlive_amd.engine import HipWhisperEngine, TokenIds
from whisperlive_amd.mt_weights import SMALL100, MTGenOptions, random_mt_weights
from whisperlive_amd.specs import get_spec
from whisperlive_amd.translation import HipMTEngine
from whisperlive_amd.weights import random_weights

spec = dataclasses.replace(SMALL100, decoder_start_id=0)
mt = HipMTEngine(spec, random_mt_weights(spec, seed=3), device=0, max_batch=8, max_rows=5, max_src=64)
o = MTGenOptions(num_beams=5, max_length=32, early_stopping=True)
rng = np.random.default_rng(0)
print("small100 dims, seeded weights, beam 5, max_length 32 (measured, HIP events)")
for n_seg in (1, 8):
    for L in (16, 64):
        srcs = [[128010] + [int(x) for x in rng.integers(4, 128000, size=L - 2)] + [2] for _ in range(n_seg)]
        for _ in range(2):
            mt.translate_ids(srcs, o)
        walls, encs, decs, steps = [], [], [], 0
        for _ in range(5):
            t0 = time.perf_counter()
            mt.translate_ids(srcs, o)
            walls.append(1e3 * (time.perf_counter() - t0))
            e, d, steps = mt.timings()
            encs.append(e)
            decs.append(d)
        e, d, w = float(np.median(encs)), float(np.median(decs)), float(np.median(walls))
        print(f"  {n_seg} segment(s) x {L} tokens: call {w:.2f} ms wall | encoder {e:.3f} ms, decode {d:.2f} ms for {steps} steps "
              f"= {d / max(steps, 1):.3f} ms/step ({n_seg * 5} rows)")

if "--mt-only" in sys.argv:
    mt.close()
    sys.exit(0)
asr_spec = get_spec("small.en")
asr = HipWhisperEngine(asr_spec, random_weights(asr_spec, seed=0), device=0)
slot = asr.create_slot(1, 5)
pcm = olm.speech_like_pcm(30.0, seed=1234)
tb = asr_spec.vocab - 1501
ids = TokenIds(tb - 106, tb - 107, tb - 1, tb, tb - 2, 220)
kw = dict(beam_size=5, patience=1.0, max_length=1 + 64, suppress_tokens=[ids.eot])


def window():
    t0 = time.perf_counter()
    T = slot.logmel(pcm)
    slot.encode(1, seek=[0], seg=[min(T - 1, 3000)])
    slot.generate([[ids.sot]], ids, **kw)
    return 1e3 * (time.perf_counter() - t0)


for _ in range(3):
    window()
solo = float(np.median([window() for _ in range(15)]))
stop, n_tr = threading.Event(), [0]
srcs8 = [[128010] + [int(x) for x in rng.integers(4, 128000, size=30)] + [2] for _ in range(8)]


def loop():
    while not stop.is_set():
        mt.translate_ids(srcs8, o)
        n_tr[0] += 1


th = threading.Thread(target=loop)
th.start()
time.sleep(0.5)
try:
    busy = float(np.median([window() for _ in range(15)]))
finally:
    stop.set()
    th.join()
print(f"ASR window (small.en, 30 s, beam 5, 64 tokens) p50: {solo:.2f} ms alone, {busy:.2f} ms beside a translation stream "
      f"(8 segments x 32 tokens per call, {n_tr[0]} calls meanwhile)")
slot.close()
asr.close()
mt.close()
