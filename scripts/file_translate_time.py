"""Wall time of translating a transcript: wlx_mt_translate_many (one job, the search on the device) against the route without it, a
loop of wlx_mt_translate over batches of max_batch (the search on the host, one synchronisation per decode step).

small100-size seeded weights, beam 5, n = 8 / 64 / 256 sources of 16 and of 64 tokens (the sources of a size are seeded by the size,
so every run of the script translates the same ones). Two regimes:
  * default: peaked weights, max_length 200 — EOS is lifted, the groups finish after 2-5 decode steps (short segments);
  * --long:  unpeaked weights, max_length 32 — no beam finishes early, every group runs 31 decode steps (the regime of
             scripts/mt_time.py, and the length of a translated sentence).
The two legs run as alternating pairs in one process; per size the script prints the median of each leg, the ratio, the
pair-to-pair spread of the ratio, the decode steps each leg ran and how many translations are token for token the same.

--end_to_end: one 10-minute synthetic recording through BatchedInferencePipeline (small.en, seeded weights, the VAD gate on, 32
tokens per chunk) without and with target_language (the --long translation model: 31 decode steps per group), alternating pairs.

The host looks at the done word after every decode step; libwlx_ab.so reads WLX_MT_STEP_BLOCK for another block length, so

    WLX_LIB=whisperlive_amd/libwlx_ab.so WLX_MT_STEP_BLOCK=8 python scripts/file_translate_time.py

measures another one (one value per process)."""
from __future__ import annotations

import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from whisperlive_amd.mt_weights import SMALL100, MTGenOptions, random_mt_weights  # noqa: E402
from whisperlive_amd.translation import HipMTEngine, HipTranslator  # noqa: E402


def mt_engine(long: bool, max_batch: int):
    spec = dataclasses.replace(SMALL100, decoder_start_id=0)
    eng = HipMTEngine(spec, random_mt_weights(spec, seed=3, peaked=not long), device=0, max_batch=max_batch, max_rows=5, max_src=256)
    o = MTGenOptions(num_beams=5, max_length=32 if long else 200, early_stopping=True, length_penalty=1.0)
    return eng, o


def header(a):
    return (f"# lib={os.environ.get('WLX_LIB', 'libwlx.so')} step_block={os.environ.get('WLX_MT_STEP_BLOCK', '1 (compiled in)')} "
            f"weights={'unpeaked, max_length 32' if a.long else 'peaked, max_length 200'} max_batch={a.max_batch} beams=5 pairs={a.pairs}")


def sizes(a):
    eng, o = mt_engine(a.long, a.max_batch)
    print(header(a))
    print("# n  src_tokens  loop_ms  many_ms  many/loop  ratio_spread  loop_steps  many_steps  same_tokens")
    for L in [int(x) for x in a.lengths.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            rng = np.random.default_rng(1000 * L + n)
            srcs = [[128010] + [int(x) for x in rng.integers(4, 128000, size=L - 2)] + [2] for _ in range(n)]

            def loop():
                out, steps = [], 0
                for k in range(0, n, a.max_batch):
                    t, _ = eng.translate_ids(srcs[k:k + a.max_batch], o)
                    out += t
                    steps += eng.timings()[2]
                return out, steps

            def many():
                t, _ = eng.translate_ids_many(srcs, o)
                return t, eng.timings()[2]
            loop(), many()                                   # warm-up: first launches, the search state's allocation
            tl, tm, ratios = [], [], []
            for p in range(a.pairs):
                legs = (loop, many) if p % 2 == 0 else (many, loop)
                got = {}
                for leg in legs:
                    t0 = time.perf_counter()
                    got[leg.__name__] = leg()
                    got[leg.__name__ + "_ms"] = (time.perf_counter() - t0) * 1e3
                tl.append(got["loop_ms"])
                tm.append(got["many_ms"])
                ratios.append(got["many_ms"] / got["loop_ms"])
            same = sum(x == y for x, y in zip(got["loop"][0], got["many"][0]))
            print(f"{n:4d} {L:4d}  {statistics.median(tl):9.2f} {statistics.median(tm):9.2f}  {statistics.median(ratios):6.3f}  "
                  f"{min(ratios):.3f}..{max(ratios):.3f}  {got['loop'][1]:6d} {got['many'][1]:6d}  {same}/{n}", flush=True)
    eng.close()


def end_to_end(a):
    from oracle.logmel import speech_like_pcm
    from whisperlive_amd import engine as E, vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.mt_tokenizer import M2M100SPTokenizer
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights
    audio = np.concatenate([speech_like_pcm(60.0, seed=200 + i) for i in range(10)]).astype(np.float32)
    mt, o = mt_engine(True, a.max_batch)
    tr = HipTranslator(None, engine=mt, tokenizer=M2M100SPTokenizer(os.path.join(ROOT, "tests", "golden", "mt_tok")), options=o)
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    spec = SPECS["small.en"]
    eng = E.HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    hip = WhisperModelHIP("small.en", engine=eng, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=12, vad_model=gate)
    pipe = BatchedInferencePipeline(hip)
    kw = dict(language="en", temperature=0.0, beam_size=5, max_new_tokens=32, without_timestamps=True, vad_filter=True,
              suppress_tokens=[-1, hip._base_tokenizer.eot], batch_size=12)

    def plain():
        segs, _ = pipe.transcribe(audio, **kw)
        return list(segs)

    def translated():
        segs, _ = pipe.transcribe(audio, target_language="de", translator=tr, **kw)
        return segs
    try:
        plain(), translated()
        tp, tt = [], []
        for p in range(a.pairs):
            for leg in ((plain, translated) if p % 2 == 0 else (translated, plain)):
                t0 = time.perf_counter()
                segs = leg()
                (tp if leg is plain else tt).append((time.perf_counter() - t0) * 1e3)
        n_tr = sum(1 for s in translated() if s.text.strip())
        steps = mt.timings()[2]
        mp, mt_ms = statistics.median(tp), statistics.median(tt)
        print(header(a))
        print(f"end to end, one {len(audio) / 16000:.0f} s file, small.en batch 12 beam 5, {len(segs)} segments ({n_tr} translated, "
              f"{steps} MT decode steps in {-(-n_tr // a.max_batch)} groups): without target_language {mp:.1f} ms "
              f"({' '.join(f'{x:.1f}' for x in tp)}), with {mt_ms:.1f} ms ({' '.join(f'{x:.1f}' for x in tt)}), "
              f"translation adds {mt_ms - mp:.1f} ms = {100 * (mt_ms - mp) / mp:.1f} %", flush=True)
    finally:
        hip.close()
        eng.close()
        gate.close()
        mt.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--sizes", default="8,64,256")
    ap.add_argument("--lengths", default="16,64")
    ap.add_argument("--max_batch", type=int, default=8)
    ap.add_argument("--long", action="store_true", help="unpeaked weights, max_length 32: 31 decode steps per group")
    ap.add_argument("--end_to_end", action="store_true", help="a 10-minute file with and without target_language")
    a = ap.parse_args(argv)
    if a.end_to_end:
        a.long = True
        return end_to_end(a)
    sizes(a)


if __name__ == "__main__":
    main()
