"""What per-item keyword boosting costs a decode step, by the method of scripts/keyword_bias_time.py: Whisper-small.en
widths, one stream, beam 5, 64 generated tokens per window, random weights; a step's time is the HIP-event time of a whole generate
divided by its decode steps, the median of --reps generates after --warmup. The table is §25's: 50 three-token phrases and 16
logit_bias entries.

  1. Nothing leaked: the unbiased step, and the single-table step (wlx_bias_set), of this build against the parent commit's library
     (--parent-lib PATH). Alternating pairs of fresh processes; the statistic is the median over the pairs of the per-pair ratio, which
     must lie inside the +-1.5 % box-to-box spread.
  2. Per item against single table, same build, same process, alternating: the table as a one-table set selected for the item
     (wlx_bias_set_items + wlx_bias_select) against wlx_bias_set of its closed form, us per step for both.
  3. The job (--job-files, default 48; 0 skips it): scripts/many_files_time.py's archive (files of 20 s, G.711 WAV and FLAC alternating,
     batch_size 12, beam 5, the gate on, 32 forced tokens per chunk, small.en widths) with a keyword list PER FILE (--job-phrases
     three-token phrases each, all lists different): ONE transcribe_many(files, keywords=lists) job against a loop of
     transcribe(file) under keyword_bias of the file's list, wall time, alternating pairs after one warm-up of each leg; and the same two
     legs without keywords, in the same process, for scale (profiles/many_files_time.txt has that pair on its own).

    python scripts/keyword_bias_items_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 5] > profiles/keyword_bias_items_time.txt
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    from whisperlive_amd import _lib
    if args.parent:
        # the parent commit's library lacks the three per-item entry points the binding's table asks for: this child's binding drops them
        # from its list and takes stubs for exactly those names (never called), through a loader of its own — ctypes itself is untouched
        class Stub:
            argtypes = restype = None

        class ParentLib(ctypes.CDLL):
            def __getattr__(self, name):
                if name in missing:
                    return Stub()
                return super().__getattr__(name)
        missing = tuple(_lib.EXPORTS_BIAS_ITEMS)
        _lib.EXPORTS_BIAS_ITEMS = []

        class Loader:                                    # stands in for the `ctypes` name inside _lib only
            def __getattr__(self, name):
                return ParentLib if name == "CDLL" else getattr(ctypes, name)
        _lib.C = Loader()
    from oracle import logmel as olm
    from whisperlive_amd import biasing
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    spec = SPECS[args.model]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = eng.create_slot(1, 5)
    tb = spec.vocab - 1501
    ids = TokenIds(tb - 106, tb - 107, tb - 1, tb, tb - 2, 220)
    T = slot.logmel(olm.speech_like_pcm(30.0, seed=1234))
    slot.encode(1, seek=[0], seg=[min(T - 1, 3000)])
    kw = dict(beam_size=5, patience=1.0, max_length=1 + args.tokens, suppress_tokens=[1, 2, 7, ids.sot, ids.eot])     # (no end of text: every call runs its budget)

    def measure(reps):
        out = []
        for i in range(args.warmup + reps):
            slot.generate([[ids.sot]], ids, **kw)
            t = slot.timings()
            if i >= args.warmup:
                out.append(1000.0 * t["generate_ms"] / max(1, t["decode_steps"]))
        return out

    rng = np.random.default_rng(5)
    phrases = [[int(x) for x in rng.integers(300, 20000, size=3)] for _ in range(args.phrases)]
    lb = {int(t): 0.5 for t in rng.choice(20000, size=16, replace=False)}
    closed = biasing.compile_bias(phrases, 2.0, lb, vocab=spec.vocab, eot=ids.eot)
    res = {"off_us": measure(args.reps)}
    slot.set_bias(closed)
    res["single_us"] = measure(args.reps)
    if not args.parent:
        compact = biasing.compile_compact(phrases, 2.0, lb, vocab=spec.vocab, eot=ids.eot)
        one = biasing.BiasSet([compact])
        single, items = [], []
        for _ in range(args.rounds):                     # alternating, same process
            slot.set_bias(closed)
            single += measure(max(1, args.reps // args.rounds))
            slot.set_bias_items(one)
            slot.select_bias([0])
            items += measure(max(1, args.reps // args.rounds))
        res.update(alt_single_us=single, alt_items_us=items,
                   table=dict(nodes=closed.n_nodes, closed_edges=closed.n_edges, compact_edges=compact.n_edges, tokens=int(closed.tok_ids.size)))
    slot.clear_bias()
    slot.close()
    eng.close()
    print("RESULT " + json.dumps(res))


def job_child(args):
    import time

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from many_files_time import make_files
    from whisperlive_amd import engine as E, vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights
    n, batch = args.job_files, 12
    files = make_files(n, 20.0)
    rng = np.random.default_rng(11)
    lists = [[[int(x) for x in rng.integers(300, 20000, size=3)] for _ in range(args.job_phrases)] for _ in range(n)]
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    spec = SPECS[args.model]
    eng = E.HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    hip = WhisperModelHIP(args.model, engine=eng, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=batch + n, vad_model=gate)
    pipe = BatchedInferencePipeline(hip)
    kw = dict(language="en", temperature=0.0, beam_size=5, max_new_tokens=32, without_timestamps=True, vad_filter=True,
              suppress_tokens=[-1, hip._base_tokenizer.eot], batch_size=batch)

    def loop(keyed):
        t0 = time.perf_counter()
        out = []
        for f, kws in zip(files, lists):
            if keyed:
                with hip.keyword_bias(phrases=kws, boost=2.0):
                    out.append(list(pipe.transcribe(f, **kw)[0]))
            else:
                out.append(list(pipe.transcribe(f, **kw)[0]))
        return time.perf_counter() - t0, out

    def job(keyed):
        t0 = time.perf_counter()
        out = pipe.transcribe_many(files, **kw, **(dict(keywords=lists, keywords_boost=2.0) if keyed else {}))
        return time.perf_counter() - t0, [s for s, _ in out]

    res = {}
    for keyed in (True, False):
        _, want = loop(keyed)
        _, got = job(keyed)
        same = all([x.tokens for x in g] == [x.tokens for x in w] for g, w in zip(got, want))
        tl, tj = [], []
        for _ in range(args.pairs):
            tl.append(loop(keyed)[0])
            tj.append(job(keyed)[0])
        res["keyed" if keyed else "plain"] = dict(loop_s=tl, job_s=tj, same=same, waves=pipe.many_timing["waves"])
    hip.close()
    eng.close()
    gate.close()
    print("RESULT " + json.dumps(res))


def run_child(args, lib):
    env = dict(os.environ)
    if lib:
        env["WLX_LIB"] = lib
    else:
        env.pop("WLX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--model", args.model, "--tokens", str(args.tokens), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--phrases", str(args.phrases), "--rounds", str(args.rounds)] + (["--parent"] if lib else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="small.en")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phrases", type=int, default=50)
    ap.add_argument("--job-child", action="store_true")
    ap.add_argument("--job-files", type=int, default=48)
    ap.add_argument("--job-phrases", type=int, default=5)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.job_child:
        return job_child(args)
    med = statistics.median
    print(f"keyword_bias_items_time: {args.model}, 1 stream, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after "
          f"{args.warmup}; step = HIP-event time of a generate / its decode steps, us", flush=True)
    legs, r_off, r_single = [], [], []
    for k in range(args.pairs):
        a = run_child(args, args.parent_lib) if args.parent_lib else None
        b = run_child(args, None)
        legs.append(b)
        line = (f"pair {k}: this build off {med(b['off_us']):8.2f}  single {med(b['single_us']):8.2f}  | alternating single "
                f"{med(b['alt_single_us']):8.2f}  per-item {med(b['alt_items_us']):8.2f}")
        if a is not None:
            r_off.append(med(b["off_us"]) / med(a["off_us"]))
            r_single.append(med(b["single_us"]) / med(a["single_us"]))
            line += f"  | parent off {med(a['off_us']):8.2f} single {med(a['single_us']):8.2f}  ratios {r_off[-1]:.4f} {r_single[-1]:.4f}"
        print(line, flush=True)
    print(f"table: {legs[0]['table']}")
    single = med([med(b["alt_single_us"]) for b in legs])
    items = med([med(b["alt_items_us"]) for b in legs])
    deltas = [med(b["alt_items_us"]) - med(b["alt_single_us"]) for b in legs]
    print(f"per-item - single table, same process: median of pairs {med(deltas):+.2f} us per step (min {min(deltas):+.2f}, max {max(deltas):+.2f}); "
          f"single {single:.2f} us, per-item {items:.2f} us ({100.0 * (items / single - 1.0):+.2f} %)")
    for name, rs in (("bias off", r_off), ("single table", r_single)):
        if rs:
            r = med(rs)
            print(f"{name}, this build / parent: median ratio {r:.4f} over {len(rs)} alternating pairs (min {min(rs):.4f}, max {max(rs):.4f}); "
                  f"within +-1.5 %: {'yes' if abs(r - 1.0) <= 0.015 else 'NO'}")
    if args.job_files > 0:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--job-child", "--model", args.model, "--pairs", str(args.pairs),
                            "--job-files", str(args.job_files), "--job-phrases", str(args.job_phrases)], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"job child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        res = json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        print(f"\nthe job: {args.job_files} files of 20 s, batch_size 12, {args.model}, wall seconds, {args.pairs} alternating pairs after one warm-up of each leg")
        for name, what in (("keyed", f"a keyword list per file ({args.job_phrases} three-token phrases each, all different)"), ("plain", "no keywords")):
            r = res[name]
            ml, mj = med(r["loop_s"]), med(r["job_s"])
            print(f"  {what}: {r['waves']} wave(s); tokens of the two legs equal file by file: {r['same']}")
            print(f"    loop of transcribe:  {fmt(r['loop_s'])}   p50 {ml:.4f}")
            print(f"    transcribe_many job: {fmt(r['job_s'])}   p50 {mj:.4f}")
            print(f"    job / loop = {mj / ml:.3f} (loop / job = {ml / mj:.2f} x)")


if __name__ == "__main__":
    main()
