"""What a grammar per item costs a decode step, by the method of scripts/keyword_bias_items_time.py: Whisper-small.en
widths, one stream, beam 5, random weights; a step's time is the HIP-event time of a whole generate divided by its decode steps, the
median of --reps generates after --warmup. The grammar is scripts/grammar_time.py's: --phrases phrases of one to three tokens.

  1. The step at 5 rows (1 item) and at 48 items x 5 rows, per process: no table, ONE grammar (wlx_grammar_set), and the pool
     (wlx_grammar_set_items) with every item selected and — at 48 items — with ONE item selected and with none.
  2. Against the parent commit's library (--parent-lib PATH), alternating fresh processes parent / this build / parent: the unconstrained
     and the single-grammar step run unchanged code, so their ratio this / parent must lie inside the spread the parent shows against
     itself (its two legs of the same pair); the per-item launch is compared with the PARENT's single-grammar step.
  3. The job (--job-files, default 48; 0 skips it): scripts/many_files_time.py's archive with a phrase list PER FILE (all different):
     ONE transcribe_many(files, grammars=lists) job against a loop of transcribe(file) under the file's grammar, wall time, alternating.

    python scripts/grammar_items_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 3] > profiles/grammar_items_time.txt
"""
import argparse
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
        _lib.EXPORTS_GRAMMAR_ITEMS = []         # the parent commit's library has no per-item entry points: its legs never call them
    from oracle import logmel as olm
    from whisperlive_amd import grammar
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    spec = SPECS[args.model]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    tb = spec.vocab - 1501
    ids = TokenIds(tb - 106, tb - 107, tb - 1, tb, tb - 2, 220)
    rng = np.random.default_rng(5)
    phrases = [[int(x) for x in rng.integers(300, 20000, size=int(rng.integers(1, 4)))] for _ in range(args.phrases)]
    g = grammar.compile_grammar(None, phrases, vocab=spec.vocab, eot=ids.eot)
    kw = dict(beam_size=5, patience=1.0, max_length=1 + args.tokens, suppress_tokens=[1, 2, 7, ids.sot, ids.eot])     # (no end of text: every call runs its budget)
    res = {"table": dict(states=g.n_states, edges=g.n_edges)}
    for items in (1, 48):
        slot = eng.create_slot(items, 5)
        T = [slot.logmel(olm.speech_like_pcm(5.0, seed=1234 + i), item=i) for i in range(items)]
        slot.encode(items, seek=[0] * items, seg=[t - 1 for t in T])

        def measure():
            out = []
            for i in range(args.warmup + args.reps):
                slot.generate([[ids.sot]] * items, ids, **kw)
                t = slot.timings()
                if i >= args.warmup:
                    out.append(1000.0 * t["generate_ms"] / max(1, t["decode_steps"]))
            return statistics.median(out)

        r = {"off": measure()}
        slot.set_grammar(g)
        r["single"] = measure()
        if not args.parent:
            slot.set_grammars(grammar.GrammarSet([g]))
            slot.select_grammars([0] * items)
            r["pool_all"] = measure()
            if items > 1:
                slot.select_grammars([0] + [-1] * (items - 1))
                r["pool_one"] = measure()
                slot.select_grammars([-1] * items)
                r["pool_none"] = measure()
        slot.clear_grammar()
        r["off_again"] = measure()
        res[str(items)] = r
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
              suppress_tokens=[hip._base_tokenizer.eot], suppress_blank=False, batch_size=batch)

    def loop():
        t0 = time.perf_counter()
        out = []
        for f, phrases in zip(files, lists):
            with hip.grammar(phrases=phrases):
                out.append(list(pipe.transcribe(f, **kw)[0]))
        return time.perf_counter() - t0, out

    def job():
        t0 = time.perf_counter()
        out = pipe.transcribe_many(files, grammars=lists, **kw)
        return time.perf_counter() - t0, [s for s, _ in out]

    _, want = loop()
    _, got = job()
    same = all([x.tokens for x in a] == [x.tokens for x in b] for a, b in zip(got, want))
    tl, tj = [], []
    for _ in range(args.pairs):
        tl.append(loop()[0])
        tj.append(job()[0])
    hip.close()
    eng.close()
    gate.close()
    print("RESULT " + json.dumps(dict(loop_s=tl, job_s=tj, same=same, waves=pipe.many_timing["waves"])))


def run(args, mode, lib=None):
    env = dict(os.environ)
    env.pop("WLX_LIB", None)
    if lib:
        env["WLX_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--model", args.model, "--tokens", str(args.tokens), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--phrases", str(args.phrases), "--pairs", str(args.pairs), "--job-files", str(args.job_files),
           "--job-phrases", str(args.job_phrases)] + (["--parent"] if lib else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--job-child", action="store_true")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="small.en")
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--phrases", type=int, default=200)
    ap.add_argument("--job-files", type=int, default=48)
    ap.add_argument("--job-phrases", type=int, default=5)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.job_child:
        return job_child(args)
    med = statistics.median
    print(f"grammar_items_time: {args.model}, 1 stream, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after "
          f"{args.warmup}; step = HIP-event time of a generate / its decode steps, us", flush=True)
    runs = []
    for k in range(args.pairs):
        a1 = run(args, "--child", args.parent_lib) if args.parent_lib else None
        b = run(args, "--child")
        a2 = run(args, "--child", args.parent_lib) if args.parent_lib else None
        runs.append((a1, b, a2))
        for items in ("1", "48"):
            r = b[items]
            line = f"{int(items) * 5:4d} rows, pair {k}: this build off {r['off']:8.2f}  single {r['single']:8.2f}  pool, all selected {r['pool_all']:8.2f}"
            if "pool_one" in r:
                line += f"  one of 48 {r['pool_one']:8.2f}  none {r['pool_none']:8.2f}"
            line += f"  off again {r['off_again']:8.2f}"
            if a1 is not None:
                line += f"  | parent off {a1[items]['off']:8.2f} {a2[items]['off']:8.2f}  single {a1[items]['single']:8.2f} {a2[items]['single']:8.2f}"
            print(line, flush=True)
    print(f"table: {runs[0][1]['table']}")
    for items in ("1", "48"):
        rows = int(items) * 5
        d = lambda x, y: med([b[items][x] - b[items][y] for _, b, _ in runs])
        print(f"{rows:4d} rows, same process, median of pairs: single - off {d('single', 'off'):+.2f} us, pool (all selected) - off {d('pool_all', 'off'):+.2f} us, "
              f"pool - single {d('pool_all', 'single'):+.2f} us" + (f", one of 48 - off {d('pool_one', 'off'):+.2f} us, none selected - off {d('pool_none', 'off'):+.2f} us"
                                                                     if items == "48" else ""))
        if args.parent_lib:
            parent = lambda a1, a2, x: 0.5 * (a1[items][x] + a2[items][x])
            for name in ("off", "single"):
                ratio = [b[items][name] / parent(a1, a2, name) for a1, b, a2 in runs]
                spread = max(abs(a2[items][name] / a1[items][name] - 1.0) for a1, _, a2 in runs)
                r = med(ratio)
                print(f"{rows:4d} rows, {name}: this build / parent, median ratio {r:.4f} over {len(ratio)} alternating pairs (min {min(ratio):.4f}, max {max(ratio):.4f}); "
                      f"the parent against itself in those pairs: up to {100.0 * spread:.2f} %; inside it: {'yes' if abs(r - 1.0) <= spread else 'NO'}")
            new = [b[items]["pool_all"] for _, b, _ in runs]
            old = [parent(a1, a2, "single") for a1, _, a2 in runs]
            print(f"{rows:4d} rows, the per-item step {med(new):.2f} us against the parent's single-grammar step {med(old):.2f} us: "
                  f"{med(new) - med(old):+.2f} us ({100.0 * (med(new) / med(old) - 1.0):+.2f} %)")
    if args.job_files > 0:
        res = run(args, "--job-child")
        fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        ml, mj = med(res["loop_s"]), med(res["job_s"])
        print(f"\nthe job: {args.job_files} files of 20 s, a grammar per file ({args.job_phrases} three-token phrases each, all different), batch_size 12, "
              f"{args.model}, wall seconds, {args.pairs} alternating pairs after one warm-up of each leg; {res['waves']} wave(s); tokens of the two "
              f"legs equal file by file: {res['same']}")
        print(f"    loop of transcribe under the file's grammar: {fmt(res['loop_s'])}   p50 {ml:.4f}")
        print(f"    transcribe_many(grammars=...) job:           {fmt(res['job_s'])}   p50 {mj:.4f}")
        print(f"    job / loop = {mj / ml:.3f} (loop / job = {ml / mj:.2f} x)")


if __name__ == "__main__":
    main()
