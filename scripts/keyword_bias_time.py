"""What keyword boosting costs a decode step, on the benchmark's decode shape: Whisper-small.en widths, one stream, beam 5,
64 generated tokens per window, random weights (the step's launches do not depend on the values).

  1. bias OFF in this build against the parent commit's library (--parent-lib PATH, a libwlx.so built from the parent): the unbiased
     step's launch list is unchanged, so the two must agree within the box-to-box spread the project records (+-1.5 %). Alternating
     pairs of fresh processes (A B A B ...), the statistic is the median over the pairs of the per-pair ratio.
  2. bias ON against bias OFF in the same process of this build: the one dependent launch per step the table adds.

Every leg is its own child process (one GPU context at a time); a step's time is the HIP-event time of a whole generate divided by its
decode steps, the median of --reps generates after --warmup.

    python scripts/keyword_bias_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 5] [--reps 30] > profiles/keyword_bias_time.txt
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
    if args.old_abi:
        # a library from before wlx_bias_*: the binding's table asks for them, so they are stubbed for THIS process only (never called)
        class Stub:
            argtypes = restype = None

        class OldLib(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if "bias" in name:
                        return Stub()
                    raise
        _lib.C.CDLL = OldLib
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

    def measure():
        out = []
        for i in range(args.warmup + args.reps):
            slot.generate([[ids.sot]], ids, **kw)
            t = slot.timings()
            if i >= args.warmup:
                out.append(1000.0 * t["generate_ms"] / max(1, t["decode_steps"]))
        return out

    res = {"off_us": measure()}
    if not args.old_abi:
        rng = np.random.default_rng(5)
        phrases = [[int(x) for x in rng.integers(300, 20000, size=3)] for _ in range(args.phrases)]
        table = biasing.compile_bias(phrases, 2.0, {int(t): 0.5 for t in rng.choice(20000, size=16, replace=False)}, vocab=spec.vocab, eot=ids.eot)
        slot.set_bias(table)
        res["on_us"] = measure()
        slot.clear_bias()
        res["off_again_us"] = measure()
        res["table"] = dict(nodes=table.n_nodes, edges=table.n_edges, tokens=int(table.tok_ids.size))
    slot.close()
    eng.close()
    print("RESULT " + json.dumps(res))


def run_child(args, lib, old_abi):
    env = dict(os.environ)
    if lib:
        env["WLX_LIB"] = lib
    else:
        env.pop("WLX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--model", args.model, "--tokens", str(args.tokens), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--phrases", str(args.phrases)] + (["--old-abi"] if old_abi else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", default="small.en")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phrases", type=int, default=50)
    args = ap.parse_args()
    if args.child:
        return child(args)
    med = statistics.median
    print(f"keyword_bias_time: {args.model}, 1 stream, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after {args.warmup}; "
          f"step = HIP-event time of a generate / its decode steps, us")
    new_legs, ratios = [], []
    for k in range(args.pairs):
        a = run_child(args, args.parent_lib, True) if args.parent_lib else None
        b = run_child(args, None, False)
        new_legs.append(b)
        line = f"pair {k}: this build off {med(b['off_us']):8.2f}  on {med(b['on_us']):8.2f}  off again {med(b['off_again_us']):8.2f}"
        if a is not None:
            ratios.append(med(b["off_us"]) / med(a["off_us"]))
            line += f"  | parent off {med(a['off_us']):8.2f}  ratio this/parent {ratios[-1]:.4f}"
        print(line, flush=True)
    off = med([med(b["off_us"]) for b in new_legs])
    on = med([med(b["on_us"]) for b in new_legs])
    deltas = [med(b["on_us"]) - med([med(b["off_us"]), med(b["off_again_us"])]) for b in new_legs]
    print(f"table: {new_legs[0]['table']}")
    print(f"bias on - off, same process: median of pairs {med(deltas):+.2f} us per step (min {min(deltas):+.2f}, max {max(deltas):+.2f}); "
          f"off {off:.2f} us, on {on:.2f} us ({100.0 * (on / off - 1.0):+.2f} %)")
    if ratios:
        r = med(ratios)
        print(f"bias off, this build / parent: median ratio {r:.4f} over {len(ratios)} alternating pairs (min {min(ratios):.4f}, max {max(ratios):.4f}); "
              f"within +-1.5 %: {'yes' if abs(r - 1.0) <= 0.015 else 'NO'}")


if __name__ == "__main__":
    main()
