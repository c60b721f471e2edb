"""What grammar-constrained decoding costs a decode step, on the benchmark's decode shape: Whisper-small.en widths, beam 5,
random weights (the step's launches do not depend on the values), at 5 decoder rows (one stream) and at 240 (48 windows in one group).

  1. grammar OFF in this build against the parent commit's library (--parent-lib PATH, a libwlx.so built from the parent): the step of a
     slot without a grammar keeps its launch list, so the two must agree within the run-to-run spread of the parent measured in the same
     session. Alternating pairs of fresh processes (A B A B ...); the statistic is the median over the pairs of the per-pair ratio, the
     spread is that of the parent's own legs (max / min of their medians).
  2. grammar ON against OFF in the same process of this build: the one dependent launch per step the grammar adds.
  3. the kernel's bytes: it stores at most (eot + 1) * 4 bytes per row (less the allowed pieces) and reads only the pieces that mix allowed
     and masked ids; the time those bytes take at the HBM rate of the micro-architecture guide (6.3 TB/s achievable) is printed next to
     the on - off difference, which is the kernel's device time PLUS the gap its dependent launch adds to the step: an upper bound of the
     kernel's own time. A kernel trace of its own is not part of this script.

Every leg is its own child process (one GPU context at a time); a step's time is the HIP-event time of a whole generate divided by its
decode steps, the median of --reps generates after --warmup.

    python scripts/grammar_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 3] [--reps 20] > profiles/grammar_time.txt
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
HBM_BYTES_PER_S = 6.3e12


def child(args):
    import numpy as np
    from whisperlive_amd import _lib
    if args.old_abi:
        # a library from before wlx_grammar_*: the binding's table asks for them, so they are stubbed for THIS process only (never called)
        class Stub:
            argtypes = restype = None

        class OldLib(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if "grammar" in name:
                        return Stub()
                    raise
        _lib.C.CDLL = OldLib
        _lib.EXPORTS_GRAMMAR = []
    from oracle import logmel as olm
    from whisperlive_amd import grammar
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    spec = SPECS[args.model]
    items = max(1, args.rows // 5)
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = eng.create_slot(items, 5)
    tb = spec.vocab - 1501
    ids = TokenIds(tb - 106, tb - 107, tb - 1, tb, tb - 2, 220)
    pcm = olm.speech_like_pcm(30.0, seed=1234)
    T = [slot.logmel(pcm, item=b) for b in range(items)]
    slot.encode(items, seek=[0] * items, seg=[min(t - 1, 3000) for t in T])
    kw = dict(beam_size=5, patience=1.0, max_length=1 + args.tokens, suppress_tokens=[1, 2, 7, ids.sot, ids.eot])     # (no end of text: every call runs its budget)

    def measure():
        out = []
        for i in range(args.warmup + args.reps):
            slot.generate([[ids.sot]] * items, ids, **kw)
            t = slot.timings()
            if i >= args.warmup:
                out.append(1000.0 * t["generate_ms"] / max(1, t["decode_steps"]))
        return out

    res = {"rows": items * 5, "off_us": measure()}
    if not args.old_abi:
        rng = np.random.default_rng(5)
        # an IVR-sized list: --phrases phrases of one to three tokens over a few hundred distinct first tokens
        phrases = [[int(x) for x in rng.integers(300, 20000, size=int(rng.integers(1, 4)))] for _ in range(args.phrases)]
        g = grammar.compile_grammar(None, phrases, vocab=spec.vocab, eot=ids.eot)
        slot.set_grammar(g)
        res["on_us"] = measure()
        slot.clear_grammar()
        res["off_again_us"] = measure()
        res["table"] = dict(states=g.n_states, edges=g.n_edges, start_edges=int(g.edge_off[1]))
        res["bytes_per_launch"] = items * 5 * (ids.eot + 1) * 4
    slot.close()
    eng.close()
    print("RESULT " + json.dumps(res))


def child_cmd(args, rows, old_abi):
    return [sys.executable, os.path.abspath(__file__), "--child", "--model", args.model, "--tokens", str(args.tokens), "--reps", str(args.reps),
            "--warmup", str(args.warmup), "--phrases", str(args.phrases), "--rows", str(rows)] + (["--old-abi"] if old_abi else [])


def run_child(args, rows, lib, old_abi):
    env = dict(os.environ)
    if lib:
        env["WLX_LIB"] = lib
    else:
        env.pop("WLX_LIB", None)
    p = subprocess.run(child_cmd(args, rows, old_abi), env=env, capture_output=True, text=True, timeout=600)
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
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--row-counts", default="5,240")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--phrases", type=int, default=200)
    args = ap.parse_args()
    if args.child:
        return child(args)
    med = statistics.median
    print(f"grammar_time: {args.model}, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after {args.warmup}; "
          f"step = HIP-event time of a generate / its decode steps, us")
    for rows in [int(x) for x in args.row_counts.split(",")]:
        new_legs, old_legs, ratios = [], [], []
        for k in range(args.pairs):
            a = run_child(args, rows, args.parent_lib, True) if args.parent_lib else None
            b = run_child(args, rows, None, False)
            new_legs.append(b)
            line = f"{rows:3d} rows, pair {k}: this build off {med(b['off_us']):8.2f}  on {med(b['on_us']):8.2f}  off again {med(b['off_again_us']):8.2f}"
            if a is not None:
                old_legs.append(med(a["off_us"]))
                ratios.append(med(b["off_us"]) / med(a["off_us"]))
                line += f"  | parent off {med(a['off_us']):8.2f}  ratio this/parent {ratios[-1]:.4f}"
            print(line, flush=True)
        off = med([med(b["off_us"]) for b in new_legs])
        on = med([med(b["on_us"]) for b in new_legs])
        deltas = [med(b["on_us"]) - med([med(b["off_us"]), med(b["off_again_us"])]) for b in new_legs]
        bytes_ = new_legs[0]["bytes_per_launch"]
        print(f"{rows:3d} rows: table {new_legs[0]['table']}")
        print(f"{rows:3d} rows: grammar on - off, same process: median of pairs {med(deltas):+.2f} us per step (min {min(deltas):+.2f}, max {max(deltas):+.2f}); "
              f"off {off:.2f} us, on {on:.2f} us ({100.0 * (on / off - 1.0):+.2f} %)")
        print(f"{rows:3d} rows: the launch stores at most {bytes_} bytes: {1e6 * bytes_ / HBM_BYTES_PER_S:.2f} us at {HBM_BYTES_PER_S / 1e12:.1f} TB/s")
        if ratios:
            spread = max(old_legs) / min(old_legs) - 1.0
            r = med(ratios)
            print(f"{rows:3d} rows: grammar off, this build / parent: median ratio {r:.4f} over {len(ratios)} alternating pairs (min {min(ratios):.4f}, "
                  f"max {max(ratios):.4f}); run-to-run spread of the parent's legs in this session {100.0 * spread:.2f} %; inside it: "
                  f"{'yes' if abs(r - 1.0) <= max(spread, 1e-9) else 'NO'}")


if __name__ == "__main__":
    main()
