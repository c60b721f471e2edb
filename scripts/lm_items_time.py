"""What a language model per item costs a decode step, on the decode shape of scripts/lm_time.py: Whisper-small.en widths,
beam 5, random weights, at 5 decoder rows (one stream) and at 240 (48 windows in one group).

  1. this build against the parent commit's library (--parent-lib PATH, a libwlx.so built from the parent), in alternating pairs of
     fresh processes (A B A B ...): a slot without a model, and a slot under wlx_lm_set (the trigram model of lm_time.py). Both keep
     their launch lists, so each ratio must lie within the run-to-run spread of the parent's own legs in the same session. The
     statistic is the median over the pairs of the per-pair ratio.
  2. in the same process of this build: the single-model launch (wlx_lm_set), the per-item launch with every item selected
     (wlx_lm_set_items, one entry per item: two models at alternating weights) and with none selected, each ON minus OFF. The
     difference is the kernel's device time plus the gap its dependent launch adds to the step.

Every leg is its own child process (one GPU context at a time); a step's time is the HIP-event time of a whole generate divided by its
decode steps, the median of --reps generates after --warmup.

    python scripts/lm_items_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 3] [--reps 20] > profiles/lm_items_time.txt
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
    from whisperlive_amd import _lib
    if args.old_abi:
        _lib.EXPORTS_LM_ITEMS = []              # a library from before wlx_lm_set_items: its legs never call it
    from oracle import logmel as olm
    from scripts.lm_time import synthetic_lm
    from whisperlive_amd import lm
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

    a, b = synthetic_lm(spec.vocab, ids.eot, 400, 1600, 50), synthetic_lm(spec.vocab, ids.eot, 300, 900, 80, seed=6)
    res = {"rows": items * 5, "off_us": measure()}
    slot.set_lm(a, 0.3)
    res["single_us"] = measure()
    slot.clear_lm()
    if not args.old_abi:
        lset = lm.LmSet()
        sel = [lset.add((a, b)[k % 2], 0.2 + 0.1 * (k % 3)) for k in range(items)]
        slot.set_lms(lset)
        slot.select_lms(sel)
        res["items_all_us"] = measure()
        slot.select_lms([-1] * items)
        res["items_none_us"] = measure()
        slot.clear_lm()
        res["entries"] = len(lset)
    res["off_again_us"] = measure()
    slot.close()
    eng.close()
    print("RESULT " + json.dumps(res))


def run_child(args, rows, lib, old_abi):
    env = dict(os.environ)
    if lib:
        env["WLX_LIB"] = lib
    else:
        env.pop("WLX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--model", args.model, "--tokens", str(args.tokens), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--rows", str(rows)] + (["--old-abi"] if old_abi else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
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
    args = ap.parse_args()
    if args.child:
        return child(args)
    med = statistics.median
    print(f"lm_items_time: {args.model}, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after {args.warmup}; "
          f"step = HIP-event time of a generate / its decode steps, us")
    for rows in [int(x) for x in args.row_counts.split(",")]:
        new_legs, old_legs = [], []
        for k in range(args.pairs):
            a = run_child(args, rows, args.parent_lib, True) if args.parent_lib else None
            b = run_child(args, rows, None, False)
            new_legs.append(b)
            line = (f"{rows:3d} rows, pair {k}: this build off {med(b['off_us']):8.2f}  single {med(b['single_us']):8.2f}  items, all selected "
                    f"{med(b['items_all_us']):8.2f}  items, none selected {med(b['items_none_us']):8.2f}  off again {med(b['off_again_us']):8.2f}")
            if a is not None:
                old_legs.append(a)
                line += f"  | parent off {med(a['off_us']):8.2f}  single {med(a['single_us']):8.2f}"
            print(line, flush=True)
        off = lambda leg: med([med(leg["off_us"]), med(leg["off_again_us"])])
        for name in ("single", "items_all", "items_none"):
            ds = [med(b[f"{name}_us"]) - off(b) for b in new_legs]
            print(f"{rows:3d} rows: {name} on - off, same process ({new_legs[0]['entries']} entries): median of pairs {med(ds):+.2f} us per step "
                  f"(min {min(ds):+.2f}, max {max(ds):+.2f})")
        for name in ("off", "single") if old_legs else ():
            ratios = [med(b[f"{name}_us"]) / med(a[f"{name}_us"]) for a, b in zip(old_legs, new_legs)]
            olds = [med(a[f"{name}_us"]) for a in old_legs]
            spread, r = max(olds) / min(olds) - 1.0, med(ratios)
            print(f"{rows:3d} rows: {name}, this build / parent: median ratio {r:.4f} over {len(ratios)} alternating pairs (min {min(ratios):.4f}, "
                  f"max {max(ratios):.4f}); run-to-run spread of the parent's legs in this session {100.0 * spread:.2f} %; inside it: "
                  f"{'yes' if abs(r - 1.0) <= max(spread, 1e-9) else 'NO'}")


if __name__ == "__main__":
    main()
