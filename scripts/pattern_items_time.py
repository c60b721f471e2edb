"""What a regular expression PER ITEM costs a decode step, on the shape of scripts/pattern_time.py: Whisper-small.en widths,
beam 5, random weights, at 5 decoder rows (1 item) and at 240 (48 items), the synthetic tokenizer's vocabulary bytes.

  (a) A slot in no mode, and a slot under wlx_pattern_set (`(\\d{8} ?)+`), in this build against the parent commit's library (--parent-lib
      PATH): this change leaves both launch lists alone, so each ratio should lie inside the run-to-run spread of the parent's own legs in
      the same session. Alternating pairs of fresh processes (A B A B ...); the statistic is the median over the pairs of the per-pair
      ratio, the spread max / min of the parent's leg medians.
  (b) The added time per step (on - off, same process, off measured before and after) of the per-item launch (wlx_pattern_set_items) for
      §30's two tables — `(\\d{8} ?)+` and a table at the cell cap — with every item on ONE table, with every item on a table of its OWN
      (as many distinct tables as items: the table with one cell changed per copy; at the cap the pool holds 16, so the items cycle through
      16), and with NO item selected; beside them the single-pattern launch of the same build in the same process, the yardstick. Each
      difference includes the gap of one dependent launch: an upper bound of the kernel's own time.

Every leg is its own child process; a step's time is the HIP-event time of a whole generate divided by its decode steps, the median of
--reps generates after --warmup.

    python scripts/pattern_items_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 3] > profiles/pattern_items_time.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.pattern_time import cap_table  # noqa: E402


def variants(p, n):
    """n distinct tables of p's shape: p with the row of its last state rewritten to spell k in base n_states (no cell of it dead)"""
    from whisperlive_amd import pattern
    out = []
    for k in range(n):
        trans = p.trans.copy()
        for c in range(p.n_classes):
            trans[-1, c] = (k // p.n_states ** c) % p.n_states
        out.append(pattern.Pattern(regex=f"{p.regex}#{k}", byte_class=p.byte_class, trans=trans, accept=p.accept))
    return out


def child(args):
    from whisperlive_amd import _lib
    if args.old_abi:
        _lib.EXPORTS_PATTERN_ITEMS = []         # the parent commit's library has no per-item entry points: its legs never call them
    from oracle import logmel as olm
    from whisperlive_amd import pattern
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.tokenizer import synthetic_tokenizer
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
        return statistics.median(out)

    off, by = pattern.token_bytes(synthetic_tokenizer(spec.vocab), ids.eot)
    eng.set_pattern_vocab(ids.eot, off, by)
    small = pattern.compile_pattern(r"(\d{8} ?)+")
    res = {"rows": items * 5, "off_us": measure()}
    slot.set_pattern(small)
    res["single_small_us"] = measure()
    slot.clear_pattern()
    if not args.old_abi:
        for name, p in (("small", small), ("cap", cap_table())):
            own = variants(p, min(items, _lib.PATTERN_SET_MAX_CELLS // (p.n_states * p.n_classes), _lib.PATTERN_SET_MAX_TABLES))
            res[f"{name}_tables"] = len(own)
            legs = {}
            legs["off0"] = measure()
            if name == "cap":
                slot.set_pattern(p)
                res["single_cap_us"] = measure()
                slot.clear_pattern()
            slot.set_patterns(pattern.PatternSet([p]))
            slot.select_patterns([0] * items)
            legs["one"] = measure()
            slot.set_patterns(pattern.PatternSet(own))
            slot.select_patterns([b % len(own) for b in range(items)])
            legs["own"] = measure()
            slot.select_patterns([-1] * items)
            legs["none"] = measure()
            slot.clear_pattern()
            legs["off1"] = measure()
            base = 0.5 * (legs["off0"] + legs["off1"])
            res[name] = {k: legs[k] - base for k in ("one", "own", "none")}
            res[name]["single"] = res[f"single_{name}_us"] - (0.5 * (res["off_us"] + legs["off0"]) if name == "small" else base)
            res[name]["off_drift"] = legs["off1"] - legs["off0"]
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
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])


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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        return child(args)
    med = statistics.median
    print(f"pattern_items_time: {args.model}, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after {args.warmup}; "
          f"step = HIP-event time of a generate / its decode steps, us")
    for rows in [int(x) for x in args.row_counts.split(",")]:
        new, old = [], []
        for k in range(args.pairs):
            if args.parent_lib:
                old.append(run_child(args, rows, args.parent_lib, True))
            new.append(run_child(args, rows, None, False))
            b = new[-1]
            line = f"{rows:3d} rows, pair {k}: this build off {b['off_us']:8.2f}  wlx_pattern_set {b['single_small_us']:8.2f}"
            if args.parent_lib:
                line += f"  | parent off {old[-1]['off_us']:8.2f}  wlx_pattern_set {old[-1]['single_small_us']:8.2f}"
            print(line, flush=True)
        if old:         # (a)
            for key, what in (("off_us", "no mode"), ("single_small_us", "wlx_pattern_set")):
                ratios = [b[key] / a[key] for a, b in zip(old, new)]
                spread = max(a[key] for a in old) / min(a[key] for a in old) - 1.0
                print(f"{rows:3d} rows (a) {what}: this build / parent, median ratio {med(ratios):.4f} over {len(ratios)} alternating pairs (min {min(ratios):.4f}, "
                      f"max {max(ratios):.4f}); run-to-run spread of the parent's legs {100.0 * spread:.2f} %; inside it: "
                      f"{'yes' if abs(med(ratios) - 1.0) <= spread else 'NO'}")
        for name in ("small", "cap"):   # (b)
            cols = {k: [b[name][k] for b in new] for k in ("single", "one", "own", "none", "off_drift")}
            print(f"{rows:3d} rows (b) {name:5s} table, on - off per step, median of {len(new)} processes (min .. max): " + "; ".join(
                f"{label} {med(v):+.2f} ({min(v):+.2f} .. {max(v):+.2f})" for label, v in (
                    ("single-pattern launch", cols["single"]), ("per item, one table", cols["one"]),
                    (f"per item, {new[0][name + '_tables']} tables", cols["own"]), ("per item, none selected", cols["none"]), ("off after - off before", cols["off_drift"]))))


if __name__ == "__main__":
    main()
