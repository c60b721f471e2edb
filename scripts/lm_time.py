"""What n-gram language-model fusion costs a decode step, on the benchmark's decode shape: Whisper-small.en widths, beam 5,
random weights (the step's launches do not depend on the values), at 5 decoder rows (one stream) and at 240 (48 windows in one group).

  1. no model set, this build against the parent commit's library (--parent-lib PATH, a libwlx.so built from the parent): the step of a
     slot without a model keeps its launch list, so the two must agree within the run-to-run spread of the parent measured in the same
     session. Alternating pairs of fresh processes (A B A B ...); the statistic is the median over the pairs of the per-pair ratio, the
     spread is that of the parent's own legs (max / min of their medians).
  2. ON against OFF in the same process of this build: a trigram model of about 10^5 edges, a model at the edge cap (2^22 edges), and —
     the yardsticks — the phrase-list grammar of scripts/grammar_time.py (200 phrases) and the small pattern of scripts/pattern_time.py.
     Each difference is the kernel's device time PLUS the gap its dependent launch adds to the step: an upper bound of the kernel's own
     time.

The models are synthetic (random tokens and scores): the launch's work depends on the table's shape, not on its values. Every context of
the cap model carries 1024 edges, so every row scatters a full chain at every step. Every leg is its own child process (one GPU context
at a time); a step's time is the HIP-event time of a whole generate divided by its decode steps, the median of --reps generates after
--warmup.

    python scripts/lm_time.py [--parent-lib whisperlive_amd/libwlx_parent.so] [--pairs 3] [--reps 20] > profiles/lm_time.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_lm(vocab, eot, n_ctx1, n_ctx2, per_ctx, seed=5):
    """a trigram automaton built as arrays: n_ctx1 one-token contexts and n_ctx2 two-token contexts of per_ctx random edges each; the
    one-token contexts are the tokens 300 .. 300 + n_ctx1 - 1, a two-token context backs off to a one-token one, every edge leads on"""
    import numpy as np
    from whisperlive_amd import lm
    rng = np.random.default_rng(seed)
    n = 1 + n_ctx1 + n_ctx2
    off = np.zeros(n + 1, np.int64)
    off[2:] = np.arange(1, n) * per_ctx
    n_edges = int(off[-1])
    base = np.sort(rng.choice(eot, size=per_ctx, replace=False)).astype(np.int32)
    tok = ((base[None, :] + rng.integers(0, eot, size=(n - 1, 1))) % eot).astype(np.int32)
    tok.sort(axis=1)                            # (a rotation of distinct tokens: distinct and, sorted, ascending within a state)
    boff = np.zeros(n, np.int32)
    boff[1 + n_ctx1:] = 1 + rng.integers(0, n_ctx1, size=n_ctx2)
    unext = np.zeros(vocab, np.int32)
    unext[300:300 + n_ctx1] = 1 + np.arange(n_ctx1)
    return lm.NgramLM(vocab, eot, 3, 1, off, boff, rng.uniform(-2, -0.1, size=n), tok.reshape(-1), rng.uniform(-9, -0.5, size=n_edges),
                      rng.integers(1, n, size=n_edges), np.where(np.arange(vocab) <= eot, rng.uniform(-12, -2, size=vocab), 0.0), unext)


def child(args):
    import numpy as np
    from whisperlive_amd import _lib
    if args.old_abi:
        _lib.EXPORTS_LM = []                    # a library from before wlx_lm_*: its legs never call them
    from oracle import logmel as olm
    from whisperlive_amd import grammar, pattern
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
        return out

    res = {"rows": items * 5, "off_us": measure()}
    if not args.old_abi:
        models = {"trigram": synthetic_lm(spec.vocab, ids.eot, 400, 1600, 50), "cap": synthetic_lm(spec.vocab, ids.eot, 400, 3696, 1024)}
        for name, m in models.items():
            slot.set_lm(m, 0.3)
            res[f"{name}_us"] = measure()
            res[f"{name}_table"] = dict(states=m.n_states, edges=m.n_edges)
            slot.clear_lm()
            eng.destroy_lm(m)
        res["off_again_us"] = measure()
        rng = np.random.default_rng(5)
        phrases = [[int(x) for x in rng.integers(300, 20000, size=int(rng.integers(1, 4)))] for _ in range(args.phrases)]
        g = grammar.compile_grammar(None, phrases, vocab=spec.vocab, eot=ids.eot)
        slot.set_grammar(g)
        res["phrases_us"] = measure()
        slot.clear_grammar()
        off, by = pattern.token_bytes(synthetic_tokenizer(spec.vocab), ids.eot)
        eng.set_pattern_vocab(ids.eot, off, by)
        slot.set_pattern(pattern.compile_pattern(r"(\d{8} ?)+"))
        res["pattern_us"] = measure()
        slot.clear_pattern()
        res["off_last_us"] = measure()
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
           "--warmup", str(args.warmup), "--phrases", str(args.phrases), "--rows", str(rows)] + (["--old-abi"] if old_abi else [])
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
    ap.add_argument("--phrases", type=int, default=200)
    args = ap.parse_args()
    if args.child:
        return child(args)
    med = statistics.median
    print(f"lm_time: {args.model}, beam 5, {args.tokens} tokens per generate, {args.reps} generates per leg after {args.warmup}; "
          f"step = HIP-event time of a generate / its decode steps, us")
    for rows in [int(x) for x in args.row_counts.split(",")]:
        new_legs, old_legs, ratios = [], [], []
        for k in range(args.pairs):
            a = run_child(args, rows, args.parent_lib, True) if args.parent_lib else None
            b = run_child(args, rows, None, False)
            new_legs.append(b)
            line = (f"{rows:3d} rows, pair {k}: this build off {med(b['off_us']):8.2f}  trigram {med(b['trigram_us']):8.2f}  cap {med(b['cap_us']):8.2f}  "
                    f"off again {med(b['off_again_us']):8.2f}  phrase list {med(b['phrases_us']):8.2f}  pattern {med(b['pattern_us']):8.2f}  "
                    f"off last {med(b['off_last_us']):8.2f}")
            if a is not None:
                old_legs.append(med(a["off_us"]))
                ratios.append(med(b["off_us"]) / med(a["off_us"]))
                line += f"  | parent off {med(a['off_us']):8.2f}  ratio this/parent {ratios[-1]:.4f}"
            print(line, flush=True)
        first = new_legs[0]
        print(f"{rows:3d} rows: models: trigram {first['trigram_table']}, cap {first['cap_table']}")
        for name, base in (("trigram", ("off_us", "off_again_us")), ("cap", ("off_us", "off_again_us")), ("phrases", ("off_again_us", "off_last_us")),
                           ("pattern", ("off_again_us", "off_last_us"))):
            ds = [med(b[f"{name}_us"]) - med([med(b[base[0]]), med(b[base[1]])]) for b in new_legs]
            print(f"{rows:3d} rows: {name} on - off, same process: median of pairs {med(ds):+.2f} us per step (min {min(ds):+.2f}, max {max(ds):+.2f})")
        if ratios:
            spread = max(old_legs) / min(old_legs) - 1.0
            r = med(ratios)
            print(f"{rows:3d} rows: no model, this build / parent: median ratio {r:.4f} over {len(ratios)} alternating pairs (min {min(ratios):.4f}, "
                  f"max {max(ratios):.4f}); run-to-run spread of the parent's legs in this session {100.0 * spread:.2f} %; inside it: "
                  f"{'yes' if abs(r - 1.0) <= max(spread, 1e-9) else 'NO'}")


if __name__ == "__main__":
    main()
