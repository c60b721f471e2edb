"""Timing of batched word alignment (wlx_align_batch: one launch sequence, post-processing on the device, one wait) against a loop of
wlx_align over the same entries (post-processing on one host thread per entry). Whisper small.en shape with seeded weights; 1, 8 and
24 entries of 60 text tokens over 1500 frames; once with the published-default head list (the upper half of the decoder: 72 heads) and
once with a 10-head list. Wall time is the host clock around calls that return with the stream idle; pass / post are the HIP-event
times of the batch call (wlx_debug_align_timings: the decoder passes with their score capture, and everything behind them). The two
sides alternate in one process; p50 of CALLS rounds after WARMUP. Every point is a child process under its own time limit; the first
one that fails ends the run. Writes profiles/align_batch_time.txt (or --out PATH).
usage: python scripts/align_time.py [--out PATH]      (child: --point HEADS:N)"""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

N_TEXT, NUM_FRAMES = 60, 3000
HEAD_LISTS = ("default", "ten")
ENTRIES = (1, 8, 24)
WARMUP, CALLS = 1, 5
STEP_LIMIT_S = 280


def point_step(name: str):
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import speech_like_pcm
    from whisperlive_amd.weights import random_weights
    from whisperlive_amd.word_timing import default_alignment_heads
    which, n = name.split(":")
    n = int(n)
    spec = SPECS["small.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7))
    slot = eng.create_slot(n, 5)
    pcm = speech_like_pcm(30.0, seed=5)
    frames = [slot.logmel(np.roll(pcm, 1600 * i), item=i) for i in range(n)]
    slot.encode(n, seek=[0] * n, seg=[f - 1 for f in frames])
    heads = default_alignment_heads(spec.dec_layers, spec.n_heads)
    if which == "ten":
        heads = [(6 + k % 6, (5 * k + 1) % spec.n_heads) for k in range(10)]
    tb = spec.vocab - 1501
    sot, eot, no_ts = tb - 106, tb - 107, tb - 1
    rng = np.random.default_rng(11)
    seqs = [[sot, no_ts] + rng.integers(300, eot - 1, size=N_TEXT).tolist() + [eot] for _ in range(n)]

    def batch():
        return slot.align_batch(seqs, 1, [NUM_FRAMES] * n, heads, eot, items=list(range(n)))

    def loop():
        return [slot.align(seqs[i], 1, NUM_FRAMES, heads, eot, item=i) for i in range(n)]
    rb, rl = batch(), loop()
    same_probs = all(a[2].tobytes() == b[2].tobytes() for a, b in zip(rb, rl))
    same_paths = sum(int(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])) for a, b in zip(rb, rl))
    t = {batch: [], loop: []}
    dev = []
    for r in range(WARMUP + CALLS):
        for f in (batch, loop):
            t0 = time.perf_counter()
            f()
            if r >= WARMUP:
                t[f].append(1e3 * (time.perf_counter() - t0))
                if f is batch:
                    dev.append(slot.align_timings())
    b, l = float(np.median(t[batch])), float(np.median(t[loop]))
    pass_ms, post_ms = float(np.median([d[0] for d in dev])), float(np.median([d[1] for d in dev]))
    print(f"{len(heads)} heads, {n} x {N_TEXT} text tokens x 1500 frames: wlx_align_batch {b:.2f} ms wall (pass {pass_ms:.2f} ms + post {post_ms:.2f} ms "
          f"device) | wlx_align loop {l:.2f} ms wall | loop / batch {l / b:.2f}x | probs bit-identical: {same_probs} | identical paths "
          f"{same_paths} of {n}", flush=True)
    slot.close()
    eng.close()
    return 0 if same_probs else 3


if __name__ == "__main__":
    if "--point" in sys.argv:
        sys.exit(point_step(sys.argv[sys.argv.index("--point") + 1]))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/align_batch_time.txt"
    lines = ["wlx_align_batch against a wlx_align loop over the same entries: Whisper small.en shape, seeded weights, "
             f"p50 of {CALLS} alternating rounds after {WARMUP} warm-up round"]
    status = 0
    for which in HEAD_LISTS:
        for n in ENTRIES:
            name = f"{which}:{n}"
            proc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--point", name],
                                  capture_output=True, text=True)
            sys.stderr.write(proc.stderr[-2000:])
            lines += [ln for ln in proc.stdout.splitlines() if ln.strip()]
            if proc.returncode not in (0, 3):
                lines.append(f"point {name} ended with status {proc.returncode}: stopping")
                status = proc.returncode
                break
            status = status or proc.returncode
        if status not in (0, 3):
            break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)
    sys.exit(status)
