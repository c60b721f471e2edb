"""Timing of the batched speaker embed (wlx_spk_embed_batch) against the same segments through wlx_spk_embed one by one and against
one embed of the summed length: WeSpeaker ResNet34 shape, seeded weights, device time (filterbank + network) from the engine's HIP
events (wlx_spk_debug_timings), p50 of 20 calls. Two shapes: 10 x 3 s on the default 45 s engine, 32 x 3 s on a max_seconds = 120
engine. Every shape is a child process under its own time limit; the first one that fails ends the run. Writes
profiles/spk_batch_time.txt (or --out PATH).
usage: python scripts/spk_batch_time.py [--out PATH]      (child: --shape N MAX_SECONDS)"""
import dataclasses
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd import spk_weights  # noqa: E402
from whisperlive_amd.synthetic import speech_like_pcm  # noqa: E402

SHAPES = ((10, 45), (32, 120))          # (segments of 3 s, the engine's max_seconds)
SEGMENT_S = 3.0
CALLS = 20
STEP_LIMIT_S = 180


def p50(call):
    """`call` returns its device milliseconds: (p50 of them, p50 of the wall time of the call)"""
    for _ in range(3):
        call()
    dev, wall = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        dev.append(call())
        wall.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(dev)), float(np.median(wall))


def shape_step(n: int, max_seconds: int):
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    spec = dataclasses.replace(spk_weights.RESNET34, max_seconds=max_seconds)
    eng = SpeakerEmbedderHIP(spec, spk_weights.fold(spk_weights.random_weights(spec, seed=0), spec), device=0)
    pcms = [speech_like_pcm(SEGMENT_S, seed=5 + i)[:int(SEGMENT_S * 16000)] for i in range(n)]
    whole = np.concatenate(pcms)

    def batch():
        eng.embed_many(pcms)
        return sum(eng.timings())

    def serial():                        # the sum of the n single embeds' device times
        total = 0.0
        for p in pcms:
            eng.embed(p)
            total += sum(eng.timings())
        return total

    def one_long():
        eng.embed(whole)
        return sum(eng.timings())
    rows = eng.embed_many(pcms)
    same = all((r.view(np.uint32) == eng.embed(p).view(np.uint32)).all() for r, p in zip(rows, pcms))
    b_dev, b_wall = p50(batch)
    s_dev, s_wall = p50(serial)
    w_dev, w_wall = p50(one_long)
    eng.close()
    print(f"{n} x {SEGMENT_S:.0f} s, max_seconds {max_seconds}: batch {b_dev:.3f} ms device ({b_wall:.3f} ms wall) | one by one "
          f"{s_dev:.3f} ms device ({s_wall:.3f} ms wall) | one embed of {n * SEGMENT_S:.0f} s {w_dev:.3f} ms device ({w_wall:.3f} ms wall) | "
          f"one by one / batch {s_dev / b_dev:.2f}x | rows bit-identical to single embeds: {same}", flush=True)
    return 0 if same and b_dev < 0.5 * s_dev else 3


if __name__ == "__main__":
    if "--shape" in sys.argv:
        at = sys.argv.index("--shape")
        sys.exit(shape_step(int(sys.argv[at + 1]), int(sys.argv[at + 2])))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/spk_batch_time.txt"
    lines = ["wlx_spk_embed_batch against wlx_spk_embed one by one: WeSpeaker ResNet34 shape, seeded weights, device time = filterbank + "
             f"network from the engine's HIP events, p50 of {CALLS} calls (floor: batch under half of one by one)"]
    status = 0
    for n, max_seconds in SHAPES:
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--shape", str(n), str(max_seconds)],
                              capture_output=True, text=True)
        sys.stderr.write(proc.stderr[-2000:])
        lines += [ln for ln in proc.stdout.splitlines() if ln.strip()]
        if proc.returncode not in (0, 3):
            lines.append(f"shape {n} x {SEGMENT_S:.0f} s ended with status {proc.returncode}: stopping")
            status = proc.returncode
            break
        status = status or proc.returncode
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)
    sys.exit(status)
