"""Timing of offline diarization of a wave of files: a loop of wlx_spk_diarize_pcm (one call and one wait per file) against
wlx_spk_diarize_many (the wave's windows in shared embed passes, the files clustered side by side, one wait per call), in ONE process on
seeded weights (WeSpeaker ResNet34 shape; tiny.en engine for the slot). Cases:
  short   48 files of 20 s, the 1.5 s / 0.75 s window grid over each whole file (25 windows a file): one many-call;
  long    16 files of 10 min (799 windows a file, 12784 in all): the many-calls diarization.plan_diarize_many cuts (8192 windows a call).
Per case: alternating pairs (loop, many), PAIRS of them after one warm-up pair, p50 and the spread of wall time and of the HIP-event time
of the clustering launches (distance matrices + agglomeration; for the loop the sum over its files, for the many route over its calls),
and whether the labels of the two routes are equal.
  --single-check   instead: the single-file path alone, as scripts/spk_cluster_time.py measures it at n = 800 (wlx_spk_cluster on rows of
                   256 around 8 directions: device time of both launches and wall time, p50 of CALLS), one line on stdout — run from
                   the root of this tree and of the parent commit's in alternating pairs, the regression check of the kernels' refactor.
Writes profiles/spk_diarize_many_time.txt (or --out PATH).
usage: python scripts/spk_diarize_many_time.py [--out PATH] [--pairs N] [--single-check]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd import file_diarization as FD  # noqa: E402
from whisperlive_amd import spk_weights  # noqa: E402
from whisperlive_amd.specs import SPECS  # noqa: E402
from whisperlive_amd.synthetic import speech_like_pcm  # noqa: E402

THRESHOLD = 0.45
CALLS = 7


def rows_around(n, dim=256, speakers=8, seed=1):          # scripts/spk_cluster_time.py
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((dim, speakers)))[0].T
    x = centres[rng.integers(0, speakers, size=n)] + 0.03 * rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def embedder():
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    spec = spk_weights.RESNET34
    return SpeakerEmbedderHIP(spec, spk_weights.fold(spk_weights.random_weights(spec, seed=0), spec), device=0)


def single_check():
    spk = embedder()
    X = rows_around(800)
    for _ in range(3):
        spk.cluster(X, THRESHOLD)
    dev, wall = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        spk.cluster(X, THRESHOLD)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(spk.cluster_timings())
    aff, ahc = float(np.median([d[0] for d in dev])), float(np.median([d[1] for d in dev]))
    print(f"single-file path, n = 800: distance matrix {aff:.4f} ms + clustering {ahc:.4f} ms = {aff + ahc:.4f} ms (HIP events), "
          f"wlx_spk_cluster wall {float(np.median(wall)):.4f} ms (p50 of {CALLS})")
    spk.close()
    return 0


def spread(xs):
    return f"{float(np.median(xs)):.2f} ms (min {min(xs):.2f}, max {max(xs):.2f})"


def case(spk, eng, name, n_files, seconds, pairs, lines):
    from whisperlive_amd.diarization import plan_diarize_many
    slot = eng.create_slot(n_files, 5)
    base = speech_like_pcm(float(seconds), seed=3).astype(np.float32)
    for item in range(n_files):
        slot.pcm_put(np.roll(base, 7919 * item), item=item)          # every file its own audio: the same signal, shifted
    n_samples = slot.pcm_count(0)
    windows = [(s, c) for s, c, _ in FD.plan_windows([(0.0, n_samples / 16000.0)])]
    calls = plan_diarize_many([len(windows)] * n_files)

    def loop():
        dev, labels = 0.0, []
        t0 = time.perf_counter()
        for item in range(n_files):
            labels.append(spk.diarize_resident(slot, item, windows, THRESHOLD)[0])
            dev += sum(spk.cluster_timings())
        return 1e3 * (time.perf_counter() - t0), dev, labels

    def many():
        dev, labels = 0.0, []
        t0 = time.perf_counter()
        for call in calls:
            got = spk.diarize_many(slot, call, [windows] * len(call), THRESHOLD, 0)
            labels += [g[0] for g in got]
            dev += sum(spk.cluster_timings())
        return 1e3 * (time.perf_counter() - t0), dev, labels

    a, b = loop(), many()                                              # the warm-up pair (it also makes both routes' buffers)
    same = all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    wall_l, wall_m, dev_l, dev_m = [], [], [], []
    for _ in range(pairs):
        a, b = loop(), many()
        wall_l.append(a[0]), dev_l.append(a[1]), wall_m.append(b[0]), dev_m.append(b[1])
    lines.append(f"{name}: {n_files} files of {seconds} s, {len(windows)} windows a file ({n_files * len(windows)} in all), "
                 f"{len(calls)} wlx_spk_diarize_many call(s); alternating pairs, p50 of {pairs}")
    lines.append(f"  loop of wlx_spk_diarize_pcm: wall {spread(wall_l)} | clustering launches {spread(dev_l)} (HIP events, summed over the files)")
    lines.append(f"  wlx_spk_diarize_many:        wall {spread(wall_m)} | clustering launches {spread(dev_m)} (HIP events, summed over the calls)")
    lines.append(f"  many / loop: wall {np.median(wall_m) / np.median(wall_l):.3f}, clustering launches {np.median(dev_m) / np.median(dev_l):.3f}; "
                 f"{int(max(x.max() for x in b[2])) + 1} cluster(s) at the most, labels equal: {same}")
    slot.close()
    return same


def main():
    if "--single-check" in sys.argv:
        return single_check()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/spk_diarize_many_time.txt"
    pairs = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 7
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    spk = embedder()
    eng = HipWhisperEngine(SPECS["tiny.en"], random_weights(SPECS["tiny.en"], seed=7))
    lines = ["offline diarization of a wave of files (threshold 0.45, windows of 1.5 s every 0.75 s): a loop of wlx_spk_diarize_pcm against "
             "wlx_spk_diarize_many, one process, seeded ResNet34-shape weights (scripts/spk_diarize_many_time.py)"]
    ok = case(spk, eng, "short", 48, 20, pairs, lines)
    ok = case(spk, eng, "long", 16, 600, pairs, lines) and ok
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    eng.close()
    spk.close()
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
