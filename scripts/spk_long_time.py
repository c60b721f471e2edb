"""Timing of the long form of the offline speaker clustering (include/wlx_spk_long.h, spk_ahc_long_kernel) against what a file of more
than 2048 windows got before it: embed_resident + file_diarization.cluster_host on one host thread. WeSpeaker ResNet34 shape with seeded
weights; rows for the clustering figures are seeded unit vectors of 256 around eight directions, threshold 0.45. Figures:
  cluster   n = 2049, 4800, 8192 rows: device time of the distance matrix and of the clustering launch (wlx_spk_debug_cluster_timings, HIP
            events, p50 of CALLS wlx_spk_cluster_long calls), microseconds per round (merge) of the clustering, the call's wall time;
  file      one resident item of an hour (about 4800 windows of 1.5 s every 0.75 s): wall time of diarize_resident_long against
            embed_resident + cluster_host on the same windows, RUNS alternating runs each, medians, the ratio and the spread (max / min)
            of either route's runs; labels equal to cluster_host on the matrix the device clustered;
  unchanged wlx_spk_cluster at n = 800 in this build and, with --parent-lib PATH, in the parent commit's library: alternating child
            processes, p50 wall and device time of each.
Writes profiles/spk_long_time.txt (or --out PATH). Exit status 3 when device and host labels differ.
usage: python scripts/spk_long_time.py [--out PATH] [--minutes M] [--parent-lib whisperlive_amd/libwlx_parent.so]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from scripts.spk_cluster_time import p50, rows_around  # noqa: E402

CALLS, RUNS, PAIRS = 5, 5, 3
THRESHOLD = 0.45


def engine():
    from whisperlive_amd import spk_weights
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    spec = spk_weights.RESNET34
    return SpeakerEmbedderHIP(spec, spk_weights.fold(spk_weights.random_weights(spec, seed=0), spec), device=0)


def child():
    """wlx_spk_cluster at n = 800 in whichever library WLX_LIB names"""
    from whisperlive_amd import _lib
    if "--old-abi" in sys.argv:
        _lib.EXPORTS_SPK_LONG = []              # the parent commit's library has no long entry points: this leg never calls them
    spk = engine()
    X = rows_around(800)
    wall = p50(lambda: spk.cluster(X, THRESHOLD), 15)
    dev = [(spk.cluster(X, THRESHOLD), spk.cluster_timings())[1] for _ in range(15)]
    print("RESULT " + json.dumps({"wall": wall, "aff": float(np.median([d[0] for d in dev])), "ahc": float(np.median([d[1] for d in dev]))}))
    spk.close()


def run_child(lib):
    env = dict(os.environ)
    env.pop("WLX_LIB", None)
    if lib:
        env["WLX_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--old-abi"] if lib else []), env=env, capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out_path, minutes, parent = arg("--out", "profiles/spk_long_time.txt"), float(arg("--minutes", 60.0)), arg("--parent-lib", None)
    from whisperlive_amd import file_diarization as FD
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import speech_like_pcm
    from whisperlive_amd.weights import random_weights
    lines = ["long form of the offline speaker clustering (wlx_spk_cluster_long / wlx_spk_diarize_pcm_long, spk_ahc_long_kernel: one workgroup, "
             "12 n bytes of LDS); rows of 256 around 8 directions, threshold 0.45"]
    # ---- unchanged: the short form against the parent commit's library, before this process opens the GPU
    legs = [(run_child(None), run_child(parent) if parent else None) for _ in range(PAIRS)]
    med = lambda side, key: float(np.median([leg[side][key] for leg in legs]))
    line = f"unchanged: wlx_spk_cluster n = 800, this build: wall {med(0, 'wall'):.2f} ms, device {med(0, 'aff'):.3f} + {med(0, 'ahc'):.3f} ms"
    if parent:
        line += f" | parent commit's library: wall {med(1, 'wall'):.2f} ms, device {med(1, 'aff'):.3f} + {med(1, 'ahc'):.3f} ms"
    lines.append(line + f" (medians of {PAIRS} alternating child processes, p50 of 15 calls each)")
    spk = engine()
    for n in (2049, 4800, 8192):
        X = rows_around(n)
        labels, _ = spk.cluster_long(X, THRESHOLD)
        dev = [(spk.cluster_long(X, THRESHOLD), spk.cluster_timings())[1] for _ in range(CALLS)]
        aff, ahc = float(np.median([d[0] for d in dev])), float(np.median([d[1] for d in dev]))
        wall = p50(lambda: spk.cluster_long(X, THRESHOLD), CALLS)
        rounds = n - (int(labels.max()) + 1)
        lines.append(f"n = {n}: device distance matrix {aff:.3f} ms + clustering {ahc:.3f} ms (HIP events, p50 of {CALLS}); {rounds} rounds, "
                     f"{1e3 * ahc / rounds:.2f} us per round | wlx_spk_cluster_long wall {wall:.1f} ms (p50 of {CALLS})")
    # ---- a whole file of an hour
    eng = HipWhisperEngine(SPECS["tiny.en"], random_weights(SPECS["tiny.en"], seed=7))
    slot = eng.create_slot(1, 5)
    slot.pcm_put(np.tile(speech_like_pcm(60.0, seed=3).astype(np.float32), int(minutes)))
    n_samples = slot.pcm_count()
    windows = [(s, c) for s, c, _ in FD.plan_windows([(0.0, n_samples / 16000.0)])]

    def host_route():
        X = np.stack(spk.embed_resident(slot, 0, windows))
        return FD.cluster_host(X / np.linalg.norm(X, axis=1, keepdims=True), THRESHOLD).labels

    dev_labels, _, _, dist = spk.diarize_resident_long(slot, 0, windows, THRESHOLD, want_embeddings=True, want_distances=True)
    aff, ahc = spk.cluster_timings()
    same = bool(np.array_equal(dev_labels, FD.cluster_host(None, THRESHOLD, dist=dist).labels))
    t_dev, t_host = [], []
    for _ in range(RUNS):
        for route, ts in ((lambda: spk.diarize_resident_long(slot, 0, windows, THRESHOLD), t_dev), (host_route, t_host)):
            t0 = time.perf_counter()
            route()
            ts.append(time.perf_counter() - t0)
    md, mh = float(np.median(t_dev)), float(np.median(t_host))
    lines.append(f"file: {minutes:.0f} min resident ({n_samples} samples), {len(windows)} windows of 1.5 s every 0.75 s, {int(dev_labels.max()) + 1} "
                 f"clusters: diarize_resident_long {md:.2f} s wall (runs {' '.join(f'{t:.2f}' for t in t_dev)}; its clustering part on the device: "
                 f"{aff:.1f} + {ahc:.1f} ms) | embed_resident + cluster_host {mh:.2f} s wall (runs {' '.join(f'{t:.2f}' for t in t_host)}) | "
                 f"{mh / md:.2f}x, {RUNS} alternating runs each; spread max / min {max(t_dev) / min(t_dev):.3f} and {max(t_host) / min(t_host):.3f}; "
                 f"labels equal to cluster_host on the device's matrix: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    slot.close(); eng.close(); spk.close()
    return 0 if same else 3


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main())
