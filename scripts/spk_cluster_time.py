"""Timing of offline speaker clustering on the device against the host oracle (file_diarization.cluster_host, NumPy float32: the only
baseline there is, no earlier version of the project clusters a file). WeSpeaker ResNet34 shape with seeded weights; embeddings for the
clustering figures are seeded unit vectors around eight directions. Figures:
  cluster   n = 100, 800, 2048 rows of 256: device time of the distance matrix + the clustering (wlx_spk_debug_cluster_timings, HIP
            events) and wall time of wlx_spk_cluster (upload, both kernels, centroids, one wait), p50 of CALLS, against the wall time of
            cluster_host on the same rows (run in full at every size; p50 of 3), and whether the labels agree;
  file      one wlx_spk_diarize_pcm of a 10-minute resident item (the 1.5 s / 0.75 s window grid over the whole file) against
            embed_resident + cluster_host on the same windows, wall, p50 of 3.
Writes profiles/spk_cluster_time.txt (or --out PATH). Exit status 3 when device and host labels differ.
usage: python scripts/spk_cluster_time.py [--out PATH] [--minutes M]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd import file_diarization as FD  # noqa: E402
from whisperlive_amd import spk_weights  # noqa: E402
from whisperlive_amd.specs import SPECS  # noqa: E402
from whisperlive_amd.synthetic import speech_like_pcm  # noqa: E402

CALLS = 7
THRESHOLD = 0.45


def p50(call, calls):
    call()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def device_distances(lib, X):
    """the matrix the device clusters (wlx_spk_debug_affinity): equality of labels is asked on the same matrix, as the tests do"""
    import ctypes as C
    out = np.zeros((len(X), len(X)), np.float32)
    f32p = C.POINTER(C.c_float)
    assert lib.wlx_spk_debug_affinity(0, X.ctypes.data_as(f32p), X.shape[0], X.shape[1], out.ctypes.data_as(f32p)) == 0
    return out


def rows_around(n, dim=256, speakers=8, seed=1):
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((dim, speakers)))[0].T
    x = centres[rng.integers(0, speakers, size=n)] + 0.03 * rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/spk_cluster_time.txt"
    minutes = float(sys.argv[sys.argv.index("--minutes") + 1]) if "--minutes" in sys.argv else 10.0
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    spec = spk_weights.RESNET34
    spk = SpeakerEmbedderHIP(spec, spk_weights.fold(spk_weights.random_weights(spec, seed=0), spec), device=0)
    lines = ["offline speaker clustering (average linkage on cosine distances, threshold 0.45): device (wlx_spk_cluster, csrc/spk_cluster.hip) "
             "against the host oracle (file_diarization.cluster_host, NumPy float32); rows of 256 around 8 directions"]
    agree = True
    for n in (100, 800, 2048):
        X = rows_around(n)
        labels, _ = spk.cluster(X, THRESHOLD)
        dev = []
        for _ in range(CALLS):
            spk.cluster(X, THRESHOLD)
            dev.append(spk.cluster_timings())
        aff, ahc = float(np.median([d[0] for d in dev])), float(np.median([d[1] for d in dev]))
        wall = p50(lambda: spk.cluster(X, THRESHOLD), CALLS)
        host = p50(lambda: FD.cluster_host(X, THRESHOLD), 3)
        same = bool(np.array_equal(labels, FD.cluster_host(X, THRESHOLD, dist=device_distances(spk.lib, X)).labels))
        agree = agree and same
        lines.append(f"n = {n}: device distance matrix {aff:.3f} ms + clustering {ahc:.3f} ms = {aff + ahc:.3f} ms (HIP events, p50 of {CALLS}) | "
                     f"wlx_spk_cluster wall {wall:.2f} ms (p50 of {CALLS}) | cluster_host wall {host:.1f} ms (run in full, p50 of 3) | "
                     f"{int(labels.max()) + 1} clusters, labels equal: {same}")
    # ---- a whole file
    eng = HipWhisperEngine(SPECS["tiny.en"], random_weights(SPECS["tiny.en"], seed=7))
    slot = eng.create_slot(1, 5)
    slot.pcm_put(speech_like_pcm(60.0 * minutes, seed=3).astype(np.float32))
    n_samples = slot.pcm_count()
    windows = [(s, c) for s, c, _ in FD.plan_windows([(0.0, n_samples / 16000.0)])]

    def device_route():
        return spk.diarize_resident(slot, 0, windows, THRESHOLD)[0]

    def host_route():
        embs = spk.embed_resident(slot, 0, windows)
        return FD.cluster_host(np.stack(embs), THRESHOLD).labels

    dev_labels, _, _, dist = spk.diarize_resident(slot, 0, windows, THRESHOLD, want_embeddings=True, want_distances=True)
    aff, ahc = spk.cluster_timings()
    same = bool(np.array_equal(dev_labels, FD.cluster_host(None, THRESHOLD, dist=dist).labels))
    agree = agree and same
    wall_dev, wall_host = p50(device_route, 3), p50(host_route, 3)
    lines.append(f"file: {minutes:.0f} min resident ({n_samples} samples), {len(windows)} windows of 1.5 s every 0.75 s: wlx_spk_diarize_pcm "
                 f"{wall_dev:.1f} ms wall (its clustering part on the device: {aff:.3f} + {ahc:.3f} ms) | embed_resident + cluster_host "
                 f"{wall_host:.1f} ms wall | {wall_host / wall_dev:.2f}x (p50 of 3); {int(dev_labels.max()) + 1} clusters, labels equal: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    slot.close(); eng.close(); spk.close()
    return 0 if agree else 3


if __name__ == "__main__":
    sys.exit(main())
