"""Timing of the HIP speaker-embedding engine (WeSpeaker ResNet34 shape, seeded weights that owe nothing to Whisper): device time per
embed at 1, 3, 10 and 30 s of audio from the engine's HIP events (wlx_spk_debug_timings: filterbank, network + pooling + head) and
the wall time of the call; beside it, for context, the torch restatement of tests/spk_oracle.py on 16 CPU threads.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.
usage: python scripts/spk_time.py [--no-cpu]      (child: --gpu SECONDS, e.g. under rocprofv3 --kernel-trace --stats)"""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd import spk_weights  # noqa: E402
from whisperlive_amd.synthetic import speech_like_pcm  # noqa: E402

SPEC = spk_weights.RESNET34
LENGTHS = (1.0, 3.0, 10.0, 30.0)
GPU_STEP_LIMIT_S = 120


def weights():
    return spk_weights.fold(spk_weights.random_weights(SPEC, seed=0), SPEC)


def gpu_step(seconds: float):
    from whisperlive_amd.diarization import SpeakerEmbedderHIP
    eng = SpeakerEmbedderHIP(SPEC, weights(), device=0)
    pcm = speech_like_pcm(seconds, seed=5)
    for _ in range(3):
        eng.embed(pcm)
    fb, nn, wall = [], [], []
    for _ in range(20):
        t0 = time.perf_counter()
        eng.embed(pcm)
        wall.append(1e3 * (time.perf_counter() - t0))
        a, b = eng.timings()
        fb.append(a)
        nn.append(b)
    eng.close()
    print(f"  HIP  {seconds:5.1f} s audio: device {np.median(fb) + np.median(nn):7.3f} ms (filterbank {np.median(fb):.3f}, network "
          f"{np.median(nn):.3f}) | call {np.median(wall):7.3f} ms wall (p50 of 20)")


def cpu_step(seconds: float):
    import torch
    sys.path.insert(0, "tests")
    import spk_oracle as O
    torch.set_num_threads(16)
    w = weights()
    pcm = speech_like_pcm(seconds, seed=5)
    O.embed(SPEC, w, pcm)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        O.embed(SPEC, w, pcm)
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"  CPU  {seconds:5.1f} s audio: {np.median(ts):8.1f} ms (torch fp32 restatement, 16 threads, float64 filterbank included)")


if __name__ == "__main__":
    if "--gpu" in sys.argv:
        gpu_step(float(sys.argv[sys.argv.index("--gpu") + 1]))
        sys.exit(0)
    print("WeSpeaker ResNet34 shape ([3,4,6,3] blocks, 32..256 channels, 80 mel bins), seeded weights, one segment per call")
    for s in LENGTHS:
        rc = subprocess.run(["timeout", "-k", "10", str(GPU_STEP_LIMIT_S), sys.executable, sys.argv[0], "--gpu", str(s)]).returncode
        if rc != 0:
            print(f"GPU step {s} s ended with status {rc}: stopping")
            sys.exit(rc)
    if "--no-cpu" not in sys.argv:
        for s in LENGTHS:
            cpu_step(s)
