"""Timing of the file path's first stage, device route against host route, for 60 s and 600 s of audio in two file shapes:
44.1 kHz stereo float32 and 48 kHz mono int16.
  device route: HIP-event time of the resampling kernel (wlx_debug_resample_timed: the block launches' summed time, product block
                size) and the wall time of Slot.put_frames + Slot.pcm() (upload in the file's format, kernel, 16 kHz mono copy back);
  host route:   wall time of the float32 channel mean + scipy.signal.resample_poly in float64 (audio_io.frames_to_mono: one CPU
                thread) + Slot.logmel's upload of the result (wlx_pcm_put).
Every GPU step is a child process under its own time limit; the first one that fails ends the run.
usage: python scripts/resample_time.py > profiles/resample_time.txt      (child: --case INDEX)"""
import ctypes as C
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

CASES = [(60, 44100, 2, "f32"), (600, 44100, 2, "f32"), (60, 48000, 1, "s16"), (600, 48000, 1, "s16")]
STEP_LIMIT_S = 240
REPEATS = 5


def frames_of(seconds, rate, channels, fmt):
    rng = np.random.default_rng(3)
    t = np.arange(seconds * rate) / rate
    cols = [0.4 * np.sin(2 * np.pi * (180 + 90 * c) * t) + 0.05 * rng.standard_normal(t.shape[0]) for c in range(channels)]
    x = np.stack(cols, axis=1)
    return (x * 32767).astype(np.int16) if fmt == "s16" else x.astype(np.float32)


def step(index: int):
    from whisperlive_amd import _lib
    from whisperlive_amd.audio_io import frames_to_mono
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    seconds, rate, channels, fmt = CASES[index]
    x = frames_of(seconds, rate, channels, fmt)
    spec = SPECS["tiny.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = eng.create_slot(1, 5)
    lib = _lib.load()
    n_out = seconds * 16000
    out = np.zeros(n_out, np.float32)
    kern, dev_wall, host_cpu, host_up = [], [], [], []
    for i in range(REPEATS + 1):                 # the first pass warms up (tap design, staging buffers, buffer growth)
        ms, n = C.c_float(0), C.c_int64(0)
        _lib.check(lib.wlx_debug_resample_timed(0, x.ctypes.data_as(C.c_void_p), x.shape[0], channels, 1 if fmt == "s16" else 0, rate, 0,
                                                out.ctypes.data_as(C.POINTER(C.c_float)), n_out, C.byref(n), C.byref(ms)))
        t0 = time.perf_counter()
        slot.put_frames(x, rate)
        got = slot.pcm()
        t1 = time.perf_counter()
        mono = frames_to_mono(x, rate)
        t2 = time.perf_counter()
        slot.pcm_put(mono)
        t3 = time.perf_counter()
        assert got.shape == mono.shape and float(np.abs(got - mono).max()) < 1e-5
        if i:
            kern.append(ms.value); dev_wall.append(1e3 * (t1 - t0)); host_cpu.append(1e3 * (t2 - t1)); host_up.append(1e3 * (t3 - t2))
    slot.close()
    eng.close()
    med = np.median
    print(f"{seconds:4d} s  {rate} Hz x {channels} {fmt} ({x.nbytes / 1e6:7.1f} MB): device route kernel {med(kern):8.3f} ms, put_frames + pcm() "
          f"{med(dev_wall):8.1f} ms wall | host route mean + resample_poly {med(host_cpu):8.1f} ms + upload {med(host_up):6.1f} ms = "
          f"{med(host_cpu) + med(host_up):8.1f} ms wall   (p50 of {REPEATS})", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        step(int(sys.argv[sys.argv.index("--case") + 1]))
        sys.exit(0)
    print("file audio -> 16 kHz mono float32 resident in the slot: device route (csrc/resample.hip) against host route (scipy, one thread)")
    for i in range(len(CASES)):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--case", str(i)]).returncode
        if rc != 0:
            print(f"case {i} ended with status {rc}: stopping")
            sys.exit(rc)
