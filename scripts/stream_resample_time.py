"""Per-packet wall time of the live path's two routes into the device PCM ring, for three wire shapes:
20 ms mu-law packets at 8 kHz, 4096-frame int16 stereo packets at 48 kHz, 4096-frame float32 mono packets at 44.1 kHz.
  device route: PcmRing.append_frames — the packet crosses PCIe in its wire format, is converted, down-mixed and resampled on the
                device, and its new 16 kHz samples come back for the session's host mirror in the same wait;
  host route:   what a client of a server without wire formats has to do — decode, float32 channel mean and
                scipy.signal.resample_poly of the packet on the host (one CPU thread), then PcmRing.append of the float32 result.
Bytes over PCIe per second of audio are computed from the shapes (host to device / device to host), not measured.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.
usage: python scripts/stream_resample_time.py > profiles/stream_resample_time.txt      (child: --case INDEX)"""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

CASES = [("mulaw", 8000, 1, 160), ("int16", 48000, 2, 4096), ("float32", 44100, 1, 4096)]
SECONDS = 10
WARMUP_PACKETS = 8
STEP_LIMIT_S = 180


def wire_frames(fmt, rate, channels):
    rng = np.random.default_rng(3)
    n = SECONDS * rate
    if fmt == "mulaw":
        return rng.integers(0, 256, (n, channels), dtype=np.uint8)
    t = np.arange(n) / rate
    x = np.stack([0.4 * np.sin(2 * np.pi * (180 + 90 * c) * t) + 0.05 * rng.standard_normal(n) for c in range(channels)], axis=1)
    return (x * 32767).astype(np.int16) if fmt == "int16" else x.astype(np.float32)


def step(index: int):
    from scipy.signal import resample_poly
    from whisperlive_amd import stream_resample as SR
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    fmt, rate, channels, pkt = CASES[index]
    code, dt = SR.WIRE_FORMATS[fmt]
    up, down = SR.ratio(rate)
    x = wire_frames(fmt, rate, channels)
    packets = [x[i: i + pkt].tobytes() for i in range(0, x.shape[0], pkt)]
    spec = SPECS["tiny.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    dev_ring, host_ring = eng.create_ring(), eng.create_ring()
    dev_ring.set_format(code, channels, rate)
    dev_ms, host_cpu_ms, host_up_ms, n_dev, n_host = [], [], [], 0, 0
    for i, raw in enumerate(packets):
        t0 = time.perf_counter()
        new, _d, _b, _r = dev_ring.append_frames(raw)
        t1 = time.perf_counter()
        mono = SR.mono_f32(np.frombuffer(raw, dtype=dt).reshape(-1, channels), code)
        y = resample_poly(mono.astype(np.float64), up, down).astype(np.float32)
        t2 = time.perf_counter()
        host_ring.append(y)
        t3 = time.perf_counter()
        n_dev += new.shape[0]; n_host += y.shape[0]
        if i >= WARMUP_PACKETS:
            dev_ms.append(1e3 * (t1 - t0)); host_cpu_ms.append(1e3 * (t2 - t1)); host_up_ms.append(1e3 * (t3 - t2))
    dev_ring.close(); host_ring.close(); eng.close()
    assert n_dev == SR.stream_count(rate, x.shape[0]) and n_host >= n_dev  # the stream holds back only the filter's look-ahead
    wire_bps = rate * channels * dt.itemsize
    q = lambda a, p: float(np.percentile(a, p))
    print(f"{fmt:8s} {rate:6d} Hz x {channels}, {pkt:4d}-frame packets ({1e3 * pkt / rate:5.1f} ms of audio, {len(dev_ms)} timed):\n"
          f"    device route  append_frames            p50 {q(dev_ms, 50):7.3f} ms  p95 {q(dev_ms, 95):7.3f} ms   "
          f"PCIe {wire_bps:7d} B/s up + 64000 B/s down per second of audio\n"
          f"    host route    resample_poly {q(host_cpu_ms, 50):7.3f} + append {q(host_up_ms, 50):7.3f} = p50 {q(np.add(host_cpu_ms, host_up_ms), 50):7.3f} ms  "
          f"p95 {q(np.add(host_cpu_ms, host_up_ms), 95):7.3f} ms   PCIe   64000 B/s up", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        step(int(sys.argv[sys.argv.index("--case") + 1]))
        sys.exit(0)
    print("live packets -> 16 kHz mono float32 in the device PCM ring: wire-format route (wlx_ring_append_frames) against host "
          "resample + wlx_ring_append; wall time per packet")
    for i in range(len(CASES)):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--case", str(i)]).returncode
        if rc != 0:
            print(f"case {i} ended with status {rc}: stopping")
            sys.exit(rc)
