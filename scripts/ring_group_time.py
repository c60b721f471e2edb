"""Per-packet wall time of a live multichannel stream's two routes into per-channel device PCM rings, for three wire shapes:
20 ms mu-law stereo packets at 8 kHz, 4096-frame int16 stereo packets at 48 kHz, 4096-frame float32 8-channel packets at 44.1 kHz.
  group route:     PcmRingGroup.append_frames — the interleaved packet crosses PCIe once, ONE launch of the split stream form fills
                   every lane, the new 16 kHz samples of all lanes come back in one copy and one wait;
  per-ring route:  what a user of the library without ring groups has to do — de-interleave the packet on the host, then one
                   PcmRing.append_frames per channel on C mono rings with a wire format: C uploads, C launches, C waits.
Both routes return the same samples (asserted on the last packet of each case). Wall time per packet, p50 / p95 after the warm-up
packets, over 10 s of audio. Every GPU step is a child process under its own time limit; the first one that fails ends the run.
usage: python scripts/ring_group_time.py [--out profiles/ring_group_time.txt]      (child: --case INDEX)"""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

CASES = [("mulaw", 8000, 2, 160), ("int16", 48000, 2, 4096), ("float32", 44100, 8, 4096)]
SECONDS = 10
WARMUP_PACKETS = 8
STEP_LIMIT_S = 180
HEADER = ("live multichannel packets -> one 16 kHz float32 device PCM ring per channel: ring group (wlx_ring_group_append_frames) against "
          "host de-interleave + one wlx_ring_append_frames per channel; wall time per packet")


def wire_frames(fmt, rate, channels):
    rng = np.random.default_rng(3)
    n = SECONDS * rate
    if fmt == "mulaw":
        return rng.integers(0, 256, (n, channels), dtype=np.uint8)
    t = np.arange(n) / rate
    x = np.stack([0.4 * np.sin(2 * np.pi * (180 + 90 * c) * t) + 0.05 * rng.standard_normal(n) for c in range(channels)], axis=1)
    return (x * 32767).astype(np.int16) if fmt == "int16" else x.astype(np.float32)


def step(index: int):
    from whisperlive_amd import stream_resample as SR
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    fmt, rate, channels, pkt = CASES[index]
    code, dt = SR.WIRE_FORMATS[fmt]
    x = wire_frames(fmt, rate, channels)
    packets = [x[i: i + pkt].tobytes() for i in range(0, x.shape[0], pkt)]
    spec = SPECS["tiny.en"]
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    group = eng.create_ring_group(code, channels, rate)
    rings = [eng.create_ring() for _ in range(channels)]
    for r in rings:
        r.set_format(code, 1, rate)
    group_ms, split_ms, rings_ms, same = [], [], [], True
    for i, raw in enumerate(packets):
        t0 = time.perf_counter()
        new, _d, _b, _r = group.append_frames(raw)
        t1 = time.perf_counter()
        cols = np.ascontiguousarray(np.frombuffer(raw, dtype=dt).reshape(-1, channels).T)      # [channels][n]: the host de-interleave
        t2 = time.perf_counter()
        outs = [rings[c].append_frames(cols[c])[0] for c in range(channels)]
        t3 = time.perf_counter()
        if i >= WARMUP_PACKETS:
            group_ms.append(1e3 * (t1 - t0)); split_ms.append(1e3 * (t2 - t1)); rings_ms.append(1e3 * (t3 - t2))
        if i == len(packets) - 1:
            same = all(np.array_equal(new[c].view(np.uint32), outs[c].view(np.uint32)) for c in range(channels))
    group.close()
    for r in rings:
        r.close()
    eng.close()
    assert same, "the two routes returned different samples"
    q = lambda a, p: float(np.percentile(a, p))
    both = np.add(split_ms, rings_ms)
    print(f"{fmt:8s} {rate:6d} Hz x {channels}, {pkt:4d}-frame packets ({1e3 * pkt / rate:5.1f} ms of audio, {len(group_ms)} timed):\n"
          f"    ring group      one append_frames                         p50 {q(group_ms, 50):7.3f} ms  p95 {q(group_ms, 95):7.3f} ms\n"
          f"    {channels} mono rings    de-interleave {q(split_ms, 50):7.3f} + {channels} x append_frames {q(rings_ms, 50):7.3f} = "
          f"p50 {q(both, 50):7.3f} ms  p95 {q(both, 95):7.3f} ms", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        step(int(sys.argv[sys.argv.index("--case") + 1]))
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/ring_group_time.txt"
    lines = [HEADER]
    for i in range(len(CASES)):
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--case", str(i)],
                           capture_output=True, text=True)
        if p.returncode != 0:
            print(p.stdout, p.stderr[-2000:])
            print(f"case {i} ended with status {p.returncode}: stopping")
            sys.exit(p.returncode)
        lines.append(p.stdout.rstrip("\n"))
    text = "\n".join(ln for block in lines for ln in block.splitlines() if not ln.startswith("[wlx]")) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text, end="")
