"""Timing of the batched VAD gate (wlx_vad_probs_batch) against the same audios through wlx_vad_probs one by one, and of the batch
worker's front half built on it (WhisperModelHIP.encode_audio_batch_gated: one upload per request, one pass of the gate, features cut
out of the resident PCM, one encoder chain) against the host-gate loop plus encode_audio_batch. Silero shapes with seeded
energy-following weights, Whisper tiny.en shape with seeded weights. Device time is the gate's own HIP-event time (device_ms_out);
wall time is the host clock around calls that return with the device idle (the gate waits for its stream; the front halves end in a
slot synchronise). The two sides of every comparison alternate in one process; p50 of CALLS rounds after WARMUP.
Shapes: 4, 8, 16 and 64 items of 30 s, and a ragged set of 8 items from 1 to 30 s. Every shape is a child process under its own time
limit; the first one that fails ends the run. Writes profiles/vad_batch_time.txt (or --out PATH).
usage: python scripts/vad_batch_time.py [--out PATH]      (child: --shape NAME)"""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd.synthetic import energy_following_vad_weights, speech_like_pcm  # noqa: E402

RAGGED_S = (1.0, 30.0, 2.5, 11.0, 4.0, 19.5, 7.0, 26.0)
SHAPES = {"4x30s": (30.0,) * 4, "8x30s": (30.0,) * 8, "16x30s": (30.0,) * 16, "64x30s": (30.0,) * 64, "ragged8": RAGGED_S}
WARMUP, CALLS = 3, 15
STEP_LIMIT_S = 240


def alternate(a, b):
    """a() and b() return their device milliseconds (or None): -> ((p50 device, p50 wall) of a, the same of b), taken in alternation"""
    res = {a: ([], []), b: ([], [])}
    for r in range(WARMUP + CALLS):
        for f in (a, b):
            t0 = time.perf_counter()
            dev = f()
            wall = 1e3 * (time.perf_counter() - t0)
            if r >= WARMUP:
                res[f][0].append(dev if dev is not None else float("nan"))
                res[f][1].append(wall)
    return tuple((float(np.median(res[f][0])), float(np.median(res[f][1]))) for f in (a, b))


def shape_step(name: str):
    from whisperlive_amd import vad
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights
    secs = SHAPES[name]
    base = [speech_like_pcm(30.0, seed=5 + i) for i in range(4)]                      # 30 s takes a while to synthesise: four, rotated
    audios = [np.roll(base[i % 4], 1600 * i)[: int(s * 16000)].copy() for i, s in enumerate(secs)]
    vm = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)

    def batch():
        vm.probs_many(audios)
        return vm.last_device_ms

    def serial():                       # what the worker's loop pays: np.pad copy + one call per audio
        total = 0.0
        for x in audios:
            vm(np.pad(x, (0, vad.WINDOW - x.shape[0] % vad.WINDOW)))
            total += vm.last_device_ms
        return total
    rows = vm.probs_many(audios)
    same = all(np.array_equal(r.view(np.uint32), vm(np.pad(x, (0, vad.WINDOW - x.shape[0] % vad.WINDOW))).view(np.uint32))
               for r, x in zip(rows, audios))
    (b_dev, b_wall), (s_dev, s_wall) = alternate(batch, serial)
    print(f"{name}: gate  batch {b_dev:.3f} ms device ({b_wall:.3f} ms wall) | one by one {s_dev:.3f} ms device ({s_wall:.3f} ms wall) | "
          f"one by one / batch {s_dev / b_dev:.2f}x device, {s_wall / b_wall:.2f}x wall | rows bit-identical to single calls: {same}", flush=True)

    spec = SPECS["tiny.en"]
    hip = WhisperModelHIP("rand", weights=random_weights(spec, seed=7), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab),
                          max_batch=len(audios), vad_model=vm)
    opts = [vad.VadOptions(min_silence_duration_ms=500)] * len(audios)     # (the synthetic pauses are 1 s: the default 2 s would cut nothing)
    slot = hip._slot()

    def gated():
        assert hip.encode_audio_batch_gated(audios, opts) is not None
        slot.timings()                  # waits for the encoder

    def host():
        kept = []
        for x, o in zip(audios, opts):
            chunks = vad.get_speech_timestamps(x, o, model=vm)
            kept.append(np.concatenate(vad.collect_chunks(x, chunks)[0]) if chunks else x)
        hip.encode_audio_batch(kept)
        slot.timings()
        return None
    _, counts = hip.encode_audio_batch_gated(audios, opts)
    (_, g_wall), (_, h_wall) = alternate(gated, host)
    print(f"{name}: front half (gate + log-mel + tiny.en encoder)  batched {g_wall:.3f} ms wall | host gate loop + encode_audio_batch "
          f"{h_wall:.3f} ms wall | {h_wall / g_wall:.2f}x | samples kept {sum(counts)} of {sum(x.shape[0] for x in audios)}", flush=True)
    hip.close()
    hip.engine.close()
    vm.close()
    return 0 if same else 3


if __name__ == "__main__":
    if "--shape" in sys.argv:
        sys.exit(shape_step(sys.argv[sys.argv.index("--shape") + 1]))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/vad_batch_time.txt"
    lines = ["wlx_vad_probs_batch against wlx_vad_probs one by one, and the batch worker's front half with and without it: Silero shapes, "
             f"seeded weights, p50 of {CALLS} alternating rounds after {WARMUP} warm-up rounds"]
    status = 0
    for name in SHAPES:
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, sys.argv[0], "--shape", name],
                              capture_output=True, text=True)
        sys.stderr.write(proc.stderr[-2000:])
        lines += [ln for ln in proc.stdout.splitlines() if ln.strip()]
        if proc.returncode not in (0, 3):
            lines.append(f"shape {name} ended with status {proc.returncode}: stopping")
            status = proc.returncode
            break
        status = status or proc.returncode
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)
    sys.exit(status)
