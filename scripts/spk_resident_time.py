"""Timing of speaker labelling from device-resident audio (wlx_spk_embed_pcm_batch) against the route it replaces on the file
endpoint: decode the file a second time (audio_io.load_audio: host float64 resample_poly) and upload every segment
(identify_speakers -> wlx_spk_embed_batch). One synthetic file of 10 minutes at 44.1 kHz stereo, about 100 segments of 1 to 8 s,
WeSpeaker ResNet34 shape with seeded weights. Two figures:
  wall    labelling the file's segments, p50 of CALLS runs of each route (the resident route starts from the audio the transcription
          left in the slot, which is where the endpoint finds it; the put_frames that put it there is printed for scale);
  device  filterbank + network of every pass (one pass per group of plan_embed_groups) from the engine's HIP events, resident against
          wlx_spk_embed_batch on the same samples, p50 of CALLS per group, summed over the groups.
Writes profiles/spk_resident_time.txt (or --out PATH). Exit status 3 when the rows differ from the upload route's bits or the resident
passes take more than 1.5 % longer on the device than the uploaded ones.
usage: python scripts/spk_resident_time.py [--out PATH] [--minutes M]"""
import io
import sys
import time
import wave

import numpy as np

sys.path.insert(0, ".")
from whisperlive_amd import audio_io, spk_weights  # noqa: E402
from whisperlive_amd.specs import SPECS  # noqa: E402
from whisperlive_amd.synthetic import speech_like_pcm  # noqa: E402

CALLS = 7
SPREAD = 0.015              # box-to-box spread of a device time


def synthetic_file(minutes: float) -> bytes:
    """44.1 kHz stereo S16 WAV: seeded speech-like audio, the second channel a delayed, quieter copy"""
    base = speech_like_pcm(60.0 * minutes, seed=3)
    n = int(len(base) * 44100 / 16000)
    left = np.interp(np.arange(n) * (16000 / 44100), np.arange(len(base)), base)
    frames = np.stack([left, 0.6 * np.roll(left, 40)], axis=1)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes((np.clip(frames, -1, 1) * 32767).astype(np.int16).tobytes())
    return buf.getvalue()


def segments_of(n_samples: int, seed: int = 4):
    """(start, n) in samples: 1 to 8 s each with 0.2 to 2 s between them, until the file ends"""
    rng = np.random.default_rng(seed)
    out, at = [], 0
    while True:
        at += int(rng.uniform(0.2, 2.0) * 16000)
        n = int(rng.uniform(1.0, 8.0) * 16000)
        if at + n > n_samples:
            return out
        out.append((at, n))
        at += n


def p50_wall(call):
    call()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/spk_resident_time.txt"
    minutes = float(sys.argv[sys.argv.index("--minutes") + 1]) if "--minutes" in sys.argv else 10.0
    from whisperlive_amd.diarization import SpeakerDiarizer, SpeakerEmbedderHIP, plan_embed_groups
    from whisperlive_amd.engine import HipWhisperEngine, ResidentPcm
    from whisperlive_amd.weights import random_weights
    spec = spk_weights.RESNET34
    spk = SpeakerEmbedderHIP(spec, spk_weights.fold(spk_weights.random_weights(spec, seed=0), spec), device=0)
    eng = HipWhisperEngine(SPECS["tiny.en"], random_weights(SPECS["tiny.en"], seed=7))
    slot = eng.create_slot(1, 5)
    data = synthetic_file(minutes)
    frames, rate = audio_io.read_audio(data)
    t0 = time.perf_counter()
    n = slot.put_frames(frames, rate)
    eng.lib.wlx_sync(eng._h, slot.sid)
    put_ms = 1e3 * (time.perf_counter() - t0)
    resident = ResidentPcm(slot, 0, n)
    ranges = segments_of(n)
    device_pcm = slot.pcm()

    # ---- the bits: every resident row against the upload route on the samples the device holds
    rows = spk.embed_resident(slot, 0, ranges)
    want = spk.embed_many([device_pcm[a:a + c] for a, c in ranges])
    same = all((r.view(np.uint32) == w.view(np.uint32)).all() for r, w in zip(rows, want))

    # ---- wall time of labelling the file
    def parent_route():
        audio = audio_io.load_audio(data)
        d = SpeakerDiarizer(embedder=spk)
        return d.identify_speakers([audio[a:min(len(audio), a + c)] for a, c in ranges])

    def resident_route():
        return SpeakerDiarizer(embedder=spk).identify_speakers_resident(resident, ranges)

    t0 = time.perf_counter()
    audio_io.load_audio(data)
    load_ms = 1e3 * (time.perf_counter() - t0)
    wall_parent, wall_resident = p50_wall(parent_route), p50_wall(resident_route)

    # ---- device time per pass, group by group, the two routes alternating
    cap = spec.max_seconds * 16000
    groups = plan_embed_groups([c for _, c in ranges], cap)
    dev_up, dev_res = [], []
    for g in groups:
        pcms, rg = [device_pcm[ranges[i][0]:ranges[i][0] + ranges[i][1]] for i in g], [ranges[i] for i in g]
        up, res = [], []
        for k in range(CALLS + 2):
            spk.embed_many(pcms)
            u = sum(spk.timings())
            spk.embed_resident(slot, 0, rg)
            r = sum(spk.timings())
            if k >= 2:
                up.append(u), res.append(r)
        dev_up.append(float(np.median(up))), dev_res.append(float(np.median(res)))
    up_ms, res_ms = sum(dev_up), sum(dev_res)
    worst = max(r / u for r, u in zip(dev_res, dev_up))
    seconds = sum(c for _, c in ranges) / 16000.0
    lines = [
        "speaker labels of one file from device-resident audio (wlx_spk_embed_pcm_batch) against a second decode + upload "
        "(load_audio + identify_speakers -> wlx_spk_embed_batch): WeSpeaker ResNet34 shape, seeded weights",
        f"file: {minutes:.0f} min at 44.1 kHz stereo S16 -> {n} samples resident (put_frames + wait {put_ms:.1f} ms, part of the transcription); "
        f"{len(ranges)} segments of 1..8 s, {seconds:.0f} s in all, {len(groups)} passes",
        f"wall, p50 of {CALLS}: second decode + upload route {wall_parent:.1f} ms (load_audio alone, first call, {load_ms:.1f} ms) | resident route "
        f"{wall_resident:.1f} ms | {wall_parent / wall_resident:.2f}x",
        f"device (filterbank + network, HIP events), p50 of {CALLS} per pass, summed over {len(groups)} passes: wlx_spk_embed_batch {up_ms:.3f} ms | "
        f"wlx_spk_embed_pcm_batch {res_ms:.3f} ms | resident / upload {res_ms / up_ms:.4f} (worst pass {worst:.4f}; bound {1 + SPREAD:.3f})",
        f"rows bit-identical to the upload route on the same samples: {same}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    slot.close(); eng.close(); spk.close()
    return 0 if same and res_ms <= (1 + SPREAD) * up_ms else 3


if __name__ == "__main__":
    sys.exit(main())
