#!/usr/bin/env python
"""A stereo call recording, one transcript per channel: (a) what a user does without the switch — split the file on the host and call
BatchedInferencePipeline.transcribe once per channel — against (b) ONE call with multichannel=True. scripts/longform_time.py's
conventions: Whisper-small shapes, seeded weights, beam 5, the seeded energy-following gate, exactly --max-new-tokens tokens per
chunk; per case one warm-up run, then the median of --repeats timed runs (wall clock around the whole case, segments consumed), then
one instrumented run that sums the HIP-event stage times.

The file: --minutes (default 10) of 44.1 kHz 16-bit stereo, each channel longform_time.stream_pcm with its own seed resampled to
44.1 kHz, as WAV and as FLAC (tests/flac_writer.py). (a) for the WAV includes the host split (a slice per channel and a mono WAV of
it); (a) is not run for the FLAC: its host split is the Python FLAC decoder, minutes per file, and says nothing about this change.
Reported per row: wall time, bytes uploaded (every put_frames / put_frames_split / pcm_put, file bytes for FLAC), generate calls and
decode steps, stage sums. Last: the device time of the ONE resample launch of put_flac (down-mix) against put_flac_split on the same
file (wlx_debug_flac_timings).
usage: python scripts/multichannel_time.py [--minutes 10] [--batch 8,24] [--repeats 3] [--out FILE]"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wav16(frames: np.ndarray, rate: int) -> bytes:
    x = np.ascontiguousarray(frames, dtype="<i2")
    ch = x.shape[1]
    fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * ch * 2, ch * 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", x.nbytes) + x.tobytes()
    return b"RIFF" + struct.pack("<I", len(body)) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--batch", default="8,24")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--model", default="small.en")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import ctypes as C

    from scipy.signal import resample_poly

    from scripts.longform_time import stream_pcm
    from tests import flac_writer as W
    from whisperlive_amd import engine as E, vad
    from whisperlive_amd.audio_io import read_audio
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.weights import random_weights

    rate = 44100
    chans = [resample_poly(stream_pcm(a.minutes * 60.0, seed).astype(np.float64), 441, 160) for seed in (1234, 4321)]
    q = np.clip(np.round(np.stack(chans, axis=1) * 32767.0), -32768, 32767).astype(np.int16)
    files = {"wav": wav16(q, rate),
             "flac": W.encode_stream(q.astype(np.int64), rate, 16, W.split_blocks(q.shape[0], 4096),
                                     subframe={"type": "fixed", "order": 2, "k": 11}, assignment=W.MID_SIDE)}
    seconds = q.shape[0] / rate
    print(json.dumps({"file_s": round(seconds, 1), "wav_bytes": len(files["wav"]), "flac_bytes": len(files["flac"])}), flush=True)

    spec = SPECS[a.model]
    eng = E.HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    tok = synthetic_tokenizer(spec.vocab)
    rows = []

    uploaded = {"bytes": 0}
    for name in ("put_frames", "put_frames_split", "pcm_put"):
        real = getattr(E.Slot, name)

        def counted(self, frames, *args, _real=real, **kw):
            uploaded["bytes"] += len(frames.data) if isinstance(frames, E.FlacFrames) else np.asarray(frames).nbytes
            return _real(self, frames, *args, **kw)
        setattr(E.Slot, name, counted)

    common = dict(language="en", temperature=0.0, beam_size=5, max_new_tokens=a.max_new_tokens, without_timestamps=True,
                  vad_filter=True)
    for bs in [int(x) for x in a.batch.split(",") if x]:
        hip = WhisperModelHIP(a.model, engine=eng, hf_tokenizer=tok, max_batch=bs + 2, vad_model=gate)
        pipe = BatchedInferencePipeline(hip)
        sup = [-1, hip._base_tokenizer.eot]

        def per_channel(data):
            frames, sr = read_audio(data)                                  # the host split: decode, slice, one mono file per channel
            n = 0
            for c in range(frames.shape[1]):
                segs, _ = pipe.transcribe(wav16(frames[:, c:c + 1], sr), suppress_tokens=sup, batch_size=bs, **common)
                n += len(list(segs))
            return n

        def one_call(data):
            segs, _ = pipe.transcribe(data, suppress_tokens=sup, batch_size=bs, multichannel=True, **common)
            return len(list(segs))

        for fmt, case, run in (("wav", "per_channel_calls", per_channel), ("wav", "multichannel", one_call),
                               ("flac", "multichannel", one_call)):
            data = files[fmt]
            n_seg = run(data)                                              # warm-up: buffers grown, decode graphs captured
            walls = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                run(data)
                walls.append(time.perf_counter() - t0)
            acc = {"logmel_ms": 0.0, "encode_ms": 0.0, "generate_ms": 0.0, "generates": 0, "decode_steps": 0}
            real_gen = hip.model.generate

            def generate(enc, prompts, **kw):
                res = real_gen(enc, prompts, **kw)
                t = enc.slot.timings()
                for k in ("logmel_ms", "encode_ms", "generate_ms", "decode_steps"):
                    acc[k] += t[k]
                acc["generates"] += 1
                return res
            hip.model.generate = generate
            uploaded["bytes"] = 0
            try:
                run(data)
            finally:
                hip.model.generate = real_gen
            wall = float(np.median(walls))
            row = dict(file=fmt, case=case, batch_size=bs, segments=n_seg, wall_s=round(wall, 4), wall_min_s=round(min(walls), 4),
                       wall_max_s=round(max(walls), 4), xRT=round(seconds / wall, 1), uploaded_bytes=uploaded["bytes"],
                       generates=acc["generates"], decode_steps=acc["decode_steps"], logmel_ms=round(acc["logmel_ms"], 2),
                       encode_ms=round(acc["encode_ms"], 2), generate_ms=round(acc["generate_ms"], 2), repeats=a.repeats)
            rows.append(row)
            print(json.dumps(row), flush=True)
        hip.close()

    # the one resample launch over the decoded device frames: down-mix against split (median of 5 each)
    slot = eng.create_slot(3, 5)
    ms = (C.c_float * 5)()
    launch = {}
    for name, put in (("downmix", lambda: slot.put_flac(files["flac"], 0)), ("split", lambda: slot.put_flac_split(files["flac"], 1))):
        put()
        got = []
        for _ in range(5):
            put()
            E.check(eng.lib.wlx_debug_flac_timings(eng._h, slot.sid, ms))
            got.append(float(ms[4]))
        launch[name] = round(float(np.median(got)), 4)
    row = dict(case="resample_launch_ms", file="flac", **launch)
    rows.append(row)
    print(json.dumps(row), flush=True)
    slot.close()
    gate.close()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
