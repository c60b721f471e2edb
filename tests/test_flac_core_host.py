"""CPU: csrc/flac_core.h — the frame decoder the device runs one lane per frame — compiled as ordinary host C++ into a stand-alone program
(tests/flac_core_check.cpp, its own main) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a child process.
1. Every frame of the matrix (tests/flac_cases.py) decodes to exactly the integers the writer was given.
2. A few thousand seeded CORRUPTIONS of the small frames, CRC-16 recomputed so that nothing in front of the decoder would stop them:
   bit flips in the subframe headers, the residual method / partition order / Rice parameter fields, inside the unary runs and in the
   raw fields. For every one the core must return a non-ok status or the RIGHT samples, and the sanitizers must stay silent. A flipped
   bit in a raw sample or in the binary part of a Rice symbol is simply another valid frame, so "right" is what the MD5-pinned oracle
   decoder (audio_io.read_flac, MD5 check off) makes of the same bytes: where the oracle decodes the frame, status ok is allowed only
   with the oracle's samples; where the oracle raises, only a non-ok status is. The oracle computes in unbounded integers: a frame
   whose oracle decode leaves int32 has no right answer in the decoder's sample type and is run for the sanitizers alone.
   This is where malformed-but-CRC-valid frames are exercised — on the CPU, never on a device."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from . import flac_cases as FC
from . import flac_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
N_CORRUPT = 3000


def _record(bps, pcm, frame, must):
    n, ch = pcm.shape
    return struct.pack("<5i", bps, ch, n, len(frame), must) + frame + pcm.astype("<i4").tobytes()


def _header_len(frame):
    """the header's bytes: 4 fixed, the coded number, the size / rate extras, the CRC-8 — found by the CRC-8 that matches"""
    for ln in range(6, 17):
        if W.crc8(frame[:ln - 1]) == frame[ln - 1]:
            return ln
    raise AssertionError("no header")


def _corruptions(rng):
    small = [c for c in FC.cases() if max(c["blocks"]) <= 300]
    pool = []
    for c in small:
        pos = 0
        for fr, n in zip(c["frames"], c["blocks"]):
            pool.append((c["bps"], c["pcm"][pos:pos + n], fr))
            pos += n
    out = []
    for i in range(N_CORRUPT):
        bps, pcm, fr = pool[rng.randint(len(pool))]
        hl = _header_len(fr)
        body_bits = (len(fr) - 2 - hl) * 8
        b = bytearray(fr)
        # a third of the flips in the first subframe's header and residual set-up (type, wasted flag, warm-up, method, partition order,
        # first Rice parameter), the rest anywhere in the subframes (later headers, parameters, unary runs, binary parts)
        flips = 1 + rng.randint(3)
        for _ in range(flips):
            at = rng.randint(min(body_bits, 8 + 6 * bps)) if rng.randint(3) == 0 else rng.randint(body_bits)
            b[hl + (at >> 3)] ^= 0x80 >> (at & 7)
        b[-2:] = W.crc16(bytes(b[:-2])).to_bytes(2, "big")
        want, must = _oracle(bytes(b), bps, pcm)
        out.append(_record(bps, want, bytes(b), must))
    return out


def _oracle(frame, bps, pcm):
    """-> (samples a status-ok decode must give, record kind): 0 = non-ok or these samples; 2 = sanitizers only; 3 = non-ok only"""
    from whisperlive_amd import audio_io
    n, ch = pcm.shape
    info = W.streaminfo(pcm, 16000, bps, n, n, md5=False)
    try:
        x, _ = audio_io.read_flac(W.metadata(info) + frame, verify_md5=False)
    except ValueError as e:
        # the oracle's own findings are rejections; anything else (numpy refusing a shape or an integer of the oracle's arithmetic on
        # a frame it was never meant to see) says nothing about the frame
        return pcm, 3 if any(m in str(e) for m in ("reserved", "padding bit", "runs past the end", "lost FLAC frame sync")) else 2
    except Exception:
        return pcm, 2
    if x.shape != (n, ch):
        return pcm, 3
    got = np.round(x.astype(np.float64) * (1 << (bps - 1)))
    if np.abs(got).max() >= (1 << 24):            # float32 holds 24-bit integers exactly; past that the oracle's own output is rounded
        return pcm, 2
    return got.astype(np.int64), 0


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_core_decodes_the_matrix_and_survives_corruptions_under_the_sanitizers(tmp_path):
    exe = tmp_path / "flac_core_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "flac_core_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    recs = []
    for c in FC.cases():
        pos = 0
        for fr, n in zip(c["frames"], c["blocks"]):
            recs.append(_record(c["bps"], c["pcm"][pos:pos + n], fr, 1))
            pos += n
    n_intact = len(recs)
    recs += _corruptions(np.random.RandomState(7))
    path = tmp_path / "records.bin"
    path.write_bytes(struct.pack("<i", len(recs)) + b"".join(recs))
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr[-3000:])
    assert run.returncode == 0, (run.stdout, run.stderr[-3000:])
    assert f"records {n_intact + N_CORRUPT} intact_bad 0 " in run.stdout and "corrupt_wrong_ok 0 " in run.stdout
