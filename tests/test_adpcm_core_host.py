"""CPU: csrc/adpcm_core.h — the block decoders the device runs one lane per (block, channel) — compiled as ordinary host C++ into a
stand-alone program (tests/adpcm_core_check.cpp, its own main) with AddressSanitizer and UndefinedBehaviorSanitizer, run as a child
process. Nothing is loaded into Python under a sanitizer.
1. Every block of the matrix (IMA and MS; 1, 2 and 8 channels; the smallest block sizes, 256 bytes, 4096 bytes with 8 channels; the
   audioop recording; encoded speech-like audio and seeded random nibbles) decodes to exactly the host oracle's samples
   (audio_io._ima_adpcm_blocks / _ms_adpcm_blocks, themselves pinned by tests/test_wav_telephony_host.py).
2. A few thousand seeded CORRUPTIONS of the small blocks: bytes overwritten anywhere, the header included. Any byte pattern is a valid
   block unless it breaks a header index; then the oracle raises, the core clamps, and the record is run for the sanitizers alone.
   Otherwise the core must give the oracle's samples. Buffers are heap blocks of exactly the stated size."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from whisperlive_amd import audio_io

from . import wav_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
N_CORRUPT = 3000
CUSTOM = [(128, 64), (300, -100), (-20, 250)]


def _oracle(kind, ch, block, coefs):
    b = np.frombuffer(block, np.uint8).reshape(1, -1)
    try:
        x = audio_io._ima_adpcm_blocks(b, ch) if kind == 0 else audio_io._ms_adpcm_blocks(b, ch, coefs)
    except ValueError:
        return None
    return x[0]


def _record(kind, ch, block, coefs):
    ba = len(block)
    want = (W.ima_samples_per_block if kind == 0 else W.ms_samples_per_block)(ba, ch)
    x = _oracle(kind, ch, block, coefs)
    must = 1 if x is not None else 2
    expect = x if x is not None else np.zeros((want, ch), np.int16)
    cf = b"".join(struct.pack("<hh", a, b) for a, b in coefs) if kind == 1 else b""
    return struct.pack("<6i", kind, ch, ba, want, len(coefs) if kind == 1 else 0, must) + cf + block + expect.astype("<i2").tobytes(), must


def _blocks(data):
    info = audio_io.wav_probe(data)
    body = data[info.data_offset: info.data_offset + info.data_bytes]
    return [body[k * info.block_align: (k + 1) * info.block_align] for k in range(len(body) // info.block_align)]


def _matrix():
    out = []
    for ch, ima_ba, ms_ba in ((1, 36, 32), (2, 72, 32), (1, 256, 256), (2, 256, 256), (8, 4096, 4096), (3, 60, 33), (1, 4, 7), (2, 8, 14)):
        for k, blk in enumerate(_blocks(W.random_adpcm(W.TAG_IMA, 3, ch, ima_ba, seed=ch))):
            out.append((0, ch, blk, W.MS_COEFS))
        for coefs in (W.MS_COEFS, CUSTOM):
            for blk in _blocks(W.random_adpcm(W.TAG_MS, 3, ch, ms_ba, seed=ch + 10, coefs=coefs)):
                out.append((1, ch, blk, coefs))
    pcm = W.speech_like(1500, 2, seed=4)
    out += [(0, 2, blk, W.MS_COEFS) for blk in _blocks(W.write_ima(pcm, 8000, 256))]
    out += [(1, 2, blk, W.MS_COEFS) for blk in _blocks(W.write_ms(pcm, 8000, 256))]
    gold = np.load(os.path.join(HERE, "golden", "adpcm_golden.npz"))
    out += [(0, 1, W.ima_pack([(int(p), int(i))], [n.tolist()], 1), W.MS_COEFS)
            for p, i, n in zip(gold["ima_pred"], gold["ima_index"], gold["ima_nibbles"])]
    return out


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_core_decodes_the_matrix_and_survives_corruptions_under_the_sanitizers(tmp_path):
    exe = tmp_path / "adpcm_core_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "adpcm_core_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    matrix = _matrix()
    recs = [_record(*m) for m in matrix]
    assert all(must == 1 for _r, must in recs)
    small = [m for m in matrix if len(m[2]) <= 256]
    rng = np.random.RandomState(11)
    n_checked = 0
    for i in range(N_CORRUPT):
        kind, ch, blk, coefs = small[rng.randint(len(small))]
        b = bytearray(blk)
        hdr = (4 if kind == 0 else 7) * ch
        for _ in range(1 + rng.randint(4)):
            at = rng.randint(hdr) if rng.randint(2) == 0 else rng.randint(len(b))       # half of the hits inside the header
            b[at] = rng.randint(256) if rng.randint(4) else (0xFF, 0x80, 0x7F, 0x00)[rng.randint(4)]
        rec = _record(kind, ch, bytes(b), coefs)
        n_checked += rec[1] == 1
        recs.append(rec)
    assert n_checked > N_CORRUPT // 4 and n_checked < N_CORRUPT        # both kinds of record occur
    path = tmp_path / "records.bin"
    path.write_bytes(struct.pack("<i", len(recs)) + b"".join(r for r, _m in recs))
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr[-3000:])
    assert run.returncode == 0, (run.stdout, run.stderr[-3000:])
    assert f"records {len(matrix) + N_CORRUPT} wrong 0 short 0 " in run.stdout
