"""Generates tests/golden/jfk_head.flac: the first 32 frames (147 456 samples, 3.34 s) of the reference's assets/jfk.flac,
24-bit stereo 44.1 kHz, byte for byte as the encoder wrote them — only STREAMINFO's total-sample count and MD5 signature are
rewritten for the shorter stream (the whole file is 1.1 MB). The MD5 is taken over samples of a decode that matched the
WHOLE file's own MD5, so the FLAC tests read an encoder's frames (LPC / fixed subframes, Rice residuals, stereo decorrelation)
and a signature the decoder under test did not make up.

Run with a checkout of the reference:  python tests/golden/make_jfk_head_flac.py REFERENCE_ROOT"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from whisperlive_amd import audio_io  # noqa: E402

FRAMES = 32


def main():
    src = os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "assets", "jfk.flac")
    b = bytearray(open(src, "rb").read())
    x, sr = audio_io.read_flac(bytes(b))                   # raises unless the decode matches the whole file's MD5
    pos = 4
    while True:                                            # metadata blocks; STREAMINFO is the first
        last, ln = b[pos] >> 7, int.from_bytes(b[pos + 1:pos + 4], "big")
        pos += 4 + ln
        if last:
            break
    info = 8
    v = int.from_bytes(b[info + 10:info + 18], "big")
    bps = ((v >> 36) & 31) + 1
    block = int.from_bytes(b[info:info + 2], "big")        # min block size == max block size: fixed-size frames
    assert block == int.from_bytes(b[info + 2:info + 4], "big")
    total = FRAMES * block
    # the end of frame FRAMES - 1 = the sync code of frame FRAMES (its one-byte frame number) that the decoder then accepts
    end = next(i for i in range(pos, len(b) - 4) if b[i] == 0xFF and b[i + 1] == 0xF8 and b[i + 4] == FRAMES
               and _decodes(b, i, info, v, total))
    ints = np.round(x[:total].astype(np.float64) * (1 << (bps - 1))).astype("<i8")
    md5 = hashlib.md5(ints.view(np.uint8).reshape(total, x.shape[1], 8)[:, :, :(bps + 7) // 8].tobytes()).digest()
    out = _patched(b, info, v, total)[:end]
    out[info + 18:info + 34] = md5
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jfk_head.flac")
    open(path, "wb").write(bytes(out))
    y, _ = audio_io.read_flac(path)
    assert np.array_equal(y, x[:total])
    print("wrote", path, len(out), "bytes", y.shape)


def _patched(b, info, v, total):
    out = bytearray(b)
    out[info + 10:info + 18] = ((v & ~((1 << 36) - 1)) | total).to_bytes(8, "big")
    return out


def _decodes(b, end, info, v, total):
    try:
        audio_io.read_flac(bytes(_patched(b, info, v, total)[:end]), verify_md5=False)
        return True
    except Exception:  # noqa: BLE001
        return False


if __name__ == "__main__":
    main()
