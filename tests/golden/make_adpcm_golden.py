"""Writes tests/golden/adpcm_golden.npz: an independent pin of the IMA ADPCM nibble arithmetic and of the G.711 tables, recorded from
Python's `audioop` (3.10; the module left the standard library in 3.13, so the tests read the recording, never the module).

ima_pred / ima_index [K]: the state a stream starts from; ima_nibbles [K, N]: seeded nibbles IN TIME ORDER; ima_out [K, N]: what
audioop.adpcm2lin(width 2) decodes them to from that state. audioop takes the HIGH nibble of a byte first, a WAVE file the LOW one:
the recording stores nibbles, not bytes, and each side packs them in its own order.
mulaw / alaw [256]: audioop.ulaw2lin / alaw2lin of every code, width 2.

usage: python tests/golden/make_adpcm_golden.py"""
import audioop
import os

import numpy as np

K, N = 24, 504          # 504 nibbles + the header's sample = one mono block of block_align 256

rng = np.random.RandomState(20240611)
pred = rng.randint(-32768, 32768, size=K).astype(np.int16)
index = rng.randint(0, 89, size=K).astype(np.uint8)
pred[:4] = [0, 32767, -32768, 12345]
index[:4] = [0, 88, 88, 0]
nibbles = rng.randint(0, 16, size=(K, N)).astype(np.uint8)
nibbles[1] = 7           # runs into the upper clamp of the predictor and of the index
nibbles[2] = 15          # ... and the lower one
nibbles[3] = 0           # the index walks down to 0 and stays
out = np.empty((K, N), np.int16)
for k in range(K):
    packed = bytes((int(nibbles[k, 2 * i]) << 4) | int(nibbles[k, 2 * i + 1]) for i in range(N // 2))
    frag, _ = audioop.adpcm2lin(packed, 2, (int(pred[k]), int(index[k])))
    out[k] = np.frombuffer(frag, "<i2")
codes = bytes(range(256))
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "adpcm_golden.npz"),
                    ima_pred=pred, ima_index=index, ima_nibbles=nibbles, ima_out=out,
                    mulaw=np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"), alaw=np.frombuffer(audioop.alaw2lin(codes, 2), "<i2"))
