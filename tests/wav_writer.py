"""Writers of the telephony WAVE formats for the tests: G.711 mu-law / A-law (tags 7 / 6), IMA / DVI ADPCM (0x11), Microsoft ADPCM (0x02).
The tests pin the DECODE (golden recordings, known-answer blocks, the host oracle against the device); these encoders only have to
write valid files whose decode resembles the input. `random_adpcm` writes files of seeded random nibbles behind valid block headers:
every nibble pattern is a valid stream, and it reaches clamps a well-behaved encoder never would."""
import struct

import numpy as np

TAG_MS, TAG_ALAW, TAG_MULAW, TAG_IMA = 0x02, 0x06, 0x07, 0x11
IMA_STEPS = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130,
             143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282,
             1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630,
             9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767]
IMA_INDEX = [-1, -1, -1, -1, 2, 4, 6, 8] * 2
MS_ADAPT = [230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230]
MS_COEFS = [(256, 0), (512, -256), (0, 0), (192, 64), (240, 0), (460, -208), (392, -232)]


def ima_samples_per_block(block_align, ch):
    return (block_align - 4 * ch) * 2 // ch + 1


def ms_samples_per_block(block_align, ch):
    return (block_align - 7 * ch) * 2 // ch + 2


def container(tag, ch, rate, bits, block_align, data, fmt_extra=b"", fact=None, extensible=False, junk=False):
    """RIFF/WAVE around `data`. fmt_extra: the bytes behind the 16 fixed ones (cbSize and the format's extension); fact: a sample count
    for a `fact` chunk; extensible: WAVE_FORMAT_EXTENSIBLE with the tag in the GUID; junk: an odd-sized chunk in front of `fmt `."""
    avg = rate * block_align // max(1, (ima_samples_per_block(block_align, ch) if tag == TAG_IMA else
                                        ms_samples_per_block(block_align, ch) if tag == TAG_MS else 1))
    if extensible:
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHH", 0xFFFE, ch, rate, avg, block_align, bits) + struct.pack("<HHI", 22, bits, 0) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, avg, block_align, bits) + fmt_extra
    chunks = b""
    if junk:
        chunks += b"JUNK" + struct.pack("<I", 3) + b"abc" + b"\0"
    chunks += b"fmt " + struct.pack("<I", len(fmt)) + fmt + (b"\0" if len(fmt) & 1 else b"")
    if fact is not None:
        chunks += b"fact" + struct.pack("<II", 4, fact)
    chunks += b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


# ------------------------------------------------------------------------------------------------ G.711
def _mulaw_value(b):
    u = ~b & 255
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return 132 - t if u & 128 else t - 132


def _alaw_value(b):
    a = (b ^ 0x55) & 255
    s = (a >> 4) & 7
    t = (a & 15) << 4
    t = t + 8 if s == 0 else (t + 0x108) << (s - 1)
    return t if a & 128 else -t


def g711_encode(pcm, tag):
    """int16 array -> the code bytes whose linear value is nearest"""
    vals = np.array([(_mulaw_value if tag == TAG_MULAW else _alaw_value)(b) for b in range(256)], np.int64)
    order = np.argsort(vals, kind="stable")
    sv = vals[order]
    x = np.asarray(pcm, np.int64).ravel()
    hi = np.clip(np.searchsorted(sv, x), 1, 255)
    pick = np.where(np.abs(sv[hi] - x) < np.abs(sv[hi - 1] - x), hi, hi - 1)
    return order[pick].astype(np.uint8)


def write_g711(pcm, rate, tag, extensible=False, fact=None, junk=False):
    """pcm: int16 [n, ch]"""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    ch = pcm.shape[1]
    data = g711_encode(pcm, tag).tobytes()
    return container(tag, ch, rate, 8, ch, data, fmt_extra=b"" if extensible else struct.pack("<H", 0), fact=fact, extensible=extensible, junk=junk)


# ------------------------------------------------------------------------------------------------ IMA ADPCM
def _ima_encode_channel(x, spb, index=0):
    """one channel -> [(predictor, index, [nibbles])] per block"""
    blocks = []
    for at in range(0, len(x), spb):
        seg = x[at:at + spb]
        pred = int(seg[0])
        head = (pred, index)
        nibs = []
        for v in seg[1:]:
            step = IMA_STEPS[index]
            d = int(v) - pred
            nib = 8 if d < 0 else 0
            d = abs(d)
            if d >= step:
                nib |= 4; d -= step
            if d >= step >> 1:
                nib |= 2; d -= step >> 1
            if d >= step >> 2:
                nib |= 1
            diff = (step >> 3) + ((step >> 2) if nib & 1 else 0) + ((step >> 1) if nib & 2 else 0) + (step if nib & 4 else 0)
            pred = max(-32768, min(32767, pred - diff if nib & 8 else pred + diff))
            index = max(0, min(88, index + IMA_INDEX[nib]))
            nibs.append(nib)
        nibs += [0] * (spb - 1 - len(nibs))
        blocks.append((head, nibs))
    return blocks


def ima_pack(heads, nibs, ch):
    """heads: [ch] of (predictor, index); nibs: [ch] lists of (spb - 1) nibbles -> one block's bytes"""
    out = bytearray()
    for c in range(ch):
        out += struct.pack("<hBB", heads[c][0], heads[c][1], 0)
    words = len(nibs[0]) // 8
    for w in range(words):
        for c in range(ch):
            n = nibs[c][8 * w: 8 * w + 8]
            out += bytes(n[2 * i] | (n[2 * i + 1] << 4) for i in range(4))
    return bytes(out)


def write_ima(pcm, rate, block_align=256, fact=None, partial=0, extensible=False):
    """pcm: int16 [n, ch] -> IMA ADPCM WAV; the last block is padded with zero nibbles. fact: True = the real sample count, an int =
    that count, None = no chunk; partial: bytes of a trailing partial block appended to the data chunk"""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    n, ch = pcm.shape
    spb = ima_samples_per_block(block_align, ch)
    per = [_ima_encode_channel(pcm[:, c].tolist(), spb) for c in range(ch)]
    data = b"".join(ima_pack([per[c][k][0] for c in range(ch)], [per[c][k][1] for c in range(ch)], ch) for k in range(len(per[0])))
    data += bytes((37 * i + 11) & 255 for i in range(partial))
    return container(TAG_IMA, ch, rate, 4, block_align, data, fmt_extra=struct.pack("<HH", 2, spb),
                     fact=n if fact is True else fact, extensible=extensible)


# ------------------------------------------------------------------------------------------------ MS ADPCM
def _ms_encode_channel(x, spb, coefs, pi):
    blocks = []
    c1, c2 = coefs[pi]
    for at in range(0, len(x), spb):
        seg = [int(v) for v in x[at:at + spb]]
        seg += [seg[-1]] * (2 - len(seg)) if len(seg) < 2 else []
        s2, s1 = seg[0], seg[1]
        delta = max(16, abs(s1 - s2) // 2)
        head = (pi, min(delta, 32767), s1, s2)
        delta = head[1]
        nibs = []
        for v in seg[2:]:
            pred = (s1 * c1 + s2 * c2) >> 8
            q = max(-8, min(7, int(round((v - pred) / delta))))
            nib = q & 15
            new = max(-32768, min(32767, pred + q * delta))
            delta = max(16, (MS_ADAPT[nib] * delta) >> 8)
            s2, s1 = s1, new
            nibs.append(nib)
        nibs += [0] * (spb - 2 - len(nibs))
        blocks.append((head, nibs))
    return blocks


def ms_pack(heads, nibs, ch, block_align):
    """heads: [ch] of (predictor index, delta, sample1, sample2); nibs: [ch] lists of (spb - 2) nibbles -> one block's bytes"""
    out = bytearray(bytes(h[0] for h in heads))
    for f in (1, 2, 3):
        for c in range(ch):
            out += struct.pack("<h", heads[c][f])
    flat = [nibs[c][i] for i in range(len(nibs[0])) for c in range(ch)]
    flat += [0] * (len(flat) & 1)
    out += bytes((flat[i] << 4) | flat[i + 1] for i in range(0, len(flat), 2))
    assert len(out) == block_align, (len(out), block_align)
    return bytes(out)


def ms_fmt_extra(spb, coefs):
    if coefs is None:
        return struct.pack("<H", 0)              # no extension: the decoder falls back to the 7 standard pairs
    return struct.pack("<HHH", 4 + 4 * len(coefs), spb, len(coefs)) + b"".join(struct.pack("<hh", a, b) for a, b in coefs)


def write_ms(pcm, rate, block_align=256, coefs=MS_COEFS, fact=None, partial=0, predictors=None, omit_extension=False):
    """pcm: int16 [n, ch] -> MS ADPCM WAV. coefs: the fmt chunk's pairs; predictors: the predictor index each channel uses (default:
    channel c uses c mod len(coefs)); omit_extension: write no coefficient table (the 7 standard pairs then hold)"""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    n, ch = pcm.shape
    spb = ms_samples_per_block(block_align, ch)
    predictors = predictors or [c % len(coefs) for c in range(ch)]
    per = [_ms_encode_channel(pcm[:, c].tolist(), spb, coefs, predictors[c]) for c in range(ch)]
    data = b"".join(ms_pack([per[c][k][0] for c in range(ch)], [per[c][k][1] for c in range(ch)], ch, block_align) for k in range(len(per[0])))
    data += bytes((37 * i + 11) & 255 for i in range(partial))
    return container(TAG_MS, ch, rate, 4, block_align, data, fmt_extra=ms_fmt_extra(spb, None if omit_extension else coefs),
                     fact=n if fact is True else fact)


# ------------------------------------------------------------------------------------------------ random streams
def random_adpcm(tag, n_blocks, ch, block_align, rate=8000, seed=0, coefs=MS_COEFS, fact=None, partial=0):
    """A file of `n_blocks` blocks of seeded random bytes behind VALID block headers (IMA: step index 0..88; MS: predictor index inside
    `coefs`, delta 16..2000)."""
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 256, size=(n_blocks, block_align)).astype(np.uint8)
    if tag == TAG_IMA:
        spb = ima_samples_per_block(block_align, ch)
        for c in range(ch):
            blocks[:, 4 * c + 2] = rng.randint(0, 89, size=n_blocks)
            blocks[:, 4 * c + 3] = 0
        extra = struct.pack("<HH", 2, spb)
    else:
        spb = ms_samples_per_block(block_align, ch)
        blocks[:, :ch] = rng.randint(0, len(coefs), size=(n_blocks, ch))
        blocks[:, ch:3 * ch] = rng.randint(16, 2000, size=(n_blocks, ch)).astype("<i2").view(np.uint8).reshape(n_blocks, 2 * ch)
        extra = ms_fmt_extra(spb, coefs)
    data = blocks.tobytes() + bytes((37 * i + 11) & 255 for i in range(partial))
    return container(tag, ch, rate, 4, block_align, data, fmt_extra=extra, fact=fact)


def speech_like(n, ch, seed=0, rate=8000):
    """int16 [n, ch]: a few drifting tones per channel under an envelope, different per channel"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / rate
    out = np.zeros((n, ch))
    for c in range(ch):
        for _ in range(4):
            f, a, ph = rng.uniform(120, 0.4 * rate / 2), rng.uniform(0.05, 0.25), rng.uniform(0, 6.28)
            out[:, c] += a * np.sin(2 * np.pi * f * t + ph) * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(0.5, 3) * t))
        out[:, c] += 0.01 * rng.randn(n)
    return np.clip(np.round(out * 20000), -32768, 32767).astype(np.int16)
