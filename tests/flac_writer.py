"""A small FLAC WRITER for the tests of the FLAC front end (csrc/flac.hip, csrc/flac_core.h): no encoder is available offline, and a
real encoder never emits most of the legal stream shapes anyway. Nothing here searches for a good encoding: the caller says, per
subframe, which type, predictor (order / coefficients / precision / shift), residual coding (Rice method, partition order, parameters,
escape partitions) and wasted-bits count to use, and per frame which channel assignment; residual = sample - prediction, so ANY
choice gives a lossless stream. STREAMINFO carries the MD5 of the samples, every frame its CRC-8 and CRC-16: audio_io.read_flac
(verify_md5=True) is the oracle the writer is pinned to (tests/test_flac_writer.py).

    encode_stream(pcm [n, channels] ints, rate, bps, blocks=[sizes], subframe=dict | f(frame, channel) -> dict,
                  assignment=int | f(frame) -> int, variable=False, first_number=0) -> bytes

A subframe dict: {"type": "constant" | "verbatim" | "fixed" | "lpc", "order": 0..4 (fixed), "coefs": [...], "precision": 1..15, "shift": 0..15
(lpc), "method": 0 | 1, "porder": partition order, "k": int or one per partition, "escape": {partition: raw width}, "wasted": bits}.
Bit strings are numpy arrays of 0 / 1 (the Rice coder and the raw fields are vectorised, so a ten-minute stream for the timing script is
written in seconds); CRC-16 runs over per-position tables, 4096 bytes at a time.
"""
from __future__ import annotations

import hashlib

import numpy as np

INDEPENDENT, LEFT_SIDE, SIDE_RIGHT, MID_SIDE = 0, 8, 9, 10
FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


# ------------------------------------------------------------------------------------------------------------------ CRCs
def _table(poly: int, width: int) -> np.ndarray:
    t = np.zeros(256, np.int64)
    top, mask = 1 << (width - 1), (1 << width) - 1
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t[i] = c
    return t


_T8 = _table(0x07, 8)
_T16 = _table(0x8005, 16)
_CRC_BLOCK = 4096
_tpos = None            # _tpos[k][i]: CRC-16 of byte i followed by k zero bytes


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = int(_T8[c ^ b])
    return c


def crc16(data) -> int:
    global _tpos
    if _tpos is None:
        t = np.empty((_CRC_BLOCK, 256), np.int64)
        t[0] = _T16
        for k in range(1, _CRC_BLOCK):
            t[k] = ((t[k - 1] << 8) & 0xFFFF) ^ _T16[t[k - 1] >> 8]
        _tpos = t
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    c = 0
    for off in range(0, a.size, _CRC_BLOCK):
        blk = a[off:off + _CRC_BLOCK]
        n = blk.size
        if n == 1:
            c = ((c << 8) & 0xFFFF) ^ int(_T16[c >> 8])
        else:               # the state in front of n bytes = those n bytes with the state folded into the first two
            c = int(_tpos[n - 1][c >> 8] ^ _tpos[n - 2][c & 0xFF])
        c ^= int(np.bitwise_xor.reduce(_tpos[n - 1 - np.arange(n), blk]))
    return c


# ------------------------------------------------------------------------------------------------------------------ bits
def bits(value: int, n: int) -> np.ndarray:
    """the low n bits of `value` (two's complement for a negative one), MSB first"""
    value &= (1 << n) - 1
    return np.array([(value >> (n - 1 - i)) & 1 for i in range(n)], np.uint8)


def bits_of(values, width: int) -> np.ndarray:
    """every value as `width` raw bits (two's complement), concatenated"""
    v = np.asarray(values, np.int64).reshape(-1, 1)
    if width == 0 or v.size == 0:
        return np.zeros(0, np.uint8)
    sh = np.arange(width - 1, -1, -1, dtype=np.int64)
    return ((v >> sh) & 1).astype(np.uint8).reshape(-1)


def unary(n: int) -> np.ndarray:
    out = np.zeros(n + 1, np.uint8)
    out[n] = 1
    return out


def rice_bits(res, k: int) -> np.ndarray:
    r = np.asarray(res, np.int64)
    if r.size == 0:
        return np.zeros(0, np.uint8)
    u = (r << 1) ^ (r >> 63)
    q = u >> k
    lens = q + 1 + k
    ends = np.cumsum(lens)
    starts = ends - lens
    out = np.zeros(int(ends[-1]), np.uint8)
    out[starts + q] = 1
    for j in range(k):
        out[starts + q + 1 + j] = (u >> (k - 1 - j)) & 1
    return out


def pack(parts) -> bytes:
    b = np.concatenate([np.asarray(p, np.uint8) for p in parts]) if parts else np.zeros(0, np.uint8)
    return np.packbits(b).tobytes()          # zero padding to the byte


def utf8_number(v: int) -> bytes:
    """FLAC's UTF-8-style coding of a frame / sample number, up to 36 bits"""
    if v < 0x80:
        return bytes([v])
    for nbytes, limit in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if v < (1 << limit):
            out = [0] * nbytes
            for i in range(nbytes - 1, 0, -1):
                out[i] = 0x80 | (v & 0x3F)
                v >>= 6
            out[0] = ((0xFF << (8 - nbytes)) & 0xFF) | v
            return bytes(out)
    raise ValueError("number over 36 bits")


# ------------------------------------------------------------------------------------------------------------------ subframe
def predict(x: np.ndarray, coefs, shift: int) -> np.ndarray:
    """the predictions of x[order:] from the TRUE samples in front of each"""
    order, n = len(coefs), x.size
    acc = np.zeros(n - order, np.int64)
    for j, c in enumerate(coefs):
        acc += int(c) * x[order - 1 - j: n - 1 - j]
    return acc >> shift


def residual_bits(res: np.ndarray, n: int, order: int, method=0, porder=0, k=0, escape=None) -> list:
    nparts = 1 << porder
    assert porder == 0 or (n % nparts == 0 and (n >> porder) >= order), "illegal partition order"
    ks = list(k) if isinstance(k, (list, tuple)) else [k] * nparts
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    parts = [bits(method, 2), bits(porder, 4)]
    o = 0
    for p in range(nparts):
        cnt = (n >> porder) - (order if p == 0 else 0) if porder else n - order
        seg = res[o:o + cnt]
        o += cnt
        if escape and p in escape:
            w = escape[p]
            assert w == 0 and not seg.any() or w > 0 and (seg.size == 0 or (-(1 << (w - 1)) <= seg.min() and seg.max() < (1 << (w - 1))))
            parts += [bits(esc, pbits), bits(w, 5), bits_of(seg, w)]
        else:
            assert 0 <= ks[p] < esc
            parts += [bits(ks[p], pbits), rice_bits(seg, ks[p])]
    return parts


def subframe_bits(x, bps: int, spec: dict) -> list:
    x = np.asarray(x, np.int64)
    n = x.size
    typ = spec.get("type", "verbatim")
    wasted = int(spec.get("wasted", 0))
    code = {"constant": 0, "verbatim": 1}.get(typ)
    coefs = None
    if typ == "fixed":
        coefs, shift = FIXED[spec["order"]], 0
        code = 8 + spec["order"]
    elif typ == "lpc":
        coefs, shift = list(spec["coefs"]), int(spec["shift"])
        code = 32 + len(coefs) - 1
    parts = [bits(0, 1), bits(code, 6)]
    if wasted:
        assert not (x & ((1 << wasted) - 1)).any(), "samples do not have that many wasted bits"
        x = x >> wasted
        bps -= wasted
        parts += [bits(1, 1), unary(wasted - 1)]
    else:
        parts.append(bits(0, 1))
    assert -(1 << (bps - 1)) <= x.min() and x.max() < (1 << (bps - 1)), "samples do not fit the subframe's width"
    if typ == "constant":
        assert (x == x[0]).all()
        parts.append(bits_of(x[:1], bps))
    elif typ == "verbatim":
        parts.append(bits_of(x, bps))
    else:
        order = len(coefs)
        parts.append(bits_of(x[:order], bps))
        if typ == "lpc":
            prec = int(spec["precision"])
            assert 1 <= prec <= 15 and 0 <= shift <= 15 and all(-(1 << (prec - 1)) <= c < (1 << (prec - 1)) for c in coefs)
            parts += [bits(prec - 1, 4), bits(shift, 5), bits_of(coefs, prec)]
        res = x[order:] - predict(x, coefs, shift) if order else x
        assert res.size == 0 or (-(1 << 31) <= res.min() and res.max() < (1 << 31)), "residual over 32 bits"
        parts += residual_bits(res, n, order, spec.get("method", 0), spec.get("porder", 0), spec.get("k", 0), spec.get("escape"))
    return parts


# ------------------------------------------------------------------------------------------------------------------ frame, stream
def frame_header(n: int, rate: int, channels: int, bps: int, number: int, variable: bool, assignment: int, stream_codes: bool = False,
                 bs_code=None) -> bytes:
    """stream_codes: code rate and width as 0 ("as STREAMINFO"). bs_code: force 6 (8-bit size) or 7 (16-bit size) for a size a table code serves"""
    if bs_code is None:
        bs_code = _BS_CODES.get(n) or (6 if n <= 256 else 7)
    sr_code = 0 if stream_codes else _SR_CODES.get(rate, 0)
    sr_extra = b""
    if not stream_codes and sr_code == 0:
        if rate % 1000 == 0 and rate // 1000 < 256:
            sr_code, sr_extra = 12, bytes([rate // 1000])
        elif rate < 65536:
            sr_code, sr_extra = 13, rate.to_bytes(2, "big")
        elif rate % 10 == 0 and rate // 10 < 65536:
            sr_code, sr_extra = 14, (rate // 10).to_bytes(2, "big")
    ss_code = 0 if stream_codes else _SS_CODES.get(bps, 0)
    ch_code = assignment if assignment >= 8 else channels - 1
    h = bytes([0xFF, 0xF8 | (1 if variable else 0), (bs_code << 4) | sr_code, (ch_code << 4) | (ss_code << 1)]) + utf8_number(number)
    if bs_code == 6:
        h += bytes([n - 1])
    elif bs_code == 7:
        h += (n - 1).to_bytes(2, "big")
    h += sr_extra
    return h + bytes([crc8(h)])


def encode_frame(x, rate: int, bps: int, number: int, variable=False, assignment=INDEPENDENT, subframes=None, stream_codes=False,
                 bs_code=None) -> bytes:
    """x: [n, channels] ints. subframes: one spec per channel (default VERBATIM)"""
    x = np.asarray(x, np.int64)
    n, ch = x.shape
    subframes = subframes or [{"type": "verbatim"}] * ch
    if assignment >= 8:
        assert ch == 2
        l, r = x[:, 0], x[:, 1]
        side = l - r
        chans = {LEFT_SIDE: [(l, bps), (side, bps + 1)], SIDE_RIGHT: [(side, bps + 1), (r, bps)],
                 MID_SIDE: [((l + r) >> 1, bps), (side, bps + 1)]}[assignment]
    else:
        chans = [(x[:, c], bps) for c in range(ch)]
    parts = []
    for (v, w), spec in zip(chans, subframes):
        parts += subframe_bits(v, w, spec)
    body = frame_header(n, rate, ch, bps, number, variable, assignment, stream_codes, bs_code) + pack(parts)
    return body + crc16(body).to_bytes(2, "big")


def streaminfo(pcm, rate: int, bps: int, min_bs: int, max_bs: int, total=None, md5=True) -> bytes:
    x = np.asarray(pcm, np.int64)
    n, ch = x.shape
    nb = (bps + 7) // 8
    raw = x.astype("<i8").view(np.uint8).reshape(n, ch, 8)[:, :, :nb]
    digest = hashlib.md5(raw.tobytes()).digest() if md5 else bytes(16)
    v = (rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | (n if total is None else total)
    return min_bs.to_bytes(2, "big") + max_bs.to_bytes(2, "big") + bytes(6) + v.to_bytes(8, "big") + digest


def metadata(info: bytes, padding: int = 0) -> bytes:
    """fLaC + STREAMINFO (+ a PADDING block)"""
    out = b"fLaC" + bytes([0x00 if padding else 0x80]) + len(info).to_bytes(3, "big") + info
    if padding:
        out += bytes([0x81]) + padding.to_bytes(3, "big") + bytes(padding)
    return out


def split_blocks(n: int, blocksize: int) -> list:
    return [blocksize] * (n // blocksize) + ([n % blocksize] if n % blocksize else [])


def encode_frames(pcm, rate: int, bps: int, blocks, subframe=None, assignment=INDEPENDENT, variable=False, first_number=0,
                  stream_codes=False, bs_code=None) -> list:
    x = np.asarray(pcm, np.int64)
    ch = x.shape[1]
    out, pos = [], 0
    for f, n in enumerate(blocks):
        subs = [(subframe(f, c) if callable(subframe) else subframe) or {"type": "verbatim"} for c in range(ch)]
        a = assignment(f) if callable(assignment) else assignment
        number = first_number + (pos if variable else f)
        out.append(encode_frame(x[pos:pos + n], rate, bps, number, variable, a, subs, stream_codes,
                                bs_code(f) if callable(bs_code) else bs_code))
        pos += n
    assert pos == x.shape[0], "the blocks do not add up to the stream"
    return out


def encode_stream(pcm, rate: int, bps: int, blocks, padding: int = 0, **kw) -> bytes:
    frames = encode_frames(pcm, rate, bps, blocks, **kw)
    info = streaminfo(pcm, rate, bps, max(16, min(blocks[:-1] or blocks)), max(blocks))
    return metadata(info, padding) + b"".join(frames)
