"""The matrix of synthetic FLAC streams the FLAC tests share (tests/flac_writer.py writes them from seeded integers): every stream is
at most 20 000 samples per channel, because the Python oracle decode is the slow part. cases() -> list of dicts
{name, data (the stream's bytes), frames (each frame's bytes), pcm (int64 [n, channels], what went in), rate, bps, blocks}."""
from __future__ import annotations

import functools

import numpy as np

from . import flac_writer as W


def noise(rng, n, ch, bps):
    return rng.randint(-(1 << (bps - 1)), 1 << (bps - 1), size=(n, ch)).astype(np.int64)


def smooth(rng, n, ch, bps, amp=0.4, jitter=2):
    t = np.arange(n)[:, None]
    f = rng.uniform(0.002, 0.03, size=(3, 1, ch))
    ph = rng.uniform(0, 6.28, size=(3, 1, ch))
    x = np.sin(6.2831853 * f * t[None] + ph).sum(axis=0) / 3.0
    return np.round(x * amp * (1 << (bps - 1))).astype(np.int64) + rng.randint(-jitter, jitter + 1, size=(n, ch))


def fit(spec, n):
    """the spec cut down to what a block of n samples allows (the short last frame of a stream)"""
    spec = dict(spec)
    order = spec.get("order", 0) if spec.get("type") == "fixed" else len(spec.get("coefs", ()))
    if spec.get("type") in ("fixed", "lpc") and order > n:
        return {"type": "verbatim", "wasted": spec.get("wasted", 0)}
    p = spec.get("porder", 0)
    while p and (n % (1 << p) or (n >> p) < order):
        p -= 1
    if p != spec.get("porder", 0):
        spec["porder"] = p
        if isinstance(spec.get("k"), (list, tuple)):
            spec["k"] = spec["k"][0]
        spec.pop("escape", None)
    return spec


def _case(name, pcm, rate, bps, blocks, subframe=None, **kw):
    if subframe is not None and not callable(subframe):
        one = subframe
        subframe = lambda f, c: one                                                       # noqa: E731
    sub = (lambda f, c: fit(subframe(f, c), blocks[f])) if subframe else None
    frames = W.encode_frames(pcm, rate, bps, blocks, subframe=sub, **kw)
    info = W.streaminfo(pcm, rate, bps, max(16, min(blocks[:-1] or blocks)), max(blocks))
    return dict(name=name, data=W.metadata(info) + b"".join(frames), frames=frames, pcm=np.asarray(pcm, np.int64), rate=rate, bps=bps,
                blocks=list(blocks))


@functools.lru_cache(maxsize=1)
def cases():
    rng = np.random.RandomState(20261019)
    out = []
    # ---- block sizes (each with a shorter last frame), widths, channel counts
    out.append(_case("bs16_8bit_mono_verbatim_last1", noise(rng, 16 * 3 + 1, 1, 8), 8000, 8, W.split_blocks(49, 16)))
    out.append(_case("bs17_16bit_stereo_fixed0to4", smooth(rng, 17 * 10 + 5, 2, 16), 16000, 16, W.split_blocks(175, 17),
                     subframe=lambda f, c: {"type": "fixed", "order": (f + c) % 5, "k": 4}))
    mid = noise(rng, 192 * 2 + 7, 2, 24)
    mid[::2, 0] |= 1
    mid[::2, 1] &= ~1                                                                     # odd l + r: the mid/side parity bit matters
    out.append(_case("bs192_24bit_midside_lpc8", mid, 44100, 24, W.split_blocks(391, 192), assignment=W.MID_SIDE,
                     subframe={"type": "lpc", "coefs": [9000, -7000, 5000, -3000, 2000, -1000, 500, -250], "precision": 15, "shift": 14,
                               "method": 1, "k": 22}))
    out.append(_case("bs256_16bit_3ch_lpc12_porder4", smooth(rng, 256 * 3 + 5, 3, 16), 48000, 16, W.split_blocks(773, 256),
                     subframe={"type": "lpc", "coefs": [1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1], "precision": 15, "shift": 0,
                               "porder": 4, "k": list(range(10, 26)), "method": 1}))       # the largest legal order for 256 / order 12
    out.append(_case("bs4096_16bit_leftside_lpc32_first_partition_empty", smooth(rng, 4096 * 2 + 5, 2, 16), 44100, 16, W.split_blocks(8197, 4096),
                     assignment=W.LEFT_SIDE,
                     subframe=lambda f, c: ({"type": "lpc", "coefs": [-1] * 32, "precision": 1, "shift": 0, "method": 1, "porder": 7, "k": 18}
                                            if c == 0 else {"type": "fixed", "order": 0, "porder": 12, "k": 14})))
    out.append(_case("bs4608_16bit_8ch_fixed2_porder9", smooth(rng, 4608 + 100, 8, 16), 96000, 16, W.split_blocks(4708, 4608),
                     subframe=lambda f, c: {"type": "fixed", "order": 2, "porder": 9 if c % 2 else 0, "k": 5}))
    side = noise(rng, 300 * 2 + 9, 2, 24)
    side[0], side[1] = ((1 << 23) - 1, -(1 << 23)), (-(1 << 23), (1 << 23) - 1)           # l - r needs the 25th bit
    out.append(_case("bs300_24bit_sideright_25bit_side_escape24", side, 32000, 24, W.split_blocks(609, 300),
                     assignment=lambda f: (W.SIDE_RIGHT, W.LEFT_SIDE, W.MID_SIDE)[f % 3],
                     subframe=lambda f, c: {"type": "fixed", "order": 0, "escape": {0: 25}} if f == 1 else {"type": "verbatim"}))
    # ---- LPC orders x precision x shift, Rice k = 14
    lp = smooth(rng, 256 * 16, 1, 16)
    combos = [(o, m) for o in (1, 8, 12, 32) for m in range(4)]

    def lpc_spec(f, c):
        o, m = combos[f]
        r = np.random.RandomState(f)
        coefs, prec, shift = (([-1] * o, 1, 0), (list(r.randint(-(1 << 14), 1 << 14, size=o)), 15, 14),
                              (list(r.randint(-2, 3, size=o)), 15, 0), ([-1 if i % 2 else 0 for i in range(o)], 1, 14))[m]
        return {"type": "lpc", "coefs": [int(v) for v in coefs], "precision": prec, "shift": shift, "k": 14, "method": f % 2}
    out.append(_case("lpc_orders_1_8_12_32_precision_1_15_shift_0_14_k14", lp, 22050, 16, [256] * 16, subframe=lpc_spec))
    # ---- Rice k = 0, escape widths 0 and bps, CONSTANT, wasted bits 1 and 7
    quiet = smooth(rng, 64 * 6, 2, 8, amp=0.3, jitter=1)
    quiet[64 * 2:64 * 3, 0] = 0                                                           # all-zero residuals: an escape partition of width 0
    quiet[64 * 4:64 * 5, 1] = -77                                                         # CONSTANT

    def quiet_spec(f, c):
        if f == 2 and c == 0:
            return {"type": "fixed", "order": 0, "porder": 1, "escape": {0: 0, 1: 0}}
        if f == 3:
            return {"type": "fixed", "order": 0, "porder": 2, "escape": {1: 8, 3: 8}, "k": 3}
        if f == 4 and c == 1:
            return {"type": "constant"}
        return {"type": "fixed", "order": 2, "k": 0, "porder": f % 3}
    out.append(_case("k0_escape0_escape8_constant", quiet, 8000, 8, [64] * 6, subframe=quiet_spec))
    wb = noise(rng, 100 * 3, 2, 16)
    wb[:, 0] &= ~127
    wb[:, 1] &= ~1
    out.append(_case("wasted_bits_7_and_1", wb, 16000, 16, [100] * 3,
                     subframe=lambda f, c: {"type": ("verbatim", "fixed", "lpc")[f], "order": 1, "coefs": [1, 1], "precision": 3, "shift": 1,
                                            "k": 12, "wasted": 7 if c == 0 else 1}))
    # ---- the four channel assignments on full-range noise (odd and even mid/side parity both occur)
    st = noise(rng, 64 * 8, 2, 16)
    out.append(_case("assignments_independent_leftside_sideright_midside", st, 16000, 16, [64] * 8,
                     assignment=lambda f: (W.INDEPENDENT, W.LEFT_SIDE, W.SIDE_RIGHT, W.MID_SIDE)[f % 4],
                     subframe={"type": "fixed", "order": 1, "k": 14}))
    # ---- variable block size, sample numbers in the 36-bit form
    vb = smooth(rng, 16 + 100 + 4096 + 33 + 1, 2, 16)
    out.append(_case("variable_blocksize_36bit_sample_number", vb, 44100, 16, [16, 100, 4096, 33, 1], variable=True,
                     first_number=(1 << 35) + 12345, subframe={"type": "fixed", "order": 1, "k": 6}))
    # ---- more frames than a wave has lanes
    for nf in (130, 65):
        out.append(_case(f"{nf}_frames_of_16", smooth(rng, 16 * nf, 1, 8, jitter=1), 16000, 8, [16] * nf, subframe={"type": "fixed", "order": 1, "k": 3}))
    # ---- header codes: "as STREAMINFO", and the 8-bit kHz / 16-bit Hz / 16-bit tens-of-Hz rate forms; forced 16-bit size code
    for rate, sc in ((44100, True), (11000, False), (44101, False), (65540, False)):
        out.append(_case(f"header_codes_rate{rate}{'_as_streaminfo' if sc else ''}", noise(rng, 40, 2, 12), rate, 12, [32, 8], stream_codes=sc,
                         bs_code=7 if rate == 11000 else None))
    return out
