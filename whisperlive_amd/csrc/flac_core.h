// flac_core.h — the decoder of ONE FLAC frame, written once for the device and the host: FLAC_HD expands to __host__ __device__
// under hipcc and to nothing otherwise, so the same text is the body of flac_frames_kernel (flac.hip) and ordinary C++ (the
// stand-alone check program of tests/test_flac_core_host.py, which runs it under the host sanitizers).
//
// flac_decode_frame walks the bytes [start, end) of one frame — frame header, per channel a subframe header with its wasted-bits
// count, CONSTANT / VERBATIM / FIXED 0-4 / LPC 1-32 subframes, partitioned Rice residuals (methods 0 and 1, escape partitions) —
// and writes the frame's `blocksize` samples of each of `channels` channels as int32 into planes: out[c * plane_stride + i].
// Left/side, side/right and mid/side frames are left DECORRELATED-NOT-YET: the side plane holds bps + 1 bits and *assign_out says
// which form it is; flac_stereo restores left and right of one sample (the finish kernel runs it per sample).
//
// Memory safety on any bit pattern: every read goes through FlacBits, which refuses a read past `end` (the reader sticks at
// the end and `over` is set); every write index is < blocksize, which the CALLER gives (the frame table's value: a header that
// codes another size, or another channel count, is an error before the first write). The prediction runs in 64-bit, samples are
// stored with unsigned wrap-around, so a damaged stream gives wrong numbers or a status, never undefined behaviour.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__
#else
#define FLAC_HD
#endif

enum {
    FLAC_OK = 0,
    FLAC_E_END = 1,          // the bitstream ran past the frame's end
    FLAC_E_RESERVED = 2,     // a reserved code (sync, block size, sample size, channel assignment, subframe type, residual method, precision, shift < 0)
    FLAC_E_PARTITION = 3,    // partition order inconsistent with the block size / predictor order, or a header that disagrees with the frame table
    FLAC_E_TAIL = 4,         // the subframes did not end exactly at end - 2 after the (zero) padding
    FLAC_E_UNSUPPORTED = 5   // more than 24 bits per sample, more than FLAC_MAX_CHANNELS channels
};
#define FLAC_MAX_CHANNELS 8
#define FLAC_MAX_BPS 24
// channel assignments as *assign_out reports them
#define FLAC_CH_INDEPENDENT 0
#define FLAC_CH_LEFT_SIDE 8
#define FLAC_CH_SIDE_RIGHT 9
#define FLAC_CH_MID_SIDE 10

struct FlacBits {
    const uint8_t* d;
    int64_t p, e;            // bit position, end in bits (a whole number of bytes)
    int over;
};

// n in 0..32
FLAC_HD static inline uint32_t flac_read(FlacBits& b, int n) {
    if (n == 0) return 0;
    if (b.p + n > b.e) { b.over = 1; b.p = b.e; return 0; }
    const int off = (int)(b.p & 7), nb = (off + n + 7) >> 3;      // <= 5 bytes
    const int64_t b0 = b.p >> 3;
    uint64_t v = 0;
    for (int i = 0; i < nb; ++i) v = (v << 8) | b.d[b0 + i];
    b.p += n;
    return (uint32_t)((v >> (nb * 8 - off - n)) & (n == 32 ? 0xFFFFFFFFull : ((1ull << n) - 1)));
}

FLAC_HD static inline int32_t flac_read_signed(FlacBits& b, int n) {
    if (n == 0) return 0;
    const uint32_t v = flac_read(b, n);
    const int64_t s = (v >> (n - 1)) ? (int64_t)v - ((int64_t)1 << n) : (int64_t)v;
    return (int32_t)s;
}

// zeros before the next 1 bit (the 1 is consumed)
FLAC_HD static inline uint32_t flac_unary(FlacBits& b) {
    uint32_t n = 0;
    while (b.p < b.e) {
        const int off = (int)(b.p & 7);
        const uint32_t chunk = b.d[b.p >> 3] & (0xFFu >> off);
        if (chunk) {
            int lead = 0;
            for (uint32_t m = 0x80u >> off; !(chunk & m); m >>= 1) ++lead;
            b.p += lead + 1;
            return n + (uint32_t)lead;
        }
        n += (uint32_t)(8 - off);
        b.p += 8 - off;
    }
    b.over = 1;
    return n;
}

// residuals of one subframe into x[order .. n)
FLAC_HD static inline int flac_residual(FlacBits& b, int32_t* x, int n, int order) {
    const uint32_t method = flac_read(b, 2);
    if (b.over) return FLAC_E_END;
    if (method > 1) return FLAC_E_RESERVED;
    const int pbits = method == 0 ? 4 : 5;
    const uint32_t esc = method == 0 ? 15u : 31u;
    const int porder = (int)flac_read(b, 4);
    if (b.over) return FLAC_E_END;
    const int nparts = 1 << porder;
    if (porder > 0 && ((n & (nparts - 1)) != 0 || (n >> porder) < order)) return FLAC_E_PARTITION;
    int o = order;
    for (int part = 0; part < nparts; ++part) {
        const int cnt = porder ? (n >> porder) - (part == 0 ? order : 0) : n - order;
        const uint32_t k = flac_read(b, pbits);
        if (k == esc) {
            const int w = (int)flac_read(b, 5);
            for (int i = 0; i < cnt && !b.over; ++i) x[o + i] = flac_read_signed(b, w);
        } else {
            for (int i = 0; i < cnt && !b.over; ++i) {
                const uint64_t q = flac_unary(b);
                const uint64_t u = (q << k) | flac_read(b, (int)k);
                x[o + i] = (int32_t)(uint32_t)((u >> 1) ^ (0 - (u & 1)));
            }
        }
        if (b.over) return FLAC_E_END;
        o += cnt;
    }
    return FLAC_OK;
}

// one subframe of `bps` bits into x[0 .. n)
FLAC_HD static inline int flac_subframe(FlacBits& b, int32_t* x, int n, int bps) {
    const uint32_t head = flac_read(b, 8);
    if (b.over) return FLAC_E_END;
    if (head & 0x80) return FLAC_E_RESERVED;
    const int typ = (int)((head >> 1) & 63);
    int wasted = 0;
    if (head & 1) {
        wasted = (int)flac_unary(b) + 1;
        if (b.over) return FLAC_E_END;
        if (wasted >= bps) return FLAC_E_RESERVED;
        bps -= wasted;
    }
    if (typ == 0) {
        const int32_t v = flac_read_signed(b, bps);
        for (int i = 0; i < n; ++i) x[i] = v;
    } else if (typ == 1) {
        for (int i = 0; i < n && !b.over; ++i) x[i] = flac_read_signed(b, bps);
    } else if ((typ >= 8 && typ <= 12) || typ >= 32) {
        int32_t coef[32];
        int order, shift = 0;
        if (typ >= 32) {
            order = (typ & 31) + 1;
            if (order > n) return FLAC_E_PARTITION;
            for (int i = 0; i < order; ++i) x[i] = flac_read_signed(b, bps);
            const int prec = (int)flac_read(b, 4) + 1;
            if (b.over) return FLAC_E_END;
            if (prec == 16) return FLAC_E_RESERVED;
            shift = flac_read_signed(b, 5);
            if (shift < 0) return FLAC_E_RESERVED;
            for (int i = 0; i < order; ++i) coef[i] = flac_read_signed(b, prec);
        } else {
            order = typ - 8;
            if (order > n) return FLAC_E_PARTITION;
            for (int i = 0; i < order; ++i) x[i] = flac_read_signed(b, bps);
            const int32_t f1[1] = {1}, f2[2] = {2, -1}, f3[3] = {3, -3, 1}, f4[4] = {4, -6, 4, -1};
            const int32_t* f = order == 1 ? f1 : order == 2 ? f2 : order == 3 ? f3 : f4;
            for (int i = 0; i < order; ++i) coef[i] = f[i];
        }
        if (b.over) return FLAC_E_END;
        const int rc = flac_residual(b, x, n, order);
        if (rc != FLAC_OK) return rc;
        if (order > 0) {
            for (int i = order; i < n; ++i) {
                int64_t acc = 0;
                for (int j = 0; j < order; ++j) acc += (int64_t)coef[j] * (int64_t)x[i - 1 - j];
                x[i] = (int32_t)(uint32_t)((uint64_t)(int64_t)x[i] + (uint64_t)(acc >> shift));
            }
        }
    } else {
        return FLAC_E_RESERVED;
    }
    if (b.over) return FLAC_E_END;
    if (wasted)
        for (int i = 0; i < n; ++i) x[i] = (int32_t)((uint32_t)x[i] << wasted);
    return FLAC_OK;
}

// left and right of one sample from the two planes' values of a stereo-decorrelated frame (a: first subframe, b: second)
FLAC_HD static inline void flac_stereo(int assign, int32_t a, int32_t b, int32_t* l, int32_t* r) {
    if (assign == FLAC_CH_LEFT_SIDE) { *l = a; *r = (int32_t)((uint32_t)a - (uint32_t)b); }
    else if (assign == FLAC_CH_SIDE_RIGHT) { *l = (int32_t)((uint32_t)a + (uint32_t)b); *r = b; }
    else if (assign == FLAC_CH_MID_SIDE) {
        const int64_t m = ((int64_t)a * 2) | (b & 1);
        *l = (int32_t)((m + b) >> 1);
        *r = (int32_t)((m - b) >> 1);
    } else { *l = a; *r = b; }
}

// One frame: bytes [start, end) of `data` (end - 2 = its CRC-16) -> out[c * plane_stride + i], c < channels, i < blocksize.
// stream_bps: STREAMINFO's width (a frame may code 0 = "as STREAMINFO"). The header must code `blocksize` samples and `channels`
// channels (what the frame table holds), else FLAC_E_PARTITION before any write.
FLAC_HD static inline int flac_decode_frame(const uint8_t* data, int64_t start, int64_t end, int stream_bps, int channels, int blocksize,
                                            int32_t* out, int64_t plane_stride, int* assign_out) {
    *assign_out = FLAC_CH_INDEPENDENT;
    if (channels < 1 || channels > FLAC_MAX_CHANNELS || stream_bps < 1 || stream_bps > FLAC_MAX_BPS) return FLAC_E_UNSUPPORTED;
    if (blocksize < 1 || blocksize > 65536 || end - start < 2) return FLAC_E_PARTITION;
    FlacBits b;
    b.d = data; b.p = start * 8; b.e = (end - 2) * 8; b.over = 0;
    const uint32_t h = flac_read(b, 32);
    if (b.over) return FLAC_E_END;
    if ((h >> 18) != 0x3FFEu || (h & 0x20000u) || (h & 1u)) return FLAC_E_RESERVED;
    const int bs_code = (int)((h >> 12) & 15), sr_code = (int)((h >> 8) & 15), ch_code = (int)((h >> 4) & 15), ss_code = (int)((h >> 1) & 7);
    const uint32_t first = flac_read(b, 8);                 // the UTF-8-style coded frame / sample number: 0 .. 6 bytes follow
    int extra = 0;
    if (first >= 0x80) {
        for (uint32_t m = 0x80; first & m; m >>= 1) ++extra;
        if (extra < 2 || extra > 7) return FLAC_E_RESERVED;
        extra -= 1;
    }
    for (int i = 0; i < extra; ++i) (void)flac_read(b, 8);
    int n;
    if (bs_code == 0) return FLAC_E_RESERVED;
    else if (bs_code == 1) n = 192;
    else if (bs_code <= 5) n = 576 << (bs_code - 2);
    else if (bs_code == 6) n = (int)flac_read(b, 8) + 1;
    else if (bs_code == 7) n = (int)flac_read(b, 16) + 1;
    else n = 256 << (bs_code - 8);
    if (sr_code == 12) (void)flac_read(b, 8);
    else if (sr_code == 13 || sr_code == 14) (void)flac_read(b, 16);
    else if (sr_code == 15) return FLAC_E_RESERVED;
    (void)flac_read(b, 8);                                  // CRC-8 (checked by the host index)
    if (b.over) return FLAC_E_END;
    int bps;
    switch (ss_code) {
        case 0: bps = stream_bps; break;
        case 1: bps = 8; break;
        case 2: bps = 12; break;
        case 4: bps = 16; break;
        case 5: bps = 20; break;
        case 6: bps = 24; break;
        case 7: return FLAC_E_UNSUPPORTED;
        default: return FLAC_E_RESERVED;
    }
    if (ch_code > 10) return FLAC_E_RESERVED;
    const int nch = ch_code < 8 ? ch_code + 1 : 2;
    if (n != blocksize || nch != channels) return FLAC_E_PARTITION;
    for (int c = 0; c < nch; ++c) {
        const int side = (ch_code == FLAC_CH_LEFT_SIDE && c == 1) || (ch_code == FLAC_CH_SIDE_RIGHT && c == 0) || (ch_code == FLAC_CH_MID_SIDE && c == 1);
        const int rc = flac_subframe(b, out + (int64_t)c * plane_stride, n, bps + side);
        if (rc != FLAC_OK) return rc;
    }
    if (((b.p + 7) >> 3) != end - 2) return FLAC_E_TAIL;
    if ((b.p & 7) && flac_read(b, 8 - (int)(b.p & 7)) != 0) return FLAC_E_TAIL;      // the padding to the byte is zero bits
    *assign_out = ch_code < 8 ? FLAC_CH_INDEPENDENT : ch_code;
    return FLAC_OK;
}
