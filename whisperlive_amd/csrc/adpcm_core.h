// adpcm_core.h — the decoders of ONE block of one channel of IMA / DVI ADPCM (WAVE tag 0x11) and Microsoft ADPCM (tag 0x02), written once
// for the device and the host: ADPCM_HD expands to __host__ __device__ under hipcc and to nothing otherwise, so the same text is the body
// of adpcm_decode_kernel (adpcm.hip) and ordinary C++ (the probe's header walk, and the stand-alone check program of
// tests/test_adpcm_core_host.py, which runs it under the host sanitizers).
//
// IMA block: per channel a 4-byte header (int16 predictor, uint8 step index, one reserved byte), then 4-byte words interleaved by
// channel, 8 nibbles each, low nibble first. Samples per block and channel = (block_align - 4 ch) * 2 / ch + 1 (the header's predictor
// is the first). step = STEPS[index]; diff = step >> 3, + step >> 2 / step >> 1 / step for the nibble's bits 0 / 1 / 2; bit 3 subtracts;
// the predictor clamps to int16, the index moves by INDEX[nibble] and clamps to 0..88.
// MS block: for each field in turn one value per channel — predictor index (uint8), delta (int16), sample1 (int16), sample2 (int16) —
// then nibbles, high nibble first, interleaved by channel. Samples per block and channel = (block_align - 7 ch) * 2 / ch + 2 (sample2,
// then sample1, then one per nibble). predicted = (sample1 * c1 + sample2 * c2) >> 8 (an arithmetic shift: the floor), new = clamp16(
// predicted + signed nibble * delta), delta = max(16, (ADAPT[nibble] * delta) >> 8), capped at ADPCM_MS_DELTA_MAX so that no product
// leaves int32 whatever the bytes are (a valid stream never gets near it).
//
// Memory safety on any bytes: every read offset is < block_align, every write index < the sample count the CALLER gives clipped to what
// the block's bytes hold; the step index and the predictor index are clamped even though the probe has checked them. A damaged block
// gives wrong numbers, never undefined behaviour.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ADPCM_HD __host__ __device__
#else
#define ADPCM_HD
#endif

#define ADPCM_IMA 0
#define ADPCM_MS 1
#define ADPCM_MAX_COEF 32                 // coefficient pairs of an MS `fmt ` extension this decoder keeps (the standard set has 7)
#define ADPCM_MS_DELTA_MAX (0x7FFFFFFF / 768 / 8)

ADPCM_HD static inline int adpcm_ima_samples(int block_align, int ch) { return (block_align - 4 * ch) * 2 / ch + 1; }
ADPCM_HD static inline int adpcm_ms_samples(int block_align, int ch) { return (block_align - 7 * ch) * 2 / ch + 2; }

ADPCM_HD static inline int adpcm_clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

ADPCM_HD static inline int adpcm_ima_step(int index) {
    static const int16_t STEPS[89] = {
        7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
        157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
        1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
        11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
    return STEPS[index < 0 ? 0 : (index > 88 ? 88 : index)];
}

// one nibble of the IMA recurrence
ADPCM_HD static inline void adpcm_ima_nibble(unsigned nib, int* pred, int* index) {
    const int step = adpcm_ima_step(*index);
    int diff = step >> 3;
    if (nib & 1) diff += step >> 2;
    if (nib & 2) diff += step >> 1;
    if (nib & 4) diff += step;
    *pred = adpcm_clamp16((nib & 8) ? *pred - diff : *pred + diff);
    // INDEX = {-1, -1, -1, -1, 2, 4, 6, 8} for the low three bits
    const int m = (int)(nib & 7);
    int i = *index + (m < 4 ? -1 : 2 * (m - 3));
    *index = i < 0 ? 0 : (i > 88 ? 88 : i);
}

// channel c of the IMA block at blk[0 .. block_align): out[i * out_stride], 0 <= i < n, n = min(want, what the block holds). -> n
ADPCM_HD static inline int adpcm_ima_block(const uint8_t* blk, int block_align, int ch, int c, int want, int16_t* out, long long out_stride) {
    if (ch < 1 || c < 0 || c >= ch || block_align < 4 * ch || want < 1) return 0;
    const int words = (block_align - 4 * ch) / (4 * ch);
    const int n = want < words * 8 + 1 ? want : words * 8 + 1;
    const uint8_t* h = blk + 4 * c;
    int pred = (int16_t)(uint16_t)(h[0] | (h[1] << 8));
    int index = h[2] > 88 ? 88 : h[2];
    out[0] = (int16_t)pred;
    int i = 1;
    for (int w = 0; i < n; ++w) {
        const uint8_t* p = blk + 4 * ch + (w * ch + c) * 4;
        uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        for (int k = 0; k < 8 && i < n; ++k, ++i, v >>= 4) {
            adpcm_ima_nibble(v & 15u, &pred, &index);
            out[(long long)i * out_stride] = (int16_t)pred;
        }
    }
    return n;
}

ADPCM_HD static inline int adpcm_ms_adapt(unsigned nib) {
    static const int16_t ADAPT[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
    return ADAPT[nib & 15u];
}

// channel c of the MS block at blk[0 .. block_align); coefs: n_coef pairs (c1, c2). -> samples written (as adpcm_ima_block)
ADPCM_HD static inline int adpcm_ms_block(const uint8_t* blk, int block_align, int ch, int c, int want, const int16_t* coefs, int n_coef,
                                          int16_t* out, long long out_stride) {
    if (ch < 1 || c < 0 || c >= ch || block_align < 7 * ch || want < 1 || n_coef < 1) return 0;
    const int held = (block_align - 7 * ch) * 2 / ch + 2;
    const int n = want < held ? want : held;
    int pi = blk[c];
    if (pi >= n_coef) pi = n_coef - 1;
    const int c1 = coefs[2 * pi], c2 = coefs[2 * pi + 1];
    const uint8_t* q = blk + ch + 2 * c;
    int delta = (int16_t)(uint16_t)(q[0] | (q[1] << 8));
    q += 2 * ch;
    int s1 = (int16_t)(uint16_t)(q[0] | (q[1] << 8));
    q += 2 * ch;
    int s2 = (int16_t)(uint16_t)(q[0] | (q[1] << 8));
    out[0] = (int16_t)s2;
    if (n > 1) out[out_stride] = (int16_t)s1;
    for (int i = 2; i < n; ++i) {
        const int k = (i - 2) * ch + c;                     // nibble number behind the header; the even one is the high nibble
        const unsigned byte = blk[7 * ch + (k >> 1)];
        const unsigned nib = (k & 1) ? (byte & 15u) : (byte >> 4);
        const int sn = nib >= 8 ? (int)nib - 16 : (int)nib;
        if (delta > ADPCM_MS_DELTA_MAX) delta = ADPCM_MS_DELTA_MAX;
        if (delta < -ADPCM_MS_DELTA_MAX) delta = -ADPCM_MS_DELTA_MAX;
        const int v = adpcm_clamp16((int)(((long long)s1 * c1 + (long long)s2 * c2) >> 8) + sn * delta);
        delta = (adpcm_ms_adapt(nib) * delta) >> 8;
        if (delta < 16) delta = 16;
        s2 = s1; s1 = v;
        out[(long long)i * out_stride] = (int16_t)v;
    }
    return n;
}
