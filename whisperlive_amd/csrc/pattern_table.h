// pattern_table.h — the host side of a regular-expression grammar (wlx_pattern_set / wlx_pattern_vocab_set; dec_pattern.hip) that needs no
// device: the check of the byte DFA and of the vocabulary's byte strings a caller hands in, and the layout of the table in the block of
// words the kernel copies into LDS. Plain C++ without a device call, so a stand-alone program can run it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace wlx {

constexpr int PATTERN_MAX_STATES = 4096;        // include/wlx_pattern.h WLX_PATTERN_MAX_STATES: a state fits the short the bias states use
constexpr int PATTERN_MAX_CELLS = 24576;        // WLX_PATTERN_MAX_CELLS: n_states * n_classes uint16 cells, 48 KiB of LDS
constexpr int PATTERN_MAX_TOKEN_BYTES = 255;    // WLX_PATTERN_MAX_TOKEN_BYTES
constexpr int PATTERN_MAX_VOCAB_BYTES = 1 << 22;        // WLX_PATTERN_MAX_VOCAB_BYTES
constexpr unsigned PATTERN_DEAD = 0xFFFFu;
// the block, in 32-bit words, every part 16-byte aligned: [4] header (n_states, n_classes, eot, cells), the byte -> class map [256 bytes],
// trans [PATTERN_MAX_CELLS] uint16 row-major (state * n_classes + class), accept [PATTERN_MAX_STATES] bytes
constexpr int PATTERN_HDR_WORDS = 4;
constexpr int PATTERN_CLASS_AT = PATTERN_HDR_WORDS;
constexpr int PATTERN_TRANS_AT = PATTERN_CLASS_AT + 256 / 4;
constexpr int PATTERN_ACCEPT_AT = PATTERN_TRANS_AT + PATTERN_MAX_CELLS / 2;
constexpr int PATTERN_TABLE_WORDS = PATTERN_ACCEPT_AT + PATTERN_MAX_STATES / 4;

// the format of include/wlx_pattern.h, violation by violation: true, or false with the reason in `msg`. Reads nothing past what the counts
// checked so far allow.
inline bool pattern_table_check(int V, int eot, int n_states, int n_classes, const uint8_t* byte_class, const uint16_t* trans,
                                const uint8_t* accept, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b, long c) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b, c); return false; };
    if (V < 1 || eot < 1 || eot >= V) return fail("pattern: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1, 0);
    if (n_states < 1 || n_states > PATTERN_MAX_STATES) return fail("pattern: %ld states outside 1..%ld", n_states, PATTERN_MAX_STATES, 0);
    if (n_classes < 1 || n_classes > 256) return fail("pattern: %ld byte classes outside 1..256", n_classes, 0, 0);
    if ((long)n_states * n_classes > PATTERN_MAX_CELLS)
        return fail("pattern: %ld states x %ld classes is more than %ld cells", n_states, n_classes, PATTERN_MAX_CELLS);
    if (!byte_class || !trans || !accept) return fail("pattern: null argument", 0, 0, 0);
    for (int b = 0; b < 256; ++b)
        if (byte_class[b] >= n_classes) return fail("pattern: byte %ld has class %ld, outside 0..%ld", b, byte_class[b], (long)n_classes - 1);
    for (int n = 0; n < n_states; ++n) {
        if (accept[n] > 1) return fail("pattern: accept[%ld] is %ld, not 0 or 1", n, accept[n], 0);
        for (int c = 0; c < n_classes; ++c) {
            const unsigned t = trans[(size_t)n * n_classes + c];
            if (t != PATTERN_DEAD && t >= (unsigned)n_states)
                return fail("pattern: state %ld moves to state %ld, neither 0xFFFF (dead) nor below %ld", n, t, n_states);
        }
    }
    return true;
}

// a CHECKED table into a block of PATTERN_TABLE_WORDS words -> the words in use from the block's start up to the last cell (the accept
// region, at its fixed place, is n_states bytes more)
inline int pattern_table_pack(uint32_t* block, int eot, int n_states, int n_classes, const uint8_t* byte_class, const uint16_t* trans,
                              const uint8_t* accept) {
    const int cells = n_states * n_classes;
    block[0] = (uint32_t)n_states; block[1] = (uint32_t)n_classes; block[2] = (uint32_t)eot; block[3] = (uint32_t)cells;
    memcpy(block + PATTERN_CLASS_AT, byte_class, 256);
    memcpy(block + PATTERN_TRANS_AT, trans, sizeof(uint16_t) * (size_t)cells);
    memcpy(block + PATTERN_ACCEPT_AT, accept, (size_t)n_states);
    return PATTERN_TRANS_AT + (cells + 1) / 2;
}

// the vocabulary's byte strings (wlx_pattern_vocab_set): tok_off[eot + 1] starts at 0 and ascends, no token longer than
// PATTERN_MAX_TOKEN_BYTES, at most PATTERN_MAX_VOCAB_BYTES bytes in all
inline bool pattern_vocab_check(int V, int eot, const int32_t* tok_off, const uint8_t* bytes, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b, long c) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b, c); return false; };
    if (V < 1 || eot < 1 || eot >= V) return fail("pattern vocabulary: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1, 0);
    if (!tok_off) return fail("pattern vocabulary: null argument", 0, 0, 0);
    if (tok_off[0] != 0) return fail("pattern vocabulary: tok_off[0] must be 0", 0, 0, 0);
    for (int t = 0; t < eot; ++t) {
        const long n = (long)tok_off[t + 1] - tok_off[t];
        if (n < 0) return fail("pattern vocabulary: the offsets descend at token %ld", t, 0, 0);
        if (n > PATTERN_MAX_TOKEN_BYTES) return fail("pattern vocabulary: token %ld has %ld bytes (at most %ld)", t, n, PATTERN_MAX_TOKEN_BYTES);
        if (tok_off[t + 1] > PATTERN_MAX_VOCAB_BYTES)
            return fail("pattern vocabulary: more than %ld bytes (token %ld ends at %ld)", PATTERN_MAX_VOCAB_BYTES, t, tok_off[t + 1]);
    }
    if (tok_off[eot] > 0 && !bytes) return fail("pattern vocabulary: null argument", 0, 0, 0);
    return true;
}

}  // namespace wlx
