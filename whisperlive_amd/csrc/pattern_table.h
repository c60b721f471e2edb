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

// ---- a POOL of tables (wlx_pattern_set_items; dec_pattern.hip dec_pattern_items_kernel): up to PATTERN_SET_MAX_TABLES tables, each within
// the limits of one table above. In 32-bit words, every part at a fixed place: one header of PATTERN_POOL_HDR_WORDS words per table SLOT
// (first cell, first accept byte, n_states, n_classes; n_states 0: no table); the 256-byte class maps, one per slot; the trans arrays
// back to back as uint16 cells, EACH starting on a 16-byte boundary (a multiple of 8 cells: the kernel copies a table with 16-byte loads,
// so a 1 x 1 table in front must not misalign the next — the region holds the pad of every table on top of the cap); the accept bytes
// back to back. A state stays a number local to its table.
constexpr int PATTERN_SET_MAX_TABLES = 64;      // include/wlx_pattern_items.h WLX_PATTERN_SET_MAX_TABLES
constexpr int PATTERN_SET_MAX_CELLS = 393216;   // WLX_PATTERN_SET_MAX_CELLS, over all tables: sixteen tables at the per-table cap, 768 KiB
constexpr int PATTERN_SET_MAX_STATES = 65536;   // WLX_PATTERN_SET_MAX_STATES, over all tables
constexpr int PATTERN_POOL_HDR_WORDS = 4;
constexpr int PATTERN_POOL_CLASS_AT = PATTERN_SET_MAX_TABLES * PATTERN_POOL_HDR_WORDS;
constexpr int PATTERN_POOL_TRANS_AT = PATTERN_POOL_CLASS_AT + PATTERN_SET_MAX_TABLES * (256 / 4);
constexpr int PATTERN_POOL_TRANS_CELLS = PATTERN_SET_MAX_CELLS + 8 * PATTERN_SET_MAX_TABLES;
constexpr int PATTERN_POOL_ACCEPT_AT = PATTERN_POOL_TRANS_AT + PATTERN_POOL_TRANS_CELLS / 2;
constexpr int PATTERN_POOL_WORDS = PATTERN_POOL_ACCEPT_AT + PATTERN_SET_MAX_STATES / 4;

// the format of include/wlx_pattern_items.h, violation by violation: true with the totals in *cells_out (the pads included: the cells the
// trans region holds up to the last table's end) and *states_out, or false with the reason in `msg`. A table's arrays are read only after
// the tables before it passed and the totals so far are within the caps.
inline bool pattern_pool_check(int V, int eot, int n_tables, const int32_t* n_states, const int32_t* n_classes, const uint8_t* byte_class,
                               const uint16_t* trans, const uint8_t* accept, int* cells_out, int* states_out, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b); return false; };
    if (V < 1 || eot < 1 || eot >= V) return fail("pattern set: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1);
    if (n_tables < 1 || n_tables > PATTERN_SET_MAX_TABLES) return fail("pattern set: %ld tables outside 1..%ld", n_tables, PATTERN_SET_MAX_TABLES);
    if (!n_states || !n_classes || !byte_class || !trans || !accept) return fail("pattern set: null argument", 0, 0);
    long cells = 0, states = 0, padded = 0;
    for (int t = 0; t < n_tables; ++t) {
        const long ns = n_states[t], nc = n_classes[t];
        char why[200] = "";
        // (the counts first, without the arrays: the totals decide whether this table's cells may be read at all)
        if (ns < 1 || ns > PATTERN_MAX_STATES || nc < 1 || nc > 256 || ns * nc > PATTERN_MAX_CELLS) {
            pattern_table_check(V, eot, (int)ns, (int)nc, nullptr, nullptr, nullptr, why, sizeof(why));
            if (msg && msg_len) snprintf(msg, msg_len, "pattern set: table %d: %s", t, why);
            return false;
        }
        if (cells + ns * nc > PATTERN_SET_MAX_CELLS) return fail("pattern set: more than %ld cells in all (at table %ld)", PATTERN_SET_MAX_CELLS, t);
        if (states + ns > PATTERN_SET_MAX_STATES) return fail("pattern set: more than %ld states in all (at table %ld)", PATTERN_SET_MAX_STATES, t);
        if (!pattern_table_check(V, eot, (int)ns, (int)nc, byte_class + (size_t)t * 256, trans + cells, accept + states, why, sizeof(why))) {
            if (msg && msg_len) snprintf(msg, msg_len, "pattern set: table %d: %s", t, why);
            return false;
        }
        cells += ns * nc;
        states += ns;
        padded = (padded + 7) / 8 * 8 + ns * nc;
    }
    if (cells_out) *cells_out = (int)padded;
    if (states_out) *states_out = (int)states;
    return true;
}

// a CHECKED set into a block of PATTERN_POOL_WORDS words. The used parts: [0, CLASS_AT + 64 * n_tables) words, the cells pattern_pool_check
// counted at TRANS_AT, `states` bytes at ACCEPT_AT; the headers of the table slots behind n_tables are zeroed, and so is every pad
inline void pattern_pool_pack(uint32_t* block, int n_tables, const int32_t* n_states, const int32_t* n_classes, const uint8_t* byte_class,
                              const uint16_t* trans, const uint8_t* accept) {
    memset(block, 0, sizeof(uint32_t) * (size_t)PATTERN_POOL_CLASS_AT);
    memcpy(block + PATTERN_POOL_CLASS_AT, byte_class, (size_t)n_tables * 256);
    uint16_t* cells = reinterpret_cast<uint16_t*>(block + PATTERN_POOL_TRANS_AT);
    uint8_t* acc = reinterpret_cast<uint8_t*>(block + PATTERN_POOL_ACCEPT_AT);
    int src = 0, at = 0, sb = 0;
    for (int t = 0; t < n_tables; ++t) {
        const int n = n_states[t] * n_classes[t];
        while (at & 7) cells[at++] = 0;         // the table starts on a 16-byte boundary
        uint32_t* hdr = block + t * PATTERN_POOL_HDR_WORDS;
        hdr[0] = (uint32_t)at; hdr[1] = (uint32_t)sb; hdr[2] = (uint32_t)n_states[t]; hdr[3] = (uint32_t)n_classes[t];
        memcpy(cells + at, trans + src, sizeof(uint16_t) * (size_t)n);
        memcpy(acc + sb, accept + sb, (size_t)n_states[t]);
        src += n; at += n; sb += n_states[t];
    }
    while (at & 7) cells[at++] = 0;             // (the kernel's last 16-byte load of the last table)
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
