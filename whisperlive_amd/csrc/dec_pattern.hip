// dec_pattern.hip — regular-expression grammars: the one launch between the vocabulary projection and the token search of a decode step
// whose slot has a pattern installed (wlx_pattern_set). A step of a slot without one does not launch it.
//
// The pattern is a DFA over the BYTES of the text, compiled on the host (whisperlive_amd/pattern.py): a 256-byte byte -> class map,
// trans[n_states][n_classes] as uint16 (0xFFFF = dead), accept[n_states]; state 0 is the start state. The vocabulary's byte strings are
// resident per engine (wlx_pattern_vocab_set): tok_off[eot + 1] and the concatenated bytes of the text tokens 0 .. eot - 1.
//
// Semantics per row (tests/test_gpu_pattern_kernel.py restates them as a Python loop over bytes). State at position p:
//   - the start state while the fed token is a prompt token (p < plen or p < 1);
//   - the parent's state at p - 1 where the fed token is >= eot (specials and timestamps are transparent);
//   - otherwise the walk of the token's bytes from the parent's state;
//   - the start state where that walk dies, or where the token has no bytes (a caller-forced prefix).
//   A parent's state outside 0 .. n_states - 1, left behind by another mode, reads as the start state.
// A row with st.nsp_row[r] > 0 writes its state and keeps its logits raw. Otherwise a text token t < eot keeps its logit iff it has at
// least one byte and its walk from the row's state does not die; eot keeps its logit iff the state accepts; ids above eot and the pad
// columns keep their bits. A logit word is what it was, or 0xff800000: no arithmetic touches a logit.
//
// Shape: the grid of dec_grammar_kernel, one workgroup of 256 threads per (row, tile of GRAMMAR_TILE ids). Per workgroup:
//   1. the class map and the table's cells in use go into LDS with 16-byte loads (static LDS: 48 KiB hold the largest table); the
//      offsets of the thread's tokens and the first piece of the tile's bytes are requested with them, in front of one barrier;
//   2. every thread walks the fed token's bytes from the parent's state out of that LDS table — the bytes come 64 per load, one a
//      lane, and go round the wave; the same uniform walk in every lane, so no broadcast through LDS and no barrier — and tile 0
//      stores the row's state (the parent's state at p - 1 is a word no workgroup of this launch writes: the rows of an item share a
//      position);
//   3. the tile's byte span [tok_off[c0], tok_off[c0 + n)) is contiguous (ids ascend); it is staged through LDS in pieces of 16 KiB
//      with 16-byte loads. Token c0 + k belongs to thread k % 256: eight tokens a thread, their offsets and their DFA states in
//      registers, so a token that straddles two pieces simply carries its state from one piece's walk into the next;
//   4. almost every token dies on its first byte. A piece is walked in two passes: the first byte of each of a thread's tokens, which all
//      lanes execute together, then the remaining bytes of the survivors. Neighbouring ids go to neighbouring lanes because survivors
//      cluster in id space (the digits, the single letters): a lane that owned eight consecutive ids would walk a cluster alone while
//      its wave waits;
//   5. the keep-bitmap of the tile (64 words of LDS) is written by wave ballots, one per (wave, token of the thread), with end-of-text's
//      bit from accept[state]; the stores are dec_grammar_kernel's.
#include "decoder.h"
#include "host.h"
#include "pattern_table.h"

namespace wlx {

#define PATTERN_THREADS 256
#define PATTERN_NEG_INF 0xff800000u
#define PATTERN_PIECE 16384                                     // bytes of the tile's span staged at a time
#define PATTERN_NPT (GRAMMAR_TILE / PATTERN_THREADS)            // tokens per thread

__global__ __launch_bounds__(PATTERN_THREADS) void dec_pattern_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp,
                                                                      SearchState st, PatternTable pt) {
    if (*st.done) return;                       // scratch steps behind the end of the call
    const int r = blockIdx.y, c0 = blockIdx.x * GRAMMAR_TILE;
    const int R = spp->R, eot = spp->eot;
    const long ldl = spp->ldl;
    if (c0 > eot) return;                       // ids above end-of-text keep their bits: nothing to do in this tile
    const int item = r / R, rb = r - item * R;
    if (st.item_done[item]) return;
    if (spp->sampling) { if (rb >= spp->num_hyp || st.row_done[r]) return; }
    else if (rb >= spp->beam) return;
    const int tid = threadIdx.x;
    const int p = st.pos[r], plen = st.plen[item], tok = st.token[r];
    if (p < 0 || p >= WLX_T_TEXT) return;
    const bool raw = st.nsp_row[r] > 0;         // the row's RAW distribution defines no_speech_prob: its state is written, its logits stay
    if (raw && blockIdx.x != 0) return;
    // (every return above depends on the row and the tile alone: the workgroup is whole at each barrier below)
    __shared__ __attribute__((aligned(16))) unsigned short s_trans[PATTERN_MAX_CELLS];
    __shared__ __attribute__((aligned(16))) unsigned char s_cls[256];
    __shared__ __attribute__((aligned(16))) unsigned char s_bytes[PATTERN_PIECE];
    __shared__ unsigned s_keep[GRAMMAR_TILE / 32];
    // ---- 1. everything that does not depend on the row's state is requested at once, in front of ONE barrier: the table's cells in use
    // and the class map, the offsets of the thread's tokens (c0 + tid + 256 j) and the first piece of the tile's bytes
    const uint4 hdr = *reinterpret_cast<const uint4*>(pt.block);
    const int n_states = (int)hdr.x, nc = (int)hdr.y;
    const int cells = min((int)hdr.w, PATTERN_MAX_CELLS);
    const int n_tok = min(GRAMMAR_TILE, eot - c0);              // text tokens of the tile (0 where the tile starts at end-of-text)
    const int span_lo = pt.tok_off[c0], span_hi = pt.tok_off[c0 + n_tok];
    int tb[PATTERN_NPT], te[PATTERN_NPT];
#pragma unroll
    for (int j = 0; j < PATTERN_NPT; ++j) {
        const int k = tid + j * PATTERN_THREADS;
        tb[j] = te[j] = 0;
        if (k < n_tok) { tb[j] = pt.tok_off[c0 + k]; te[j] = pt.tok_off[c0 + k + 1]; }
    }
    {
        const uint4* gt = reinterpret_cast<const uint4*>(pt.block + PATTERN_TRANS_AT);
        uint4* lt = reinterpret_cast<uint4*>(s_trans);
        const int n16 = (cells * 2 + 15) >> 4;
        for (int i = tid; i < n16; i += PATTERN_THREADS) lt[i] = gt[i];
        if (tid < 16) reinterpret_cast<uint4*>(s_cls)[tid] = reinterpret_cast<const uint4*>(pt.block + PATTERN_CLASS_AT)[tid];
    }
    int pb = span_lo & ~15;                     // (a multiple of 16; the bytes are padded to one)
    auto stage = [&](int at) {
        const uint4* gb = reinterpret_cast<const uint4*>(pt.bytes + at);
        const int n16 = (min(PATTERN_PIECE, span_hi - at) + 15) >> 4;
        for (int i = tid; i < n16; i += PATTERN_THREADS) reinterpret_cast<uint4*>(s_bytes)[i] = gb[i];
    };
    if (!raw) stage(pb);
    // ... and the fed token's walk has its four dependent global reads (ancestor, its state, the token's offsets, its first 64 bytes, one a
    // lane) under way before the barrier too: the row's state is the start state while the fed token is a prompt token
    const bool generated = p >= plen && p >= 1, text = generated && (unsigned)tok < (unsigned)eot;
    const int lane = tid & 63;
    int ps = 0, fb = 0, fe = 0, mine = 0;
    if (generated) ps = pt.state[(long)st.anc[(long)r * WLX_T_TEXT + p - 1] * WLX_T_TEXT + p - 1];
    if (text) {
        fb = pt.tok_off[tok]; fe = pt.tok_off[tok + 1];
        if (fb + lane < fe) mine = pt.bytes[fb + lane];
    }
    __syncthreads();
    // ---- 2. the row's state
    if (ps < 0 || ps >= n_states) ps = 0;       // (a state another table or mode left behind: never indexes past this one)
    int state = ps;                             // a special or a timestamp is transparent: the parent's state
    if (text) {                                 // a text token: the walk of its bytes, or the start state (uniform in the workgroup)
        unsigned s = fe > fb ? (unsigned)ps : PATTERN_DEAD;
        for (int q0 = fb; q0 < fe && s != PATTERN_DEAD; q0 += 64) {        // 64 bytes per load, handed round the wave
            if (q0 > fb) mine = q0 + lane < fe ? pt.bytes[q0 + lane] : 0;
            const int n = min(64, fe - q0);
            for (int i = 0; i < n && s != PATTERN_DEAD; ++i) s = s_trans[s * nc + s_cls[__shfl(mine, i)]];
        }
        state = s == PATTERN_DEAD ? 0 : (int)s;
    }
    if (blockIdx.x == 0 && tid == 0) pt.state[(long)r * WLX_T_TEXT + p] = (short)state;
    if (raw) return;
    // ---- 3. / 4. the thread's tokens, piece by piece: first bytes together, then the survivors
    unsigned ts[PATTERN_NPT];
#pragma unroll
    for (int j = 0; j < PATTERN_NPT; ++j) ts[j] = te[j] > tb[j] ? (unsigned)state : PATTERN_DEAD;      // a token without bytes is never allowed
    for (;;) {
        const int pe = pb + min(PATTERN_PIECE, span_hi - pb);
#pragma unroll
        for (int j = 0; j < PATTERN_NPT; ++j) {
            const int lo = max(tb[j], pb);
            if (lo < min(te[j], pe) && ts[j] != PATTERN_DEAD) {
                ts[j] = s_trans[ts[j] * nc + s_cls[s_bytes[lo - pb]]];
                tb[j] = lo + 1;
            }
        }
#pragma unroll
        for (int j = 0; j < PATTERN_NPT; ++j) {
            const int hi = min(te[j], pe);
            unsigned s = ts[j];
            for (int q = max(tb[j], pb); q < hi && s != PATTERN_DEAD; ++q) s = s_trans[s * nc + s_cls[s_bytes[q - pb]]];
            ts[j] = s;
        }
        pb += PATTERN_PIECE;
        if (pb >= span_hi) break;               // (uniform in the workgroup)
        __syncthreads();                        // the walk of the piece before is over
        stage(pb);
        __syncthreads();
    }
    // ---- 5. the tile's allowed ids: the tokens whose walk lived, and end-of-text where the state accepts
    const bool accepts = reinterpret_cast<const unsigned char*>(pt.block + PATTERN_ACCEPT_AT)[state] != 0;
#pragma unroll
    for (int j = 0; j < PATTERN_NPT; ++j) {
        const int k = tid + j * PATTERN_THREADS;
        const bool alive = k < n_tok ? ts[j] != PATTERN_DEAD : (c0 + k == eot && accepts);
        const unsigned long long m = __ballot(alive);
        if ((tid & 63) == 0) {
            s_keep[(k >> 5)] = (unsigned)m;
            s_keep[(k >> 5) + 1] = (unsigned)(m >> 32);
        }
    }
    __syncthreads();
    float* lrow = logits + (long)r * ldl;
    if ((ldl & 3) == 0 && (reinterpret_cast<unsigned long long>(logits) & 15ull) == 0) {
        // 16-byte pieces, two per thread: piece k covers ids c0 + 4k .. c0 + 4k + 3, all below ldl (a multiple of 4 above eot)
#pragma unroll
        for (int j = 0; j < GRAMMAR_TILE / 4 / PATTERN_THREADS; ++j) {
            const int k = tid + j * PATTERN_THREADS;
            const int col = c0 + 4 * k;
            if (col > eot) break;
            unsigned keep = (s_keep[k >> 3] >> ((k & 7) * 4)) & 0xfu;
            if (col + 3 > eot) keep |= (0xfu << (eot + 1 - col)) & 0xfu;        // ids above end-of-text keep their bits
            if (keep == 0xfu) continue;
            uint4* q = reinterpret_cast<uint4*>(lrow + col);
            uint4 v = make_uint4(PATTERN_NEG_INF, PATTERN_NEG_INF, PATTERN_NEG_INF, PATTERN_NEG_INF);
            if (keep) {
                const uint4 in = *q;
                if (keep & 1u) v.x = in.x;
                if (keep & 2u) v.y = in.y;
                if (keep & 4u) v.z = in.z;
                if (keep & 8u) v.w = in.w;
            }
            *q = v;
        }
    } else {
        // any other row stride: one word per thread and trip
        unsigned* urow = reinterpret_cast<unsigned*>(lrow);
        for (int k = tid; k < GRAMMAR_TILE; k += PATTERN_THREADS) {
            const int col = c0 + k;
            if (col > eot) break;
            if (!((s_keep[k >> 5] >> (k & 31)) & 1u)) urow[col] = PATTERN_NEG_INF;
        }
    }
}

void launch_dec_pattern(float* logits, const SearchParams* sp_dev, int rows, int V, const SearchState& st, const PatternTable& p, hipStream_t s) {
    const int tiles = (V + GRAMMAR_TILE - 1) / GRAMMAR_TILE;
    hipLaunchKernelGGL(dec_pattern_kernel, dim3(tiles, rows), dim3(PATTERN_THREADS), 0, s, logits, sp_dev, st, p);
}

}  // namespace wlx
