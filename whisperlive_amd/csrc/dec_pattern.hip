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

// ---- a pattern per item (wlx_pattern_set_items / wlx_pattern_select): a pool of tables (pattern_table.h), the table of a
// row the one selected for its item of the decode group. The semantics per row are dec_pattern_kernel's on that table, bit for bit; an
// item without a table (sel < 0) has its rows' states written as 0, and no table word, byte or logit of it is read.
//
// Everything dec_pattern_kernel stages — the table, the tile's token offsets, the tile's bytes — is the same for all rows of one item, so
// the grid is one workgroup of 256 threads per (ITEM, tile of GRAMMAR_TILE ids), and the staging of a launch no longer grows with the beam:
//   1. lane b of every wave looks at row b of the item (R <= 16): two ballots give every wave the same two uniform masks — the rows that
//      owe the launch a state (inside the beam; in sampling mode not done and below num_hyp; a position inside the text) and, of those,
//      the rows whose logits are masked (not nsp_row). A workgroup leaves at once for a finished call or item, a tile above end-of-text, a
//      deselected item (tile 0 writes the zeros), no row to walk, or — any tile but 0 — no row to mask. A skipped row is a cleared bit in a
//      uniform mask and a skipped trip of a uniform loop below: never a divergent barrier;
//   2. staged once, in front of ONE barrier: the item's class map and its cells in use (16-byte loads: every table of the pool starts on
//      a 16-byte boundary) into the same static 48 KiB, each thread's token offsets (eight tokens a thread, interleaved as in §30), the
//      first 16 KiB piece of the tile's bytes — and, with them, the dependent reads of the fed-token walks;
//   3. the fed-token walks are dealt over the four waves, wave w taking rows w, w + 4, w + 8, w + 12: each walk is uniform in its wave, the
//      bytes 64 per load handed round the wave. Lane 0 leaves the state (and, in end-of-text's tile, its accept flag) in LDS, tile 0 stores
//      it; one more barrier, and every thread knows every row's state;
//   4. the per-token states of ALL rows of the item sit in registers at once, two rows to a VGPR (a state is 16 bits, 0xFFFF dead): eight
//      tokens x eight row pairs = 64 VGPRs, one pass for any beam. The LDS of a workgroup allows two workgroups a CU, two waves a SIMD,
//      which leaves each wave 256 VGPRs: a second pass over eight rows would buy no occupancy and cost a second trip through the pieces.
//      A pair neither of whose rows is masked is a skipped uniform branch. Per piece of bytes every row is walked before the next piece
//      is staged — a tile's bytes are read from L2 once per ITEM — in §30's two-pass shape: the first byte of each of the thread's tokens
//      for all rows (the byte and its class are fetched once for the rows), then the remaining bytes while any row survives;
//   5. a keep-bitmap per masked row (256 B each, written by wave ballots; none is reused, so one barrier), then dec_pattern_kernel's
//      stores row by row. No arithmetic touches a logit.
// Static LDS only (68.3 KiB), no launch attribute raised, no scratch.
#define PATTERN_ITEM_ROWS 16                                    // rows of one item (wlx_slot_create: max_rows_per_item <= 16)
#define PATTERN_ITEM_PAIRS (PATTERN_ITEM_ROWS / 2)

// one byte of class `c` for the two rows packed into `w`
__device__ __forceinline__ unsigned pattern_step2(unsigned w, int c, int nc, const unsigned short* trans) {
    unsigned a = w & 0xFFFFu, b = w >> 16;
    if (a != PATTERN_DEAD) a = trans[a * nc + c];
    if (b != PATTERN_DEAD) b = trans[b * nc + c];
    return a | (b << 16);
}

__global__ __launch_bounds__(PATTERN_THREADS) void dec_pattern_items_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp,
                                                                            SearchState st, PatternItems pi) {
    if (*st.done) return;                       // scratch steps behind the end of the call
    const int item = blockIdx.y, tile = blockIdx.x, c0 = tile * GRAMMAR_TILE;
    const int R = spp->R, eot = spp->eot;
    const long ldl = spp->ldl;
    if (c0 > eot) return;                       // ids above end-of-text keep their bits: nothing to do in this tile
    if (st.item_done[item]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = item * R;
    // ---- 1. the item's rows: which owe a state, which are masked (uniform masks, the same in the four waves)
    bool walks = false, masks = false;
    int p_l = 0;
    if (lane < min(R, PATTERN_ITEM_ROWS)) {
        const int r = r0 + lane;
        bool on = spp->sampling ? (lane < spp->num_hyp && !st.row_done[r]) : lane < spp->beam;
        p_l = st.pos[r];
        on = on && p_l >= 0 && p_l < WLX_T_TEXT;
        walks = on;
        masks = on && !(st.nsp_row[r] > 0);     // a row whose RAW distribution defines no_speech_prob: its state is written, its logits stay
    }
    const unsigned walk_m = (unsigned)__ballot(walks), live_m = (unsigned)__ballot(masks);
    const int t = pi.sel[item];
    if (t < 0) {                                // no table for this item: the start state, and the rows' logits stay as they are
        if (tile == 0 && wave == 0 && walks) pi.state[(long)(r0 + lane) * WLX_T_TEXT + p_l] = 0;
        return;
    }
    if (!walk_m || (!live_m && tile != 0)) return;
    // (every return above depends on the item and the tile alone: the workgroup is whole at each barrier below)
    __shared__ __attribute__((aligned(16))) unsigned short s_trans[PATTERN_MAX_CELLS];
    __shared__ __attribute__((aligned(16))) unsigned char s_cls[256];
    __shared__ __attribute__((aligned(16))) unsigned char s_bytes[PATTERN_PIECE];
    __shared__ unsigned s_keep[PATTERN_ITEM_ROWS][GRAMMAR_TILE / 32];
    __shared__ int s_st[PATTERN_ITEM_ROWS];     // row b's state, its accept flag in bit 16
    // ---- 2. everything that does not depend on a row's state, in front of ONE barrier
    const uint4 hdr = reinterpret_cast<const uint4*>(pi.pool)[t];      // first cell, first accept byte, n_states, n_classes
    const int n_states = (int)hdr.z, nc = (int)hdr.w;
    const int cells = min(n_states * nc, PATTERN_MAX_CELLS);
    const int n_tok = min(GRAMMAR_TILE, eot - c0);              // text tokens of the tile (0 where the tile starts at end-of-text)
    const int span_lo = pi.tok_off[c0], span_hi = pi.tok_off[c0 + n_tok];
    int tb[PATTERN_NPT], te[PATTERN_NPT];
#pragma unroll
    for (int j = 0; j < PATTERN_NPT; ++j) {
        const int k = tid + j * PATTERN_THREADS;
        tb[j] = te[j] = 0;
        if (k < n_tok) { tb[j] = pi.tok_off[c0 + k]; te[j] = pi.tok_off[c0 + k + 1]; }
    }
    {
        const uint4* gt = reinterpret_cast<const uint4*>(pi.pool + PATTERN_POOL_TRANS_AT) + (hdr.x >> 3);
        uint4* lt = reinterpret_cast<uint4*>(s_trans);
        const int n16 = (cells * 2 + 15) >> 4;
        for (int i = tid; i < n16; i += PATTERN_THREADS) lt[i] = gt[i];
        if (tid < 16) reinterpret_cast<uint4*>(s_cls)[tid] = reinterpret_cast<const uint4*>(pi.pool + PATTERN_POOL_CLASS_AT + t * 64)[tid];
    }
    int pb = span_lo & ~15;                     // (a multiple of 16; the bytes are padded to one)
    auto stage = [&](int at) {
        const uint4* gb = reinterpret_cast<const uint4*>(pi.bytes + at);
        const int n16 = (min(PATTERN_PIECE, span_hi - at) + 15) >> 4;
        for (int i = tid; i < n16; i += PATTERN_THREADS) reinterpret_cast<uint4*>(s_bytes)[i] = gb[i];
    };
    if (live_m) stage(pb);
    // ... and the four dependent global reads of each fed-token walk of this wave (ancestor, its state, the token's offsets, its first 64
    // bytes, one a lane) are under way before the barrier too
    const int plen = st.plen[item];
    int w_p[4], w_ps[4], w_fb[4], w_fe[4], w_mine[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rb = wave + 4 * i, r = r0 + rb;
        w_p[i] = __shfl(p_l, rb);
        w_ps[i] = w_fb[i] = w_fe[i] = w_mine[i] = 0;
        if ((walk_m >> rb) & 1u) {
            const int p = w_p[i], tok = st.token[r];
            if (p >= plen && p >= 1) {          // a generated position: the parent's state (else the start state, and no walk)
                w_ps[i] = pi.state[(long)st.anc[(long)r * WLX_T_TEXT + p - 1] * WLX_T_TEXT + p - 1];
                if ((unsigned)tok < (unsigned)eot) {
                    w_fb[i] = pi.tok_off[tok]; w_fe[i] = pi.tok_off[tok + 1];
                    if (w_fb[i] + lane < w_fe[i]) w_mine[i] = pi.bytes[w_fb[i] + lane];
                    if (w_fe[i] == w_fb[i]) w_fe[i] = -1;       // a text token without bytes: the start state
                }
            }
        }
    }
    __syncthreads();
    // ---- 3. the rows' states, wave w the rows w, w + 4, w + 8, w + 12 (uniform within the wave)
    const bool eot_tile = (unsigned)(eot - c0) < (unsigned)GRAMMAR_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rb = wave + 4 * i;
        if (!((walk_m >> rb) & 1u)) continue;
        int ps = w_ps[i];
        if (ps < 0 || ps >= n_states) ps = 0;   // (a state another table or mode left behind: never indexes past this one)
        int state = ps;                         // a prompt position (0), a special or a timestamp (transparent): no walk
        const int fb = w_fb[i], fe = w_fe[i];
        if (fe != 0) {                          // a text token: the walk of its bytes, or the start state
            unsigned s = fe > fb ? (unsigned)ps : PATTERN_DEAD;
            int mine = w_mine[i];
            for (int q0 = fb; q0 < fe && s != PATTERN_DEAD; q0 += 64) {        // 64 bytes per load, handed round the wave
                if (q0 > fb) mine = q0 + lane < fe ? pi.bytes[q0 + lane] : 0;
                const int n = min(64, fe - q0);
                for (int k = 0; k < n && s != PATTERN_DEAD; ++k) s = s_trans[s * nc + s_cls[__shfl(mine, k)]];
            }
            state = s == PATTERN_DEAD ? 0 : (int)s;
        }
        if (lane == 0) {
            int acc = 0;
            if (eot_tile) acc = reinterpret_cast<const unsigned char*>(pi.pool + PATTERN_POOL_ACCEPT_AT)[hdr.y + state] != 0;
            s_st[rb] = state | (acc << 16);
            if (tile == 0) pi.state[(long)(r0 + rb) * WLX_T_TEXT + w_p[i]] = (short)state;
        }
    }
    if (!live_m) return;                        // (tile 0 of an item whose rows all stay raw: uniform)
    __syncthreads();
    // ---- 4. the thread's tokens under every masked row, piece by piece: first bytes together, then the survivors
    unsigned ts[PATTERN_NPT][PATTERN_ITEM_PAIRS];
#pragma unroll
    for (int q = 0; q < PATTERN_ITEM_PAIRS; ++q) {
        unsigned w = 0xFFFFFFFFu;               // a row that is not masked is dead from the start
        if ((live_m >> (2 * q)) & 3u) {
            const unsigned a = (live_m >> (2 * q)) & 1u ? (unsigned)s_st[2 * q] & 0xFFFFu : PATTERN_DEAD;
            const unsigned b = (live_m >> (2 * q)) & 2u ? (unsigned)s_st[2 * q + 1] & 0xFFFFu : PATTERN_DEAD;
            w = a | (b << 16);
        }
#pragma unroll
        for (int j = 0; j < PATTERN_NPT; ++j) ts[j][q] = te[j] > tb[j] ? w : 0xFFFFFFFFu;   // a token without bytes is never allowed
    }
    for (;;) {
        const int pe = pb + min(PATTERN_PIECE, span_hi - pb);
#pragma unroll
        for (int j = 0; j < PATTERN_NPT; ++j) {
            const int lo = max(tb[j], pb);
            if (lo < min(te[j], pe)) {
                const int c = s_cls[s_bytes[lo - pb]];
#pragma unroll
                for (int q = 0; q < PATTERN_ITEM_PAIRS; ++q)
                    if ((live_m >> (2 * q)) & 3u) ts[j][q] = pattern_step2(ts[j][q], c, nc, s_trans);
                tb[j] = lo + 1;
            }
        }
#pragma unroll
        for (int j = 0; j < PATTERN_NPT; ++j) {
            const int hi = min(te[j], pe);
            for (int x = max(tb[j], pb); x < hi; ++x) {
                unsigned all = 0xFFFFFFFFu;
#pragma unroll
                for (int q = 0; q < PATTERN_ITEM_PAIRS; ++q) all &= ts[j][q];
                if (all == 0xFFFFFFFFu) break;  // the token is dead under every row
                const int c = s_cls[s_bytes[x - pb]];
#pragma unroll
                for (int q = 0; q < PATTERN_ITEM_PAIRS; ++q)
                    if ((live_m >> (2 * q)) & 3u) ts[j][q] = pattern_step2(ts[j][q], c, nc, s_trans);
            }
        }
        pb += PATTERN_PIECE;
        if (pb >= span_hi) break;               // (uniform in the workgroup)
        __syncthreads();                        // the walk of the piece before is over
        stage(pb);
        __syncthreads();
    }
    // ---- 5. per masked row the tile's allowed ids: the tokens whose walk lived, and end-of-text where the row's state accepts
#pragma unroll
    for (int q = 0; q < PATTERN_ITEM_PAIRS; ++q) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int rb = 2 * q + h;
            if (!((live_m >> rb) & 1u)) continue;
            const bool accepts = (s_st[rb] >> 16) & 1;
#pragma unroll
            for (int j = 0; j < PATTERN_NPT; ++j) {
                const int k = tid + j * PATTERN_THREADS;
                const bool alive = k < n_tok ? ((ts[j][q] >> (16 * h)) & 0xFFFFu) != PATTERN_DEAD : (c0 + k == eot && accepts);
                const unsigned long long m = __ballot(alive);
                if (lane == 0) {
                    s_keep[rb][k >> 5] = (unsigned)m;
                    s_keep[rb][(k >> 5) + 1] = (unsigned)(m >> 32);
                }
            }
        }
    }
    __syncthreads();
    const bool wide = (ldl & 3) == 0 && (reinterpret_cast<unsigned long long>(logits) & 15ull) == 0;
    for (int rb = 0; rb < PATTERN_ITEM_ROWS; ++rb) {
        if (!((live_m >> rb) & 1u)) continue;
        float* lrow = logits + (long)(r0 + rb) * ldl;
        const unsigned* keep_row = s_keep[rb];
        if (wide) {
            // 16-byte pieces, two per thread: piece k covers ids c0 + 4k .. c0 + 4k + 3, all below ldl (a multiple of 4 above eot)
#pragma unroll
            for (int j = 0; j < GRAMMAR_TILE / 4 / PATTERN_THREADS; ++j) {
                const int k = tid + j * PATTERN_THREADS;
                const int col = c0 + 4 * k;
                if (col > eot) break;
                unsigned keep = (keep_row[k >> 3] >> ((k & 7) * 4)) & 0xfu;
                if (col + 3 > eot) keep |= (0xfu << (eot + 1 - col)) & 0xfu;    // ids above end-of-text keep their bits
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
                if (!((keep_row[k >> 5] >> (k & 31)) & 1u)) urow[col] = PATTERN_NEG_INF;
            }
        }
    }
}

void launch_dec_pattern_items(float* logits, const SearchParams* sp_dev, int items, int V, const SearchState& st, const PatternItems& pi,
                              hipStream_t s) {
    const int tiles = (V + GRAMMAR_TILE - 1) / GRAMMAR_TILE;
    hipLaunchKernelGGL(dec_pattern_items_kernel, dim3(tiles, items), dim3(PATTERN_THREADS), 0, s, logits, sp_dev, st, pi);
}

}  // namespace wlx
