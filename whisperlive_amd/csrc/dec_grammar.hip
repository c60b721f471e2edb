// dec_grammar.hip — grammar-constrained decoding: the one launch between the vocabulary projection and the token search of a decode step
// whose slot has a grammar installed (wlx_grammar_set). A step of a slot without one does not launch it.
//
// The grammar is a DFA over token ids, determinised on the host (whisperlive_amd/grammar.py): state n carries the sorted list of its edges
// (token, next state) and an accept flag. Row r at position p is in state next(state of its parent row at p - 1, token fed at p), kept per
// (cache row, position) like the bias states (dec_bias.hip), so it follows the beam's re-ordering; a special or timestamp token (>= eot)
// keeps the parent's state, a text token without an edge (a caller-forced prefix) restarts at state 0. The row's logits then lose every
// text token that is no edge of its state, and end-of-text unless the state accepts: those words become -inf (0xff800000), all others keep
// their bits. No arithmetic touches a logit.
//
// Shape: one workgroup of 256 threads per (row, tile of GRAMMAR_TILE ids). Every workgroup of a row walks to the row's state itself — it
// reads the parent's state at p - 1, a word no workgroup of this launch writes (the rows of an item share a position) — and the workgroup
// of tile 0 alone stores it. The allowed set of a tile is a bitmap in LDS (64 words) that the threads fill from the state's edge list; a
// 16-byte piece with no allowed id is stored without being read, one with all four allowed is not touched at all.
#include "decoder.h"
#include "grammar_table.h"
#include "host.h"

namespace wlx {

#define GRAMMAR_THREADS 256
#define GRAMMAR_NEG_INF 0xff800000u

__global__ __launch_bounds__(GRAMMAR_THREADS) void dec_grammar_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp,
                                                                      SearchState st, GrammarTable g) {
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
    // (every return above depends on the row and the tile alone: the workgroup is whole at each barrier below)
    const int n_states = g.block[0];
    const int* edge_off = g.block + GRAMMAR_OFF_AT;
    const int* edge_tok = g.block + GRAMMAR_TOK_AT;
    const int* edge_next = g.block + GRAMMAR_NEXT_AT;
    __shared__ int s_state;
    __shared__ unsigned s_keep[GRAMMAR_TILE / 32];
    if (tid == 0) s_state = 0;
    if (tid < GRAMMAR_TILE / 32) s_keep[tid] = 0u;
    // ---- the row's state: the start state while the fed token is a prompt token (the first generated position)
    int ps = 0;
    const bool generated = p >= plen && p >= 1;
    if (generated) {
        const int parent = st.anc[(long)r * WLX_T_TEXT + p - 1];
        ps = g.state[(long)parent * WLX_T_TEXT + p - 1];
        if (ps < 0 || ps >= n_states) ps = 0;   // (a state another grammar or a bias table left behind: never indexes past this one)
    }
    __syncthreads();
    if (generated && tok < eot) {               // a text token: its edge, or the start state (the tokens of a state are distinct: one hit at most)
        const int lo = edge_off[ps], hi = edge_off[ps + 1];
        for (int i = lo + tid; i < hi; i += GRAMMAR_THREADS)
            if (edge_tok[i] == tok) s_state = edge_next[i];
    } else if (generated && tid == 0) s_state = ps;     // a special or a timestamp is transparent: the parent's state
    __syncthreads();
    const int state = s_state;
    if (blockIdx.x == 0 && tid == 0) g.state[(long)r * WLX_T_TEXT + p] = (short)state;
    // a row whose RAW distribution defines no_speech_prob inside the search keeps its logits as they are
    if (st.nsp_row[r] > 0) return;
    // ---- the tile's allowed ids: the state's edge tokens, and end-of-text where the state accepts
    const int e0 = edge_off[state], e1 = edge_off[state + 1];
    for (int i = e0 + tid; i < e1; i += GRAMMAR_THREADS) {
        const unsigned t = (unsigned)(edge_tok[i] - c0);
        if (t < (unsigned)GRAMMAR_TILE) atomicOr(&s_keep[t >> 5], 1u << (t & 31));
    }
    if (tid == 0 && (unsigned)(eot - c0) < (unsigned)GRAMMAR_TILE && g.block[GRAMMAR_ACCEPT_AT + state])
        atomicOr(&s_keep[(eot - c0) >> 5], 1u << ((eot - c0) & 31));
    __syncthreads();
    float* lrow = logits + (long)r * ldl;
    if ((ldl & 3) == 0 && (reinterpret_cast<unsigned long long>(logits) & 15ull) == 0) {
        // 16-byte pieces: piece k covers ids c0 + 4k .. c0 + 4k + 3, all below ldl (a multiple of 4 above eot)
        for (int k = tid; k < GRAMMAR_TILE / 4; k += GRAMMAR_THREADS) {
            const int col = c0 + 4 * k;
            if (col > eot) break;
            unsigned keep = (s_keep[k >> 3] >> ((k & 7) * 4)) & 0xfu;
            if (col + 3 > eot) keep |= (0xfu << (eot + 1 - col)) & 0xfu;        // ids above end-of-text keep their bits
            if (keep == 0xfu) continue;
            uint4* q = reinterpret_cast<uint4*>(lrow + col);
            uint4 v = make_uint4(GRAMMAR_NEG_INF, GRAMMAR_NEG_INF, GRAMMAR_NEG_INF, GRAMMAR_NEG_INF);
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
        // rows that are not 16-byte aligned (no row stride of the engine's): one word per thread
        unsigned* urow = reinterpret_cast<unsigned*>(lrow);
        for (int k = tid; k < GRAMMAR_TILE; k += GRAMMAR_THREADS) {
            const int col = c0 + k;
            if (col > eot) break;
            if (!((s_keep[k >> 5] >> (k & 31)) & 1u)) urow[col] = GRAMMAR_NEG_INF;
        }
    }
}

void launch_dec_grammar(float* logits, const SearchParams* sp_dev, int rows, int V, const SearchState& st, const GrammarTable& g, hipStream_t s) {
    const int tiles = (V + GRAMMAR_TILE - 1) / GRAMMAR_TILE;
    hipLaunchKernelGGL(dec_grammar_kernel, dim3(tiles, rows), dim3(GRAMMAR_THREADS), 0, s, logits, sp_dev, st, g);
}

}  // namespace wlx
