// mt.h — launchers of the gfx950 kernels of the M2M100 translation engine (mt.hip; engine in mt_engine.hip).
// The projections go through the encoder GEMM of gemm.hip (launch_gemm, GEMM_STORE_F16 / GEMM_RESID_F32) and the
// LayerNorms through launch_layernorm_f16; what is M2M100-specific lives here.
#pragma once
#include "kernels.h"

namespace wlx {

#define WLX_MT_MAX_SRC 1024      // max_position_embeddings of M2M100 / small100
#define WLX_MT_MAXK 32           // candidates per decoder row of the search: 2 x num_beams, num_beams <= 16
#define WLX_MT_CHUNKS 64         // vocabulary chunks of the first top-k stage

// x[r][:] = scale * E[tok[r]][:] + sinpos[pos[r]][:]  (fp32 rows of the residual stream). E is the PACKED fp16 image of
// the shared embedding (launch_pack_linear layout, KT k-tiles), sinpos fp32 [n_pos][d].
void launch_mt_embed(const int* tok, const int* pos, int rows, const half_t* Ep, int KT, float scale,
                     const float* sinpos, int d, float* x, hipStream_t s);

// y = max(y, 0) over an fp16 [M][N] matrix with row stride ld (the ReLU of M2M100's MLP, behind a GEMM_STORE_F16)
void launch_mt_relu_f16(half_t* y, long ld, int M, int N, hipStream_t s);

// Attention, head_dim 64, non-causal, fp16 operands, fp32 softmax and accumulation. Group g owns query rows
// [q0, q0 + nq) and key rows [k0, k0 + nk) (rows of Q / K / V with strides ldq / ldk / ldv; head h at column 64 h).
// With `anc` (decoder self-attention, KV cache with the beam ancestry table): key j of group g lives in row
// anc[g * ld_anc + j] * tmax + j of K / V. Q is pre-scaled (1/8 folded into q_proj). grid = groups x heads. max_nq: the largest nq of
// the launch (<= 16), which sets the workgroup's wave count.
struct MtAttnGroup { int q0, nq, k0, nk; };
void launch_mt_attn(const half_t* Q, long ldq, const half_t* K, long ldk, const half_t* V, long ldv, half_t* O, long ldo,
                    const MtAttnGroup* groups, int n_groups, int max_nq, int heads, const int* anc, int ld_anc, int tmax, hipStream_t s);

// k / v of the decode step's rows (columns [d, 3d) of the fused qkv rows) -> row r * tmax + t of the layer's caches
void launch_mt_kv_append(const half_t* qkv, long ldqkv, int rows, int d, half_t* Kc, half_t* Vc, int tmax, int t,
                         hipStream_t s);

// Search front end over fp32 logits [rows][vocab]: per row the log-partition function of the UNMASKED logits (log_softmax
// comes before the logits processors in Hugging Face's beam search) and the top-k of the logits with the row's banned
// tokens (no_repeat_ngram, ban[r][0..nban[r]) ) at -inf. out_val[r][k] = logit - logZ (log-probability), out_idx[r][k].
// Two launches: chunks of the vocabulary, then a merge per row. k <= WLX_MT_MAXK.
void launch_mt_topk(const float* logits, int rows, int vocab, const int* ban, const int* nban, int ban_ld, int k,
                    float* chunk_scratch, int* chunk_idx_scratch, float* out_val, int* out_idx, hipStream_t s);

// ---- device search (mt_search.hip): Hugging Face's _beam_search / greedy bookkeeping of mt_engine.hip run_generate, statement for
// statement, on state that stays on the device for a whole generate. Iteration i of the search (i = 0 .. max_length - 2) feeds position
// t = i with cur_len = i + 1 tokens per row; sequences, finished sequences and the ancestry table are double-buffered on the parity
// of i (iteration i reads buffer i & 1 and writes the other; greedy search keeps sequences in buffer 0).
struct MtSearchParams {
    int B, R, ML, T, V;                 // items, beams per item, max_length (the row stride of the sequence tables), ancestry stride, vocabulary
    int eos, pad, start, forced_eos;    // forced_eos < 0: none
    int nng, early_stopping, lp_positive, ban_ld;
};
struct MtSearchState {
    int* run[2];                        // running sequences [rows][ML], decoder start included
    int* fin[2];                        // finished sequences [rows][ML]
    float *run_score, *fin_score;       // [rows]
    int *fin_len, *fin_done;            // [rows]
    int *unsat, *item_done;             // [B]
    float* greedy_score;                // [B]
    int* anc[2];                        // beam ancestry [rows][T]
    int *tok, *pos;                     // next step's decoder input [rows]
    MtAttnGroup* gself;                 // next step's self-attention groups [rows]: {r, 1, 0, t + 1}
    int *ban, *nban;                    // no_repeat_ngram bans of the next top-k [rows][ban_ld], [rows]
    const float* lp;                    // lp[len] = (float)pow(len, length_penalty), len = 1 .. ML (host-made: the device only divides)
    int* ctl;                           // device words: done, arrival counter, step flags, cur_len, decode steps
    int* h_done;                        // PINNED host words: done, cur_len, decode steps — stored after the results below
    int* h_n;                           // pinned results [B]: generated tokens (decoder start and final EOS excluded)
    float* h_score;                     // pinned results [B]
    int* h_tok;                         // pinned results [B][ML]
};
// resets the whole state for a generate of P.B items (rows = B * R workgroups)
void launch_mt_search_init(const MtSearchParams& P, const MtSearchState& S, hipStream_t s);
// ban / nban of iteration i from the running sequences: the rule, order and ban_ld truncation of run_generate's banned_ngrams
void launch_mt_search_bans(const MtSearchParams& P, const MtSearchState& S, int i, hipStream_t s);
// iteration i of the search over the top-k candidates tk_val / tk_idx [rows][K] (K = 1 greedy, 2 R beam search; unread when
// `force_now`: the forced EOS at max_length - 1 takes no decode step). One workgroup per item; the workgroup that arrives last
// evaluates the group's stop condition and, when the generate is over, stores the results and then the done words. A launch that
// finds the group done changes nothing.
void launch_mt_search_step(const MtSearchParams& P, const MtSearchState& S, const float* tk_val, const int* tk_idx, int i,
                           int force_now, hipStream_t s);

}  // namespace wlx
