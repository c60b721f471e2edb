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

}  // namespace wlx
