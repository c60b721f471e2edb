// align.h — word alignment's post-processing on the device (align.hip): cost matrix + dynamic time warping of a ragged batch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace wlx {

constexpr int AL_MAX_TOK = 448;        // tokens of one entry (WLX_T_TEXT)
constexpr int AL_MAX_NF = 1500;        // frames of one entry (WLX_T_AUDIO)
constexpr int AL_ROW = 1536;           // floats per (head, token) row of raw scores (WLX_T_AUDIO_PAD, as dec_align_scores_kernel writes them)
constexpr int AL_TRACE_LDS_WORDS = 12288;   // a DTW trace of up to 48 KiB stays in LDS, a larger one goes to the entry's global scratch

// one entry of a batch. Offsets in elements of their buffers: scores [n_heads][n_tok][AL_ROW], stats [n_heads][nf][2] (mean, std),
// x [N][nf] (the DTW cost), trace [N][ceil(nf / 16)] words of 2 bits per cell (only where it does not fit LDS).
struct AlignEnt {
    long long score_off, stat_off, x_off, trace_off;
    int n_tok, nf, N, pad_;
};
struct AlignPlan {
    size_t score_floats, stat_floats, x_floats, trace_words;
    int max_rows, max_nf, max_N;
};

// fills the offsets of `ent` (n_tok, nf, N given) back to back and the totals. n_heads == 0: DTW alone (x and trace only).
void align_layout(AlignEnt* ent, int n, int n_heads, AlignPlan* plan);
// raw scores -> x (softmax over frames IN PLACE in `scores`, token-axis mean / std, normalise, median of odd width mw <= 15, head mean, negate)
void launch_align_cost(const AlignEnt* d_ent, int n, int n_heads, int n_sot, int mw, const AlignPlan& plan, float* scores, float* stats,
                       float* x, hipStream_t st);
// one workgroup per entry: forward pass, trace, backtrack; path rows at e * path_stride of ti / fi, its length in n_path[e]
void launch_align_dtw(const AlignEnt* d_ent, int n, int max_N, const float* x, unsigned* trace, int32_t* ti, int32_t* fi, int path_stride,
                      int32_t* n_path, hipStream_t st);

}  // namespace wlx
