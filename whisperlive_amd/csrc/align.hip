// align.hip — word alignment after the decoder pass, on the device (gfx950): from the raw cross-attention scores of the alignment
// heads to the DTW path, for a ragged batch of entries in one launch sequence (wlx_align_batch).
//
// Arithmetic, all float32, in this order (the host restatement is engine_decode.hip align_postprocess, the definition oracle/alignment.py):
//   1. align_softmax_kernel   one wave per (head, token) row: lane l holds frames l, l + 64, ...; max by a 64-lane butterfly; e = expf(s - max);
//                             each lane adds its e in ascending frame order, the lanes' sums meet in a butterfly (xor 32, 16, .. 1);
//                             w = e * (1 / sum), written over the scores.
//   2. align_stats_kernel     one thread per (head, frame): mean = (w_0 + w_1 + ...) / n_tok in token order, then
//                             std = sqrtf(((w_0 - mean)^2 + ...) / n_tok) in token order (two passes, population std).
//   3. align_median_kernel    z = (w - mean) / std (a true division); the median of width mw along time with reflect padding is a SELECTION
//                             (rank counting, no arithmetic); acc += median in head order; x = -(acc / n_heads).
//   4. align_dtw_kernel       cost = x + min(diagonal, up, left) with the definition's three-way comparison: one add per cell.
#include "align.h"
#include <algorithm>
#include <cmath>

namespace wlx {

void align_layout(AlignEnt* ent, int n, int n_heads, AlignPlan* plan) {
    AlignPlan p{};
    for (int e = 0; e < n; ++e) {
        AlignEnt& a = ent[e];
        a.score_off = (long long)p.score_floats; a.stat_off = (long long)p.stat_floats;
        a.x_off = (long long)p.x_floats; a.trace_off = (long long)p.trace_words;
        a.pad_ = 0;
        p.score_floats += (size_t)n_heads * a.n_tok * AL_ROW;
        p.stat_floats += (size_t)n_heads * a.nf * 2;
        p.x_floats += (size_t)a.N * a.nf;
        const size_t tw = (size_t)a.N * ((a.nf + 15) / 16);
        if (tw > (size_t)AL_TRACE_LDS_WORDS) p.trace_words += tw;
        p.max_rows = std::max(p.max_rows, n_heads * a.n_tok);
        p.max_nf = std::max(p.max_nf, a.nf);
        p.max_N = std::max(p.max_N, a.N);
    }
    *plan = p;
}

namespace {

constexpr int SM_K = (AL_MAX_NF + 63) / 64;     // frames a lane of the softmax wave holds

__global__ __launch_bounds__(256) void align_softmax_kernel(const AlignEnt* __restrict__ ent, int n_heads, float* __restrict__ scores) {
    const AlignEnt E = ent[blockIdx.y];
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, nf = E.nf;
    if (r >= n_heads * E.n_tok) return;
    float* p = scores + E.score_off + (size_t)r * AL_ROW;
    float v[SM_K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < SM_K; ++k) {
        const int f = k * 64 + lane;
        v[k] = f < nf ? p[f] : -INFINITY;
        mx = fmaxf(mx, v[k]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SM_K; ++k) {
        v[k] = (k * 64 + lane) < nf ? expf(v[k] - mx) : 0.f;
        sum += v[k];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < SM_K; ++k) {
        const int f = k * 64 + lane;
        if (f < nf) p[f] = v[k] * inv;
    }
}

__global__ __launch_bounds__(256) void align_stats_kernel(const AlignEnt* __restrict__ ent, const float* __restrict__ w, float* __restrict__ stats) {
    const AlignEnt E = ent[blockIdx.z];
    const int f = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, nt = E.n_tok;
    if (f >= E.nf) return;
    const float* p = w + E.score_off + (size_t)h * nt * AL_ROW + f;
    float sum = 0.f;
    for (int t = 0; t < nt; ++t) sum += p[(size_t)t * AL_ROW];
    const float mean = sum / (float)nt;
    float var = 0.f;
    for (int t = 0; t < nt; ++t) { const float d = p[(size_t)t * AL_ROW] - mean; var += d * d; }
    float2* o = reinterpret_cast<float2*>(stats + E.stat_off) + (size_t)h * E.nf + f;
    *o = make_float2(mean, sqrtf(var / (float)nt));
}

constexpr int MED_TT = 4;       // text rows per workgroup: one read of a head's (mean, std) serves four rows

// thread tid stands at frame position g = f0 - PAD + tid (reflected into the row where the median runs); the inner 256 - 2 PAD threads own an output
template <int MW>
__global__ __launch_bounds__(256) void align_median_kernel(const AlignEnt* __restrict__ ent, int n_heads, int n_sot, const float* __restrict__ w,
                                                           const float* __restrict__ stats, float* __restrict__ x) {
    constexpr int PAD = MW / 2, TF = 256 - 2 * PAD;
    __shared__ float zs[2][MED_TT][256];
    const AlignEnt E = ent[blockIdx.z];
    const int nf = E.nf, N = E.N, nt = E.n_tok, tid = threadIdx.x;
    const int f0 = blockIdx.x * TF, i0 = blockIdx.y * MED_TT;
    if (f0 >= nf || i0 >= N) return;                    // (uniform over the workgroup)
    const bool med = MW > 1 && nf > PAD;                // the definition leaves a row no longer than the padding as it is
    const int g = f0 - PAD + tid;
    int r = g;
    if (med) { if (r < 0) r = -r; if (r >= nf) r = 2 * (nf - 1) - r; }
    const bool valid = r >= 0 && r < nf;
    const bool owner = tid >= PAD && tid < 256 - PAD && g < nf;
    const float2* sp = reinterpret_cast<const float2*>(stats + E.stat_off);
    const float* wp = w + E.score_off + (size_t)(n_sot + i0) * AL_ROW + (valid ? r : 0);
    float acc[MED_TT];
#pragma unroll
    for (int tt = 0; tt < MED_TT; ++tt) acc[tt] = 0.f;
    for (int h = 0; h < n_heads; ++h) {
        const float2 ms = valid ? sp[(size_t)h * nf + r] : make_float2(0.f, 1.f);
        float (*zb)[256] = zs[h & 1];
#pragma unroll
        for (int tt = 0; tt < MED_TT; ++tt) {
            const float wv = (valid && i0 + tt < N) ? wp[((size_t)h * nt + tt) * AL_ROW] : 0.f;
            zb[tt][tid] = (wv - ms.x) / ms.y;
        }
        __syncthreads();        // (one per head: the next head writes the other buffer)
        if (owner) {
#pragma unroll
            for (int tt = 0; tt < MED_TT; ++tt) {
                float m = zb[tt][tid];
                if (med) {
                    float v[MW];
#pragma unroll
                    for (int k = 0; k < MW; ++k) v[k] = zb[tt][tid - PAD + k];
#pragma unroll
                    for (int k = 0; k < MW; ++k) {      // v[k] is the PAD-th order statistic iff fewer than PAD + 1 values are below it and more than PAD are not above
                        int lt = 0, le = 0;
#pragma unroll
                        for (int j = 0; j < MW; ++j) { lt += v[j] < v[k] ? 1 : 0; le += v[j] <= v[k] ? 1 : 0; }
                        if (lt <= PAD && PAD < le) m = v[k];
                    }
                }
                acc[tt] += m;
            }
        }
    }
    if (owner) {
#pragma unroll
        for (int tt = 0; tt < MED_TT; ++tt)
            if (i0 + tt < N) x[E.x_off + (size_t)(i0 + tt) * nf + g] = -(acc[tt] / (float)n_heads);
    }
}

// ---- dynamic time warping. Row i of the cost matrix belongs to thread i; at step d it stands at column d - i, so the three cells it needs are
// its own last value (left), row i - 1's last value (up) and row i - 1's value before that (diagonal): the value it took as `up` one step earlier.
// N <= 64: one wave, the neighbour's value by a lane shift, no barrier. N > 64: the values cross through LDS, one barrier per step.
// x is read 16 steps ahead into a register queue indexed by d & 15 (static after unrolling), so a step never waits for memory.
template <bool MULTI>
__device__ __forceinline__ void dtw_forward(const float* __restrict__ x, int N, int M, int W, unsigned* trace, float (*exch)[512]) {
    const int i = threadIdx.x;
    const bool row = i < N;
    const float* xr = x + (size_t)(row ? i : 0) * M;
    const int steps = N + M - 1;
    float q[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int j = k - i; q[k] = (row && j >= 0 && j < M) ? xr[j] : 0.f; }
    float val = INFINITY, diag = i == 0 ? 0.f : INFINITY;
    unsigned tw = 0;
    if (MULTI) { exch[0][i] = INFINITY; exch[1][i] = INFINITY; __syncthreads(); }
    for (int d0 = 0; d0 < steps; d0 += 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int d = d0 + k, j = d - i;
            float up;
            if (MULTI) up = i > 0 ? exch[(d + 1) & 1][i - 1] : INFINITY;
            else { up = __shfl_up(val, 1); if (i == 0) up = INFINITY; }
            if (row && j >= 0 && j < M) {
                const float c0 = diag, c1 = up, c2 = val;
                float cc; unsigned t;
                if (c0 < c1 && c0 < c2) { cc = c0; t = 0; }
                else if (c1 < c0 && c1 < c2) { cc = c1; t = 1; }
                else { cc = c2; t = 2; }
                val = q[k] + cc;
                tw |= t << (2 * (j & 15));
                if ((j & 15) == 15 || j == M - 1) { trace[(size_t)i * W + (j >> 4)] = tw; tw = 0; }
            }
            diag = up;
            const int jn = j + 16;
            q[k] = (row && jn >= 0 && jn < M) ? xr[jn] : 0.f;
            if (MULTI) { exch[d & 1][i] = val; __syncthreads(); }
        }
    }
}

__global__ __launch_bounds__(448) void align_dtw_kernel(const AlignEnt* __restrict__ ent, const float* __restrict__ x, unsigned* __restrict__ gtrace,
                                                        int32_t* __restrict__ ti, int32_t* __restrict__ fi, int path_stride, int32_t* __restrict__ n_path) {
    __shared__ unsigned ltrace[AL_TRACE_LDS_WORDS];
    __shared__ unsigned pathbuf[2048];          // the path as the backtrack meets it (end first): text index | time index << 16
    __shared__ float exch[2][512];
    __shared__ int s_cnt;
    const AlignEnt E = ent[blockIdx.x];
    const int N = E.N, M = E.nf, W = (M + 15) / 16, tid = threadIdx.x;
    unsigned* trace = (size_t)N * W > (size_t)AL_TRACE_LDS_WORDS ? gtrace + E.trace_off : ltrace;
    const float* xe = x + E.x_off;
    if (N > 64) dtw_forward<true>(xe, N, M, W, trace, exch);
    else if (tid < 64) dtw_forward<false>(xe, N, M, W, trace, exch);
    __syncthreads();
    if (tid == 0) {
        int i = N, j = M, cnt = 0;
        while ((i > 0 || j > 0) && cnt < 2048) {
            pathbuf[cnt++] = ((unsigned)(i - 1) & 0xffffu) | ((unsigned)(j - 1) << 16);
            int t;
            if (i == 0) t = 2;
            else if (j == 0) t = 1;
            else t = (int)((trace[(size_t)(i - 1) * W + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u);
            if (t == 0) { --i; --j; } else if (t == 1) --i; else --j;
        }
        s_cnt = cnt;
    }
    __syncthreads();
    const int cnt = s_cnt;
    for (int p = tid; p < cnt && p < path_stride; p += blockDim.x) {
        const unsigned v = pathbuf[cnt - 1 - p];
        ti[(size_t)blockIdx.x * path_stride + p] = (int32_t)(int16_t)(v & 0xffffu);
        fi[(size_t)blockIdx.x * path_stride + p] = (int32_t)v >> 16;
    }
    if (tid == 0) n_path[blockIdx.x] = cnt;
}

template <int MW>
void median_go(const AlignEnt* d_ent, int n, int n_heads, int n_sot, const AlignPlan& plan, const float* w, const float* stats, float* x, hipStream_t st) {
    constexpr int TF = 256 - 2 * (MW / 2);
    hipLaunchKernelGGL(align_median_kernel<MW>, dim3((plan.max_nf + TF - 1) / TF, (plan.max_N + MED_TT - 1) / MED_TT, n), dim3(256), 0, st,
                       d_ent, n_heads, n_sot, w, stats, x);
}

}  // namespace

void launch_align_cost(const AlignEnt* d_ent, int n, int n_heads, int n_sot, int mw, const AlignPlan& plan, float* scores, float* stats, float* x,
                       hipStream_t st) {
    hipLaunchKernelGGL(align_softmax_kernel, dim3((plan.max_rows + 3) / 4, n), dim3(256), 0, st, d_ent, n_heads, scores);
    hipLaunchKernelGGL(align_stats_kernel, dim3((plan.max_nf + 255) / 256, n_heads, n), dim3(256), 0, st, d_ent, scores, stats);
    switch (mw) {
        case 1: median_go<1>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 3: median_go<3>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 5: median_go<5>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 7: median_go<7>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 9: median_go<9>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 11: median_go<11>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        case 13: median_go<13>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
        default: median_go<15>(d_ent, n, n_heads, n_sot, plan, scores, stats, x, st); break;
    }
}

void launch_align_dtw(const AlignEnt* d_ent, int n, int max_N, const float* x, unsigned* trace, int32_t* ti, int32_t* fi, int path_stride,
                      int32_t* n_path, hipStream_t st) {
    const int threads = std::max(64, (max_N + 63) / 64 * 64);
    hipLaunchKernelGGL(align_dtw_kernel, dim3(n), dim3(threads), 0, st, d_ent, x, trace, ti, fi, path_stride, n_path);
}

}  // namespace wlx
