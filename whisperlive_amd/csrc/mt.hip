// mt.hip — the M2M100-specific kernels of the translation engine (mt_engine.hip): token embedding with M2M100's
// sinusoidal positions, the ReLU of the MLP, attention over short variable-length sequences (encoder self-attention,
// decoder cross-attention with per-item source lengths, decoder self-attention through the beam ancestry table), the
// KV-cache append of a decode step and the two-stage log-softmax + top-k front end of the beam search.
#include "mt.h"

#include <math.h>

namespace wlx {

// ---------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void mt_embed_kernel(const int* __restrict__ tok, const int* __restrict__ pos,
                                                       const half_t* __restrict__ Ep, int KT, float scale,
                                                       const float* __restrict__ sinpos, int d, float* __restrict__ x) {
    const int r = blockIdx.x;
    const int n = tok[r], p = pos[r];
    const int c = n & 15, nt = n >> 4;
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        const int kt = k >> 5, g = (k & 31) >> 3, e = k & 7;   // packed fragment element of E[n][k] (common.h)
        const float ev = (float)Ep[(((long)nt * KT + kt) * 64 + g * 16 + c) * 8 + e];
        x[(long)r * d + k] = scale * ev + sinpos[(long)p * d + k];
    }
}

void launch_mt_embed(const int* tok, const int* pos, int rows, const half_t* Ep, int KT, float scale,
                     const float* sinpos, int d, float* x, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(mt_embed_kernel, dim3(rows), dim3(256), 0, s, tok, pos, Ep, KT, scale, sinpos, d, x);
}

// ---------------------------------------------------------------- ReLU
__global__ __launch_bounds__(256) void mt_relu_kernel(half_t* __restrict__ y, long ld, int M, int N) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n8 = N >> 3;
    if (i >= (long)M * n8) return;
    const int m = (int)(i / n8), j = (int)(i - (long)m * n8);
    f16x8* p = reinterpret_cast<f16x8*>(y + (long)m * ld) + j;
    f16x8 v = *p;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] > (half_t)0 ? v[e] : (half_t)0;
    *p = v;
}

void launch_mt_relu_f16(half_t* y, long ld, int M, int N, hipStream_t s) {
    const long total = (long)M * (N >> 3);          // N: the FFN width, a multiple of 64 (validated at engine creation)
    if (total <= 0) return;
    hipLaunchKernelGGL(mt_relu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, y, ld, M, N);
}

// ---------------------------------------------------------------- attention
// One workgroup = NW waves = up to 4 NW query rows of ONE group and one head; each wave owns MT_QW rows (NW = 4 for the encoder and
// the cross-attention of up to 16 beam rows, NW = 1 for the one-row groups of the decoder self-attention). Keys go through LDS in
// tiles of 64 (K transposed, so lane j reads key j's dims conflict-free; V row-major, lane = output dim), shared by every query
// row of the workgroup: the R beam rows of an item read its cross K / V once per tile. Scores and the P.V products are fp32 VALU
// FMAs on fp16 operands (no MFMA: the groups are short — a source is <= 1024 tokens, a decode step has one query row per group —
// and the whole encoder pass takes < 1.1 ms at small100 size). Online softmax in fp32.
#define MT_QW 4
template <int NW>
__global__ __launch_bounds__(NW * 64) void mt_attn_kernel(const half_t* __restrict__ Q, long ldq, const half_t* __restrict__ K,
                                                      long ldk, const half_t* __restrict__ V, long ldv, half_t* __restrict__ O,
                                                      long ldo, const MtAttnGroup* __restrict__ groups,
                                                      const int* __restrict__ anc, int ld_anc, int tmax) {
    __shared__ float qs[NW * MT_QW][64];
    __shared__ half_t kt[64][64 + 2];      // [dim][key]
    __shared__ half_t vs[64][64];          // [key][dim]
    __shared__ float ps[NW][MT_QW][64];
    const MtAttnGroup G = groups[blockIdx.x];
    const int h = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < NW * MT_QW * 64; i += NW * 64) {
        const int qi = i >> 6, dd = i & 63;
        qs[qi][dd] = qi < G.nq ? (float)Q[(long)(G.q0 + qi) * ldq + h * 64 + dd] : 0.f;
    }
    float m[MT_QW], l[MT_QW], acc[MT_QW];
#pragma unroll
    for (int i = 0; i < MT_QW; ++i) { m[i] = -INFINITY; l[i] = 0.f; acc[i] = 0.f; }
    for (int j0 = 0; j0 < G.nk; j0 += 64) {
        __syncthreads();                   // (previous tile fully consumed; first trip: qs written)
#pragma unroll
        for (int u = 0; u < 8 / NW; ++u) {                 // 64 keys x 8 pieces of 16 bytes, NW * 64 pieces per pass
            const int key = (tid >> 3) + 8 * NW * u, c8 = (tid & 7) * 8;
            const int j = j0 + key;
            f16x8 kv = {}, vv = {};
            if (j < G.nk) {
                const long row = anc ? (long)anc[(long)G.q0 * ld_anc + j] * tmax + j : (long)G.k0 + j;
                kv = *reinterpret_cast<const f16x8*>(K + row * ldk + h * 64 + c8);
                vv = *reinterpret_cast<const f16x8*>(V + row * ldv + h * 64 + c8);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) kt[c8 + e][key] = kv[e];
            *reinterpret_cast<f16x8*>(&vs[key][c8]) = vv;
        }
        __syncthreads();
        const bool live = j0 + lane < G.nk;
        float s[MT_QW];
#pragma unroll
        for (int i = 0; i < MT_QW; ++i) s[i] = 0.f;
#pragma unroll 8
        for (int dd = 0; dd < 64; ++dd) {
            const float kd = (float)kt[dd][lane];
#pragma unroll
            for (int i = 0; i < MT_QW; ++i) s[i] += qs[wave * MT_QW + i][dd] * kd;
        }
#pragma unroll
        for (int i = 0; i < MT_QW; ++i) {
            const float si = live ? s[i] : -INFINITY;
            const float mn = fmaxf(m[i], wave_max(si));
            const float p = live ? __expf(si - mn) : 0.f;
            const float corr = m[i] == -INFINITY ? 0.f : __expf(m[i] - mn);
            l[i] = l[i] * corr + wave_sum(p);
            acc[i] *= corr;
            m[i] = mn;
            ps[wave][i][lane] = p;
        }
        __builtin_amdgcn_wave_barrier();   // ps of this wave written before its own lanes read it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int nj = min(64, G.nk - j0);
        for (int j = 0; j < nj; ++j) {
            const float vj = (float)vs[j][lane];
#pragma unroll
            for (int i = 0; i < MT_QW; ++i) acc[i] += ps[wave][i][j] * vj;
        }
    }
#pragma unroll
    for (int i = 0; i < MT_QW; ++i) {
        const int qi = wave * MT_QW + i;
        if (qi < G.nq) O[(long)(G.q0 + qi) * ldo + h * 64 + lane] = (half_t)(l[i] > 0.f ? acc[i] / l[i] : 0.f);
    }
}

void launch_mt_attn(const half_t* Q, long ldq, const half_t* K, long ldk, const half_t* V, long ldv, half_t* O, long ldo,
                    const MtAttnGroup* groups, int n_groups, int max_nq, int heads, const int* anc, int ld_anc, int tmax, hipStream_t s) {
    if (n_groups <= 0) return;
    if (max_nq <= MT_QW)
        hipLaunchKernelGGL(mt_attn_kernel<1>, dim3(n_groups, heads), dim3(64), 0, s, Q, ldq, K, ldk, V, ldv, O, ldo, groups, anc,
                           ld_anc, tmax);
    else
        hipLaunchKernelGGL(mt_attn_kernel<4>, dim3(n_groups, heads), dim3(256), 0, s, Q, ldq, K, ldk, V, ldv, O, ldo, groups, anc,
                           ld_anc, tmax);
}

// ---------------------------------------------------------------- KV-cache append
__global__ __launch_bounds__(256) void mt_kv_append_kernel(const half_t* __restrict__ qkv, long ldqkv, int d,
                                                           half_t* __restrict__ Kc, half_t* __restrict__ Vc, int tmax, int t) {
    const int r = blockIdx.x;
    const long dst = ((long)r * tmax + t) * d;
    for (int c = threadIdx.x * 8; c < d; c += blockDim.x * 8) {
        *reinterpret_cast<f16x8*>(Kc + dst + c) = *reinterpret_cast<const f16x8*>(qkv + (long)r * ldqkv + d + c);
        *reinterpret_cast<f16x8*>(Vc + dst + c) = *reinterpret_cast<const f16x8*>(qkv + (long)r * ldqkv + 2 * d + c);
    }
}

void launch_mt_kv_append(const half_t* qkv, long ldqkv, int rows, int d, half_t* Kc, half_t* Vc, int tmax, int t,
                         hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(mt_kv_append_kernel, dim3(rows), dim3(256), 0, s, qkv, ldqkv, d, Kc, Vc, tmax, t);
}

// ---------------------------------------------------------------- log-softmax + top-k
#define MT_CHUNK_LDS 4096      // vocab <= WLX_MT_CHUNKS * MT_CHUNK_LDS (checked at engine creation)

// block arg-max over (v, idx) pairs: larger value wins, the smaller index on a tie; every thread gets the result
__device__ __forceinline__ void mt_block_argmax(float& v, int& idx, float* rv, int* ri) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi >= 0 && (idx < 0 || oi < idx))) { v = ov; idx = oi; }
    }
    __syncthreads();
    if (lane == 0) { rv[wave] = v; ri[wave] = idx; }
    __syncthreads();
    v = rv[0]; idx = ri[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (rv[w] > v || (rv[w] == v && ri[w] >= 0 && (idx < 0 || ri[w] < idx))) { v = rv[w]; idx = ri[w]; }
}

__global__ __launch_bounds__(256) void mt_topk_chunk_kernel(const float* __restrict__ logits, int vocab, const int* __restrict__ ban,
                                                            const int* __restrict__ nban, int ban_ld, int k,
                                                            float* __restrict__ part, int* __restrict__ cand_idx,
                                                            float* __restrict__ cand_val) {
    __shared__ float vals[MT_CHUNK_LDS];
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int ch = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int cs = (vocab + WLX_MT_CHUNKS - 1) / WLX_MT_CHUNKS;
    const int c0 = ch * cs, n = max(0, min(cs, vocab - c0));
    const float* x = logits + (long)r * vocab + c0;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) { const float v = x[i]; vals[i] = v; mx = fmaxf(mx, v); }
    {   // chunk max, then sum of exp (unmasked: log_softmax precedes the processors)
        float v = mx; int dummy = 0;
        mt_block_argmax(v, dummy, rv, ri);
        mx = v;
    }
    float se = 0.f;
    for (int i = tid; i < n; i += 256) se += __expf(vals[i] - mx);
    se = wave_sum(se);
    __syncthreads();
    if ((tid & 63) == 0) rv[tid >> 6] = se;
    __syncthreads();
    if (tid == 0) {
        part[((long)r * WLX_MT_CHUNKS + ch) * 2 + 0] = mx;
        part[((long)r * WLX_MT_CHUNKS + ch) * 2 + 1] = rv[0] + rv[1] + rv[2] + rv[3];
    }
    __syncthreads();
    const int nb = nban ? nban[r] : 0;
    for (int i = tid; i < nb; i += 256) {
        const int b = ban[(long)r * ban_ld + i] - c0;
        if (b >= 0 && b < n) vals[b] = -INFINITY;
    }
    __syncthreads();
    for (int q = 0; q < k; ++q) {
        float v = -INFINITY; int idx = -1;
        for (int i = tid; i < n; i += 256)
            if (vals[i] > v) { v = vals[i]; idx = i; }
        mt_block_argmax(v, idx, rv, ri);
        if (tid == 0) {
            const long o = ((long)r * WLX_MT_CHUNKS + ch) * k + q;
            cand_val[o] = v;
            cand_idx[o] = idx >= 0 ? c0 + idx : -1;
            if (idx >= 0) vals[idx] = -INFINITY;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mt_topk_merge_kernel(const float* __restrict__ part, const int* __restrict__ cand_idx,
                                                            const float* __restrict__ cand_val, int k,
                                                            float* __restrict__ out_val, int* __restrict__ out_idx) {
    __shared__ float cv[WLX_MT_CHUNKS * WLX_MT_MAXK];
    __shared__ int ci[WLX_MT_CHUNKS * WLX_MT_MAXK];
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int nc = WLX_MT_CHUNKS * k;
    for (int i = tid; i < nc; i += 256) {
        cv[i] = cand_val[(long)r * nc + i];
        ci[i] = cand_idx[(long)r * nc + i];
    }
    float M = -INFINITY;
    for (int c = 0; c < WLX_MT_CHUNKS; ++c) M = fmaxf(M, part[((long)r * WLX_MT_CHUNKS + c) * 2]);
    float Z = 0.f;
    for (int c = 0; c < WLX_MT_CHUNKS; ++c) {
        const float mc = part[((long)r * WLX_MT_CHUNKS + c) * 2], sc = part[((long)r * WLX_MT_CHUNKS + c) * 2 + 1];
        if (mc > -INFINITY) Z += sc * __expf(mc - M);
    }
    const float logZ = M + __logf(Z);
    __syncthreads();
    for (int q = 0; q < k; ++q) {
        // candidates compete by (value, smaller vocabulary index); slot positions carry the index
        float v = -INFINITY; int slot = -1;
        for (int i = tid; i < nc; i += 256) {
            if (ci[i] < 0) continue;
            if (cv[i] > v || (cv[i] == v && (slot < 0 || ci[i] < ci[slot]))) { v = cv[i]; slot = i; }
        }
        int key = slot >= 0 ? ci[slot] : -1;   // reduce on the vocabulary index so that ties resolve identically
        float vv = v;
        mt_block_argmax(vv, key, rv, ri);
        if (tid == 0) {
            out_val[(long)r * k + q] = key >= 0 ? vv - logZ : -INFINITY;
            out_idx[(long)r * k + q] = key;
        }
        __syncthreads();
        if (key >= 0)
            for (int i = tid; i < nc; i += 256)
                if (ci[i] == key) ci[i] = -1;
        __syncthreads();
    }
}

void launch_mt_topk(const float* logits, int rows, int vocab, const int* ban, const int* nban, int ban_ld, int k,
                    float* chunk_scratch, int* chunk_idx_scratch, float* out_val, int* out_idx, hipStream_t s) {
    if (rows <= 0) return;
    float* part = chunk_scratch;                                            // [rows][CHUNKS][2]
    float* cval = chunk_scratch + (long)rows * WLX_MT_CHUNKS * 2;           // [rows][CHUNKS][k]
    hipLaunchKernelGGL(mt_topk_chunk_kernel, dim3(WLX_MT_CHUNKS, rows), dim3(256), 0, s, logits, vocab, ban, nban, ban_ld, k,
                       part, chunk_idx_scratch, cval);
    hipLaunchKernelGGL(mt_topk_merge_kernel, dim3(rows), dim3(256), 0, s, part, chunk_idx_scratch, cval, k, out_val, out_idx);
}

}  // namespace wlx
