// dec_vocab.hip — the final LayerNorm + tied output projection of a decoder step (see decoder.hip for the step as a whole): dec_vocab_kernel,
// its dispatch, and the three functions launch_dec_gemv / dec_gemv_kernel_name (dec_gemv.hip) call: vocab2_ok, vocab2_launch, vocab2_kernel_name.
#include "dec_gemv_internal.h"
#include <algorithm>
#include <cstdio>

namespace wlx {

// ------------------------------------------------------------------ vocabulary projection: final LayerNorm + tied output projection
// (round 4) The one bandwidth-sized launch of a decode step: V x d_model fp16 (80 MB Whisper-small, 133 MB large-v3) against <= 64
// rows. As an instance of dec_gemv2_kernel it was 1621 workgroups that each normalised ALL rows before their 48 KiB of weights
// could be used — 19 us at 5 rows (4.2 TB/s) but 51-80 us at 60 rows (the LayerNorm prologue, not HBM: 1621 x 60 rows x 3 KiB of
// fp32 loads, ~11 ns per wave-level load per CU). Here a workgroup is 8 waves that share ONE LayerNorm of the rows (fp16 rows in
// LDS) and then each wave owns a PAIR of 16-column tiles over the whole K: every weight fragment is loaded once (non-temporal,
// straight into registers, two chunks of KC k-tiles x 2 tiles in flight = 24 KiB per wave) and multiplied against all MT row
// tiles from LDS — no K split, no cross-wave reduction, fp32 logits leave as 16-byte pieces. 203 workgroups for V = 51864: one
// round on 256 CUs. A row's result does not depend on how many rows share the launch (same code, same summation order).
struct VocabParams {
    const float* X; long ldx; const float* gamma; const float* beta;
    const half_t* Wp; int M, N, NT;            // rows, real outputs, 16-column tiles of the packed weights
    float* Y; long ldy;
    const float* slab; long slab_stride;       // SLABS: the rows are X + the WLX_FC2_KS partial-sum slabs of the LAST layer's K-split MLP projection
    WLX_TR_FIELD
};
// SLABS (round 5, one row tile): the last decoder layer's MLP output projection used to stay a single launch because its consumer — this
// projection, then 1621 workgroups that would each have summed the slabs — made the split a loss; as ONE launch with K = 4 d_model it is
// the slowest projection of the step (11-13 us at 5 rows against 4.3 us for the K-split form, profiles/r5b_*). With 203 workgroups that
// share one LayerNorm the slab reads are three small loads per row, so the last layer splits like the others.
template <int KT, int KC, int MT, bool SLABS>
__global__ __launch_bounds__(512) void dec_vocab_kernel(VocabParams p) {
    static_assert(!SLABS || MT == 1, "slab rows: decode steps of one row tile");
    constexpr int K = KT * 32, LNV = (K + 255) / 256, NC = KT / KC, LDXS = K + 8;
    constexpr bool LNT = (K % 256) != 0;                    // d_model 384 = 1.5 x 256: the second float4 unit is live on lanes 0..31 only (see dec_gemv2_kernel)
    static_assert((K % 256 == 0 || K == 384) && KT % KC == 0 && NC % 2 == 0, "d_model a multiple of 256 (or 384); an even number of K chunks");
    constexpr int RPT = (MT == 1) ? 2 : 4;                  // LayerNorm rows a wave requests per trip (8 waves: 16 / 32 rows per trip)
    constexpr int NTRIP = (MT * 16 + 8 * RPT - 1) / (8 * RPT);
    extern __shared__ __attribute__((aligned(16))) half_t vxs[];   // [M][LDXS] fp16 LayerNorm rows
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    WLX_TR_BEGIN();
    const int pair = blockIdx.x * 8 + wave;
    const int t0 = (2 * pair < p.NT) ? 2 * pair : p.NT - 1, t1 = (2 * pair + 1 < p.NT) ? 2 * pair + 1 : p.NT - 1;
    const bool tail_on = !LNT || lane < 32;
    const int tback = LNT ? (tail_on ? 0 : lane) : 0;
    // ---- first trip's rows FIRST (vmcnt retires in order: the LayerNorm must not wait behind the weight stream)
    float4 x[RPT][LNV];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = (wave + 8 * i < p.M) ? wave + 8 * i : p.M - 1;
        const float4* x4 = reinterpret_cast<const float4*>(p.X + (long)r * p.ldx) + lane;
#pragma unroll
        for (int j = 0; j < LNV; ++j) x[i][j] = x4[64 * j - ((j == LNV - 1) ? tback : 0)];
    }
    float4 xsl[SLABS ? WLX_FC2_KS : 1][RPT][LNV];
    if constexpr (SLABS) {
#pragma unroll
        for (int q = 0; q < WLX_FC2_KS; ++q)
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int r = (wave + 8 * i < p.M) ? wave + 8 * i : p.M - 1;
                const float4* s4 = reinterpret_cast<const float4*>(p.slab + q * p.slab_stride + (long)r * p.ldx) + lane;
#pragma unroll
                for (int j = 0; j < LNV; ++j) xsl[q][i][j] = s4[64 * j - ((j == LNV - 1) ? tback : 0)];
            }
    }
    float4 gq[LNV], bq[LNV];
    {
        const float4* g4 = reinterpret_cast<const float4*>(p.gamma) + lane;
        const float4* b4 = reinterpret_cast<const float4*>(p.beta) + lane;
#pragma unroll
        for (int j = 0; j < LNV; ++j) { const int tb = (j == LNV - 1) ? tback : 0; gq[j] = g4[64 * j - tb]; bq[j] = b4[64 * j - tb]; }
    }
    asm volatile("" ::: "memory");                         // compile-time fence: the weight requests stay behind the row requests
    const half_t* wq[2] = {p.Wp + (long)t0 * KT * 512 + lane * 8, p.Wp + (long)t1 * KT * 512 + lane * 8};
    f16x8 wf[2][KC][2];                                     // [ring buffer][k-tile of the chunk][tile of the pair]
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < KC; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) wf[b][j][i] = ld_nt_f16x8(wq[i] + (b * KC + j) * 512);
    constexpr float invK = 1.0f / (float)K;
    auto ln_row = [&](float4 (&xr)[LNV], int r, bool keep) {
        if constexpr (LNT) { if (!tail_on) xr[LNV - 1] = make_float4(0.f, 0.f, 0.f, 0.f); }
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < LNV; ++j) sm += (xr[j].x + xr[j].y) + (xr[j].z + xr[j].w);
        const float mean = dpp_wave_sum(sm) * invK;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < LNV; ++j) {
            xr[j].x -= mean; xr[j].y -= mean; xr[j].z -= mean; xr[j].w -= mean;
            if constexpr (LNT) { if (j == LNV - 1 && !tail_on) xr[j] = make_float4(0.f, 0.f, 0.f, 0.f); }
            q += (xr[j].x * xr[j].x + xr[j].y * xr[j].y) + (xr[j].z * xr[j].z + xr[j].w * xr[j].w);
        }
        const float rstd = rsqrtf(dpp_wave_sum(q) * invK + 1e-5f);
        half_t* dst = vxs + (long)r * LDXS + lane * 4;
#pragma unroll
        for (int j = 0; j < LNV; ++j) {
            const f16x4 hv = {(half_t)(xr[j].x * rstd * gq[j].x + bq[j].x), (half_t)(xr[j].y * rstd * gq[j].y + bq[j].y),
                              (half_t)(xr[j].z * rstd * gq[j].z + bq[j].z), (half_t)(xr[j].w * rstd * gq[j].w + bq[j].w)};
            if (keep && (j < LNV - 1 || tail_on)) *reinterpret_cast<f16x4*>(dst + 256 * j) = hv;
        }
    };
    // first trip: straight-line and unconditional (a wave without a row normalises the clamped row it loaded and keeps nothing)
    if constexpr (SLABS) {                                  // the row = ((x + s0) + s1): the association of every other consumer of the slabs
#pragma unroll
        for (int q = 0; q < WLX_FC2_KS; ++q)
#pragma unroll
            for (int i = 0; i < RPT; ++i)
#pragma unroll
                for (int j = 0; j < LNV; ++j) { x[i][j].x += xsl[q][i][j].x; x[i][j].y += xsl[q][i][j].y; x[i][j].z += xsl[q][i][j].z; x[i][j].w += xsl[q][i][j].w; }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) ln_row(x[i], (wave + 8 * i < p.M) ? wave + 8 * i : p.M - 1, wave + 8 * i < p.M);
#pragma unroll 1
    for (int tr = 1; tr < NTRIP; ++tr) {                    // (49..64 rows, or 33..48: a second trip behind the weight stream)
        const int rb = wave + 8 * RPT * tr;
        if (rb >= p.M) break;
        float4 y[RPT][LNV];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int r = (rb + 8 * i < p.M) ? rb + 8 * i : p.M - 1;
            const float4* x4 = reinterpret_cast<const float4*>(p.X + (long)r * p.ldx) + lane;
#pragma unroll
            for (int j = 0; j < LNV; ++j) y[i][j] = x4[64 * j - ((j == LNV - 1) ? tback : 0)];
        }
#pragma unroll
        for (int i = 0; i < RPT; ++i) ln_row(y[i], (rb + 8 * i < p.M) ? rb + 8 * i : p.M - 1, rb + 8 * i < p.M);
    }
    WLX_TR_MARK(1);
    __syncthreads();
    // ---- the pair's columns over the whole K: chunk ch from ring buffer ch & 1, refilled with chunk ch + 2 behind its MFMAs
    const half_t* xr[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xr[mt] = vxs + (long)((mt * 16 + c < p.M) ? mt * 16 + c : p.M - 1) * LDXS + g * 8;   // rows >= M re-read a valid row (never stored)
    f32x4 acc[2][MT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[i][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            f16x8 xf[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const f16x8*>(xr[mt] + (ch * KC + j) * 32);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[i][mt] = mfma16(wf[ch & 1][j][i], xf[mt], acc[i][mt]);
        }
        if (ch + 2 < NC) {
#pragma unroll
            for (int j = 0; j < KC; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) wf[ch & 1][j][i] = ld_nt_f16x8(wq[i] + ((ch + 2) * KC + j) * 512);
        }
    }
    WLX_TR_MARK(2);
    // ---- fp32 logits: lane (c, g) holds columns g*4 .. g*4+3 of row mt*16 + c
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int nt = 2 * pair + i;
        if (nt >= p.NT) continue;
        const int n = nt * 16 + g * 4;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = mt * 16 + c;
            if (row >= p.M) continue;
            float* yp = p.Y + (long)row * p.ldy + n;
            const f32x4 v = acc[i][mt];
            if (n + 3 < p.N) *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
            else { if (n < p.N) yp[0] = v[0]; if (n + 1 < p.N) yp[1] = v[1]; if (n + 2 < p.N) yp[2] = v[2]; }
        }
    }
    WLX_TR_END(p.trc);
}

template <int KT, int KC, int MT, bool SLABS>
static void vocab_go(const VocabParams& p, hipStream_t s) {
    const size_t shm = (size_t)p.M * (KT * 32 + 8) * sizeof(half_t);
    if (shm > 64 * 1024) {          // > 64 KiB of dynamic LDS: opt in once per device (first launch of a shape happens outside capture)
        static std::atomic<signed char> granted[64] = {};
        lds_optin(reinterpret_cast<const void*>(&dec_vocab_kernel<KT, KC, MT, SLABS>), granted, "the batched vocabulary projection falls back");
    }
    const int pairs = (p.NT + 1) / 2;
    hipLaunchKernelGGL((dec_vocab_kernel<KT, KC, MT, SLABS>), dim3((pairs + 7) / 8), dim3(512), shm, s, p);
}
// ---- THE dispatch of dec_vocab_kernel, as dec_gemv.hip gemv2_dispatch: vocab2_ok, vocab2_launch and vocab2_kernel_name go through it
template <int KT_, int KC_, int MT_, bool SLABS_>
struct VocabArgs { static constexpr int KT = KT_, KC = KC_, MT = MT_; static constexpr bool SLABS = SLABS_; };
// row tiles of one launch: 1..4; rows + slabs: decode steps of one row tile
template <int KT, int KC, class Leaf>
static bool vocab2_dispatch_mt(int MT, bool slabs, Leaf& leaf) {
    if (slabs) return MT == 1 && leaf(VocabArgs<KT, KC, 1, true>{});
    return MT == 1 ? leaf(VocabArgs<KT, KC, 1, false>{}) : MT == 2 ? leaf(VocabArgs<KT, KC, 2, false>{}) : MT == 3 ? leaf(VocabArgs<KT, KC, 3, false>{})
         : MT == 4 ? leaf(VocabArgs<KT, KC, 4, false>{}) : false;
}
// the KT -> KC table, once: the d_model of the Whisper family as an even number of chunks of KC k-tiles
template <class Leaf>
static bool vocab2_dispatch(int KT, int MT, bool slabs, Leaf leaf) {
    switch (KT) {
        case 12: return vocab2_dispatch_mt<12, 3>(MT, slabs, leaf);
        case 16: return vocab2_dispatch_mt<16, 4>(MT, slabs, leaf);
        case 24: return vocab2_dispatch_mt<24, 6>(MT, slabs, leaf);
        case 32: return vocab2_dispatch_mt<32, 4>(MT, slabs, leaf);
        case 40: return vocab2_dispatch_mt<40, 5>(MT, slabs, leaf);
        default: return false;
    }
}
// rows one launch of dec_vocab_kernel takes: its fp16 LayerNorm rows must fit the workgroup's LDS (152 KiB: d_model <= 1024 64 rows,
// large-v3 60 -> 48 = three whole row tiles). A wider pass (round 5: up to WLX_MAX_DEC_ROWS rows per step) runs as consecutive row
// chunks, each streaming the weights again (Whisper-small 80 MB = ~25 us per 64 rows of a ~1 ms step).
static int vocab2_chunk_rows(int K) {
    int r = 64;
    while (r > 16 && (size_t)r * (K + 8) * sizeof(half_t) > WLX_G2_LDS_MAX) r -= 16;
    return r;
}
bool vocab2_ok(const GemvParams& p) {
    if (g_decode_v1 || p.in_mode != GEMV_IN_LN || p.out_mode != GEMV_OUT_F32 || p.bias || p.Mtot != 0) return false;
    if (p.xsrc != GEMV_X_PLAIN && !(p.xsrc == GEMV_X_SLABS && p.M <= 16 && p.slab != nullptr)) return false;   // rows + slabs: decode steps of one row tile
    if (p.M < 1 || p.M > WLX_MAX_DEC_ROWS || p.K != p.KT * 32 || p.N < 256) return false;
    const int rows = std::min(p.M, vocab2_chunk_rows(p.K));
    if (!vocab2_dispatch(p.KT, (rows + 15) / 16, p.xsrc == GEMV_X_SLABS, [](auto) { return true; })) return false;
    const size_t shm = (size_t)rows * (p.K + 8) * sizeof(half_t);
    if (shm > 64 * 1024 && g_lds_optin_refused.load(std::memory_order_relaxed)) return false;   // the device refused the raised LDS limit once: general kernel
    return shm <= WLX_G2_LDS_MAX;
}
void vocab2_launch(const GemvParams& g, hipStream_t s) {
    const int CH = vocab2_chunk_rows(g.K);
    for (int r0 = 0; r0 < g.M; r0 += CH) {
        VocabParams p{};
        p.X = g.X + (long)r0 * g.ldx; p.ldx = g.ldx; p.gamma = g.gamma; p.beta = g.beta; p.Wp = g.Wp; p.M = std::min(CH, g.M - r0); p.N = g.N; p.NT = (g.N + 15) / 16;
        p.Y = g.Y + (long)r0 * g.ldy; p.ldy = g.ldy;
        if (g.xsrc == GEMV_X_SLABS) { p.slab = g.slab; p.slab_stride = g.slab_stride; }
#ifdef WLX_TRACE
        p.trc = trace_next("vocab2");
#endif
        const bool launched = vocab2_dispatch(g.KT, (p.M + 15) / 16, g.xsrc == GEMV_X_SLABS, [&](auto a) { using A = decltype(a); vocab_go<A::KT, A::KC, A::MT, A::SLABS>(p, s); return true; });
        if (!launched) { dispatch_bug("dec_vocab_kernel", s); return; }
    }
}
// the name leaf: the template arguments of the instantiation vocab2_launch runs for the first row chunk
const char* vocab2_kernel_name(const GemvParams& p) {
    static thread_local char buf[64];
    vocab2_dispatch(p.KT, (std::min(p.M, vocab2_chunk_rows(p.K)) + 15) / 16, p.xsrc == GEMV_X_SLABS,
                    [&](auto a) { using A = decltype(a); snprintf(buf, sizeof(buf), "dec_vocab_kernel<%d, %d, %d>", A::KT, A::KC, A::MT); return true; });
    return buf;
}

}  // namespace wlx
