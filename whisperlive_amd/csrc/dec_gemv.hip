// dec_gemv.hip — the skinny GEMMs of a decoder step (see decoder.hip for the step as a whole): the first-generation dec_gemv_kernel (the
// fallback for widths the lean kernel refuses), the lean dec_gemv2_kernel with its staging helpers, the host rules that pick an instantiation
// (gemv2_cfg*, gemv_chunked) and the one dispatch walk that probe, launch and name go through. launch_dec_gemv hands the final LayerNorm +
// vocabulary projection to dec_vocab.hip.
#include "dec_gemv_internal.h"
#include <algorithm>
#include <cstdio>

namespace wlx {

// ------------------------------------------------------------------ skinny GEMM ("GEMV") with fused prologue/epilogue
#define GV_CH 6   // k-tiles per register chunk

template <int MT, int NTB, int IN>
__global__ __launch_bounds__(512) void dec_gemv_kernel(GemvParams p) {
    if (p.done && *p.done) return;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nw = blockDim.x >> 6;
    const int KT = p.KT;
    const int KTW = (KT + nw - 1) / nw;
    const int kt0 = wave * KTW;
    const int kt1 = (kt0 + KTW < KT) ? kt0 + KTW : KT;
    const int NT_total = (p.N + 15) >> 4;

    const half_t* wbase[NTB];
#pragma unroll
    for (int i = 0; i < NTB; ++i) {
        int nt = blockIdx.x * NTB + i;
        if (nt >= NT_total) nt = NT_total - 1;
        wbase[i] = p.Wp + ((long)nt * KT * 64 + lane) * 8;
    }

    f32x4 acc[NTB][MT];
#pragma unroll
    for (int i = 0; i < NTB; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[i][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- issue the first chunk of weight-fragment loads before anything else
    f16x8 wf[GV_CH][NTB];
#pragma unroll
    for (int j = 0; j < GV_CH; ++j) {
        int kt = kt0 + j;
        if (kt > KT - 1) kt = KT - 1;
#pragma unroll
        for (int i = 0; i < NTB; ++i) wf[j][i] = ld_f16x8(wbase[i] + (long)kt * 512);
    }

    f16x8 xf[GV_CH][MT];
    float* red = smem;                         // [2][nw][MT*16]
    float* accred = smem + 2 * nw * MT * 16;   // [nw][NTB*MT][64][4]

    if constexpr (IN == GEMV_IN_LN) {
        // LayerNorm over K = d_model of every live row, statistics shared through LDS.
        // (host guarantees KTW <= GV_CH in this mode: one chunk per wave)
        const float invK = 1.0f / (float)p.K;
        float mean[MT], rstd[MT];
        if constexpr (MT == 1) {
            float xr[GV_CH][8];
            const bool rowok = c < p.M;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                const int kt = kt0 + j;
                if (kt < kt1 && rowok) {
                    const float4* xp = reinterpret_cast<const float4*>(p.X + (long)c * p.ldx + kt * 32 + g * 8);
                    float4 a = xp[0], b = xp[1];
                    xr[j][0] = a.x; xr[j][1] = a.y; xr[j][2] = a.z; xr[j][3] = a.w;
                    xr[j][4] = b.x; xr[j][5] = b.y; xr[j][6] = b.z; xr[j][7] = b.w;
#pragma unroll
                    for (int e = 0; e < 8; ++e) s += xr[j][e];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) xr[j][e] = 0.f;
                }
            }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (g == 0) red[wave * 16 + c] = s;
            __syncthreads();
            float tot = 0.f;
            for (int w = 0; w < nw; ++w) tot += red[w * 16 + c];
            mean[0] = tot * invK;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                if (kt0 + j < kt1 && rowok) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { float dlt = xr[j][e] - mean[0]; q += dlt * dlt; }
                }
            }
            q += __shfl_xor(q, 16, 64);
            q += __shfl_xor(q, 32, 64);
            if (g == 0) red[nw * 16 + wave * 16 + c] = q;
            __syncthreads();
            float qt = 0.f;
            for (int w = 0; w < nw; ++w) qt += red[nw * 16 + w * 16 + c];
            rstd[0] = rsqrtf(qt * invK + 1e-5f);
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                const int kt = kt0 + j;
                f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kt < kt1 && rowok) {
                    const float4* gp = reinterpret_cast<const float4*>(p.gamma + kt * 32 + g * 8);
                    const float4* bp = reinterpret_cast<const float4*>(p.beta + kt * 32 + g * 8);
                    float4 g0 = gp[0], g1 = gp[1], b0 = bp[0], b1 = bp[1];
                    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (half_t)((xr[j][e] - mean[0]) * rstd[0] * gg[e] + bb[e]);
                }
                xf[j][0] = o;
            }
        } else {
            // MT > 1 (prefill / batched rows): three passes over x (L1/L2 resident) instead of
            // holding MT*48 raw floats in registers.
            float s[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                s[mt] = 0.f;
                const int m = mt * 16 + c;
                if (m < p.M)
                    for (int kt = kt0; kt < kt1; ++kt) {
                        const float4* xp = reinterpret_cast<const float4*>(p.X + (long)m * p.ldx + kt * 32 + g * 8);
                        float4 a = xp[0], b = xp[1];
                        s[mt] += a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
                    }
                s[mt] += __shfl_xor(s[mt], 16, 64);
                s[mt] += __shfl_xor(s[mt], 32, 64);
                if (g == 0) red[(wave * MT + mt) * 16 + c] = s[mt];
            }
            __syncthreads();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float tot = 0.f;
                for (int w = 0; w < nw; ++w) tot += red[(w * MT + mt) * 16 + c];
                mean[mt] = tot * invK;
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float q = 0.f;
                const int m = mt * 16 + c;
                if (m < p.M)
                    for (int kt = kt0; kt < kt1; ++kt) {
                        const float4* xp = reinterpret_cast<const float4*>(p.X + (long)m * p.ldx + kt * 32 + g * 8);
                        float4 a = xp[0], b = xp[1];
                        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) { float dlt = v[e] - mean[mt]; q += dlt * dlt; }
                    }
                q += __shfl_xor(q, 16, 64);
                q += __shfl_xor(q, 32, 64);
                if (g == 0) red[nw * MT * 16 + (wave * MT + mt) * 16 + c] = q;
            }
            __syncthreads();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float qt = 0.f;
                for (int w = 0; w < nw; ++w) qt += red[nw * MT * 16 + (w * MT + mt) * 16 + c];
                rstd[mt] = rsqrtf(qt * invK + 1e-5f);
            }
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                const int kt = kt0 + j;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int m = mt * 16 + c;
                    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (kt < kt1 && m < p.M) {
                        const float4* xp = reinterpret_cast<const float4*>(p.X + (long)m * p.ldx + kt * 32 + g * 8);
                        const float4* gp = reinterpret_cast<const float4*>(p.gamma + kt * 32 + g * 8);
                        const float4* bp = reinterpret_cast<const float4*>(p.beta + kt * 32 + g * 8);
                        float4 a = xp[0], b = xp[1], g0 = gp[0], g1 = gp[1], b0 = bp[0], b1 = bp[1];
                        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[e] = (half_t)((v[e] - mean[mt]) * rstd[mt] * gg[e] + bb[e]);
                    }
                    xf[j][mt] = o;
                }
            }
        }
    }

    for (int base = kt0; base < kt1; base += GV_CH) {
        if constexpr (IN == GEMV_IN_F16) {
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                const int kt = base + j;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int m = mt * 16 + c;
                    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (kt < kt1 && m < p.M) o = ld_f16x8(p.Xh + (long)m * p.ldxh + kt * 32 + g * 8);
                    xf[j][mt] = o;
                }
            }
        } else if constexpr (IN == GEMV_IN_XATTN) {
            // combine the WLX_XSPLIT partials of the cross attention: per split a NORMALISED fp16 O row and fp32 (m, l)
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                const int kt = base + j;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int m = mt * 16 + c;
                    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (kt < kt1 && m < p.M) {
                        const int k = kt * 32 + g * 8;
                        const int h = k >> 6, dd = k & 63;
                        const int item = m / p.R, qi = m - item * p.R;
                        const long ih = (long)item * p.H + h;
                        const float* mlp = p.part_ml + (ih * 16 + qi) * (WLX_XSPLIT * 2);
                        float wsp[WLX_XSPLIT];
                        float mmax = WLX_NEG_INF, den = 0.f;
#pragma unroll
                        for (int sp = 0; sp < WLX_XSPLIT; ++sp) mmax = fmaxf(mmax, mlp[sp * 2]);
#pragma unroll
                        for (int sp = 0; sp < WLX_XSPLIT; ++sp) { wsp[sp] = __expf(mlp[sp * 2] - mmax) * mlp[sp * 2 + 1]; den += wsp[sp]; }
                        float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int sp = 0; sp < WLX_XSPLIT; ++sp) {
                            const f16x8 ov = ld_f16x8(p.part_o + ((ih * WLX_XSPLIT + sp) * 16 + qi) * 64 + dd);
#pragma unroll
                            for (int e = 0; e < 8; ++e) num[e] += wsp[sp] * (float)ov[e];
                        }
                        const float inv = 1.0f / den;
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[e] = (half_t)(num[e] * inv);
                    }
                    xf[j][mt] = o;
                }
            }
        }
        // prefetch the next chunk of weights (wave-uniform branch)
        f16x8 wn[GV_CH][NTB];
        const bool more = base + GV_CH < kt1;
        if (more) {
#pragma unroll
            for (int j = 0; j < GV_CH; ++j) {
                int kt = base + GV_CH + j;
                if (kt > KT - 1) kt = KT - 1;
#pragma unroll
                for (int i = 0; i < NTB; ++i) wn[j][i] = ld_f16x8(wbase[i] + (long)kt * 512);
            }
        }
#pragma unroll
        for (int j = 0; j < GV_CH; ++j) {
            if (base + j < kt1) {
#pragma unroll
                for (int i = 0; i < NTB; ++i)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[i][mt] = mfma16(wf[j][i], xf[j][mt], acc[i][mt]);
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < GV_CH; ++j)
#pragma unroll
                for (int i = 0; i < NTB; ++i) wf[j][i] = wn[j][i];
        }
    }

    // ---- cross-wave K reduction through LDS
#pragma unroll
    for (int i = 0; i < NTB; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            *reinterpret_cast<f32x4*>(accred + (((long)wave * (NTB * MT) + (i * MT + mt)) * 64 + lane) * 4) = acc[i][mt];
    __syncthreads();

    for (int pair = wave; pair < NTB * MT; pair += nw) {
        const int i = pair / MT, mt = pair - i * MT;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int w = 0; w < nw; ++w) {
            f32x4 t = *reinterpret_cast<const f32x4*>(accred + (((long)w * (NTB * MT) + pair) * 64 + lane) * 4);
            v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
        }
        const int ntile = blockIdx.x * NTB + i;
        if (ntile >= NT_total) continue;
        const int n = ntile * 16 + g * 4;
        const int m = mt * 16 + c;
        if (m >= p.M) continue;
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = v[r] + ((p.bias && n + r < p.N) ? p.bias[n + r] : 0.f);
        switch (p.out_mode) {
            case GEMV_OUT_F16:
            case GEMV_OUT_GELU_F16: {
                if (p.out_mode == GEMV_OUT_GELU_F16) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = gelu_erf(o[r]);
                }
                f16x4 h = {(half_t)(o[0] * p.qscale), (half_t)(o[1] * p.qscale),
                           (half_t)(o[2] * p.qscale), (half_t)(o[3] * p.qscale)};   // qscale = 1 unless a q projection
                *reinterpret_cast<f16x4*>(p.Yh + (long)m * p.ldyh + n) = h;
            } break;
            case GEMV_OUT_F32: {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < p.N) p.Y[(long)m * p.ldy + n + r] = o[r];
            } break;
            case GEMV_OUT_RESID: {
                float4* xp = reinterpret_cast<float4*>(p.Xres + (long)m * p.ldxres + n);
                float4 t = *xp;
                t.x += o[0]; t.y += o[1]; t.z += o[2]; t.w += o[3];
                *xp = t;
            } break;
            case GEMV_OUT_QKV: {
                if (n < p.d) {
                    f16x4 h = {(half_t)(o[0] * p.qscale), (half_t)(o[1] * p.qscale),
                               (half_t)(o[2] * p.qscale), (half_t)(o[3] * p.qscale)};
                    *reinterpret_cast<f16x4*>(p.Yh + (long)m * p.ldyh + n) = h;
                } else {
                    f16x4 h = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
                    const long off = (long)p.row_cache[m] * p.cache_row_stride + (long)p.row_pos[m] * p.d;
                    if (n < 2 * p.d) *reinterpret_cast<f16x4*>(p.Kc + off + (n - p.d)) = h;
                    else *reinterpret_cast<f16x4*>(p.Vc + off + (n - 2 * p.d)) = h;
                }
            } break;
            default: break;
        }
    }
}

// ------------------------------------------------------------------ third generation: the LEAN skinny GEMM
// Measured on MI355X (scripts/ubench/chain3.hip): a dependent chain of 48-workgroup launches that stream
// 1.2 MB each costs 2.0 us per launch, and every KiB of straight-line code a launch executes adds ~0.4 us — the
// instruction cache is cold at every launch and cold code is fetched at ~3 GB/s, before or after the loads are issued.
// dec_gemv1_kernel is 5-7 KiB of fully unrolled, clamped, 64-bit-indexed code: 2-3 us of instruction fetch per launch,
// more than its HBM time. This kernel executes ~1 KiB:
//   * the wave's K slice is EXACT (host picks nw x CH x NCH == KT), so no clamps or predicates: loads are
//     base + immediate offset; rows >= M are never masked — MFMA output column j depends only on B column j, and
//     columns >= M are simply not stored;
//   * LayerNorm rows are reduced with DPP adds (12 VALU ops) instead of 12 dependent ds_bpermute round trips;
//   * everything rarely needed (ragged K, M > 16, d_model not a multiple of 256) stays in the older kernels.
__device__ __forceinline__ float wave_sum_dpp(float v) { return dpp_wave_sum(v); }   // common.h: 6 v_add_f32_dpp

// copy M rows x K fp16 (16-byte units) global -> LDS rows of stride ldxs for ONE WAVE's own K slice (round 6, log G2): wave w copies columns [0, K) of
// the M rows of ITS slice (X and xs already point at the slice) with its 64 lanes and is the only reader of what it wrote, so no workgroup barrier stands
// between the staging and the MFMAs: a wave's LDS operations execute in order, and a wave starts its MFMAs when ITS loads have landed instead of when the
// slowest wave's have. (A rolled load->store loop pays one full L2 round trip per unit, hence the peeled first trip.)
// `after_first_loads` runs once, between the first trip's global loads and its LDS stores (every lane runs it, also lanes without a unit): the caller
// requests its weight stream there, behind the activation loads.
template <int P, class F>
__device__ __forceinline__ void stage_rows_f16_wave(const half_t* __restrict__ X, long ldx, int M, int K, half_t* xs, int ldxs, int lane,
                                                    F&& after_first_loads) {
    // P units per lane are requested together before anything is stored (P = what five rows of the slice need: one round trip); a unit index past
    // the end is clamped to the lane's previous unit, which is then stored twice with its own value
    const int kv8 = K >> 3, total = M * kv8;
    {
        int m_[P], k_[P];
        f16x8 v_[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            int u = lane + 64 * q;
            if (u >= total) u = (q == 0) ? total - 1 : (lane + 64 * (q - 1) < total ? lane + 64 * (q - 1) : total - 1);
            m_[q] = u / kv8; k_[q] = u - m_[q] * kv8;
            v_[q] = ld_f16x8(X + (long)m_[q] * ldx + k_[q] * 8);
        }
        after_first_loads();
#pragma unroll
        for (int q = 0; q < P; ++q) *reinterpret_cast<f16x8*>(xs + m_[q] * ldxs + k_[q] * 8) = v_[q];
    }
#pragma unroll 1
    for (int u0 = lane + 64 * P; u0 < total; u0 += 128) {
        const int u1 = u0 + 64;
        const int m0 = u0 / kv8, k0 = u0 - m0 * kv8;
        const int uc = (u1 < total) ? u1 : u0;
        const int m1 = uc / kv8, k1 = uc - m1 * kv8;
        const f16x8 v0 = ld_f16x8(X + (long)m0 * ldx + k0 * 8);
        const f16x8 v1 = ld_f16x8(X + (long)m1 * ldx + k1 * 8);
        *reinterpret_cast<f16x8*>(xs + m0 * ldxs + k0 * 8) = v0;
        *reinterpret_cast<f16x8*>(xs + m1 * ldxs + k1 * 8) = v1;
    }
}

// (Tried and dropped: a quarter-tile variant for fc2 — each 16-column tile shared by four workgroups, weights re-packed so
// a 1 KiB load holds four rows x four k-tiles, four MFMAs per load into per-lane-group accumulators, no cross-workgroup
// reduction. Numerically exact (all parity tests green) and it cuts the weight-load instructions per CU from 96 to 24, but
// every one of the 192 workgroups must stage the whole 5 x 3072 activation block: 5.5 us per launch vs 5.1.)

// Round 2, second half — three changes that each remove latency the decode-step trace showed (profiles/r2e_*):
//   * XS (GemvXsrc): the residual rows of the LayerNorm prologue / residual epilogue may be "rows + partial-sum slabs"
//     (GEMV_OUT_SLAB below) or, for layer 0, gathered from the embedding tables (the embedding launch is gone);
//   * GEMV_OUT_SLAB: the MLP output projection (K = 4 d_model: 96 KiB of weights and the whole 5 x 3072 activation block
//     per 16-column workgroup, on 48 CUs — the slowest launch of a layer, 4.8 us) is cut into WLX_FC2_KS K slices, grid
//     (tiles, slices); every slice workgroup writes its fp32 partial tile to its own slab and NOBODY reduces them in that
//     launch: the next layer's first projection sums rows + slabs in its LayerNorm prologue, and the next residual update
//     (the attention output projection) writes the sum back — a cross-workgroup reduction costs a launch boundary or a
//     grid barrier (>= 3 us either way), the deferred one costs WLX_FC2_KS more 1 KiB loads per row;
//   (Measured and dropped: LayerNorm helper waves beyond the nw MFMA waves, a wave per row — their dummy weight requests,
//   needed to keep hipcc's wait counting uniform, delayed the real weight stream by 0.6 us per launch, profiles/r2f_*.)
template <int CH, int LNV, int IN, int OUT, int NTB, int MT, int XS>
// (<= 8 waves wherever the kernel holds more than one row tile of fragments: 256 VGPRs per lane — at 16 waves the
// two- and three-tile residual projections spilled, 36-180 bytes of scratch per lane)
__global__ __launch_bounds__((IN == GEMV_IN_LN || OUT == GEMV_OUT_SLAB || MT > 1 || CH > 6 || IN == GEMV_IN_XATTN) ? 512 : 1024) void dec_gemv2_kernel(WLX_G2_HEAD_PARAMS GemvParams p_in) {
    // Row chunks (prompt prefill, round 3): a pass over up to 448 rows runs every projection as ONE launch whose grid.z walks
    // chunks of 48 rows (three MFMA row tiles, the widest this kernel holds); a chunk is this kernel on rebased row pointers.
    // Decode steps launch with Mtot = 0 and skip the block (a scalar branch).
    // Row tiles (batched decode steps, round 4): 17..64 rows run as row chunks of ONE 16-row MFMA tile each (the MT = 1
    // instantiations — the ones tuned for a single stream), the chunk index folded into blockIdx.x so that the rt_nz
    // workgroups that stream the same weight tile are (a) on one XCD (ids 8 apart: one L2 fetches the tile from HBM once)
    // and (b) dispatched back to back: lin = ((tile / 8) * rt_nz + chunk) * 8 + tile % 8. The three-tile form (48 rows per
    // workgroup) made every one of the N / 16 workgroups normalise / stage ALL rows on N / 16 CUs (60 rows, d_model 768:
    // 7.1 us per residual projection at 0.04 of the HBM peak); row tiles spread the same work over 4x the CUs.
    GemvParams p = p_in;
#if WLX_KERNARG_HEAD
    // The argument head (dec_gemv_internal.h GemvHead): what the first trip of loads and the weight request need arrives in SGPRs with the wave. Nothing in
    // front of the weight request reads a field that only the struct holds, so the first wait on the scalar counter stands behind it. (Where hipcc puts
    // the struct's own scalar fetch is its choice: in the rows + slabs form it issues it behind the activation and weight requests, not at entry.)
    p.Wp = h_wp; p.gamma = h_gamma; p.beta = h_beta;
    p.M = h_dims & 0xff; p.nwm = (h_dims >> 8) & 0xff; p.KTW = (h_dims >> 16) & 0xff; p.xstage = (h_dims >> 24) & 1;
    p.KT = h_kt & 0xff; p.KTS = (h_kt >> 8) & 0xff; p.K = p.KT * 32;          // (gemv2_cfg: K == 32 KT)
    const int h_mtot = (int)((unsigned)h_kt >> 16);
    if constexpr (IN == GEMV_IN_LN) {
        if constexpr (XS != GEMV_X_EMBED) { p.X = static_cast<const float*>(h_rows); p.ldx = h_ld; }
        if constexpr (XS == GEMV_X_SLABS) { p.slab = const_cast<float*>(static_cast<const float*>(h_aux)); p.slab_stride = h_aux_i; }
    } else if constexpr (IN == GEMV_IN_F16) {
        p.Xh = static_cast<const half_t*>(h_rows); p.ldxh = h_ld;
    } else {
        p.part_o = static_cast<const half_t*>(h_rows); p.part_ml = static_cast<const float*>(h_aux); p.R = h_aux_i & 0xffff; p.H = h_aux_i >> 16;
    }
#else
    const int h_mtot = p_in.Mtot;
#endif
    int tile = blockIdx.x;
#if WLX_KERNARG_HEAD
    int row0 = 0;
#endif
    if (h_mtot > 0) {
#if WLX_KERNARG_HEAD
        // The chunk fields are read where they are used, through the kernel-argument pointer and behind a compile-time fence: as fields of p_in hipcc
        // hoists their scalar fetch above this branch, and a decode step, which never takes it, then waits for that fetch before it may reuse the
        // destination registers — in front of its first trip's loads.
        const __attribute__((address_space(4))) char* ka = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const __attribute__((address_space(4))) GemvParams& pc = *reinterpret_cast<const __attribute__((address_space(4))) GemvParams*>(ka + sizeof(GemvHead));
#else
        const GemvParams& pc = p_in;
#endif
        const int c_nz = pc.rt_nz, c_magic = pc.rt_magic, c_tiles = pc.rt_tiles, c_chunk = pc.chunk, c_mtot = pc.Mtot;
        int zc = (int)blockIdx.z;
        if (c_nz > 0) {
            const int lin = (int)blockIdx.x, t = lin >> 3;
            const int tq = (int)(((unsigned)t * (unsigned)c_magic) >> 16);            // t / rt_nz (host: magic = 65536 / nz + 1, exact for t < 32768)
            zc = t - tq * c_nz;
            tile = tq * 8 + (lin & 7);
            if (tile >= c_tiles) return;                                              // (the tile count is padded to a multiple of 8)
        }
        const int CHK = c_chunk;
        const int r0 = zc * CHK;
        p.M = (c_mtot - r0 < CHK) ? c_mtot - r0 : CHK;
#if WLX_KERNARG_HEAD
        row0 = r0;
    }
    {
        // (with the argument head the rebase stands OUTSIDE the branch, by a row offset that is 0 for a decode step, and tests no pointer: inside the
        // branch, or behind a test, every pointer of the struct is a value merged behind a branch, and the merge waits for the struct's scalar
        // fetch in front of the first trip's loads. A pointer the form does not use is moved and never read.)
        // The pointers the head holds, and the row tables of the embedding gather, move here; the struct's other pointers move where the epilogue
        // operands are requested (rebase_late): scalar arithmetic on a struct field up here is one more wait in front of the first loads.
        const long r0 = row0;
        p.X += r0 * p.ldx; p.Xh += r0 * p.ldxh;
        if constexpr (IN == GEMV_IN_LN) p.slab += r0 * p.ldx;
        if constexpr (XS == GEMV_X_EMBED) { p.emb_token += r0; p.row_cache += r0; p.row_pos += r0; }
    }
    auto rebase_late = [&]() {
        long r0 = row0;
        asm volatile("" : "+s"(r0));            // (an opaque value: the products below are otherwise computed once, above both ways to load_weights)
        p.Yh += r0 * p.ldyh; p.Y += r0 * p.ldy; p.Xres += r0 * p.ldxres;
        if constexpr (IN != GEMV_IN_LN) p.slab += r0 * p.ldxres;
        if constexpr (XS != GEMV_X_EMBED) { p.row_cache += r0; p.row_pos += r0; }
    };
#else
        if (p.emb_token) p.emb_token += r0;
        if (p.X) p.X += (long)r0 * p.ldx;
        if (p.Xh) p.Xh += (long)r0 * p.ldxh;
        if (p.Yh) p.Yh += (long)r0 * p.ldyh;
        if (p.Y) p.Y += (long)r0 * p.ldy;
        if (p.Xres) p.Xres += (long)r0 * p.ldxres;
        if (p.slab) p.slab += (long)r0 * ((IN == GEMV_IN_LN) ? p.ldx : p.ldxres);
        if (p.row_cache) p.row_cache += r0;
        if (p.row_pos) p.row_pos += r0;
    }
#endif
    static_assert(XS == GEMV_X_PLAIN || IN == GEMV_IN_LN || (IN == GEMV_IN_F16 && OUT == GEMV_OUT_RESID && NTB == 1),
                  "slab / embedding sources: LayerNorm prologue or residual epilogue only");
    static_assert(OUT != GEMV_OUT_SLAB || (IN == GEMV_IN_F16 && NTB == 1), "K-split form: fp16 rows in");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // nw = waves that stream weights and run MFMAs; the LayerNorm prologue and the cross-attention combine may bring extra
    // waves that only help with the prologue (and load no weights: their wp is clamped to wave 0's slice, results unused)
    const int nw = p.nwm;
    WLX_TR_BEGIN();
    constexpr int NP = NTB * MT;                                           // (n-tile, 16-row tile) pairs of this workgroup
    // LayerNorm rows are held as NV float4 per lane, d_model = 256 NV. LNV == 15 stands for d_model 384 = 1.5 x 256 (tiny / tiny.en, round 5:
    // they ran on the first-generation kernel): two units, the second live on lanes 0..31 only — the other lanes load a clamped address,
    // hold zeros and store nothing. For every other LNV the masks below are compile-time constants and the code is what it was.
    constexpr bool LNT = (LNV == 15);
    constexpr int NV = LNT ? 2 : LNV;
    const bool tail_on = !LNT || lane < 32;
    const int tback = LNT ? (tail_on ? 0 : lane) : 0;                      // float4 units to step back in the last unit (inactive lanes read lane 0's)
    (void)tail_on; (void)tback;
    float* accred = smem;                                                  // [nw][NP][64][4]
    half_t* xs = reinterpret_cast<half_t*>(smem + nw * NP * 256);          // fp16 activation rows

    // (Tried and dropped: sub-tile workgroups — a 16-column tile shared by 2-4 workgroups, each streaming a quarter of
    // the weight rows with the other lanes masked. It spreads N = 768 layers over 192 CUs but does not reduce the number
    // of load INSTRUCTIONS a CU issues, which is what bounds these launches (~11 ns per wave-level load): no gain.)
    const bool streams = (IN != GEMV_IN_XATTN) || wave < nw;               // this wave streams weights and runs MFMAs (helper waves: XATTN only)
    const int kx0 = (streams ? wave : 0) * p.KTW;                          // first k-tile of this wave inside its K slice
    const int ks0 = (OUT == GEMV_OUT_SLAB) ? (int)blockIdx.y * p.KTS : 0;  // first k-tile of this workgroup's K slice
    const int kw0 = ks0 + kx0;                                             // ... of this wave, inside the weight matrix
    const half_t* wp = p.Wp + ((long)(tile * NTB) * p.KT + kw0) * 512 + lane * 8;
    const long wstep = (long)p.KT * 512;                                   // next n-tile
    f16x8 wf[CH][NTB];
    // epilogue operands of the FIRST pair this wave finishes (pair = wave: n-tile pair / MT, row tile pair % MT),
    // requested now (every lane, clamped row: no branch around a load); further pairs (batched rows) load theirs late
    int crow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) crow[mt] = (mt * 16 + c < p.M) ? mt * 16 + c : p.M - 1;
    const int pair0 = (wave < NP) ? wave : 0;
    const int nt_e = tile * NTB + pair0 / MT;
    const int n_e = nt_e * 16 + g * 4;
    int row_e = (pair0 % MT) * 16 + c;
    if (row_e >= p.M) row_e = p.M - 1;
    float4 bias_e = make_float4(0.f, 0.f, 0.f, 0.f), res_e = bias_e;
    int rc_e = 0, rp_e = 0;
    float4 slab_e[(OUT == GEMV_OUT_RESID && XS == GEMV_X_SLABS) ? WLX_FC2_KS : 1];
    auto load_epilogue_operands = [&]() {
        int row_q = row_e;
#if WLX_KERNARG_HEAD
        rebase_late();
        asm volatile("" : "+v"(row_q));         // (opaque, as the row offset of rebase_late: the row's byte offset is not computed above the first loads)
#endif
        if constexpr (OUT != GEMV_OUT_F32) bias_e = *reinterpret_cast<const float4*>(p.bias + n_e);
        if constexpr (OUT == GEMV_OUT_RESID) res_e = *reinterpret_cast<const float4*>(p.Xres + (long)row_q * p.ldxres + n_e);
        if constexpr (OUT == GEMV_OUT_QKV) { rc_e = p.row_cache[row_q]; rp_e = p.row_pos[row_q]; }
        if constexpr (OUT == GEMV_OUT_RESID && XS == GEMV_X_SLABS) {       // the residual is rows + slabs (summed at the store)
#pragma unroll
            for (int sl = 0; sl < WLX_FC2_KS; ++sl)
                slab_e[sl] = *reinterpret_cast<const float4*>(p.slab + sl * p.slab_stride + (long)row_q * p.ldxres + n_e);
        }
        if constexpr (OUT == GEMV_OUT_SLAB) { if (blockIdx.y != 0) bias_e = make_float4(0.f, 0.f, 0.f, 0.f); }   // the bias once: slice 0
    };
    // Their addresses come from the struct. With the argument head they are requested BEHIND the weight stream (load_weights), so that the wait for
    // the struct's scalar fetch stands behind the first trip's loads and the weight request instead of in front of them; vmcnt retires in order and
    // the epilogue needs the weights' MFMAs first, so nothing waits longer for it.
#if !WLX_KERNARG_HEAD
    load_epilogue_operands();
#endif
    // The weight stream is requested AFTER the activation loads have been issued (round 2): vmcnt retires in order, so with the weights first the wave's wait for its few activation
    // loads (L2) was a wait for its whole weight slice (HBM) as well, and the LayerNorm / staging / combine that must
    // precede the MFMAs started only once the weights had landed (decode-step trace: "LN done" 1.4 us into a 2.2 us
    // launch). With the activations first their wait is vmcnt(#weight loads): the prologue runs under the weight stream.
    auto load_weights = [&]() {
        // compile-time fence: hipcc otherwise hoists these address-independent loads back above the activation loads
        asm volatile("" ::: "memory");
        // helper waves of the combine (wave >= nw, they leave before the MFMAs) issue the same NUMBER of loads, all of one
        // already-requested KiB: a branch around the loads would make hipcc count the waits that follow for the path
        // WITHOUT weights in flight, i.e. drain the weight stream inside the combine on the waves that do have it
        const half_t* wq = streams ? wp : p.Wp + ((long)(tile * NTB) * p.KT + ks0) * 512 + lane * 8;   // (helpers: this workgroup's own first KiB — one shared line for every workgroup's helpers was a hot spot in L2)
        const long js = streams ? 512 : 0, is = streams ? wstep : 0;
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int i = 0; i < NTB; ++i) wf[j][i] = ld_nt_f16x8(wq + i * is + j * js);
#if WLX_KERNARG_HEAD
        asm volatile("" ::: "memory");          // (the epilogue operands stay behind the weight requests: see load_epilogue_operands;
        __builtin_amdgcn_sched_barrier(0);      //  so does their scalar address arithmetic, which the scheduler otherwise lifts in front of the first loads)
        load_epilogue_operands();
#endif
    };

    f32x4 acc[NTB][MT];
#pragma unroll
    for (int i = 0; i < NTB; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[i][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f16x8 xf[CH][MT];

    if constexpr (IN == GEMV_IN_F16) {
        const half_t* xr[MT];
        int xstep;                                                          // halfs between k-tiles of a row
        if (MT == 1 && p.xstage) {
            // One stream (M <= 16): the fp16 rows go through LDS — fetching B fragments straight from global costs CH
            // loads per wave of 64-byte pieces (16 waves x 6 = 96 load instructions per workgroup for K = 3072, as many
            // as the weights; a CU retires one per ~11 ns), the copy through LDS M * K / 8 / 64 = 30.
            const int Ks = (OUT == GEMV_OUT_SLAB) ? p.KTS * 32 : p.K;      // columns of the rows this workgroup multiplies
            const int ldxs = Ks + 8;
            // every wave stages and reads only its own K slice: no workgroup barrier (stage_rows_f16_wave)
            stage_rows_f16_wave<(CH * 4 * 5 + 63) / 64>(p.Xh + (ks0 + kx0) * 32, p.ldxh, p.M, p.KTW * 32, xs + kx0 * 32, ldxs, lane, [&]() { load_weights(); });
            WLX_TR_MARK(1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            xr[0] = xs + crow[0] * ldxs + kx0 * 32 + g * 8;                 // lanes of rows >= M re-read a valid row (never stored)
            xstep = 32;
        } else {
            // batched rows, or K too large for the LDS budget (large-v3 fc2: 5 x 5120 fp16 + partials > 64 KiB):
            // fragments straight from global
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xr[mt] = p.Xh + (long)crow[mt] * p.ldxh + kw0 * 32 + g * 8;
            xstep = 32;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[j][mt] = *reinterpret_cast<const f16x8*>(xr[mt] + j * xstep);
        if (!(MT == 1 && p.xstage)) load_weights();                         // (staged form: requested inside stage_rows_f16_wave)
#pragma unroll 1
        for (int ch = 1; ch < p.NCH; ++ch) {                               // big-K layers of the larger models only
            f16x8 wn[CH][NTB], xn[CH][MT];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
#pragma unroll
                for (int i = 0; i < NTB; ++i) wn[j][i] = ld_nt_f16x8(wp + i * wstep + (ch * CH + j) * 512);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) xn[j][mt] = *reinterpret_cast<const f16x8*>(xr[mt] + (ch * CH + j) * xstep);
            }
#pragma unroll
            for (int j = 0; j < CH; ++j) {
#pragma unroll
                for (int i = 0; i < NTB; ++i) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[i][mt] = mfma16(wf[j][i], xf[j][mt], acc[i][mt]);
                    wf[j][i] = wn[j][i];
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) xf[j][mt] = xn[j][mt];
            }
        }
    } else if constexpr (IN == GEMV_IN_LN && XS != GEMV_X_PLAIN) {
        // rows from slabs or the embedding tables: ONE row per wave in the first trip (its pieces are 3-5x the registers of a
        // plain row; the host picks a K split with at least as many waves as rows, all of them streaming weights — helper waves
        // with clamped dummy loads were measured 0.6 us SLOWER per launch, profiles/r2f_*) — except the four-wave shapes of
        // round 6 (PF2 below: K = 1024 / 1280), which request the wave's second row together with its first.
        // wave w normalises rows w, w + nw, ...; a row = LNV float4 per lane (d_model = 256 LNV).
        const int nwl = nw;
        constexpr int NSL = (XS == GEMV_X_SLABS) ? WLX_FC2_KS : 1;
        float4 x[NV], sl[NSL][NV];
        f16x4 te[NV];
        int tok0 = 0, pos0 = 0;
        // request the pieces of row r (wave-uniform, clamped by the caller): rows, + slabs, or embedding + position
        auto request_row = [&](int r, float4 (&x)[NV], float4 (&sl)[NSL][NV], f16x4 (&te)[NV], int& tok, int& pos) {
            if constexpr (XS == GEMV_X_EMBED) {
                tok = p.emb_token[r];
                // (position and cache row in one word: both are scalar loads here — a vector load inside the lane-0 store
                // branch below would make hipcc drain the whole weight stream in front of it)
                pos = p.row_pos[r] | (p.row_cache[r] << 16);               // position < 448, cache row < 32768
                const half_t* tp = p.tok_emb + (long)tok * p.K + lane * 4;
                const float4* pp = reinterpret_cast<const float4*>(p.pos_emb + (long)(pos & 0xffff) * p.K) + lane;
#pragma unroll
                for (int j = 0; j < NV; ++j) { const int tb = (j == NV - 1) ? tback : 0; te[j] = ld_f16x4(tp + 256 * j - 4 * tb); x[j] = pp[64 * j - tb]; }
            } else {
                const float4* x4 = reinterpret_cast<const float4*>(p.X + (long)r * p.ldx) + lane;
#pragma unroll
                for (int j = 0; j < NV; ++j) x[j] = x4[64 * j - ((j == NV - 1) ? tback : 0)];
                if constexpr (XS == GEMV_X_SLABS) {
#pragma unroll
                    for (int q = 0; q < NSL; ++q) {
                        const float4* s4 = reinterpret_cast<const float4*>(p.slab + q * p.slab_stride + (long)r * p.ldx) + lane;
#pragma unroll
                        for (int j = 0; j < NV; ++j) sl[q][j] = s4[64 * j - ((j == NV - 1) ? tback : 0)];
                    }
                }
            }
        };
        // the row itself from its pieces (same association as the residual epilogue: ((x + s0) + s1) ...)
        auto combine_row = [&](int r, bool keep, float4 (&x)[NV], const float4 (&sl)[NSL][NV], const f16x4 (&te)[NV], int tok, int pos) {
            if constexpr (XS == GEMV_X_SLABS) {
#pragma unroll
                for (int q = 0; q < NSL; ++q)
#pragma unroll
                    for (int j = 0; j < NV; ++j) { x[j].x += sl[q][j].x; x[j].y += sl[q][j].y; x[j].z += sl[q][j].z; x[j].w += sl[q][j].w; }
            }
            if constexpr (XS == GEMV_X_EMBED) {
#pragma unroll
                for (int j = 0; j < NV; ++j) { x[j].x += (float)te[j][0]; x[j].y += (float)te[j][1]; x[j].z += (float)te[j][2]; x[j].w += (float)te[j][3]; }
                if (tile == 0 && keep) {            // workgroup 0 (of its row chunk) leaves the rows where the residual updates expect them
                    float4* o4 = reinterpret_cast<float4*>(p.Xres + (long)r * p.ldxres) + lane;
#pragma unroll
                    for (int j = 0; j < NV; ++j) if (j < NV - 1 || tail_on) o4[64 * j] = x[j];
                    if (lane == 0) p.intok[(long)(pos >> 16) * WLX_T_TEXT + (pos & 0xffff)] = tok;
                }
            }
        };
        const int ra = (wave < p.M) ? wave : p.M - 1;
        request_row(ra, x, sl, te, tok0, pos0);
        // The four-wave shapes of one stream's step (log G9: (CH, LNV) = (6, 3), (8, 4), (10, 5) — instantiated for nothing else) have fewer waves than
        // rows: the wave's SECOND row is requested together with its first, as the PLAIN-rows prologue below does — a clamped row for the waves that
        // have none (every wave issues the same loads: no branch around a request)
        constexpr bool PF2 = MT == 1 && ((CH == 6 && LNV == 3) || (CH == 8 && LNV == 4) || (CH == 10 && LNV == 5));
        float4 xb[NV], slb[NSL][NV];
        f16x4 teb[NV];
        int tokb = 0, posb = 0;
        const int rb = (wave + nwl < p.M) ? wave + nwl : p.M - 1;
        if constexpr (PF2) request_row(rb, xb, slb, teb, tokb, posb);
        const float4* g4 = reinterpret_cast<const float4*>(p.gamma) + lane;
        const float4* b4 = reinterpret_cast<const float4*>(p.beta) + lane;
        float4 gq[NV], bq[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { const int tb = (j == NV - 1) ? tback : 0; gq[j] = g4[64 * j - tb]; bq[j] = b4[64 * j - tb]; }
        load_weights();
        const int ldxs = p.K + 8;
        constexpr float invK = LNT ? (1.0f / 384.0f) : 1.0f / (256.0f * NV);
        auto ln_row = [&](float4 (&x)[NV], int r, bool keep) {
            if constexpr (LNT) { if (!tail_on) x[NV - 1] = make_float4(0.f, 0.f, 0.f, 0.f); }
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) sm += (x[j].x + x[j].y) + (x[j].z + x[j].w);
            const float mean = wave_sum_dpp(sm) * invK;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                x[j].x -= mean; x[j].y -= mean; x[j].z -= mean; x[j].w -= mean;
                if constexpr (LNT) { if (j == NV - 1 && !tail_on) x[j] = make_float4(0.f, 0.f, 0.f, 0.f); }
                q += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
            }
            const float rstd = rsqrtf(wave_sum_dpp(q) * invK + 1e-5f);
            half_t* dst = xs + (long)r * ldxs + lane * 4;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f16x4 hv = {(half_t)(x[j].x * rstd * gq[j].x + bq[j].x), (half_t)(x[j].y * rstd * gq[j].y + bq[j].y),
                                  (half_t)(x[j].z * rstd * gq[j].z + bq[j].z), (half_t)(x[j].w * rstd * gq[j].w + bq[j].w)};
                if (keep && (j < NV - 1 || tail_on)) *reinterpret_cast<f16x4*>(dst + 256 * j) = hv;
            }
        };
        // first trip: straight-line and UNCONDITIONAL (a wave without a row normalises the clamped row it loaded and keeps
        // nothing): inside an `if (wave < M)` hipcc sinks the row loads into the branch, behind the weights. It must not
        // share a loop with the later trips either: hipcc's wait insertion merges the two ways into a loop body by the
        // NEWEST request of either, so the first trip would wait for the weight stream it is meant to overlap.
        combine_row(ra, wave < p.M, x, sl, te, tok0, pos0);
        ln_row(x, ra, wave < p.M);
        if constexpr (PF2) {
            combine_row(rb, wave + nwl < p.M, xb, slb, teb, tokb, posb);
            ln_row(xb, rb, wave + nwl < p.M);
        }
        if constexpr (MT == 1) {
#pragma unroll 1
            for (int r = wave + (PF2 ? 2 : 1) * nwl; r < p.M; r += nwl) {   // more rows than waves (9..16 rows)
                float4 x2[NV], sl2[NSL][NV];
                f16x4 te2[NV];
                int tok2 = 0, pos2 = 0;
                request_row(r, x2, sl2, te2, tok2, pos2);
                combine_row(r, true, x2, sl2, te2, tok2, pos2);
                ln_row(x2, r, true);
            }
        } else {
            // batched streams (17..48 rows: 3..6 rows per wave): two rows per trip, both requested before either is
            // normalised, so a trip pays ONE round trip to L2 instead of one per row
#pragma unroll 1
            for (int r = wave + nwl; r < p.M; r += 2 * nwl) {
                const int r1 = r + nwl;
                const bool has1 = r1 < p.M;
                float4 x2[NV], sl2[NSL][NV], x3[NV], sl3[NSL][NV];
                f16x4 te2[NV], te3[NV];
                int tok2 = 0, pos2 = 0, tok3 = 0, pos3 = 0;
                request_row(r, x2, sl2, te2, tok2, pos2);
                request_row(has1 ? r1 : r, x3, sl3, te3, tok3, pos3);
                combine_row(r, true, x2, sl2, te2, tok2, pos2);
                ln_row(x2, r, true);
                combine_row(has1 ? r1 : r, has1, x3, sl3, te3, tok3, pos3);
                ln_row(x3, has1 ? r1 : r, has1);
            }
        }
        WLX_TR_MARK(1);
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const half_t* xr = xs + crow[mt] * ldxs + kx0 * 32 + g * 8;     // lanes of rows >= M re-read a valid row (never stored)
#pragma unroll
            for (int j = 0; j < CH; ++j) xf[j][mt] = *reinterpret_cast<const f16x8*>(xr + j * 32);
        }
    } else if constexpr (IN == GEMV_IN_LN) {
        // wave w normalises rows w, w + nw, ...; a row = LNV float4 per lane (d_model = 256 LNV)
        // first trip's rows (this wave's row and the one nw below it) are requested before anything else
        float4 x[NV], y[NV];
        {
            const int ra = (wave < p.M) ? wave : p.M - 1, rb = (wave + nw < p.M) ? wave + nw : ra;
            const float4* x4 = reinterpret_cast<const float4*>(p.X + (long)ra * p.ldx) + lane;
            const float4* y4 = reinterpret_cast<const float4*>(p.X + (long)rb * p.ldx) + lane;
#pragma unroll
            for (int j = 0; j < NV; ++j) { const int tb = (j == NV - 1) ? tback : 0; x[j] = x4[64 * j - tb]; y[j] = y4[64 * j - tb]; }
        }
        const float4* g4 = reinterpret_cast<const float4*>(p.gamma) + lane;
        const float4* b4 = reinterpret_cast<const float4*>(p.beta) + lane;
        float4 gq[NV], bq[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { const int tb = (j == NV - 1) ? tback : 0; gq[j] = g4[64 * j - tb]; bq[j] = b4[64 * j - tb]; }
        load_weights();
        const int ldxs = p.K + 8;
        constexpr float invK = LNT ? (1.0f / 384.0f) : 1.0f / (256.0f * NV);
        auto ln_row = [&](float4 (&x)[NV], int r) {
            if constexpr (LNT) { if (!tail_on) x[NV - 1] = make_float4(0.f, 0.f, 0.f, 0.f); }
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) sm += (x[j].x + x[j].y) + (x[j].z + x[j].w);
            const float mean = wave_sum_dpp(sm) * invK;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                x[j].x -= mean; x[j].y -= mean; x[j].z -= mean; x[j].w -= mean;
                if constexpr (LNT) { if (j == NV - 1 && !tail_on) x[j] = make_float4(0.f, 0.f, 0.f, 0.f); }
                q += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
            }
            const float rstd = rsqrtf(wave_sum_dpp(q) * invK + 1e-5f);
            half_t* dst = xs + (long)r * ldxs + lane * 4;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f16x4 hv = {(half_t)(x[j].x * rstd * gq[j].x + bq[j].x), (half_t)(x[j].y * rstd * gq[j].y + bq[j].y),
                                  (half_t)(x[j].z * rstd * gq[j].z + bq[j].z), (half_t)(x[j].w * rstd * gq[j].w + bq[j].w)};
                if (j < NV - 1 || tail_on) *reinterpret_cast<f16x4*>(dst + 256 * j) = hv;
            }
        };
        // first trip, straight-line: its rows were requested at the top. (It must not share a loop with the later trips:
        // hipcc's wait insertion merges the two ways into a loop body by the NEWEST request of either, so a body that
        // also re-loads x / y for a later trip makes the first trip wait for all but five of everything outstanding —
        // i.e. for the weight stream the reordering above is meant to overlap.)
        if (wave < p.M) {
            const bool has1 = wave + nw < p.M;
#pragma unroll 1
            for (int u = 0; u < (has1 ? 2 : 1); ++u) {                      // rolled: one copy of the row code (code size is latency here)
                if (u) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) x[j] = y[j];
                }
                ln_row(x, u ? wave + nw : wave);
            }
        }
#pragma unroll 1
        for (int r = wave + 2 * nw; r < p.M; r += 2 * nw) {                 // batched rows (M > 2 nw): rows r and r + nw per trip
            const int r1 = r + nw;
            const bool has1 = r1 < p.M;
            const float4* x4 = reinterpret_cast<const float4*>(p.X + (long)r * p.ldx) + lane;
            const float4* y4 = reinterpret_cast<const float4*>(p.X + (long)(has1 ? r1 : r) * p.ldx) + lane;
            float4 x2[NV], y2[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) { const int tb = (j == NV - 1) ? tback : 0; x2[j] = x4[64 * j - tb]; y2[j] = y4[64 * j - tb]; }
#pragma unroll 1
            for (int u = 0; u < (has1 ? 2 : 1); ++u) {
                if (u) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) x2[j] = y2[j];
                }
                ln_row(x2, u ? r1 : r);
            }
        }
        WLX_TR_MARK(1);
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const half_t* xr = xs + crow[mt] * ldxs + kx0 * 32 + g * 8;     // lanes of rows >= M re-read a valid row (never stored)
#pragma unroll
            for (int j = 0; j < CH; ++j) xf[j][mt] = *reinterpret_cast<const f16x8*>(xr + j * 32);
        }
    } else {   // GEMV_IN_XATTN: the WLX_XSPLIT partials (normalised fp16 O, fp32 (m, l) contiguous per row) are combined into fp16 rows in LDS, like the
        // LayerNorm rows. (A CU retires one wave-level load instruction per ~11 ns: the fp32 / 4-dim / separate-(m,l) form needed 240 of them per
        // workgroup, the forms below 90.)
        const int ldxs = p.K + 8;
        const int n_it = p.M * p.H * 8;                                     // (row, head, 8-dim group) items of the workgroup's rows
        const float rH = 1.0f / (float)p.H, rR = 1.0f / (float)p.R;
        if constexpr (MT == 1) {
            // One row tile (round 6, log G3): every wave combines exactly the columns of ITS K slice — items (row, 8-dim group) of columns
            // [c0, c0 + W) — and is their only reader, so neither helper waves nor a workgroup barrier between the combine and the MFMAs are needed
            // (the launcher starts nw waves): a wave goes on when ITS partials have landed. The first two items of a lane are requested together, the
            // weights right behind them (5 rows x 192 columns = 120 items: one round trip).
            const int W = p.KTW * 32, c0 = kx0 * 32, wg8 = W >> 3;
            const int n_w = p.M * wg8;
            const float rG = 1.0f / (float)wg8;
            auto item_ptrs = [&](int u, const float4*& mlp, const half_t*& op, int& m, int& col) {
                const int uu = (u < n_w) ? u : n_w - 1;
                m = (int)(((float)uu + 0.5f) * rG);                         // uu / wg8 (exact: small integers)
                col = c0 + (uu - m * wg8) * 8;
                const int hh = col >> 6, q8 = (col >> 3) & 7;
                const int item = (int)(((float)m + 0.5f) * rR), qi = m - item * p.R;
                const long ih = (long)item * p.H + hh;
                mlp = reinterpret_cast<const float4*>(p.part_ml + (ih * 16 + qi) * (WLX_XSPLIT * 2));
                op = p.part_o + (ih * WLX_XSPLIT * 16 + qi) * 64 + q8 * 8;
            };
            auto finish = [&](const float4 (&ml)[WLX_XSPLIT / 2], const f16x8 (&ov)[WLX_XSPLIT], int m, int col, bool keep) {
                float mmax = fmaxf(ml[0].x, ml[0].z);
#pragma unroll
                for (int sp = 1; sp < WLX_XSPLIT / 2; ++sp) mmax = fmaxf(mmax, fmaxf(ml[sp].x, ml[sp].z));
                float den = 0.f;
                float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT; ++sp) {                   // (the arithmetic and its order are the batched form's below: identical rows)
                    const float mm = (sp & 1) ? ml[sp >> 1].z : ml[sp >> 1].x, ll = (sp & 1) ? ml[sp >> 1].w : ml[sp >> 1].y;
                    const float w = __expf(mm - mmax) * ll;
                    den += w;
#pragma unroll
                    for (int e = 0; e < 8; ++e) num[e] += w * (float)ov[sp][e];
                }
                const float inv = 1.0f / den;
                const f16x8 hv = {(half_t)(num[0] * inv), (half_t)(num[1] * inv), (half_t)(num[2] * inv), (half_t)(num[3] * inv),
                                  (half_t)(num[4] * inv), (half_t)(num[5] * inv), (half_t)(num[6] * inv), (half_t)(num[7] * inv)};
                if (keep) *reinterpret_cast<f16x8*>(xs + m * ldxs + col) = hv;
            };
            {
                // NPL items per lane requested together (what five rows of the slice need: 2 for six k-tiles per wave, 3 for eight — one round trip)
                constexpr int NPL = (CH * 4 * 5 + 63) / 64 < 2 ? 2 : (CH * 4 * 5 + 63) / 64;
                const float4* mlpq[NPL]; const half_t* opq[NPL]; int mq[NPL], colq[NPL];
                float4 mlq[NPL][WLX_XSPLIT / 2];
                f16x8 ovq[NPL][WLX_XSPLIT];
#pragma unroll
                for (int q = 0; q < NPL; ++q) item_ptrs(lane + 64 * q, mlpq[q], opq[q], mq[q], colq[q]);
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT / 2; ++sp)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) mlq[q][sp] = mlpq[q][sp];
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT; ++sp)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) ovq[q][sp] = ld_f16x8(opq[q] + sp * 1024);
                load_weights();
#pragma unroll
                for (int q = 0; q < NPL; ++q) finish(mlq[q], ovq[q], mq[q], colq[q], lane + 64 * q < n_w);
            }
#pragma unroll 1
            for (int u = lane + 64 * ((CH * 4 * 5 + 63) / 64 < 2 ? 2 : (CH * 4 * 5 + 63) / 64); u < n_w; u += 64) {   // more items per wave than the peeled ones (batched rows up to 16)
                const float4* mlp; const half_t* op; int m, col;
                item_ptrs(u, mlp, op, m, col);
                float4 ml[WLX_XSPLIT / 2];
                f16x8 ov[WLX_XSPLIT];
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT / 2; ++sp) ml[sp] = mlp[sp];
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT; ++sp) ov[sp] = ld_f16x8(op + sp * 1024);
                finish(ml, ov, m, col, true);
            }
            WLX_TR_MARK(1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            // Batched rows (two or three row tiles): every wave of the workgroup (more than the nw MFMA waves) combines — one (row, head, 8-dim
            // group) per thread, 12 16-byte loads in flight.
            // One (row, head, 8-dim group) per call. The FIRST trip is straight-line code run by every thread (clamped item, result not stored when
            // out of range) with the weight request right behind its loads; later trips (M * H * 8 > blockDim) run in a separate loop — sharing one
            // loop would make hipcc wait for the weights inside the first trip (its wait insertion merges loop paths by the newest request of either).
            auto combine = [&](int it0, bool first) {
                const int it = (it0 < n_it) ? it0 : n_it - 1;
                const int q8 = it & 7, hm = it >> 3;
                const int m = (int)(((float)hm + 0.5f) * rH), hh = hm - m * p.H;
                const int item = (int)(((float)m + 0.5f) * rR), qi = m - item * p.R;
                const long ih = (long)item * p.H + hh;
                const float4* mlp = reinterpret_cast<const float4*>(p.part_ml + (ih * 16 + qi) * (WLX_XSPLIT * 2));
                const half_t* op = p.part_o + (ih * WLX_XSPLIT * 16 + qi) * 64 + q8 * 8;
                float4 ml[WLX_XSPLIT / 2];
                f16x8 ov[WLX_XSPLIT];
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT / 2; ++sp) ml[sp] = mlp[sp];               // (m, l) of splits 2 sp, 2 sp + 1
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT; ++sp) ov[sp] = ld_f16x8(op + sp * 1024);
                if (first) load_weights();                                  // behind the first trip's partial loads
                float mmax = fmaxf(ml[0].x, ml[0].z);
#pragma unroll
                for (int sp = 1; sp < WLX_XSPLIT / 2; ++sp) mmax = fmaxf(mmax, fmaxf(ml[sp].x, ml[sp].z));
                float den = 0.f;
                float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int sp = 0; sp < WLX_XSPLIT; ++sp) {
                    const float mm = (sp & 1) ? ml[sp >> 1].z : ml[sp >> 1].x, ll = (sp & 1) ? ml[sp >> 1].w : ml[sp >> 1].y;
                    const float w = __expf(mm - mmax) * ll;
                    den += w;
#pragma unroll
                    for (int e = 0; e < 8; ++e) num[e] += w * (float)ov[sp][e];
                }
                const float inv = 1.0f / den;
                const f16x8 hv = {(half_t)(num[0] * inv), (half_t)(num[1] * inv), (half_t)(num[2] * inv), (half_t)(num[3] * inv),
                                  (half_t)(num[4] * inv), (half_t)(num[5] * inv), (half_t)(num[6] * inv), (half_t)(num[7] * inv)};
                if (it0 < n_it) *reinterpret_cast<f16x8*>(xs + m * ldxs + hh * 64 + q8 * 8) = hv;
            };
            combine(tid, true);
#pragma unroll 1
            for (int it0 = tid + blockDim.x; it0 < n_it; it0 += blockDim.x) combine(it0, false);
            WLX_TR_MARK(1);
            __syncthreads();
            if (!streams) return;                                           // helper waves are done (no later barrier needs them: ended waves leave the barrier count)
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const half_t* xr = xs + crow[mt] * ldxs + kx0 * 32 + g * 8;
#pragma unroll
            for (int j = 0; j < CH; ++j) xf[j][mt] = *reinterpret_cast<const f16x8*>(xr + j * 32);
        }
    }
    WLX_TR_MARK(2);
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int i = 0; i < NTB; ++i)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[i][mt] = mfma16(wf[j][i], xf[j][mt], acc[i][mt]);

    // ---- cross-wave K reduction through LDS in a fixed order; wave w finishes pairs w, w + nw, ...
#pragma unroll
    for (int i = 0; i < NTB; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            *reinterpret_cast<f32x4*>(accred + ((wave * NP + i * MT + mt) * 64 + lane) * 4) = acc[i][mt];
    WLX_TR_MARK(3);
    __syncthreads();
#ifdef WLX_TRACE
    if (wave >= NP) { WLX_TR_END_WAVES(p.trc); return; }
#else
    if (wave >= NP) return;
#endif
#pragma unroll 1
    for (int pair = wave; pair < NP; pair += nw) {
    const int nt_p = tile * NTB + pair / MT;
    const int n_p = nt_p * 16 + g * 4;
    const int row_p = (pair % MT) * 16 + c;
    if (pair != wave) {                        // not the pair whose operands were requested up front
        const int rr = (row_p < p.M) ? row_p : p.M - 1;
        if constexpr (OUT != GEMV_OUT_F32) bias_e = *reinterpret_cast<const float4*>(p.bias + n_p);
        if constexpr (OUT == GEMV_OUT_RESID) res_e = *reinterpret_cast<const float4*>(p.Xres + (long)rr * p.ldxres + n_p);
        if constexpr (OUT == GEMV_OUT_RESID && XS == GEMV_X_SLABS) {
#pragma unroll
            for (int sl = 0; sl < WLX_FC2_KS; ++sl)
                slab_e[sl] = *reinterpret_cast<const float4*>(p.slab + sl * p.slab_stride + (long)rr * p.ldxres + n_p);
        }
        if constexpr (OUT == GEMV_OUT_SLAB) { if (blockIdx.y != 0) bias_e = make_float4(0.f, 0.f, 0.f, 0.f); }
        if constexpr (OUT == GEMV_OUT_QKV) { rc_e = p.row_cache[rr]; rp_e = p.row_pos[rr]; }
    }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float* ar = accred + (pair * 64 + lane) * 4;
#pragma unroll 2
    for (int w = 0; w < nw; ++w) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(ar + w * (NP * 256));
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    WLX_TR_MARK(4);
    if (row_p < p.M && (NTB == 1 || nt_p * 16 < p.N)) {
        const int c = row_p;                   // (shadows the lane's column index: below, c is the activation row)
        const int n_e = n_p;
        float o0 = v[0] + bias_e.x, o1 = v[1] + bias_e.y, o2 = v[2] + bias_e.z, o3 = v[3] + bias_e.w;
        if constexpr (OUT == GEMV_OUT_F16 || OUT == GEMV_OUT_GELU_F16) {
            if constexpr (OUT == GEMV_OUT_GELU_F16) { o0 = gelu_erf(o0); o1 = gelu_erf(o1); o2 = gelu_erf(o2); o3 = gelu_erf(o3); }
            const f16x4 h = {(half_t)(o0 * p.qscale), (half_t)(o1 * p.qscale), (half_t)(o2 * p.qscale), (half_t)(o3 * p.qscale)};
            *reinterpret_cast<f16x4*>(p.Yh + (long)c * p.ldyh + n_e) = h;
        } else if constexpr (OUT == GEMV_OUT_F32) {
            float* yp = p.Y + (long)c * p.ldy + n_e;
            if (n_e + 3 < p.N) *reinterpret_cast<float4*>(yp) = make_float4(o0, o1, o2, o3);
            else { if (n_e < p.N) yp[0] = o0; if (n_e + 1 < p.N) yp[1] = o1; if (n_e + 2 < p.N) yp[2] = o2; }
        } else if constexpr (OUT == GEMV_OUT_RESID) {
            if constexpr (XS == GEMV_X_SLABS) {                             // rows + slabs (the LayerNorm prologue's association)
#pragma unroll
                for (int sl = 0; sl < WLX_FC2_KS; ++sl) { res_e.x += slab_e[sl].x; res_e.y += slab_e[sl].y; res_e.z += slab_e[sl].z; res_e.w += slab_e[sl].w; }
            }
            *reinterpret_cast<float4*>(p.Xres + (long)c * p.ldxres + n_e) =
                make_float4(res_e.x + o0, res_e.y + o1, res_e.z + o2, res_e.w + o3);
        } else if constexpr (OUT == GEMV_OUT_SLAB) {                        // this K slice's partial tile; summed by the consumers
            *reinterpret_cast<float4*>(p.slab + blockIdx.y * p.slab_stride + (long)c * p.ldxres + n_e) = make_float4(o0, o1, o2, o3);
        } else {   // GEMV_OUT_QKV: the 16-column tile lies entirely in q, k or v (d % 16 == 0)
            if (n_e < p.d) {
                const f16x4 h = {(half_t)(o0 * p.qscale), (half_t)(o1 * p.qscale), (half_t)(o2 * p.qscale), (half_t)(o3 * p.qscale)};
                *reinterpret_cast<f16x4*>(p.Yh + (long)c * p.ldyh + n_e) = h;
            } else {
                const f16x4 h = {(half_t)o0, (half_t)o1, (half_t)o2, (half_t)o3};
                const bool isk = n_e < 2 * p.d;
                half_t* dst = (isk ? p.Kc : p.Vc) + (long)rc_e * p.cache_row_stride + (long)rp_e * p.d + (n_e - (isk ? p.d : 2 * p.d));
                *reinterpret_cast<f16x4*>(dst) = h;
            }
        }
    }
    }
    WLX_TR_MARK(5);
    WLX_TR_END_WAVES(p.trc);
}

// the raised dynamic-LDS limit (dec_gemv_internal.h), shared with dec_vocab.hip
std::atomic<bool> g_lds_optin_refused{false};
void lds_optin(const void* kernel, std::atomic<signed char> (&granted)[64], const char* what) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || granted[dev].load(std::memory_order_acquire) != 0) return;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WLX_G2_LDS_MAX);
    if (e == hipSuccess) { granted[dev].store(1, std::memory_order_release); return; }
    // the caller's launch then fails with the runtime's own error, which the engine's hipGetLastError check reports for
    // THIS call; later calls take the general kernel (gemv2_cfg, vocab2_ok)
    (void)hipGetLastError();
    g_lds_optin_refused.store(true);
    fprintf(stderr, "[wlx] device %d refused %d KiB of dynamic LDS (%s): %s to the general kernel\n", dev, WLX_G2_LDS_MAX / 1024, hipGetErrorString(e), what);
}
// the argument head of a launch (dec_gemv_internal.h): every slot repeats a field of p, chosen by the input form as the kernel reads it back
static bool g2_head_fits(const GemvParams& p) {
    const long lim = 0x7fffffffL;
    return p.KT >= 0 && p.KT <= 255 && p.KTS >= 0 && p.KTS <= 255 && p.Mtot >= 0 && p.Mtot <= 65535 && p.M >= 0 && p.M <= 255 &&
           p.ldx >= 0 && p.ldx <= lim && p.ldxh >= 0 && p.ldxh <= lim && p.slab_stride >= 0 && p.slab_stride <= lim &&
           (p.in_mode != GEMV_IN_XATTN || (p.R >= 0 && p.R <= 0xffff && p.H >= 0 && p.H <= 0x7fff));
}
bool g2_head(const GemvParams& p, GemvHead* h) {
    if (!g2_head_fits(p) || p.nwm < 0 || p.nwm > 255 || p.KTW < 0 || p.KTW > 255) return false;
    *h = GemvHead{};
    h->gamma = p.gamma; h->beta = p.beta; h->wp = p.Wp;
    h->dims = p.M | (p.nwm << 8) | (p.KTW << 16) | ((p.xstage ? 1 : 0) << 24);
    h->kt = p.KT | (p.KTS << 8) | (int)((unsigned)p.Mtot << 16);
    if (p.in_mode == GEMV_IN_LN) {
        if (p.xsrc != GEMV_X_EMBED) { h->rows = p.X; h->ld = (int)p.ldx; }      // (embedding rows: a dependent gather through the struct's tables)
        if (p.xsrc == GEMV_X_SLABS) { h->aux = p.slab; h->aux_i = (int)p.slab_stride; }
    } else if (p.in_mode == GEMV_IN_F16) {
        h->rows = p.Xh; h->ld = (int)p.ldxh;
    } else {
        h->rows = p.part_o; h->aux = p.part_ml; h->aux_i = p.R | (p.H << 16);
    }
    return true;
}
// one launch of an instantiation
template <int CH, int LNV, int IN, int OUT, int NTB, int MT, int XS>
static void g2_launch(dim3 grid, dim3 block, size_t shm, hipStream_t s, const GemvParams& p) {
#if WLX_KERNARG_HEAD
    GemvHead h;
    if (!g2_head(p, &h)) { dispatch_bug("dec_gemv2_kernel (argument head)", s); return; }
#endif
    if (shm > 64 * 1024) {
        static std::atomic<signed char> granted[64] = {};
        lds_optin(reinterpret_cast<const void*>(&dec_gemv2_kernel<CH, LNV, IN, OUT, NTB, MT, XS>), granted, "batched decode projections fall back");
    }
    hipLaunchKernelGGL((dec_gemv2_kernel<CH, LNV, IN, OUT, NTB, MT, XS>), grid, block, shm, s, WLX_G2_HEAD_ARGS(h) p);
}
void dispatch_bug(const char* kernel, hipStream_t s) {
    fprintf(stderr, "[wlx] launch_dec_gemv: no %s instantiation for a configuration its probe accepted\n", kernel);
    (void)hipLaunchKernel(nullptr, dim3(1), dim3(64), nullptr, 0, s);
}

struct Gemv2Cfg { bool ok, xstage; int nw, CH, NCH, LNV, NTB, MT; size_t shm; };   // (LNV: the kernel's argument, 1 where no LayerNorm runs)
// gemv2_cfg, first decision: waves and chunk width. The KTf k-tiles of a workgroup = nw waves x NCH chunks x CH k-tiles; with them LNV.
static bool gemv2_cfg_waves(const GemvParams& p, int KTf, Gemv2Cfg& c) {
    const int cap = (p.in_mode == GEMV_IN_F16 && p.out_mode != GEMV_OUT_SLAB && p.M <= 16) ? 16 : 8;
    // exact factorisation KTf = nw * CH * NCH, CH in {6, 5, 4}: fewest chunks first, then the widest chunk
    int best_nch = 1 << 30;
    // one stream's step, LayerNorm over K = 1024 / 1280: four waves of 8 / 10 k-tiles instead of eight of 4 / 5 (logs G8 and G9, below)
    const bool ln_wide = p.in_mode == GEMV_IN_LN && p.M <= 8 && p.Mtot == 0 && (p.K == 1024 || p.K == 1280);
    // Log G9 (round 6): a layer's FIRST projection (rows + slabs / embedding rows) of one stream's step as FOUR waves for K = 1024 / 1280 (8 / 10 k-tiles
    // per wave instead of eight waves of 4 / 5), the wave's second row requested together with its first (PF2 in the kernel: without that prefetch
    // the four-wave shape LOST 0.6-1 %): large-v3 +1.6 %, medium.en +0.9 %, profiles/r6az_*. K = 768 keeps one row per wave (six waves of four: the
    // four-wave shape measured +0.1 %, inside the spread).
    if (p.in_mode == GEMV_IN_LN && p.xsrc != GEMV_X_PLAIN && !(ln_wide && p.out_mode == GEMV_OUT_QKV)) {
        // slab / embedding rows: one row per wave, so at least min(M, 8) waves, each streaming CH >= 2 k-tiles
        const int want = std::min(p.M, 8);
        for (int CH = 6; CH >= 2; --CH) {
            if (KTf % CH || KTf / CH > 8 || KTf / CH < want) continue;
            best_nch = 1; c.nw = KTf / CH; c.CH = CH; c.NCH = 1;
            break;
        }
    } else {     // (the split combine as 8 weight-streaming waves instead of 4 + helpers measured equal, profiles/r2h_*: not instantiated any more)
        // Fewer waves with longer K slices (log G5, round 6): once no workgroup barrier stands in front of the MFMAs (wave-local staging, log G2) a wave's
        // cost is its fixed part (row loads, LDS reduction leg, its place at the epilogue's barrier) more than its k-tiles — K = 768 as two waves of twelve
        // k-tiles instead of four of six (step graph 367.9 -> 363.6 us, headline +0.8 %), 1024 as four of eight instead of eight of four (medium.en
        // +2.9 %), 512 as two of eight (+0.3 %). Measured and left alone (profiles/r6as_*, r6ao_*): ONE wave of 24 k-tiles for K = 768 (-2.0 %: one wave
        // cannot keep 24 KiB of loads in flight AND the chain of 24 dependent MFMAs is 0.4 us), two waves of sixteen for K = 1024 (equal), K = 1280 as five
        // waves of eight (uneven over the four SIMDs: -1 %; it runs as four of ten, below), the row tiles of a batched step (12 windows per decode -1.8 %:
        // Mtot > 0 keeps the narrow slices), the split combine of the cross-attention output projection as three waves of eight / two of twelve with
        // three / four items peeled per lane (-1.5 % / -10 %: its waves are bound by the partials they gather, not by their count). Wide slices stay
        // within their launch bound (512 threads: an instantiation bound to 512 launched with 1024 is 'unspecified launch failure') and on SIMD-even counts.
        // The widest chunk tried is 12 (6 was the pick until log G5). scripts/gemv_pick_probe.cpp prints the picks on the host.
        // (8 / 12 k-tiles per wave: fp16 rows in only, staged rows (one row tile) — the split combine peels two items per lane for six k-tiles)
        // K = 1280 as four waves of ten k-tiles instead of eight of five (large-v3 step graph 1300 -> 1288 us, +1.1 %: profiles/r6au_*).
        // Log G8 (round 6): the LayerNorm-fronted projections on PLAIN rows of one stream's step (cross-attention query where it is not fused, first MLP
        // projection) as four waves instead of eight for K = 1024 / 1280 — 8 / 10 k-tiles per wave, five rows in two row trips: large-v3 step graph
        // 1287 -> 1250 us (+3.5 %), medium.en 859 -> 832 us (+2.9 %), profiles/r6aw_*.
        const int chmax = (p.in_mode == GEMV_IN_F16 && p.M <= 16 && p.Mtot == 0) ? 12 : ln_wide ? 10 : 6;
        for (int CH = chmax; CH >= 4; --CH) {
            if (CH != 12 && CH != 10 && CH != 8 && CH > 6) continue;
            if (ln_wide && CH > 6 && CH * 128 != p.K) continue;
            if (KTf % CH) continue;
            const int q = KTf / CH;                     // = nw * NCH
            for (int nw = std::min(CH > 6 ? std::min(cap, 8) : cap, q); nw >= 1; --nw) {
                if (q % nw) continue;
                if (CH > 6 && nw > 4 && (nw & 3)) break;
                const int nch = q / nw;
                if (nch < best_nch) { best_nch = nch; c.nw = nw; c.CH = CH; c.NCH = nch; }
                break;
            }
        }
    }
    if (p.in_mode == GEMV_IN_LN && p.K == 384) {
        // d_model 384 (tiny / tiny.en, round 5): 12 k-tiles as six waves of two, so that six waves share the LayerNorm of the rows
        // (the general search above would pick two waves of six k-tiles: three LayerNorm trips for five rows)
        best_nch = 1; c.nw = 6; c.CH = 2; c.NCH = 1;
    }
    if (best_nch == (1 << 30)) return false;
    if (p.in_mode != GEMV_IN_F16 && c.NCH != 1) return false;
    c.LNV = 1;
    if (p.in_mode == GEMV_IN_LN) {
        if (p.K == 384) c.LNV = 15;                 // 1.5 x 256: see dec_gemv2_kernel
        else {
            if (p.K % 256 || p.K / 256 < 2 || p.K / 256 > 5) return false;
            c.LNV = p.K / 256;
        }
    }
    return true;
}
// gemv2_cfg, second decision: 16-column tiles per workgroup (the staging decision may still take two back to one)
static int gemv2_cfg_tiles(const GemvParams& p) {
    int NTB = (p.out_mode == GEMV_OUT_F32 && p.N > 8192) ? 2 : 1;
    // more 16-column tiles than CUs (large-v3's first MLP projection: 320): two tiles per workgroup keep the launch to one
    // round of workgroups and halve the redundant LayerNorm prologues.
    if (p.in_mode == GEMV_IN_LN && p.out_mode == GEMV_OUT_GELU_F16 && p.xsrc == GEMV_X_PLAIN && (p.N + 15) / 16 > 256 && ((p.N + 15) / 16) % 2 == 0) NTB = 2;
    // row tiles of a batched step (round 4): every 16-column workgroup of a LayerNorm-fronted projection normalises its 16 rows again —
    // at 60 rows ~90 % of its instructions. Two column tiles per workgroup halve that redundant work (and the workgroup count) for the
    // wide projections (>= 128 tiles: QKV, first MLP projection).
    if (p.Mtot > 0 && p.rt_nz > 0 && p.in_mode == GEMV_IN_LN && p.xsrc == GEMV_X_PLAIN &&
        (p.out_mode == GEMV_OUT_GELU_F16 || p.out_mode == GEMV_OUT_QKV) && (p.N + 15) / 16 >= 128 && ((p.N + 15) / 16) % 2 == 0) NTB = 2;
    // ... four where the tile count allows (60 rows, Whisper-small: first projection 6.6 -> 6.1 us, first MLP projection 6.5 -> 5.9 us; the 4 x 12
    // configuration +1.5 %, profiles/r4r_*).
    if (NTB == 2 && p.Mtot > 0 && p.rt_nz > 0 && ((p.N + 15) / 16) % 4 == 0 && p.M <= 16) NTB = 4;
    // The row-tiled fp16-rows-in residual projections stage their 16 rows x K per 16-column workgroup as well. Two column tiles per
    // workgroup cost a single slot latency (4.7 -> 5.3 us per launch: half as many workgroups for a launch of 192) but save work, and with
    // three or more slots decoding on the device the GPU is work-bound: 4 x 12 windows +3 % (profiles/r4r_*). The engine
    // passes that situation in as GemvParams::busy_device.
    if (p.busy_device && p.Mtot > 0 && p.rt_nz > 0 && p.M <= 16 && p.in_mode == GEMV_IN_F16 && p.out_mode == GEMV_OUT_RESID && p.xsrc == GEMV_X_PLAIN && ((p.N + 15) / 16) % 2 == 0) NTB = 2;   // (one row tile per chunk: the only two-tile instantiation)
    // (measured and dropped, profiles/r4t_*: two tiles for the N = d_model LayerNorm + query projection under a busy device — no change;
    // four tiles for the residual projections — spills at their 1024-thread launch bound, -17 %)
    return NTB;
}
// gemv2_cfg, third decision: row tiles, whether the fp16 rows are staged through LDS, and the LDS budget
static bool gemv2_cfg_staging(const GemvParams& p, int KTf, Gemv2Cfg& c) {
    c.MT = (p.M + 15) / 16;
    c.shm = sizeof(float) * (size_t)c.nw * c.NTB * c.MT * 256;
    const size_t xs_bytes = (size_t)p.M * (KTf * 32 + 8) * sizeof(half_t);    // fp16 activation rows
    // two tiles per workgroup are an optimisation, not a requirement: where their reduction buffer plus the staged rows pass
    // a CU's LDS (large-v3's first MLP projection at 41..48 rows: 49 + 124 KiB) one tile per workgroup still runs lean —
    // this shape used to fall back to the first-generation kernel (48-row prompt-prefill chunks of large-v3)
    if (c.NTB == 2 && p.out_mode == GEMV_OUT_GELU_F16 && c.shm + xs_bytes > WLX_G2_LDS_MAX) {
        c.NTB = 1;
        c.shm = sizeof(float) * (size_t)c.nw * c.NTB * c.MT * 256;
    }
    c.xstage = true;
    // (row tiles of a batched step may stage past the default 64 KiB — large-v3's K-split MLP projection: 16 x 2560 fp16 = 82 KiB)
    const size_t xstage_max = (p.Mtot > 0 && p.rt_nz > 0) ? (size_t)WLX_G2_LDS_MAX : (size_t)64 * 1024;
    if (p.in_mode == GEMV_IN_F16 && (c.MT > 1 || c.shm + xs_bytes > xstage_max)) c.xstage = false;   // fragments from global instead
    if (c.xstage) c.shm += xs_bytes;
    if (c.shm > WLX_G2_LDS_MAX) return false;                          // beyond a CU's LDS (160 KiB, less a margin): older kernel
    if (c.shm > 64 * 1024 && g_lds_optin_refused.load(std::memory_order_relaxed)) return false;   // the device refused the raised limit once
    return true;
}
// what the lean kernel takes at all, then the three decisions in sequence; ok = false: the first-generation kernel
static Gemv2Cfg gemv2_cfg(const GemvParams& p) {
    Gemv2Cfg c{};
    if (g_decode_v1 || p.M > 48 || p.M < 1) return c;
    if (p.bias ? (p.N & 15) != 0 : p.out_mode != GEMV_OUT_F32) return c;      // bias <=> not the vocabulary projection
    const bool combo = (p.in_mode == GEMV_IN_LN && (p.out_mode == GEMV_OUT_QKV || p.out_mode == GEMV_OUT_F16 ||
                                                    p.out_mode == GEMV_OUT_GELU_F16 || p.out_mode == GEMV_OUT_F32)) ||
                       (p.in_mode != GEMV_IN_LN && p.out_mode == GEMV_OUT_RESID) ||
                       (p.in_mode == GEMV_IN_F16 && p.out_mode == GEMV_OUT_SLAB);
    if (!combo || p.K != p.KT * 32) return c;
#if WLX_KERNARG_HEAD
    if (!g2_head_fits(p)) return c;                                           // (a field past its slot of the argument head: no Whisper shape)
#endif
    // sources other than the plain rows: one row tile, and only where the kernel is instantiated for them
    if (p.xsrc != GEMV_X_PLAIN) {
        const bool ln_ok = p.in_mode == GEMV_IN_LN && p.out_mode == GEMV_OUT_QKV;
        const bool res_ok = p.in_mode == GEMV_IN_F16 && p.out_mode == GEMV_OUT_RESID && p.xsrc == GEMV_X_SLABS;
        if (!(ln_ok || res_ok)) return c;
    }
    int KTf = p.KT;                                                           // k-tiles one workgroup multiplies
    if (p.out_mode == GEMV_OUT_SLAB) {
        if (p.KTS < 1 || p.KT % p.KTS || p.KT / p.KTS != WLX_FC2_KS) return c;
        KTf = p.KTS;
    }
    if (!gemv2_cfg_waves(p, KTf, c)) return c;
    c.NTB = gemv2_cfg_tiles(p);
    c.ok = gemv2_cfg_staging(p, KTf, c);
    return c;
}

// ---- THE dispatch of dec_gemv2_kernel: one walk from (parameters, configuration) to the template arguments <CH, LNV, IN, OUT, NTB, MT, XS>,
// handed to `leaf` as a G2Args value. gemv2_ok (leaf: say yes), gemv2_launch (leaf: g2_launch) and dec_gemv_kernel_name (leaf: print the
// arguments) all go through it, so what is probed, what runs and what is named cannot differ. false: no instantiation for this configuration.
template <int CH_, int LNV_, int IN_, int OUT_, int NTB_, int MT_, int XS_>
struct G2Args { static constexpr int CH = CH_, LNV = LNV_, IN = IN_, OUT = OUT_, NTB = NTB_, MT = MT_, XS = XS_; };
// The rows a launch reads decide which (CH, LNV) pairs and which output modes exist: LayerNorm over slab / embedding rows (a layer's first
// projection), LayerNorm over plain rows, or no LayerNorm (fp16 rows in, split combine).
enum G2Rows { G2_LN_XS, G2_LN_PLAIN, G2_NO_LN };
// LayerNorm over plain rows: column tiles per workgroup, NTBMAX = what the output mode is instantiated for (four tiles: one row tile only)
template <int CH, int LNV, int OUT, int MT, int NTBMAX, class Leaf>
static bool gemv2_dispatch_ntb(const Gemv2Cfg& c, Leaf& leaf) {
    if (c.NTB == 1) return leaf(G2Args<CH, LNV, GEMV_IN_LN, OUT, 1, MT, GEMV_X_PLAIN>{});
    if constexpr (NTBMAX >= 2) { if (c.NTB == 2) return leaf(G2Args<CH, LNV, GEMV_IN_LN, OUT, 2, MT, GEMV_X_PLAIN>{}); }
    if constexpr (NTBMAX >= 4 && MT == 1) { if (c.NTB == 4) return leaf(G2Args<CH, LNV, GEMV_IN_LN, OUT, 4, 1, GEMV_X_PLAIN>{}); }
    return false;
}
template <int ROWS, int CH, int LNV, int MT, class Leaf>
static bool gemv2_dispatch_modes(const GemvParams& p, const Gemv2Cfg& c, Leaf& leaf) {
    if constexpr (ROWS == G2_LN_XS) {                 // one column tile, QKV only
        if (p.out_mode != GEMV_OUT_QKV || c.NTB != 1) return false;
        if (p.xsrc == GEMV_X_SLABS) return leaf(G2Args<CH, LNV, GEMV_IN_LN, GEMV_OUT_QKV, 1, MT, GEMV_X_SLABS>{});
        return p.xsrc == GEMV_X_EMBED && leaf(G2Args<CH, LNV, GEMV_IN_LN, GEMV_OUT_QKV, 1, MT, GEMV_X_EMBED>{});
    } else if constexpr (ROWS == G2_LN_PLAIN) {
        switch (p.out_mode) {
            case GEMV_OUT_QKV: return gemv2_dispatch_ntb<CH, LNV, GEMV_OUT_QKV, MT, 4>(c, leaf);
            case GEMV_OUT_F16: return gemv2_dispatch_ntb<CH, LNV, GEMV_OUT_F16, MT, 1>(c, leaf);
            case GEMV_OUT_GELU_F16: return gemv2_dispatch_ntb<CH, LNV, GEMV_OUT_GELU_F16, MT, 4>(c, leaf);
            case GEMV_OUT_F32: return gemv2_dispatch_ntb<CH, LNV, GEMV_OUT_F32, MT, 2>(c, leaf);
            default: return false;
        }
    } else {
        if (p.in_mode == GEMV_IN_XATTN) {             // the split combine: at most six k-tiles per wave (two items peeled per lane)
            if constexpr (CH <= 6) { if (p.out_mode == GEMV_OUT_RESID && p.xsrc == GEMV_X_PLAIN && c.NTB == 1) return leaf(G2Args<CH, 1, GEMV_IN_XATTN, GEMV_OUT_RESID, 1, MT, GEMV_X_PLAIN>{}); }
            return false;
        }
        if (p.in_mode != GEMV_IN_F16) return false;
        if (p.out_mode == GEMV_OUT_SLAB) return p.xsrc == GEMV_X_PLAIN && c.NTB == 1 && leaf(G2Args<CH, 1, GEMV_IN_F16, GEMV_OUT_SLAB, 1, MT, GEMV_X_PLAIN>{});
        if (p.out_mode != GEMV_OUT_RESID) return false;
        if (p.xsrc == GEMV_X_SLABS) return c.NTB == 1 && leaf(G2Args<CH, 1, GEMV_IN_F16, GEMV_OUT_RESID, 1, MT, GEMV_X_SLABS>{});
        if (p.xsrc != GEMV_X_PLAIN) return false;
        if (c.NTB == 1) return leaf(G2Args<CH, 1, GEMV_IN_F16, GEMV_OUT_RESID, 1, MT, GEMV_X_PLAIN>{});
        if constexpr (MT == 1) { if (c.NTB == 2) return leaf(G2Args<CH, 1, GEMV_IN_F16, GEMV_OUT_RESID, 2, 1, GEMV_X_PLAIN>{}); }   // (row tiles under a busy device)
        return false;
    }
}
// one (CH, LNV) pair of a list below; MTMAX = 3: any row-tile count of a 48-row chunk, 1: one row tile only (the wide chunks, d_model 384)
template <int ROWS, int CH, int LNV, int MTMAX, class Leaf>
static bool gemv2_dispatch_pair(const GemvParams& p, const Gemv2Cfg& c, Leaf& leaf) {
    if (c.CH != CH || c.LNV != LNV) return false;
    if (c.MT == 1) return gemv2_dispatch_modes<ROWS, CH, LNV, 1>(p, c, leaf);
    if constexpr (MTMAX == 3) return c.MT == 2 ? gemv2_dispatch_modes<ROWS, CH, LNV, 2>(p, c, leaf) : c.MT == 3 && gemv2_dispatch_modes<ROWS, CH, LNV, 3>(p, c, leaf);
    return false;
}
// The (CH, LNV) pairs that exist, once. The Whisper family: d_model 384 (2,15), 512 (4,2), 768 (6,3), 1024 (4,4) / (8,4), 1280 (5,5) / (10,5);
// slab / embedding rows run one row per wave, hence their narrower chunks (gemv2_cfg_waves). At most one pair of a list matches a configuration.
template <class Leaf>
static bool gemv2_dispatch(const GemvParams& p, const Gemv2Cfg& c, Leaf leaf) {
    if (p.in_mode == GEMV_IN_LN && p.xsrc != GEMV_X_PLAIN)
        return gemv2_dispatch_pair<G2_LN_XS, 4, 3, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 3, 3, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 2, 2, 3>(p, c, leaf) ||
               gemv2_dispatch_pair<G2_LN_XS, 4, 4, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 5, 5, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 2, 15, 1>(p, c, leaf) ||
               gemv2_dispatch_pair<G2_LN_XS, 6, 3, 1>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 8, 4, 1>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_XS, 10, 5, 1>(p, c, leaf);
    if (p.in_mode == GEMV_IN_LN)
        return gemv2_dispatch_pair<G2_LN_PLAIN, 6, 3, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_PLAIN, 5, 5, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_PLAIN, 4, 2, 3>(p, c, leaf) ||
               gemv2_dispatch_pair<G2_LN_PLAIN, 4, 4, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_PLAIN, 10, 5, 1>(p, c, leaf) || gemv2_dispatch_pair<G2_LN_PLAIN, 8, 4, 1>(p, c, leaf) ||
               gemv2_dispatch_pair<G2_LN_PLAIN, 2, 15, 1>(p, c, leaf);   // (2,15), one row tile: batched rows run as row tiles
    // no LayerNorm: 8 / 10 / 12 k-tiles per wave with fp16 rows in and one row tile only. gemv2_cfg_waves searches CH in {12, 10, 8, 6, 5, 4}
    // here: no other value arrives (the pick sweep, tests/test_gemv_picks.py).
    return gemv2_dispatch_pair<G2_NO_LN, 12, 1, 1>(p, c, leaf) || gemv2_dispatch_pair<G2_NO_LN, 10, 1, 1>(p, c, leaf) || gemv2_dispatch_pair<G2_NO_LN, 8, 1, 1>(p, c, leaf) ||
           gemv2_dispatch_pair<G2_NO_LN, 6, 1, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_NO_LN, 5, 1, 3>(p, c, leaf) || gemv2_dispatch_pair<G2_NO_LN, 4, 1, 3>(p, c, leaf);
}
// the lean kernel runs these parameters (of one row chunk: gemv_chunked) with configuration *out
static bool gemv2_ok(const GemvParams& p, Gemv2Cfg* out) {
    const Gemv2Cfg c = gemv2_cfg(p);
    if (!c.ok || !gemv2_dispatch(p, c, [](auto) { return true; })) return false;   // (the probe leaf: instantiates nothing)
    if (out) *out = c;
    return true;
}
// the fields the launcher derives from the configuration (what the kernel, and its argument head, read back)
static void gemv2_launch_fields(GemvParams& p, const Gemv2Cfg& c) {
    p.KTW = c.CH * c.NCH; p.NCH = c.NCH; p.xstage = c.xstage ? 1 : 0; p.nwm = c.nw;
    if (p.Mtot > 0 && p.chunk <= 0) p.chunk = 48;
}
static void gemv2_launch(const GemvParams& p0, const Gemv2Cfg& c, hipStream_t s) {
    GemvParams p = p0;
    gemv2_launch_fields(p, c);
#ifdef WLX_TRACE
    { static thread_local char nm[512][48]; const int q = g_trace_seq < 512 ? g_trace_seq : 511;
      snprintf(nm[q], 48, "gemv2<%d,%d,%d> N%d K%d", p.in_mode, p.out_mode, p.xsrc, p.N, p.K); p.trc = trace_next(nm[q]); }
#endif
    const int NT_total = (p.N + 15) / 16;
    dim3 grid((NT_total + c.NTB - 1) / c.NTB, p.out_mode == GEMV_OUT_SLAB ? p.KT / p.KTS : 1, p.Mtot > 0 ? (p.Mtot + p.chunk - 1) / p.chunk : 1), block(c.nw * 64);
    if (p.Mtot > 0 && p.rt_nz > 0) {       // row tiles folded into x (see dec_gemv2_kernel)
        p.rt_tiles = (int)grid.x;
        p.rt_magic = 65536 / p.rt_nz + 1;
        grid.x = ((grid.x + 7) / 8) * 8 * p.rt_nz;
        grid.z = 1;
    }
    if (p.in_mode == GEMV_IN_XATTN && c.MT > 1) {      // helper waves for the batched combine: one thread per (row, head, 8-dim group), <= 512 (the launch bound)
        const int want = (p.M * p.H * 8 + 63) / 64;
        block.x = 64 * std::max(c.nw, std::min(8, want));
    }
    const bool launched = gemv2_dispatch(p, c, [&](auto a) { using A = decltype(a); g2_launch<A::CH, A::LNV, A::IN, A::OUT, A::NTB, A::MT, A::XS>(grid, block, c.shm, s, p); return true; });
    if (!launched) dispatch_bug("dec_gemv2_kernel", s);
}
// more than 48 rows (prompt prefill): the lean kernel in row chunks of 48 (grid.z), configured for a full chunk
// 17..WLX_MAX_DEC_ROWS rows (batched decode steps): row chunks of one 16-row tile folded into blockIdx.x (round 4, see
// dec_gemv2_kernel).
static GemvParams gemv_chunked(const GemvParams& p) {
    constexpr int rt_max = WLX_MAX_DEC_ROWS;
    // rows per tile: 16 (one MFMA row tile per workgroup; 32- and 48-row tiles were measured in round 4 for <= 64 rows and lost)
    int rt_chunk = 16;
    // Round 5 (wide batches): the fp16-rows-in residual projections (attention output, cross-attention output, MLP down: 1024-thread
    // workgroups, one per CU, no LayerNorm prologue to repeat) take two or three row tiles per workgroup where that saves ROUNDS of
    // workgroups: N = 768 at 120 rows is 48 x 8 = 384 workgroups on 256 CUs with 16-row tiles, 192 with 32-row tiles (6.7 -> 5.8 us per
    // launch; large-v3 at 160 rows 16.7 -> 13.9 us; profiles/r5h_rowtile_chunk_by_rows.txt). Cost model: rounds x (1 + 0.35 per extra row
    // tile). The LayerNorm-fronted projections stay on 16 rows (every workgroup re-normalises its rows: 32-row tiles measured 10-40 % slower).
    if (p.in_mode == GEMV_IN_F16 && p.out_mode == GEMV_OUT_RESID && p.xsrc == GEMV_X_PLAIN && !p.busy_device && p.M > 64) {
        static const int n_cu = [] { int dev = 0, n = 256; (void)hipGetDevice(&dev); hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) n = pr.multiProcessorCount; return n; }();
        const int tiles = (p.N + 15) / 16;
        double best = 1e300;
        for (int mt = 1; mt <= 3; ++mt) {
            const long wgs = (long)tiles * ((p.M + 16 * mt - 1) / (16 * mt));
            const double cost = (double)((wgs + n_cu - 1) / n_cu) * (1.0 + 0.35 * (mt - 1));
            if (cost < best - 1e-9) { best = cost; rt_chunk = 16 * mt; }
        }
    }
    GemvParams q = p;
    if (p.Mtot != 0 || p.in_mode == GEMV_IN_XATTN) return q;
    // Which projections: measured per kernel at 20 / 40 / 60 rows (profiles/r4a-c_*): row tiles win wherever the launch has few
    // column tiles (N = d_model: 7.1 -> 4.2 us at 60 rows, large-v3 6.7 -> 4.8 us at 40) and for Whisper-small's wide ones
    // (first MLP projection 10.3 -> 6.9 us); large-v3's N = 3 d / 4 d projections (10-13 MB of weights re-read per row tile
    // through L2) were faster as three-tile workgroups (8.7 vs 11.8 us, 9.1 vs 9.8 us) — with ONE column tile per workgroup. With the four
    // column tiles per workgroup the row-tiled LayerNorm projections got later in the round they are not (large-v3, 40 rows: first
    // projection 8.8 -> 7.7 us, first MLP projection 9.2 -> 7.6 us, step 2183 -> 2087 us; profiles/r4lv3rt_decode_step.txt): every
    // LayerNorm-fronted projection whose tile count divides by four is cut too from three row tiles up (60 rows: 3157 -> 2857 us; 20 rows,
    // two row tiles: 1845 -> 1905 us, left as it was).
    const bool ln_wide4 = rt_chunk == 16 && p.M > 32 && p.in_mode == GEMV_IN_LN && p.xsrc == GEMV_X_PLAIN && (p.out_mode == GEMV_OUT_QKV || p.out_mode == GEMV_OUT_GELU_F16) &&
                          (p.N & 15) == 0 && ((p.N >> 4) & 3) == 0;
    const bool rt_shape = p.N <= 1536 || (long)p.N * p.K <= 3200000L || ln_wide4;
    if (!g_decode_v1 && p.M > rt_chunk && p.M <= rt_max && rt_shape) { q.Mtot = p.M; q.M = rt_chunk; q.chunk = rt_chunk; q.rt_nz = (p.M + rt_chunk - 1) / rt_chunk; }
    else if (p.M > 48 && p.xsrc != GEMV_X_EMBED) { q.Mtot = p.M; q.M = 48; q.chunk = 48; }
    return q;
}
// (Round 6, measured and dropped — "wide passes": from 64 / 128 rows the LayerNorms as their own launch (fp16 rows, the prologue's arithmetic) and
// every K = d_model projection with fp16 rows in on 64-ROW tiles (MT = 4, one or two column tiles per workgroup), so that a weight tile is fetched
// from L2 once per 64 rows instead of once per 16. Parity green (210 GPU tests). Whisper-small at 120 / 240 rows: step 1.007 / 1.442 ms against
// 0.913 / 1.365 ms on the 16-row tiles; large-v3 at 80 / 160 rows: 3.61 / 4.85 against 3.06 / 5.03 ms — the three LayerNorm launches per layer
// (2 us each) and the 64-row workgroups' lower occupancy cost what the saved L2 re-reads give back; only large-v3 at 160 rows gains (3.6 %).
// profiles/r6c_wide_rows_*, r6d_wide_rows_*; DESIGN.md §7.3 B4. The 16-row tiles stay.)

int dec_gemv_slab_split(int M, int K, int N) {
    if (WLX_FC2_KS < 2) return 0;                                             // (the slab count is a compile-time constant of the consumers: -DWLX_FC2_KS)
    if (g_decode_v1 || M < 1 || K % 32 || (K / 32) % WLX_FC2_KS || K < 2048) return 0;
    GemvParams p0{};
    p0.in_mode = GEMV_IN_F16; p0.out_mode = GEMV_OUT_SLAB; p0.M = M; p0.K = K; p0.KT = K / 32; p0.N = N; p0.KTS = p0.KT / WLX_FC2_KS;
    static const float dummy_bias = 0.f;
    p0.bias = &dummy_bias;                                                    // (cfg only asks whether there is one)
    const GemvParams p = gemv_chunked(p0);                                    // row chunks: decided for a full chunk (16 or 48 rows)
    Gemv2Cfg c;
    if (!gemv2_ok(p, &c) || (p.M <= 16 && !c.xstage)) return 0;
    return WLX_FC2_KS;
}

template <int MT, int NTB>
static void gemv_dispatch_in(const GemvParams& p, dim3 grid, dim3 block, size_t shm, hipStream_t s) {
    switch (p.in_mode) {
        case GEMV_IN_LN: hipLaunchKernelGGL((dec_gemv_kernel<MT, NTB, GEMV_IN_LN>), grid, block, shm, s, p); break;
        case GEMV_IN_F16: hipLaunchKernelGGL((dec_gemv_kernel<MT, NTB, GEMV_IN_F16>), grid, block, shm, s, p); break;
        default: hipLaunchKernelGGL((dec_gemv_kernel<MT, NTB, GEMV_IN_XATTN>), grid, block, shm, s, p); break;
    }
}

bool dec_gemv_head(const GemvParams& p_any, GemvHead* h, GemvParams* launched) {
    if (vocab2_ok(p_any)) return false;
    GemvParams p = gemv_chunked(p_any);
    Gemv2Cfg c;
    if (!gemv2_ok(p, &c)) return false;
    gemv2_launch_fields(p, c);
    *launched = p;
    return g2_head(p, h);
}
bool dec_gemv_is_lean(const GemvParams& p) { return vocab2_ok(p) || gemv2_ok(gemv_chunked(p), nullptr); }

// the name leaf of gemv2_dispatch (the vocabulary projection names itself): the template arguments of the instantiation launch_dec_gemv runs, not a
// second account of them
const char* dec_gemv_kernel_name(const GemvParams& p_any) {
    if (vocab2_ok(p_any)) return vocab2_kernel_name(p_any);
    static thread_local char buf[64];
    const GemvParams p = gemv_chunked(p_any);
    Gemv2Cfg c2;
    if (gemv2_ok(p, &c2)) {
        gemv2_dispatch(p, c2, [&](auto a) { using A = decltype(a); snprintf(buf, sizeof(buf), "dec_gemv2_kernel<%d, %d, %d, %d, %d, %d, %d>", A::CH, A::LNV, A::IN, A::OUT, A::NTB, A::MT, A::XS); return true; });
        return buf;
    }
    const int MT = (p.M + 15) / 16;
    snprintf(buf, sizeof(buf), "dec_gemv_kernel<%d, %d, %d>", MT > 4 ? 4 : MT, MT == 1 ? 2 : 1, p.in_mode);
    return buf;
}

void launch_dec_gemv(const GemvParams& p, hipStream_t s) {
    if (vocab2_ok(p)) { vocab2_launch(p, s); return; }
    Gemv2Cfg c2;
    const GemvParams pc = gemv_chunked(p);
    if (gemv2_ok(pc, &c2)) { gemv2_launch(pc, c2, s); return; }   // (from here on the first-generation kernel: it knows neither xsrc nor GEMV_OUT_SLAB)
    if (p.M > 16 * WLX_MAX_MT) {
        // the general kernel holds WLX_MAX_MT row tiles per launch: a wider pass (round 5) runs as consecutive row chunks on rebased row
        // pointers (64 rows; the split-combine prologue indexes its partials by (item, row in item), so its chunks are whole items)
        const int CHK = (p.in_mode == GEMV_IN_XATTN && p.R > 0) ? (16 * WLX_MAX_MT / p.R) * p.R : 16 * WLX_MAX_MT;
        for (int r0 = 0; r0 < p.M; r0 += CHK) {
            GemvParams q = p;
            q.M = std::min(CHK, p.M - r0);
            if (q.X) q.X += (long)r0 * q.ldx;
            if (q.Xh) q.Xh += (long)r0 * q.ldxh;
            if (q.Yh) q.Yh += (long)r0 * q.ldyh;
            if (q.Y) q.Y += (long)r0 * q.ldy;
            if (q.Xres) q.Xres += (long)r0 * q.ldxres;
            if (q.row_cache) q.row_cache += r0;
            if (q.row_pos) q.row_pos += r0;
            if (q.in_mode == GEMV_IN_XATTN) {
                const int items0 = r0 / q.R;
                q.part_o += (long)items0 * q.H * WLX_XSPLIT * 16 * 64;
                q.part_ml += (long)items0 * q.H * 16 * WLX_XSPLIT * 2;
            }
            launch_dec_gemv(q, s);
        }
        return;
    }
    const int MT = (p.M + 15) / 16;
    const int NT_total = (p.N + 15) / 16;
    // waves per workgroup: enough K-split that each wave streams <= GV_CH k-tiles per chunk and,
    // in LN mode, exactly one chunk. Wide-N projections keep 4 waves; the big-K fc2 uses more.
    int nw = (p.KT + GV_CH - 1) / GV_CH;
    if (nw < 1) nw = 1;
    if (nw > 8) nw = 8;    // 512-thread workgroups keep 256 VGPRs per lane (LN mode: d_model <= 8*6*32 = 1536)
    const int NTB = (MT == 1) ? 2 : 1;
    dim3 grid((NT_total + NTB - 1) / NTB), block(nw * 64);
    const size_t shm = sizeof(float) * ((size_t)2 * nw * MT * 16 + (size_t)nw * NTB * MT * 256);
    switch (MT) {
        case 1: gemv_dispatch_in<1, 2>(p, grid, block, shm, s); break;
        case 2: gemv_dispatch_in<2, 1>(p, grid, block, shm, s); break;
        case 3: gemv_dispatch_in<3, 1>(p, grid, block, shm, s); break;
        default: gemv_dispatch_in<4, 1>(p, grid, block, shm, s); break;
    }
}

}  // namespace wlx
