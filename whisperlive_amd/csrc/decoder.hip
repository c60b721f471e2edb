// decoder.hip — one autoregressive decoder step on gfx950 (the inner loop of
// ctranslate2.models.Whisper.generate, called from
// whisper_live/transcriber/transcriber_faster_whisper.py:1394-1407 and
// whisper_live/batch_inference.py:355-357; network: HF modeling_whisper.py:416-498).
//
// The step is HBM/latency bound: M = beams x items (5..40) rows against ~278 MB of fp16 weights
// (Whisper-small). Every projection is a skinny GEMM  Y[M x N] = X[M x K] * W^T  done with MFMA
// 16x16x32 in the swapped form (weights = A operand, read as pre-packed contiguous 1 KiB
// fragments straight into registers; the <=64 activation rows = B operand held in registers),
// K split across the waves of a workgroup and combined through LDS, so each weight byte is read
// exactly once per step and stores are deterministic (no atomics). LayerNorm is fused into the
// prologue of the consuming projection (the weight fragment loads are issued BEFORE the
// prologue so their HBM latency overlaps the statistics), bias / GELU / residual-accumulate /
// q-scaling / KV-cache append into the epilogue. Beam reordering never moves the KV cache: an
// int16 ancestry table maps (row, position) -> cache row. All per-step scalars (position,
// tokens, ancestry, done flag) live in device memory so one captured hipGraph replays every step.
// This file: the embedding, the self- and cross-attention kernels, the split combine and the alignment scores. The projections are in
// dec_gemv.hip (skinny GEMMs and their dispatch) and dec_vocab.hip (the vocabulary projection).
#include "decoder.h"

namespace wlx {

bool g_decode_v1 = false;

#ifdef WLX_TRACE
unsigned long long* g_trace_buf = nullptr;
int g_trace_seq = 0;
const char* g_trace_names[512];
#endif

// ------------------------------------------------------------------ embedding
__global__ __launch_bounds__(256) void dec_embed_kernel(const half_t* __restrict__ tok_emb,
                                                        const float* __restrict__ pos_emb, int d,
                                                        const int* __restrict__ token,
                                                        const int* __restrict__ pos,
                                                        const int* __restrict__ cache, int* __restrict__ intok,
                                                        float* __restrict__ x, const int* __restrict__ done WLX_TR_PARAM) {
    if (done && *done) return;
    WLX_TR_BEGIN();
    const int r = blockIdx.x;
    const int tok = token[r], p = pos[r];
    if (threadIdx.x == 0) intok[(long)cache[r] * WLX_T_TEXT + p] = tok;
    const half_t* te = tok_emb + (long)tok * d;
    const float* pe = pos_emb + (long)p * d;
    for (int i = threadIdx.x * 4; i < d; i += 256 * 4) {
        f16x4 t = ld_f16x4(te + i);
        float4 pv = *reinterpret_cast<const float4*>(pe + i);
        *reinterpret_cast<float4*>(x + (long)r * d + i) =
            make_float4((float)t[0] + pv.x, (float)t[1] + pv.y, (float)t[2] + pv.z, (float)t[3] + pv.w);
    }
    WLX_TR_END(trc);
}

void launch_dec_embed(const half_t* tok_emb, const float* pos_emb, int d, const RowTables& rt, int rows,
                      float* x, const int* done, hipStream_t s) {
    hipLaunchKernelGGL(dec_embed_kernel, dim3(rows), dim3(256), 0, s, tok_emb, pos_emb, d, rt.token, rt.pos,
                       rt.cache, rt.intok, x, done WLX_TR_ARG("embed"));
}

// ------------------------------------------------------------------ causal self-attention over the KV cache
// One wave per (row, head); positions 0..pos[row]; the history of a row is read through the ancestry table.
// Flash-style over blocks of 64 positions so one rolled loop serves every length (code size is latency here: the
// two-pass form was 4.6 KiB of straight-line code, ~1.8 us of cold instruction fetch per launch):
//   per block: lane p looks up the cache row of position p (one dependent trip), then the K and the V rows are requested together — one
//   more trip —, both as lane = (position group pg, 8-dim chunk dc): 8 positions x a whole 128-byte row per load instruction (round 6; the
//   K rows were lane = position before), scores = 8 dims in the lane + a 3-step DPP butterfly over the 8 dc lanes, block max / sum by DPP,
//   and the (pg, dc) lanes accumulate their 8 dims over their 8 positions with the running-max rescale (their probabilities are in-lane).
//   tail: the 8 position groups are summed through LDS, lane d writes output dim d.
// IDENT: the rows read their history through their OWN ancestry row (every decode step; prefill rows share one): the
// ancestry row address then needs no table lookup, so the first block's cache-row lookup is requested at once, next to
// the scalar loads of the row's position, instead of behind them — one dependent trip less (of three) per launch.
// Round 3: SA_NW waves per (row, head). A wave walks every SA_NW-th block of 64 positions and the waves' (m, l, o) are merged
// through LDS in a fixed order. With one wave the blocks of a long history were a serial chain of dependent round trips
// (ancestry -> K / V -> softmax): a step at positions 225..288 (a window conditioned on the reference's full prompt) cost
// 6.4 us per layer here against 2.9 us at t = 32. Histories of <= 64 positions run exactly as before on wave 0 — the other
// waves leave at once, and ended waves do not count at the barrier.
// Round 6: EIGHT waves — one block of 64 positions per wave up to the 448-position context, no wave walks a second block. Measured twice: with
// the K rows fetched lane = position a step at positions 200 / 300 / 447 cost 398 / 412 / 425 us with 4 or 8 waves (profiles/r6b_*: the K fetch
// was what grew); with whole-row K fetches 390 / 408 / 411 us with 4 waves and 390 / 396 / 402 with 8 (profiles/r6w_step_by_position_sa8.txt) —
// now the second dependent trip is what is left. Histories of <= 256 positions are bit-identical to the 4-wave form (same blocks, same merge order).
// The decode steps (IDENT) run 8 waves; the prompt prefill (<= 228 positions, thousands of workgroups) keeps 4 — with 8 its 224-token pass
// measured 0.94 against 0.91 ms (four waves per workgroup launched only to leave).
constexpr int SA_PF_NW = 4;   // the non-IDENT passes (prompt prefill, teacher-forced rows) and batched steps (> 16 rows)
constexpr int SA_NW = 8;      // the steps of one stream (IDENT, <= 16 rows)
template <bool IDENT, int NW>
__global__ __launch_bounds__(64 * NW) void dec_self_attn2_kernel(const half_t* __restrict__ q, long ldq,
                                                                    const half_t* __restrict__ Kc,
                                                                    const half_t* __restrict__ Vc, long crs, int d,
                                                                    const int* __restrict__ pos,
                                                                    const int* __restrict__ ancrow,
                                                                    const short* __restrict__ anc,
                                                                    half_t* __restrict__ out, long ldo WLX_TR_PARAM) {
    __shared__ int crow_s[NW][64];
    __shared__ float part_s[NW][8][64];
    __shared__ float ml_s[NW][2];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x, h = blockIdx.y;
    WLX_TR_BEGIN();
    // the cache rows of this wave's FIRST block, requested together with the row's position, before anything depends on either
    // (clamped to the ancestry row's 448 entries, whatever the history length turns out to be) — without it
    // the waves of the later blocks paid a second dependent round trip (position -> ancestry -> K / V)
    const short* ar = anc + (long)(IDENT ? r : ancrow[r]) * WLX_T_TEXT;
    int cr0 = 0;
    if constexpr (IDENT) cr0 = ar[(w * 64 + lane < WLX_T_TEXT) ? w * 64 + lane : WLX_T_TEXT - 1];   // (8 x 64 > 448: the last wave's lanes past the row)
    const int len = pos[r] + 1;
    const int nblk = (len + 63) >> 6;
    if (w >= nblk) return;                                  // (wave 0 always stays: len >= 1)
    int* crow = crow_s[w];
    const int pg = lane >> 3, dc = lane & 7;
    const int hoff = h * WLX_HEAD_DIM;
    float qf[8];                                            // this lane's 8 query dims (dc * 8 ..)
    {
        const f16x8 qv = ld_f16x8(q + (long)r * ldq + hoff + dc * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)qv[e];
    }
    const int icrs = (int)crs;                             // 32-bit element offsets: cache_rows * 448 * d < 2^31
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float mrun = WLX_NEG_INF, lrun = 0.f;
    WLX_TR_MARK(1);
#pragma unroll 1
    for (int p0 = w * 64; p0 < len; p0 += 64 * NW) {
        const int p = p0 + lane;
        const bool ok = p < len;
        int cr;
        if (IDENT && p0 == w * 64) cr = ok ? cr0 : __builtin_amdgcn_readlane(cr0, 0);  // (a masked lane: any valid row — the block's first position's)
        else cr = ar[ok ? p : len - 1];
        crow[lane] = cr;                                    // (visible to this same wave after the wait the reads below carry)
        // K AND V chunks, the same element offsets in both caches: lane (pg, dc) takes dims dc*8 .. dc*8+7 of positions p0 + u*8 + pg, so a
        // load instruction covers 8 positions x one whole 128-byte row each = 8 cache lines. (Through round 5 the K rows were read lane =
        // position, 16 bytes of 64 different lines per instruction, eight times over: the step grew 48 us from position 8 to 447, twice what the
        // bytes cost — profiles/r6b_step_by_position.txt.)
        f16x8 kk[8], vv[8];
        bool okp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int pp = p0 + u * 8 + pg;
            okp[u] = pp < len;
            const unsigned off = (unsigned)(crow[u * 8 + pg] * icrs + (okp[u] ? pp : len - 1) * d + hoff + dc * 8);
            kk[u] = ld_f16x8(Kc + off);
            vv[u] = ld_f16x8(Vc + off);
        }
        // scores: 8 dims in the lane, then the 8 dc lanes of a position summed by a 3-step butterfly (all 8 end with the same bits)
        float sc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaf((float)kk[u][e], qf[e], a);
            sc[u] = a;
        }
        WLX_DPP_SUM8x8(sc);
        float bm = WLX_NEG_INF;
#pragma unroll
        for (int u = 0; u < 8; ++u) { sc[u] = okp[u] ? sc[u] : WLX_NEG_INF; bm = fmaxf(bm, sc[u]); }
        const float mnew = fmaxf(mrun, dpp_wave_max(bm));   // finite: position p0 is valid
        const float alpha = __expf(mrun - mnew);
        float pe[8], bs = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) { pe[u] = __expf(sc[u] - mnew); bs += pe[u]; }   // 0 for masked positions
        lrun = lrun * alpha + dpp_wave_sum(dc == 0 ? bs : 0.f);                      // (each position once: its dc = 0 lane)
        mrun = mnew;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = fmaf(pe[u], (float)vv[u][e], o[e]);
    }
    WLX_TR_MARK(2);
    // sum the 8 position groups: part[pg][dim]; lane d then owns output dim d
    *reinterpret_cast<float4*>(&part_s[w][pg][dc * 8]) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(&part_s[w][pg][dc * 8 + 4]) = make_float4(o[4], o[5], o[6], o[7]);
    float acc = 0.f;
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) acc += part_s[w][g8][lane];
    if (nblk == 1) {                                        // one block: wave 0 alone, as before
        out[(long)r * ldo + hoff + lane] = (half_t)(acc / lrun);
    } else {
        // merge the waves' partial (m, l, o) in wave order: o = sum_w o_w e^(m_w - m), l = sum_w l_w e^(m_w - m)
        part_s[w][0][lane] = acc;                           // (this wave's own row of part_s: read above by the same lanes' wave only)
        if (lane == 0) { ml_s[w][0] = mrun; ml_s[w][1] = lrun; }
        __syncthreads();                                    // the waves that left at the top do not count
        if (w == 0) {
            const int nw = nblk < NW ? nblk : NW;
            float m = ml_s[0][0];
            for (int k = 1; k < nw; ++k) m = fmaxf(m, ml_s[k][0]);
            float L = 0.f, O = 0.f;
            for (int k = 0; k < nw; ++k) {
                const float f = __expf(ml_s[k][0] - m);
                L += ml_s[k][1] * f;
                O += part_s[k][0][lane] * f;
            }
            out[(long)r * ldo + hoff + lane] = (half_t)(O / L);
        }
    }
    WLX_TR_MARK(3);
    WLX_TR_END(trc);
}

void launch_dec_self_attn(const half_t* q, long ldq, const half_t* Kc, const half_t* Vc, long crs, int d, int H,
                          const RowTables& rt, int rows, half_t* out, long ldo, const int* done, bool ident_ancestry, hipStream_t s) {
    (void)done;   // a step that runs after the search raised `done` only rewrites scratch (engine_decode.hip decoder_pass)
    // 8 waves for the steps of one stream (<= 16 rows: up to 16 x H workgroups, the launch is one latency chain long); batched steps (hundreds of
    // rows x H workgroups) keep 4, like the prefill: their extra waves would only be launched to leave
    if (ident_ancestry && rows <= 16)
        hipLaunchKernelGGL((dec_self_attn2_kernel<true, SA_NW>), dim3(rows, H), dim3(64 * SA_NW), 0, s, q, ldq, Kc, Vc, crs, d, rt.pos,
                           rt.ancrow, rt.anc, out, ldo WLX_TR_ARG("self_attn"));
    else if (ident_ancestry)
        hipLaunchKernelGGL((dec_self_attn2_kernel<true, SA_PF_NW>), dim3(rows, H), dim3(64 * SA_PF_NW), 0, s, q, ldq, Kc, Vc, crs, d, rt.pos,
                           rt.ancrow, rt.anc, out, ldo WLX_TR_ARG("self_attn"));
    else
        hipLaunchKernelGGL((dec_self_attn2_kernel<false, SA_PF_NW>), dim3(rows, H), dim3(64 * SA_PF_NW), 0, s, q, ldq, Kc, Vc, crs, d, rt.pos,
                           rt.ancrow, rt.anc, out, ldo WLX_TR_ARG("self_attn"));
}

// ------------------------------------------------------------------ decode cross-attention (flash-decoding split over keys)
// grid (split, head, group): the R rows of an item share the item's encoder K/V, so they form ONE 16-row MFMA query
// tile (scores transposed as in attention.hip: S^T = K Q^T, softmax in-lane + 2 DPP steps, O^T = V^T P^T).
// One WORKGROUP of XA_TPS waves per (split, head, group), one 32-key tile per wave: six waves pull 8 KiB each, form
// their (m, l, O) over one tile and merge through LDS into the split's partial.
//   * K and V come TILE-PACKED from the encoder's cross-K/V GEMM epilogue (gemm.hip GEMM_CROSS_KV): per (layer, item,
//     head, 32-key tile) a 4 KiB image in MFMA operand order, so every load is one contiguous 1 KiB per wave (the
//     row-major K / transposed V of the first generations cost 12 strided loads of 32-64 byte segments per tile);
//     keys >= 1500 of the padding are zero in V (never written) and masked to -inf in the scores.
//   * the partial handed to the consumer projection is the NORMALISED fp16 O plus fp32 (m, l), the (m, l) of a row's
//     eight splits contiguous: the consumer's combine is bound by load-instruction count per CU, not by bytes.
#define XA_TPS (WLX_T_AUDIO_PAD / 32 / WLX_XSPLIT)
__global__ __launch_bounds__(XA_TPS * 64) void dec_cross_attn_kernel(const half_t* __restrict__ q, long ldq,
                                                                     const half_t* __restrict__ Kp, const half_t* __restrict__ Vp,
                                                                     long item_stride, int H, int R, int rows,
                                                                     const int* __restrict__ group_item,
                                                                     half_t* __restrict__ part_o, float* __restrict__ part_ml WLX_TR_PARAM) {
    constexpr int TPS = XA_TPS;
    static_assert(TPS * WLX_XSPLIT * 32 == WLX_T_AUDIO_PAD && TPS >= 4, "key padding must cover every split; >= 4 waves combine");
    __shared__ __attribute__((aligned(16))) float Os[TPS][16][68];
    __shared__ float MLs[TPS][16][2];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sp = blockIdx.x, h = blockIdx.y, grp = blockIdx.z;
    WLX_TR_BEGIN();
    const int item = group_item[grp];
    constexpr int T = WLX_T_AUDIO;
    const int tile = sp * TPS + wave;
    const int key0 = tile * 32;
    const long toff = (long)item * item_stride + ((long)h * (WLX_T_AUDIO_PAD / 32) + tile) * 2048 + lane * 8;
    f16x8 kf[2][2], vf[4];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) kf[s2][kt] = ld_f16x8(Kp + toff + (s2 * 2 + kt) * 512);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vf[dt] = ld_f16x8(Vp + toff + dt * 512);
    int row = grp * R + c;
    const bool qok = (c < R) && (row < rows);
    if (!qok) row = grp * R;  // any valid row; result discarded
    f16x8 qf[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) qf[kt] = ld_f16x8(q + (long)row * ldq + h * WLX_HEAD_DIM + kt * 32 + g * 8);
    WLX_TR_MARK(1);

    f32x4 st[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) st[s2] = mfma16(kf[s2][kt], qf[kt], st[s2]);
    }
    float pv[8];
    float tmax = WLX_NEG_INF;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = key0 + s2 * 16 + g * 4 + r;
            const float v = (key < T) ? st[s2][r] : WLX_NEG_INF;
            pv[s2 * 4 + r] = v;
            tmax = fmaxf(tmax, v);
        }
    tmax = rows4_max(tmax);                                      // (v_permlane swaps instead of ds_bpermute round trips: see dec_cq_cross_attn_kernel)
    const float msafe = (tmax == WLX_NEG_INF) ? 0.f : tmax;      // a fully masked tile: every p = exp(-inf) = 0
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { pv[i] = __expf(pv[i] - msafe); psum += pv[i]; }
    psum = rows4_sum(psum);
    const f16x8 pf = {(half_t)pv[0], (half_t)pv[1], (half_t)pv[2], (half_t)pv[3],
                      (half_t)pv[4], (half_t)pv[5], (half_t)pv[6], (half_t)pv[7]};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const f32x4 a = mfma16(vf[dt], pf, (f32x4){0.f, 0.f, 0.f, 0.f});
        *reinterpret_cast<f32x4*>(&Os[wave][c][dt * 16 + g * 4]) = a;
    }
    if (g == 0) { MLs[wave][c][0] = tmax; MLs[wave][c][1] = psum; }
    WLX_TR_MARK(2);
    __syncthreads();
    if (wave < 4) {
        // wave dt merges output dims dt*16 .. dt*16+15 of all 16 query rows over the TPS tiles (fixed order)
        const int dt = wave;
        float mw[TPS], lw[TPS];
        float M = WLX_NEG_INF;
#pragma unroll
        for (int w = 0; w < TPS; ++w) { mw[w] = MLs[w][c][0]; lw[w] = MLs[w][c][1]; M = fmaxf(M, mw[w]); }
        float l = 0.f;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < TPS; ++w) {
            const float e = (mw[w] == WLX_NEG_INF) ? 0.f : __expf(mw[w] - M);
            l += e * lw[w];
            const f32x4 t = *reinterpret_cast<const f32x4*>(&Os[w][c][dt * 16 + g * 4]);
            o[0] += e * t[0]; o[1] += e * t[1]; o[2] += e * t[2]; o[3] += e * t[3];
        }
        const long ih = (long)grp * H + h;
        const float inv = 1.0f / l;               // every split starts below key 1500: l > 0
        const f16x4 hv = {(half_t)(o[0] * inv), (half_t)(o[1] * inv), (half_t)(o[2] * inv), (half_t)(o[3] * inv)};
        *reinterpret_cast<f16x4*>(part_o + ((ih * WLX_XSPLIT + sp) * 16 + c) * 64 + dt * 16 + g * 4) = hv;
        if (dt == 0 && g == 0) *reinterpret_cast<float2*>(part_ml + (ih * 16 + c) * (WLX_XSPLIT * 2) + sp * 2) = make_float2(M, l);
    }
    WLX_TR_MARK(3);
    WLX_TR_END(trc);
}

// ------------------------------------------------------------------ fused LayerNorm + cross-attention query + cross-attention
// One launch instead of two (LN2 + q projection, then attention): the workgroup of (split, head, group) computes the
// 64 query columns of ITS head for the group's <= 16 rows itself — LayerNorm of the rows (one wave per row, DPP), the
// head's 4 n-tiles x KT k-tiles of Wcq streamed by its six waves (KT/6 k-tiles x 4 n-tiles each), K-reduction through
// LDS — and goes straight on to its 32-key tiles. The eight split-workgroups of a head repeat the head's 96 KiB of Wcq;
// the blockIdx -> (head, split) map puts them on ONE XCD (workgroup ids are dealt round-robin over the 8 XCDs), so the
// repeats are L2 hits, not HBM reads. What it buys: one launch boundary (1.6 us) and one launch's fixed latency per
// layer; what it costs: ~200 load instructions per CU instead of ~60 (2.2 us of issue at ~11 ns each).
// Eligibility (launcher): d_model = 256 * LNV with KT % 6 == 0 — Whisper-small; other sizes keep the two launches.
// Argument order (kernel-argument preload, 14 dwords): everything the requests in front of the K / V loads need — row base and stride, gamma, beta,
// the weights, the group table, R, rows — arrives in SGPRs at wave start; H and KT are the template's (the launcher serves d_model = 256 * LNV only).
// The tail (bias, q scale, K / V bases and stride, the partials) is fetched by the wave and first waited for behind the weight requests.
template <int LNV, int KPW>
__global__ __launch_bounds__(XA_TPS * 64) void dec_cq_cross_attn_kernel(
    const float* X, long ldx, const float* __restrict__ gamma, const float* __restrict__ beta,
    const half_t* __restrict__ Wp, const int* __restrict__ group_item, int R, int rows,
    const half_t* __restrict__ Kp, const half_t* __restrict__ Vp, long item_stride, const float* __restrict__ bias, float qscale,
    half_t* __restrict__ part_o, float* __restrict__ part_ml WLX_TR_PARAM) {
    constexpr int TPS = XA_TPS;
    constexpr int H = 4 * LNV, KT = 8 * LNV;
    static_assert(TPS == 6 && KT == TPS * KPW, "six waves: KT/6 k-tiles of the query projection and one key tile each");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    WLX_TR_BEGIN();
    // ---- grid (H x splits, groups). The group's item is the one value of the front that lives in memory: requested FIRST, from an address made of
    // preloaded SGPRs alone, and waited for in front of the K / V requests only. (It was requested between the LayerNorm operands and the weights and
    // waited for right there: a scalar round trip, cache-cold at every launch, behind the argument fetch that H, R and rows needed, with the sixteen
    // weight requests and the gamma / beta exchange queued behind both.)
    const int grp = blockIdx.y, wg = blockIdx.x;
    const int item_rq = group_item[grp];
    // ---- (head, split) of this workgroup: the 8 splits of a head share blockIdx.x % 8, i.e. one XCD (H * 8 is a multiple of 8: in every group)
    int h, sp;
    {
        const int x = wg & 7, j = wg >> 3, full = H >> 3, rem = H & 7;
        if (rem == 0 || rem == 4) {                                        // (selects, not branches: H is a constant here)
            const bool whole = j < 8 * full;
            h = whole ? (j >> 3) * 8 + x : 8 * full + (x >> 1);
            sp = whole ? (j & 7) : (x & 1) * 4 + (j - 8 * full);
        } else { h = wg >> 3; sp = wg & 7; }
    }
    constexpr int d = KT * 32;
    constexpr int ldxs = d + 8;
    // LDS: [0, xs_bytes) fp16 LayerNorm rows; then a region shared in time by the K-reduction partials and the
    // attention merge buffers; then the 16 x 64 fp16 query tile
    half_t* xs = reinterpret_cast<half_t*>(smem);
    float* regB = smem + ((R * ldxs * 2 + 15) / 16) * 4;
    float* accred = regB;                                                  // [6][4][64][4]
    float (*Os)[16][68] = reinterpret_cast<float (*)[16][68]>(regB);       // [6][16][68]
    float* MLs = regB + TPS * 16 * 68;                                     // [6][16][2]
    half_t* qs = reinterpret_cast<half_t*>(MLs + TPS * 16 * 2);            // [16][72]

    // ---- request order: row of the first trip, this wave's [gamma | beta] piece, the 16 weight fragments — nothing in front of
    // them waits for memory — then the gamma / beta exchange and the first trip's LayerNorm, then K / V and the bias. The row comes FIRST (round 2):
    // vmcnt retires in order. The workgroup's 174 wave-level loads take ~1.9 us to issue (one per ~11 ns per CU) and every wave used to reach the
    // exchange's LDS store, the barrier and its LayerNorm only behind all 29 of its own: the rows were normalised when the LAST load had landed. Now
    // the exchange stands behind 20 requests and the LayerNorm runs while the weights are in flight; K / V, first needed behind the query
    // projection, are requested behind it. (X is not __restrict__ on purpose: as invariant loads the row requests are tied to nothing and hipcc
    // placed them behind the weights; as ordinary loads they keep their place between the fences.)
    const int nrow = (rows - grp * R < R) ? rows - grp * R : R;           // live rows of this group
    float4 x0[LNV];
    {
        const int r0 = (wave < nrow) ? wave : nrow - 1;
        const float4* x4 = reinterpret_cast<const float4*>(X + (long)(grp * R + r0) * ldx) + lane;
#pragma unroll
        for (int j = 0; j < LNV; ++j) x0[j] = x4[64 * j];
    }
    // gamma / beta (round 6, log G1): ONE KiB piece of [gamma | beta] per wave (six waves, 2 x 3 pieces) instead of all of both on every wave,
    // shared through LDS before the first row is normalised — 30 of the workgroup's 204 wave-level loads less in front
    // of its weights and K / V, and this launch is bound by exactly that count (a CU retires one per ~11 ns, L1 hit or not). Same values into the
    // same arithmetic: bit-identical. In-kernel timeline (profiles/r6ad_*): rows normalised 0.26 us LATER (the exchange's barrier), query tile
    // ready 0.35 us earlier, workgroup 5.06 -> 4.76 us. The same exchange in dec_gemv2_kernel's LayerNorm prologues measured the other way — first
    // projection 2.04 -> 2.27 us, first MLP projection 1.90 -> 2.31 us per workgroup, step graph +11 us: there the weights are 24 of 72-120 loads
    // and a wave's normalisation waited for nobody else's loads (scripts/patches/r6ad_*.diff) — so it is used here only.
    static_assert(2 * LNV == TPS, "one [gamma | beta] piece per wave");
    float4 gq[LNV], bq[LNV];
    float4 gbp = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const float* src = (wave < LNV) ? gamma + wave * 256 : beta + (wave - LNV) * 256;
        gbp = reinterpret_cast<const float4*>(src)[lane];
    }
    asm volatile("" ::: "memory");     // compile-time fence: keep the requests below behind the ones above
    __builtin_amdgcn_sched_barrier(0); // (and the instruction scheduler)
    const int kw0 = wave * KPW;
    const half_t* wp = Wp + ((long)(h * 4) * KT + kw0) * 512 + lane * 8;
    f16x8 wf[KPW][4];
#pragma unroll
    for (int j = 0; j < KPW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) wf[j][i] = ld_nt_f16x8(wp + (long)i * KT * 512 + j * 512);
    constexpr float invK = 1.0f / (256.0f * LNV);
    auto ln_row = [&](float4 (&x)[LNV], int r, bool keep) {           // LayerNorm: wave w normalises rows w, w + 6, ... of the group
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < LNV; ++j) sm += (x[j].x + x[j].y) + (x[j].z + x[j].w);
        const float mean = dpp_wave_sum(sm) * invK;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < LNV; ++j) {
            x[j].x -= mean; x[j].y -= mean; x[j].z -= mean; x[j].w -= mean;
            q += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
        }
        const float rstd = rsqrtf(dpp_wave_sum(q) * invK + 1e-5f);
        half_t* dst = xs + r * ldxs + lane * 4;
#pragma unroll
        for (int j = 0; j < LNV; ++j) {
            const f16x4 hv = {(half_t)(x[j].x * rstd * gq[j].x + bq[j].x), (half_t)(x[j].y * rstd * gq[j].y + bq[j].y),
                              (half_t)(x[j].z * rstd * gq[j].z + bq[j].z), (half_t)(x[j].w * rstd * gq[j].w + bq[j].w)};
            if (keep) *reinterpret_cast<f16x4*>(dst + 256 * j) = hv;
        }
    };
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    {   // the exchange: waits for this wave's first four loads, sixteen more in flight
        float4* gbs4 = reinterpret_cast<float4*>(qs + 16 * 72);       // [2 LNV][64] float4 behind the query tile
        gbs4[wave * 64 + lane] = gbp;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LNV; ++j) { gq[j] = gbs4[j * 64 + lane]; bq[j] = gbs4[(LNV + j) * 64 + lane]; }
    }
    // first trip: straight-line and UNCONDITIONAL (a wave without a row normalises the clamped row it loaded and
    // keeps nothing): inside an `if (wave < nrow)` hipcc sinks the row loads into the branch, behind the weights.
    // (The row passes through opaque values: hipcc otherwise lifts the row sums, and the wait for the row, in front of the weight requests.)
#pragma unroll
    for (int j = 0; j < LNV; ++j) asm volatile("" : "+v"(x0[j].x), "+v"(x0[j].y), "+v"(x0[j].z), "+v"(x0[j].w));
    ln_row(x0, (wave < nrow) ? wave : nrow - 1, wave < nrow);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // the K / V addresses are the first use of the group's item and of the argument tail (compile-time fence and sched_barrier; the item passes
    // through an opaque value HERE: its address arithmetic, and the scalar wait with it, is otherwise lifted in front of the weights)
    int item = item_rq, hq = h;        // (the head too: the bias address, which needs the argument tail, is made of it)
    asm volatile("" : "+s"(item), "+s"(hq));
    const int tile = sp * TPS + wave;
    const int key0 = tile * 32;
    const long toff = (long)item * item_stride + ((long)h * (WLX_T_AUDIO_PAD / 32) + tile) * 2048 + lane * 8;
    f16x8 kf[2][2], vf[4];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) kf[s2][kt] = ld_f16x8(Kp + toff + (s2 * 2 + kt) * 512);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vf[dt] = ld_f16x8(Vp + toff + dt * 512);
    const float4 bq4 = *reinterpret_cast<const float4*>(bias + hq * 64 + (wave & 3) * 16 + g * 4);
#pragma unroll 1
    for (int r = wave + TPS; r < nrow; r += TPS) {                          // groups of more than six rows (prefill)
        const float4* x4 = reinterpret_cast<const float4*>(X + (long)(grp * R + r) * ldx) + lane;
        float4 x[LNV];
#pragma unroll
        for (int j = 0; j < LNV; ++j) x[j] = x4[64 * j];
        ln_row(x, r, true);
    }
    WLX_TR_MARK(1);
    __syncthreads();
    // ---- the head's query columns: this wave's K slice of all 4 n-tiles
    const int crow = (c < nrow) ? c : nrow - 1;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const half_t* xr = xs + crow * ldxs + kw0 * 32 + g * 8;
#pragma unroll
        for (int j = 0; j < KPW; ++j) {
            const f16x8 xf = *reinterpret_cast<const f16x8*>(xr + j * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = mfma16(wf[j][i], xf, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(accred + ((wave * 4 + i) * 64 + lane) * 4) = acc[i];
    __syncthreads();
    if (wave < 4) {      // wave i finishes n-tile i: fixed-order sum over the six K slices, bias, q scale -> fp16 query tile
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < TPS; ++w) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(accred + ((w * 4 + wave) * 64 + lane) * 4);
            v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
        }
        const f16x4 hv = {(half_t)((v[0] + bq4.x) * qscale), (half_t)((v[1] + bq4.y) * qscale),
                          (half_t)((v[2] + bq4.z) * qscale), (half_t)((v[3] + bq4.w) * qscale)};
        *reinterpret_cast<f16x4*>(qs + c * 72 + wave * 16 + g * 4) = hv;     // query row c, head dims wave*16 + g*4 ..
    }
    WLX_TR_MARK(2);
    __syncthreads();                                                        // qs complete; accred dead (Os aliases it)
    f16x8 qf[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) qf[kt] = *reinterpret_cast<const f16x8*>(qs + c * 72 + kt * 32 + g * 8);

    // ---- attention over this wave's tile: identical to dec_cross_attn_kernel from here on
    constexpr int T = WLX_T_AUDIO;
    f32x4 st[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) st[s2] = mfma16(kf[s2][kt], qf[kt], st[s2]);
    }
    float pv[8];
    float tmax = WLX_NEG_INF;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = key0 + s2 * 16 + g * 4 + r;
            const float v = (key < T) ? st[s2][r] : WLX_NEG_INF;
            pv[s2 * 4 + r] = v;
            tmax = fmaxf(tmax, v);
        }
    // (max / sum over the four 16-lane rows by v_permlane16/32_swap, round 6: the ds_bpermute form cost four dependent LDS round trips in the tail
    // of the launch; same values — max is exact, the sum's additions commute)
    tmax = rows4_max(tmax);
    const float msafe = (tmax == WLX_NEG_INF) ? 0.f : tmax;
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { pv[i] = __expf(pv[i] - msafe); psum += pv[i]; }
    psum = rows4_sum(psum);
    const f16x8 pf = {(half_t)pv[0], (half_t)pv[1], (half_t)pv[2], (half_t)pv[3],
                      (half_t)pv[4], (half_t)pv[5], (half_t)pv[6], (half_t)pv[7]};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const f32x4 a = mfma16(vf[dt], pf, (f32x4){0.f, 0.f, 0.f, 0.f});
        *reinterpret_cast<f32x4*>(&Os[wave][c][dt * 16 + g * 4]) = a;
    }
    if (g == 0) { MLs[(wave * 16 + c) * 2] = tmax; MLs[(wave * 16 + c) * 2 + 1] = psum; }
    __syncthreads();
    if (wave < 4) {
        const int dt = wave;
        float mw[TPS], lw[TPS];
        float M = WLX_NEG_INF;
#pragma unroll
        for (int w = 0; w < TPS; ++w) { mw[w] = MLs[(w * 16 + c) * 2]; lw[w] = MLs[(w * 16 + c) * 2 + 1]; M = fmaxf(M, mw[w]); }
        float l = 0.f;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < TPS; ++w) {
            const float e = (mw[w] == WLX_NEG_INF) ? 0.f : __expf(mw[w] - M);
            l += e * lw[w];
            const f32x4 t = *reinterpret_cast<const f32x4*>(&Os[w][c][dt * 16 + g * 4]);
            o[0] += e * t[0]; o[1] += e * t[1]; o[2] += e * t[2]; o[3] += e * t[3];
        }
        const long ih = (long)grp * H + h;
        const float inv = 1.0f / l;
        const f16x4 hv = {(half_t)(o[0] * inv), (half_t)(o[1] * inv), (half_t)(o[2] * inv), (half_t)(o[3] * inv)};
        *reinterpret_cast<f16x4*>(part_o + ((ih * WLX_XSPLIT + sp) * 16 + c) * 64 + dt * 16 + g * 4) = hv;
        if (dt == 0 && g == 0) *reinterpret_cast<float2*>(part_ml + (ih * 16 + c) * (WLX_XSPLIT * 2) + sp * 2) = make_float2(M, l);
    }
    WLX_TR_MARK(3);
    WLX_TR_END(trc);
}

// dynamic LDS of a workgroup: the fp16 LayerNorm rows, the region the K-reduction partials and the merge buffers share, the query tile, [gamma | beta]
static size_t cq_cross_attn_shm(int d, int R) {
    const size_t xs_floats = (size_t)((R * (d + 8) * 2 + 15) / 16) * 4;
    return sizeof(float) * (xs_floats + (size_t)XA_TPS * 16 * 68 + XA_TPS * 16 * 2) + 16 * 72 * sizeof(half_t) + 6 * 1024;
}
// eligibility: d_model 768 (LNV = 3, KT = 24 = 6 waves x 4 k-tiles), groups of <= 16 rows
bool dec_cq_cross_attn_eligible(int d, int H, int R) {
    if (g_decode_v1 || d != 768 || H * 64 != d || R < 1 || R > 16) return false;
    return cq_cross_attn_shm(d, R) <= 64 * 1024;
}
void launch_dec_cq_cross_attn(const float* X, long ldx, const float* gamma, const float* beta, const half_t* Wp, const float* bias,
                              float qscale, int d, const half_t* Kp, const half_t* Vp, long item_stride, int H, int R, int groups,
                              int rows, const int* group_item, half_t* part_o, float* part_ml, hipStream_t s) {
    // d_model 768 and 12 heads (dec_cq_cross_attn_eligible) are template constants of the one instantiation; grid.y walks the groups
    hipLaunchKernelGGL((dec_cq_cross_attn_kernel<3, 4>), dim3(H * WLX_XSPLIT, groups), dim3(XA_TPS * 64), cq_cross_attn_shm(d, R), s, X, ldx, gamma, beta,
                       Wp, group_item, R, rows, Kp, Vp, item_stride, bias, qscale, part_o, part_ml WLX_TR_ARG("cq_cross_attn"));
}

// ------------------------------------------------------------------ split combine of the cross attention, on its own
// For batched rows (> 16) the fused form — every workgroup of the output projection combining ALL rows' eight split
// partials in its prologue — costs 12 us of a 14.6 us launch at 40 rows x 20 heads (80 workgroups each looping 13 times
// over 6400 (row, head, 8-dim) items; profiles/r2s decode-step timeline). Here one thread per item does it once, the
// result goes to the fp16 attention rows and the projection runs as a plain fp16-rows-in launch. (Up to 16 rows the fused
// form stays: one trip, no extra launch.)
__global__ __launch_bounds__(256) void dec_xattn_combine_kernel(const half_t* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                int M, int H, int R, half_t* __restrict__ out, long ldo WLX_TR_PARAM) {
    WLX_TR_BEGIN();
    const int it0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = it0 < M * H * 8;
    const int it = live ? it0 : M * H * 8 - 1;              // (clamped: every thread runs the same code; only live ones store)
    const int q8 = it & 7, hm = it >> 3;
    const int m = hm / H, hh = hm - m * H;
    const int item = m / R, qi = m - item * R;
    const long ih = (long)item * H + hh;
    const float4* mlp = reinterpret_cast<const float4*>(part_ml + (ih * 16 + qi) * (WLX_XSPLIT * 2));
    const half_t* op = part_o + (ih * WLX_XSPLIT * 16 + qi) * 64 + q8 * 8;
    float4 ml[WLX_XSPLIT / 2];
    f16x8 ov[WLX_XSPLIT];
#pragma unroll
    for (int sp = 0; sp < WLX_XSPLIT / 2; ++sp) ml[sp] = mlp[sp];
#pragma unroll
    for (int sp = 0; sp < WLX_XSPLIT; ++sp) ov[sp] = ld_f16x8(op + sp * 1024);
    float mmax = fmaxf(ml[0].x, ml[0].z);
#pragma unroll
    for (int sp = 1; sp < WLX_XSPLIT / 2; ++sp) mmax = fmaxf(mmax, fmaxf(ml[sp].x, ml[sp].z));
    float den = 0.f;
    float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sp = 0; sp < WLX_XSPLIT; ++sp) {        // (the arithmetic and its order are the fused combine's: identical rows)
        const float mm = (sp & 1) ? ml[sp >> 1].z : ml[sp >> 1].x, ll = (sp & 1) ? ml[sp >> 1].w : ml[sp >> 1].y;
        const float w = __expf(mm - mmax) * ll;
        den += w;
#pragma unroll
        for (int e = 0; e < 8; ++e) num[e] += w * (float)ov[sp][e];
    }
    const float inv = 1.0f / den;
    const f16x8 hv = {(half_t)(num[0] * inv), (half_t)(num[1] * inv), (half_t)(num[2] * inv), (half_t)(num[3] * inv),
                      (half_t)(num[4] * inv), (half_t)(num[5] * inv), (half_t)(num[6] * inv), (half_t)(num[7] * inv)};
    if (live) *reinterpret_cast<f16x8*>(out + (long)m * ldo + hh * 64 + q8 * 8) = hv;
    WLX_TR_END(trc);
}
void launch_dec_xattn_combine(const half_t* part_o, const float* part_ml, int M, int H, int R, half_t* out, long ldo, hipStream_t s) {
    hipLaunchKernelGGL(dec_xattn_combine_kernel, dim3((M * H * 8 + 255) / 256), dim3(256), 0, s, part_o, part_ml, M, H, R, out, ldo WLX_TR_ARG("xattn_combine"));
}

// ------------------------------------------------------------------ cross-attention scores of one head, for word alignment
// (ctranslate2 Whisper.align, called from transcriber_faster_whisper.py:1657: the QK of the alignment heads over a
// teacher-forced pass). Raw scores q.k (q already carries head_dim^-0.5) of `rows` query rows against the 1536 padded
// keys of one (item, head), written as fp32 [rows][1536]; the softmax over the first num_frames/2 keys, the
// normalisation, median filter and DTW run on the host side of wlx_align (they are O(tokens x 1500) scalar work).
// grid (WLX_XSPLIT key splits, row tiles of 16); XA_TPS waves per workgroup, one tile-packed 32-key tile each.
__global__ __launch_bounds__(XA_TPS * 64) void dec_align_scores_kernel(const half_t* __restrict__ q, long ldq,
                                                                       const half_t* __restrict__ Kp, int h, int rows,
                                                                       float* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = tid >> 6;
    const int tile = blockIdx.x * XA_TPS + wave;
    const int row0 = blockIdx.y * 16;
    const long toff = ((long)h * (WLX_T_AUDIO_PAD / 32) + tile) * 2048 + lane * 8;
    f16x8 kf[2][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) kf[s2][kt] = ld_f16x8(Kp + toff + (s2 * 2 + kt) * 512);
    int row = row0 + c;
    const bool ok = row < rows;
    if (!ok) row = rows - 1;
    f16x8 qf[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) qf[kt] = ld_f16x8(q + (long)row * ldq + h * WLX_HEAD_DIM + kt * 32 + g * 8);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) st = mfma16(kf[s2][kt], qf[kt], st);
        // st[r] = score of key tile*32 + s2*16 + g*4 + r for query row c
        if (ok) *reinterpret_cast<f32x4*>(out + (long)row * WLX_T_AUDIO_PAD + tile * 32 + s2 * 16 + g * 4) = st;
    }
}

void launch_dec_align_scores(const half_t* q, long ldq, const half_t* Kp_item, int h, int rows, float* out, hipStream_t s) {
    hipLaunchKernelGGL(dec_align_scores_kernel, dim3(WLX_XSPLIT, (rows + 15) / 16), dim3(XA_TPS * 64), 0, s, q, ldq, Kp_item, h, rows, out);
}

void launch_dec_cross_attn(const half_t* q, long ldq, const half_t* Kp, const half_t* Vp, long item_stride, int H, int R,
                           int groups, int rows, const int* group_item, half_t* part_o, float* part_ml, hipStream_t s) {
    hipLaunchKernelGGL(dec_cross_attn_kernel, dim3(WLX_XSPLIT, H, groups), dim3(XA_TPS * 64), 0, s, q, ldq, Kp, Vp, item_stride,
                       H, R, rows, group_item, part_o, part_ml WLX_TR_ARG("cross_attn"));
}

}  // namespace wlx
