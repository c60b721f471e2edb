// spk.hip — kernels of the speaker-embedding engine (spk.h): Kaldi filterbank, the ResNet convolutions, statistics pooling and
// the embedding head of WeSpeaker ResNet34. Every reduction runs in a fixed order: two embeds of the same audio are bit-identical.
// ONE launcher family: every launch takes a ragged batch of 1..WLX_SPK_MAX_BATCH items, and a single embed is a batch of one. For
// n == 1 the filterbank, mean-removal and convolution launchers pick a kernel without the by-value table around the same body: the
// table's cost per launch was measured outside the run-to-run spread there (profiles/single_as_batch_of_one.txt).
#include "spk.h"

namespace wlx {

// ------------------------------------------------------------------------------------------------ ragged batch
// N items of different lengths in one pass, packed without padding: at a stage of geometry (H, C) item i is its own [H][W_i][C]
// image at pixel offset H * sum_{j<i} W_j. Every kernel below finds its item, moves the base pointers there and runs the
// per-item body (*_body / *_tile / *_quad) with the item's own W / OW / T, so a tap outside the item's image is padding (zero),
// never a neighbour's pixel, and every reduction keeps its per-item order: an item's bits do not depend on its neighbours, its
// position or the table's fill. The table of widths, column offsets and first workgroups travels BY VALUE in the kernel arguments
// (1 KiB, copied by the launch call itself): no staging buffer and no copy that could outlive the launcher's frame.
struct SpkItem {
    int W;           // columns of the item at the launch's input (frames, for the front end and the pooling)
    int in0, out0;   // sum of the earlier items' columns at the input and at the output
    int blk0;        // first workgroup (blockIdx.x) of the item, where the grid's x runs over all items
};
struct SpkBatch {
    int n;
    SpkItem it[WLX_SPK_MAX_BATCH];
};
struct SpkOffsets {
    long off[WLX_SPK_MAX_BATCH];
};

// the item that owns workgroup `blk`: the last one with blk0 <= blk (blk0 is strictly increasing: every item has work)
__device__ __forceinline__ int spk_item_of(const SpkBatch& tab, int blk) {
    int lo = 0, hi = tab.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.it[mid].blk0 <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Host side: items of `widths` columns, `units_per_col` work units per OUTPUT column, `per_blk` units per workgroup. False when a
// width is < 1, an item alone exceeds `unit_cap` units or the grid exceeds 2^31 - 1 workgroups.
static bool spk_table(const int* widths, int n, int stride, long units_per_col, int per_blk, long unit_cap, SpkBatch& tab, long& blocks) {
    if (!widths || n < 1 || n > WLX_SPK_MAX_BATCH) return false;
    long in0 = 0, out0 = 0;
    blocks = 0;
    tab.n = n;
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 1) return false;
        const long ow = (widths[i] - 1) / stride + 1, units = ow * units_per_col;
        if (units > unit_cap || in0 > 0x7fffffffL || out0 > 0x7fffffffL || blocks > 0x7fffffffL) return false;
        tab.it[i] = SpkItem{widths[i], (int)in0, (int)out0, (int)blocks};
        in0 += widths[i], out0 += ow, blocks += (units + per_blk - 1) / per_blk;
    }
    for (int i = n; i < WLX_SPK_MAX_BATCH; ++i) tab.it[i] = SpkItem{0, 0, 0, 0};
    return blocks <= 0x7fffffffL;
}

// ------------------------------------------------------------------------------------------------ filterbank
// One workgroup per frame. The DFT is direct (400 x 256 multiply-adds per frame, fp32, four partial sums per bin): at 100 frames
// per second it is noise beside the network, and its twiddles are table entries rounded from float64, exact in their index
// (k n mod 512), so the only fp32 error is the accumulation.
// `src`: the frame's 400 samples, `dst`: its n_mels outputs.
__device__ __forceinline__ void spk_fbank_body(const float* __restrict__ src, const float* __restrict__ window,
                                               const float* __restrict__ twiddle, const float* __restrict__ mel, int n_mels,
                                               float* __restrict__ dst) {
    __shared__ float x[WLX_SPK_FRAME];
    __shared__ float tw[WLX_SPK_NFFT];
    __shared__ float pw[WLX_SPK_BINS];
    __shared__ float part[4];
    const int tid = threadIdx.x;
    float a = src[tid] * 32768.f, b = 0.f;
    if (tid + 256 < WLX_SPK_FRAME) b = src[tid + 256] * 32768.f;
    tw[tid] = twiddle[tid];
    tw[tid + 256] = twiddle[tid + 256];
    const float ws = wave_sum(a + b);
    if ((tid & 63) == 0) part[tid >> 6] = ws;
    __syncthreads();
    const float mean = (((part[0] + part[1]) + part[2]) + part[3]) * (1.f / WLX_SPK_FRAME);
    x[tid] = a - mean;
    if (tid + 256 < WLX_SPK_FRAME) x[tid + 256] = b - mean;
    __syncthreads();
    // pre-emphasis against the previous sample (the first against itself), then the window
    const float z0 = (x[tid] - 0.97f * x[tid > 0 ? tid - 1 : 0]) * window[tid];
    float z1 = 0.f;
    if (tid + 256 < WLX_SPK_FRAME) z1 = (x[tid + 256] - 0.97f * x[tid + 255]) * window[tid + 256];
    __syncthreads();
    x[tid] = z0;
    if (tid + 256 < WLX_SPK_FRAME) x[tid + 256] = z1;
    __syncthreads();
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < WLX_SPK_FRAME; n += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (tid * (n + j)) & (WLX_SPK_NFFT - 1);
            const float v = x[n + j];
            re[j] += v * tw[idx];
            im[j] += v * tw[(idx - WLX_SPK_NFFT / 4) & (WLX_SPK_NFFT - 1)];
        }
    }
    const float r = (re[0] + re[1]) + (re[2] + re[3]), i = (im[0] + im[1]) + (im[2] + im[3]);
    pw[tid] = r * r + i * i;
    __syncthreads();
    if (tid < n_mels) {
        const float* m = mel + (long)tid * WLX_SPK_BINS;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < WLX_SPK_BINS; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] += m[k + j] * pw[k + j];
        }
        const float s = (e[0] + e[1]) + (e[2] + e[3]);
        dst[tid] = logf(fmaxf(s, 1.1920928955078125e-07f));
    }
}

// one item without the tables, selected by the launcher on n == 1 (as spk_conv_kernel below: the 1.5 KiB of arguments measured 0.8 us
// on the 24 us front end of a 1 s embed, outside the run-to-run spread)
__global__ __launch_bounds__(256) void spk_fbank_kernel(const float* __restrict__ pcm, const float* __restrict__ window,
                                                         const float* __restrict__ twiddle, const float* __restrict__ mel, int n_mels,
                                                         float* __restrict__ logmel) {
    const long t = blockIdx.x;
    spk_fbank_body(pcm + t * WLX_SPK_SHIFT, window, twiddle, mel, n_mels, logmel + t * n_mels);
}

__global__ __launch_bounds__(256) void spk_fbank_batch_kernel(const float* __restrict__ pcm, SpkOffsets offs, SpkBatch tab,
                                                               const float* __restrict__ window, const float* __restrict__ twiddle,
                                                               const float* __restrict__ mel, int n_mels, float* __restrict__ logmel) {
    const int i = spk_item_of(tab, (int)blockIdx.x);
    const long t = (int)blockIdx.x - tab.it[i].blk0;
    spk_fbank_body(pcm + offs.off[i] + t * WLX_SPK_SHIFT, window, twiddle, mel, n_mels, logmel + (long)blockIdx.x * n_mels);
}

bool launch_spk_fbank_batch(const float* pcm, const long* offsets, const int* frames, int n, const float* window, const float* twiddle,
                            const float* mel, int n_mels, float* logmel, hipStream_t s) {
    SpkBatch tab;
    long blocks;
    if (!pcm || !offsets || !logmel || !spk_table(frames, n, 1, 1, 1, 1L << 30, tab, blocks)) return false;
    for (int i = 0; i < n; ++i)
        if (offsets[i] < 0) return false;
    if (n == 1) {
        hipLaunchKernelGGL(spk_fbank_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pcm + offsets[0], window, twiddle, mel, n_mels, logmel);
        return true;
    }
    SpkOffsets offs;
    for (int i = 0; i < WLX_SPK_MAX_BATCH; ++i) offs.off[i] = i < n ? offsets[i] : 0;
    hipLaunchKernelGGL(spk_fbank_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pcm, offs, tab, window, twiddle, mel, n_mels, logmel);
    return true;
}

__device__ __forceinline__ void spk_cmn_body(float* __restrict__ logmel, int T, int n_mels, half_t* __restrict__ out16, int b) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int t = tid; t < T; t += 256) acc += logmel[(long)t * n_mels + b];
    const float ws = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = ws;
    __syncthreads();
    const float mean = (((part[0] + part[1]) + part[2]) + part[3]) / (float)T;
    for (int t = tid; t < T; t += 256) {
        const float v = logmel[(long)t * n_mels + b] - mean;
        logmel[(long)t * n_mels + b] = v;
        out16[(long)b * T + t] = (half_t)v;
    }
}

__global__ __launch_bounds__(256) void spk_cmn_kernel(float* __restrict__ logmel, int T, int n_mels, half_t* __restrict__ out16) {
    spk_cmn_body(logmel, T, n_mels, out16, (int)blockIdx.x);          // one item without the table (n == 1, as spk_fbank_kernel)
}

__global__ __launch_bounds__(256) void spk_cmn_batch_kernel(float* __restrict__ logmel, SpkBatch tab, int n_mels,
                                                             half_t* __restrict__ out16) {
    const SpkItem it = tab.it[blockIdx.y];
    spk_cmn_body(logmel + (long)it.in0 * n_mels, it.W, n_mels, out16 + (long)it.in0 * n_mels, (int)blockIdx.x);
}

bool launch_spk_cmn_batch(float* logmel, const int* frames, int n, int n_mels, half_t* out16, hipStream_t s) {
    SpkBatch tab;
    long blocks;
    if (!logmel || !out16 || !spk_table(frames, n, 1, 1, 1, 1L << 30, tab, blocks)) return false;
    if (n == 1) {
        hipLaunchKernelGGL(spk_cmn_kernel, dim3((unsigned)n_mels), dim3(256), 0, s, logmel, frames[0], n_mels, out16);
        return true;
    }
    hipLaunchKernelGGL(spk_cmn_batch_kernel, dim3((unsigned)n_mels, (unsigned)n), dim3(256), 0, s, logmel, tab, n_mels, out16);
    return true;
}

// ------------------------------------------------------------------------------------------------ convolution
// Implicit GEMM in the swapped form of common.h: D[n = output channel][m = output pixel] = sum_k W[n][k] X[m][k] with
// k = tap * Cin + ci. NHWC makes the 8 halfs a lane feeds per MFMA (k = g * 8 .. g * 8 + 7 of a 32-wide k-tile) contiguous in
// memory for every tap, so the activation fragment is one 16-byte load from the input image, zero where the tap falls into the
// padding; no im2col buffer and no LDS. A wave owns 16 pixels x NT * 16 output channels, a workgroup four waves = 64 pixels.
// Each lane ends with 4 consecutive channels of one pixel: one 8-byte store.
// `tile`: the 64-pixel tile of this image the workgroup owns, `nt0`: its first 16-channel tile.
template <int NT>
__device__ __forceinline__ void spk_conv_tile(const half_t* __restrict__ in, const half_t* __restrict__ Wp,
                                              const float* __restrict__ bias, const half_t* __restrict__ resid,
                                              half_t* __restrict__ out, int H, int W, int Cin, int OH, int OW, int Cout, int stride,
                                              int ks, int relu, long tile, int nt0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const long P = (long)OH * OW;
    const long m0 = (tile * 4 + wave) * 16;
    if (m0 >= P) return;                       // wave-uniform: the MFMAs below always run with all 64 lanes
    const long m = m0 + c;
    const bool live = m < P;
    const int oh = live ? (int)(m / OW) : 0, ow = live ? (int)(m % OW) : 0;
    const int cpt = Cin >> 5, KT = ks * ks * cpt, pad = ks >> 1;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const half_t* wbase = Wp + ((long)nt0 * KT * 64 + lane) * 8;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    int kt = 0;
    for (int kh = 0; kh < ks; ++kh) {
        for (int kw = 0; kw < ks; ++kw) {
            const int ih = oh * stride + kh - pad, iw = ow * stride + kw - pad;
            const bool ok = live && ih >= 0 && ih < H && iw >= 0 && iw < W;
            const half_t* src = in + ((long)(ok ? ih : 0) * W + (ok ? iw : 0)) * Cin + g * 8;
            for (int q = 0; q < cpt; ++q, ++kt) {
                const f16x8 b = ok ? ld_f16x8(src + q * 32) : zero;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const f16x8 a = ld_f16x8(wbase + ((long)j * KT + kt) * 512);
                    acc[j] = mfma16(a, b, acc[j]);
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = (nt0 + j) * 16 + g * 4;
        const float4 bv = *reinterpret_cast<const float4*>(bias + n);
        float v[4] = {acc[j][0] + bv.x, acc[j][1] + bv.y, acc[j][2] + bv.z, acc[j][3] + bv.w};
        if (resid) {
            const f16x4 rv = ld_f16x4(resid + m * Cout + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
        }
        f16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (half_t)(relu ? fmaxf(v[r], 0.f) : v[r]);
        *reinterpret_cast<f16x4*>(out + m * Cout + n) = o;
    }
}

// One item without the table: a 1 KiB by-value table on each of the 35 convolution launches of an
// embed measured 11 - 13 us of device time per embed (1.5 %, ten times the run-to-run spread) over this form; launch_spk_conv_batch
// selects it on n == 1. Same tile function, same bits.
template <int NT>
__global__ __launch_bounds__(256) void spk_conv_kernel(const half_t* __restrict__ in, const half_t* __restrict__ Wp,
                                                        const float* __restrict__ bias, const half_t* __restrict__ resid,
                                                        half_t* __restrict__ out, int H, int W, int Cin, int OH, int OW, int Cout,
                                                        int stride, int ks, int relu) {
    spk_conv_tile<NT>(in, Wp, bias, resid, out, H, W, Cin, OH, OW, Cout, stride, ks, relu, (long)blockIdx.x, (int)blockIdx.y * NT);
}

template <int NT>
__global__ __launch_bounds__(256) void spk_conv_batch_kernel(const half_t* __restrict__ in, const half_t* __restrict__ Wp,
                                                              const float* __restrict__ bias, const half_t* __restrict__ resid,
                                                              half_t* __restrict__ out, SpkBatch tab, int H, int Cin, int OH, int Cout,
                                                              int stride, int ks, int relu) {
    const SpkItem it = tab.it[spk_item_of(tab, (int)blockIdx.x)];          // workgroup-uniform: the item of all four waves
    const int OW = (it.W - 1) / stride + 1;
    const long o0 = (long)OH * it.out0 * Cout;
    spk_conv_tile<NT>(in + (long)H * it.in0 * Cin, Wp, bias, resid ? resid + o0 : nullptr, out + o0, H, it.W, Cin, OH, OW, Cout, stride,
                      ks, relu, (long)((int)blockIdx.x - it.blk0), (int)blockIdx.y * NT);
}

bool launch_spk_conv_batch(const half_t* in, int H, const int* widths, int n, int Cin, const half_t* Wp, const float* bias,
                           const half_t* resid, int Cout, int stride, int ks, bool relu, half_t* out, hipStream_t s) {
    if (!in || !Wp || !bias || !out) return false;
    if (H < 1 || Cin < 32 || Cin % 32 || Cout < 32 || Cout % 32 || (stride != 1 && stride != 2) || (ks != 1 && ks != 3)) return false;
    const int OH = (H - 1) / stride + 1;
    SpkBatch tab;
    long blocks;
    if (!spk_table(widths, n, stride, OH, 64, 1L << 30, tab, blocks)) return false;
    const int r = relu ? 1 : 0;
    if (n == 1) {
        const int W = widths[0], OW = (W - 1) / stride + 1;
        if (Cout % 64 == 0)
            hipLaunchKernelGGL(spk_conv_kernel<4>, dim3((unsigned)blocks, (unsigned)(Cout / 64)), dim3(256), 0, s, in, Wp, bias, resid, out, H,
                               W, Cin, OH, OW, Cout, stride, ks, r);
        else
            hipLaunchKernelGGL(spk_conv_kernel<2>, dim3((unsigned)blocks, (unsigned)(Cout / 32)), dim3(256), 0, s, in, Wp, bias, resid, out, H,
                               W, Cin, OH, OW, Cout, stride, ks, r);
        return true;
    }
    if (Cout % 64 == 0)
        hipLaunchKernelGGL(spk_conv_batch_kernel<4>, dim3((unsigned)blocks, (unsigned)(Cout / 64)), dim3(256), 0, s, in, Wp, bias, resid, out,
                           tab, H, Cin, OH, Cout, stride, ks, r);
    else
        hipLaunchKernelGGL(spk_conv_batch_kernel<2>, dim3((unsigned)blocks, (unsigned)(Cout / 32)), dim3(256), 0, s, in, Wp, bias, resid, out,
                           tab, H, Cin, OH, Cout, stride, ks, r);
    return true;
}

void spk_pack_conv(const float* w, int Cout, int Cin, int ks, half_t* Wp) {
    const int cpt = Cin / 32, KT = ks * ks * cpt;
    for (int nt = 0; nt < Cout / 16; ++nt)
        for (int kt = 0; kt < KT; ++kt) {
            const int tap = kt / cpt, kh = tap / ks, kw = tap % ks;
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int n = nt * 16 + (l & 15), ci = (kt % cpt) * 32 + (l >> 4) * 8 + e;
                    Wp[(((size_t)nt * KT + kt) * 64 + l) * 8 + e] = (half_t)w[(((size_t)n * Cin + ci) * ks + kh) * ks + kw];
                }
        }
}

// The stem (Cin = 1, K = 9): a thread computes 4 output channels of one pixel on the vector ALU.
// `i`: the (pixel, channel quad) of this image the thread computes.
__device__ __forceinline__ void spk_conv_c1_quad(const half_t* __restrict__ in, const float* __restrict__ w,
                                                 const float* __restrict__ bias, const half_t* __restrict__ resid,
                                                 half_t* __restrict__ out, int H, int W, int OH, int OW, int Cout, int stride, int relu,
                                                 long i) {
    const int q = Cout >> 2;
    if (i >= (long)OH * OW * q) return;
    const long m = i / q;
    const int n = (int)(i % q) * 4;
    const int oh = (int)(m / OW), ow = (int)(m % OW);
    float v[4] = {bias[n], bias[n + 1], bias[n + 2], bias[n + 3]};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ih = oh * stride + kh - 1, iw = ow * stride + kw - 1;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            const float x = (float)in[(long)ih * W + iw];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += x * w[(n + r) * 9 + kh * 3 + kw];
        }
    if (resid) {
        const f16x4 rv = ld_f16x4(resid + m * Cout + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
    }
    f16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (half_t)(relu ? fmaxf(v[r], 0.f) : v[r]);
    *reinterpret_cast<f16x4*>(out + m * Cout + n) = o;
}

__global__ __launch_bounds__(256) void spk_conv_c1_batch_kernel(const half_t* __restrict__ in, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const half_t* __restrict__ resid,
                                                                 half_t* __restrict__ out, SpkBatch tab, int H, int OH, int Cout,
                                                                 int stride, int relu) {
    const SpkItem it = tab.it[spk_item_of(tab, (int)blockIdx.x)];
    const int OW = (it.W - 1) / stride + 1;
    const long o0 = (long)OH * it.out0 * Cout;
    spk_conv_c1_quad(in + (long)H * it.in0, w, bias, resid ? resid + o0 : nullptr, out + o0, H, it.W, OH, OW, Cout, stride, relu,
                     (long)((int)blockIdx.x - it.blk0) * 256 + threadIdx.x);
}

bool launch_spk_conv_c1_batch(const half_t* in, int H, const int* widths, int n, const float* w, const float* bias, const half_t* resid,
                              int Cout, int stride, bool relu, half_t* out, hipStream_t s) {
    if (!in || !w || !bias || !out) return false;
    if (H < 1 || Cout < 4 || Cout % 4 || (stride != 1 && stride != 2)) return false;
    const int OH = (H - 1) / stride + 1;
    SpkBatch tab;
    long blocks;
    if (!spk_table(widths, n, stride, (long)OH * (Cout / 4), 256, 1L << 38, tab, blocks)) return false;
    hipLaunchKernelGGL(spk_conv_c1_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, w, bias, resid, out, tab, H, OH, Cout, stride,
                       relu ? 1 : 0);
    return true;
}

// ------------------------------------------------------------------------------------------------ pooling and head
// A workgroup owns 64 channels of one frequency row; its four waves take the frames t = wave, wave + 4, ... Two passes (mean, then
// squared deviations) in fp32.
__device__ __forceinline__ void spk_pool_body(const half_t* __restrict__ x, int F, int T, int C, float eps, float* __restrict__ out,
                                              int f, int c0) {
    __shared__ float part[4][64];
    const int ch = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = c0 + ch;
    const half_t* p = x + (long)f * T * C + c;
    float acc = 0.f;
    for (int t = sl; t < T; t += 4) acc += (float)p[(long)t * C];
    part[sl][ch] = acc;
    __syncthreads();
    const float mean = (((part[0][ch] + part[1][ch]) + part[2][ch]) + part[3][ch]) / (float)T;
    __syncthreads();
    acc = 0.f;
    for (int t = sl; t < T; t += 4) {
        const float d = (float)p[(long)t * C] - mean;
        acc += d * d;
    }
    part[sl][ch] = acc;
    __syncthreads();
    if (sl == 0) {
        const float var = (((part[0][ch] + part[1][ch]) + part[2][ch]) + part[3][ch]) / (float)(T - 1);
        out[(long)c * F + f] = mean;
        out[(long)C * F + (long)c * F + f] = sqrtf(var + eps);
    }
}

__global__ __launch_bounds__(256) void spk_pool_batch_kernel(const half_t* __restrict__ x, SpkBatch tab, int F, int C, float eps,
                                                              float* __restrict__ out) {
    const SpkItem it = tab.it[blockIdx.z];
    spk_pool_body(x + (long)F * it.in0 * C, F, it.W, C, eps, out + (long)blockIdx.z * 2 * C * F, (int)blockIdx.x, (int)blockIdx.y * 64);
}

bool launch_spk_pool_batch(const half_t* x, int F, const int* frames, int n, int C, float eps, float* out, hipStream_t s) {
    if (!x || !out || F < 1 || C < 64 || C % 64) return false;
    SpkBatch tab;
    long blocks;
    if (!spk_table(frames, n, 1, 1, 1, 1L << 30, tab, blocks)) return false;
    for (int i = 0; i < n; ++i)
        if (frames[i] < 2) return false;
    hipLaunchKernelGGL(spk_pool_batch_kernel, dim3((unsigned)F, (unsigned)(C / 64), (unsigned)n), dim3(256), 0, s, x, tab, F, C, eps, out);
    return true;
}

__device__ __forceinline__ void spk_linear_body(const float* __restrict__ x, const half_t* __restrict__ W, const float* __restrict__ b,
                                                int D, float* __restrict__ y, int e) {
    const int lane = threadIdx.x;
    const half_t* w = W + (long)e * D;
    float acc = 0.f;
    for (int i = lane * 8; i < D; i += 512) {
        const f16x8 wv = ld_f16x8(w + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)wv[j] * x[i + j];
    }
    acc = wave_sum(acc);
    if (lane == 0) y[e] = acc + b[e];
}

__device__ __forceinline__ void spk_l2norm_body(float* __restrict__ y, int E) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int i = tid; i < E; i += 256) acc += y[i] * y[i];
    const float ws = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = ws;
    __syncthreads();
    // an all-zero head output stays zero instead of turning into NaN; every other row comes back with unit norm, however small it
    // was (a floor under the sum of squares would leave a row of norm < 1e-15 short of 1)
    const float ss = ((part[0] + part[1]) + part[2]) + part[3];
    const float inv = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
    for (int i = tid; i < E; i += 256) y[i] *= inv;
}

__global__ __launch_bounds__(64) void spk_linear_batch_kernel(const float* __restrict__ x, const half_t* __restrict__ W,
                                                               const float* __restrict__ b, int D, int E, float* __restrict__ y) {
    spk_linear_body(x + (long)blockIdx.y * D, W, b, D, y + (long)blockIdx.y * E, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void spk_l2norm_batch_kernel(float* __restrict__ y, int E) { spk_l2norm_body(y + (long)blockIdx.x * E, E); }

// false, before any launch: a null pointer, n < 1, E < 1, or a D the 8-wide loads of spk_linear_body cannot serve (D < 8, D % 8: the last
// load of a row would run past it). `normalize` false stops behind the linear layer (the one-launch hook of the head).
bool launch_spk_head_batch(const float* pooled, const half_t* W, const float* b, int E, int D, int n, float* emb, hipStream_t s, bool normalize) {
    if (!pooled || !W || !b || !emb || n < 1 || E < 1 || D < 8 || D % 8) return false;
    hipLaunchKernelGGL(spk_linear_batch_kernel, dim3((unsigned)E, (unsigned)n), dim3(64), 0, s, pooled, W, b, D, E, emb);
    if (normalize) hipLaunchKernelGGL(spk_l2norm_batch_kernel, dim3((unsigned)n), dim3(256), 0, s, emb, E);
    return true;
}

}  // namespace wlx
