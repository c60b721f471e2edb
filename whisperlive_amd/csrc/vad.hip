// vad.hip — Silero-VAD speech probabilities on gfx950: the network the reference
// reaches through faster_whisper.vad.get_speech_timestamps -> onnxruntime, one CPU thread
// (whisper_live/transcriber/transcriber_faster_whisper.py:830-838, whisper_live/batch_inference.py:245-248; I/O contract
// whisper_live/vad.py:50-109). CPU restatement: oracle/silero_vad.py.
//
// Shape of the work, 30 s chunk = 938 windows of 512 samples (+64 context):
//   front end (independent per window): STFT-as-conv 258x256 on 4 frames -> |.| -> 4 x (conv1d k3 + ReLU) -> feature[128]
//     -> input half of the LSTM gates gx[512] = W_ih f + b_ih + b_hh.      ~1.1 MFLOP and 2.3 KB of PCM per window against
//     0.7 MB of fp32 weights that stay in L2: arithmetic on the vector ALUs, all activations of a window group in LDS,
//     one workgroup per VAD_WT windows (235 workgroups for 30 s: fills the chip once).
//   recurrence (sequential over windows): g = gx[t] + W_hh h; (i,f,g,o) -> c,h.   ONE workgroup: W_hh (256 KB fp32)
//     lives in the registers of 512 lanes for the whole sequence — lane (unit j, quarter q) holds the four gate rows of
//     unit j over 32 of the 128 inputs — so a step is 8 broadcast LDS reads of h, 64 packed FMAs, a 2-step quad DPP
//     reduction, the gate non-linearities and one barrier. It is latency-bound by construction (938 dependent steps);
//     the CPU path it replaces is the same chain at ~30-50 us per step.
//   output: p[t] = sigmoid(w_out . relu(h_t) + b), parallel over windows.
//   ONE pass for every entry point (vad_run_batch): up to 64 sequences packed window after window, the front end and the recurrence
//     per item (one recurrence workgroup per item, side by side). wlx_vad_probs / _resident / _pcm are a batch of one; an item's bits
//     do not depend on its neighbours, its position or the table's fill.
// fp32 throughout (the gate thresholds at 0.5 / 0.35 are compared against these numbers; the oracle's own fp32-vs-fp64
// difference is 5e-7). Everything is deterministic: fixed summation orders, no atomics.
#include "engine.h"
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

namespace wlx {

constexpr int VAD_WINDOW = 512, VAD_CTX = 64, VAD_NFFT = 256, VAD_HOP = 128, VAD_BINS = 129, VAD_H = 128;
constexpr int VAD_XLEN = VAD_CTX + VAD_WINDOW + VAD_CTX;   // 640: context + window + reflected tail
constexpr int VAD_BSTRIDE = 260;                             // basisT row: 129 real + 129 imaginary filters, padded
constexpr int VAD_WT = 4;                                    // windows per front-end workgroup
constexpr int VAD_FE_THREADS = 256;

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct VadW {            // device pointers, kernel layouts (see vad_repack)
    const float* basisT;   // [256 n][260]: [n][k] real filter k, [n][129 + k] imaginary filter k
    const float* w1T;      // [129 ci][3][128 co]
    const float* w2T;      // [128 ci][3][64 co]
    const float* w3T;      // [64 ci][2][64 co]   taps 1, 2 (tap 0 only ever meets the left zero pad)
    const float* w4T;      // [64 ci][128 co]      centre tap (input length 1)
    const float* b1; const float* b2; const float* b3; const float* b4;
    const float* wihT;     // [128 k][512 r]
    const float* bias;     // [512] b_ih + b_hh
    const float* whhP;     // [4 gate][32 e][512 lane]: W_hh[gate*128 + j][32q + e], lane = 4j + q
    const float* out_w;    // [128]
    float out_b;
};

__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// ---------------------------------------------------------------------------------------------------------------------
// front end: VAD_WT windows per workgroup, PCM -> gx
// One workgroup's work: windows [w0, w0 + VAD_WT) of ONE sequence of `n` samples
// and `n_windows` windows whose gx rows start at `gx`. A sample position < 0 or >= n, or a window >= n_windows, reads 0.
__device__ __forceinline__ void vad_frontend_body(const float* __restrict__ pcm, long long n, int n_windows, int w0, const VadW& W,
                                                  float* __restrict__ gx) {
    __shared__ __attribute__((aligned(16))) float xs[VAD_WT][VAD_XLEN];
    __shared__ __attribute__((aligned(16))) float mag[VAD_WT][VAD_BINS][6];    // positions -1..4 (zero pads at both ends)
    __shared__ __attribute__((aligned(16))) float y1[VAD_WT][128][6];
    __shared__ __attribute__((aligned(16))) float y2[VAD_WT][64][4];           // positions -1..1 (+1 unused)
    __shared__ float y3[VAD_WT][64];
    __shared__ float y4[VAD_WT][VAD_H];
    __shared__ float nyq[16][VAD_WT * 4][2];
    const int tid = threadIdx.x;

    // ---- A: context + window (zeros before the start and past the end), then the reflected tail
    for (int i = tid; i < VAD_WT * (VAD_CTX + VAD_WINDOW); i += VAD_FE_THREADS) {
        const int w = i / (VAD_CTX + VAD_WINDOW), o = i - w * (VAD_CTX + VAD_WINDOW);
        const long long src = (long long)(w0 + w) * VAD_WINDOW - VAD_CTX + o;
        xs[w][o] = (src >= 0 && src < n && w0 + w < n_windows) ? pcm[src] : 0.0f;
    }
    __syncthreads();
    {
        const int w = tid >> 6, j = tid & 63;                                   // 256 threads = 4 windows x 64
        xs[w][VAD_CTX + VAD_WINDOW + j] = xs[w][VAD_CTX + VAD_WINDOW - 2 - j];
    }
    __syncthreads();

    // ---- B: STFT magnitude. Bins 0..127: lane (k, half) does 8 frames (2 windows); the Nyquist bin is split over n.
    {
        const int k = tid & 127, half = tid >> 7;
        float re[8], im[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) re[f] = im[f] = 0.0f;
        const float* bp = W.basisT + k;
        for (int nn = 0; nn < VAD_NFFT; nn += 4) {
            float br[4], bi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { br[u] = bp[(nn + u) * VAD_BSTRIDE]; bi[u] = bp[(nn + u) * VAD_BSTRIDE + VAD_BINS]; }
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                const f32x4 s = *reinterpret_cast<const f32x4*>(&xs[half * 2 + (f >> 2)][(f & 3) * VAD_HOP + nn]);
#pragma unroll
                for (int u = 0; u < 4; ++u) { re[f] = fmaf(br[u], s[u], re[f]); im[f] = fmaf(bi[u], s[u], im[f]); }
            }
        }
#pragma unroll
        for (int f = 0; f < 8; ++f) mag[half * 2 + (f >> 2)][k][1 + (f & 3)] = sqrtf(re[f] * re[f] + im[f] * im[f]);
        // Nyquist bin (k = 128): lane (frame f, part p) sums 16 taps; 16 parts are added in fixed order below
        const int f = tid & 15, p = tid >> 4;
        float nr = 0.0f, ni = 0.0f;
#pragma unroll 4
        for (int u = 0; u < 16; ++u) {
            const int nn = p * 16 + u;
            const float s = xs[f >> 2][(f & 3) * VAD_HOP + nn];
            nr = fmaf(W.basisT[nn * VAD_BSTRIDE + 128], s, nr);
            ni = fmaf(W.basisT[nn * VAD_BSTRIDE + VAD_BINS + 128], s, ni);
        }
        nyq[p][f][0] = nr; nyq[p][f][1] = ni;
        for (int i = tid; i < VAD_WT * VAD_BINS; i += VAD_FE_THREADS) {          // zero pads of mag
            mag[i / VAD_BINS][i % VAD_BINS][0] = 0.0f; mag[i / VAD_BINS][i % VAD_BINS][5] = 0.0f;
        }
    }
    __syncthreads();
    if (tid < VAD_WT * 4) {
        float nr = 0.0f, ni = 0.0f;
        for (int p = 0; p < 16; ++p) { nr += nyq[p][tid][0]; ni += nyq[p][tid][1]; }
        mag[tid >> 2][128][1 + (tid & 3)] = sqrtf(nr * nr + ni * ni);
    }
    __syncthreads();

    // ---- C: conv 129 -> 128, stride 1: lane (co, window pair) -> 2 windows x 4 positions
    {
        const int co = tid & 127, wh = tid >> 7;
        float acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[a][t] = 0.0f;
        for (int ci = 0; ci < VAD_BINS; ++ci) {
            const float wa = W.w1T[(ci * 3 + 0) * 128 + co], wb = W.w1T[(ci * 3 + 1) * 128 + co], wc = W.w1T[(ci * 3 + 2) * 128 + co];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float* m = mag[wh * 2 + a][ci];
                const f32x2 m01 = *reinterpret_cast<const f32x2*>(m), m23 = *reinterpret_cast<const f32x2*>(m + 2),
                            m45 = *reinterpret_cast<const f32x2*>(m + 4);
                acc[a][0] = fmaf(wc, m23[0], fmaf(wb, m01[1], fmaf(wa, m01[0], acc[a][0])));
                acc[a][1] = fmaf(wc, m23[1], fmaf(wb, m23[0], fmaf(wa, m01[1], acc[a][1])));
                acc[a][2] = fmaf(wc, m45[0], fmaf(wb, m23[1], fmaf(wa, m23[0], acc[a][2])));
                acc[a][3] = fmaf(wc, m45[1], fmaf(wb, m45[0], fmaf(wa, m23[1], acc[a][3])));
            }
        }
        const float b = W.b1[co];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float* y = y1[wh * 2 + a][co];
            y[0] = 0.0f; y[5] = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) y[1 + t] = fmaxf(acc[a][t] + b, 0.0f);
        }
    }
    __syncthreads();

    // ---- D: conv 128 -> 64, stride 2 (4 -> 2 positions): lane (co, window)
    {
        const int co = tid & 63, w = tid >> 6;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll 4
        for (int ci = 0; ci < 128; ++ci) {
            const float wa = W.w2T[(ci * 3 + 0) * 64 + co], wb = W.w2T[(ci * 3 + 1) * 64 + co], wc = W.w2T[(ci * 3 + 2) * 64 + co];
            const float* y = y1[w][ci];
            const f32x2 p01 = *reinterpret_cast<const f32x2*>(y), p23 = *reinterpret_cast<const f32x2*>(y + 2);
            const float p4 = y[4];
            a0 = fmaf(wc, p23[0], fmaf(wb, p01[1], fmaf(wa, p01[0], a0)));      // positions -1, 0, 1
            a1 = fmaf(wc, p4, fmaf(wb, p23[1], fmaf(wa, p23[0], a1)));          // positions  1, 2, 3
        }
        const float b = W.b2[co];
        y2[w][co][0] = 0.0f;
        y2[w][co][1] = fmaxf(a0 + b, 0.0f);
        y2[w][co][2] = fmaxf(a1 + b, 0.0f);
    }
    __syncthreads();

    // ---- E: conv 64 -> 64, stride 2 (2 -> 1 position; taps 1, 2 meet positions 0, 1)
    {
        const int co = tid & 63, w = tid >> 6;
        float a = 0.0f;
#pragma unroll 4
        for (int ci = 0; ci < 64; ++ci)
            a = fmaf(W.w3T[(ci * 2 + 1) * 64 + co], y2[w][ci][2], fmaf(W.w3T[(ci * 2 + 0) * 64 + co], y2[w][ci][1], a));
        y3[w][co] = fmaxf(a + W.b3[co], 0.0f);
    }
    __syncthreads();

    // ---- F: conv 64 -> 128 on one position (centre tap)
    {
        const int co = tid & 127, wh = tid >> 7;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll 4
        for (int ci = 0; ci < 64; ++ci) {
            const float wv = W.w4T[ci * 128 + co];
            a0 = fmaf(wv, y3[wh * 2][ci], a0);
            a1 = fmaf(wv, y3[wh * 2 + 1][ci], a1);
        }
        const float b = W.b4[co];
        y4[wh * 2][co] = fmaxf(a0 + b, 0.0f);
        y4[wh * 2 + 1][co] = fmaxf(a1 + b, 0.0f);
    }
    __syncthreads();

    // ---- G: input half of the gates: rows r = tid, tid + 256 for the 4 windows
    {
        float acc[2][VAD_WT];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int w = 0; w < VAD_WT; ++w) acc[a][w] = 0.0f;
#pragma unroll 4
        for (int k = 0; k < VAD_H; ++k) {
            const float wa = W.wihT[k * 512 + tid], wb = W.wihT[k * 512 + 256 + tid];
#pragma unroll
            for (int w = 0; w < VAD_WT; ++w) {
                const float f = y4[w][k];
                acc[0][w] = fmaf(wa, f, acc[0][w]);
                acc[1][w] = fmaf(wb, f, acc[1][w]);
            }
        }
        const float ba = W.bias[tid], bb = W.bias[256 + tid];
#pragma unroll
        for (int w = 0; w < VAD_WT; ++w)
            if (w0 + w < n_windows) {
                gx[(long long)(w0 + w) * 512 + tid] = acc[0][w] + ba;
                gx[(long long)(w0 + w) * 512 + 256 + tid] = acc[1][w] + bb;
            }
    }
}

// ---- ragged batch: up to WLX_VAD_MAX_BATCH sequences of different lengths, packed window after window without padding: item i owns
// windows [w0, w0 + T) of gx / hs / probs. The table travels BY VALUE in the kernel arguments (2 KiB, copied by the launch call itself,
// like spk.hip's item table): no staging buffer, no copy that could outlive the caller's frame. Only items with T >= 1 are in it.
struct VadItem {
    const float* pcm;    // the item's first sample (device)
    long long n;         // its samples: positions >= n read 0
    int T;               // its windows (ceil(n / 512) + extra zero windows)
    int w0;              // its first window in the packed buffers
    int g0;              // its first front-end workgroup (groups of VAD_WT windows, rounded up PER ITEM: no workgroup straddles two items)
    int pad_;
};
struct VadBatch {
    int n;
    VadItem it[WLX_VAD_MAX_BATCH];
};

// the item that owns front-end workgroup `grp`: the last one with g0 <= grp (g0 is strictly increasing: every item has a window)
__device__ __forceinline__ int vad_item_of(const VadBatch& tab, int grp) {
    int lo = 0, hi = tab.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.it[mid].g0 <= grp) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(VAD_FE_THREADS) void vad_frontend_batch_kernel(VadBatch tab, VadW W, float* __restrict__ gx) {
    const VadItem it = tab.it[vad_item_of(tab, (int)blockIdx.x)];              // workgroup-uniform
    vad_frontend_body(it.pcm, it.n, it.T, ((int)blockIdx.x - it.g0) * VAD_WT, W, gx + (long long)it.w0 * 512);
}

// ---------------------------------------------------------------------------------------------------------------------
// recurrence: one workgroup, W_hh register-resident
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {      // DPP quad_perm move: CTRL = p0 | p1 << 2 | p2 << 4 | p3 << 6
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// One workgroup's whole sequence: T steps from zero h and c over the gx rows at `gx`, states to the hs rows at `hs`.
__device__ __forceinline__ void vad_lstm_body(const float* __restrict__ gx, const float* __restrict__ whhP, float* __restrict__ hs, int T) {
    __shared__ __attribute__((aligned(16))) float hbuf[2][VAD_H];
    const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
    f32x2 wi[16], wf[16], wg[16], wo[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        wi[e] = f32x2{whhP[((0 * 32 + 2 * e) * 512) + tid], whhP[((0 * 32 + 2 * e + 1) * 512) + tid]};
        wf[e] = f32x2{whhP[((1 * 32 + 2 * e) * 512) + tid], whhP[((1 * 32 + 2 * e + 1) * 512) + tid]};
        wg[e] = f32x2{whhP[((2 * 32 + 2 * e) * 512) + tid], whhP[((2 * 32 + 2 * e + 1) * 512) + tid]};
        wo[e] = f32x2{whhP[((3 * 32 + 2 * e) * 512) + tid], whhP[((3 * 32 + 2 * e + 1) * 512) + tid]};
    }
    if (tid < VAD_H) hbuf[0][tid] = 0.0f;
    float c = 0.0f;
    float gxv = T > 0 ? gx[q * VAD_H + j] : 0.0f;          // lane q brings in gate q's input half for unit j
    {   // consume every preloaded register once before the loop: the compiler then settles all pending loads HERE instead
        // of carrying a conservative vmcnt wait into the loop header, where it would also drain the previous step's store
        f32x2 chk = {gxv, 0.0f};
#pragma unroll
        for (int e = 0; e < 16; ++e) chk += wi[e] + wf[e] + wg[e] + wo[e];
        if (chk[0] + chk[1] == 1.2345e38f && T < 0) hs[tid] = chk[0];
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float gnext = gx[(long long)min(t + 1, T - 1) * 512 + q * VAD_H + j];      // branch-free prefetch
        const f32x4* hp = reinterpret_cast<const f32x4*>(&hbuf[t & 1][32 * q]);
        f32x2 ai = {0.0f, 0.0f}, af = {0.0f, 0.0f}, ag = {0.0f, 0.0f}, ao = {0.0f, 0.0f};
#pragma unroll
        for (int e4 = 0; e4 < 8; ++e4) {
            const f32x4 h4 = hp[e4];
            const f32x2 lo = {h4[0], h4[1]}, hi = {h4[2], h4[3]};
            ai = __builtin_elementwise_fma(wi[2 * e4], lo, ai); ai = __builtin_elementwise_fma(wi[2 * e4 + 1], hi, ai);
            af = __builtin_elementwise_fma(wf[2 * e4], lo, af); af = __builtin_elementwise_fma(wf[2 * e4 + 1], hi, af);
            ag = __builtin_elementwise_fma(wg[2 * e4], lo, ag); ag = __builtin_elementwise_fma(wg[2 * e4 + 1], hi, ag);
            ao = __builtin_elementwise_fma(wo[2 * e4], lo, ao); ao = __builtin_elementwise_fma(wo[2 * e4 + 1], hi, ao);
        }
        // Transpose-reduce over the quad: every lane holds a partial of all four gates over its quarter of h; after two
        // exchange steps lane q holds the complete pre-activation of gate q (3 DPP moves instead of an 8-move butterfly),
        // applies that gate's non-linearity once (tanh(x) = 2 sigmoid(2x) - 1 keeps the code uniform), and the four
        // activations are broadcast back: 4 transcendental instructions per lane and step instead of 10.
        const float p0 = ai[0] + ai[1], p1 = af[0] + af[1], p2 = ag[0] + ag[1], p3 = ao[0] + ao[1];
        const bool b0 = q & 1, b1 = q & 2;
        const float xa = (b0 ? p1 : p0) + quad_perm<0xB1>(b0 ? p0 : p1);        // gate b0      over lanes {q, q^1}
        const float xb = (b0 ? p3 : p2) + quad_perm<0xB1>(b0 ? p2 : p3);        // gate 2 + b0
        const float s = (b1 ? xb : xa) + quad_perm<0x4E>(b1 ? xa : xb) + gxv;   // gate q, all four lanes
        const float sg2 = (q == 2) ? 2.0f : 1.0f;
        float a = sigmoidf_(sg2 * s);
        a = (q == 2) ? 2.0f * a - 1.0f : a;
        const float gi = quad_perm<0x00>(a), gf = quad_perm<0x55>(a), gg = quad_perm<0xAA>(a), go = quad_perm<0xFF>(a);
        c = gf * c + gi * gg;
        const float h = go * tanhf_(c);
        // all four lanes of the quad hold the same h: unconditional stores (same LDS word; hs keeps one word per lane) so
        // that no divergent branch hides the outstanding store from the compiler's vmcnt bookkeeping
        hbuf[(t + 1) & 1][j] = h;
        hs[(long long)t * 512 + tid] = h;
        gxv = gnext;
        // LDS-only barrier: __syncthreads() would also drain vmcnt, i.e. wait out the latency of the hs store and of the
        // gx prefetch on every one of the T dependent steps
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

// blockIdx.x is the item; the recurrences are independent and run side by side, one CU each (a workgroup takes a CU's
// whole register file, so items beyond the free CUs queue behind the first to finish)
__global__ __launch_bounds__(512) void vad_lstm_batch_kernel(VadBatch tab, const float* __restrict__ gx, const float* __restrict__ whhP,
                                                              float* __restrict__ hs) {
    const int T = tab.it[blockIdx.x].T;
    const long long row0 = (long long)tab.it[blockIdx.x].w0 * 512;
    vad_lstm_body(gx + row0, whhP, hs + row0, T);
}

// output layer: p[t] = sigmoid(w_out . relu(h_t) + b); one wave per window
__global__ __launch_bounds__(256) void vad_out_kernel(const float* __restrict__ hs, const float* __restrict__ out_w, float out_b,
                                                       float* __restrict__ probs, int T) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const float* h = hs + (long long)t * 512;                      // [unit j][4 identical copies]
    float v = out_w[lane] * fmaxf(h[4 * lane], 0.0f) + out_w[64 + lane] * fmaxf(h[4 * (64 + lane)], 0.0f);
    v = dpp_wave_sum(v);
    if (lane == 0) probs[t] = 1.0f / (1.0f + expf(-(v + out_b)));
}

}  // namespace wlx

// ---------------------------------------------------------------------------------------------------------------------
// C-ABI
using namespace wlx;

struct wlx_vad {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<void*> pool;
    VadW W{};
    float *d_pcm = nullptr, *d_gx = nullptr, *d_hs = nullptr, *d_probs = nullptr;
    float* h_pin = nullptr;              // pinned staging: PCM in
    long long cap_samples = 0;
    float* h_probs = nullptr;            // pinned staging: probabilities out
    long long cap_windows = 0;           // windows d_gx / d_hs / d_probs / h_probs hold
    std::mutex mu;
};

static int vad_upload(wlx_vad* v, const std::vector<float>& host, const float** out) {
    float* p = nullptr;
    CKR(dalloc(v->pool, &p, host.size(), false));
    CK(hipMemcpyAsync(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, v->stream));   // never the legacy stream
    CK(hipStreamSynchronize(v->stream));
    *out = p;
    return WLX_OK;
}

// the per-window buffers (front-end output, LSTM states, probabilities): what every entry point needs, whoever holds the samples
static int vad_reserve_windows(wlx_vad* v, long long wins) {
    if (wins <= v->cap_windows) return WLX_OK;
    long long cap = 16000LL * 64 / VAD_WINDOW + 1;
    while (cap < wins) cap *= 2;
    for (float* p : {v->d_gx, v->d_hs, v->d_probs})
        if (p) (void)hipFree(p);
    if (v->h_probs) (void)hipHostFree(v->h_probs);
    v->d_gx = v->d_hs = v->d_probs = v->h_probs = nullptr;
    v->cap_windows = 0;
    // grown with the longest chunk seen, the old buffers freed above: owned by name, not by a free list
    CK(hipMalloc((void**)&v->d_gx, cap * 512 * sizeof(float)));
    CK(hipMalloc((void**)&v->d_hs, cap * 512 * sizeof(float)));
    CK(hipMalloc((void**)&v->d_probs, cap * sizeof(float)));
    CK(hipHostMalloc((void**)&v->h_probs, cap * sizeof(float), hipHostMallocDefault));
    v->cap_windows = cap;
    return WLX_OK;
}

static int vad_reserve(wlx_vad* v, long long n_samples) {
    if (n_samples <= v->cap_samples) return WLX_OK;
    long long cap = 16000LL * 64;                                    // 64 s covers every streaming chunk (<= 45 s buffer)
    while (cap < n_samples) cap *= 2;
    if (v->d_pcm) (void)hipFree(v->d_pcm);
    if (v->h_pin) (void)hipHostFree(v->h_pin);
    v->d_pcm = v->h_pin = nullptr;
    v->cap_samples = 0;
    CKR(vad_reserve_windows(v, cap / VAD_WINDOW + 1));
    // grown with the longest chunk seen, the old buffers freed above: owned by name, not by a free list
    CK(hipMalloc((void**)&v->d_pcm, cap * sizeof(float)));
    CK(hipHostMalloc((void**)&v->h_pin, cap * sizeof(float), hipHostMallocDefault));
    v->cap_samples = cap;
    return WLX_OK;
}

extern "C" int32_t wlx_vad_create(const wlx_vad_weights* w, int32_t device, wlx_vad** out) {
    if (!w || !out) return set_error(WLX_ERR_ARG, "wlx_vad_create: null argument");
    const float* need[] = {w->stft_basis, w->enc_w[0], w->enc_w[1], w->enc_w[2], w->enc_w[3], w->enc_b[0], w->enc_b[1],
                           w->enc_b[2], w->enc_b[3], w->lstm_w_ih, w->lstm_w_hh, w->lstm_b_ih, w->lstm_b_hh, w->out_w, w->out_b};
    for (const float* p : need)
        if (!p) return set_error(WLX_ERR_WEIGHT, "wlx_vad_create: a weight pointer is null");
    CK(hipSetDevice(device));
    wlx_vad* v = new wlx_vad();
    v->device = device;
    auto bail = [&](int rc) { wlx_vad_destroy(v); return rc; };
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&v->ev0) != hipSuccess ||
        hipEventCreate(&v->ev1) != hipSuccess)
        return bail(set_error(WLX_ERR_HIP, "wlx_vad_create: stream/event creation failed"));
    // ---- repack into the kernel layouts
    std::vector<float> t;
    int rc;
    t.assign(256 * VAD_BSTRIDE, 0.0f);
    for (int r = 0; r < 258; ++r)
        for (int n = 0; n < 256; ++n) t[n * VAD_BSTRIDE + r] = w->stft_basis[r * 256 + n];
    if ((rc = vad_upload(v, t, &v->W.basisT))) return bail(rc);
    auto conv_t = [&](const float* src, int cout, int cin, int j0, int nj, const float** dst) {   // [co][ci][3] -> [ci][nj][co]
        t.assign((size_t)cin * nj * cout, 0.0f);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int j = 0; j < nj; ++j) t[((size_t)ci * nj + j) * cout + co] = src[((size_t)co * cin + ci) * 3 + j0 + j];
        return vad_upload(v, t, dst);
    };
    if ((rc = conv_t(w->enc_w[0], 128, 129, 0, 3, &v->W.w1T))) return bail(rc);
    if ((rc = conv_t(w->enc_w[1], 64, 128, 0, 3, &v->W.w2T))) return bail(rc);
    if ((rc = conv_t(w->enc_w[2], 64, 64, 1, 2, &v->W.w3T))) return bail(rc);
    if ((rc = conv_t(w->enc_w[3], 128, 64, 1, 1, &v->W.w4T))) return bail(rc);
    const int bn[4] = {128, 64, 64, 128};
    const float** bd[4] = {&v->W.b1, &v->W.b2, &v->W.b3, &v->W.b4};
    for (int i = 0; i < 4; ++i) {
        t.assign(w->enc_b[i], w->enc_b[i] + bn[i]);
        if ((rc = vad_upload(v, t, bd[i]))) return bail(rc);
    }
    t.assign(128 * 512, 0.0f);
    for (int r = 0; r < 512; ++r)
        for (int k = 0; k < 128; ++k) t[k * 512 + r] = w->lstm_w_ih[r * 128 + k];
    if ((rc = vad_upload(v, t, &v->W.wihT))) return bail(rc);
    t.assign(512, 0.0f);
    for (int r = 0; r < 512; ++r) t[r] = w->lstm_b_ih[r] + w->lstm_b_hh[r];
    if ((rc = vad_upload(v, t, &v->W.bias))) return bail(rc);
    t.assign(4 * 32 * 512, 0.0f);
    for (int g = 0; g < 4; ++g)
        for (int e = 0; e < 32; ++e)
            for (int lane = 0; lane < 512; ++lane) {
                const int j = lane >> 2, q = lane & 3;
                t[(g * 32 + e) * 512 + lane] = w->lstm_w_hh[(g * 128 + j) * 128 + 32 * q + e];
            }
    if ((rc = vad_upload(v, t, &v->W.whhP))) return bail(rc);
    t.assign(w->out_w, w->out_w + 128);
    if ((rc = vad_upload(v, t, &v->W.out_w))) return bail(rc);
    v->W.out_b = w->out_b[0];
    if ((rc = vad_reserve(v, 16000LL * 64))) return bail(rc);
    *out = v;
    return WLX_OK;
}

extern "C" void wlx_vad_destroy(wlx_vad* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void* p : v->pool) (void)hipFree(p);
    for (float* p : {v->d_pcm, v->d_gx, v->d_hs, v->d_probs})
        if (p) (void)hipFree(p);
    if (v->h_pin) (void)hipHostFree(v->h_pin);
    if (v->h_probs) (void)hipHostFree(v->h_probs);
    if (v->ev0) (void)hipEventDestroy(v->ev0);
    if (v->ev1) (void)hipEventDestroy(v->ev1);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

// ------------------------------------------------------------------ the pass (every wlx_vad_probs* entry point ends in vad_run_batch)
// The geometry of a pass: the table of the items that have a window (window offsets, front-end groups rounded up per item), T_i of
// EVERY item, the packed window count and the sample total. The sample pointers are filled in by the caller.
struct VadPlan {
    VadBatch tab;
    int src[WLX_VAD_MAX_BATCH];              // table entry -> item of the call
    int T[WLX_VAD_MAX_BATCH];
    long long windows = 0, samples = 0;
    int groups = 0;
};

// Everything both batch entry points refuse on the arguments alone. Nothing of the caller's is written here.
static int vad_plan(const char* who, const int64_t* n_samples, const int32_t* extra, int32_t n, int64_t cap, VadPlan& pl) {
    if (n < 1 || n > WLX_VAD_MAX_BATCH) return set_error(WLX_ERR_ARG, "%s: %d items (1..%d)", who, n, WLX_VAD_MAX_BATCH);
    pl.tab.n = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t ni = n_samples[i];
        const int ex = extra ? extra[i] : 0;
        if (ni < 0) return set_error(WLX_ERR_ARG, "%s: item %d has a negative sample count", who, i);
        if (ex < 0 || ex > 4) return set_error(WLX_ERR_ARG, "%s: item %d: extra_zero_windows out of range", who, i);
        if (ni > 16000LL * 3600 || (pl.samples += ni) > 16000LL * 3600) return set_error(WLX_ERR_ARG, "%s: more than 3600 s of audio", who);
        const int T = (int)((ni + VAD_WINDOW - 1) / VAD_WINDOW) + ex;
        pl.T[i] = T;
        if (T == 0) continue;
        pl.src[pl.tab.n] = i;
        pl.tab.it[pl.tab.n++] = VadItem{nullptr, (long long)ni, T, (int)pl.windows, pl.groups, 0};
        pl.windows += T;
        pl.groups += (T + VAD_WT - 1) / VAD_WT;
    }
    for (int k = pl.tab.n; k < WLX_VAD_MAX_BATCH; ++k) pl.tab.it[k] = VadItem{nullptr, 0, 0, 0, 0, 0};
    if (pl.windows > cap) return set_error(WLX_ERR_ARG, "%s: %lld windows do not fit the output buffer (%lld)", who, pl.windows, (long long)cap);
    return WLX_OK;
}

// the plan of the single entry points, which keep their own refusals: one item of T >= 1 windows over the n samples at `pcm`
static void vad_plan_one(const float* pcm, long long n, int T, VadPlan& pl) {
    pl.tab.n = 1;
    pl.tab.it[0] = VadItem{pcm, n, T, 0, 0, 0};
    for (int k = 1; k < WLX_VAD_MAX_BATCH; ++k) pl.tab.it[k] = VadItem{nullptr, 0, 0, 0, 0, 0};
    pl.src[0] = 0, pl.T[0] = T;
    pl.windows = T, pl.samples = n, pl.groups = (T + VAD_WT - 1) / VAD_WT;
}

// the pass itself on v->stream, behind whatever the caller put there (an upload, a wait for another stream): one launch of each kernel
// over the packed windows, one download, one wait. v->mu is held, the device is set and the per-window buffers hold pl.windows.
// The three launches of the pass, each over the packed windows of `pl`. vad_run_batch and the wlx_vad_debug_* hooks call these and
// nothing else, so a hook launches what the pass launches.
static void vad_launch_frontend(const VadPlan& pl, const VadW& W, float* gx, hipStream_t st) {
    hipLaunchKernelGGL(vad_frontend_batch_kernel, dim3(pl.groups), dim3(VAD_FE_THREADS), 0, st, pl.tab, W, gx);
}
static void vad_launch_lstm(const VadPlan& pl, const float* gx, const VadW& W, float* hs, hipStream_t st) {
    hipLaunchKernelGGL(vad_lstm_batch_kernel, dim3(pl.tab.n), dim3(512), 0, st, pl.tab, gx, W.whhP, hs);
}
static void vad_launch_out(const float* hs, const VadW& W, float* probs, int T, hipStream_t st) {
    hipLaunchKernelGGL(vad_out_kernel, dim3((T + 3) / 4), dim3(256), 0, st, hs, W.out_w, W.out_b, probs, T);
}

static int vad_run_batch(wlx_vad* v, const VadPlan& pl, float* probs_out, float* device_ms_out) {
    const int T = (int)pl.windows;
    CK(hipEventRecord(v->ev0, v->stream));
    vad_launch_frontend(pl, v->W, v->d_gx, v->stream);
    vad_launch_lstm(pl, v->d_gx, v->W, v->d_hs, v->stream);
    vad_launch_out(v->d_hs, v->W, v->d_probs, T, v->stream);
    CK(hipGetLastError());
    CK(hipEventRecord(v->ev1, v->stream));
    CK(hipMemcpyAsync(v->h_probs, v->d_probs, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, v->stream));
    CK(hipStreamSynchronize(v->stream));
    memcpy(probs_out, v->h_probs, (size_t)T * sizeof(float));
    if (device_ms_out) CK(hipEventElapsedTime(device_ms_out, v->ev0, v->ev1));
    return WLX_OK;
}

// ------------------------------------------------------------------ one sequence: a batch of one (the refusals are each entry point's own)
extern "C" int32_t wlx_vad_probs(wlx_vad* v, const float* pcm, int64_t n, float* probs_out, int32_t cap,
                                 int32_t* n_windows_out, float* device_ms_out) {
    if (!v || !n_windows_out || (n > 0 && (!pcm || !probs_out))) return set_error(WLX_ERR_ARG, "wlx_vad_probs: null argument");
    if (n < 0) return set_error(WLX_ERR_ARG, "wlx_vad_probs: negative sample count");
    const long long T = (n + VAD_WINDOW - 1) / VAD_WINDOW;
    *n_windows_out = (int32_t)T;
    if (device_ms_out) *device_ms_out = 0.0f;
    if (T == 0) return WLX_OK;
    if (T > cap) return set_error(WLX_ERR_ARG, "wlx_vad_probs: %lld windows do not fit the output buffer (%d)", T, cap);
    std::lock_guard<std::mutex> lk(v->mu);
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();                  // a stale error of this thread must not be blamed on the launches below
    CKR(vad_reserve(v, n));
    memcpy(v->h_pin, pcm, (size_t)n * sizeof(float));
    CK(hipMemcpyAsync(v->d_pcm, v->h_pin, (size_t)n * sizeof(float), hipMemcpyHostToDevice, v->stream));
    VadPlan pl;
    vad_plan_one(v->d_pcm, n, (int)T, pl);
    return vad_run_batch(v, pl, probs_out, device_ms_out);
}

// The same on samples that are already in HBM: [start, start + n) of a client's PCM ring (ring.hip wlx_ring_*, include/wlx.h) — the
// gate of a streaming session reads the ring the socket thread filled, no second host-to-device copy.
extern "C" int32_t wlx_vad_probs_resident(wlx_vad* v, wlx_ring* r, int64_t start, int64_t n, int32_t extra_zero_windows, float* probs_out, int32_t cap,
                                          int32_t* n_windows_out, float* device_ms_out) {
    if (!v || !r || !n_windows_out || (n > 0 && !probs_out)) return set_error(WLX_ERR_ARG, "wlx_vad_probs_resident: null argument");
    if (n < 0) return set_error(WLX_ERR_ARG, "wlx_vad_probs_resident: negative sample count");
    CKR(PcmLease::same_device("wlx_vad_probs_resident", "ring", r->device, "VAD model", v->device));
    if (extra_zero_windows < 0 || extra_zero_windows > 4) return set_error(WLX_ERR_ARG, "wlx_vad_probs_resident: extra_zero_windows out of range");
    const long long T = (n + VAD_WINDOW - 1) / VAD_WINDOW + extra_zero_windows;
    *n_windows_out = (int32_t)T;
    if (device_ms_out) *device_ms_out = 0.0f;
    if (T == 0) return WLX_OK;
    if (T > cap) return set_error(WLX_ERR_ARG, "wlx_vad_probs_resident: %lld windows do not fit the output buffer (%d)", T, cap);
    std::lock_guard<std::mutex> lk(v->mu);
    PcmLease L;
    L.open_ring(r);
    const float* pcm;
    CKR(L.range("wlx_vad_probs_resident", start, n, &pcm));
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();
    CKR(vad_reserve(v, n + (long long)extra_zero_windows * VAD_WINDOW));
    VadPlan pl;
    vad_plan_one(pcm, n, (int)T, pl);
    return vad_run_batch(v, pl, probs_out, device_ms_out);
}

// The same on a slot item's resident PCM (wlx_pcm_put / wlx_pcm_put_frames): the gate of a FILE reads the 16 kHz copy the front end left
// in HBM. Nothing of the VAD object grows with the file but the per-window buffers: d_pcm and h_pin are not touched.
extern "C" int32_t wlx_vad_probs_pcm(wlx_vad* v, wlx_engine* e, int32_t slot, int32_t item, int64_t start, int64_t n, int32_t extra_zero_windows,
                                     float* probs_out, int32_t cap, int32_t* n_windows_out, float* device_ms_out) {
    if (!v || !e || !n_windows_out || (n > 0 && !probs_out)) return set_error(WLX_ERR_ARG, "wlx_vad_probs_pcm: null argument");
    if (n < 0 || start < 0) return set_error(WLX_ERR_ARG, "wlx_vad_probs_pcm: negative position or sample count");
    CKR(PcmLease::same_device("wlx_vad_probs_pcm", "engine", e->device, "VAD model", v->device));
    if (extra_zero_windows < 0 || extra_zero_windows > 4) return set_error(WLX_ERR_ARG, "wlx_vad_probs_pcm: extra_zero_windows out of range");
    PcmLease L;
    CKR(L.open_slot(e, slot));
    CKR(L.item("wlx_vad_probs_pcm", item));
    const long long T = (n + VAD_WINDOW - 1) / VAD_WINDOW + extra_zero_windows;
    *n_windows_out = (int32_t)T;
    if (device_ms_out) *device_ms_out = 0.0f;
    const float* pcm;
    CKR(L.range("wlx_vad_probs_pcm", start, n, &pcm));
    if (T == 0) return WLX_OK;
    if (T > cap) return set_error(WLX_ERR_ARG, "wlx_vad_probs_pcm: %lld windows do not fit the output buffer (%d)", T, cap);
    std::lock_guard<std::mutex> lk(v->mu);
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();
    CKR(vad_reserve_windows(v, T));
    CKR(L.order(v->stream));
    VadPlan pl;
    vad_plan_one(pcm, n, (int)T, pl);
    return vad_run_batch(v, pl, probs_out, device_ms_out);
}

// ------------------------------------------------------------------ ragged batch (include/wlx.h wlx_vad_probs_batch)
extern "C" int32_t wlx_vad_probs_batch(wlx_vad* v, const float* pcm, const int64_t* n_samples, const int32_t* extra_zero_windows, int32_t n,
                                       float* probs_out, int64_t cap, int32_t* n_windows_out, float* device_ms_out) {
    if (!v || !pcm || !n_samples || !probs_out || !n_windows_out) return set_error(WLX_ERR_ARG, "wlx_vad_probs_batch: null argument");
    VadPlan pl;
    CKR(vad_plan("wlx_vad_probs_batch", n_samples, extra_zero_windows, n, cap, pl));
    std::lock_guard<std::mutex> lk(v->mu);
    if (pl.windows > 0) {
        CK(hipSetDevice(v->device));
        (void)hipGetLastError();
        CKR(vad_reserve(v, pl.samples));
        CKR(vad_reserve_windows(v, pl.windows));
    }
    for (int i = 0; i < n; ++i) n_windows_out[i] = pl.T[i];
    if (device_ms_out) *device_ms_out = 0.0f;
    if (pl.windows == 0) return WLX_OK;
    // the segments lie back to back in `pcm`: one copy to the pinned buffer, one to the device, and the table points into it
    if (pl.samples > 0) {
        memcpy(v->h_pin, pcm, (size_t)pl.samples * sizeof(float));
        CK(hipMemcpyAsync(v->d_pcm, v->h_pin, (size_t)pl.samples * sizeof(float), hipMemcpyHostToDevice, v->stream));
    }
    std::vector<long long> off(n + 1, 0);
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + n_samples[i];
    for (int k = 0; k < pl.tab.n; ++k) pl.tab.it[k].pcm = v->d_pcm + off[pl.src[k]];
    return vad_run_batch(v, pl, probs_out, device_ms_out);
}

extern "C" int32_t wlx_vad_probs_pcm_batch(wlx_vad* v, wlx_engine* e, int32_t slot, int32_t first_item, const int64_t* n_samples,
                                           const int32_t* extra_zero_windows, int32_t n, float* probs_out, int64_t cap,
                                           int32_t* n_windows_out, float* device_ms_out) {
    if (!v || !e || !n_samples || !probs_out || !n_windows_out) return set_error(WLX_ERR_ARG, "wlx_vad_probs_pcm_batch: null argument");
    CKR(PcmLease::same_device("wlx_vad_probs_pcm_batch", "engine", e->device, "VAD model", v->device));
    VadPlan pl;
    CKR(vad_plan("wlx_vad_probs_pcm_batch", n_samples, extra_zero_windows, n, cap, pl));
    PcmLease L;
    CKR(L.open_slot(e, slot));
    CKR(L.item("wlx_vad_probs_pcm_batch", first_item, n));
    // (an item with n == 0 and extra windows reads no sample: its pointer is never dereferenced, the slot may hold no PCM buffer yet)
    const float* pcm[WLX_VAD_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        L.view(first_item + i);
        CKR(L.range("wlx_vad_probs_pcm_batch", 0, n_samples[i], &pcm[i]));
    }
    std::lock_guard<std::mutex> lk(v->mu);
    if (pl.windows > 0) {
        CK(hipSetDevice(v->device));
        (void)hipGetLastError();
        CKR(vad_reserve_windows(v, pl.windows));
    }
    for (int i = 0; i < n; ++i) n_windows_out[i] = pl.T[i];
    if (device_ms_out) *device_ms_out = 0.0f;
    if (pl.windows == 0) return WLX_OK;
    CKR(L.order(v->stream));
    for (int k = 0; k < pl.tab.n; ++k) pl.tab.it[k].pcm = pcm[pl.src[k]];
    return vad_run_batch(v, pl, probs_out, device_ms_out);
}

// ------------------------------------------------------------------ kernel-level test hooks (include/wlx.h wlx_vad_debug_*)
// ONE launch each of the launch functions of the pass, on the object's stream under its mutex, with the object's repacked weights. The
// output lives in a buffer of the call (not d_gx / d_hs / d_probs, which have no room for guard words): the caller's words go in, the
// launch runs, all of them come back.
namespace {
struct VadHookBufs {       // device buffers of one hook call: the stream is waited for and they are freed on every return path
    hipStream_t st;
    std::vector<void*> pool;
    explicit VadHookBufs(hipStream_t s) : st(s) {}
    ~VadHookBufs() {
        (void)hipStreamSynchronize(st);
        for (void* p : pool) (void)hipFree(p);
    }
    int upload(float** d, const float* h, size_t n) {
        CKR(dalloc(pool, d, n, false));
        CK(hipMemcpyAsync(*d, h, n * sizeof(float), hipMemcpyHostToDevice, st));
        return WLX_OK;
    }
    int finish(float* h, const float* d, size_t n) {
        CK(hipGetLastError());
        CK(hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        return WLX_OK;
    }
};
constexpr int64_t VAD_HOOK_MAX_WINDOWS = 1 << 19;      // 2^28 words of gx / hs
}  // namespace

extern "C" int32_t wlx_vad_debug_frontend(wlx_vad* v, const float* pcm, const int64_t* n_samples, const int32_t* extra_zero_windows, int32_t n,
                                          float* gx, int64_t cap_windows) {
    if (!v || !pcm || !n_samples || !gx) return set_error(WLX_ERR_ARG, "wlx_vad_debug_frontend: null argument");
    if (cap_windows < 1 || cap_windows > VAD_HOOK_MAX_WINDOWS)
        return set_error(WLX_ERR_ARG, "wlx_vad_debug_frontend: capacity %lld outside 1..2^19 windows", (long long)cap_windows);
    VadPlan pl;
    CKR(vad_plan("wlx_vad_debug_frontend", n_samples, extra_zero_windows, n, cap_windows, pl));
    if (pl.windows == 0) return WLX_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();
    CKR(vad_reserve(v, pl.samples));
    if (pl.samples > 0) {
        memcpy(v->h_pin, pcm, (size_t)pl.samples * sizeof(float));
        CK(hipMemcpyAsync(v->d_pcm, v->h_pin, (size_t)pl.samples * sizeof(float), hipMemcpyHostToDevice, v->stream));
    }
    std::vector<long long> off(n + 1, 0);
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + n_samples[i];
    for (int k = 0; k < pl.tab.n; ++k) pl.tab.it[k].pcm = v->d_pcm + off[pl.src[k]];
    VadHookBufs B(v->stream);
    const size_t words = (size_t)cap_windows * 512 + WLX_DEBUG_GUARD;
    float* d_gx = nullptr;
    CKR(B.upload(&d_gx, gx, words));
    vad_launch_frontend(pl, v->W, d_gx, v->stream);
    return B.finish(gx, d_gx, words);
}

extern "C" int32_t wlx_vad_debug_lstm(wlx_vad* v, const float* gx, const int32_t* T, int32_t n, float* hs, int64_t cap_windows) {
    if (!v || !gx || !T || !hs) return set_error(WLX_ERR_ARG, "wlx_vad_debug_lstm: null argument");
    if (cap_windows < 1 || cap_windows > VAD_HOOK_MAX_WINDOWS)
        return set_error(WLX_ERR_ARG, "wlx_vad_debug_lstm: capacity %lld outside 1..2^19 windows", (long long)cap_windows);
    if (n < 1 || n > WLX_VAD_MAX_BATCH) return set_error(WLX_ERR_ARG, "wlx_vad_debug_lstm: %d items (1..%d)", n, WLX_VAD_MAX_BATCH);
    int64_t samples[WLX_VAD_MAX_BATCH];                      // T windows are T * 512 samples to vad_plan, which builds the table as is
    for (int i = 0; i < n; ++i) {
        if (T[i] < 0) return set_error(WLX_ERR_ARG, "wlx_vad_debug_lstm: item %d has a negative window count", i);
        samples[i] = (int64_t)T[i] * VAD_WINDOW;
    }
    VadPlan pl;
    CKR(vad_plan("wlx_vad_debug_lstm", samples, nullptr, n, cap_windows, pl));
    if (pl.windows == 0) return WLX_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();
    VadHookBufs B(v->stream);
    const size_t words = (size_t)cap_windows * 512 + WLX_DEBUG_GUARD;
    float *d_gx = nullptr, *d_hs = nullptr;
    CKR(B.upload(&d_gx, gx, (size_t)pl.windows * 512));
    CKR(B.upload(&d_hs, hs, words));
    vad_launch_lstm(pl, d_gx, v->W, d_hs, v->stream);
    return B.finish(hs, d_hs, words);
}

extern "C" int32_t wlx_vad_debug_out(wlx_vad* v, const float* hs, int32_t T, float* probs, int64_t cap_windows) {
    if (!v || !hs || !probs) return set_error(WLX_ERR_ARG, "wlx_vad_debug_out: null argument");
    if (cap_windows < 1 || cap_windows > VAD_HOOK_MAX_WINDOWS)
        return set_error(WLX_ERR_ARG, "wlx_vad_debug_out: capacity %lld outside 1..2^19 windows", (long long)cap_windows);
    if (T < 0) return set_error(WLX_ERR_ARG, "wlx_vad_debug_out: negative window count");
    if (T > cap_windows) return set_error(WLX_ERR_ARG, "wlx_vad_debug_out: %d windows do not fit the output buffer (%lld)", T, (long long)cap_windows);
    if (T == 0) return WLX_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    CK(hipSetDevice(v->device));
    (void)hipGetLastError();
    VadHookBufs B(v->stream);
    const size_t words = (size_t)cap_windows + WLX_DEBUG_GUARD;
    float *d_hs = nullptr, *d_probs = nullptr;
    CKR(B.upload(&d_hs, hs, (size_t)T * 512));
    CKR(B.upload(&d_probs, probs, words));
    vad_launch_out(d_hs, v->W, d_probs, T, v->stream);
    return B.finish(probs, d_probs, words);
}

// ------------------------------------------------------------------ host: hysteresis segmentation of the probabilities
// whisperlive_amd/vad.py speech_segments_from_probs (= faster_whisper.vad.get_speech_timestamps' loop, as the reference calls it at
// whisper_live/transcriber/transcriber_faster_whisper.py:825-852) statement for statement, in C: the loop runs on the host BETWEEN the VAD launch
// and the log-mel launch — the GPU waits for it — and costs 36 us for the 250 windows of an 8 s chunk and 136 us for 30 s in Python, ~2 us here
// (round 6). The thresholds arrive as doubles already rounded to float32 (numpy compares a float32 probability with a Python float in float32);
// the durations are the Python code's floats (max_speech may be +inf); positions are integers. Python's `gap // 2` floors.
extern "C" int32_t wlx_vad_segments(const float* probs, int32_t n_windows, int64_t n_samples, double thr, double neg, double min_speech, double pad,
                                    double max_speech, double min_silence, double min_silence_at_max, int64_t* start_end_out, int32_t cap,
                                    int32_t* n_out) {
    if (!probs || n_windows < 0 || !start_end_out || !n_out || cap < 0) return set_error(WLX_ERR_ARG, "wlx_vad_segments: bad argument");
    const int64_t W = 512;
    int32_t ns = 0;
    auto push = [&](int64_t a, int64_t b) -> bool { if (ns >= cap) return false; start_end_out[2 * ns] = a; start_end_out[2 * ns + 1] = b; ++ns; return true; };
    bool have_cur = false, active = false;
    int64_t cur_start = 0, silence_from = 0, cut_at = 0, resume_at = 0;
    for (int32_t i = 0; i < n_windows; ++i) {
        const double p = (double)probs[i];
        const int64_t pos = W * i;
        if (p >= thr && silence_from) {
            silence_from = 0;
            if (resume_at < cut_at) resume_at = pos;
        }
        if (p >= thr && !active) { active = true; cur_start = pos; have_cur = true; continue; }
        if (active && (double)(pos - cur_start) > max_speech) {
            if (cut_at) {
                if (!push(cur_start, cut_at)) return set_error(WLX_ERR_ARG, "wlx_vad_segments: more segments than the output holds");
                have_cur = false;
                if (resume_at < cut_at) active = false;
                else { cur_start = resume_at; have_cur = true; }
                cut_at = resume_at = silence_from = 0;
            } else {
                if (!push(cur_start, pos)) return set_error(WLX_ERR_ARG, "wlx_vad_segments: more segments than the output holds");
                have_cur = false;
                cut_at = resume_at = silence_from = 0;
                active = false;
                continue;
            }
        }
        if (p < neg && active) {
            if (!silence_from) silence_from = pos;
            if ((double)(pos - silence_from) > min_silence_at_max) cut_at = silence_from;
            if ((double)(pos - silence_from) < min_silence) continue;
            if ((double)(silence_from - cur_start) > min_speech) { if (!push(cur_start, silence_from)) return set_error(WLX_ERR_ARG, "wlx_vad_segments: more segments than the output holds"); }
            have_cur = false;
            cut_at = resume_at = silence_from = 0;
            active = false;
        }
    }
    if (have_cur && (double)(n_samples - cur_start) > min_speech) { if (!push(cur_start, n_samples)) return set_error(WLX_ERR_ARG, "wlx_vad_segments: more segments than the output holds"); }
    auto floordiv2 = [](int64_t g) -> int64_t { return (g >= 0) ? g / 2 : -((-g + 1) / 2); };
    auto clamp0 = [](double v) -> int64_t { return (int64_t)(v > 0.0 ? v : 0.0); };
    for (int32_t i = 0; i < ns; ++i) {
        int64_t& s_ = start_end_out[2 * i]; int64_t& e_ = start_end_out[2 * i + 1];
        if (i == 0) s_ = clamp0((double)s_ - pad);
        if (i != ns - 1) {
            int64_t& s2 = start_end_out[2 * i + 2];
            const int64_t gap = s2 - e_;
            if ((double)gap < 2.0 * pad) {
                e_ += floordiv2(gap);
                const int64_t t = s2 - floordiv2(gap);
                s2 = t > 0 ? t : 0;
            } else {
                const double ee = (double)e_ + pad;
                e_ = (int64_t)(ee < (double)n_samples ? ee : (double)n_samples);
                s2 = clamp0((double)s2 - pad);
            }
        } else {
            const double ee = (double)e_ + pad;
            e_ = (int64_t)(ee < (double)n_samples ? ee : (double)n_samples);
        }
    }
    *n_out = ns;
    return WLX_OK;
}
