// kernels.h — host-callable launchers of the gfx950 kernels (one .hip file per group).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace wlx {

// ---------------------------------------------------------------- pack.hip
// W[n][k] fp32 (row stride ldw) -> packed fp16 fragments at n-tile offset nt0 of a [NT_total][KT] image.
void launch_pack_linear(const float* W, int N, int K, long ldw, half_t* Wp, int KT, int nt0, hipStream_t s);
// conv weight W[c][ci][3] fp32 -> rows n=c, k = j*Cin + ci
void launch_pack_conv3(const float* W, int Cout, int Cin, half_t* Wp, int KT, hipStream_t s);
void launch_f32_to_f16(const float* src, half_t* dst, long n, hipStream_t s);

// ---------------------------------------------------------------- logmel.hip
struct LogmelConsts {          // device pointers, built once per engine
    const float* window;       // [400] periodic Hann
    const float* twiddle;      // [400][2] cos, sin of 2*pi*j/400 (float64-rounded)
    const float* filters;      // [n_mels][201] Slaney mel filterbank
    const int*   frange;       // [n_mels][2] first/last+1 non-zero bin
};
// up to WLX_LM_MAXB items per launch (blockIdx.y = item): per item the PCM, its length, the feature matrix, T = (n+160)/160 and a uint scratch
#define WLX_LM_MAXB 16
// An item's samples are pcm[0 .. n), or — round 6, the PCM ring — the CONCATENATION of nr ranges of `pcm`: rng = device table of
// nr x {first sample of the range in pcm, position of that sample in the concatenation} (int64 pairs, positions ascending from 0);
// the loads that bring a tile's samples into LDS walk the table (a tile of 8 frames spans at most a few ranges).
#define WLX_LM_MAXRANGES 256
struct LogmelBatch {
    int n_items;
    const float* pcm[WLX_LM_MAXB]; long n[WLX_LM_MAXB]; float* feats[WLX_LM_MAXB]; int T[WLX_LM_MAXB]; unsigned* gmax[WLX_LM_MAXB];
    const long long* rng[WLX_LM_MAXB]; int nr[WLX_LM_MAXB];
};
// The chunk-gather form (include/wlx.h wlx_logmel_chunks): chunk c = the concatenation of nr ranges, rows r0 .. r0 + nr of ONE range table
// `rng` (same pair layout as above) over ONE PCM buffer, n samples in all, T = (n + 160) / 160 frames into feature item `item`
// (feats0 + item * item_stride, gmax0 + item). The descriptors live in device memory: up to 64 chunks (a slot's max_batch) per launch.
struct LogmelChunk { long long n; int T, r0, nr, item; };
void launch_logmel_chunks(const float* pcm, const LogmelChunk* chunks, int n_chunks, int Tmax, const long long* rng, float* feats0,
                          long item_stride, unsigned* gmax0, int n_mels, const LogmelConsts& c, long ld, hipStream_t s);
void launch_logmel_batch(const LogmelBatch& lb, int n_mels, const LogmelConsts& c, long ld, hipStream_t s);
// pcm [n] f32 device -> feats [n_mels][ld] f32 device (T = (n+160)/160 columns valid); gmax: 1 uint scratch
void launch_logmel(const float* pcm, long n, int n_mels, const LogmelConsts& c, float* feats, long ld,
                   int T, unsigned* gmax, hipStream_t s);
// feats window [seek, seek+seg) -> time-major fp16 featT rows 1..3000 (row stride n_mels), zero beyond seg
struct PrepWindows { int seek[64]; int seg[64]; };     // per item of a slot (wlx_slot_create: max_batch <= 64)
void launch_prep_windows(const float* feats0, long ld, int n_mels, long item_stride, const PrepWindows& w, int items,
                         half_t* featT0, long featT_stride, hipStream_t s);

// ---------------------------------------------------------------- gemm.hip
enum GemmMode : int {
    GEMM_STORE_F16 = 0,    // C[m][n] = f16(acc + bias)
    GEMM_GELU_F16 = 1,     // C[m][n] = f16(gelu(acc + bias))
    GEMM_GELU_POS_F32 = 2, // X[m][n] = gelu(acc + bias) + pos[m][n]          (conv2 + positions)
    GEMM_RESID_F32 = 3,    // X[m][n] += acc + bias                            (residual stream)
    GEMM_QKV = 4,          // n<d: q (scaled) ; d<=n<2d: k ; else v transposed
    GEMM_CROSS_KV = 5      // per decoder layer l: k rows, v transposed
};
struct GemmParams {
    const half_t* A; long lda; long strideA;   // activations, row-major fp16; z-batch stride
    const half_t* Wp; int KT;                  // packed weights
    int M, N;                                  // rows per z-batch, real output columns
    int mode;
    const float* bias;                         // [N] or null
    half_t* C; long ldc; long strideC;         // fp16 output (modes 0,1; q for mode 4)
    float* X; long ldx; long strideX;          // fp32 output (modes 2,3)
    const float* pos;                          // [M][N] (mode 2)
    // mode 4/5 extras
    int d;                                     // d_model
    float qscale;
    half_t* Kout; long ldk;                    // k rows  [rows][d]
    half_t* Vt; long ldvt;                     // v transposed [d][ldvt] per item
    int rows_per_item;                         // 1500
    long kv_item_stride_k, kv_item_stride_v;   // per item
    long kv_layer_stride_k, kv_layer_stride_v; // per decoder layer (mode 5)
    int xcd_a, xcd_b;                          // (set by the launcher, second GEMM form) XCD-aware tile map: a m-parts x b n-parts
    int epi_lds;                               // (set by the launcher, second GEMM form) fp16 outputs leave through an LDS-transposed epilogue
    int g3_gx, g3_tiles;                       // (set by the launcher, third GEMM form) tiles along n, tiles in all
};
void launch_gemm(const GemmParams& p, int zbatch, hipStream_t s);
// test hooks: the form launch_gemm picks (0..2 second-form tiles, 3 large-M form); one launch on a given form (gemm.hip)
int gemm_form_of(const GemmParams& p, int zbatch);
void launch_gemm_form(const GemmParams& p, int zbatch, int form, GemmParams* ran, hipStream_t s);
// per-device set-up of the GEMM kernels (large dynamic-LDS opt-in); returns a hipError_t value
int gemm_prepare_device();
// x fp32 [M][d] -> fp16 LN(x)*gamma+beta [M][d]
void launch_layernorm_f16(const float* x, long ldx, const float* gamma, const float* beta,
                          half_t* out, long ldo, int M, int d, hipStream_t s);
// x fp32 [M][d] -> fp32 LN (final encoder LN, API copy) and fp16
void launch_layernorm_f16_f32(const float* x, long ldx, const float* gamma, const float* beta,
                              half_t* out16, float* out32, long ldo, int M, int d, hipStream_t s);

// ---------------------------------------------------------------- attention.hip
// non-causal encoder self-attention, head_dim 64. Q,K row-major fp16 (q pre-scaled), Vt [H*64][ldvt].
void launch_attn_encoder(const half_t* Q, long ldq, const half_t* K, long ldk, const half_t* Vt, long ldvt,
                         half_t* O, long ldo, int T, int H, int items,
                         long item_stride_q, long item_stride_k, long item_stride_vt, long item_stride_o,
                         hipStream_t s);

// ---------------------------------------------------------------- resample.hip
// file audio -> 16 kHz mono float32: sample conversion, channel mean and polyphase resampling (scipy.signal.resample_poly's filter)
constexpr size_t RS_BLOCK_BYTES = 8u << 20;                                // file bytes per staged block of the product path
struct ResamplePlan { int up, down, half_len, tile; const float* taps; }; // tile: outputs per workgroup; taps: device, [2 * half_len + 1], cached per device and ratio
// the two halves of the bounded staging a run streams the file through: device blocks, and (product path) pinned host blocks with
// the event recorded behind the copy out of each
struct ResampleStage { unsigned char* pinned[2]; unsigned char* dev[2]; hipEvent_t copied[2]; bool used[2]; };
int resample_check_args(const void* frames, long long n_frames, int channels, int sample_format, int sample_rate);
int resample_ratio(int sample_rate, int* up, int* down, int* tile);      // 16000 / rate reduced and its tile; needs no device
int resample_plan(int device, int sample_rate, ResamplePlan* out);        // WLX_ERR_ARG for a ratio the kernel does not serve
long long resample_out_len(const ResamplePlan& pl, long long n_frames);   // ceil(n_frames * up / down)
long long resample_reach(const ResamplePlan& pl);                         // smallest legal block, in input frames
long long resample_default_block(int channels, int sample_format);        // frames per staged block of the product path
// host frames -> d_out[0 .. out_len), one copy and one launch per block of `block_frames` input frames on `st`; waits for `st`.
// kernel_ms (nullable): the launches' summed HIP-event time. split_stride > 0: the channel-split form — no down-mix, channel c goes to
// d_out + c * split_stride (one launch per block still, blockIdx.y = channel).
int resample_run(const ResamplePlan& pl, const void* frames, long long n_frames, int channels, int sample_format, long long block_frames,
                 ResampleStage& sg, float* d_out, hipStream_t st, float* kernel_ms, long long split_stride = 0);
// device float32 frames [n_frames][channels] -> d_out[0 .. out_len): one launch on `st`, no copy, no wait (the FLAC front end, flac.hip)
int resample_run_device(const ResamplePlan& pl, const float* d_frames, long long n_frames, int channels, float* d_out, hipStream_t st);
// ... and its channel-split sibling: channel c -> d_out + c * out_stride, one launch with blockIdx.y = channel
int resample_run_device_split(const ResamplePlan& pl, const float* d_frames, long long n_frames, int channels, float* d_out,
                              long long out_stride, hipStream_t st);

// flac.hip: host -> device on `st` through the two pinned staging blocks of `sg` (two copies in flight; *blk counts blocks across calls),
// or straight from the caller's memory when sg is null. Does not wait: the caller synchronises and then clears sg->used.
int staged_upload(ResampleStage* sg, int* blk, void* dst, const void* src, size_t n, hipStream_t st);

// The STREAM form (the live path: wlx_ring_append_frames; test hook wlx_debug_resample_stream): the same kernel fed packet by packet.
// With J input frames seen and M outputs emitted, a packet of n frames completes the outputs [M, M') whose newest input exists
// (flush: all of the one-shot's ceil(J' up / down), frames past the end being zero). The state is J, M and the last `tail_len` <=
// resample_reach input frames on the device, in the wire format; a call stages [tail | packet] and launches ONE grid over [M, M')
// with the window's absolute start as j_base — an output depends on absolute input indices only, so the packet seams cannot move a
// bit against the one-shot.
struct ResampleStream {
    ResamplePlan pl{};
    int fmt = 0, channels = 0, rate = 0;
    bool closed = false;                                    // flushed: no further packets
    long long J = 0, M = 0;
    unsigned char* tail = nullptr; long long tail_len = 0;  // device, [resample_reach][channels] in the wire format
    unsigned char* stage = nullptr; size_t stage_cap = 0;   // device, bytes: [tail | packet], grown on demand
};
int resample_format_bytes(int sample_format);                                               // 4 / 2 / 1; 0 for an unknown code
int resample_stream_check(int sample_format, int channels, int sample_rate);                // host only: format, channels, RATES
long long resample_stream_count(int up, int down, int half_len, long long frames_seen, int flush);   // M' as a function of J'
int resample_stream_open(int device, int sample_format, int channels, int sample_rate, ResampleStream* rs);
long long resample_stream_next(const ResampleStream& rs, long long n_frames, int flush);    // M' - M of the next call
int resample_stream_reserve(ResampleStream& rs, long long n_frames);                        // staging for a packet; nothing of rs in flight
// copies and ONE launch on `st`, output M lands at d_dst[0]; does not wait (the caller's frames are pageable: wait before returning them).
// lane_stride > 0: the channel-split form of a ring group — no down-mix, ONE launch with blockIdx.y = channel, channel c's output M lands
// at d_dst[c * lane_stride]; window, tail and staging are the same whole interleaved frames.
int resample_stream_enqueue(ResampleStream& rs, const void* frames, long long n_frames, int flush, float* d_dst, hipStream_t st,
                            long long lane_stride = 0);
void resample_stream_free(ResampleStream& rs);

}  // namespace wlx
