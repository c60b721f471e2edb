// resample.hip — the device audio front end of the file path: sample conversion (int16 / float32), channel down-mix and polyphase
// resampling to 16 kHz in one kernel (include/wlx.h wlx_pcm_put_frames; test hook wlx_debug_resample).
//
// Arithmetic = scipy.signal.resample_poly(mean over channels, up, down) with its default filter, which is what
// whisperlive_amd/audio_io.py load_audio computes on the host in float64:
//   half_len = 10 * max(up, down);  h = up * firwin(2 * half_len + 1, 1 / max(up, down), window = ("kaiser", 5.0))
//   y[m] = sum_j x[j] * h[half_len + m * down - j * up]          (indices inside h; x is zero outside the file)
// The taps are designed here in double (sinc x Kaiser, unit gain at DC), rounded to float32 once and cached per device and ratio.
// The kernel accumulates in float32, ALWAYS in the same order for a given output (k ascending = input index descending from the newest
// sample the output reaches), and an output depends on nothing but the absolute input indices: where a block or tile seam falls
// cannot change a bit of the result.
//
// Work split: a workgroup of 256 lanes owns a tile of 1024 consecutive outputs (512 ... 64 for the steep down-sampling ratios whose
// input span would not fit otherwise, resample_ratio). It copies the whole tap table into LDS in its natural
// order and stages the input span its tile reaches — (tile - 1) * down / up frames plus 2 * half_len / up of history and look-ahead —
// converting and down-mixing on the way in, so every file sample is converted once per tile and then read ~(taps per output * up /
// down) times from LDS. The natural order of h IS the phase order: lane i of a wave reads h[p_i + k * up] with p_i = (half_len + m_i *
// down) mod up for consecutive m_i, i.e. addresses that step by (down mod up) — odd for 441 against 160 / 320 / 640 / 80, so the
// lanes of a half wave fall into distinct banks; up = 1 or 2 (every rate that is a multiple of 8 kHz) is an LDS broadcast. The input
// reads step by down / up frames per lane (two- to four-way conflicts at 96 / 192 kHz, where the kernel is still far shorter than
// the upload of its input). The job is bound by the PCIe upload, not by this kernel.
//
// The channel-split form (include/wlx.h wlx_pcm_put_frames_split, wlx_pcm_put_flac_split; test hook wlx_debug_resample_split) is the
// SPLIT instantiation of the same kernel: blockIdx.y = channel c, the staging loop reads sample r * channels + c — no mean, no
// division — and the outputs go to out + c * out_stride. Tap table, LDS layout, tile, accumulation order and seam logic are the ones
// above, so channel c is BIT-IDENTICAL to the down-mix form run on the one-channel array frames[:, c]: the mono path of that form does
// no division either (its `ch > 1` branch is not taken), and an output depends on nothing but the absolute input indices.
//
// The STREAM form (include/wlx.h wlx_ring_set_format / wlx_ring_append_frames; test hook wlx_debug_resample_stream; kernels.h
// ResampleStream) is the same kernel fed packet by packet: raw = [the last `reach` frames | the packet] with j_base its absolute
// start, [m0, m1) = the outputs the packet completes, `out` rebased so that output m0 lands where the caller wants it. It adds the
// 8-bit wire formats of live sources (uint8, G.711 mu-law / A-law) to rs_sample; nothing else in the kernel knows about streams.
//
// The stream form of the SPLIT instantiation (include/wlx.h wlx_ring_group_append_frames) is the two together: the same [tail | packet]
// window of whole interleaved frames, shared by all channels, one grid over [M, M') x channels, channel c's outputs rebased into lane c
// of the group (out_stride = the lane stride). All five formats have a split instantiation for it; lane c is bit-identical to the
// stream form of the down-mix kernel fed channel c alone, for the reason given above.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <tuple>
#include "host.h"
#include "resample_core.h"

namespace wlx {

struct ResampleArgs {
    const void* raw;        // interleaved frames [j_base, j_base + raw_frames) of the file, in the file's format
    long long j_base, raw_frames, n_frames;
    int channels;
    int up, down, half_len;
    int tile;               // outputs per workgroup
    const float* taps;      // [2 * half_len + 1]
    float* out;             // out[m] for m in [m0, m1)
    long long m0, m1;
    long long out_stride;   // SPLIT only: channel c writes out[c * out_stride + m]
};

template <int FMT, bool SPLIT = false>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleArgs p) {
    extern __shared__ float rs_lds[];
    const int ntaps = 2 * p.half_len + 1;
    float* hs = rs_lds;
    float* xs = rs_lds + ntaps;
    const long long mA = p.m0 + (long long)blockIdx.x * p.tile;
    const long long mB = mA + p.tile < p.m1 ? mA + p.tile : p.m1;
    // the input span of the tile: j with 0 <= half_len + m * down - j * up <= 2 * half_len for some m in [mA, mB)
    const long long j_lo = -floor_div(-(mA * p.down - p.half_len), p.up);          // ceil((mA * down - half_len) / up)
    const long long j_hi = floor_div((long long)p.half_len + (mB - 1) * p.down, p.up);
    const int span = (int)(j_hi - j_lo + 1);
    for (int i = threadIdx.x; i < ntaps; i += RS_THREADS) hs[i] = p.taps[i];
    const int ch = p.channels;
    const float fch = (float)ch;
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long j = j_lo + i;
        float v = 0.f;
        const long long r = j - p.j_base;
        if (j >= 0 && j < p.n_frames && r >= 0 && r < p.raw_frames) {
            const long long b = r * ch;
            v = rs_sample<FMT>(p.raw, SPLIT ? b + blockIdx.y : b);
            if (!SPLIT && ch > 1) {                          // the float32 mean: channels added in order, one division
                for (int c = 1; c < ch; ++c) v += rs_sample<FMT>(p.raw, b + c);
                v = v / fch;
            }
        }
        xs[i] = v;
    }
    __syncthreads();
    float* out = SPLIT ? p.out + (long long)blockIdx.y * p.out_stride : p.out;
    for (long long m = mA + threadIdx.x; m < mB; m += RS_THREADS) {
        if (p.half_len == 0) {                                 // 16 kHz in: the converted, down-mixed sample itself (a -0.0f stays -0.0f)
            out[m] = xs[m - j_lo];
            continue;
        }
        const long long t = (long long)p.half_len + m * p.down;
        const long long jh = t / p.up;                         // the newest input the output reaches
        const int ph = (int)(t - jh * p.up);                   // its tap = the output's phase
        const int K = (2 * p.half_len - ph) / p.up + 1;
        const float* x = xs + (jh - j_lo);
        const float* h = hs + ph;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(x[-k], h[(long)k * p.up], acc);
        out[m] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ the plan of one ratio
static double bessel_i0(double x) {             // sum ((x / 2)^k / k!)^2: converges in ~25 terms at x = 5
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

static long long gcd_ll(long long a, long long b) { while (b) { long long t = a % b; a = b; b = t; } return a; }

void resample_design(int up, int down, std::vector<float>& taps, int* half_len_out) {
    if (up == down) {                           // 16 kHz in: conversion and down-mix only (the kernel copies, the tap is not read)
        taps.assign(1, 1.0f);
        *half_len_out = 0;
        return;
    }
    const int mx = std::max(up, down), hl = 10 * mx, n = 2 * hl + 1;
    const double c = 1.0 / mx, pi = 3.14159265358979323846, i0b = bessel_i0(5.0);
    std::vector<double> h((size_t)n);
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double m = (double)(i - hl), a = pi * c * m;
        const double sinc = (i == hl) ? 1.0 : std::sin(a) / a;
        const double r = m / (double)hl;
        const double w = bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h[i] = c * sinc * w;
        s += h[i];
    }
    taps.resize((size_t)n);
    for (int i = 0; i < n; ++i) taps[i] = (float)((double)up * (h[i] / s));
    *half_len_out = hl;
}

// 16000 / sample_rate reduced, and the tile the kernel runs that ratio with. SERVED (include/wlx.h; mirrored by
// whisperlive_amd/engine.py resample_supported): max(up, down) <= RS_MAX_RATIO, and the tap table plus the input span of RS_MIN_TILE
// outputs fit RS_MAX_LDS. Needs no device.
int resample_ratio(int sample_rate, int* up, int* down, int* tile) {
    if (sample_rate <= 0) return set_error(WLX_ERR_ARG, "sample rate %d must be positive", sample_rate);
    const long long g = gcd_ll(16000, sample_rate);
    const long long u = 16000 / g, d = sample_rate / g;
    if (std::max(u, d) > RS_MAX_RATIO)
        return set_error(WLX_ERR_ARG, "sample rate %d Hz: 16000 / rate reduces to %lld / %lld, over the %d the device resampler serves "
                         "(resample on the host)", sample_rate, u, d, RS_MAX_RATIO);
    const int hl = u == d ? 0 : 10 * (int)std::max(u, d);
    int t = RS_TILE;
    while (t > RS_MIN_TILE && rs_lds_bytes((int)u, (int)d, hl, t) > (size_t)RS_MAX_LDS) t /= 2;
    if (rs_lds_bytes((int)u, (int)d, hl, t) > (size_t)RS_MAX_LDS)
        return set_error(WLX_ERR_ARG, "sample rate %d Hz: the tap table and the input span of %d outputs do not fit the device resampler's "
                         "LDS (resample on the host)", sample_rate, RS_MIN_TILE);
    *up = (int)u; *down = (int)d; *tile = t;
    return WLX_OK;
}

// the filter's reach in input frames: the smallest block that still yields one output (resample_block_outputs >= 1)
long long resample_reach(const ResamplePlan& pl) { return (2LL * pl.half_len + pl.up - 1) / pl.up + 2; }
// outputs a block of `block_frames` input frames serves, wherever it starts
static long long resample_block_outputs(const ResamplePlan& pl, long long block_frames) {
    return ((block_frames - 2) * pl.up - 2LL * pl.half_len) / pl.down + 1;
}

int resample_plan(int device, int sample_rate, ResamplePlan* out) {
    int up = 0, down = 0, tile = 0;
    CKR(resample_ratio(sample_rate, &up, &down, &tile));
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, ResamplePlan> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({device, up, down});
    if (it != cache.end()) { *out = it->second; return WLX_OK; }
    std::vector<float> taps;
    ResamplePlan pl{};
    pl.up = up; pl.down = down; pl.tile = tile;
    resample_design(up, down, taps, &pl.half_len);
    CK(hipSetDevice(device));
    float* d = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&d), taps.size() * sizeof(float)));      // lives as long as the process: <= 51 KB per ratio and device
    CKR(upload_sync(d, taps.data(), taps.size() * sizeof(float)));
    pl.taps = d;
    cache[{device, up, down}] = pl;
    *out = pl;
    return WLX_OK;
}

long long resample_out_len(const ResamplePlan& pl, long long n_frames) { return (n_frames * pl.up + pl.down - 1) / pl.down; }

long long resample_default_block(int channels, int sample_format) {
    return (long long)(RS_BLOCK_BYTES / ((size_t)channels * (size_t)resample_format_bytes(sample_format)));
}

// one launch: the down-mix form (split_stride == 0: grid.y = 1) or the split form (grid.y = channels, p.out_stride = split_stride)
static void rs_launch(int sample_format, unsigned grid, size_t lds, hipStream_t st, ResampleArgs& p, long long split_stride) {
    if (split_stride > 0) {
        p.out_stride = split_stride;
        const dim3 g(grid, (unsigned)p.channels);
        switch (sample_format) {                        // the 8-bit formats reach here from a ring group and from a G.711 WAV file (adpcm.hip)
        case WLX_PCM_S16: hipLaunchKernelGGL((resample_kernel<WLX_PCM_S16, true>), g, dim3(RS_THREADS), lds, st, p); break;
        case WLX_PCM_U8: hipLaunchKernelGGL((resample_kernel<WLX_PCM_U8, true>), g, dim3(RS_THREADS), lds, st, p); break;
        case WLX_PCM_MULAW: hipLaunchKernelGGL((resample_kernel<WLX_PCM_MULAW, true>), g, dim3(RS_THREADS), lds, st, p); break;
        case WLX_PCM_ALAW: hipLaunchKernelGGL((resample_kernel<WLX_PCM_ALAW, true>), g, dim3(RS_THREADS), lds, st, p); break;
        default: hipLaunchKernelGGL((resample_kernel<WLX_PCM_F32, true>), g, dim3(RS_THREADS), lds, st, p); break;
        }
        return;
    }
    switch (sample_format) {                            // the 8-bit formats reach here from the stream form and from a G.711 WAV file (adpcm.hip)
    case WLX_PCM_S16: hipLaunchKernelGGL(resample_kernel<WLX_PCM_S16>, dim3(grid), dim3(RS_THREADS), lds, st, p); break;
    case WLX_PCM_U8: hipLaunchKernelGGL(resample_kernel<WLX_PCM_U8>, dim3(grid), dim3(RS_THREADS), lds, st, p); break;
    case WLX_PCM_MULAW: hipLaunchKernelGGL(resample_kernel<WLX_PCM_MULAW>, dim3(grid), dim3(RS_THREADS), lds, st, p); break;
    case WLX_PCM_ALAW: hipLaunchKernelGGL(resample_kernel<WLX_PCM_ALAW>, dim3(grid), dim3(RS_THREADS), lds, st, p); break;
    default: hipLaunchKernelGGL(resample_kernel<WLX_PCM_F32>, dim3(grid), dim3(RS_THREADS), lds, st, p); break;
    }
}

int resample_run(const ResamplePlan& pl, const void* frames, long long n_frames, int channels, int sample_format, long long block_frames,
                 ResampleStage& sg, float* d_out, hipStream_t st, float* kernel_ms, long long split_stride) {
    const size_t fb = (size_t)channels * (size_t)resample_format_bytes(sample_format);
    const long long n_out = resample_out_len(pl, n_frames);
    const long long per = block_frames >= resample_reach(pl) ? resample_block_outputs(pl, block_frames) : 0;
    if (per < 1) return set_error(WLX_ERR_ARG, "block of %lld frames is smaller than the filter's reach (%lld)", block_frames, resample_reach(pl));
    const size_t lds = rs_lds_bytes(pl.up, pl.down, pl.half_len, pl.tile);
    std::vector<hipEvent_t> evs;
    int rc = WLX_OK;
    long long blk = 0;
    for (long long m0 = 0; m0 < n_out && rc == WLX_OK; m0 += per, ++blk) {
        const long long m1 = std::min(n_out, m0 + per);
        // the file frames outputs [m0, m1) reach, clamped to the file
        long long a = m0 * pl.down - pl.half_len;
        long long j_lo = a >= 0 ? (a + pl.up - 1) / pl.up : -((-a) / pl.up);
        long long j_hi = ((long long)pl.half_len + (m1 - 1) * pl.down) / pl.up;
        j_lo = std::max(j_lo, 0LL); j_hi = std::min(j_hi, n_frames - 1);
        const long long nfr = std::max(0LL, j_hi - j_lo + 1);            // <= block_frames by the choice of `per`
        const int b = (int)(blk & 1);
        const char* src = static_cast<const char*>(frames) + (size_t)j_lo * fb;
        rc = [&]() -> int {
            if (nfr > 0) {
                if (sg.pinned[b]) {
                    // the pinned half is free once the copy out of it (two blocks ago) has run
                    if (sg.used[b]) CK(hipEventSynchronize(sg.copied[b]));
                    std::memcpy(sg.pinned[b], src, (size_t)nfr * fb);
                    CK(hipMemcpyAsync(sg.dev[b], sg.pinned[b], (size_t)nfr * fb, hipMemcpyHostToDevice, st));
                    CK(hipEventRecord(sg.copied[b], st));
                    sg.used[b] = true;
                } else {
                    CK(hipMemcpyAsync(sg.dev[b], src, (size_t)nfr * fb, hipMemcpyHostToDevice, st));   // pageable source: staged by the runtime before it returns
                }
            }
            ResampleArgs p{};
            p.raw = sg.dev[b]; p.j_base = j_lo; p.raw_frames = nfr; p.n_frames = n_frames; p.channels = channels;
            p.up = pl.up; p.down = pl.down; p.half_len = pl.half_len; p.tile = pl.tile; p.taps = pl.taps; p.out = d_out; p.m0 = m0; p.m1 = m1;
            const unsigned grid = (unsigned)((m1 - m0 + pl.tile - 1) / pl.tile);
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (kernel_ms) {
                CK(hipEventCreate(&e0)); evs.push_back(e0);
                CK(hipEventCreate(&e1)); evs.push_back(e1);
                CK(hipEventRecord(e0, st));
            }
            rs_launch(sample_format, grid, lds, st, p, split_stride);
            CK(hipGetLastError());
            if (kernel_ms) CK(hipEventRecord(e1, st));
            return WLX_OK;
        }();
    }
    if (rc == WLX_OK) {
        hipError_t he = hipStreamSynchronize(st);     // the caller's frames and the staging halves may be reused after return
        if (he != hipSuccess) rc = set_error(WLX_ERR_HIP, "resample: %s", hipGetErrorString(he));
    } else {
        (void)hipStreamSynchronize(st);
    }
    sg.used[0] = sg.used[1] = false;
    if (kernel_ms) {
        float total = 0.f;
        for (size_t i = 0; i + 1 < evs.size() && rc == WLX_OK; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, evs[i], evs[i + 1]) == hipSuccess) total += ms;
        }
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        *kernel_ms = total;
    }
    return rc;
}

// The device-source path (flac.hip): the file's float32 frames are in HBM already, so the whole file is ONE block — raw = the device
// frames, j_base = 0, raw_frames = n_frames — and one launch of the same kernel with the same arithmetic. Does not wait.
int resample_run_device(const ResamplePlan& pl, const float* d_frames, long long n_frames, int channels, float* d_out, hipStream_t st) {
    const long long n_out = resample_out_len(pl, n_frames);
    if (n_out <= 0) return WLX_OK;
    ResampleArgs p{};
    p.raw = d_frames; p.j_base = 0; p.raw_frames = n_frames; p.n_frames = n_frames; p.channels = channels;
    p.up = pl.up; p.down = pl.down; p.half_len = pl.half_len; p.tile = pl.tile; p.taps = pl.taps; p.out = d_out; p.m0 = 0; p.m1 = n_out;
    const unsigned grid = (unsigned)((n_out + pl.tile - 1) / pl.tile);
    hipLaunchKernelGGL(resample_kernel<WLX_PCM_F32>, dim3(grid), dim3(RS_THREADS), rs_lds_bytes(pl.up, pl.down, pl.half_len, pl.tile), st, p);
    CK(hipGetLastError());
    return WLX_OK;
}

// The split sibling: channel c of the device frames -> d_out + c * out_stride, one launch with grid.y = channels. Does not wait.
int resample_run_device_split(const ResamplePlan& pl, const float* d_frames, long long n_frames, int channels, float* d_out,
                              long long out_stride, hipStream_t st) {
    const long long n_out = resample_out_len(pl, n_frames);
    if (n_out <= 0) return WLX_OK;
    ResampleArgs p{};
    p.raw = d_frames; p.j_base = 0; p.raw_frames = n_frames; p.n_frames = n_frames; p.channels = channels;
    p.up = pl.up; p.down = pl.down; p.half_len = pl.half_len; p.tile = pl.tile; p.taps = pl.taps; p.out = d_out; p.m0 = 0; p.m1 = n_out;
    const unsigned grid = (unsigned)((n_out + pl.tile - 1) / pl.tile);
    rs_launch(WLX_PCM_F32, grid, rs_lds_bytes(pl.up, pl.down, pl.half_len, pl.tile), st, p, out_stride);
    CK(hipGetLastError());
    return WLX_OK;
}

// one validation for the product entry point and the hook: everything that does not need a device
int resample_check_args(const void* frames, long long n_frames, int channels, int sample_format, int sample_rate) {
    if (n_frames < 0) return set_error(WLX_ERR_ARG, "negative frame count");
    if (n_frames > (1LL << 50)) return set_error(WLX_ERR_ARG, "frame count out of range");      // n_frames * up stays inside int64
    if (channels < 1 || channels > WLX_PCM_MAX_CHANNELS) return set_error(WLX_ERR_ARG, "channels %d outside 1..%d", channels, WLX_PCM_MAX_CHANNELS);
    if (sample_format != WLX_PCM_F32 && sample_format != WLX_PCM_S16) return set_error(WLX_ERR_ARG, "unknown sample format %d", sample_format);
    if (sample_rate <= 0) return set_error(WLX_ERR_ARG, "sample rate %d must be positive", sample_rate);
    if (n_frames > 0 && !frames) return set_error(WLX_ERR_ARG, "null frames");
    int up, down, tile;
    return resample_ratio(sample_rate, &up, &down, &tile);
}

// ------------------------------------------------------------------------------------------------ the stream form (kernels.h)
int resample_format_bytes(int sample_format) {
    switch (sample_format) {
    case WLX_PCM_F32: return 4;
    case WLX_PCM_S16: return 2;
    case WLX_PCM_U8: case WLX_PCM_MULAW: case WLX_PCM_ALAW: return 1;
    default: return 0;
    }
}

int resample_stream_check(int sample_format, int channels, int sample_rate) {
    if (!resample_format_bytes(sample_format)) return set_error(WLX_ERR_ARG, "unknown sample format %d", sample_format);
    if (channels < 1 || channels > WLX_PCM_MAX_CHANNELS) return set_error(WLX_ERR_ARG, "channels %d outside 1..%d", channels, WLX_PCM_MAX_CHANNELS);
    int up, down, tile;
    return resample_ratio(sample_rate, &up, &down, &tile);
}

// no flush: the outputs whose newest input, floor((half_len + m * down) / up), is below J', i.e. half_len + m * down <= J' * up - 1;
// flush: the one-shot length. The first never exceeds the second, and both grow with J'.
long long resample_stream_count(int up, int down, int half_len, long long frames_seen, int flush) {
    if (flush) return (frames_seen * up + down - 1) / down;
    const long long a = frames_seen * up - 1 - half_len;
    return a < 0 ? 0 : a / down + 1;
}

int resample_stream_open(int device, int sample_format, int channels, int sample_rate, ResampleStream* rs) {
    CKR(resample_stream_check(sample_format, channels, sample_rate));
    ResampleStream s{};
    CKR(resample_plan(device, sample_rate, &s.pl));
    s.fmt = sample_format; s.channels = channels; s.rate = sample_rate;
    CK(hipSetDevice(device));
    CK(hipMalloc(reinterpret_cast<void**>(&s.tail), (size_t)resample_reach(s.pl) * channels * resample_format_bytes(sample_format)));   // owned by name: resample_stream_free
    *rs = s;
    return WLX_OK;
}

long long resample_stream_next(const ResampleStream& rs, long long n_frames, int flush) {
    return resample_stream_count(rs.pl.up, rs.pl.down, rs.pl.half_len, rs.J + n_frames, flush) - rs.M;
}

int resample_stream_reserve(ResampleStream& rs, long long n_frames) {
    const size_t need = (size_t)(rs.tail_len + n_frames) * rs.channels * resample_format_bytes(rs.fmt);
    if (need <= rs.stage_cap) return WLX_OK;
    size_t cap = std::max<size_t>(rs.stage_cap, 64u << 10);
    while (cap < need) cap *= 2;
    unsigned char* nb = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&nb), cap) != hipSuccess) {          // replaces rs.stage, freed below: nothing of it is in flight between calls
        (void)hipGetLastError();
        return set_error(WLX_ERR_NOMEM, "stream resampler: %zu bytes of staging cannot be had", cap);
    }
    if (rs.stage) CK(hipFree(rs.stage));
    rs.stage = nb; rs.stage_cap = cap;
    return WLX_OK;
}

int resample_stream_enqueue(ResampleStream& rs, const void* frames, long long n_frames, int flush, float* d_dst, hipStream_t st,
                            long long lane_stride) {
    const size_t fb = (size_t)rs.channels * resample_format_bytes(rs.fmt);
    const long long tl = rs.tail_len, total = tl + n_frames;
    const long long n_new = resample_stream_next(rs, n_frames, flush);
    if (n_new > 0 || n_frames > 0) {
        if (tl > 0) CK(hipMemcpyAsync(rs.stage, rs.tail, (size_t)tl * fb, hipMemcpyDeviceToDevice, st));
        if (n_frames > 0) CK(hipMemcpyAsync(rs.stage + (size_t)tl * fb, frames, (size_t)n_frames * fb, hipMemcpyHostToDevice, st));
    }
    if (n_new > 0) {
        ResampleArgs p{};
        // the window [J - tail_len, J') of the stream; frames at and past J' read as zero, which only a flush's outputs reach
        p.raw = rs.stage; p.j_base = rs.J - tl; p.raw_frames = total; p.n_frames = rs.J + n_frames; p.channels = rs.channels;
        p.up = rs.pl.up; p.down = rs.pl.down; p.half_len = rs.pl.half_len; p.tile = rs.pl.tile; p.taps = rs.pl.taps;
        // the kernel writes out[m] at the absolute m: output M lands at d_dst (the pointer is rebased on the host, never read here)
        p.out = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(d_dst) - (uintptr_t)rs.M * sizeof(float));
        p.m0 = rs.M; p.m1 = rs.M + n_new;
        const unsigned grid = (unsigned)((n_new + rs.pl.tile - 1) / rs.pl.tile);
        // lane_stride > 0 (a ring group): the split instantiation, channel c's output M lands at d_dst + c * lane_stride
        rs_launch(rs.fmt, grid, rs_lds_bytes(rs.pl.up, rs.pl.down, rs.pl.half_len, rs.pl.tile), st, p, lane_stride);
        CK(hipGetLastError());
    }
    if (n_frames > 0) {                                     // the new tail: the last min(J', reach) frames of the window
        const long long keep = std::min(total, resample_reach(rs.pl));
        CK(hipMemcpyAsync(rs.tail, rs.stage + (size_t)(total - keep) * fb, (size_t)keep * fb, hipMemcpyDeviceToDevice, st));
        rs.tail_len = keep;
    }
    rs.J += n_frames; rs.M += n_new;
    if (flush) rs.closed = true;
    return WLX_OK;
}

void resample_stream_free(ResampleStream& rs) {
    if (rs.tail) (void)hipFree(rs.tail);
    if (rs.stage) (void)hipFree(rs.stage);
    rs.tail = rs.stage = nullptr; rs.stage_cap = 0; rs.tail_len = 0;
}

}  // namespace wlx

using namespace wlx;

// ------------------------------------------------------------------------------------------------ test hooks (host.h HookScope)
// split: out is [channels][cap] and channel c lands in row c (the split instantiation); else out is [cap] (the down-mix)
static int debug_resample(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format, int32_t sample_rate,
                          int64_t block_frames, float* out, int64_t cap, int64_t* n_out, float* kernel_ms, bool split = false) {
    if (!out || !n_out || cap < 0) return set_error(WLX_ERR_ARG, "null argument");
    CKR(resample_check_args(frames, n_frames, channels, sample_format, sample_rate));
    if (block_frames < 0) return set_error(WLX_ERR_ARG, "negative block size");
    int up, down, tile;
    CKR(resample_ratio(sample_rate, &up, &down, &tile));
    {   // reach and output length need no device either
        ResamplePlan tmp{}; tmp.up = up; tmp.down = down;
        tmp.half_len = up == down ? 0 : 10 * std::max(up, down);
        if (block_frames == 0) block_frames = resample_default_block(channels, sample_format);
        if (block_frames < resample_reach(tmp))
            return set_error(WLX_ERR_ARG, "block of %lld frames is smaller than the filter's reach (%lld)", (long long)block_frames, resample_reach(tmp));
        if (resample_out_len(tmp, n_frames) > cap) return set_error(WLX_ERR_ARG, "output buffer too small");
    }
    HookScope S;
    CKR(S.begin(device));
    ResamplePlan pl{};
    CKR(resample_plan(device, sample_rate, &pl));
    const long long nout = resample_out_len(pl, n_frames);
    *n_out = nout;
    if (nout == 0) return WLX_OK;
    const size_t fb = (size_t)channels * (size_t)resample_format_bytes(sample_format);
    const long long bf = std::min<long long>(block_frames, n_frames);
    ResampleStage sg{};
    unsigned char *r0 = nullptr, *r1 = nullptr;
    float* dout = nullptr;
    CKR(S.alloc(&r0, (size_t)bf * fb));
    CKR(S.alloc(&r1, (size_t)bf * fb));
    const size_t out_floats = (size_t)cap * (split ? (size_t)channels : 1);
    CKR(S.upload(&dout, out, out_floats));                  // copied in AND out
    sg.dev[0] = r0; sg.dev[1] = r1;
    CKR(resample_run(pl, frames, n_frames, channels, sample_format, block_frames, sg, dout, S.st, kernel_ms, split ? (long long)cap : 0));
    CKR(S.download(out, dout, out_floats));
    return S.finish();
}

extern "C" int32_t wlx_debug_resample(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                      int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out) {
    return debug_resample(device, frames, n_frames, channels, sample_format, sample_rate, block_frames, out, cap, n_out, nullptr);
}

extern "C" int32_t wlx_debug_resample_timed(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                            int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out,
                                            float* kernel_ms_out) {
    if (!kernel_ms_out) return set_error(WLX_ERR_ARG, "null argument");
    return debug_resample(device, frames, n_frames, channels, sample_format, sample_rate, block_frames, out, cap, n_out, kernel_ms_out);
}

extern "C" int32_t wlx_debug_resample_split(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                            int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out) {
    return debug_resample(device, frames, n_frames, channels, sample_format, sample_rate, block_frames, out, cap, n_out, nullptr, true);
}

// ------------------------------------------------------------------------------------------------ the stream form: planner and hook
extern "C" int32_t wlx_resample_stream_count(int32_t sample_rate, int64_t frames_seen, int32_t flush, int64_t* n_out) {
    if (!n_out) return set_error(WLX_ERR_ARG, "null argument");
    if (frames_seen < 0 || frames_seen > (1LL << 50)) return set_error(WLX_ERR_ARG, "frame count out of range");
    int up, down, tile;
    CKR(resample_ratio(sample_rate, &up, &down, &tile));
    *n_out = resample_stream_count(up, down, up == down ? 0 : 10 * std::max(up, down), frames_seen, flush);
    return WLX_OK;
}

extern "C" int32_t wlx_debug_resample_stream(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                             int32_t sample_rate, const int64_t* cuts, int32_t n_cuts, int32_t flush, float* out,
                                             int64_t cap, int64_t* n_out, int64_t* per_call_counts) {
    if (!out || !n_out || cap < 0 || n_cuts < 0 || (n_cuts > 0 && !cuts) || flush < 0 || flush > 2) return set_error(WLX_ERR_ARG, "bad argument");
    if (n_frames < 0 || n_frames > (1LL << 50)) return set_error(WLX_ERR_ARG, "frame count out of range");
    if (n_frames > 0 && !frames) return set_error(WLX_ERR_ARG, "null frames");
    CKR(resample_stream_check(sample_format, channels, sample_rate));
    for (int i = 0; i < n_cuts; ++i)
        if (cuts[i] < (i ? cuts[i - 1] : 0) || cuts[i] > n_frames) return set_error(WLX_ERR_ARG, "cut %d = %lld is out of order or past the end", i, (long long)cuts[i]);
    int up, down, tile;
    CKR(resample_ratio(sample_rate, &up, &down, &tile));
    const long long total = resample_stream_count(up, down, up == down ? 0 : 10 * std::max(up, down), n_frames, flush);
    if (total > cap) return set_error(WLX_ERR_ARG, "output buffer too small");
    HookScope S;
    CKR(S.begin(device));
    // the stream state is owned by name (resample_stream_free), released behind the stream's work and before S lets go of the rest
    struct Owner {
        HookScope& S; ResampleStream rs{};
        ~Owner() { (void)hipStreamSynchronize(S.st); resample_stream_free(rs); }
    } R{S};
    ResampleStream& rs = R.rs;
    CKR(resample_stream_open(device, sample_format, channels, sample_rate, &rs));
    float* dout = nullptr;
    CKR(S.upload(&dout, out, (size_t)cap));                  // copied in AND out (cap == 0: one float nobody reads)
    const size_t fb = (size_t)channels * resample_format_bytes(sample_format);
    const int n_calls = n_cuts + 1 + (flush == 1 ? 1 : 0);
    for (int c = 0; c < n_calls; ++c) {
        const bool tail_call = c == n_cuts + 1;              // flush == 1: the empty flushing packet behind the data
        const long long a = tail_call ? n_frames : (c ? cuts[c - 1] : 0), b = tail_call ? n_frames : (c < n_cuts ? cuts[c] : n_frames);
        const int fl = tail_call || (flush == 2 && c == n_cuts);
        const long long before = rs.M;
        CKR(resample_stream_reserve(rs, b - a));
        CKR(resample_stream_enqueue(rs, static_cast<const char*>(frames) + (size_t)a * fb, b - a, fl, dout + before, S.st));
        CK(hipStreamSynchronize(S.st));                      // as the product call: a packet is done when its call returns
        if (per_call_counts) per_call_counts[c] = rs.M - before;
    }
    CKR(S.download(out, dout, (size_t)cap));
    CKR(S.finish());
    *n_out = rs.M;
    return WLX_OK;
}
