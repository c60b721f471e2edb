// put_many.hip — a WAVE of files into consecutive slot items in one call (include/wlx.h wlx_pcm_put_many; test hooks
// wlx_debug_resample_many, wlx_debug_flac_decode_many, wlx_debug_put_many_budget): every upload and every launch of the call is
// enqueued on the slot's stream, the host waits ONCE, then reads the FLAC status words. The number of launches depends on which kinds
// of entry are present, never on how many there are (one ADPCM decode launch per ADPCM file aside: adpcm.hip's own, which takes no wait).
//
// Each entry keeps the contract of the single-file entry point of its kind, bit for bit:
//   resample_many_kernel     the ragged form of resample_kernel's down-mix instantiation (resample.hip). A device table holds one record
//                            per entry (RsManyEnt); workgroup b finds its entry as the last one whose first tile is <= b, and from there
//                            runs resample_kernel's body statement for statement: the same span, the same staging loop with the same
//                            conversions (resample_core.h rs_sample, switched at run time), the same fmaf chain over k ascending. An
//                            output depends on nothing but absolute input indices, so which workgroup of which launch computes it
//                            cannot move a bit. Dynamic LDS = the largest need among the launch's entries.
//   flac_frames_many_kernel  one LANE per frame over the concatenated frame tables of all FLAC entries of the sub-batch: the frame
//                            names its entry (FlacFrame::pad), the entry's record (FlacManyEnt) its width, channels and planes; the
//                            decoder is flac_core.h's flac_decode_frame, as in flac_frames_kernel. The frames of 24 voicemail files
//                            fill the waves one file's 80 frames cannot.
//   flac_finish_many_kernel  flac_finish_kernel per frame with the entry's record: stereo undone, scaled, interleaved; zeros for a
//                            frame that failed.
// G.711 code bytes and WLX_PUT_FRAMES frames are the ragged resampler's input as they are; an ADPCM file is decoded by adpcm_launch.
//
// Scratch: ONE device block, the slot's (Slot::flac), laid out per sub-batch as
//   [resample records | FLAC entry records | FLAC frame table | every entry's input bytes]  <- uploaded as one contiguous image
//   [status words | per entry: int32 planes, float32 frames]
// Entries whose needs (put_many_plan.h) do not fit the budget together run as consecutive sub-batches that reuse the block in stream
// order; the status words of each sub-batch are copied to pinned host memory behind its launches, still without a wait.
#include <atomic>
#include <cmath>
#include <cstring>
#include <type_traits>
#include "engine.h"
#include "flac_core.h"
#include "frontend.h"
#include "put_many_plan.h"
#include "resample_core.h"

namespace wlx {

static_assert(WLX_PUT_MANY_MAX == 64, "the entry search of resample_many_kernel is sized for a short table");

struct RsManyEnt {
    const void* raw;            // interleaved frames [0, n_frames) of the entry, in its format (device)
    long long n_frames, n_out;
    int channels, fmt;
    int up, down, half_len, tile;
    const float* taps;          // [2 * half_len + 1]
    float* out;                 // out[m] for m in [0, n_out)
    int first_tile, pad;        // the entry owns workgroups [first_tile, next entry's first_tile)
};

struct FlacManyEnt {
    long long planes_base, plane_stride;    // int32 elements from the planes pointer; samples per plane
    long long out_base;                     // elements from the output pointer: the entry's [total][channels]
    int bps, channels;
    float scale;
    int pad;
};

__device__ __forceinline__ float rs_sample_rt(int fmt, const void* raw, long long idx) {
    switch (fmt) {
    case WLX_PCM_S16: return rs_sample<WLX_PCM_S16>(raw, idx);
    case WLX_PCM_U8: return rs_sample<WLX_PCM_U8>(raw, idx);
    case WLX_PCM_MULAW: return rs_sample<WLX_PCM_MULAW>(raw, idx);
    case WLX_PCM_ALAW: return rs_sample<WLX_PCM_ALAW>(raw, idx);
    default: return rs_sample<WLX_PCM_F32>(raw, idx);
    }
}

// lds_floats: the launch's dynamic LDS; a record whose tile would not fit it is skipped (the host never builds one)
__global__ __launch_bounds__(RS_THREADS) void resample_many_kernel(const RsManyEnt* __restrict__ tab, int n_ent, int lds_floats) {
    extern __shared__ float rsm_lds[];
    int e = 0;
    for (int i = 1; i < n_ent; ++i)
        if (tab[i].first_tile <= (int)blockIdx.x) e = i;
    const RsManyEnt p = tab[e];
    const long long tix = (long long)blockIdx.x - p.first_tile;
    if (tix < 0 || p.tile < 1 || p.up < 1 || p.down < 1 || p.half_len < 0 || p.channels < 1) return;
    const int ntaps = 2 * p.half_len + 1;
    float* hs = rsm_lds;
    float* xs = rsm_lds + ntaps;
    const long long mA = tix * p.tile;
    if (mA >= p.n_out) return;
    const long long mB = mA + p.tile < p.n_out ? mA + p.tile : p.n_out;
    // the input span of the tile: j with 0 <= half_len + m * down - j * up <= 2 * half_len for some m in [mA, mB)
    const long long j_lo = -floor_div(-(mA * p.down - p.half_len), p.up);          // ceil((mA * down - half_len) / up)
    const long long j_hi = floor_div((long long)p.half_len + (mB - 1) * p.down, p.up);
    if (j_hi - j_lo + 1 < 0 || j_hi - j_lo + 1 + ntaps > (long long)lds_floats) return;
    const int span = (int)(j_hi - j_lo + 1);
    for (int i = threadIdx.x; i < ntaps; i += RS_THREADS) hs[i] = p.taps[i];
    const int ch = p.channels;
    const float fch = (float)ch;
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long j = j_lo + i;
        float v = 0.f;
        if (j >= 0 && j < p.n_frames) {
            const long long b = j * ch;
            v = rs_sample_rt(p.fmt, p.raw, b);
            if (ch > 1) {                                    // the float32 mean: channels added in order, one division
                for (int c = 1; c < ch; ++c) v += rs_sample_rt(p.fmt, p.raw, b + c);
                v = v / fch;
            }
        }
        xs[i] = v;
    }
    __syncthreads();
    float* out = p.out;
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

constexpr int FLACM_FRAMES_THREADS = 64;     // one wave: 64 frames, of whichever entries
constexpr int FLACM_FINISH_THREADS = 256;

// status word of a frame: flac_core.h status in the low byte, the channel assignment the finish kernel has to undo above it
__global__ __launch_bounds__(FLACM_FRAMES_THREADS) void flac_frames_many_kernel(const uint8_t* __restrict__ bytes, const FlacFrame* __restrict__ tab,
                                                                                int n_frames, const FlacManyEnt* __restrict__ ents, int n_ent,
                                                                                int32_t* __restrict__ planes, int* __restrict__ status) {
    const int f = blockIdx.x * FLACM_FRAMES_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const FlacFrame t = tab[f];
    if ((unsigned)t.pad >= (unsigned)n_ent) { status[f] = FLAC_E_PARTITION; return; }
    const FlacManyEnt en = ents[t.pad];
    int assign = 0;
    const int rc = flac_decode_frame(bytes, t.start, t.end, en.bps, en.channels, t.n, planes + en.planes_base + t.first, en.plane_stride, &assign);
    status[f] = rc | (assign << 8);
}

// T = float: sample * scale, the front end's frames. T = int32_t: the integers themselves (wlx_debug_flac_decode_many). A frame whose
// status is not FLAC_OK stores zeros (its planes hold whatever the decoder had written when it stopped).
template <class T>
__global__ __launch_bounds__(FLACM_FINISH_THREADS) void flac_finish_many_kernel(const FlacFrame* __restrict__ tab, const int* __restrict__ status,
                                                                                const FlacManyEnt* __restrict__ ents, int n_ent,
                                                                                const int32_t* __restrict__ planes_all, T* __restrict__ out_all) {
    const FlacFrame t = tab[blockIdx.x];
    if ((unsigned)t.pad >= (unsigned)n_ent) return;
    const FlacManyEnt en = ents[t.pad];
    const int st = status[blockIdx.x];
    const bool ok = (st & 0xFF) == FLAC_OK;
    const int assign = st >> 8;
    const int channels = en.channels;
    const long long plane_stride = en.plane_stride;
    const int32_t* planes = planes_all + en.planes_base;
    T* out = out_all + en.out_base;
    const float scale = en.scale;
    for (int i = threadIdx.x; i < t.n; i += FLACM_FINISH_THREADS) {
        const long long j = t.first + i;
        T* o = out + j * channels;
        if (!ok) {
            for (int c = 0; c < channels; ++c) o[c] = (T)0;
        } else if (assign != FLAC_CH_INDEPENDENT) {          // two channels by construction (flac_decode_frame)
            int32_t l, r;
            flac_stereo(assign, planes[j], planes[plane_stride + j], &l, &r);
            o[0] = std::is_same<T, float>::value ? (T)((float)l * scale) : (T)l;
            o[1] = std::is_same<T, float>::value ? (T)((float)r * scale) : (T)r;
        } else {
            for (int c = 0; c < channels; ++c) {
                const int32_t v = planes[(long long)c * plane_stride + j];
                o[c] = std::is_same<T, float>::value ? (T)((float)v * scale) : (T)v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches (no wait)
static int rs_many_launch(const RsManyEnt* d_tab, int n_ent, long long grid, size_t lds, hipStream_t st) {
    if (grid <= 0) return WLX_OK;
    hipLaunchKernelGGL(resample_many_kernel, dim3((unsigned)grid), dim3(RS_THREADS), lds, st, d_tab, n_ent, (int)(lds / sizeof(float)));
    CK(hipGetLastError());
    return WLX_OK;
}

template <class T>
static int flac_many_launch(const uint8_t* d_bytes, const FlacFrame* d_tab, int nf, const FlacManyEnt* d_ents, int n_ent, int32_t* d_planes,
                            int* d_status, T* d_out, hipStream_t st) {
    if (nf <= 0) return WLX_OK;
    hipLaunchKernelGGL(flac_frames_many_kernel, dim3((unsigned)((nf + FLACM_FRAMES_THREADS - 1) / FLACM_FRAMES_THREADS)), dim3(FLACM_FRAMES_THREADS),
                       0, st, d_bytes, d_tab, nf, d_ents, n_ent, d_planes, d_status);
    CK(hipGetLastError());
    hipLaunchKernelGGL(flac_finish_many_kernel<T>, dim3((unsigned)nf), dim3(FLACM_FINISH_THREADS), 0, st, d_tab, d_status, d_ents, n_ent,
                       static_cast<const int32_t*>(d_planes), d_out);
    CK(hipGetLastError());
    return WLX_OK;
}

static RsManyEnt rs_ent(const ResamplePlan& pl, const void* raw, long long n_frames, int channels, int fmt, float* out) {
    RsManyEnt r{};
    r.raw = raw; r.n_frames = n_frames; r.n_out = resample_out_len(pl, n_frames); r.channels = channels; r.fmt = fmt;
    r.up = pl.up; r.down = pl.down; r.half_len = pl.half_len; r.tile = pl.tile; r.taps = pl.taps; r.out = out;
    return r;
}

// first tiles and the launch's LDS for the records of one launch -> the grid (WLX_ERR_ARG past 2^31 - 1 workgroups)
static int rs_many_shape(std::vector<RsManyEnt>& recs, long long* grid, size_t* lds) {
    std::vector<long long> n_out;
    std::vector<int> tile, first;
    *lds = 0;
    for (const RsManyEnt& r : recs) {
        n_out.push_back(r.n_out);
        tile.push_back(r.tile);
        *lds = std::max(*lds, rs_lds_bytes(r.up, r.down, r.half_len, r.tile));
    }
    *grid = put_many_tiles(n_out, tile, first);
    if (*grid < 0) return set_error(WLX_ERR_ARG, "the ragged resample launch would need more than 2^31 - 1 workgroups");
    for (size_t k = 0; k < recs.size(); ++k) recs[k].first_tile = first[k];
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ the product call
static std::atomic<size_t> g_put_many_budget{PUT_MANY_BUDGET};
static std::atomic<int> g_put_many_last_batches{0};      // sub-batches of the last call that enqueued anything (the budget hook reports it)

struct PmEntry {
    int kind = 0;
    bool live = false;              // passed every host check: takes part in the launches
    long long n_out = 0;            // samples at 16 kHz
    int fmt = WLX_PCM_F32, channels = 1;
    long long n_frames = 0;         // the resampler's input frames
    ResamplePlan pl{};
    const void* src = nullptr;      // what goes up: PCM samples, frames, the FLAC file, the WAV data chunk
    size_t src_bytes = 0;
    bool flac = false, adpcm = false;
    FlacStream fs;
    WavStream ws;
    size_t need = 0;
    size_t in_off = 0, planes_off = 0, frames_off = 0;      // placement in the scratch of the entry's sub-batch
    size_t status_at = 0;           // FLAC: its first status word in the call's host copy
};

struct Piece { size_t off; const void* src; size_t n; };

// pieces (ascending, disjoint offsets from `base`) -> device, as ONE contiguous image of `bytes` bytes through the slot's pinned halves:
// staged_upload's protocol (flac.hip), so the two interleave on one block counter. The gaps between pieces carry whatever the pinned
// half held: they are the 256-byte padding of the layout, which nothing reads.
static int upload_image(ResampleStage* sg, int* blk, unsigned char* base, const std::vector<Piece>& pieces, size_t bytes, hipStream_t st) {
    for (size_t b0 = 0; b0 < bytes; b0 += RS_BLOCK_BYTES, ++*blk) {
        const size_t len = std::min(bytes - b0, (size_t)RS_BLOCK_BYTES);
        const int b = *blk & 1;
        if (sg->used[b]) CK(hipEventSynchronize(sg->copied[b]));      // the pinned half is free once the copy out of it (two blocks ago) has run
        for (const Piece& p : pieces) {
            const size_t lo = std::max(p.off, b0), hi = std::min(p.off + p.n, b0 + len);
            if (lo < hi) std::memcpy(sg->pinned[b] + (lo - b0), static_cast<const char*>(p.src) + (lo - p.off), hi - lo);
        }
        CK(hipMemcpyAsync(base + b0, sg->pinned[b], len, hipMemcpyHostToDevice, st));
        CK(hipEventRecord(sg->copied[b], st));
        sg->used[b] = true;
    }
    return WLX_OK;
}

// the host checks of one entry: everything the single-file entry point of its kind answers before any launch. -> the entry's status
static int pm_probe(Engine* e, const wlx_put_entry& in, PmEntry& x) {
    x.kind = in.kind;
    if (!in.data || in.n <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    int rate = 16000;
    switch (in.kind) {
    case WLX_PUT_PCM:
        if (in.n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
        x.src = in.data; x.src_bytes = (size_t)in.n * sizeof(float); x.n_out = in.n;
        return WLX_OK;
    case WLX_PUT_FRAMES:
        CKR(resample_check_args(in.data, in.n, in.channels, in.sample_format, in.sample_rate));
        if (in.n > (int64_t)in.sample_rate * 3600 + in.sample_rate) return set_error(WLX_ERR_ARG, "audio chunk too long");
        rate = in.sample_rate; x.fmt = in.sample_format; x.channels = in.channels; x.n_frames = in.n;
        x.src = in.data; x.src_bytes = (size_t)in.n * (size_t)in.channels * (size_t)resample_format_bytes(in.sample_format);
        break;
    case WLX_PUT_FLAC:
        CKR(flac_index(static_cast<const uint8_t*>(in.data), in.n, x.fs));
        CKR(flac_served(x.fs));
        rate = x.fs.info.sample_rate; x.fmt = WLX_PCM_F32; x.channels = x.fs.info.channels; x.n_frames = x.fs.info.total_samples;
        x.src = in.data; x.src_bytes = (size_t)in.n; x.flac = true;
        break;
    case WLX_PUT_WAV: {
        CKR(wav_index(static_cast<const uint8_t*>(in.data), in.n, x.ws));
        CKR(wav_served(x.ws));
        const wlx_wav_info& wi = x.ws.info;
        rate = wi.sample_rate; x.channels = wi.channels; x.n_frames = wi.n_frames;
        x.src = static_cast<const uint8_t*>(in.data) + wi.data_offset;
        x.adpcm = x.ws.kind >= 0;
        if (x.adpcm) {
            x.fmt = WLX_PCM_F32;
            x.src_bytes = (size_t)adpcm_blocks(x.ws) * (size_t)wi.block_align;
        } else {
            x.fmt = wi.format_tag == WAV_TAG_MULAW ? WLX_PCM_MULAW : WLX_PCM_ALAW;
            x.src_bytes = (size_t)wi.n_frames * (size_t)wi.channels;
        }
        break;
    }
    default:
        return set_error(WLX_ERR_ARG, "unknown entry kind %d", in.kind);
    }
    CKR(resample_plan(e->device, rate, &x.pl));
    x.n_out = resample_out_len(x.pl, x.n_frames);
    if (x.n_out > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    // the entry's share of a sub-batch's scratch: its resample record, its input bytes, and what its decoder works in
    const size_t ns = (size_t)x.n_frames * (size_t)x.channels;
    x.need = 256 + pm_up256(x.src_bytes);
    if (x.adpcm) x.need += pm_up256(ns * sizeof(float));
    if (x.flac) {
        const size_t nf = x.fs.frames.size();
        x.need += 256 + pm_up256(nf * sizeof(FlacFrame)) + pm_up256(nf * sizeof(int)) + 2 * pm_up256(ns * 4);
    }
    return WLX_OK;
}

// one sub-batch on the slot's stream: image upload, FLAC decode + finish, ADPCM decodes, the ragged resample, the status copy. No wait.
static int pm_enqueue(Slot* s, std::vector<PmEntry>& X, int first_item, const PutBatch& bt, int* blk, int* h_status) {
    unsigned char* base = s->flac.buf;
    std::vector<int> rs_of, flac_of;                      // entries with a resample record / a FLAC record, in order
    size_t n_frames_tab = 0;
    for (int k = bt.first; k < bt.last; ++k) {
        if (!X[(size_t)k].live) continue;
        if (X[(size_t)k].kind != WLX_PUT_PCM) rs_of.push_back(k);
        if (X[(size_t)k].flac) { flac_of.push_back(k); n_frames_tab += X[(size_t)k].fs.frames.size(); }
    }
    // ---- layout: the uploaded zone, then the work zone
    size_t o = 0;
    const size_t rs_off = o; o += pm_up256(rs_of.size() * sizeof(RsManyEnt));
    const size_t fe_off = o; o += pm_up256(flac_of.size() * sizeof(FlacManyEnt));
    const size_t tab_off = o; o += pm_up256(n_frames_tab * sizeof(FlacFrame));
    for (int k : rs_of) { X[(size_t)k].in_off = o; o += pm_up256(X[(size_t)k].src_bytes); }
    const size_t image_bytes = o;
    const size_t st_off = o; o += pm_up256(n_frames_tab * sizeof(int));
    for (int k : rs_of) {
        PmEntry& x = X[(size_t)k];
        const size_t ns = (size_t)x.n_frames * (size_t)x.channels;
        if (x.flac) { x.planes_off = o; o += pm_up256(ns * 4); }
        if (x.flac || x.adpcm) { x.frames_off = o; o += pm_up256(ns * 4); }
    }
    if (o > s->flac.cap) return set_error(WLX_ERR_STATE, "wlx_pcm_put_many: a sub-batch of %zu bytes in a scratch of %zu", o, s->flac.cap);
    // ---- the tables
    std::vector<RsManyEnt> recs;
    std::vector<FlacManyEnt> fents;
    std::vector<FlacFrame> tab;
    tab.reserve(n_frames_tab);
    for (int k : rs_of) {
        PmEntry& x = X[(size_t)k];
        const void* raw = (x.flac || x.adpcm) ? base + x.frames_off : base + x.in_off;
        recs.push_back(rs_ent(x.pl, raw, x.n_frames, x.channels, x.fmt, s->pcm + (size_t)(first_item + k) * s->pcm_cap));
    }
    long long grid = 0;
    size_t lds = 0;
    CKR(rs_many_shape(recs, &grid, &lds));
    for (int k : flac_of) {
        PmEntry& x = X[(size_t)k];
        FlacManyEnt fe{};
        fe.planes_base = (long long)(x.planes_off / 4); fe.plane_stride = x.fs.info.total_samples; fe.out_base = (long long)(x.frames_off / 4);
        fe.bps = x.fs.info.bits_per_sample; fe.channels = x.fs.info.channels; fe.scale = std::ldexp(1.0f, -(x.fs.info.bits_per_sample - 1));
        for (FlacFrame f : x.fs.frames) {
            f.start += (long long)x.in_off; f.end += (long long)x.in_off; f.pad = (int)fents.size();
            tab.push_back(f);
        }
        fents.push_back(fe);
    }
    // ---- uploads: the waveforms straight into their items, everything else as one image
    for (int k = bt.first; k < bt.last; ++k) {
        PmEntry& x = X[(size_t)k];
        if (x.live && x.kind == WLX_PUT_PCM)
            CKR(staged_upload(&s->rs, blk, s->pcm + (size_t)(first_item + k) * s->pcm_cap, x.src, x.src_bytes, s->stream));
    }
    if (!rs_of.empty()) {
        std::vector<Piece> pieces;
        pieces.push_back(Piece{rs_off, recs.data(), recs.size() * sizeof(RsManyEnt)});
        if (!fents.empty()) pieces.push_back(Piece{fe_off, fents.data(), fents.size() * sizeof(FlacManyEnt)});
        if (!tab.empty()) pieces.push_back(Piece{tab_off, tab.data(), tab.size() * sizeof(FlacFrame)});
        for (int k : rs_of) pieces.push_back(Piece{X[(size_t)k].in_off, X[(size_t)k].src, X[(size_t)k].src_bytes});
        CKR(upload_image(&s->rs, blk, base, pieces, image_bytes, s->stream));
    }
    // ---- launches
    if (!tab.empty()) {
        CKR(flac_many_launch<float>(base, reinterpret_cast<const FlacFrame*>(base + tab_off), (int)tab.size(),
                                    reinterpret_cast<const FlacManyEnt*>(base + fe_off), (int)fents.size(), reinterpret_cast<int32_t*>(base),
                                    reinterpret_cast<int*>(base + st_off), reinterpret_cast<float*>(base), s->stream));
        size_t at = X[(size_t)flac_of[0]].status_at;
        CK(hipMemcpyAsync(h_status + at, base + st_off, tab.size() * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    }
    for (int k : rs_of) {
        PmEntry& x = X[(size_t)k];
        if (x.adpcm) CKR(adpcm_launch_f32(x.ws, base + x.in_off, reinterpret_cast<float*>(base + x.frames_off), s->stream));
    }
    if (!rs_of.empty()) CKR(rs_many_launch(reinterpret_cast<const RsManyEnt*>(base + rs_off), (int)recs.size(), grid, lds, s->stream));
    return WLX_OK;
}

}  // namespace wlx

using namespace wlx;

extern "C" int32_t wlx_pcm_put_many(wlx_engine* e, int32_t slot, int32_t first_item, int32_t n, const wlx_put_entry* entries,
                                    wlx_put_result* results) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!entries || !results) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_PUT_MANY_MAX) return set_error(WLX_ERR_ARG, "wlx_pcm_put_many: %d entries outside 1..%d", n, WLX_PUT_MANY_MAX);
    if (first_item < 0 || (long long)first_item + n > s->B)
        return set_error(WLX_ERR_ARG, "wlx_pcm_put_many: items [%d, %lld) outside the slot's %d", first_item, (long long)first_item + n, s->B);
    CK(hipSetDevice(e->device));
    // ---- host: everything that can refuse an entry, before any launch and before any item's PCM is touched
    std::vector<PmEntry> X((size_t)n);
    std::vector<size_t> need((size_t)n, 0);
    std::vector<char> live((size_t)n, 0), over;
    for (int k = 0; k < n; ++k) {
        results[k].status = pm_probe(e, entries[k], X[(size_t)k]);
        results[k].n_out = 0;
        if (results[k].status == WLX_ERR_HIP || results[k].status == WLX_ERR_NOMEM) return results[k].status;    // (the tap table of a new ratio)
        live[(size_t)k] = results[k].status == WLX_OK;
        need[(size_t)k] = X[(size_t)k].need;
    }
    const size_t budget = g_put_many_budget.load();
    const std::vector<PutBatch> batches = put_many_pack(need, live, budget, over);
    size_t scratch = 0, longest = 0, n_status = 0;
    for (const PutBatch& b : batches) scratch = std::max(scratch, b.bytes);
    bool recorded = false, any = false;
    for (int k = 0; k < n; ++k) {
        PmEntry& x = X[(size_t)k];
        if (over[(size_t)k]) {
            live[(size_t)k] = 0;
            results[k].status = set_error(WLX_ERR_ARG, "wlx_pcm_put_many: entry %d needs %zu bytes of scratch by itself, the budget is %zu: "
                                          "put it alone", k, x.need, budget);
        }
        x.live = live[(size_t)k] != 0;
        if (!x.live) continue;
        any = true;
        longest = std::max(longest, (size_t)x.n_out);
        recorded = recorded || std::find(s->lm_items.begin(), s->lm_items.end(), first_item + k) != s->lm_items.end();
        if (x.flac) { x.status_at = n_status; n_status += x.fs.frames.size(); }
    }
    if (!any) return WLX_OK;
    if (scratch > s->flac.cap) {                // grown before anything else changes: a refusal leaves the slot as it was
        unsigned char* nb = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&nb), scratch) != hipSuccess) {
            (void)hipGetLastError();
            return set_error(WLX_ERR_NOMEM, "wlx_pcm_put_many: scratch of %zu bytes (file bytes, frame tables, int32 planes, float32 frames) cannot be had", scratch);
        }
        CK(hipStreamSynchronize(s->stream));
        if (s->flac.buf) (void)hipFree(s->flac.buf);
        s->flac.buf = nb; s->flac.cap = scratch;
    }
    if (n_status > s->h_put_status_cap) {       // pinned, for the slot's life: the status words come back without a wait
        size_t cap = std::max<size_t>(s->h_put_status_cap, 64u << 10);
        while (cap < n_status) cap *= 2;
        int* nb = nullptr;
        CKR(halloc(s->host_allocs, &nb, cap));
        s->h_put_status = nb; s->h_put_status_cap = cap;
    }
    CKR(slot_resample_stage(s));
    if (longest > s->pcm_cap || recorded)
        CKR(flush_logmel(e, s));                // a recorded log-mel request reads a target item's PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, longest));
    // ---- device: every sub-batch behind the other on the slot's stream; one wait
    for (int k = 0; k < n; ++k)
        if (X[(size_t)k].live) s->npcm[first_item + k] = 0;      // (a failed run leaves no half-written audio resident)
    int blk = 0;
    int rc = WLX_OK;
    g_put_many_last_batches.store((int)batches.size());
    for (size_t b = 0; b < batches.size() && rc == WLX_OK; ++b) rc = pm_enqueue(s, X, first_item, batches[b], &blk, s->h_put_status);
    hipError_t he = hipStreamSynchronize(s->stream);       // the caller's memory and the staging halves may be reused after return
    s->rs.used[0] = s->rs.used[1] = false;
    if (rc == WLX_OK && he != hipSuccess) rc = set_error(WLX_ERR_HIP, "wlx_pcm_put_many: %s", hipGetErrorString(he));
    if (s->flac.cap > 2 * RS_BLOCK_BYTES) {                // a wave's scratch does not stay with the slot
        (void)hipFree(s->flac.buf);
        s->flac.buf = nullptr; s->flac.cap = 0;
    }
    if (rc != WLX_OK) {
        for (int k = 0; k < n; ++k) s->npcm[first_item + k] = 0;      // the call's error: no item of the call keeps PCM
        return rc;
    }
    for (int k = 0; k < n; ++k) {
        PmEntry& x = X[(size_t)k];
        if (!x.live) continue;
        if (x.flac) {
            const long long bad = put_many_first_bad(s->h_put_status + x.status_at, x.fs.frames.size());
            if (bad >= 0) {
                results[k].status = set_error(WLX_ERR_DATA, "FLAC (entry %d): frame %lld does not decode (status %d: 1 past its end, 2 reserved code, "
                                              "3 inconsistent partition / header, 4 does not end at its CRC, 5 unsupported width)", k, bad,
                                              s->h_put_status[x.status_at + (size_t)bad] & 0xFF);
                continue;
            }
        }
        s->npcm[first_item + k] = x.n_out;
        results[k].n_out = x.n_out;
    }
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ test hooks (host.h HookScope)
extern "C" int32_t wlx_debug_put_many_budget(int64_t bytes, int64_t* previous, int32_t* last_sub_batches) {
    if (bytes > 0 && (size_t)bytes < PUT_MANY_MIN_BUDGET) return set_error(WLX_ERR_ARG, "a budget under %zu bytes", PUT_MANY_MIN_BUDGET);
    const size_t old = bytes == 0 ? g_put_many_budget.load() : g_put_many_budget.exchange(bytes > 0 ? (size_t)bytes : PUT_MANY_BUDGET);
    if (previous) *previous = (int64_t)old;
    if (last_sub_batches) *last_sub_batches = g_put_many_last_batches.load();
    return WLX_OK;
}

extern "C" int32_t wlx_debug_resample_many(int32_t device, int32_t n, const void* const* frames, const int64_t* n_frames, const int32_t* channels,
                                           const int32_t* sample_formats, const int32_t* sample_rates, float* out, const int64_t* out_off,
                                           int64_t cap, int64_t* n_out) {
    if (!frames || !n_frames || !channels || !sample_formats || !sample_rates || !out || !out_off || !n_out || cap < 0)
        return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_PUT_MANY_MAX) return set_error(WLX_ERR_ARG, "%d entries outside 1..%d", n, WLX_PUT_MANY_MAX);
    for (int k = 0; k < n; ++k) {
        CKR(resample_stream_check(sample_formats[k], channels[k], sample_rates[k]));
        if (n_frames[k] < 0 || n_frames[k] > (1LL << 31)) return set_error(WLX_ERR_ARG, "entry %d: frame count out of range", k);
        if (n_frames[k] > 0 && !frames[k]) return set_error(WLX_ERR_ARG, "entry %d: null frames", k);
        int up, down, tile;
        CKR(resample_ratio(sample_rates[k], &up, &down, &tile));
        const long long no = (n_frames[k] * up + down - 1) / down;
        if (out_off[k] < 0 || out_off[k] > cap || no > cap - out_off[k]) return set_error(WLX_ERR_ARG, "entry %d: output outside the buffer", k);
    }
    std::vector<RsManyEnt> recs;                             // (declared before S: it outlives the stream's copy out of it on every return path)
    HookScope S;
    CKR(S.begin(device));
    float* dout = nullptr;
    CKR(S.upload(&dout, out, (size_t)cap));                  // copied in AND out
    for (int k = 0; k < n; ++k) {
        ResamplePlan pl{};
        CKR(resample_plan(device, sample_rates[k], &pl));
        unsigned char* raw = nullptr;
        const size_t nb = (size_t)n_frames[k] * (size_t)channels[k] * (size_t)resample_format_bytes(sample_formats[k]);
        CKR(S.upload(&raw, static_cast<const unsigned char*>(frames[k]), nb));
        recs.push_back(rs_ent(pl, raw, n_frames[k], channels[k], sample_formats[k], dout + out_off[k]));
        n_out[k] = recs.back().n_out;
    }
    long long grid = 0;
    size_t lds = 0;
    CKR(rs_many_shape(recs, &grid, &lds));
    RsManyEnt* dtab = nullptr;
    CKR(S.upload(&dtab, recs.data(), recs.size()));
    CKR(rs_many_launch(dtab, n, grid, lds, S.st));
    CKR(S.download(out, dout, (size_t)cap));
    return S.finish();
}

extern "C" int32_t wlx_debug_flac_decode_many(int32_t device, int32_t n, const void* const* bytes, const int64_t* n_bytes, int32_t* samples_out,
                                              const int64_t* out_off, int64_t cap_samples, int64_t* n_frames_out, int32_t* channels_out,
                                              int32_t* status_out) {
    if (!bytes || !n_bytes || !samples_out || !out_off || !n_frames_out || !channels_out || !status_out || cap_samples < 0)
        return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_PUT_MANY_MAX) return set_error(WLX_ERR_ARG, "%d entries outside 1..%d", n, WLX_PUT_MANY_MAX);
    std::vector<FlacStream> fs((size_t)n);
    std::vector<FlacFrame> tab;
    std::vector<FlacManyEnt> fents;
    std::vector<size_t> in_off((size_t)n), first_frame((size_t)n);
    size_t o = 0, planes = 0;
    for (int k = 0; k < n; ++k) {
        if (!bytes[k] || n_bytes[k] <= 0) return set_error(WLX_ERR_ARG, "entry %d: empty", k);
        CKR(flac_index(static_cast<const uint8_t*>(bytes[k]), n_bytes[k], fs[(size_t)k]));
        const wlx_flac_info& fi = fs[(size_t)k].info;
        // the hook decodes what the core decodes: any rate, <= 24 bits, <= 8 channels
        if (fi.channels > FLAC_MAX_CHANNELS || fi.bits_per_sample > FLAC_MAX_BPS || fi.total_samples <= 0)
            return set_error(WLX_ERR_ARG, "entry %d: FLAC stream of %d channels x %d bits, %lld samples: outside the decoder's scope", k, fi.channels,
                             fi.bits_per_sample, (long long)fi.total_samples);
        const long long ns = (long long)fi.total_samples * fi.channels;
        if (out_off[k] < 0 || out_off[k] > cap_samples || ns > cap_samples - out_off[k]) return set_error(WLX_ERR_ARG, "entry %d: output outside the buffer", k);
        in_off[(size_t)k] = o; o += pm_up256((size_t)n_bytes[k]);
        FlacManyEnt fe{};
        fe.planes_base = (long long)planes; fe.plane_stride = fi.total_samples; fe.out_base = out_off[k];
        fe.bps = fi.bits_per_sample; fe.channels = fi.channels; fe.scale = 1.0f;
        planes += (size_t)ns;
        first_frame[(size_t)k] = tab.size();
        for (FlacFrame f : fs[(size_t)k].frames) {
            f.start += (long long)in_off[(size_t)k]; f.end += (long long)in_off[(size_t)k]; f.pad = k;
            tab.push_back(f);
        }
        fents.push_back(fe);
        if (tab.size() >= 0x7FFFFFFFu / 2) return set_error(WLX_ERR_ARG, "too many frames");
    }
    std::vector<int> status(tab.size());                 // (declared before S: it outlives the stream's copies on every return path)
    HookScope S;
    CKR(S.begin(device));
    unsigned char* d_bytes = nullptr;
    CKR(S.alloc(&d_bytes, o));
    for (int k = 0; k < n; ++k)
        CK(hipMemcpyAsync(d_bytes + in_off[(size_t)k], bytes[k], (size_t)n_bytes[k], hipMemcpyHostToDevice, S.st));
    FlacFrame* d_tab = nullptr;
    FlacManyEnt* d_ents = nullptr;
    int32_t *d_planes = nullptr, *d_out = nullptr;
    int* d_status = nullptr;
    CKR(S.upload(&d_tab, tab.data(), tab.size()));
    CKR(S.upload(&d_ents, fents.data(), fents.size()));
    CKR(S.alloc(&d_planes, planes));
    CKR(S.alloc(&d_status, tab.size()));
    CKR(S.upload(&d_out, samples_out, (size_t)cap_samples));      // copied in AND out
    CKR(flac_many_launch<int32_t>(d_bytes, d_tab, (int)tab.size(), d_ents, n, d_planes, d_status, d_out, S.st));
    CKR(S.download(status.data(), d_status, status.size()));
    CKR(S.download(samples_out, d_out, (size_t)cap_samples));
    CKR(S.finish());
    for (int k = 0; k < n; ++k) {
        status_out[k] = put_many_first_bad(status.data() + first_frame[(size_t)k], fs[(size_t)k].frames.size()) >= 0 ? WLX_ERR_DATA : WLX_OK;
        n_frames_out[k] = fs[(size_t)k].info.total_samples;
        channels_out[k] = fs[(size_t)k].info.channels;
    }
    return WLX_OK;
}
