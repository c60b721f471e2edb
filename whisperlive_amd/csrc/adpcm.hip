// adpcm.hip — the telephony WAV front end of the file path (include/wlx.h wlx_wav_probe, wlx_pcm_put_wav, wlx_pcm_put_wav_split; test
// hook wlx_debug_adpcm_decode): G.711 mu-law / A-law (WAVE tags 7 / 6), IMA / DVI ADPCM (0x11) and Microsoft ADPCM (0x02). The file's
// data chunk crosses PCIe once, as it is, and feeds the resampler of resample.hip without leaving HBM.
//
// Host: wav_index walks the RIFF chunks (`fmt `, `fact`, `data`), works out the frame count and, for the ADPCM tags, reads every
// block's header: an IMA step index above 88 or an MS predictor index outside the coefficient table is a damaged stream.
// G.711: no decode launch. The bytes ARE the resampler's input: resample_run streams them through the slot's staging blocks into
// resample_kernel<WLX_PCM_MULAW / ALAW> (the live ring's instantiations), one byte per sample.
// ADPCM: adpcm_decode_kernel, one LANE per (block, channel) — the recurrence is serial inside a block, blocks are independent. A
// workgroup owns G consecutive blocks: it copies their bytes into LDS with coalesced loads, its first G * channels lanes run
// adpcm_core.h's block decoder from LDS into an int16 LDS tile laid out as the output is ([sample][channel] within a block), and all
// lanes store the tile as coalesced float32 interleaved frames [n_frames][channels] = int16 * 2^-15: what flac_finish_kernel leaves
// for a FLAC file. Then ONE launch of resample_kernel<WLX_PCM_F32> over those frames. One wait, at the end.
// LDS banks: lanes of neighbouring blocks read the byte rows and write the tile rows at one fixed stride, so both strides are padded
// to an ODD number of dwords (adpcm_shape): without that a block_align of 256 bytes would put every lane of a wave on one bank.
#include <cstring>
#include <type_traits>
#include "engine.h"
#include "adpcm_core.h"
#include "frontend.h"

namespace wlx {

constexpr int ADPCM_THREADS = 256;
constexpr size_t ADPCM_MAX_LDS = 64 * 1024;   // byte rows + sample tile of a workgroup (the default dynamic-LDS limit)

struct AdpcmShape { int G, bstride, tstride; size_t lds; };     // blocks per workgroup, LDS bytes per byte row, int16 per tile row

// G = 0: one block does not fit the LDS
static AdpcmShape adpcm_shape(int block_align, int ch, int spb) {
    AdpcmShape s{};
    s.bstride = (((block_align + 3) / 4) | 1) * 4;
    s.tstride = ((((long long)spb * ch * 2 + 3) / 4) | 1) * 2;
    const size_t per = (size_t)s.bstride + (size_t)s.tstride * 2;
    const size_t coef_bytes = 2 * ADPCM_MAX_COEF * sizeof(int16_t);           // behind the tile: the MS coefficient pairs
    s.G = (int)std::min<size_t>((size_t)(ADPCM_THREADS / ch), (ADPCM_MAX_LDS - coef_bytes) / per);
    s.lds = (size_t)s.G * per + coef_bytes;
    return s;
}

static inline unsigned rd16(const uint8_t* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }
static inline unsigned long long rd32(const uint8_t* p) { return (unsigned long long)rd16(p) | ((unsigned long long)rd16(p + 2) << 16); }

// WLX_OK: `out` holds the file's shape (served or not). WLX_ERR_DATA: no RIFF / WAVE, no `fmt ` / `data` chunk, a damaged block header.
int wav_index(const uint8_t* b, long long n, WavStream& out) {
    if (!b || n < 12 || std::memcmp(b, "RIFF", 4) || std::memcmp(b + 8, "WAVE", 4)) return set_error(WLX_ERR_DATA, "WAV: not a RIFF/WAVE file");
    const uint8_t *fmt = nullptr, *data = nullptr;
    long long fmt_len = 0, data_len = 0, fact = 0;
    for (long long pos = 12; pos + 8 <= n;) {
        const long long size = (long long)rd32(b + pos + 4), body = pos + 8, len = std::min(size, n - body);
        if (!std::memcmp(b + pos, "fmt ", 4)) { fmt = b + body; fmt_len = len; }
        else if (!std::memcmp(b + pos, "fact", 4) && len >= 4) fact = (long long)rd32(b + body);
        else if (!std::memcmp(b + pos, "data", 4)) { data = b + body; data_len = len; break; }
        pos = body + size + (size & 1);
    }
    if (!fmt || !data || fmt_len < 16) return set_error(WLX_ERR_DATA, "WAV: no fmt / data chunk");
    wlx_wav_info& wi = out.info;
    wi.format_tag = (int32_t)rd16(fmt);
    wi.channels = (int32_t)rd16(fmt + 2);
    wi.sample_rate = (int32_t)rd32(fmt + 4);
    wi.block_align = (int32_t)rd16(fmt + 12);
    wi.bits_per_sample = (int32_t)rd16(fmt + 14);
    if (wi.format_tag == WAV_TAG_EXT && fmt_len >= 26) wi.format_tag = (int32_t)rd16(fmt + 24);
    wi.data_offset = data - b;
    wi.data_bytes = data_len;
    wi.samples_per_block = 0; wi.n_frames = 0; wi.served = 0;
    const int ch = wi.channels, ba = wi.block_align, tag = wi.format_tag;
    if (ch < 1) return set_error(WLX_ERR_DATA, "WAV: the fmt chunk counts 0 channels");
    bool shape_ok = false;
    if (tag == WAV_TAG_MULAW || tag == WAV_TAG_ALAW) {
        if (wi.bits_per_sample == 8) {
            wi.samples_per_block = 1;
            wi.n_frames = data_len / ch;
            shape_ok = true;
        }
    } else if (tag == WAV_TAG_IMA || tag == WAV_TAG_MS) {
        out.kind = tag == WAV_TAG_IMA ? ADPCM_IMA : ADPCM_MS;
        if (out.kind == ADPCM_MS) {
            static const int16_t STD[14] = {256, 0, 512, -256, 0, 0, 192, 64, 240, 0, 460, -208, 392, -232};
            const int nc = fmt_len >= 22 ? (int)rd16(fmt + 20) : 0;
            if (nc > 0 && fmt_len >= 22 + 4LL * nc) {
                out.n_coef = nc;
                for (int i = 0; i < 2 * std::min(nc, ADPCM_MAX_COEF); ++i) out.coefs[i] = (int16_t)rd16(fmt + 22 + 2 * i);
            } else {
                out.n_coef = 7;
                std::memcpy(out.coefs, STD, sizeof(STD));
            }
        }
        const int hdr = (out.kind == ADPCM_IMA ? 4 : 7) * ch;
        out.layout_ok = wi.bits_per_sample == 4 && ba >= hdr &&
                        (out.kind == ADPCM_IMA ? (ba - hdr) % (4 * ch) == 0 : ((ba - hdr) * 2) % ch == 0);
        if (out.layout_ok) {
            wi.samples_per_block = out.kind == ADPCM_IMA ? adpcm_ima_samples(ba, ch) : adpcm_ms_samples(ba, ch);
            const long long blocks = data_len / ba;              // a trailing partial block is dropped
            wi.n_frames = blocks * wi.samples_per_block;
            if (fact > 0 && fact < wi.n_frames) wi.n_frames = fact;
            for (long long k = 0; k < blocks; ++k) {
                const uint8_t* blk = data + k * ba;
                for (int c = 0; c < ch; ++c) {
                    if (out.kind == ADPCM_IMA && blk[4 * c + 2] > 88)
                        return set_error(WLX_ERR_DATA, "WAV: IMA ADPCM block %lld, channel %d: step index %d is above 88", k, c, (int)blk[4 * c + 2]);
                    if (out.kind == ADPCM_MS && blk[c] >= out.n_coef)
                        return set_error(WLX_ERR_DATA, "WAV: MS ADPCM block %lld, channel %d: predictor index %d, the fmt chunk holds %d "
                                         "coefficient pairs", k, c, (int)blk[c], out.n_coef);
                }
            }
            shape_ok = out.n_coef <= ADPCM_MAX_COEF && ch <= WLX_PCM_MAX_CHANNELS && adpcm_shape(ba, ch, wi.samples_per_block).G >= 1;
        }
    } else if ((tag == 1 || tag == 3) && wi.bits_per_sample >= 8) {
        wi.samples_per_block = 1;
        wi.n_frames = data_len / ((long long)ch * (wi.bits_per_sample / 8));
    }
    wi.served = shape_ok && ch <= WLX_PCM_MAX_CHANNELS && wi.n_frames > 0 && wi.sample_rate > 0 &&
                wi.n_frames <= (long long)wi.sample_rate * 3600 + wi.sample_rate &&
                resample_check_args(b, wi.n_frames, ch, WLX_PCM_F32, wi.sample_rate) == WLX_OK;
    return WLX_OK;
}

int wav_served(const WavStream& w) {
    if (w.info.served) return WLX_OK;
    return set_error(WLX_ERR_ARG, "WAV file of tag 0x%x, %d Hz x %d channels x %d bits, block_align %d, %lld frames: outside what the device "
                     "route serves (G.711 / IMA / MS ADPCM, 1..%d channels, <= 3600 s, a rate the resampler serves, a block that fits the "
                     "decoder's LDS): decode on the host", w.info.format_tag, w.info.sample_rate, w.info.channels, w.info.bits_per_sample,
                     w.info.block_align, (long long)w.info.n_frames, WLX_PCM_MAX_CHANNELS);
}

// ------------------------------------------------------------------------------------------------ kernel
struct AdpcmArgs {
    const uint8_t* bytes;       // the data chunk: block k at bytes + k * block_align (the base is 4-byte aligned and readable to the next multiple of 4)
    void* out;                  // [n_frames][channels], float32 (int16 * 2^-15) or int16 (the hook)
    long long n_blocks, n_frames;
    int block_align, channels, spb;
    int G, bstride, tstride;
    int n_coef;
    int16_t coefs[2 * ADPCM_MAX_COEF];
};

template <int KIND, class T>
__global__ __launch_bounds__(ADPCM_THREADS) void adpcm_decode_kernel(AdpcmArgs p) {
    extern __shared__ uint32_t adpcm_lds[];
    uint8_t* rows = reinterpret_cast<uint8_t*>(adpcm_lds);
    int16_t* tile = reinterpret_cast<int16_t*>(rows + (size_t)p.G * p.bstride);
    int16_t* cf = tile + (size_t)p.G * p.tstride;                      // MS: the coefficient pairs
    const int ba = p.block_align, ch = p.channels;
    const long long g0 = (long long)blockIdx.x * p.G;
    const int ng = (int)(p.n_blocks - g0 < p.G ? p.n_blocks - g0 : p.G);
    const long long byte0 = g0 * ba;
    const int total = ng * ba;
    if (KIND == ADPCM_MS)
        for (int i = threadIdx.x; i < 2 * ADPCM_MAX_COEF; i += ADPCM_THREADS) cf[i] = p.coefs[i];
    if ((ba & 3) == 0) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.bytes + byte0);
        for (int i = threadIdx.x; i < total / 4; i += ADPCM_THREADS) {
            const int idx = i * 4, g = idx / ba, r = idx - g * ba;
            *reinterpret_cast<uint32_t*>(rows + (size_t)g * p.bstride + r) = src[i];
        }
    } else {                                                           // MS block sizes need not be whole dwords: aligned loads, byte stores
        const long long a0 = byte0 & ~3LL;
        const int lead = (int)(byte0 - a0), nd = (lead + total + 3) / 4;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.bytes + a0);
        for (int i = threadIdx.x; i < nd; i += ADPCM_THREADS) {
            const uint32_t v = src[i];
            for (int k = 0; k < 4; ++k) {
                const int idx = i * 4 + k - lead;
                if (idx >= 0 && idx < total) {
                    const int g = idx / ba, r = idx - g * ba;
                    rows[(size_t)g * p.bstride + r] = (uint8_t)(v >> (8 * k));
                }
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < ng * ch) {
        const int g = threadIdx.x / ch, c = threadIdx.x - g * ch;
        const uint8_t* blk = rows + (size_t)g * p.bstride;
        int16_t* o = tile + (size_t)g * p.tstride + c;
        if (KIND == ADPCM_IMA) (void)adpcm_ima_block(blk, ba, ch, c, p.spb, o, ch);
        else (void)adpcm_ms_block(blk, ba, ch, c, p.spb, cf, p.n_coef, o, ch);
    }
    __syncthreads();
    const int per = p.spb * ch;
    const long long base = g0 * per, limit = p.n_frames * ch;         // the `fact` cut may end inside the last block
    T* out = static_cast<T*>(p.out);
    for (int k = threadIdx.x; k < ng * per; k += ADPCM_THREADS) {
        if (base + k >= limit) break;
        const int g = k / per, r = k - g * per;
        const int16_t v = tile[(size_t)g * p.tstride + r];
        out[base + k] = std::is_same<T, float>::value ? (T)((float)v * (1.0f / 32768.0f)) : (T)v;
    }
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the blocks the frame count needs (a `fact` chunk may leave whole blocks unused) and their bytes
long long adpcm_blocks(const WavStream& w) { return (w.info.n_frames + w.info.samples_per_block - 1) / w.info.samples_per_block; }

// the decode launch on `st`; no wait. d_bytes: the data chunk's first adpcm_blocks(w) blocks; out: [n_frames][channels] of T
template <class T>
static int adpcm_launch(const WavStream& w, const uint8_t* d_bytes, T* out, hipStream_t st) {
    const wlx_wav_info& wi = w.info;
    const AdpcmShape sh = adpcm_shape(wi.block_align, wi.channels, wi.samples_per_block);
    AdpcmArgs p{};
    p.bytes = d_bytes; p.out = out; p.n_blocks = adpcm_blocks(w); p.n_frames = wi.n_frames;
    p.block_align = wi.block_align; p.channels = wi.channels; p.spb = wi.samples_per_block;
    p.G = sh.G; p.bstride = sh.bstride; p.tstride = sh.tstride;
    p.n_coef = std::max(1, std::min(w.n_coef, ADPCM_MAX_COEF));
    std::memcpy(p.coefs, w.coefs, sizeof(p.coefs));
    const unsigned grid = (unsigned)((p.n_blocks + sh.G - 1) / sh.G);
    const size_t lds = sh.lds;
    if (w.kind == ADPCM_IMA) hipLaunchKernelGGL((adpcm_decode_kernel<ADPCM_IMA, T>), dim3(grid), dim3(ADPCM_THREADS), lds, st, p);
    else hipLaunchKernelGGL((adpcm_decode_kernel<ADPCM_MS, T>), dim3(grid), dim3(ADPCM_THREADS), lds, st, p);
    CK(hipGetLastError());
    return WLX_OK;
}

// the float32 launch by name, for put_many.hip (frontend.h)
int adpcm_launch_f32(const WavStream& w, const uint8_t* d_bytes, float* out, hipStream_t st) { return adpcm_launch<float>(w, d_bytes, out, st); }

}  // namespace wlx

using namespace wlx;

extern "C" int32_t wlx_wav_probe(const void* bytes, int64_t n_bytes, wlx_wav_info* out) {
    if (!bytes || !out || n_bytes < 0) return set_error(WLX_ERR_ARG, "null argument");
    WavStream w;
    CKR(wav_index(static_cast<const uint8_t*>(bytes), n_bytes, w));
    *out = w.info;
    return WLX_OK;
}

// wlx_pcm_put_wav (split = false: the down-mix into `item`) and wlx_pcm_put_wav_split (split = true: channel c into item + c)
static int pcm_put_wav(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_wav_info* info_out, int64_t* n_out,
                       bool split) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!bytes || n_bytes <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    // ---- host: everything that can refuse the file, before any launch and before the item's PCM is touched
    WavStream w;
    CKR(wav_index(static_cast<const uint8_t*>(bytes), n_bytes, w));
    if (info_out) *info_out = w.info;
    CKR(wav_served(w));
    const wlx_wav_info& wi = w.info;
    const long long total = wi.n_frames;
    const int ch = wi.channels;
    const int n_items = split ? ch : 1;
    if (item + n_items > s->B)
        return set_error(WLX_ERR_ARG, "wlx_pcm_put_wav_split: items [%d, %d) outside the slot's %d", item, item + n_items, s->B);
    ResamplePlan pl{};
    CKR(resample_plan(e->device, wi.sample_rate, &pl));
    const int64_t n = resample_out_len(pl, total);
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CK(hipSetDevice(e->device));
    const uint8_t* data = static_cast<const uint8_t*>(bytes) + wi.data_offset;
    const bool adpcm = w.kind >= 0;
    const size_t in_bytes = adpcm ? (size_t)adpcm_blocks(w) * (size_t)wi.block_align : 0;
    const size_t frames_at = up256(in_bytes), need = adpcm ? frames_at + up256((size_t)total * ch * sizeof(float)) : 0;
    if (need > s->flac.cap) {                // grown before anything else changes: a refusal leaves the slot as it was
        unsigned char* nb = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&nb), need) != hipSuccess) {
            (void)hipGetLastError();
            return set_error(WLX_ERR_NOMEM, "WAV scratch of %zu bytes (data chunk, float32 frames) cannot be had", need);
        }
        CK(hipStreamSynchronize(s->stream));
        if (s->flac.buf) (void)hipFree(s->flac.buf);
        s->flac.buf = nb; s->flac.cap = need;
    }
    CKR(slot_resample_stage(s));
    bool recorded = false;
    for (int c = 0; c < n_items; ++c) recorded = recorded || std::find(s->lm_items.begin(), s->lm_items.end(), (int)item + c) != s->lm_items.end();
    if ((size_t)n > s->pcm_cap || recorded)
        CKR(flush_logmel(e, s));            // a recorded log-mel request reads this item's PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, (size_t)n));
    for (int c = 0; c < n_items; ++c) s->npcm[item + c] = 0;      // (a failed run leaves no half-written audio resident)
    float* dst = s->pcm + (size_t)item * s->pcm_cap;
    const long long stride = split ? (long long)s->pcm_cap : 0;
    if (!adpcm) {
        // G.711: the code bytes are the resampler's input, one byte per sample; resample_run uploads them block by block and waits once
        const int fmt = wi.format_tag == WAV_TAG_MULAW ? WLX_PCM_MULAW : WLX_PCM_ALAW;
        CKR(resample_run(pl, data, total, ch, fmt, resample_default_block(ch, fmt), s->rs, dst, s->stream, nullptr, stride));
    } else {
        // ---- device: upload, decode, resample; one wait
        float* frames = reinterpret_cast<float*>(s->flac.buf + frames_at);
        int rc = [&]() -> int {
            int blk = 0;
            CKR(staged_upload(&s->rs, &blk, s->flac.buf, data, in_bytes, s->stream));
            CKR(adpcm_launch<float>(w, s->flac.buf, frames, s->stream));
            if (split) CKR(resample_run_device_split(pl, frames, total, ch, dst, stride, s->stream));
            else CKR(resample_run_device(pl, frames, total, ch, dst, s->stream));
            return WLX_OK;
        }();
        hipError_t he = hipStreamSynchronize(s->stream);       // the caller's bytes and the staging halves may be reused after return
        s->rs.used[0] = s->rs.used[1] = false;
        if (rc == WLX_OK && he != hipSuccess) rc = set_error(WLX_ERR_HIP, "%s: %s", split ? "wlx_pcm_put_wav_split" : "wlx_pcm_put_wav", hipGetErrorString(he));
        if (s->flac.cap > 2 * RS_BLOCK_BYTES) {                // a long file's scratch does not stay with the slot
            (void)hipFree(s->flac.buf);
            s->flac.buf = nullptr; s->flac.cap = 0;
        }
        CKR(rc);
    }
    for (int c = 0; c < n_items; ++c) s->npcm[item + c] = n;
    if (n_out) *n_out = n;
    return WLX_OK;
}

extern "C" int32_t wlx_pcm_put_wav(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_wav_info* info_out,
                                   int64_t* n_out) {
    return pcm_put_wav(e, slot, item, bytes, n_bytes, info_out, n_out, false);
}

extern "C" int32_t wlx_pcm_put_wav_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* bytes, int64_t n_bytes,
                                         wlx_wav_info* info_out, int64_t* n_out) {
    return pcm_put_wav(e, slot, first_item, bytes, n_bytes, info_out, n_out, true);
}

// ------------------------------------------------------------------------------------------------ test hook (host.h HookScope)
extern "C" int32_t wlx_debug_adpcm_decode(int32_t device, const void* bytes, int64_t n_bytes, int16_t* samples_out, int64_t cap_samples,
                                          int64_t* n_frames_out, int32_t* channels_out) {
    if (!bytes || !samples_out || !n_frames_out || !channels_out || n_bytes <= 0 || cap_samples < 0) return set_error(WLX_ERR_ARG, "null argument");
    WavStream w;
    CKR(wav_index(static_cast<const uint8_t*>(bytes), n_bytes, w));
    const wlx_wav_info& wi = w.info;
    // the hook decodes what the kernel decodes: any rate
    if (w.kind < 0 || !w.layout_ok || wi.channels > WLX_PCM_MAX_CHANNELS || w.n_coef > ADPCM_MAX_COEF || wi.n_frames <= 0 ||
        wi.n_frames > (1LL << 31) || adpcm_shape(wi.block_align, wi.channels, wi.samples_per_block).G < 1)
        return set_error(WLX_ERR_ARG, "WAV file of tag 0x%x, %d channels, block_align %d, %lld frames: outside the ADPCM decoder's scope",
                         wi.format_tag, wi.channels, wi.block_align, (long long)wi.n_frames);
    const long long total = wi.n_frames;
    const int ch = wi.channels;
    if (total * ch > cap_samples) return set_error(WLX_ERR_ARG, "output buffer too small");
    HookScope S;
    CKR(S.begin(device));
    const size_t in_bytes = (size_t)adpcm_blocks(w) * (size_t)wi.block_align;
    unsigned char* d_bytes = nullptr;
    int16_t* d_out = nullptr;
    CKR(S.alloc(&d_bytes, up256(in_bytes)));
    CKR(S.alloc(&d_out, (size_t)total * ch));
    CK(hipMemcpyAsync(d_bytes, static_cast<const uint8_t*>(bytes) + wi.data_offset, in_bytes, hipMemcpyHostToDevice, S.st));
    CKR(adpcm_launch<int16_t>(w, d_bytes, d_out, S.st));
    CKR(S.download(samples_out, d_out, (size_t)total * ch));
    CKR(S.finish());
    *n_frames_out = total;
    *channels_out = ch;
    return WLX_OK;
}
