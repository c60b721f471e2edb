// flac.hip — the FLAC front end of the file path (include/wlx.h wlx_flac_probe, wlx_pcm_put_flac; test hook wlx_debug_flac_decode):
// the file's COMPRESSED bytes cross PCIe once, are decoded in HBM and feed the resampler of resample.hip without leaving it.
//
// Host: STREAMINFO, then a frame index built WITHOUT decoding (flac_index): a frame ends where the next one provably starts — a sync
// code whose header parses, whose CRC-8 matches, whose coded frame / sample number is the expected next one, and in front of which the
// CRC-16 of the current frame's bytes matches. Anything less is a false sync inside a frame and the scan goes on.
// Device: flac_frames_kernel, one LANE per frame, runs flac_core.h's flac_decode_frame into planar int32 scratch and writes one
// status word per frame; flac_finish_kernel, one workgroup per frame and one lane per sample, undoes the stereo decorrelation, scales
// by 2^-(bps - 1) and stores float32 interleaved [n][channels]; then ONE launch of resample_kernel<WLX_PCM_F32> over those frames.
// One wait, at the end, then the status words are read.
// The STREAMINFO MD5 is NOT checked on this route (it would mean bringing every sample back to the host): the per-frame CRC-16 on
// the host and the per-frame "ended exactly at end - 2" check on the device stand in for it. The Python decoder of audio_io.py keeps
// the MD5 check; it is the oracle of the tests and the fallback for the streams this route refuses.
#include <chrono>
#include <cmath>
#include <cstring>
#include <type_traits>
#include "engine.h"
#include "flac_core.h"
#include "frontend.h"

namespace wlx {


// ------------------------------------------------------------------------------------------------ CRCs
struct FlacCrc {
    uint8_t t8[256];
    uint16_t t16[8][256];        // t16[k][i]: CRC-16 of byte i followed by k zero bytes (slicing by 8)
    FlacCrc() {
        for (int i = 0; i < 256; ++i) {
            uint8_t c = (uint8_t)i;
            for (int k = 0; k < 8; ++k) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1);
            t8[i] = c;
            uint16_t d = (uint16_t)(i << 8);
            for (int k = 0; k < 8; ++k) d = (uint16_t)((d & 0x8000) ? (d << 1) ^ 0x8005 : d << 1);
            t16[0][i] = d;
        }
        for (int k = 1; k < 8; ++k)
            for (int i = 0; i < 256; ++i) t16[k][i] = (uint16_t)((t16[k - 1][i] << 8) ^ t16[0][t16[k - 1][i] >> 8]);
    }
};
static const FlacCrc& flac_crc() { static const FlacCrc c; return c; }

static uint8_t crc8(const uint8_t* p, size_t n) {
    const FlacCrc& T = flac_crc();
    uint8_t c = 0;
    for (size_t i = 0; i < n; ++i) c = T.t8[c ^ p[i]];
    return c;
}

static uint16_t crc16(uint16_t c, const uint8_t* p, size_t n) {
    const FlacCrc& T = flac_crc();
    while (n >= 8) {
        c ^= (uint16_t)((p[0] << 8) | p[1]);
        c = (uint16_t)(T.t16[7][c >> 8] ^ T.t16[6][c & 0xFF] ^ T.t16[5][p[2]] ^ T.t16[4][p[3]] ^ T.t16[3][p[4]] ^ T.t16[2][p[5]] ^
                       T.t16[1][p[6]] ^ T.t16[0][p[7]]);
        p += 8; n -= 8;
    }
    for (; n; --n, ++p) c = (uint16_t)((c << 8) ^ T.t16[0][(c >> 8) ^ *p]);
    return c;
}

// ------------------------------------------------------------------------------------------------ frame header
struct FlacHeader { int variable, blocksize, rate, channels, ch_code, bps, len; unsigned long long number; };

// -> 1: a frame header with a matching CRC-8 starts at p; 0: not one (reserved code, short, CRC-8). rate / bps 0 = "as STREAMINFO"
static int flac_header(const uint8_t* b, long long p, long long nbytes, FlacHeader* h) {
    if (p + 6 > nbytes || b[p] != 0xFF || (b[p + 1] & 0xFE) != 0xF8) return 0;
    h->variable = b[p + 1] & 1;
    const int bs_code = b[p + 2] >> 4, sr_code = b[p + 2] & 15, ch_code = b[p + 3] >> 4, ss_code = (b[p + 3] >> 1) & 7;
    if (b[p + 3] & 1) return 0;
    if (bs_code == 0 || sr_code == 15 || ch_code > 10 || ss_code == 3) return 0;
    long long q = p + 4;
    const unsigned first = b[q++];
    unsigned long long num = first;
    if (first >= 0x80) {
        int ones = 0;
        for (unsigned m = 0x80; first & m; m >>= 1) ++ones;
        if (ones < 2 || ones > 7) return 0;                       // 7 ones: 0xFE, the 36-bit form
        num = ones == 7 ? 0 : (first & (0x7Fu >> ones));
        for (int i = 1; i < ones; ++i) {
            if (q >= nbytes || (b[q] & 0xC0) != 0x80) return 0;
            num = (num << 6) | (b[q++] & 0x3F);
        }
    }
    if (!h->variable && num > 0x7FFFFFFFull) return 0;            // a frame number has at most 31 bits
    h->number = num;
    int n;
    if (bs_code == 1) n = 192;
    else if (bs_code <= 5) n = 576 << (bs_code - 2);
    else if (bs_code == 6) { if (q + 1 > nbytes) return 0; n = b[q] + 1; q += 1; }
    else if (bs_code == 7) { if (q + 2 > nbytes) return 0; n = ((b[q] << 8) | b[q + 1]) + 1; q += 2; }
    else n = 256 << (bs_code - 8);
    static const int rates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    int rate;
    if (sr_code < 12) rate = rates[sr_code];
    else if (sr_code == 12) { if (q + 1 > nbytes) return 0; rate = b[q] * 1000; q += 1; }
    else { if (q + 2 > nbytes) return 0; rate = ((b[q] << 8) | b[q + 1]) * (sr_code == 14 ? 10 : 1); q += 2; }
    static const int widths[8] = {0, 8, 12, -1, 16, 20, 24, 32};
    if (q + 1 > nbytes) return 0;
    if (crc8(b + p, (size_t)(q - p)) != b[q]) return 0;
    h->blocksize = n; h->rate = rate; h->channels = ch_code < 8 ? ch_code + 1 : 2; h->ch_code = ch_code; h->bps = widths[ss_code];
    h->len = (int)(q + 1 - p);
    return 1;
}

// ------------------------------------------------------------------------------------------------ metadata + frame index
// WLX_OK: `out` holds the stream's shape and its frame table (served or not). WLX_ERR_DATA: damaged. WLX_ERR_ARG: a container or a
// stream shape this front end does not take apart at all (Ogg, a tag in front of the magic, a mid-stream change of shape).
int flac_index(const uint8_t* b, long long nbytes, FlacStream& out) {
    if (!b || nbytes < 4) return set_error(WLX_ERR_DATA, "FLAC: %lld bytes hold no stream", nbytes);
    if (!std::memcmp(b, "OggS", 4)) return set_error(WLX_ERR_ARG, "Ogg FLAC is not served by the device route");
    if (!std::memcmp(b, "ID3", 3)) return set_error(WLX_ERR_ARG, "an ID3 tag in front of the fLaC magic is not served by the device route");
    if (std::memcmp(b, "fLaC", 4)) return set_error(WLX_ERR_DATA, "FLAC: no fLaC magic");
    long long pos = 4;
    const uint8_t* si = nullptr;
    for (;;) {
        if (pos + 4 > nbytes) return set_error(WLX_ERR_DATA, "FLAC: the metadata runs past the end of the data");
        const int last = b[pos] >> 7, typ = b[pos] & 0x7F;
        const long long ln = ((long long)b[pos + 1] << 16) | (b[pos + 2] << 8) | b[pos + 3];
        if (pos + 4 + ln > nbytes) return set_error(WLX_ERR_DATA, "FLAC: the metadata runs past the end of the data");
        if (typ == 0 && ln >= 34 && !si) si = b + pos + 4;
        pos += 4 + ln;
        if (last) break;
    }
    if (!si) return set_error(WLX_ERR_DATA, "FLAC: no STREAMINFO block");
    wlx_flac_info& fi = out.info;
    const int max_bs = (si[2] << 8) | si[3];
    unsigned long long x = 0;
    for (int i = 10; i < 18; ++i) x = (x << 8) | si[i];
    fi.sample_rate = (int32_t)(x >> 44);
    fi.channels = (int32_t)((x >> 41) & 7) + 1;
    fi.bits_per_sample = (int32_t)((x >> 36) & 31) + 1;
    fi.total_samples = (int64_t)(x & ((1ull << 36) - 1));
    fi.max_blocksize = max_bs;
    if (fi.sample_rate <= 0) return set_error(WLX_ERR_DATA, "FLAC: STREAMINFO holds a sample rate of 0");

    out.frames.clear();
    long long done = 0;
    int variable = -1, biggest = 0;
    unsigned long long base = 0;         // the first frame's coded number: a stream cut out of a longer one does not start at 0
    FlacHeader h{};
    if (pos >= nbytes) {
        if (fi.total_samples != 0) return set_error(WLX_ERR_DATA, "FLAC: no frames, STREAMINFO counts %lld samples", (long long)fi.total_samples);
    } else if (!flac_header(b, pos, nbytes, &h)) {
        return set_error(WLX_ERR_DATA, "FLAC: lost frame sync at byte %lld", pos);
    }
    while (pos < nbytes) {
        // `h` is the accepted header of the frame at `pos`
        if (variable < 0) { variable = h.variable; base = h.number; }
        if ((h.rate && h.rate != fi.sample_rate) || (h.bps && h.bps != fi.bits_per_sample) || h.channels != fi.channels || h.variable != variable)
            return set_error(WLX_ERR_ARG, "FLAC: frame %zu changes the rate, width, channel count or blocking of the stream: not served by "
                             "the device route", out.frames.size());
        if (h.number != base + (unsigned long long)(variable ? done : (long long)out.frames.size()))
            return set_error(WLX_ERR_DATA, "FLAC: frame %zu carries number %llu", out.frames.size(), h.number);
        // the frame's end: the next position that provably starts its successor
        const unsigned long long want = base + (variable ? (unsigned long long)(done + h.blocksize) : (unsigned long long)out.frames.size() + 1);
        long long q = pos + h.len, crc_at = pos, next = -1;
        uint16_t crc = 0;
        FlacHeader hn{};
        while (q + 1 < nbytes) {
            const void* f = std::memchr(b + q, 0xFF, (size_t)(nbytes - 1 - q));
            if (!f) break;
            q = (const uint8_t*)f - b;
            if ((b[q + 1] & 0xFE) == 0xF8 && flac_header(b, q, nbytes, &hn) && hn.number == want && q - pos >= h.len + 2) {
                crc = crc16(crc, b + crc_at, (size_t)(q - crc_at));      // CRC-16 over [pos, q), its own two bytes included: 0 when they match
                crc_at = q;
                if (crc == 0) { next = q; break; }
            }
            ++q;
        }
        const long long end = next >= 0 ? next : nbytes;
        if (next < 0) {
            if (end - pos < h.len + 2 || crc16(crc, b + crc_at, (size_t)(end - crc_at)) != 0)
                return set_error(WLX_ERR_DATA, "FLAC: frame %zu at byte %lld has no CRC-consistent end (truncated or damaged)", out.frames.size(), pos);
        }
        if (out.frames.size() >= 0x7FFFFFFFu / 2) return set_error(WLX_ERR_ARG, "FLAC: too many frames");
        out.frames.push_back(FlacFrame{pos, end, done, h.blocksize, 0});
        done += h.blocksize;
        biggest = std::max(biggest, h.blocksize);
        pos = end;
        h = hn;
    }
    if (fi.total_samples != 0 && done != fi.total_samples)
        return set_error(WLX_ERR_DATA, "FLAC: the frames hold %lld samples, STREAMINFO counts %lld", done, (long long)fi.total_samples);
    fi.total_samples = done;
    fi.n_frames = (int32_t)out.frames.size();
    if (biggest > fi.max_blocksize) fi.max_blocksize = biggest;
    fi.served = fi.channels >= 1 && fi.channels <= FLAC_MAX_CHANNELS && fi.channels <= WLX_PCM_MAX_CHANNELS && fi.bits_per_sample <= FLAC_MAX_BPS &&
                done > 0 && done <= (long long)fi.sample_rate * 3600 + fi.sample_rate && resample_check_args(b, done, fi.channels, WLX_PCM_F32, fi.sample_rate) == WLX_OK;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ kernels
constexpr int FLAC_FRAMES_THREADS = 64;      // one wave: 64 frames; the grid spreads a file's frames over the CUs
constexpr int FLAC_FINISH_THREADS = 256;

// status word of a frame: flac_core.h status in the low byte, the channel assignment the finish kernel has to undo above it
__global__ __launch_bounds__(FLAC_FRAMES_THREADS) void flac_frames_kernel(const uint8_t* __restrict__ bytes, const FlacFrame* __restrict__ tab,
                                                                          int n_frames, int bps, int channels, int32_t* __restrict__ planes,
                                                                          long long plane_stride, int* __restrict__ status) {
    const int f = blockIdx.x * FLAC_FRAMES_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const FlacFrame t = tab[f];
    int assign = 0;
    const int rc = flac_decode_frame(bytes, t.start, t.end, bps, channels, t.n, planes + t.first, plane_stride, &assign);
    status[f] = rc | (assign << 8);
}

// T = float: sample * scale, the front end's frames. T = int32_t: the integers themselves (wlx_debug_flac_decode). A frame whose status is
// not FLAC_OK stores zeros (its planes hold whatever the decoder had written when it stopped).
template <class T>
__global__ __launch_bounds__(FLAC_FINISH_THREADS) void flac_finish_kernel(const FlacFrame* __restrict__ tab, const int* __restrict__ status,
                                                                          const int32_t* __restrict__ planes, long long plane_stride, int channels,
                                                                          float scale, T* __restrict__ out) {
    const FlacFrame t = tab[blockIdx.x];
    const int st = status[blockIdx.x];
    const bool ok = (st & 0xFF) == FLAC_OK;
    const int assign = st >> 8;
    for (int i = threadIdx.x; i < t.n; i += FLAC_FINISH_THREADS) {
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

// ------------------------------------------------------------------------------------------------ device run
struct FlacDev { uint8_t* bytes; FlacFrame* tab; int* status; int32_t* planes; void* frames; };

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the scratch layout: file bytes | frame table | status words | int32 planes | output frames (out_elem bytes per sample)
static size_t flac_layout(const FlacStream& s, long long nbytes, unsigned char* base, FlacDev* d) {
    const size_t nf = s.frames.size(), ns = (size_t)s.info.total_samples * (size_t)s.info.channels;
    size_t o = 0;
    d->bytes = base + o; o += up256((size_t)nbytes);
    d->tab = reinterpret_cast<FlacFrame*>(base + o); o += up256(nf * sizeof(FlacFrame));
    d->status = reinterpret_cast<int*>(base + o); o += up256(nf * sizeof(int));
    d->planes = reinterpret_cast<int32_t*>(base + o); o += up256(ns * sizeof(int32_t));
    d->frames = base + o; o += up256(ns * 4);
    return o;
}

// host -> device on `st`: through the two pinned staging blocks when there are any (two copies in flight, as resample_run), else straight
// from the caller's pageable memory (kernels.h: adpcm.hip uploads a WAV file's data chunk the same way)
int staged_upload(ResampleStage* sg, int* blk, void* dst, const void* src, size_t n, hipStream_t st) {
    if (!sg) {
        if (n) CK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st));
        return WLX_OK;
    }
    for (size_t off = 0; off < n; off += RS_BLOCK_BYTES, ++*blk) {
        const size_t len = std::min(n - off, (size_t)RS_BLOCK_BYTES);
        const int b = *blk & 1;
        if (sg->used[b]) CK(hipEventSynchronize(sg->copied[b]));      // the pinned half is free once the copy out of it (two blocks ago) has run
        std::memcpy(sg->pinned[b], static_cast<const char*>(src) + off, len);
        CK(hipMemcpyAsync(static_cast<char*>(dst) + off, sg->pinned[b], len, hipMemcpyHostToDevice, st));
        CK(hipEventRecord(sg->copied[b], st));
        sg->used[b] = true;
    }
    return WLX_OK;
}

// upload + frames kernel + finish kernel on `st`; no wait. ev (nullable): 4 events recorded around the three stages
template <class T>
static int flac_launch(const FlacStream& s, const void* bytes, long long nbytes, const FlacDev& d, ResampleStage* sg, hipStream_t st, hipEvent_t* ev) {
    const int nf = (int)s.frames.size(), ch = s.info.channels;
    const long long total = s.info.total_samples;
    int blk = 0;
    if (ev) CK(hipEventRecord(ev[0], st));
    CKR(staged_upload(sg, &blk, d.bytes, bytes, (size_t)nbytes, st));
    CKR(staged_upload(sg, &blk, d.tab, s.frames.data(), (size_t)nf * sizeof(FlacFrame), st));
    if (ev) CK(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned)((nf + FLAC_FRAMES_THREADS - 1) / FLAC_FRAMES_THREADS)), dim3(FLAC_FRAMES_THREADS), 0, st,
                       d.bytes, d.tab, nf, s.info.bits_per_sample, ch, d.planes, total, d.status);
    CK(hipGetLastError());
    if (ev) CK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(flac_finish_kernel<T>, dim3((unsigned)nf), dim3(FLAC_FINISH_THREADS), 0, st, d.tab, d.status, d.planes, total, ch,
                       std::ldexp(1.0f, -(s.info.bits_per_sample - 1)), static_cast<T*>(d.frames));
    CK(hipGetLastError());
    if (ev) CK(hipEventRecord(ev[3], st));
    return WLX_OK;
}

int flac_check_status(const int* status, size_t nf) {
    for (size_t f = 0; f < nf; ++f)
        if ((status[f] & 0xFF) != FLAC_OK)
            return set_error(WLX_ERR_DATA, "FLAC: frame %zu does not decode (status %d: 1 past its end, 2 reserved code, 3 inconsistent partition / "
                             "header, 4 does not end at its CRC, 5 unsupported width)", f, status[f] & 0xFF);
    return WLX_OK;
}

int flac_served(const FlacStream& s) {
    if (s.info.served) return WLX_OK;
    return set_error(WLX_ERR_ARG, "FLAC stream of %d Hz x %d channels x %d bits, %lld samples: outside what the device route serves (1..%d "
                     "channels, <= %d bits, <= 3600 s, a rate the resampler serves): decode on the host", s.info.sample_rate, s.info.channels,
                     s.info.bits_per_sample, (long long)s.info.total_samples, FLAC_MAX_CHANNELS, FLAC_MAX_BPS);
}

}  // namespace wlx

using namespace wlx;

extern "C" int32_t wlx_flac_probe(const void* bytes, int64_t n_bytes, wlx_flac_info* out) {
    if (!bytes || !out || n_bytes < 0) return set_error(WLX_ERR_ARG, "null argument");
    FlacStream s;
    CKR(flac_index(static_cast<const uint8_t*>(bytes), n_bytes, s));
    *out = s.info;
    return WLX_OK;
}

// wlx_pcm_put_flac (split = false: the down-mix into `item`) and wlx_pcm_put_flac_split (split = true: channel c into item + c): the
// same probe, upload, frame decode and finish; they differ in the ONE resample launch behind them and in the items that become resident
static int pcm_put_flac(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_flac_info* info_out,
                        int64_t* n_out, bool split) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!bytes || n_bytes <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    // ---- host: everything that can refuse the stream, before any launch and before the item's PCM is touched
    const auto t0 = std::chrono::steady_clock::now();
    FlacStream fs;
    CKR(flac_index(static_cast<const uint8_t*>(bytes), n_bytes, fs));
    s->flac.index_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->flac.timed = false;
    if (info_out) *info_out = fs.info;
    CKR(flac_served(fs));
    const long long total = fs.info.total_samples;
    const int ch = fs.info.channels;
    const int n_items = split ? ch : 1;         // the items that take audio: item .. item + n_items - 1
    if (item + n_items > s->B)
        return set_error(WLX_ERR_ARG, "wlx_pcm_put_flac_split: items [%d, %d) outside the slot's %d", item, item + n_items, s->B);
    ResamplePlan pl{};
    CKR(resample_plan(e->device, fs.info.sample_rate, &pl));
    const int64_t n = resample_out_len(pl, total);
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CK(hipSetDevice(e->device));
    FlacDev d{};
    const size_t need = flac_layout(fs, n_bytes, nullptr, &d);
    if (need > s->flac.cap) {                // grown before anything else changes: a refusal leaves the slot as it was
        unsigned char* nb = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&nb), need) != hipSuccess) {
            (void)hipGetLastError();
            return set_error(WLX_ERR_NOMEM, "FLAC scratch of %zu bytes (file bytes, frame table, int32 planes, float32 frames) cannot be had", need);
        }
        CK(hipStreamSynchronize(s->stream));
        if (s->flac.buf) (void)hipFree(s->flac.buf);
        s->flac.buf = nb; s->flac.cap = need;
    }
    (void)flac_layout(fs, n_bytes, s->flac.buf, &d);
    CKR(slot_resample_stage(s));
    for (hipEvent_t& ev : s->flac.ev) if (!ev) CK(hipEventCreate(&ev));
    bool recorded = false;
    for (int c = 0; c < n_items; ++c) recorded = recorded || std::find(s->lm_items.begin(), s->lm_items.end(), (int)item + c) != s->lm_items.end();
    if ((size_t)n > s->pcm_cap || recorded)
        CKR(flush_logmel(e, s));            // a recorded log-mel request reads this item's PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, (size_t)n));
    // ---- device: upload, decode, finish, resample; one wait
    for (int c = 0; c < n_items; ++c) s->npcm[item + c] = 0;      // (a failed run leaves no half-written audio resident)
    const size_t nf = fs.frames.size();
    std::vector<int> status_host;
    int* status = nullptr;
    int rc = [&]() -> int {
        CKR(flac_launch<float>(fs, bytes, n_bytes, d, &s->rs, s->stream, s->flac.ev));
        if (split)
            CKR(resample_run_device_split(pl, static_cast<const float*>(d.frames), total, ch, s->pcm + (size_t)item * s->pcm_cap,
                                          (long long)s->pcm_cap, s->stream));
        else
            CKR(resample_run_device(pl, static_cast<const float*>(d.frames), total, ch, s->pcm + (size_t)item * s->pcm_cap, s->stream));
        CK(hipEventRecord(s->flac.ev[4], s->stream));
        if (nf * sizeof(int) <= RS_BLOCK_BYTES) {      // the status words come back through a pinned block (the copies out of it are ahead in the stream)
            status = reinterpret_cast<int*>(s->rs.pinned[0]);
        } else {
            status_host.resize(nf);
            status = status_host.data();
        }
        CK(hipMemcpyAsync(status, d.status, nf * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        return WLX_OK;
    }();
    hipError_t he = hipStreamSynchronize(s->stream);       // the caller's bytes and the staging halves may be reused after return
    s->rs.used[0] = s->rs.used[1] = false;
    if (rc == WLX_OK && he != hipSuccess) rc = set_error(WLX_ERR_HIP, "%s: %s", split ? "wlx_pcm_put_flac_split" : "wlx_pcm_put_flac", hipGetErrorString(he));
    if (rc == WLX_OK) rc = flac_check_status(status, nf);
    if (rc == WLX_OK) s->flac.timed = true;
    if (s->flac.cap > 2 * RS_BLOCK_BYTES) {                // a long file's scratch does not stay with the slot
        (void)hipFree(s->flac.buf);
        s->flac.buf = nullptr; s->flac.cap = 0;
    }
    CKR(rc);
    for (int c = 0; c < n_items; ++c) s->npcm[item + c] = n;
    if (n_out) *n_out = n;
    return WLX_OK;
}

extern "C" int32_t wlx_pcm_put_flac(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_flac_info* info_out,
                                    int64_t* n_out) {
    return pcm_put_flac(e, slot, item, bytes, n_bytes, info_out, n_out, false);
}

extern "C" int32_t wlx_pcm_put_flac_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* bytes, int64_t n_bytes,
                                          wlx_flac_info* info_out, int64_t* n_out) {
    return pcm_put_flac(e, slot, first_item, bytes, n_bytes, info_out, n_out, true);
}

// ------------------------------------------------------------------------------------------------ test hooks (host.h HookScope)
extern "C" int32_t wlx_debug_flac_timings(wlx_engine* e, int32_t slot, float* ms_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!ms_out) return set_error(WLX_ERR_ARG, "null argument");
    if (!s->flac.timed) return set_error(WLX_ERR_STATE, "no completed wlx_pcm_put_flac on this slot");
    CK(hipSetDevice(e->device));
    ms_out[0] = s->flac.index_ms;
    for (int i = 0; i < 4; ++i) CK(hipEventElapsedTime(&ms_out[1 + i], s->flac.ev[i], s->flac.ev[i + 1]));
    return WLX_OK;
}

extern "C" int32_t wlx_debug_flac_decode(int32_t device, const void* bytes, int64_t n_bytes, int32_t* samples_out, int64_t cap_samples,
                                         int64_t* n_frames_out, int32_t* channels_out) {
    if (!bytes || !samples_out || !n_frames_out || !channels_out || n_bytes <= 0 || cap_samples < 0) return set_error(WLX_ERR_ARG, "null argument");
    FlacStream fs;
    CKR(flac_index(static_cast<const uint8_t*>(bytes), n_bytes, fs));
    // the hook decodes what the core decodes: any rate, <= 24 bits, <= 8 channels
    if (fs.info.channels > FLAC_MAX_CHANNELS || fs.info.bits_per_sample > FLAC_MAX_BPS || fs.info.total_samples <= 0)
        return set_error(WLX_ERR_ARG, "FLAC stream of %d channels x %d bits, %lld samples: outside the decoder's scope", fs.info.channels,
                         fs.info.bits_per_sample, (long long)fs.info.total_samples);
    const long long total = fs.info.total_samples;
    const int ch = fs.info.channels;
    if (total * ch > cap_samples) return set_error(WLX_ERR_ARG, "output buffer too small");
    std::vector<int> status(fs.frames.size());          // (declared before S: it outlives the stream's copies on every return path)
    HookScope S;
    CKR(S.begin(device));
    FlacDev d{};
    const size_t need = flac_layout(fs, n_bytes, nullptr, &d);
    unsigned char* base = nullptr;
    CKR(S.alloc(&base, need));
    (void)flac_layout(fs, n_bytes, base, &d);
    CKR(flac_launch<int32_t>(fs, bytes, n_bytes, d, nullptr, S.st, nullptr));
    CKR(S.download(status.data(), d.status, status.size()));
    CKR(S.download(samples_out, static_cast<const int32_t*>(d.frames), (size_t)total * ch));
    CKR(S.finish());
    CKR(flac_check_status(status.data(), status.size()));
    *n_frames_out = total;
    *channels_out = ch;
    return WLX_OK;
}
