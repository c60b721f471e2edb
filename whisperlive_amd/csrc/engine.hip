// engine.hip — C-ABI (include/wlx.h) over the gfx950 kernels: weight ingestion/repacking, slots
// (one HIP stream + all scratch per concurrent stream), and the host orchestration of log-mel -> encoder.
// Decode (prefill -> hipGraph-replayed steps): engine_decode.hip; the PCM rings' write side: ring.hip; wlx_debug_* hooks: engine_debug.hip.
#include "engine.h"
#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>

using namespace wlx;

extern "C" int32_t wlx_abi_version(void) { return WLX_ABI_VERSION; }

// Slaney mel filterbank exactly as faster-whisper's FeatureExtractor.get_mel_filters builds it
// (librosa.filters.mel(sr=16000, n_fft=400, n_mels, htk=False, norm="slaney"); float64 math,
// float32 storage). Equals HF audio_utils.mel_filter_bank(201, n, 0, 8000, 16000, "slaney", "slaney").
static void build_mel_filters(int n_mels, std::vector<float>& w, std::vector<int>& range) {
    const int nb = 201;
    std::vector<double> fft(nb), melf(n_mels + 2);
    for (int i = 0; i < nb; ++i) fft[i] = (double)i * 8000.0 / 200.0;
    const double max_mel = 45.245640471924965, f_sp = 200.0 / 3.0, min_log_hz = 1000.0;
    const double min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    const double step = max_mel / (double)(n_mels + 1);   // np.linspace(0, max_mel, n_mels + 2)
    for (int i = 0; i < n_mels + 2; ++i) {
        double m = (i == n_mels + 1) ? max_mel : (double)i * step;
        melf[i] = (m >= min_log_mel) ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
    }
    w.assign((size_t)n_mels * nb, 0.f);
    range.assign((size_t)n_mels * 2, 0);
    for (int i = 0; i < n_mels; ++i) {
        const double fd0 = melf[i + 1] - melf[i], fd1 = melf[i + 2] - melf[i + 1];
        const double enorm = 2.0 / (melf[i + 2] - melf[i]);
        int lo = nb, hi = 0;
        for (int b = 0; b < nb; ++b) {
            const double lower = -(melf[i] - fft[b]) / fd0, upper = (melf[i + 2] - fft[b]) / fd1;
            const double v = std::max(0.0, std::min(lower, upper));
            const float f = (float)((double)(float)v * enorm);
            w[(size_t)i * nb + b] = f;
            if (f != 0.f) { lo = std::min(lo, b); hi = std::max(hi, b + 1); }
        }
        if (lo >= hi) { lo = 0; hi = 0; }
        range[2 * i] = lo; range[2 * i + 1] = hi;
    }
}

static int build_logmel_consts(Engine* e) {
    std::vector<float> win(400), tw(800), filt;
    std::vector<int> range;
    const double PI2 = 6.283185307179586476925286766559;
    for (int i = 0; i < 400; ++i) {
        win[i] = (float)(0.5 - 0.5 * std::cos(PI2 * (double)i / 400.0));   // np.hanning(401)[:-1]
        tw[2 * i] = (float)std::cos(PI2 * (double)i / 400.0);
        tw[2 * i + 1] = (float)std::sin(PI2 * (double)i / 400.0);
    }
    build_mel_filters(e->spec.n_mels, filt, range);
    float *dwin, *dtw, *dfilt; int* drange;
    CKR(dalloc(e->allocs, &dwin, 400, true)); CKR(dalloc(e->allocs, &dtw, 800, true));
    CKR(dalloc(e->allocs, &dfilt, filt.size(), true)); CKR(dalloc(e->allocs, &drange, range.size(), true));
    CKR(upload_sync(dwin, win.data(), 400 * 4));
    CKR(upload_sync(dtw, tw.data(), 800 * 4));
    CKR(upload_sync(dfilt, filt.data(), filt.size() * 4));
    CKR(upload_sync(drange, range.data(), range.size() * 4));
    e->lm.window = dwin; e->lm.twiddle = dtw; e->lm.filters = dfilt; e->lm.frange = drange;
    return WLX_OK;
}

static int engine_load(Engine* e, const wlx_tensor* weights, int n_weights) {
    const wlx_spec& sp = e->spec;
    const int d = sp.d_model, F = sp.ffn, V = sp.vocab;
    std::vector<void*>& A = e->allocs;
    Weights ws;
    CKR(ws.open(weights, n_weights));
    CKR(build_logmel_consts(e));
    const wlx_tensor* t; const float* src;
    auto conv = [&](const char* name, int cin, half_t** W, int* KT) -> int {
        CKR(ws.need(name, {d, cin, 3}, &t));
        CKR(alloc_packed(A, d, 3 * cin, W, KT, true));
        CKR(ws.device_f32(t, &src));
        launch_pack_conv3(src, d, cin, *W, *KT, ws.st);
        return WLX_OK;
    };
    auto positions = [&](const char* name, int rows, float** out) -> int {
        CKR(ws.need(name, {rows, d}, &t));
        CKR(dalloc(A, out, (size_t)rows * d, true));
        CKR(ws.device_f32(t, &src));
        CK(hipMemcpyAsync(*out, src, (size_t)rows * d * 4, hipMemcpyDeviceToDevice, ws.st));
        return WLX_OK;
    };
    // ---- encoder stem
    int KT;
    CKR(conv("model.encoder.conv1.weight", sp.n_mels, &e->conv1_w, &e->conv1_KT));
    CKR(conv("model.encoder.conv2.weight", d, &e->conv2_w, &KT));
    CKR(ws.alloc_vec(A, "model.encoder.conv1.bias", d, &e->conv1_b, true));
    CKR(ws.alloc_vec(A, "model.encoder.conv2.bias", d, &e->conv2_b, true));
    CKR(positions("model.encoder.embed_positions.weight", sp.n_audio_ctx, &e->enc_pos));
    LayerOpts o{/*k_bias=*/false, /*q_scale=*/1.f, /*zero=*/true};
    e->enc.resize(sp.enc_layers);
    for (int l = 0; l < sp.enc_layers; ++l)
        CKR(load_layer(ws, A, "model.encoder.layers." + std::to_string(l) + ".", d, F, o, e->enc[l]));
    CKR(ws.alloc_vec(A, "model.encoder.layer_norm.weight", d, &e->enc_ln_g, true));
    CKR(ws.alloc_vec(A, "model.encoder.layer_norm.bias", d, &e->enc_ln_b, true));
    // ---- decoder
    CKR(ws.need("model.decoder.embed_tokens.weight", {V, d}, &t));
    CKR(dalloc(A, &e->tok_emb16, (size_t)V * d, true));
    CKR(ws.device_f32(t, &src));
    launch_f32_to_f16(src, e->tok_emb16, (long)V * d, ws.st);
    CKR(alloc_packed(A, V, d, &e->Wvocab, &KT, true));
    launch_pack_linear(src, V, d, d, e->Wvocab, KT, 0, ws.st);   // tied output projection
    CKR(positions("model.decoder.embed_positions.weight", sp.n_text_ctx, &e->dec_pos));
    CKR(alloc_packed(A, (int64_t)sp.dec_layers * 2 * d, d, &e->Wckv, nullptr, true));
    CKR(dalloc(A, &e->bckv, (size_t)sp.dec_layers * 2 * d, true));
    o.Wckv = e->Wckv; o.bckv = e->bckv;
    e->dec.resize(sp.dec_layers);
    for (o.l = 0; o.l < sp.dec_layers; ++o.l)
        CKR(load_layer(ws, A, "model.decoder.layers." + std::to_string(o.l) + ".", d, F, o, e->dec[o.l]));
    CKR(ws.alloc_vec(A, "model.decoder.layer_norm.weight", d, &e->dec_ln_g, true));
    CKR(ws.alloc_vec(A, "model.decoder.layer_norm.bias", d, &e->dec_ln_b, true));
    return ws.finish();
}

// The process holds device memory that PyTorch (or another runtime) manages — a weight tensor arrived with on_device = 1: the
// embedder issues NULL-stream work of its own (engine.py itself converts weight tensors with torch on the device), and the CU-mask
// constructor only builds BLOCKING streams, which synchronise implicitly with the NULL stream: a second engine loading while a slot
// captures its step graph invalidates the capture (include/wlx.h). With no WLX_SLOT_CU_MASK in the environment such a process gets
// ordinary non-blocking streams.
static std::atomic<bool> g_embedded_device_memory{false};
extern "C" int32_t wlx_engine_create(const wlx_spec* spec, const wlx_tensor* weights, int32_t n_weights,
                                     int32_t device, wlx_engine** out) {
    if (!spec || !weights || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (spec->d_model % 64 || spec->d_model / 64 != spec->n_heads)
        return set_error(WLX_ERR_ARG, "d_model must be 64*n_heads");
    if (spec->d_model % 128 || spec->d_model > 1536) return set_error(WLX_ERR_ARG, "d_model must be a multiple of 128, <= 1536");
    if (spec->ffn % 128) return set_error(WLX_ERR_ARG, "ffn must be a multiple of 128");
    if (spec->n_mels != 80 && spec->n_mels != 128) return set_error(WLX_ERR_ARG, "n_mels must be 80 or 128");
    if (spec->n_audio_ctx != WLX_T_AUDIO || spec->n_text_ctx != WLX_T_TEXT)
        return set_error(WLX_ERR_ARG, "n_audio_ctx/n_text_ctx must be 1500/448");
    if (spec->vocab > 1024 * 52) return set_error(WLX_ERR_ARG, "vocab too large");
    int ndev = 0;
    CK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(WLX_ERR_ARG, "device %d out of range (%d)", device, ndev);
    CK(hipSetDevice(device));
    if (int pe = gemm_prepare_device()) return set_error(WLX_ERR_HIP, "GEMM kernel set-up failed on device %d (hip error %d)", device, pe);
    wlx_engine* e = new wlx_engine();
    e->spec = *spec;
    e->device = device;
    e->H = spec->n_heads;
    for (int i = 0; i < n_weights; ++i)
        if (weights[i].on_device) { g_embedded_device_memory.store(true); break; }
    const char* ng = getenv("WLX_NO_GRAPH");
    e->use_graph = !(ng && ng[0] == '1');
    const char* v1 = wlx_ab("WLX_DECODE_V1");
    g_decode_v1 = (v1 && v1[0] == '1');
    int rc = engine_load(e, weights, n_weights);
    if (rc != WLX_OK) {
        for (void* p : e->allocs) (void)hipFree(p);
        delete e;
        return rc;
    }
    *out = e;
    return WLX_OK;
}

// live slots per device that may hold a hardware queue of their own (WLX_DEDICATED_QUEUES, default 4 = the reference server's
// max_clients); the SAME number is the demotion threshold: one more live slot and every slot goes back to the shared pool
static int max_dedicated_queues() {
    static const int v = [] { const char* e = getenv("WLX_DEDICATED_QUEUES"); return e ? atoi(e) : 4; }();
    return v;
}
std::atomic<int> wlx::g_dedicated_live[64];        // live slots with a hardware queue of their own, per device (create_slot_stream)
std::atomic<int> wlx::g_slots_live[64];            // live slots per device
static std::atomic<bool> g_demote[64];             // more live slots than dedicated queues allowed: dedicated slots fall back at their next call
static std::atomic<unsigned> g_promote_epoch[64];  // raised when g_demote falls: a shared-pool slot tries ONCE per epoch to take a queue of its own
static void slot_free(Slot* s) {
    if (!s) return;
    if (s->device_of >= 0 && s->device_of < 64) {
        if (s->dedicated_queue) g_dedicated_live[s->device_of].fetch_sub(1);
        if (s->counted && g_slots_live[s->device_of].fetch_sub(1) - 1 <= max_dedicated_queues()) {
            if (g_demote[s->device_of].exchange(false)) g_promote_epoch[s->device_of].fetch_add(1);
        }
    }
    if (s->align_scores) (void)hipFree(s->align_scores);
    if (s->align_post) (void)hipFree(s->align_post);
    if (s->flac.buf) (void)hipFree(s->flac.buf);
    for (hipEvent_t ev : s->flac.ev) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {s->ev_al0, s->ev_al1, s->ev_al2}) if (ev) (void)hipEventDestroy(ev);
    for (auto& kv : s->graphs) (void)hipGraphExecDestroy(kv.second);
    for (void* p : s->allocs) (void)hipFree(p);
    for (void* p : s->host_allocs) (void)hipHostFree(p);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->ev_lm0) (void)hipEventDestroy(s->ev_lm0);
    if (s->ev_lm1) (void)hipEventDestroy(s->ev_lm1);
    if (s->ev_en0) (void)hipEventDestroy(s->ev_en0);
    if (s->ev_en1) (void)hipEventDestroy(s->ev_en1);
    for (hipEvent_t ev : s->rs.copied) if (ev) (void)hipEventDestroy(ev);
    if (s->ck_staged) (void)hipEventDestroy(s->ck_staged);
    if (s->ev_sel) (void)hipEventDestroy(s->ev_sel);
    if (s->ev_pcm) (void)hipEventDestroy(s->ev_pcm);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" void wlx_engine_destroy(wlx_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (Slot* s : e->slots) slot_free(s);
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
}

extern "C" int32_t wlx_engine_spec(const wlx_engine* e, wlx_spec* out) {
    if (!e || !out) return set_error(WLX_ERR_ARG, "null argument");
    *out = e->spec;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// slots
static bool dedicated_streams_possible();
int wlx::slot_acquire(wlx_engine* e, int slot, SlotGuard& g) {
    if (!e) return set_error(WLX_ERR_ARG, "null engine");
    Slot* s = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (slot < 0 || slot >= (int)e->slots.size() || !e->slots[slot]) return set_error(WLX_ERR_ARG, "bad slot %d", slot);
        s = e->slots[slot];
        if (!s->call_mu.try_lock())
            return set_error(WLX_ERR_STATE, "slot %d is busy in another call (a slot serves one call at a time)", slot);
        g.s = s;
    }
    // From here on the slot is ours (call_mu) and the engine mutex is released: a stream swap below waits for the slot's own
    // stream, which must not keep other slots out of the library.
    const int dv = s->device_of;
    if (dv < 0 || dv >= 64) return WLX_OK;
    // more slots than dedicated hardware queues exist on this device now: give the queue back (see create_slot_stream: past
    // ~6 busy hardware queues everything collapses; eight ordinary streams over the shared pool run at 1883 xRT, eight with
    // four dedicated queues at 1145). The slot's captured graphs do not depend on the stream they were captured on.
    // ... or the process has since become an embedder of another runtime's device memory (a later engine's weights arrived as device
    // pointers: g_embedded_device_memory): the CU-mask streams are BLOCKING streams and that runtime's NULL-stream work would invalidate
    // this slot's captures, so a slot created before that engine gives its stream back at its next call too (the flag was
    // read at stream creation only).
    if (s->dedicated_queue && (g_demote[dv].load() || !dedicated_streams_possible())) {
        hipStream_t ns = nullptr;
        if (hipSetDevice(dv) == hipSuccess && hipStreamSynchronize(s->stream) == hipSuccess &&
            hipStreamCreateWithFlags(&ns, hipStreamNonBlocking) == hipSuccess) {
            (void)hipStreamDestroy(s->stream);
            s->stream = ns;
            s->dedicated_queue = false;
            g_dedicated_live[dv].fetch_sub(1);
        } else {
            (void)hipGetLastError();
        }
    } else if (!s->dedicated_queue && s->counted && !g_demote[dv].load() && dedicated_streams_possible() &&
               s->promote_epoch != g_promote_epoch[dv].load() && g_dedicated_live[dv].load() < max_dedicated_queues()) {
        // ... and back: the device is down to <= WLX_DEDICATED_QUEUES live slots again (the fifth client left, a batch
        // lane was released) — a slot that was demoted, or created while the device was crowded, takes a queue of its own at its
        // next call. ONE attempt per slot and per "crowd left" event (g_promote_epoch, raised where g_demote falls): with
        // WLX_SLOT_CU_MASK=off, or where the dedicated constructor fails, the steady state costs nothing — the unconditional form
        // synchronised the slot stream and created + destroyed a stream on EVERY call.
        s->promote_epoch = g_promote_epoch[dv].load();
        hipStream_t ns = nullptr;
        bool ded = false;
        if (hipSetDevice(dv) == hipSuccess && hipStreamSynchronize(s->stream) == hipSuccess &&
            create_slot_stream(dv, &ns, &ded) == WLX_OK) {
            if (ded) { (void)hipStreamDestroy(s->stream); s->stream = ns; s->dedicated_queue = true; }
            else (void)hipStreamDestroy(ns);
        } else {
            (void)hipGetLastError();
        }
    }
    return WLX_OK;
}

// ---- PcmLease (engine.h): the slot half, and what both halves share. The ring half is in ring.hip.
int PcmLease::same_device(const char* who, const char* what, int device, const char* reader, int reader_device) {
    return device == reader_device ? WLX_OK : set_error(WLX_ERR_ARG, "%s: the %s lives on device %d, the %s on %d", who, what, device, reader, reader_device);
}

int PcmLease::open_slot(wlx_engine* e, int slot) { return slot_acquire(e, slot, sg_); }

int PcmLease::item(const char* who, int first, int count) {
    if (first < 0 || first + (int64_t)count > sg_.s->B)
        return set_error(WLX_ERR_ARG, "%s: items [%d, %lld) outside the slot's %d", who, first, (long long)first + count, sg_.s->B);
    view(first);
    return WLX_OK;
}

void PcmLease::view(int item) {
    const Slot* s = sg_.s;
    item_ = item;
    buf = s->pcm ? s->pcm + (size_t)item * s->pcm_cap : nullptr;
    base = 0, resident = s->npcm[item];
}

int PcmLease::range(const char* who, int64_t start, int64_t n, const float** p) const {
    if (start >= base && start - base <= resident - n) {
        if (p) *p = buf + (start - base);
        return WLX_OK;
    }
    const long long a = start, b = start + n;
    return r_ ? set_error(WLX_ERR_STATE, "%s: [%lld, %lld) is not resident (ring holds [%lld, %lld))", who, a, b, (long long)base, (long long)(base + resident))
              : set_error(WLX_ERR_STATE, "%s: [%lld, %lld) is not resident (item %d holds %lld samples)", who, a, b, item_, (long long)resident);
}

// whatever wrote the PCM on the slot's stream is finished before the reader's launches read it (wlx_pcm_put_frames returns behind its
// resample launches). The device is set.
int PcmLease::order(hipStream_t reader) {
    Slot* s = sg_.s;
    if (!s) return WLX_OK;
    if (!s->ev_pcm) CK(hipEventCreateWithFlags(&s->ev_pcm, hipEventDisableTiming));
    CK(hipEventRecord(s->ev_pcm, s->stream));
    CK(hipStreamWaitEvent(reader, s->ev_pcm, 0));
    return WLX_OK;
}

int wlx::slot_grow_audio(Engine* e, Slot* s, size_t n_samples) {
    if (n_samples <= s->pcm_cap) return WLX_OK;
    // grow PCM + feature buffers (sizes rounded up to whole 30 s windows)
    size_t cap = ((n_samples + 479999) / 480000) * 480000;
    CK(hipStreamSynchronize(s->stream));
    float* npcm; float* nfe;
    long ld = (long)(cap / 160 + 64);
    CKR(dalloc(s->allocs, &npcm, (size_t)s->B * cap, false));
    CKR(dalloc(s->allocs, &nfe, (size_t)s->B * e->spec.n_mels * ld, true));
    // (old buffers stay in the pool until slot destruction; growth is rare: 1-2 times per stream)
    if (s->pcm_cap) {
        // keep what the other items of a batch already hold: a batched encode runs log-mel item by item, and a later,
        // longer item must not wipe the earlier items' PCM / features / frame counts
        CK(hipMemcpy2DAsync(npcm, cap * sizeof(float), s->pcm, s->pcm_cap * sizeof(float), s->pcm_cap * sizeof(float),
                            (size_t)s->B, hipMemcpyDeviceToDevice, s->stream));
        CK(hipMemcpy2DAsync(nfe, (size_t)ld * sizeof(float), s->feats, (size_t)s->feat_ld * sizeof(float),
                            (size_t)s->feat_ld * sizeof(float), (size_t)s->B * e->spec.n_mels, hipMemcpyDeviceToDevice, s->stream));
        CK(hipStreamSynchronize(s->stream));
    }
    s->pcm = npcm; s->pcm_cap = cap; s->feats = nfe; s->feat_ld = ld;
    return WLX_OK;
}

// A slot's stream gets a HARDWARE QUEUE OF ITS OWN. HIP multiplexes ordinary streams round robin over GPU_MAX_HW_QUEUES = 4
// hardware queues (the null stream and this library's utility stream take two of them), so with four concurrent clients two
// slots shared one queue and their decode chains serialised: 4 streams ran at 1826 xRT. A stream created through
// hipExtStreamCreateWithCUMask owns its queue (the CU mask is a property of the queue) — here with EVERY CU enabled, so
// nothing is restricted: 2734 xRT for the same four streams, single stream unchanged (profiles/r3b_streams4_*.json,
// profiles/r3b_streams4_dedicated_queues_overlap.txt). Raising GPU_MAX_HW_QUEUES instead is NOT an option: 5, 6 and 8 run the
// same workload at 610-640 xRT. WLX_SLOT_CU_MASK=off restores ordinary streams; =stride4 / contig4 give slot k a quarter of
// the CUs (every 4th CU: a decode step is as fast on 64 CUs spread over all XCDs as on 256 — 373 us — but the encoder is not).
// Only the first WLX_DEDICATED_QUEUES (4 = the reference server's max_clients) live slots of a device get one: with 8 dedicated
// queues (+ the null and utility streams' two) the same 8-stream workload drops from 1883 xRT (shared queues) to 1135 — past
// some number of busy hardware queues the command processor time-slices them (profiles/r3c_bench_s8_default.json).
static std::string slot_stream_mode() {
    static const char* cu_mode = getenv("WLX_SLOT_CU_MASK");
    if (cu_mode) return cu_mode;
    return g_embedded_device_memory.load() ? "off" : "full";
}
static bool dedicated_streams_possible() { return slot_stream_mode() != "off" && max_dedicated_queues() > 0; }
int wlx::create_slot_stream(int device, hipStream_t* out, bool* dedicated_out) {
    const int max_dedicated = max_dedicated_queues();
    static std::atomic<int> slot_seq{0};
    std::string m = slot_stream_mode();
    {   // once per process AND MODE: which kind of stream the slots get (the default synchronises implicitly with the NULL
        // stream; r05: the mode can change when an engine brings device-resident weights — say so again then)
        static std::atomic<int> said{0};
        const int bit = (m == "off") ? 1 : 2;
        if (!(said.fetch_or(bit) & bit) && getenv("WLX_QUIET") == nullptr)
            fprintf(stderr, "[wlx] slot streams: WLX_SLOT_CU_MASK=%s%s, up to %d hardware queues per device%s\n", m.c_str(),
                    (m == "off" && g_embedded_device_memory.load()) ? " (weights were handed over as device pointers of another runtime: non-blocking streams unless the variable says otherwise)" : "",
                    max_dedicated,
                    m == "off" ? "" : " (CU-mask streams are blocking streams: keep NULL-stream work of this process off the device, or set WLX_SLOT_CU_MASK=off)");
    }
    *dedicated_out = false;
    if (m != "off") {
        if (device < 0 || device >= 64 || g_dedicated_live[device].fetch_add(1) >= max_dedicated) {
            if (device >= 0 && device < 64) g_dedicated_live[device].fetch_sub(1);
            m = "off";
        } else {
            *dedicated_out = true;
        }
    }
    auto undo = [&] { if (*dedicated_out) { g_dedicated_live[device].fetch_sub(1); *dedicated_out = false; } };
    if (m == "prio_high" || m == "prio_alt") {
        // (A/B) priority streams draw their hardware queues from a per-priority pool, separate from the normal-priority pool
        // the null and utility streams live in, and — unlike the CU-mask constructor — take the non-blocking flag
        int lo = 0, hi = 0;
        CK(hipDeviceGetStreamPriorityRange(&lo, &hi));          // numerically lower = higher priority
        const int k = slot_seq.fetch_add(1);
        const int pr = (m == "prio_alt" && (k & 1)) ? lo : hi;
        if (hipStreamCreateWithPriority(out, hipStreamNonBlocking, pr) == hipSuccess) return WLX_OK;
        (void)hipGetLastError();
        undo();
    } else if (m != "off") {
        hipDeviceProp_t prop;
        CK(hipGetDeviceProperties(&prop, device));
        const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
        const int k = slot_seq.fetch_add(1);
        std::vector<uint32_t> mask(words, 0u);
        const int parts = (m == "contig2") ? 2 : ((m == "stride4" || m == "contig4") ? 4 : 1);
        for (int cu = 0; cu < ncu; ++cu) {
            const bool mine = (m == "stride4") ? (cu % parts == k % parts) : (cu * parts / ncu == k % parts);
            if (mine) mask[cu >> 5] |= 1u << (cu & 31);
        }
        if (hipExtStreamCreateWithCUMask(out, (uint32_t)words, mask.data()) == hipSuccess) return WLX_OK;
        (void)hipGetLastError();           // not supported here: an ordinary stream (shared queues) is still correct
        undo();
    }
    CK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return WLX_OK;
}

// one working set of the decoder pass: `rows` scratch rows and row-table entries, cross-attention partials for `groups` groups
static int alloc_decbufs(Engine* e, Slot* s, DecBufs& b, size_t rows, size_t groups, bool prefill) {
    const size_t d = e->spec.d_model, F = e->spec.ffn, group_items = prefill ? groups : rows;   // (the step set's group table has always held a row's worth)
    b.slab_rows = (int)rows; b.prefill = prefill;
    CKR(dalloc(s->allocs, &b.xd, rows * d, true)); CKR(dalloc(s->allocs, &b.qd, rows * d, true)); CKR(dalloc(s->allocs, &b.attnd, rows * d, true));
    CKR(dalloc(s->allocs, &b.hd, rows * F, true)); CKR(dalloc(s->allocs, &b.slab, (size_t)WLX_FC2_KS * rows * d, true));
    CKR(dalloc(s->allocs, &b.part_o, groups * e->H * WLX_XSPLIT * 16 * 64, true));
    CKR(dalloc(s->allocs, &b.part_ml, groups * e->H * WLX_XSPLIT * 16 * 2, true));
    CKR(dalloc(s->allocs, &b.d_token, rows, true)); CKR(dalloc(s->allocs, &b.d_pos, rows, true)); CKR(dalloc(s->allocs, &b.d_cache, rows, true));
    CKR(dalloc(s->allocs, &b.d_ancrow, rows, true)); CKR(dalloc(s->allocs, &b.d_group_item, group_items, true));
    return WLX_OK;
}

extern "C" int32_t wlx_slot_create(wlx_engine* e, int32_t max_batch, int32_t max_rows_per_item, int32_t* slot_out) {
    if (!e || !slot_out) return set_error(WLX_ERR_ARG, "null argument");
    if (max_batch < 1 || max_batch > 64) return set_error(WLX_ERR_ARG, "max_batch out of range");
    if (max_rows_per_item < 1 || max_rows_per_item > 16) return set_error(WLX_ERR_ARG, "max_rows_per_item must be 1..16");
    if (max_batch * max_rows_per_item > WLX_MAX_DEC_ROWS) return set_error(WLX_ERR_ARG, "max_batch*max_rows_per_item must be <= %d", WLX_MAX_DEC_ROWS);
    CK(hipSetDevice(e->device));
    const wlx_spec& sp = e->spec;
    const int d = sp.d_model, F = sp.ffn, L = sp.dec_layers, B = max_batch, R = max_rows_per_item;
    {   // what the slot will hold (its large terms), checked against the device BEFORE the first allocation (--batch_max_size 64
        // builds 64 x 5-row slots — ~11 GB per lane for Whisper-small, ~45 GB for large-v3 — and used to fail, if at all, deep inside
        // the allocation list with a bare hipMalloc error)
        const double TBd = (double)B * WLX_T_AUDIO, rows = (double)std::max(64, B * R);
        const double bytes = 2.0 * B * 480000 * 4 + (double)B * ((WLX_N_FRAMES + 2) * (sp.n_mels * 2.0 + d * 2.0)) +       // PCM + features, window, conv
                             TBd * d * (4 + 2 + 2 + 2 + 2 + 4) + 2.0 * B * WLX_T_AUDIO_PAD * d * 2 + TBd * F * 2 +            // encoder activations
                             2.0 * L * B * WLX_T_AUDIO_PAD * d * 2 +                                                           // cross K / V
                             2.0 * L * (double)B * R * WLX_T_TEXT * d * 2 +                                                     // self-attention KV cache
                             rows * (((sp.vocab + 15) / 16) * 16 * 4.0 + d * 8.0 + F * 2.0) + (double)WLX_T_TEXT * (d * 16.0 + F * 2.0);   // logits, step + prefill rows
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (bytes > (double)free_b)
                return set_error(WLX_ERR_NOMEM, "a slot of %d items x %d rows needs ~%.1f GB of device memory (encoder activations, cross K/V, KV cache, logits); "
                            "%.1f GB are free on device %d: lower max_batch (--batch_max_size) or the number of lanes", B, R, bytes / 1e9, free_b / 1e9, e->device);
        } else (void)hipGetLastError();
        if (bytes > 8e9 && getenv("WLX_QUIET") == nullptr)
            fprintf(stderr, "[wlx] slot of %d items x %d rows: ~%.1f GB of device memory\n", B, R, bytes / 1e9);
    }
    Slot* s = new Slot();
    s->B = B; s->R = R; s->cache_rows = B * R; s->rows_cap = std::max(64, B * R); s->groups_cap = std::max(B, 4);
    s->nframes.assign(B, 0);
    s->npcm.assign(B, 0);
    int rc = [&]() -> int {
        s->device_of = e->device;
        if (e->device >= 0 && e->device < 64) {
            s->counted = true;
            s->promote_epoch = g_promote_epoch[e->device].load();
            if (g_slots_live[e->device].fetch_add(1) + 1 > max_dedicated_queues()) g_demote[e->device].store(true);
        }
        if (s->counted && g_demote[e->device].load()) {
            CK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));        // past 4 live slots: the shared pool
        } else {
            CKR(create_slot_stream(e->device, &s->stream, &s->dedicated_queue));
        }
        CK(hipEventCreate(&s->ev0)); CK(hipEventCreate(&s->ev1));
        CK(hipEventCreate(&s->ev_lm0)); CK(hipEventCreate(&s->ev_lm1));
        CK(hipEventCreate(&s->ev_en0)); CK(hipEventCreate(&s->ev_en1));
        CKR(slot_grow_audio(e, s, 480000));
        CKR(dalloc(s->allocs, &s->gmax, (size_t)B, true));
        CKR(dalloc(s->allocs, &s->d_rng, (size_t)2 * WLX_LM_MAXRANGES, true));
        s->featT_stride = (long)(WLX_N_FRAMES + 2) * sp.n_mels + 64;
        s->h1_stride = (long)(WLX_N_FRAMES + 2) * d;
        CKR(dalloc(s->allocs, &s->featT, (size_t)B * s->featT_stride, true));
        CKR(dalloc(s->allocs, &s->h1, (size_t)B * s->h1_stride, true));
        const size_t TB = (size_t)B * WLX_T_AUDIO;
        CKR(dalloc(s->allocs, &s->x, TB * d, true));
        CKR(dalloc(s->allocs, &s->ln, TB * d, true));
        CKR(dalloc(s->allocs, &s->q, TB * d, true));
        CKR(dalloc(s->allocs, &s->k, (size_t)B * WLX_T_AUDIO_PAD * d, true));
        CKR(dalloc(s->allocs, &s->vt, (size_t)B * d * WLX_T_AUDIO_PAD, true));
        CKR(dalloc(s->allocs, &s->attn, TB * d, true));
        CKR(dalloc(s->allocs, &s->h2, TB * F, true));
        CKR(dalloc(s->allocs, &s->enc16, TB * d, true));
        CKR(dalloc(s->allocs, &s->enc32, TB * d, true));
        CKR(dalloc(s->allocs, &s->ck, (size_t)L * B * WLX_T_AUDIO_PAD * d, true));
        CKR(dalloc(s->allocs, &s->cvt, (size_t)L * B * d * WLX_T_AUDIO_PAD, true));
        CKR(dalloc(s->allocs, &s->kc, (size_t)L * s->cache_rows * WLX_T_TEXT * d, true));
        CKR(dalloc(s->allocs, &s->vc, (size_t)L * s->cache_rows * WLX_T_TEXT * d, true));
        const int RC = s->rows_cap;
        CKR(alloc_decbufs(e, s, s->step, (size_t)RC, (size_t)s->groups_cap, false));
        {   // the prompt prefill's working set: up to WLX_T_TEXT rows (engine_decode.hip prefill_tokens, gen_prefill)
            CKR(alloc_decbufs(e, s, s->pf, (size_t)WLX_T_TEXT, (size_t)(WLX_T_TEXT + 15) / 16, true));
            // usable when every projection of this model takes the lean kernel in row chunks (d_model a multiple of 256, ...)
            GemvParams q{};
            static const float dummy_bias = 0.f;
            q.M = 96; q.bias = &dummy_bias; q.xsrc = GEMV_X_PLAIN;
            auto lean = [&](int in, int out, int N, int K) { q.in_mode = in; q.out_mode = out; q.N = N; q.K = K; q.KT = K / 32; return dec_gemv_is_lean(q); };
            s->pf_ok = lean(GEMV_IN_LN, GEMV_OUT_QKV, 3 * d, d) && lean(GEMV_IN_F16, GEMV_OUT_RESID, d, d) && lean(GEMV_IN_LN, GEMV_OUT_F16, d, d) &&
                       lean(GEMV_IN_LN, GEMV_OUT_GELU_F16, F, d) && lean(GEMV_IN_F16, GEMV_OUT_RESID, d, F);
        }
        s->ldl = ((sp.vocab + 15) / 16) * 16;
        CKR(dalloc(s->allocs, &s->logits, (size_t)RC * s->ldl, true));
        const int CR = std::max(s->cache_rows, RC);
        CKR(dalloc(s->allocs, &s->d_anc, (size_t)CR * WLX_T_TEXT, true));
        CKR(dalloc(s->allocs, &s->d_intok, (size_t)CR * WLX_T_TEXT, true));
        SearchState& st = s->st;
        CKR(dalloc(s->allocs, &st.step, 1, true)); CKR(dalloc(s->allocs, &st.done, 1, true)); CKR(dalloc(s->allocs, &st.n_finished, 1, true));
        CKR(dalloc(s->allocs, &st.item_done, (size_t)B, true)); CKR(dalloc(s->allocs, &st.plen, (size_t)B, true));
        CKR(dalloc(s->allocs, &st.cum, (size_t)RC, true)); CKR(dalloc(s->allocs, &st.row_done, (size_t)RC, true));
        CKR(dalloc(s->allocs, &st.cand_score, (size_t)RC * WLX_MAX_CAND, true));
        CKR(dalloc(s->allocs, &st.cand_tok, (size_t)RC * WLX_MAX_CAND, true));
        CKR(dalloc(s->allocs, &st.samp_tok, (size_t)RC, true)); CKR(dalloc(s->allocs, &st.samp_lp, (size_t)RC, true));
        // the results of a generate live in pinned host memory (round 6, search.hip finish_item): the update kernels store them there and the host
        // reads them when it sees the done word — no copies, no wait for the step that is already in flight behind the finish
        {
            const size_t ints = (size_t)B * (2 + 2 * WLX_MAX_HYP + (size_t)WLX_MAX_HYP * WLX_T_TEXT);
            CKR(halloc(s->host_allocs, &s->h_hyp, ints));
            memset(s->h_hyp, 0, ints * sizeof(int));
            s->max_items = B;
            CKR(halloc(s->host_allocs, &s->h_pf, (size_t)(5 * WLX_T_TEXT + 64)));
            st.n_hyp_host = s->h_hyp;
            st.hyp_len = st.n_hyp_host + B;
            st.hyp_score = reinterpret_cast<float*>(st.hyp_len + (size_t)B * WLX_MAX_HYP);
            st.no_speech = st.hyp_score + (size_t)B * WLX_MAX_HYP;
            st.hyp_tokens = reinterpret_cast<int*>(st.no_speech + B);
        }
        CKR(dalloc(s->allocs, &st.n_hyp, (size_t)B, true));
        CKR(dalloc(s->allocs, &st.nsp_row, (size_t)RC, true));
        st.token = s->step.d_token; st.pos = s->step.d_pos; st.anc = s->d_anc; st.intok = s->d_intok;
        CKR(dalloc(s->allocs, &st.scan_stats, (size_t)RC * SC_MAXCH * SC_NSTAT, true));
        CKR(dalloc(s->allocs, &st.scan_cv, (size_t)RC * (SC_MAXCH + 1) * WLX_MAX_CAND, true));
        CKR(dalloc(s->allocs, &st.scan_ci, (size_t)RC * (SC_MAXCH + 1) * WLX_MAX_CAND, true));
        CKR(dalloc(s->allocs, &st.rule, (size_t)RC * 4, true));
        CKR(dalloc(s->allocs, &s->d_align_tgt, (size_t)WLX_T_TEXT, true));
        CKR(dalloc(s->allocs, &s->d_align_prob, (size_t)WLX_T_TEXT, true));
        CKR(dalloc(s->allocs, &s->d_sp, 1, true));
        CKR(dalloc(s->allocs, &s->d_suppress, (size_t)(1024 * 52 / 32), true));
        CKR(dalloc(s->allocs, &s->d_lang_ids, WLX_LANG_MAX, true));
        CKR(dalloc(s->allocs, &s->d_probs, (size_t)B * WLX_LANG_MAX, true));
        CKR(dalloc(s->allocs, &s->d_tokprob, (size_t)RC, true));
        s->h_stage_ints = 1 << 16;
        CKR(halloc(s->host_allocs, &s->h_stage, s->h_stage_ints));
        // the search kernels raise this pinned word themselves when every item is finished (no per-step D2H copy)
        s->st.done_host = s->h_stage + (s->h_stage_ints - 4);
        s->h_gen_bytes = gen_staging(nullptr, RC, B).bytes;         // wlx_generate's pinned set-up staging
        CKR(halloc(s->host_allocs, &s->h_gen, s->h_gen_bytes));
        CK(hipStreamSynchronize(s->stream));      // (allocations were zeroed on the utility stream and waited for in dalloc)
        return WLX_OK;
    }();
    if (rc != WLX_OK) { slot_free(s); return rc; }
    std::lock_guard<std::mutex> g(e->mu);
    // ids are never reused: a stale handle of a destroyed slot must fail ("bad slot"), not reach its successor
    e->slots.push_back(s);
    const int id = (int)e->slots.size() - 1;
    *slot_out = id;
    return WLX_OK;
}

extern "C" int32_t wlx_slot_destroy(wlx_engine* e, int32_t slot) {
    if (!e) return set_error(WLX_ERR_ARG, "null engine");
    Slot* s = nullptr;
    for (;;) {      // wait for a call still running on the slot in another thread (a session being torn down mid-chunk)
        {
            std::lock_guard<std::mutex> g(e->mu);
            if (slot < 0 || slot >= (int)e->slots.size() || !e->slots[slot]) return set_error(WLX_ERR_ARG, "bad slot %d", slot);
            if (e->slots[slot]->call_mu.try_lock()) {
                s = e->slots[slot];
                e->slots[slot] = nullptr;        // no other thread can reach it any more
                break;
            }
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    s->call_mu.unlock();
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(s->stream);
    slot_free(s);
    return WLX_OK;
}

// Log-mel requests are collected and launched together (round 4): wlx_logmel_resident only records the item; the launches — ONE set of
// three kernels for all recorded items — go out in front of the first consumer of the features (wlx_encode, wlx_features_get), of a
// timing read, or of anything that overwrites what a recorded item depends on (its PCM, the audio buffers).
int wlx::flush_logmel(Engine* e, Slot* s) {
    if (s->lm_items.empty()) return WLX_OK;
    CK(hipSetDevice(e->device));
    CK(hipEventRecord(s->ev_lm0, s->stream));
    for (size_t i0 = 0; i0 < s->lm_items.size(); i0 += WLX_LM_MAXB) {
        LogmelBatch lb{};
        for (size_t i = i0; i < s->lm_items.size() && i < i0 + WLX_LM_MAXB; ++i) {
            const int item = s->lm_items[i], k = lb.n_items++;
            const int64_t n = s->npcm[item];
            lb.pcm[k] = s->pcm + (size_t)item * s->pcm_cap; lb.n[k] = (long)n;
            lb.feats[k] = s->feats + (size_t)item * e->spec.n_mels * s->feat_ld; lb.T[k] = (int)((n + 160) / 160);
            lb.gmax[k] = s->gmax + item;
        }
        launch_logmel_batch(lb, e->spec.n_mels, e->lm, s->feat_ld, s->stream);
    }
    s->lm_items.clear();
    CK(hipGetLastError());
    CK(hipEventRecord(s->ev_lm1, s->stream));
    s->lm_pending = true;
    return WLX_OK;
}

extern "C" int32_t wlx_sync(wlx_engine* e, int32_t slot) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    CK(hipSetDevice(e->device));
    CKR(flush_logmel(e, s));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

extern "C" int32_t wlx_timings_get(wlx_engine* e, int32_t slot, wlx_timings* out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!out) return set_error(WLX_ERR_ARG, "null out");
    CKR(flush_logmel(e, s));
    if (s->en_pending) {                      // the last encoder pass
        CK(hipSetDevice(e->device));
        CK(hipEventSynchronize(s->ev_en1));
        CK(hipEventElapsedTime(&s->tm.encode_ms, s->ev_en0, s->ev_en1));
        s->en_pending = false;
    }
    if (s->gen_pending) {                     // the last generate: its results were read from pinned memory without waiting for the stream
        CK(hipSetDevice(e->device));
        CK(hipEventSynchronize(s->ev1));
        CK(hipEventElapsedTime(&s->tm.generate_ms, s->ev0, s->ev1));
        int steps = 0;
        CK(hipMemcpy(&steps, s->st.step, 4, hipMemcpyDeviceToHost));
        s->tm.decode_steps = steps;
        s->gen_pending = false;
    }
    if (s->lm_pending) {                      // the last log-mel launch: waited for here, not in wlx_logmel_resident
        CK(hipSetDevice(e->device));
        CK(hipEventSynchronize(s->ev_lm1));
        CK(hipEventElapsedTime(&s->tm.logmel_ms, s->ev_lm0, s->ev_lm1));
        s->lm_pending = false;
    }
    *out = s->tm;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// log-mel
extern "C" int32_t wlx_pcm_put(wlx_engine* e, int32_t slot, int32_t item, const float* pcm, int64_t n) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!pcm || n <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CK(hipSetDevice(e->device));
    if ((size_t)n > s->pcm_cap || std::find(s->lm_items.begin(), s->lm_items.end(), (int)item) != s->lm_items.end())
        CKR(flush_logmel(e, s));            // a recorded log-mel request reads this item's PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, (size_t)n));
    float* dp = s->pcm + (size_t)item * s->pcm_cap;
    CK(hipMemcpyAsync(dp, pcm, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    CK(hipStreamSynchronize(s->stream));   // the caller's PCM buffer may be reused after return
    s->npcm[item] = n;
    return WLX_OK;
}

// the staging of the file front ends (wlx_pcm_put_frames, wlx_pcm_put_flac): two pinned and two device blocks, for the slot's life
int wlx::slot_resample_stage(Slot* s) {
    if (s->rs_ready) return WLX_OK;
    for (int b = 0; b < 2; ++b) {
        if (!s->rs.pinned[b]) CKR(halloc(s->host_allocs, &s->rs.pinned[b], RS_BLOCK_BYTES));
        if (!s->rs.dev[b]) CKR(dalloc(s->allocs, &s->rs.dev[b], RS_BLOCK_BYTES, false));
        if (!s->rs.copied[b]) CK(hipEventCreateWithFlags(&s->rs.copied[b], hipEventDisableTiming));
    }
    s->rs_ready = true;
    return WLX_OK;
}

// file frames -> 16 kHz mono float32 in the item's PCM buffer (resample.hip): wlx_pcm_put with the conversion, the down-mix and the
// resampler on the device. Everything is validated before the first byte of `frames` is read.
extern "C" int32_t wlx_pcm_put_frames(wlx_engine* e, int32_t slot, int32_t item, const void* frames, int64_t n_frames, int32_t channels,
                                      int32_t sample_format, int32_t sample_rate, int64_t* n_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!frames || n_frames <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    CKR(resample_check_args(frames, n_frames, channels, sample_format, sample_rate));
    if (n_frames > (int64_t)sample_rate * 3600 + sample_rate) return set_error(WLX_ERR_ARG, "audio chunk too long");
    ResamplePlan pl{};
    CKR(resample_plan(e->device, sample_rate, &pl));
    const int64_t n = resample_out_len(pl, n_frames);
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CK(hipSetDevice(e->device));
    if ((size_t)n > s->pcm_cap || std::find(s->lm_items.begin(), s->lm_items.end(), (int)item) != s->lm_items.end())
        CKR(flush_logmel(e, s));            // a recorded log-mel request reads this item's PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, (size_t)n));
    const long long block = resample_default_block(channels, sample_format);
    CKR(slot_resample_stage(s));
    s->npcm[item] = 0;                      // (a failed run leaves no half-written audio resident)
    CKR(resample_run(pl, frames, n_frames, channels, sample_format, block, s->rs, s->pcm + (size_t)item * s->pcm_cap, s->stream, nullptr));
    s->npcm[item] = n;
    if (n_out) *n_out = n;
    return WLX_OK;
}

// the channel-split form (resample.hip): channel c of the file -> item first_item + c, one upload, no down-mix. Everything is validated
// before the first byte of `frames` is read and before any item's PCM is touched.
extern "C" int32_t wlx_pcm_put_frames_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* frames, int64_t n_frames,
                                            int32_t channels, int32_t sample_format, int32_t sample_rate, int64_t* n_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!frames || n_frames <= 0) return set_error(WLX_ERR_ARG, "empty audio");
    CKR(resample_check_args(frames, n_frames, channels, sample_format, sample_rate));
    if (first_item < 0 || (int64_t)first_item + channels > s->B)
        return set_error(WLX_ERR_ARG, "wlx_pcm_put_frames_split: items [%d, %lld) outside the slot's %d", first_item,
                         (long long)first_item + channels, s->B);
    if (n_frames > (int64_t)sample_rate * 3600 + sample_rate) return set_error(WLX_ERR_ARG, "audio chunk too long");
    ResamplePlan pl{};
    CKR(resample_plan(e->device, sample_rate, &pl));
    const int64_t n = resample_out_len(pl, n_frames);
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CK(hipSetDevice(e->device));
    bool recorded = false;
    for (int c = 0; c < channels; ++c)
        recorded = recorded || std::find(s->lm_items.begin(), s->lm_items.end(), first_item + c) != s->lm_items.end();
    if ((size_t)n > s->pcm_cap || recorded)
        CKR(flush_logmel(e, s));            // a recorded log-mel request reads one of these items' PCM (or the buffers are about to be re-allocated)
    CKR(slot_grow_audio(e, s, (size_t)n));
    const long long block = resample_default_block(channels, sample_format);
    CKR(slot_resample_stage(s));
    for (int c = 0; c < channels; ++c) s->npcm[first_item + c] = 0;      // (a failed run leaves no half-written audio resident)
    CKR(resample_run(pl, frames, n_frames, channels, sample_format, block, s->rs, s->pcm + (size_t)first_item * s->pcm_cap, s->stream, nullptr,
                     (long long)s->pcm_cap));
    for (int c = 0; c < channels; ++c) s->npcm[first_item + c] = n;
    if (n_out) *n_out = n;
    return WLX_OK;
}

extern "C" int32_t wlx_pcm_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap, int64_t* n_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    const int64_t n = s->npcm[item];
    if (n_out) *n_out = n;
    if (!out) return WLX_OK;
    if (n <= 0) return set_error(WLX_ERR_STATE, "item %d: no PCM resident", item);
    if (n > cap) return set_error(WLX_ERR_ARG, "output buffer too small");
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(out, s->pcm + (size_t)item * s->pcm_cap, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

// the range reader of a PCM ring, and the asynchronous one: it returns behind its launch (engine.h PcmLease)
extern "C" int32_t wlx_logmel_ring(wlx_engine* e, int32_t slot, int32_t item, wlx_ring* r, const int64_t* ranges, int32_t n_ranges,
                                   int32_t* n_frames_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!r || !ranges || n_ranges < 1) return set_error(WLX_ERR_ARG, "wlx_logmel_ring: bad argument");
    if (n_ranges > WLX_LM_MAXRANGES) return set_error(WLX_ERR_ARG, "wlx_logmel_ring: more than %d ranges", WLX_LM_MAXRANGES);
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    CKR(PcmLease::same_device("wlx_logmel_ring", "ring", r->device, "engine", e->device));
    CK(hipSetDevice(e->device));
    PcmLease L;
    L.open_ring(r);
    long long tab[2 * WLX_LM_MAXRANGES];
    int64_t total = 0, prev_end = L.base;
    for (int i = 0; i < n_ranges; ++i) {
        const int64_t a = ranges[2 * i], b = ranges[2 * i + 1];
        if (a < prev_end || b <= a) return set_error(a < L.base ? WLX_ERR_STATE : WLX_ERR_ARG, "wlx_logmel_ring: range %d = [%lld, %lld) is empty, out of order or no longer resident (ring starts at %lld)",
                                                i, (long long)a, (long long)b, (long long)L.base);
        if (b > L.base + L.resident) return set_error(WLX_ERR_STATE, "wlx_logmel_ring: range %d ends at %lld, the ring at %lld", i, (long long)b, (long long)(L.base + L.resident));
        tab[2 * i] = a - L.base; tab[2 * i + 1] = total;
        total += b - a;
        prev_end = b;
    }
    if (total > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CKR(L.before_launch(s->stream));
    CKR(flush_logmel(e, s));                         // requests recorded earlier go out first (one of them may be this item's)
    CKR(slot_grow_audio(e, s, (size_t)total));       // the feature buffers are sized with the audio buffers
    CK(hipMemcpyAsync(s->d_rng, tab, (size_t)n_ranges * 2 * sizeof(long long), hipMemcpyHostToDevice, s->stream));   // (pageable source: staged before the call returns)
    const int T = (int)((total + 160) / 160);
    LogmelBatch lb{};
    lb.n_items = 1; lb.pcm[0] = L.buf; lb.n[0] = (long)total; lb.feats[0] = s->feats + (size_t)item * e->spec.n_mels * s->feat_ld; lb.T[0] = T;
    lb.gmax[0] = s->gmax + item; lb.rng[0] = s->d_rng; lb.nr[0] = n_ranges;
    CK(hipEventRecord(s->ev_lm0, s->stream));
    launch_logmel_batch(lb, e->spec.n_mels, e->lm, s->feat_ld, s->stream);
    CK(hipGetLastError());
    CK(hipEventRecord(s->ev_lm1, s->stream));
    CKR(L.launched(s->stream));
    s->lm_pending = true;
    s->npcm[item] = 0;                               // the item's own PCM buffer does not hold this audio (wlx_logmel_resident would be wrong)
    s->nframes[item] = T;
    if (n_frames_out) *n_frames_out = T;
    return WLX_OK;
}

// B chunks cut out of resident PCM into B feature items, one launch of each kernel (include/wlx.h): out of ONE item's buffer
// (wlx_logmel_chunks: src_items == nullptr, every chunk reads src_item) or each chunk out of its own source (wlx_logmel_chunks_multi:
// chunk c reads src_items[c]). A slot's PCM is one allocation with row stride pcm_cap, so the multi form hands the kernel the row of the
// LOWEST source as its base and adds (src_items[c] - lowest) * pcm_cap to the chunk's range starts on the host: logmel_chunks_kernel
// only ever adds a range start to its base pointer (its reflections are in the chunk's concatenated coordinates, logmel.hip), so it
// is the same kernel with the same arithmetic. Everything is validated before anything is staged, recorded or launched.
static int logmel_chunks_run(wlx_engine* e, int32_t slot, int32_t src_item, const int32_t* src_items, const int64_t* ranges,
                             const int32_t* range_off, int32_t n_chunks, int32_t first_item, int32_t* n_frames_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    const char* fn = src_items ? "wlx_logmel_chunks_multi" : "wlx_logmel_chunks";
    if (!ranges || !range_off || !n_frames_out || n_chunks < 1) return set_error(WLX_ERR_ARG, "%s: bad argument", fn);
    if (first_item < 0 || first_item + (int64_t)n_chunks > s->B) {
        if (!src_items && (src_item < 0 || src_item >= s->B)) return set_error(WLX_ERR_ARG, "bad item %d", src_item);
        return set_error(WLX_ERR_ARG, "%s: items [%d, %lld) outside the slot's %d", fn, first_item, (long long)first_item + n_chunks, s->B);
    }
    int src_lo = src_item, src_hi = src_item;
    for (int c = 0; c < n_chunks; ++c) {
        const int src = src_items ? src_items[c] : src_item;
        if (src < 0 || src >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", src);
        if (s->npcm[src] <= 0) return set_error(WLX_ERR_STATE, "item %d: no PCM resident (call wlx_pcm_put first)", src);
        src_lo = c == 0 ? src : std::min(src_lo, src);
        src_hi = c == 0 ? src : std::max(src_hi, src);
    }
    int64_t longest = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t resident = s->npcm[src_items ? src_items[c] : src_item];
        const int64_t r0 = range_off[c], nr = (int64_t)range_off[c + 1] - r0;
        if (r0 < 0 || (c == 0 && r0 != 0)) return set_error(WLX_ERR_ARG, "%s: range_off must start at 0 and ascend", fn);
        if (nr < 1 || nr > WLX_LM_MAXRANGES) return set_error(WLX_ERR_ARG, "%s: chunk %d has %lld ranges (1..%d)", fn, c, (long long)nr, WLX_LM_MAXRANGES);
        int64_t total = 0, prev_end = 0;
        for (int64_t i = r0; i < r0 + nr; ++i) {
            const int64_t a = ranges[2 * i], b = ranges[2 * i + 1];
            if (a < prev_end || b <= a) return set_error(WLX_ERR_ARG, "%s: chunk %d range %lld = [%lld, %lld) is empty, out of order or overlaps",
                                                          fn, c, (long long)(i - r0), (long long)a, (long long)b);
            if (b > resident) return set_error(WLX_ERR_STATE, "%s: chunk %d range %lld ends at %lld, the resident PCM at %lld", fn, c,
                                               (long long)(i - r0), (long long)b, (long long)resident);
            total += b - a;
            prev_end = b;
        }
        longest = std::max(longest, total);
    }
    // the kernel keeps a range's physical start as an int offset from its base pointer (logmel.hip rphys): the sources' rows must lie
    // within 2^31 - 1 samples of the lowest one, at the row stride the buffers will have when the launch goes out
    {
        const size_t cap_after = std::max(s->pcm_cap, (((size_t)longest + 479999) / 480000) * 480000);
        if ((uint64_t)(src_hi - src_lo) * cap_after + cap_after > 0x7fffffffull)
            return set_error(WLX_ERR_ARG, "%s: source items %d and %d lie %llu samples apart, past the 2^31 - 1 the chunk kernel addresses "
                             "(use neighbouring source items)", fn, src_lo, src_hi, (unsigned long long)((uint64_t)(src_hi - src_lo) * cap_after));
    }
    CK(hipSetDevice(e->device));
    if (!s->h_chunks) {
        CKR(halloc(s->host_allocs, &s->h_chunks, (size_t)s->B));
        CKR(halloc(s->host_allocs, &s->h_crng, (size_t)s->B * WLX_LM_MAXRANGES * 2));
        CKR(dalloc(s->allocs, &s->d_chunks, (size_t)s->B, true));
        CKR(dalloc(s->allocs, &s->d_crng, (size_t)s->B * WLX_LM_MAXRANGES * 2, true));
        CK(hipEventCreateWithFlags(&s->ck_staged, hipEventDisableTiming));
    }
    CKR(flush_logmel(e, s));                         // requests recorded earlier go out first (they may read or write these items)
    CKR(slot_grow_audio(e, s, (size_t)longest));     // the feature buffers are sized with the audio buffers (the resident PCM moves with them)
    if (s->ck_pending) { CK(hipEventSynchronize(s->ck_staged)); s->ck_pending = false; }   // the previous call's copy has left the pinned tables
    int Tmax = 0, nrows = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int r0 = range_off[c], nr = range_off[c + 1] - r0;
        const long long row = src_items ? (long long)(src_items[c] - src_lo) * (long long)s->pcm_cap : 0;   // the source's row, from the base
        int64_t total = 0;
        for (int i = 0; i < nr; ++i) {
            s->h_crng[2 * (nrows + i)] = row + ranges[2 * (r0 + i)]; s->h_crng[2 * (nrows + i) + 1] = total;
            total += ranges[2 * (r0 + i) + 1] - ranges[2 * (r0 + i)];
        }
        const int T = (int)((total + 160) / 160);
        s->h_chunks[c] = LogmelChunk{(long long)total, T, nrows, nr, first_item + c};
        nrows += nr;
        Tmax = std::max(Tmax, T);
        n_frames_out[c] = T;
    }
    CK(hipMemcpyAsync(s->d_chunks, s->h_chunks, (size_t)n_chunks * sizeof(LogmelChunk), hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->d_crng, s->h_crng, (size_t)nrows * 2 * sizeof(long long), hipMemcpyHostToDevice, s->stream));
    CK(hipEventRecord(s->ck_staged, s->stream));
    s->ck_pending = true;
    CK(hipEventRecord(s->ev_lm0, s->stream));
    launch_logmel_chunks(s->pcm + (size_t)src_lo * s->pcm_cap, s->d_chunks, n_chunks, Tmax, s->d_crng, s->feats,
                         (long)e->spec.n_mels * s->feat_ld, s->gmax, e->spec.n_mels, e->lm, s->feat_ld, s->stream);
    CK(hipGetLastError());
    CK(hipEventRecord(s->ev_lm1, s->stream));
    s->lm_pending = true;
    for (int c = 0; c < n_chunks; ++c) {
        const int item = first_item + c;
        s->nframes[item] = s->h_chunks[c].T;
        bool is_src = item == src_item;
        for (int k = 0; src_items && k < n_chunks && !is_src; ++k) is_src = src_items[k] == item;
        if (!is_src) s->npcm[item] = 0;              // the item's own PCM buffer does not hold this audio; the source(s) stay resident
    }
    return WLX_OK;
}

extern "C" int32_t wlx_logmel_chunks(wlx_engine* e, int32_t slot, int32_t src_item, const int64_t* ranges, const int32_t* range_off,
                                     int32_t n_chunks, int32_t first_item, int32_t* n_frames_out) {
    return logmel_chunks_run(e, slot, src_item, nullptr, ranges, range_off, n_chunks, first_item, n_frames_out);
}

extern "C" int32_t wlx_logmel_chunks_multi(wlx_engine* e, int32_t slot, const int32_t* src_items, const int64_t* ranges, const int32_t* range_off,
                                           int32_t n_chunks, int32_t first_item, int32_t* n_frames_out) {
    if (!src_items) return set_error(WLX_ERR_ARG, "wlx_logmel_chunks_multi: null src_items");
    return logmel_chunks_run(e, slot, -1, src_items, ranges, range_off, n_chunks, first_item, n_frames_out);
}

extern "C" int32_t wlx_logmel_resident(wlx_engine* e, int32_t slot, int32_t item, int32_t* n_frames_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item %d", item);
    const int64_t n = s->npcm[item];
    if (n <= 0) return set_error(WLX_ERR_STATE, "item %d: no PCM resident (call wlx_pcm_put first)", item);
    CK(hipSetDevice(e->device));
    const int T = (int)((n + 160) / 160);
    float* dp = s->pcm + (size_t)item * s->pcm_cap;
    float* df = s->feats + (size_t)item * e->spec.n_mels * s->feat_ld;
    // No launch and no host wait here (round 4): the frame count is a function of the sample count; the request is recorded and goes out
    // together with the other items' (flush_logmel) in front of the first consumer. A batch of 12 windows used to be 36 launches and 12
    // launch -> wait round trips in front of its encoder; the launch's time is read lazily by wlx_timings_get.
    (void)dp; (void)df;
    if (std::find(s->lm_items.begin(), s->lm_items.end(), (int)item) == s->lm_items.end()) s->lm_items.push_back(item);
    s->nframes[item] = T;
    if (n_frames_out) *n_frames_out = T;
    return WLX_OK;
}

extern "C" int32_t wlx_logmel(wlx_engine* e, int32_t slot, int32_t item, const float* pcm, int64_t n,
                              int32_t* n_frames_out) {
    CKR(wlx_pcm_put(e, slot, item, pcm, n));
    return wlx_logmel_resident(e, slot, item, n_frames_out);
}

extern "C" int32_t wlx_features_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap_floats,
                                    int32_t* n_frames_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (item < 0 || item >= s->B) return set_error(WLX_ERR_ARG, "bad item");
    const int T = s->nframes[item], nm = e->spec.n_mels;
    if (n_frames_out) *n_frames_out = T;
    if (!out) return WLX_OK;
    CKR(flush_logmel(e, s));
    if ((int64_t)T * nm > cap_floats) return set_error(WLX_ERR_ARG, "output buffer too small");
    CK(hipSetDevice(e->device));
    const float* df = s->feats + (size_t)item * nm * s->feat_ld;
    CK(hipMemcpy2DAsync(out, (size_t)T * 4, df, (size_t)s->feat_ld * 4, (size_t)T * 4, nm, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

extern "C" int32_t wlx_features_set(wlx_engine* e, int32_t slot, int32_t item, const float* feats,
                                    int32_t n_mels, int32_t n_frames) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (item < 0 || item >= s->B || !feats) return set_error(WLX_ERR_ARG, "bad item / null");
    if (n_mels != e->spec.n_mels || n_frames < 1) return set_error(WLX_ERR_ARG, "features must be [%d, T>=1]", e->spec.n_mels);
    CK(hipSetDevice(e->device));
    CKR(flush_logmel(e, s));                // (a recorded request for this item must not overwrite the features set here)
    CKR(slot_grow_audio(e, s, (size_t)n_frames * 160));
    float* df = s->feats + (size_t)item * n_mels * s->feat_ld;
    CK(hipMemcpy2DAsync(df, (size_t)s->feat_ld * 4, feats, (size_t)n_frames * 4, (size_t)n_frames * 4, n_mels,
                        hipMemcpyHostToDevice, s->stream));
    CK(hipStreamSynchronize(s->stream));
    s->nframes[item] = n_frames;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// encoder
extern "C" int32_t wlx_encode(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* seek, const int32_t* seg) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (batch < 1 || batch > s->B) return set_error(WLX_ERR_ARG, "batch %d out of range (slot max %d)", batch, s->B);
    const wlx_spec& sp = e->spec;
    const int d = sp.d_model, F = sp.ffn, nm = sp.n_mels, H = e->H, T = WLX_T_AUDIO;
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    // (every window validated BEFORE anything is recorded or launched: a refused call must leave the slot's timing events and
    // `en_pending` of the previous encode untouched — ADVICE r04)
    PrepWindows pw{};                       // the windows of the batch: one launch (blockIdx.y = item)
    for (int b = 0; b < batch; ++b) {
        const int sk = seek ? seek[b] : 0;
        int sg = seg ? seg[b] : (s->nframes[b] - sk);
        if (sk < 0 || sg < 0 || sk + sg > s->nframes[b])
            return set_error(WLX_ERR_ARG, "item %d: window [%d,%d) outside %d feature frames", b, sk, sk + sg, s->nframes[b]);
        if (sg > WLX_N_FRAMES) sg = WLX_N_FRAMES;
        pw.seek[b] = sk; pw.seg[b] = sg;
    }
    CKR(flush_logmel(e, s));                // the recorded log-mel requests of the batch: one launch of each kernel
    CK(hipEventRecord(s->ev_en0, st));
    launch_prep_windows(s->feats, s->feat_ld, nm, (long)nm * s->feat_ld, pw, batch, s->featT, (long)s->featT_stride, st);
    GemmParams g{};
    // conv1 (k=3, s=1, p=1) + GELU: K-row of frame t = featT rows t..t+2 (row 0 / 3001 are the zero pad)
    g.A = s->featT; g.lda = nm; g.strideA = s->featT_stride; g.Wp = e->conv1_w; g.KT = e->conv1_KT;
    g.M = WLX_N_FRAMES; g.N = d; g.mode = GEMM_GELU_F16; g.bias = e->conv1_b;
    g.C = s->h1 + d; g.ldc = d; g.strideC = s->h1_stride;
    launch_gemm(g, batch, st);
    // conv2 (k=3, s=2, p=1) + GELU + sinusoidal positions -> fp32 residual stream
    g = GemmParams{};
    g.A = s->h1; g.lda = 2 * d; g.strideA = s->h1_stride; g.Wp = e->conv2_w; g.KT = 3 * d / 32;
    g.M = T; g.N = d; g.mode = GEMM_GELU_POS_F32; g.bias = e->conv2_b;
    g.X = s->x; g.ldx = d; g.strideX = (long)T * d; g.pos = e->enc_pos;
    launch_gemm(g, batch, st);
    const int M = batch * T;
    for (int l = 0; l < sp.enc_layers; ++l) {
        const LayerW& w = e->enc[l];
        launch_layernorm_f16(s->x, d, w.ln1_g, w.ln1_b, s->ln, d, M, d, st);
        g = GemmParams{};
        g.A = s->ln; g.lda = d; g.Wp = w.Wqkv; g.KT = d / 32; g.M = M; g.N = 3 * d; g.mode = GEMM_QKV; g.bias = w.bqkv;
        g.C = s->q; g.ldc = d; g.d = d; g.qscale = 0.125f; g.Kout = s->k; g.ldk = d; g.Vt = s->vt; g.ldvt = WLX_T_AUDIO_PAD;
        g.rows_per_item = T; g.kv_item_stride_k = (long)WLX_T_AUDIO_PAD * d; g.kv_item_stride_v = (long)d * WLX_T_AUDIO_PAD;
        launch_gemm(g, 1, st);
        launch_attn_encoder(s->q, d, s->k, d, s->vt, WLX_T_AUDIO_PAD, s->attn, d, T, H, batch, (long)T * d,
                            (long)WLX_T_AUDIO_PAD * d, (long)d * WLX_T_AUDIO_PAD, (long)T * d, st);
        g = GemmParams{};
        g.A = s->attn; g.lda = d; g.Wp = w.Wo; g.KT = d / 32; g.M = M; g.N = d; g.mode = GEMM_RESID_F32; g.bias = w.bo;
        g.X = s->x; g.ldx = d;
        launch_gemm(g, 1, st);
        launch_layernorm_f16(s->x, d, w.ln3_g, w.ln3_b, s->ln, d, M, d, st);
        g = GemmParams{};
        g.A = s->ln; g.lda = d; g.Wp = w.W1; g.KT = d / 32; g.M = M; g.N = F; g.mode = GEMM_GELU_F16; g.bias = w.b1;
        g.C = s->h2; g.ldc = F;
        launch_gemm(g, 1, st);
        g = GemmParams{};
        g.A = s->h2; g.lda = F; g.Wp = w.W2; g.KT = F / 32; g.M = M; g.N = d; g.mode = GEMM_RESID_F32; g.bias = w.b2;
        g.X = s->x; g.ldx = d;
        launch_gemm(g, 1, st);
    }
    launch_layernorm_f16_f32(s->x, d, e->enc_ln_g, e->enc_ln_b, s->enc16, s->enc32, d, M, d, st);
    // cross-attention K/V of every decoder layer in one GEMM (N = L*2d)
    g = GemmParams{};
    g.A = s->enc16; g.lda = d; g.Wp = e->Wckv; g.KT = d / 32; g.M = M; g.N = sp.dec_layers * 2 * d; g.mode = GEMM_CROSS_KV;
    g.bias = e->bckv; g.d = d; g.Kout = s->ck; g.ldk = d; g.Vt = s->cvt; g.ldvt = WLX_T_AUDIO_PAD; g.rows_per_item = T;
    g.kv_item_stride_k = (long)WLX_T_AUDIO_PAD * d; g.kv_item_stride_v = (long)d * WLX_T_AUDIO_PAD;
    g.kv_layer_stride_k = (long)s->B * WLX_T_AUDIO_PAD * d; g.kv_layer_stride_v = (long)s->B * d * WLX_T_AUDIO_PAD;
    launch_gemm(g, 1, st);
    CK(hipGetLastError());
    CK(hipEventRecord(s->ev_en1, st));
    // No host wait (round 4): everything that consumes the encoder output is ordered on the slot's stream, and the time is read lazily
    // by wlx_timings_get. The caller's next call — wlx_generate's host-side set-up, ~0.3 ms of staging and copies — now overlaps the
    // encoder on the GPU instead of following it.
    s->en_pending = true;
    s->enc_batch = batch;
    return WLX_OK;
}

extern "C" int32_t wlx_encoder_output_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap_floats) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (item < 0 || item >= s->enc_batch) return set_error(WLX_ERR_STATE, "item %d not encoded", item);
    const size_t n = (size_t)WLX_T_AUDIO * e->spec.d_model;
    if (!out || (int64_t)n > cap_floats) return set_error(WLX_ERR_ARG, "output buffer too small");
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(out, s->enc32 + (size_t)item * n, n * 4, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

