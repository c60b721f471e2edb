// spk_engine.hip — the speaker-embedding engine behind `enable_diarization` (include/wlx.h wlx_spk_*): WeSpeaker ResNet34 on the
// kernels of spk.hip. One engine per GPU on a non-blocking stream of its own; every buffer is sized at create for max_seconds of
// audio and fully rewritten by each call up to the extent that call reads, so no call sees another's data. Calls are serialised
// by the engine's mutex. ONE pass (spk_run_batch) serves every entry point: up to WLX_SPK_MAX_BATCH segments as one ragged batch
// through the same buffers (the sum of their lengths is what has to fit max_seconds). wlx_spk_embed is a batch of one;
// wlx_spk_embed_batch uploads its items; wlx_spk_embed_pcm_batch / _ring_batch run the pass on ranges of audio that is already in HBM
// (a slot item's PCM, a client's PCM ring), with no upload. wlx_spk_cluster / wlx_spk_diarize_pcm / wlx_spk_diarize_many cluster
// embeddings on the device (spk_cluster.hip) on ONE path, a file being a wave of one: the passes of the windows of a wave of files in
// different items of one slot enqueued back to back — shared passes, the files clustered side by side — and one wait. Below the engine:
// the one-launch test hooks wlx_spk_debug_fbank / _conv / _pool (one item) and _conv_batch / _pool_batch (ragged), each pair on one
// implementation, as are wlx_spk_debug_affinity / _ahc and their many-forms.
#include <cmath>
#include <mutex>
#include "engine.h"
#include "host.h"
#include "spk.h"

namespace wlx {
namespace {

struct SpkConv {
    half_t* Wp = nullptr;
    float* bias = nullptr;
    int cin = 0, cout = 0, stride = 1, ks = 3;
};
struct SpkBlock {
    SpkConv c1, c2, sc;
    bool has_sc = false;
};

// Kaldi's tables in float64, rounded once: Hamming window, cos(2 pi j / 512), and the triangular mel banks over 20 Hz .. Nyquist on
// the 1127 ln(1 + f / 700) scale, evaluated at the centres of the first 256 FFT bins (the Nyquist bin carries no weight)
void spk_tables(int n_mels, std::vector<float>& window, std::vector<float>& twiddle, std::vector<float>& mel) {
    const double pi = 3.14159265358979323846;
    window.resize(WLX_SPK_FRAME);
    for (int i = 0; i < WLX_SPK_FRAME; ++i) window[i] = (float)(0.54 - 0.46 * std::cos(2.0 * pi * i / (WLX_SPK_FRAME - 1)));
    twiddle.resize(WLX_SPK_NFFT);
    for (int j = 0; j < WLX_SPK_NFFT; ++j) twiddle[j] = (float)std::cos(2.0 * pi * j / WLX_SPK_NFFT);
    auto to_mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double lo = to_mel(20.0), hi = to_mel(8000.0), delta = (hi - lo) / (n_mels + 1), bin_hz = 16000.0 / WLX_SPK_NFFT;
    mel.assign((size_t)n_mels * WLX_SPK_BINS, 0.f);
    for (int b = 0; b < n_mels; ++b) {
        const double left = lo + b * delta, centre = left + delta, right = centre + delta;
        for (int k = 0; k < WLX_SPK_BINS; ++k) {
            const double m = to_mel(bin_hz * k);
            const double up = (m - left) / (centre - left), down = (right - m) / (right - centre);
            mel[(size_t)b * WLX_SPK_BINS + k] = (float)std::max(0.0, std::min(up, down));
        }
    }
}

int upload_tables(std::vector<void*>& pool, int n_mels, float** window, float** twiddle, float** mel) {
    std::vector<float> w, t, m;
    spk_tables(n_mels, w, t, m);
    CKR(dalloc(pool, window, w.size(), false));
    CKR(dalloc(pool, twiddle, t.size(), false));
    CKR(dalloc(pool, mel, m.size(), false));
    CKR(upload_sync(*window, w.data(), w.size() * sizeof(float)));
    CKR(upload_sync(*twiddle, t.data(), t.size() * sizeof(float)));
    return upload_sync(*mel, m.data(), m.size() * sizeof(float));
}

// a named tensor as host floats (a device tensor is copied back on the utility stream)
int fetch(const Weights& ws, const std::string& name, std::initializer_list<int64_t> shape, std::vector<float>& out) {
    const wlx_tensor* t;
    CKR(ws.need(name, shape, &t));
    size_t n = 1;
    for (int64_t s : shape) n *= (size_t)s;
    out.resize(n);
    if (t->on_device) {
        hipStream_t us = util_stream();
        if (!us) return set_error(WLX_ERR_HIP, "utility stream creation failed");
        CK(hipMemcpyAsync(out.data(), t->data, n * sizeof(float), hipMemcpyDeviceToHost, us));
        CK(hipStreamSynchronize(us));
    } else {
        std::copy(reinterpret_cast<const float*>(t->data), reinterpret_cast<const float*>(t->data) + n, out.begin());
    }
    return WLX_OK;
}

int load_conv(const Weights& ws, std::vector<void*>& pool, const std::string& name, int cout, int cin, int ks, int stride, SpkConv& c) {
    std::vector<float> w, b;
    CKR(fetch(ws, name + ".weight", {cout, cin, ks, ks}, w));
    CKR(fetch(ws, name + ".bias", {cout}, b));
    std::vector<half_t> packed(spk_packed_halfs(cout, cin, ks));
    spk_pack_conv(w.data(), cout, cin, ks, packed.data());
    CKR(dalloc(pool, &c.Wp, packed.size(), false));
    CKR(dalloc(pool, &c.bias, b.size(), false));
    CKR(upload_sync(c.Wp, packed.data(), packed.size() * sizeof(half_t)));
    CKR(upload_sync(c.bias, b.data(), b.size() * sizeof(float)));
    c.cin = cin, c.cout = cout, c.ks = ks, c.stride = stride;
    return WLX_OK;
}

}  // namespace
}  // namespace wlx

using namespace wlx;

struct wlx_spk {
    int device = 0;
    wlx_spk_spec spec{};
    hipStream_t st = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::vector<void*> pool;
    std::mutex mu;
    float *window = nullptr, *twiddle = nullptr, *mel = nullptr;
    float *stem_w = nullptr, *stem_b = nullptr, *head_b = nullptr;
    half_t* head_W = nullptr;
    std::vector<SpkBlock> blocks;
    long max_samples = 0;
    int pool_dim = 0;
    // per-call buffers
    float *pcm = nullptr, *logmel = nullptr, *pooled = nullptr, *emb = nullptr;
    half_t* feat16 = nullptr;
    half_t* act[4] = {nullptr, nullptr, nullptr, nullptr};
    float* h_emb = nullptr;          // pinned [WLX_SPK_MAX_BATCH][embed_dim]: where a batch's embeddings land before they are dealt to rows
    float fbank_ms = 0.f, net_ms = 0.f;
    bool timed = false;
    // offline clustering (spk_cluster.hip), allocated by the first call that clusters and shared by all of them (a file is a wave of one):
    // one table of up to WLX_SPK_MANY_MAX_ROWS embeddings the passes write into, the files' distance matrices back to back, results per
    // row / per file, and their pinned landing places
    bool mn_ready = false;
    float *mn_emb = nullptr, *mn_dist = nullptr, *mn_cent = nullptr, *mn_heights = nullptr;
    int *mn_merges = nullptr, *mn_labels = nullptr, *mn_counts = nullptr;
    float *h_mn_emb = nullptr, *h_mn_cent = nullptr;
    int* h_mn_int = nullptr;         // [labels WLX_SPK_MANY_MAX_ROWS | (n_merges, K) x WLX_SPK_MANY_MAX_FILES]
    hipEvent_t ev_cl[4] = {nullptr, nullptr, nullptr, nullptr};          // around the distance matrices [0, 1] and the clustering [2, 3]
    float aff_ms = 0.f, ahc_ms = 0.f;
    bool cl_timed = false;
};

static void spk_free(wlx_spk* k) {
    if (!k) return;
    (void)hipSetDevice(k->device);
    if (k->st) (void)hipStreamSynchronize(k->st);
    for (hipEvent_t e : k->ev)
        if (e) (void)hipEventDestroy(e);
    for (void* p : k->pool) (void)hipFree(p);
    if (k->h_emb) (void)hipHostFree(k->h_emb);
    for (hipEvent_t e : k->ev_cl)
        if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)k->h_mn_emb, (void*)k->h_mn_cent, (void*)k->h_mn_int})
        if (p) (void)hipHostFree(p);
    if (k->st) (void)hipStreamDestroy(k->st);
    delete k;
}

static int spk_build(wlx_spk* k, const wlx_tensor* weights, int n_weights) {
    const wlx_spk_spec& sp = k->spec;
    CK(hipSetDevice(k->device));
    CK(hipStreamCreateWithFlags(&k->st, hipStreamNonBlocking));
    for (hipEvent_t& e : k->ev) CK(hipEventCreate(&e));
    CKR(upload_tables(k->pool, sp.n_mels, &k->window, &k->twiddle, &k->mel));
    Weights ws;
    CKR(ws.open(weights, n_weights));
    const int m = sp.planes;
    std::vector<float> w, b;
    CKR(fetch(ws, "conv1.weight", {m, 1, 3, 3}, w));
    CKR(fetch(ws, "conv1.bias", {m}, b));
    CKR(dalloc(k->pool, &k->stem_w, w.size(), false));
    CKR(dalloc(k->pool, &k->stem_b, b.size(), false));
    CKR(upload_sync(k->stem_w, w.data(), w.size() * sizeof(float)));
    CKR(upload_sync(k->stem_b, b.data(), b.size() * sizeof(float)));
    int cin = m;
    for (int L = 0; L < 4; ++L) {
        const int planes = m << L;
        for (int B = 0; B < sp.blocks[L]; ++B) {
            const int stride = (B == 0 && L > 0) ? 2 : 1;
            const std::string p = "layer" + std::to_string(L + 1) + "." + std::to_string(B) + ".";
            SpkBlock blk;
            CKR(load_conv(ws, k->pool, p + "conv1", planes, cin, 3, stride, blk.c1));
            CKR(load_conv(ws, k->pool, p + "conv2", planes, planes, 3, 1, blk.c2));
            blk.has_sc = stride != 1 || cin != planes;
            if (blk.has_sc) CKR(load_conv(ws, k->pool, p + "shortcut", planes, cin, 1, stride, blk.sc));
            k->blocks.push_back(blk);
            cin = planes;
        }
    }
    k->pool_dim = 2 * (m << 3) * (sp.n_mels >> 3);
    CKR(fetch(ws, "seg_1.weight", {sp.embed_dim, k->pool_dim}, w));
    CKR(fetch(ws, "seg_1.bias", {sp.embed_dim}, b));
    std::vector<half_t> w16(w.size());
    for (size_t i = 0; i < w.size(); ++i) w16[i] = (half_t)w[i];
    CKR(dalloc(k->pool, &k->head_W, w16.size(), false));
    CKR(dalloc(k->pool, &k->head_b, b.size(), false));
    CKR(upload_sync(k->head_W, w16.data(), w16.size() * sizeof(half_t)));
    CKR(upload_sync(k->head_b, b.data(), b.size() * sizeof(float)));
    CKR(ws.finish());

    k->max_samples = (long)sp.max_seconds * 16000;
    const size_t Tmax = (size_t)spk_frames(k->max_samples);
    CKR(dalloc(k->pool, &k->pcm, (size_t)k->max_samples, false));
    CKR(dalloc(k->pool, &k->logmel, Tmax * sp.n_mels, false));
    CKR(dalloc(k->pool, &k->feat16, Tmax * sp.n_mels, false));
    // the stem's output is the largest activation: every stride-2 stage halves H and W and doubles C
    for (half_t*& a : k->act) CKR(dalloc(k->pool, &a, Tmax * sp.n_mels * m, false));
    // (a batch packs its items into the buffers above: sum T_i <= spk_frames(sum n_i), and from the second stage on the rounded-up
    // halves sum to at most (sum W_i + n) / 2 columns of half the rows and twice the channels: under the stem's extent, n <= sum W_i.
    // A single embed is the case n = 1, sum T_i = T)
    CKR(dalloc(k->pool, &k->pooled, (size_t)k->pool_dim * WLX_SPK_MAX_BATCH, false));
    CKR(dalloc(k->pool, &k->emb, (size_t)sp.embed_dim * WLX_SPK_MAX_BATCH, false));
    CK(hipHostMalloc(reinterpret_cast<void**>(&k->h_emb), (size_t)sp.embed_dim * WLX_SPK_MAX_BATCH * sizeof(float), hipHostMallocDefault));
    return WLX_OK;
}

extern "C" int32_t wlx_spk_create(const wlx_spk_spec* spec, const wlx_tensor* weights, int32_t n_weights, int32_t device, wlx_spk** out) {
    if (!spec || !weights || !out || n_weights < 1) return set_error(WLX_ERR_ARG, "null argument");
    if (spec->n_mels < 8 || spec->n_mels % 8 || spec->n_mels > 256)
        return set_error(WLX_ERR_ARG, "n_mels %d must be a multiple of 8 in 8..256", spec->n_mels);
    if (spec->planes < 32 || spec->planes % 32 || spec->planes > 128)
        return set_error(WLX_ERR_ARG, "planes %d must be 32, 64, 96 or 128", spec->planes);
    for (int L = 0; L < 4; ++L)
        if (spec->blocks[L] < 1 || spec->blocks[L] > 64) return set_error(WLX_ERR_ARG, "blocks[%d] = %d outside 1..64", L, spec->blocks[L]);
    if (spec->embed_dim < 1 || spec->embed_dim > 1024) return set_error(WLX_ERR_ARG, "embed_dim %d outside 1..1024", spec->embed_dim);
    if (spec->max_seconds < 1 || spec->max_seconds > 120) return set_error(WLX_ERR_ARG, "max_seconds %d outside 1..120", spec->max_seconds);
    if (!(spec->pool_eps >= 0.f)) return set_error(WLX_ERR_ARG, "pool_eps must be >= 0");
    int n = 0;
    CK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_error(WLX_ERR_ARG, "device %d outside 0..%d", device, n - 1);
    wlx_spk* k = new wlx_spk();
    k->device = device;
    k->spec = *spec;
    const int rc = spk_build(k, weights, n_weights);
    if (rc != WLX_OK) {
        spk_free(k);
        return rc;
    }
    *out = k;
    return WLX_OK;
}

extern "C" void wlx_spk_destroy(wlx_spk* k) {
    if (!k) return;
    { std::lock_guard<std::mutex> g(k->mu); }      // a call in flight finishes first
    spk_free(k);
}

// ------------------------------------------------------------------------------------------------ the pass and its entry points
// What the three batch entry points decide on the arguments alone: status and the zero row of every item that is too short, and of the
// m items that take part their frames and the row of `out` each fills. Written to the CALLER's arrays only by spk_plan_commit, after
// every refusal of the entry point has had its turn.
struct SpkPlan {
    long offs[WLX_SPK_MAX_BATCH];            // first sample of the item in the buffer the front end reads
    int widths[WLX_SPK_MAX_BATCH], row[WLX_SPK_MAX_BATCH], m = 0;
    long total = 0;
};

static int spk_plan(const char* who, const wlx_spk* k, const int64_t* starts, const int64_t* n_samples, int n, SpkPlan& pl) {
    if (n < 1 || n > WLX_SPK_MAX_BATCH) return set_error(WLX_ERR_ARG, "%s: %d items outside 1..%d", who, n, WLX_SPK_MAX_BATCH);
    long at = 0;
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 0 || n_samples[i] > k->max_samples)
            return set_error(WLX_ERR_ARG, "%s: item %d: %lld samples outside 0..the engine's %d s", who, i, (long long)n_samples[i], k->spec.max_seconds);
        if (starts && starts[i] < 0) return set_error(WLX_ERR_ARG, "%s: item %d starts at %lld", who, i, (long long)starts[i]);
        if (n_samples[i] >= WLX_SPK_MIN_SAMPLES) {
            pl.offs[pl.m] = starts ? (long)starts[i] : at, pl.widths[pl.m] = spk_frames((long)n_samples[i]), pl.row[pl.m] = i;
            ++pl.m;
        }
        at += (long)n_samples[i];
    }
    pl.total = at;
    if (at > k->max_samples)
        return set_error(WLX_ERR_ARG, "%s: %ld samples in %d items exceed the engine's %d s", who, at, n, k->spec.max_seconds);
    return WLX_OK;
}

static void spk_plan_commit(const wlx_spk* k, const int64_t* n_samples, int n, float* out, int32_t* status) {
    const int E = k->spec.embed_dim;
    for (int i = 0; i < n; ++i) {
        const bool too_short = n_samples[i] < WLX_SPK_MIN_SAMPLES;
        status[i] = too_short ? WLX_ERR_TOO_SHORT : WLX_OK;
        if (too_short) std::fill(out + (size_t)i * E, out + (size_t)(i + 1) * E, 0.f);
    }
}

// The launches of the pass on k->st, behind whatever the caller put there (an upload, a wait for another stream): item a of the plan is
// the samples src[offs[a] ...) — the engine's upload buffer or resident audio, the launches do not know which; its embedding is row a of
// `emb` (device). Nothing is waited for: the plan's tables travel in the kernel arguments. k->mu is held and the device is set.
static int spk_enqueue_batch(wlx_spk* k, const float* src, const SpkPlan& pl, float* emb) {
    const wlx_spk_spec& sp = k->spec;
    hipStream_t st = k->st;
    const int m = pl.m;
    int widths[WLX_SPK_MAX_BATCH];
    std::copy(pl.widths, pl.widths + m, widths);
    CK(hipEventRecord(k->ev[0], st));
    if (!launch_spk_fbank_batch(src, pl.offs, widths, m, k->window, k->twiddle, k->mel, sp.n_mels, k->logmel, st) ||
        !launch_spk_cmn_batch(k->logmel, widths, m, sp.n_mels, k->feat16, st))
        return set_error(WLX_ERR_ARG, "front end refused a batch of %d", m);
    CK(hipEventRecord(k->ev[1], st));
    int H = sp.n_mels;
    half_t *x = k->act[0], *t1 = k->act[1], *y = k->act[2], *sc = k->act[3];
    if (!launch_spk_conv_c1_batch(k->feat16, H, widths, m, k->stem_w, k->stem_b, nullptr, sp.planes, 1, true, x, st))
        return set_error(WLX_ERR_ARG, "stem convolution refused a batch of %d", m);
    for (const SpkBlock& b : k->blocks) {
        const int s = b.c1.stride, OH = (H - 1) / s + 1;
        int ow[WLX_SPK_MAX_BATCH];
        for (int i = 0; i < m; ++i) ow[i] = (widths[i] - 1) / s + 1;
        bool ok = launch_spk_conv_batch(x, H, widths, m, b.c1.cin, b.c1.Wp, b.c1.bias, nullptr, b.c1.cout, s, 3, true, t1, st);
        const half_t* resid = x;
        if (b.has_sc) {
            ok = ok && launch_spk_conv_batch(x, H, widths, m, b.sc.cin, b.sc.Wp, b.sc.bias, nullptr, b.sc.cout, s, 1, false, sc, st);
            resid = sc;
        }
        ok = ok && launch_spk_conv_batch(t1, OH, ow, m, b.c2.cin, b.c2.Wp, b.c2.bias, resid, b.c2.cout, 1, 3, true, y, st);
        if (!ok) return set_error(WLX_ERR_ARG, "convolution refused a batch of %d at H %d x Cin %d", m, H, b.c1.cin);
        std::swap(x, y);
        H = OH;
        std::copy(ow, ow + m, widths);
    }
    if (!launch_spk_pool_batch(x, H, widths, m, sp.planes << 3, sp.pool_eps, k->pooled, st))
        return set_error(WLX_ERR_ARG, "pooling refused a batch of %d", m);
    if (!launch_spk_head_batch(k->pooled, k->head_W, k->head_b, sp.embed_dim, k->pool_dim, m, emb, st))
        return set_error(WLX_ERR_ARG, "head refused a batch of %d at %d -> %d", m, k->pool_dim, sp.embed_dim);
    CK(hipEventRecord(k->ev[2], st));
    CK(hipGetLastError());
    return WLX_OK;
}

// The pass for the embed entry points: one launch sequence, one download, one wait; row a of the pass goes to row pl.row[a] of `out`.
static int spk_run_batch(wlx_spk* k, const float* src, const SpkPlan& pl, float* out) {
    const wlx_spk_spec& sp = k->spec;
    hipStream_t st = k->st;
    const int m = pl.m;
    CKR(spk_enqueue_batch(k, src, pl, k->emb));
    CK(hipMemcpyAsync(k->h_emb, k->emb, (size_t)m * sp.embed_dim * sizeof(float), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    for (int a = 0; a < m; ++a) std::copy(k->h_emb + (size_t)a * sp.embed_dim, k->h_emb + (size_t)(a + 1) * sp.embed_dim, out + (size_t)pl.row[a] * sp.embed_dim);
    CK(hipEventElapsedTime(&k->fbank_ms, k->ev[0], k->ev[1]));
    CK(hipEventElapsedTime(&k->net_ms, k->ev[1], k->ev[2]));
    k->timed = true;
    return WLX_OK;
}

// one segment: a batch of one with refusals of its own (too short is the RETURN value here, and `out` stays untouched)
extern "C" int32_t wlx_spk_embed(wlx_spk* k, const float* pcm, int64_t n_samples, float* out) {
    if (!k || !pcm || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (n_samples < WLX_SPK_MIN_SAMPLES)
        return set_error(WLX_ERR_TOO_SHORT, "%lld samples: under 0.3 s of audio", (long long)n_samples);
    if (n_samples > k->max_samples)
        return set_error(WLX_ERR_ARG, "%lld samples exceed the engine's %d s", (long long)n_samples, k->spec.max_seconds);
    SpkPlan pl;
    pl.offs[0] = 0, pl.widths[0] = spk_frames((long)n_samples), pl.row[0] = 0, pl.m = 1, pl.total = (long)n_samples;
    std::lock_guard<std::mutex> g(k->mu);
    CK(hipSetDevice(k->device));
    CK(hipMemcpyAsync(k->pcm, pcm, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, k->st));
    return spk_run_batch(k, k->pcm, pl, out);
}

extern "C" int32_t wlx_spk_embed_batch(wlx_spk* k, const float* pcm, const int64_t* n_samples, int32_t n, float* out, int32_t* status) {
    if (!k || !pcm || !n_samples || !out || !status) return set_error(WLX_ERR_ARG, "null argument");
    SpkPlan pl;
    CKR(spk_plan("wlx_spk_embed_batch", k, nullptr, n_samples, n, pl));
    spk_plan_commit(k, n_samples, n, out, status);
    if (pl.m == 0) return WLX_OK;
    std::lock_guard<std::mutex> g(k->mu);
    CK(hipSetDevice(k->device));
    // one upload: the caller's items lie back to back, the short ones among them are carried along and never read
    CK(hipMemcpyAsync(k->pcm, pcm, (size_t)pl.total * sizeof(float), hipMemcpyHostToDevice, k->st));
    return spk_run_batch(k, k->pcm, pl, out);
}

// The same on ranges of a slot item's resident PCM (wlx_pcm_put / wlx_pcm_put_frames): the front end reads s->pcm where the upload route
// reads k->pcm, nothing else differs, so no sample crosses the bus.
extern "C" int32_t wlx_spk_embed_pcm_batch(wlx_spk* k, wlx_engine* e, int32_t slot, int32_t item, const int64_t* starts,
                                           const int64_t* n_samples, int32_t n, float* out, int32_t* status) {
    if (!k || !e || !starts || !n_samples || !out || !status) return set_error(WLX_ERR_ARG, "wlx_spk_embed_pcm_batch: null argument");
    CKR(PcmLease::same_device("wlx_spk_embed_pcm_batch", "engine", e->device, "speaker engine", k->device));
    SpkPlan pl;
    CKR(spk_plan("wlx_spk_embed_pcm_batch", k, starts, n_samples, n, pl));
    PcmLease L;
    CKR(L.open_slot(e, slot));
    CKR(L.item("wlx_spk_embed_pcm_batch", item));
    if (L.resident <= 0 || !L.buf) return set_error(WLX_ERR_STATE, "wlx_spk_embed_pcm_batch: item %d: no PCM resident", item);
    for (int i = 0; i < n; ++i) CKR(L.range("wlx_spk_embed_pcm_batch", starts[i], n_samples[i]));
    spk_plan_commit(k, n_samples, n, out, status);
    if (pl.m == 0) return WLX_OK;
    std::lock_guard<std::mutex> g(k->mu);
    CK(hipSetDevice(k->device));
    CKR(L.order(k->st));
    return spk_run_batch(k, L.buf, pl, out);
}

// The same on absolute stream positions of a device PCM ring: a range never wraps, position p is L.buf[p - L.base] (engine.h Ring).
extern "C" int32_t wlx_spk_embed_ring_batch(wlx_spk* k, wlx_ring* r, const int64_t* starts, const int64_t* n_samples, int32_t n, float* out,
                                            int32_t* status) {
    if (!k || !r || !starts || !n_samples || !out || !status) return set_error(WLX_ERR_ARG, "wlx_spk_embed_ring_batch: null argument");
    CKR(PcmLease::same_device("wlx_spk_embed_ring_batch", "ring", r->device, "speaker engine", k->device));
    SpkPlan pl;
    CKR(spk_plan("wlx_spk_embed_ring_batch", k, starts, n_samples, n, pl));
    std::lock_guard<std::mutex> g(k->mu);
    PcmLease L;
    L.open_ring(r);
    for (int i = 0; i < n; ++i) CKR(L.range("wlx_spk_embed_ring_batch", starts[i], n_samples[i]));
    spk_plan_commit(k, n_samples, n, out, status);
    if (pl.m == 0) return WLX_OK;
    for (int a = 0; a < pl.m; ++a) pl.offs[a] -= (long)L.base;
    CK(hipSetDevice(k->device));
    return spk_run_batch(k, L.buf, pl, out);
}

// ------------------------------------------------------------------------------------------------ offline clustering (spk_cluster.hip)
// ONE path behind wlx_spk_cluster, wlx_spk_diarize_pcm and wlx_spk_diarize_many: a file is a wave of one.
static int spk_cluster_opts_ok(const char* who, const wlx_spk_cluster_opts* o) {
    if (!(o->threshold >= 0.f && o->threshold <= 2.f))
        return set_error(WLX_ERR_ARG, "%s: threshold %g is not a cosine distance in [0, 2]", who, (double)o->threshold);
    if (o->max_clusters < 0) return set_error(WLX_ERR_ARG, "%s: max_clusters %d is negative", who, o->max_clusters);
    return WLX_OK;
}

// the buffers of a clustering call, made by the first one (an engine that only embeds never pays for them). k->mu is held.
static int spk_many_reserve(wlx_spk* k) {
    if (k->mn_ready) return WLX_OK;
    const size_t R = WLX_SPK_MANY_MAX_ROWS, F = WLX_SPK_MANY_MAX_FILES, E = (size_t)k->spec.embed_dim;
    if (!k->mn_emb) CKR(dalloc(k->pool, &k->mn_emb, R * E, false));
    if (!k->mn_cent) CKR(dalloc(k->pool, &k->mn_cent, R * E, false));
    if (!k->mn_dist) CKR(dalloc(k->pool, &k->mn_dist, (size_t)WLX_SPK_MANY_MAX_CELLS, false));
    if (!k->mn_heights) CKR(dalloc(k->pool, &k->mn_heights, R, false));
    if (!k->mn_merges) CKR(dalloc(k->pool, &k->mn_merges, 2 * R, false));
    if (!k->mn_labels) CKR(dalloc(k->pool, &k->mn_labels, R, false));
    if (!k->mn_counts) CKR(dalloc(k->pool, &k->mn_counts, 2 * F, false));
    if (!k->h_mn_emb) CK(hipHostMalloc(reinterpret_cast<void**>(&k->h_mn_emb), R * E * sizeof(float), hipHostMallocDefault));
    if (!k->h_mn_cent) CK(hipHostMalloc(reinterpret_cast<void**>(&k->h_mn_cent), R * E * sizeof(float), hipHostMallocDefault));
    if (!k->h_mn_int) CK(hipHostMalloc(reinterpret_cast<void**>(&k->h_mn_int), (R + 2 * F) * sizeof(int), hipHostMallocDefault));
    for (hipEvent_t& e : k->ev_cl)
        if (!e) CK(hipEventCreate(&e));
    k->mn_ready = true;
    return WLX_OK;
}

// What the windows of a wave of files come to on the arguments alone. Rows of the table k->mn_emb are the windows that take part, file by
// file: file f owns rows [row0[f], row0[f] + m_of[f]) and, with m_of[f] >= 2, an entry of `cf`: a matrix and a workgroup of the clustering.
struct SpkWave {
    std::vector<long> w0;              // [n_files + 1]: first window of file f in the packed arrays (set by the entry point)
    std::vector<SpkPlan> plans;        // the ragged passes over the windows that take part
    std::vector<long> win_of;          // the packed window behind row a of the table
    std::vector<int> row0, m_of;
    std::vector<SpkClusterFile> cf;    // the files the clustering launches see, in row order; cf[c] is file cf_file[c]
    std::vector<int> cf_file;
    bool any_single = false;           // a file of one window that takes part: its embedding is its centroid
};

// After every refusal on the arguments has had its turn: the windows of the files with ok[f] that take part, grouped greedily in order
// into passes — a pass closes at WLX_SPK_MAX_BATCH windows or when the next one would take it over max_seconds; only windows that take
// part are counted — and what is known without the device: status, n_clusters (1 for a file with a window that takes part), label 0 / -1
// and the zero row of every window that takes none. Window i of file f starts at sample item_off[f] + starts[i] of the buffer the passes read.
static void spk_wave_plan(const wlx_spk* k, SpkWave& wv, const char* ok, const long* item_off, const int64_t* starts, const int64_t* n_samples,
                          const wlx_spk_cluster_opts* opts, int32_t* labels, int32_t* status, int32_t* n_clusters, float* emb_out) {
    const int n_files = (int)wv.w0.size() - 1, E = k->spec.embed_dim;
    wv.row0.assign((size_t)n_files, 0), wv.m_of.assign((size_t)n_files, 0);
    SpkPlan cur;
    size_t doff = 0;
    for (int f = 0; f < n_files; ++f) {
        wv.row0[f] = (int)wv.win_of.size();
        for (long i = wv.w0[f]; i < wv.w0[f + 1]; ++i) {
            const bool out = !ok[f] || n_samples[i] < WLX_SPK_MIN_SAMPLES;
            status[i] = !ok[f] ? WLX_ERR_STATE : out ? WLX_ERR_TOO_SHORT : WLX_OK;
            labels[i] = out ? -1 : 0;
            if (out && emb_out) std::fill(emb_out + (size_t)i * E, emb_out + (size_t)(i + 1) * E, 0.f);
            if (out) continue;
            if (cur.m > 0 && (cur.m >= WLX_SPK_MAX_BATCH || cur.total + (long)n_samples[i] > k->max_samples)) {
                wv.plans.push_back(cur);
                cur = SpkPlan();
            }
            cur.offs[cur.m] = item_off[f] + (long)starts[i], cur.widths[cur.m] = spk_frames((long)n_samples[i]), cur.row[cur.m] = (int)wv.win_of.size();
            ++cur.m, cur.total += (long)n_samples[i];
            wv.win_of.push_back(i);
        }
        const int m = wv.m_of[f] = (int)wv.win_of.size() - wv.row0[f];
        n_clusters[f] = m > 0 ? 1 : 0;
        wv.any_single = wv.any_single || m == 1;
        if (m >= 2) {
            wv.cf.push_back(SpkClusterFile{doff, wv.row0[f], m, opts[f].threshold, opts[f].max_clusters});
            wv.cf_file.push_back(f);
            doff += (size_t)m * m;
        }
    }
    if (cur.m > 0) wv.plans.push_back(cur);
}

// The files of `cf` (m >= 2 rows each of k->mn_emb, written by work already on k->st): distance matrices, clustering, centroids and the
// downloads into the pinned buffers, all enqueued; the caller waits once. dist_out (host, may be null) gets the matrices, packed file by
// file, before the clustering overwrites them: its copy sits between the two timed intervals.
static int spk_cluster_enqueue(wlx_spk* k, const char* who, const std::vector<SpkClusterFile>& cf, float* dist_out, bool want_centroids) {
    hipStream_t st = k->st;
    const int E = k->spec.embed_dim, C = (int)cf.size();
    const size_t rows = (size_t)cf.back().row0 + cf.back().m, cells = cf.back().doff + (size_t)cf.back().m * cf.back().m;
    CK(hipEventRecord(k->ev_cl[0], st));
    if (!launch_spk_affinity(k->mn_emb, cf.data(), C, E, k->mn_dist, st)) return set_error(WLX_ERR_ARG, "%s: the distance matrices refused %d file(s)", who, C);
    CK(hipEventRecord(k->ev_cl[1], st));
    if (dist_out) CK(hipMemcpyAsync(dist_out, k->mn_dist, cells * sizeof(float), hipMemcpyDeviceToHost, st));
    CK(hipEventRecord(k->ev_cl[2], st));
    if (!launch_spk_ahc(k->mn_dist, cf.data(), C, k->mn_merges, k->mn_heights, k->mn_labels, k->mn_counts, st))
        return set_error(WLX_ERR_ARG, "%s: the clustering refused %d file(s)", who, C);
    CK(hipEventRecord(k->ev_cl[3], st));
    if (want_centroids) {
        if (!launch_spk_centroids(k->mn_emb, k->mn_labels, k->mn_counts, cf.data(), C, E, k->mn_cent, st))
            return set_error(WLX_ERR_ARG, "%s: the centroids refused %d file(s)", who, C);
        CK(hipMemcpyAsync(k->h_mn_cent, k->mn_cent, rows * E * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(k->h_mn_int, k->mn_labels, rows * sizeof(int), hipMemcpyDeviceToHost, st));
    CK(hipMemcpyAsync(k->h_mn_int + WLX_SPK_MANY_MAX_ROWS, k->mn_counts, (size_t)2 * C * sizeof(int), hipMemcpyDeviceToHost, st));
    return WLX_OK;
}

// after the wait: per clustered file K, its first K centroids and the labels of its rows dealt to the caller's windows; the times
static int spk_cluster_collect(wlx_spk* k, const char* who, const SpkWave& wv, int32_t* labels, float* centroids, int32_t* n_clusters) {
    const int E = k->spec.embed_dim;
    for (size_t c = 0; c < wv.cf.size(); ++c) {
        const SpkClusterFile& cf = wv.cf[c];
        const int f = wv.cf_file[c], K = k->h_mn_int[WLX_SPK_MANY_MAX_ROWS + 2 * c + 1];
        if (K < 1 || K > cf.m) return set_error(WLX_ERR_HIP, "%s: the clustering of file %d (%d rows) reported %d clusters", who, f, cf.m, K);
        n_clusters[f] = K;
        if (centroids) std::copy(k->h_mn_cent + (size_t)cf.row0 * E, k->h_mn_cent + (size_t)(cf.row0 + K) * E, centroids + (size_t)wv.w0[f] * E);
        for (int a = cf.row0; a < cf.row0 + cf.m; ++a) labels[wv.win_of[a]] = k->h_mn_int[a];
    }
    CK(hipEventElapsedTime(&k->aff_ms, k->ev_cl[0], k->ev_cl[1]));
    CK(hipEventElapsedTime(&k->ahc_ms, k->ev_cl[2], k->ev_cl[3]));
    k->cl_timed = true;
    return WLX_OK;
}

// host rows: one file whose windows are its rows, uploaded into the table
extern "C" int32_t wlx_spk_cluster(wlx_spk* k, const float* emb, int32_t n, int32_t dim, const wlx_spk_cluster_opts* opts, int32_t* labels,
                                   float* centroids, int32_t* n_clusters) {
    const char* who = "wlx_spk_cluster";
    if (!k || !emb || !opts || !labels || !n_clusters) return set_error(WLX_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > WLX_SPK_CLUSTER_MAX) return set_error(WLX_ERR_ARG, "%s: %d rows outside 1..%d", who, n, WLX_SPK_CLUSTER_MAX);
    if (dim != k->spec.embed_dim) return set_error(WLX_ERR_ARG, "%s: dim %d is not the engine's %d", who, dim, k->spec.embed_dim);
    CKR(spk_cluster_opts_ok(who, opts));
    if (n == 1) {                     // one row is its own cluster and its own centroid
        labels[0] = 0, *n_clusters = 1;
        if (centroids) std::copy(emb, emb + dim, centroids);
        return WLX_OK;
    }
    SpkWave wv;
    wv.w0 = {0, n};
    for (int a = 0; a < n; ++a) wv.win_of.push_back(a);
    wv.cf.push_back(SpkClusterFile{0, 0, n, opts->threshold, opts->max_clusters});
    wv.cf_file.push_back(0);
    std::lock_guard<std::mutex> g(k->mu);
    CK(hipSetDevice(k->device));
    CKR(spk_many_reserve(k));
    CK(hipMemcpyAsync(k->mn_emb, emb, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, k->st));
    CKR(spk_cluster_enqueue(k, who, wv.cf, nullptr, centroids != nullptr));
    CK(hipStreamSynchronize(k->st));
    return spk_cluster_collect(k, who, wv, labels, centroids, n_clusters);
}

// The device's part of a planned wave with a window that takes part: every pass a ragged batch whose head writes its rows straight into
// the table, then the clustering on that table; ONE wait, then the rows, centroids and labels dealt to the caller's windows. `src` is the
// buffer the plan's offsets count from, inside the lease L.
static int spk_wave_run(wlx_spk* k, const char* who, PcmLease& L, const float* src, const SpkWave& wv, int32_t* labels, int32_t* n_clusters,
                        float* emb_out, float* dist_out, float* centroids) {
    const int M = (int)wv.win_of.size(), E = k->spec.embed_dim, n_files = (int)wv.m_of.size();
    std::lock_guard<std::mutex> g(k->mu);
    CK(hipSetDevice(k->device));
    CKR(spk_many_reserve(k));
    CKR(L.order(k->st));
    for (const SpkPlan& pl : wv.plans) CKR(spk_enqueue_batch(k, src, pl, k->mn_emb + (size_t)pl.row[0] * E));
    if (emb_out || (centroids && wv.any_single)) CK(hipMemcpyAsync(k->h_mn_emb, k->mn_emb, (size_t)M * E * sizeof(float), hipMemcpyDeviceToHost, k->st));
    if (!wv.cf.empty()) CKR(spk_cluster_enqueue(k, who, wv.cf, dist_out, centroids != nullptr));
    CK(hipStreamSynchronize(k->st));
    CK(hipEventElapsedTime(&k->fbank_ms, k->ev[0], k->ev[1]));          // (of the last pass)
    CK(hipEventElapsedTime(&k->net_ms, k->ev[1], k->ev[2]));
    k->timed = true;
    if (emb_out)
        for (int a = 0; a < M; ++a) std::copy(k->h_mn_emb + (size_t)a * E, k->h_mn_emb + (size_t)(a + 1) * E, emb_out + (size_t)wv.win_of[a] * E);
    if (centroids)                    // one window is its own cluster, its embedding the centroid
        for (int f = 0; f < n_files; ++f)
            if (wv.m_of[f] == 1) std::copy(k->h_mn_emb + (size_t)wv.row0[f] * E, k->h_mn_emb + (size_t)(wv.row0[f] + 1) * E, centroids + (size_t)wv.w0[f] * E);
    if (wv.cf.empty()) return WLX_OK;
    return spk_cluster_collect(k, who, wv, labels, centroids, n_clusters);
}

// A whole file: a wave of one behind refusals of its own — an item with nothing resident or a window past its end refuses the call.
extern "C" int32_t wlx_spk_diarize_pcm(wlx_spk* k, wlx_engine* e, int32_t slot, int32_t item, const int64_t* starts, const int64_t* n_samples,
                                       int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels, int32_t* status, float* emb_out,
                                       float* dist_out, float* centroids, int32_t* n_clusters) {
    const char* who = "wlx_spk_diarize_pcm";
    if (!k || !e || !starts || !n_samples || !opts || !labels || !status || !n_clusters) return set_error(WLX_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > WLX_SPK_CLUSTER_MAX) return set_error(WLX_ERR_ARG, "%s: %d windows outside 1..%d", who, n, WLX_SPK_CLUSTER_MAX);
    CKR(spk_cluster_opts_ok(who, opts));
    CKR(PcmLease::same_device(who, "engine", e->device, "speaker engine", k->device));
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 0 || n_samples[i] > k->max_samples)
            return set_error(WLX_ERR_ARG, "%s: window %d: %lld samples outside 0..the engine's %d s", who, i, (long long)n_samples[i], k->spec.max_seconds);
        if (starts[i] < 0) return set_error(WLX_ERR_ARG, "%s: window %d starts at %lld", who, i, (long long)starts[i]);
    }
    PcmLease L;
    CKR(L.open_slot(e, slot));
    CKR(L.item(who, item));
    if (L.resident <= 0 || !L.buf) return set_error(WLX_ERR_STATE, "%s: item %d: no PCM resident", who, item);
    for (int i = 0; i < n; ++i) CKR(L.range(who, starts[i], n_samples[i]));
    SpkWave wv;
    wv.w0 = {0, n};
    const char ok = 1;
    const long item_off = 0;          // (the passes read the item's own buffer)
    spk_wave_plan(k, wv, &ok, &item_off, starts, n_samples, opts, labels, status, n_clusters, emb_out);
    if (wv.win_of.empty()) return WLX_OK;
    CKR(spk_wave_run(k, who, L, L.buf, wv, labels, n_clusters, emb_out, dist_out, centroids));
    if (dist_out && wv.m_of[0] == 1) dist_out[0] = 0.f;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ a wave of files (wlx_spk_diarize_many)
// The files of a wave lie in the items of ONE slot, rows of one allocation: the front end addresses a window as an offset from item 0
// (item * pcm_cap + start), so a pass mixes the windows of different files as it mixes those of one.
extern "C" int32_t wlx_spk_diarize_many(wlx_spk* k, wlx_engine* e, int32_t slot, int32_t n_files, const int32_t* items, const int32_t* n_windows,
                                        const int64_t* starts, const int64_t* n_samples, const wlx_spk_cluster_opts* opts, int32_t* labels,
                                        int32_t* status, int32_t* file_status, int32_t* n_clusters, float* emb_out, float* centroids) {
    const char* who = "wlx_spk_diarize_many";
    if (!k || !e || !items || !n_windows || !starts || !n_samples || !opts || !labels || !status || !file_status || !n_clusters)
        return set_error(WLX_ERR_ARG, "%s: null argument", who);
    if (n_files < 1 || n_files > WLX_SPK_MANY_MAX_FILES) return set_error(WLX_ERR_ARG, "%s: %d files outside 1..%d", who, n_files, WLX_SPK_MANY_MAX_FILES);
    SpkWave wv;
    std::vector<long>& w0 = wv.w0;
    w0.assign((size_t)n_files + 1, 0);
    for (int f = 0; f < n_files; ++f) {
        if (n_windows[f] < 0 || n_windows[f] > WLX_SPK_CLUSTER_MAX)
            return set_error(WLX_ERR_ARG, "%s: file %d: %d windows outside 0..%d", who, f, n_windows[f], WLX_SPK_CLUSTER_MAX);
        w0[f + 1] = w0[f] + n_windows[f];
        CKR(spk_cluster_opts_ok(who, &opts[f]));
        for (int g = 0; g < f; ++g)
            if (items[g] == items[f]) return set_error(WLX_ERR_ARG, "%s: files %d and %d both name item %d", who, g, f, items[f]);
    }
    if (w0[n_files] > WLX_SPK_MANY_MAX_ROWS)
        return set_error(WLX_ERR_ARG, "%s: %ld windows in all exceed %d", who, w0[n_files], WLX_SPK_MANY_MAX_ROWS);
    size_t cells = 0;
    for (int f = 0; f < n_files; ++f) {
        size_t m = 0;
        for (long i = w0[f]; i < w0[f + 1]; ++i) {
            if (n_samples[i] < 0 || n_samples[i] > k->max_samples)
                return set_error(WLX_ERR_ARG, "%s: file %d window %ld: %lld samples outside 0..the engine's %d s", who, f, i - w0[f], (long long)n_samples[i], k->spec.max_seconds);
            if (starts[i] < 0) return set_error(WLX_ERR_ARG, "%s: file %d window %ld starts at %lld", who, f, i - w0[f], (long long)starts[i]);
            m += n_samples[i] >= WLX_SPK_MIN_SAMPLES;
        }
        cells += m * m;
    }
    if (cells > (size_t)WLX_SPK_MANY_MAX_CELLS)
        return set_error(WLX_ERR_ARG, "%s: the distance matrices of the files take %zu floats, over %zu", who, cells, (size_t)WLX_SPK_MANY_MAX_CELLS);
    CKR(PcmLease::same_device(who, "engine", e->device, "speaker engine", k->device));
    PcmLease L;
    CKR(L.open_slot(e, slot));
    for (int f = 0; f < n_files; ++f) CKR(L.item(who, items[f]));
    // residency is a file's own matter: an item without PCM, or a window past its count, costs that file only
    L.view(0);
    const float* base = L.buf;
    std::vector<char> ok((size_t)n_files, 0);
    std::vector<long> item_off((size_t)n_files, 0);
    for (int f = 0; f < n_files; ++f) {
        L.view(items[f]);
        bool good = L.resident > 0 && L.buf;
        for (long i = w0[f]; good && i < w0[f + 1]; ++i) good = starts[i] <= L.resident - n_samples[i];
        ok[f] = good, item_off[f] = good ? (long)(L.buf - base) : 0;
        file_status[f] = good ? WLX_OK : WLX_ERR_STATE;          // (every refusal on the arguments has had its turn)
    }
    spk_wave_plan(k, wv, ok.data(), item_off.data(), starts, n_samples, opts, labels, status, n_clusters, emb_out);
    if (wv.win_of.empty()) return WLX_OK;
    return spk_wave_run(k, who, L, base, wv, labels, n_clusters, emb_out, nullptr, centroids);
}

extern "C" int32_t wlx_spk_debug_cluster_timings(wlx_spk* k, float* affinity_ms, float* ahc_ms) {
    if (!k || !affinity_ms || !ahc_ms) return set_error(WLX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> g(k->mu);
    if (!k->cl_timed) return set_error(WLX_ERR_STATE, "no clustering has run on this engine");
    *affinity_ms = k->aff_ms;
    *ahc_ms = k->ahc_ms;
    return WLX_OK;
}

extern "C" int32_t wlx_spk_debug_timings(wlx_spk* k, float* fbank_ms, float* net_ms) {
    if (!k || !fbank_ms || !net_ms) return set_error(WLX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> g(k->mu);
    if (!k->timed) return set_error(WLX_ERR_STATE, "no embed has run on this engine");
    *fbank_ms = k->fbank_ms;
    *net_ms = k->net_ms;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ one-launch hooks (host.h HookScope)

extern "C" int32_t wlx_spk_debug_fbank(int32_t device, const float* pcm, int64_t n_samples, int32_t n_mels, float* frames_out,
                                       uint16_t* image_out, int32_t cap_frames, int32_t* n_frames_out) {
    if (!pcm || !frames_out || !image_out || !n_frames_out) return set_error(WLX_ERR_ARG, "null argument");
    if (n_mels < 1 || n_mels > 256) return set_error(WLX_ERR_ARG, "n_mels %d outside 1..256", n_mels);
    if (n_samples < WLX_SPK_FRAME || n_samples > (1LL << 28)) return set_error(WLX_ERR_ARG, "n_samples %lld outside 400..2^28", (long long)n_samples);
    const int T = spk_frames((long)n_samples);
    if (T > cap_frames) return set_error(WLX_ERR_ARG, "%d frames exceed the caller's %d", T, cap_frames);
    HookScope S;
    CKR(S.begin(device));
    float *window, *twiddle, *mel, *dpcm, *dlm;
    half_t* d16;
    CKR(upload_tables(S.allocs, n_mels, &window, &twiddle, &mel));
    CKR(S.upload(&dpcm, pcm, (size_t)n_samples));
    CKR(S.alloc(&dlm, (size_t)T * n_mels));
    CKR(S.alloc(&d16, (size_t)T * n_mels));
    const long offset = 0;          // one item at the start of the upload
    if (!launch_spk_fbank_batch(dpcm, &offset, &T, 1, window, twiddle, mel, n_mels, dlm, S.st) ||
        !launch_spk_cmn_batch(dlm, &T, 1, n_mels, d16, S.st))
        return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(frames_out, dlm, (size_t)T * n_mels));
    CKR(S.download(h16(image_out), d16, (size_t)T * n_mels));
    *n_frames_out = T;
    return S.finish();
}

// wlx_spk_debug_conv (n = 1, widths = {W}) and wlx_spk_debug_conv_batch behind their own geometry checks: `Wsum` / `OWsum` columns in
// all at the input / the output, stride is 1 or 2.
static int spk_debug_conv_run(int device, const uint16_t* in, int H, int n, const int32_t* widths, long Wsum, long OWsum, int Cin, const float* w,
                              const float* bias, const uint16_t* resid, int Cout, int stride, int ksize, int relu, uint16_t* out) {
    const bool c1 = Cin == 1;
    if (c1 ? (ksize != 3 || Cout < 4 || Cout % 4 || Cout > 1024)
           : ((ksize != 1 && ksize != 3) || Cin < 32 || Cin % 32 || Cin > 1024 || Cout < 32 || Cout % 32 || Cout > 1024))
        return set_error(WLX_ERR_ARG, "Cin %d / Cout %d / ksize %d: Cin = 1 (ksize 3, Cout a multiple of 4) or Cin and Cout multiples of 32 up "
                         "to 1024 with ksize 1 or 3", Cin, Cout, ksize);
    const int OH = (H - 1) / stride + 1;
    const size_t n_out = (size_t)OH * OWsum * Cout;
    std::vector<float> zeros;          // (host staging declared before S: it outlives the stream's copies on every return path)
    std::vector<half_t> packed;
    HookScope S;
    CKR(S.begin(device));
    half_t *din, *dres = nullptr, *dout;
    float* dbias;
    CKR(S.upload(&din, h16(in), (size_t)H * Wsum * Cin));
    if (!bias) zeros.assign((size_t)Cout, 0.f);
    CKR(S.upload(&dbias, bias ? bias : zeros.data(), (size_t)Cout));
    if (resid) CKR(S.upload(&dres, h16(resid), n_out));
    CKR(S.upload(&dout, h16(out), n_out));
    bool ok;
    if (c1) {
        float* dw;
        CKR(S.upload(&dw, w, (size_t)Cout * 9));
        ok = launch_spk_conv_c1_batch(din, H, widths, n, dw, dbias, dres, Cout, stride, relu != 0, dout, S.st);
    } else {
        packed.resize(spk_packed_halfs(Cout, Cin, ksize));
        spk_pack_conv(w, Cout, Cin, ksize, packed.data());
        half_t* dWp;
        CKR(S.upload(&dWp, packed.data(), packed.size()));
        ok = launch_spk_conv_batch(din, H, widths, n, Cin, dWp, dbias, dres, Cout, stride, ksize, relu != 0, dout, S.st);
    }
    if (!ok) return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(h16(out), dout, n_out));
    return S.finish();
}

extern "C" int32_t wlx_spk_debug_conv(int32_t device, const uint16_t* in, int32_t H, int32_t W, int32_t Cin, const float* w, const float* bias,
                                      const uint16_t* resid, int32_t Cout, int32_t stride, int32_t ksize, int32_t relu, uint16_t* out) {
    if (!in || !w || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (H < 1 || W < 1 || (long)H * W > (1L << 24)) return set_error(WLX_ERR_ARG, "H %d x W %d outside 1..2^24 pixels", H, W);
    if (stride != 1 && stride != 2) return set_error(WLX_ERR_ARG, "stride %d must be 1 or 2", stride);
    return spk_debug_conv_run(device, in, H, 1, &W, W, (W - 1) / stride + 1, Cin, w, bias, resid, Cout, stride, ksize, relu, out);
}

extern "C" int32_t wlx_spk_debug_conv_batch(int32_t device, const uint16_t* in, int32_t H, int32_t n, const int32_t* widths, int32_t Cin,
                                            const float* w, const float* bias, const uint16_t* resid, int32_t Cout, int32_t stride,
                                            int32_t ksize, int32_t relu, uint16_t* out) {
    if (!in || !w || !out || !widths) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_SPK_MAX_BATCH) return set_error(WLX_ERR_ARG, "%d items outside 1..%d", n, WLX_SPK_MAX_BATCH);
    if (stride != 1 && stride != 2) return set_error(WLX_ERR_ARG, "stride %d must be 1 or 2", stride);
    long Wsum = 0, OWsum = 0;
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 1 || widths[i] > (1 << 24)) return set_error(WLX_ERR_ARG, "widths[%d] = %d outside 1..2^24", i, widths[i]);
        Wsum += widths[i], OWsum += (widths[i] - 1) / stride + 1;
    }
    if (H < 1 || (long)H * Wsum > (1L << 24)) return set_error(WLX_ERR_ARG, "H %d x sum of widths %ld outside 1..2^24 pixels", H, Wsum);
    return spk_debug_conv_run(device, in, H, n, widths, Wsum, OWsum, Cin, w, bias, resid, Cout, stride, ksize, relu, out);
}

// wlx_spk_debug_pool (n = 1, frames = {T}) and wlx_spk_debug_pool_batch behind their own range checks: `Tsum` frames in all
static int spk_debug_pool_run(int device, const uint16_t* x, int F, int n, const int32_t* frames, long Tsum, int C, float eps, float* out) {
    HookScope S;
    CKR(S.begin(device));
    half_t* dx;
    float* dout;
    const size_t n_out = (size_t)n * 2 * F * C;
    CKR(S.upload(&dx, h16(x), (size_t)F * Tsum * C));
    CKR(S.upload(&dout, out, n_out));
    if (!launch_spk_pool_batch(dx, F, frames, n, C, eps, dout, S.st)) return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(out, dout, n_out));
    return S.finish();
}

extern "C" int32_t wlx_spk_debug_pool(int32_t device, const uint16_t* x, int32_t F, int32_t T, int32_t C, float eps, float* out) {
    if (!x || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (F < 1 || F > 4096 || T < 2 || T > (1 << 20) || C < 64 || C % 64 || C > 4096 || !(eps >= 0.f))
        return set_error(WLX_ERR_ARG, "F %d / T %d / C %d: F in 1..4096, T in 2..2^20, C a multiple of 64 up to 4096", F, T, C);
    return spk_debug_pool_run(device, x, F, 1, &T, T, C, eps, out);
}

extern "C" int32_t wlx_spk_debug_pool_batch(int32_t device, const uint16_t* x, int32_t F, int32_t n, const int32_t* frames, int32_t C,
                                            float eps, float* out) {
    if (!x || !out || !frames) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_SPK_MAX_BATCH) return set_error(WLX_ERR_ARG, "%d items outside 1..%d", n, WLX_SPK_MAX_BATCH);
    if (F < 1 || F > 4096 || C < 64 || C % 64 || C > 4096 || !(eps >= 0.f))
        return set_error(WLX_ERR_ARG, "F %d / C %d: F in 1..4096, C a multiple of 64 up to 4096", F, C);
    long Tsum = 0;
    for (int i = 0; i < n; ++i) {
        if (frames[i] < 2 || frames[i] > (1 << 20)) return set_error(WLX_ERR_ARG, "frames[%d] = %d outside 2..2^20", i, frames[i]);
        Tsum += frames[i];
    }
    if (Tsum > (1 << 20)) return set_error(WLX_ERR_ARG, "%ld frames in all exceed 2^20", Tsum);
    return spk_debug_pool_run(device, x, F, n, frames, Tsum, C, eps, out);
}

// The ragged filterbank and mean removal over n windows of ONE upload, as spk_enqueue_batch launches them: item i is the frames[i] frames
// from sample offsets[i] on (any offset: windows may overlap and come in any order), outputs packed back to back in item order.
extern "C" int32_t wlx_spk_debug_fbank_batch(int32_t device, const float* pcm, int64_t n_samples, int32_t n, const int64_t* offsets,
                                             const int32_t* frames, int32_t n_mels, float* frames_out, uint16_t* image_out) {
    if (!pcm || !offsets || !frames || !frames_out || !image_out) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_SPK_MAX_BATCH) return set_error(WLX_ERR_ARG, "%d items outside 1..%d", n, WLX_SPK_MAX_BATCH);
    if (n_mels < 1 || n_mels > 256) return set_error(WLX_ERR_ARG, "n_mels %d outside 1..256", n_mels);
    if (n_samples < WLX_SPK_FRAME || n_samples > (1LL << 28)) return set_error(WLX_ERR_ARG, "n_samples %lld outside 400..2^28", (long long)n_samples);
    long offs[WLX_SPK_MAX_BATCH];
    long Tsum = 0;
    for (int i = 0; i < n; ++i) {
        if (frames[i] < 1 || frames[i] > (1 << 20)) return set_error(WLX_ERR_ARG, "frames[%d] = %d outside 1..2^20", i, frames[i]);
        if (offsets[i] < 0 || offsets[i] > n_samples - WLX_SPK_FRAME - (int64_t)(frames[i] - 1) * WLX_SPK_SHIFT)
            return set_error(WLX_ERR_ARG, "item %d: %d frames from sample %lld on leave the %lld samples", i, frames[i], (long long)offsets[i],
                             (long long)n_samples);
        offs[i] = (long)offsets[i];
        Tsum += frames[i];
    }
    if (Tsum > (1 << 20)) return set_error(WLX_ERR_ARG, "%ld frames in all exceed 2^20", Tsum);
    HookScope S;
    CKR(S.begin(device));
    float *window, *twiddle, *mel, *dpcm, *dlm;
    half_t* d16;
    CKR(upload_tables(S.allocs, n_mels, &window, &twiddle, &mel));
    CKR(S.upload(&dpcm, pcm, (size_t)n_samples));
    CKR(S.alloc(&dlm, (size_t)Tsum * n_mels));
    CKR(S.alloc(&d16, (size_t)Tsum * n_mels));
    if (!launch_spk_fbank_batch(dpcm, offs, frames, n, window, twiddle, mel, n_mels, dlm, S.st) ||
        !launch_spk_cmn_batch(dlm, frames, n, n_mels, d16, S.st))
        return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(frames_out, dlm, (size_t)Tsum * n_mels));
    CKR(S.download(h16(image_out), d16, (size_t)Tsum * n_mels));
    return S.finish();
}

// The embedding head: W rounded to fp16 as spk_load rounds seg_1.weight, the linear layer alone (normalize = 0) or with the l2norm
// behind it (normalize = 1); rows of `emb` past n are not touched.
extern "C" int32_t wlx_spk_debug_head(int32_t device, const float* pooled, const float* W, const float* b, int32_t n, int32_t D, int32_t E,
                                      int32_t normalize, float* emb) {
    if (!pooled || !W || !b || !emb) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > 65535 || D < 8 || D % 8 || D > (1 << 16) || E < 1 || E > (1 << 16) || (long)E * D > (1L << 26))
        return set_error(WLX_ERR_ARG, "n %d / D %d / E %d: n in 1..65535, D a multiple of 8 and E >= 1, both up to 2^16, E D up to 2^26", n, D, E);
    if (normalize != 0 && normalize != 1) return set_error(WLX_ERR_ARG, "normalize %d must be 0 or 1", normalize);
    std::vector<half_t> w16((size_t)E * D);          // (declared before S: it outlives the stream's copy on every return path)
    for (size_t i = 0; i < w16.size(); ++i) w16[i] = (half_t)W[i];
    HookScope S;
    CKR(S.begin(device));
    float *dx, *db, *demb;
    half_t* dW;
    CKR(S.upload(&dx, pooled, (size_t)n * D));
    CKR(S.upload(&dW, w16.data(), w16.size()));
    CKR(S.upload(&db, b, (size_t)E));
    CKR(S.alloc(&demb, (size_t)n * E));
    if (!launch_spk_head_batch(dx, dW, db, E, D, n, demb, S.st, normalize != 0)) return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(emb, demb, (size_t)n * E));
    return S.finish();
}

// ---- the clustering kernels (spk_cluster.hip), one launch each over files packed back to back: file f at row0 = ns[0] + .. + ns[f-1], its
// matrix at ns[0]^2 + .. + ns[f-1]^2. wlx_spk_debug_affinity / _ahc are the case of one file behind refusals of their own.
static int spk_debug_many_table(const int32_t* ns, int n_files, const wlx_spk_cluster_opts* opts, std::vector<SpkClusterFile>& files, size_t& rows,
                                size_t& cells) {
    if (n_files < 1 || n_files > WLX_SPK_MANY_MAX_FILES) return set_error(WLX_ERR_ARG, "%d files outside 1..%d", n_files, WLX_SPK_MANY_MAX_FILES);
    rows = cells = 0;
    for (int f = 0; f < n_files; ++f) {
        if (ns[f] < 1 || ns[f] > WLX_SPK_CLUSTER_MAX) return set_error(WLX_ERR_ARG, "ns[%d] = %d outside 1..%d", f, ns[f], WLX_SPK_CLUSTER_MAX);
        files.push_back(SpkClusterFile{cells, (int)rows, ns[f], opts ? opts[f].threshold : 0.f, opts ? opts[f].max_clusters : 0});
        rows += (size_t)ns[f], cells += (size_t)ns[f] * ns[f];
    }
    if (rows > WLX_SPK_MANY_MAX_ROWS || cells > (size_t)WLX_SPK_MANY_MAX_CELLS)
        return set_error(WLX_ERR_ARG, "%zu rows / %zu matrix floats in all exceed %d / %zu", rows, cells, WLX_SPK_MANY_MAX_ROWS, (size_t)WLX_SPK_MANY_MAX_CELLS);
    return WLX_OK;
}

extern "C" int32_t wlx_spk_debug_affinity_many(int32_t device, const float* X, int32_t n_files, const int32_t* ns, int32_t dim, float* dist_out) {
    if (!X || !ns || !dist_out) return set_error(WLX_ERR_ARG, "null argument");
    if (dim < 1 || dim > 1024) return set_error(WLX_ERR_ARG, "dim %d outside 1..1024", dim);
    std::vector<SpkClusterFile> files;
    size_t rows, cells;
    CKR(spk_debug_many_table(ns, n_files, nullptr, files, rows, cells));
    HookScope S;
    CKR(S.begin(device));
    float *dX, *dD;
    CKR(S.upload(&dX, X, rows * dim));
    CKR(S.alloc(&dD, cells));
    if (!launch_spk_affinity(dX, files.data(), n_files, dim, dD, S.st)) return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(dist_out, dD, cells));
    return S.finish();
}

extern "C" int32_t wlx_spk_debug_affinity(int32_t device, const float* X, int32_t n, int32_t dim, float* dist_out) {
    if (!X || !dist_out) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_SPK_CLUSTER_MAX || dim < 1 || dim > 1024)
        return set_error(WLX_ERR_ARG, "n %d / dim %d: n in 1..%d, dim in 1..1024", n, dim, WLX_SPK_CLUSTER_MAX);
    return wlx_spk_debug_affinity_many(device, X, 1, &n, dim, dist_out);
}

// The caller's heights and merges hold rows - `less` entries: copied in and out, so what no merge writes comes back unchanged
static int spk_debug_ahc_run(const char* who, int device, const float* dist, const int32_t* ns, int n_files, const wlx_spk_cluster_opts* opts,
                             size_t less, int32_t* labels, int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters) {
    std::vector<SpkClusterFile> files;
    size_t rows, cells;
    CKR(spk_debug_many_table(ns, n_files, opts, files, rows, cells));
    for (int f = 0; f < n_files; ++f) CKR(spk_cluster_opts_ok(who, &opts[f]));
    const size_t nh = rows - less;
    std::vector<int> counts((size_t)2 * n_files, 0);          // (declared before S: it outlives the stream's copies on every return path)
    HookScope S;
    CKR(S.begin(device));
    float *dD, *dH;
    int *dM, *dL, *dC;
    const size_t room = std::max(nh, (size_t)1);              // (one row merges nothing: one entry of room, never written)
    CKR(S.upload(&dD, dist, cells));
    CKR(S.upload(&dH, nh ? heights : nullptr, room));
    CKR(S.upload(&dM, nh ? merges : nullptr, 2 * room));
    CKR(S.alloc(&dL, rows));
    CKR(S.alloc(&dC, (size_t)2 * n_files));
    if (!launch_spk_ahc(dD, files.data(), n_files, dM, dH, dL, dC, S.st)) return set_error(WLX_ERR_ARG, "the launcher refused the shape");
    CKR(S.download(labels, dL, rows));
    if (nh) {
        CKR(S.download(heights, dH, nh));
        CKR(S.download(merges, dM, 2 * nh));
    }
    CKR(S.download(counts.data(), dC, (size_t)2 * n_files));
    CKR(S.finish());
    for (int f = 0; f < n_files; ++f) n_merges[f] = counts[2 * f], n_clusters[f] = counts[2 * f + 1];
    return WLX_OK;
}

// heights [n - 1] and merges [n - 1][2]: one file's merges start at row 0 and end inside them
extern "C" int32_t wlx_spk_debug_ahc(int32_t device, const float* dist, int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels,
                                     int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters) {
    if (!dist || !opts || !labels || !merges || !heights || !n_merges || !n_clusters) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_SPK_CLUSTER_MAX) return set_error(WLX_ERR_ARG, "n %d outside 1..%d", n, WLX_SPK_CLUSTER_MAX);
    return spk_debug_ahc_run("wlx_spk_debug_ahc", device, dist, &n, 1, opts, 1, labels, merges, heights, n_merges, n_clusters);
}

// heights [rows] and merges [rows][2], file f's at its row0
extern "C" int32_t wlx_spk_debug_ahc_many(int32_t device, const float* dist, int32_t n_files, const int32_t* ns, const wlx_spk_cluster_opts* opts,
                                          int32_t* labels, int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters) {
    if (!dist || !ns || !opts || !labels || !merges || !heights || !n_merges || !n_clusters) return set_error(WLX_ERR_ARG, "null argument");
    return spk_debug_ahc_run("wlx_spk_debug_ahc_many", device, dist, ns, n_files, opts, 0, labels, merges, heights, n_merges, n_clusters);
}
