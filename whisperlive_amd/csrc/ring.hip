// ring.hip — the write side of the device PCM rings (include/wlx.h wlx_ring_*, wlx_ring_group_*; engine.h RingStore):
// whisper_live/backend/base.py:173-234 on the device. One store, one trim-and-grow rule, one append behind the mono ring and the
// ring group, and the ring half of PcmLease, through which the readers come: wlx_logmel_ring (engine.hip), wlx_vad_probs_resident
// (vad.hip), wlx_spk_embed_ring_batch (spk_engine.hip).
#include "engine.h"
#include <algorithm>

using namespace wlx;

static void store_free(wlx_ring_group* st) {
    (void)hipSetDevice(st->device);
    if (st->stream) (void)hipStreamSynchronize(st->stream);
    for (wlx_ring* r : st->lanes) {
        if (r->read_pending && r->last_read) (void)hipEventSynchronize(r->last_read);   // a reader launched on the lane has run
        if (r->last_read) (void)hipEventDestroy(r->last_read);
        delete r;
    }
    if (st->stream) (void)hipStreamDestroy(st->stream);
    if (st->buf) (void)hipFree(st->buf);
    resample_stream_free(st->fmt);
    delete st;
}

// split: a group's store, one lane per channel, with its wire format from the start; else the one lane of a mono ring, no format yet
static int store_create(const char* fn, wlx_engine* e, int64_t capacity_samples, bool split, int32_t sample_format, int32_t channels,
                        int32_t sample_rate, wlx_ring_group** out) {
    if (capacity_samples < 0 || capacity_samples > 16000LL * 3600) return set_error(WLX_ERR_ARG, "ring capacity out of range");
    if (split) CKR(resample_stream_check(sample_format, channels, sample_rate));
    const int n_lanes = split ? channels : 1;
    CK(hipSetDevice(e->device));
    wlx_ring_group* st = new wlx_ring_group();
    st->device = e->device; st->split = split; st->lone = !split;
    st->cap = (size_t)(capacity_samples > 0 ? capacity_samples : 16000LL * 64);
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&st->buf), (size_t)n_lanes * st->cap * sizeof(float));   // owned by name: make_room grows it
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking);
    for (int c = 0; c < n_lanes && he == hipSuccess; ++c) {
        wlx_ring* r = new wlx_ring();
        r->device = e->device; r->store = st; r->buf = st->buf + (size_t)c * st->cap;
        st->lanes.push_back(r);
        he = hipEventCreateWithFlags(&r->last_read, hipEventDisableTiming);
    }
    int rc = WLX_OK;
    if (he != hipSuccess) {
        (void)hipGetLastError();
        rc = set_error(WLX_ERR_HIP, "%s: %s", fn, hipGetErrorString(he));
    } else if (split) {
        rc = resample_stream_open(e->device, sample_format, channels, sample_rate, &st->fmt);
        st->has_format = rc == WLX_OK;
    }
    if (rc != WLX_OK) { store_free(st); return rc; }
    *out = st;
    return WLX_OK;
}

// ---- PcmLease (engine.h): the ring half. No append, trim or growth while the lease is held.
void PcmLease::open_ring(wlx_ring* r) {
    lane_ = std::unique_lock<std::mutex>(r->mu);
    r_ = r;
    buf = r->buf, base = r->base, resident = r->resident;
}

// a reader launched from ANOTHER stream may still be pending: its event is about to be re-recorded on this stream, so this stream first
// waits for it (the new record then stands for both; one session = one slot = one stream makes this the rare case)
int PcmLease::before_launch(hipStream_t reader) {
    if (r_->read_pending && r_->last_read_stream != reader) CK(hipStreamWaitEvent(reader, r_->last_read, 0));
    return WLX_OK;
}

// a later trim or growth waits for this launch before it moves the samples (wait_readers)
int PcmLease::launched(hipStream_t reader) {
    CK(hipEventRecord(r_->last_read, reader));
    r_->read_pending = true;
    r_->last_read_stream = reader;
    return WLX_OK;
}

// readers launched but possibly not run yet: wait for them before data moves under them
static int wait_readers(RingStore* st) {
    for (wlx_ring* r : st->lanes)
        if (r->read_pending) { CK(hipEventSynchronize(r->last_read)); r->read_pending = false; }
    return WLX_OK;
}

// The front half of every append (the store's and the lanes' mutexes are held): the trim rule of add_frames, then room for n more
// samples behind the resident ones, for all lanes in lockstep — ONE trim decision, at most ONE growth.
static int make_room(RingStore* st, int64_t n, int64_t max_resident, int64_t trim, int64_t* dropped_out) {
    const int64_t resident = st->lanes[0]->resident;
    int64_t dropped = 0, keep = resident;
    if (max_resident > 0 && trim > 0 && resident > max_resident) {
        // add_frames (base.py:191-198): the buffer is past its cap — the oldest `trim` samples go, the rest moves to the front
        dropped = std::min<int64_t>(trim, resident);
        keep = resident - dropped;
        CKR(wait_readers(st));
        for (wlx_ring* r : st->lanes)
            for (int64_t done = 0; done < keep; done += dropped) {                  // pieces of <= `dropped` samples: source and destination never overlap
                const int64_t m = std::min<int64_t>(dropped, keep - done);
                CK(hipMemcpyAsync(r->buf + done, r->buf + dropped + done, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, st->stream));
            }
        for (wlx_ring* r : st->lanes) { r->base += dropped; r->resident = keep; }
    }
    if ((size_t)(keep + n) > st->cap) {                                            // a packet larger than the head-room: grow (rare)
        size_t cap = st->cap;
        while (cap < (size_t)(keep + n)) cap *= 2;
        float* nb = nullptr;
        CK(hipMalloc(reinterpret_cast<void**>(&nb), st->lanes.size() * cap * sizeof(float)));   // replaces st->buf, which is freed below: no free list
        CKR(wait_readers(st));
        for (size_t c = 0; c < st->lanes.size() && keep > 0; ++c)
            CK(hipMemcpyAsync(nb + c * cap, st->lanes[c]->buf, (size_t)keep * sizeof(float), hipMemcpyDeviceToDevice, st->stream));
        CK(hipStreamSynchronize(st->stream));
        CK(hipFree(st->buf));
        st->buf = nb; st->cap = cap;
        for (size_t c = 0; c < st->lanes.size(); ++c) st->lanes[c]->buf = nb + c * cap;
    }
    *dropped_out = dropped;
    return WLX_OK;
}

// Every append, under the name `fn` of its entry point. wire: `data` is n wire frames for the store's format, resampled into the
// lanes, and new_out [lanes][cap] takes the new samples back; else n 16 kHz floats for the one lane. Every refusal comes before
// anything is staged or launched and changes nothing.
static int store_append(const char* fn, RingStore* st, bool wire, const void* data, int64_t n, int32_t flush, int64_t max_resident,
                        int64_t trim, float* new_out, int64_t cap, int64_t* n_new_out, int64_t* dropped_out, int64_t* base_out,
                        int64_t* resident_out) {
    std::lock_guard<std::mutex> lk(st->mu);
    if (wire && !st->has_format) return set_error(WLX_ERR_STATE, "%s: the ring has no wire format (wlx_ring_set_format)", fn);
    if (!wire && st->has_format) return set_error(WLX_ERR_STATE, "%s: the ring has a wire format (wlx_ring_append_frames)", fn);
    ResampleStream& rs = st->fmt;
    int64_t n_new = n;
    if (wire) {
        if (rs.closed) return set_error(WLX_ERR_STATE, "%s: the stream has been flushed", fn);
        if (n > (1LL << 50) - rs.J) return set_error(WLX_ERR_ARG, "frame count out of range");
        n_new = resample_stream_next(rs, n, flush);
    }
    if (n_new > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    if (new_out && cap < n_new)
        return set_error(WLX_ERR_ARG, "%s: %lld new samples%s, room for %lld", fn, (long long)n_new, st->split ? " per lane" : "", (long long)cap);
    std::vector<std::unique_lock<std::mutex>> held;             // no reader is launched on any lane while the store changes
    held.reserve(st->lanes.size());
    for (wlx_ring* r : st->lanes) held.emplace_back(r->mu);
    CK(hipSetDevice(st->device));
    if (wire) CKR(resample_stream_reserve(rs, n));
    int64_t dropped = 0;
    CKR(make_room(st, n_new, max_resident, trim, &dropped));
    const int64_t resident = st->lanes[0]->resident;
    float* dst = st->buf + resident;                            // lane c's write position is dst + c * st->cap
    if (wire) CKR(resample_stream_enqueue(rs, data, n, flush, dst, st->stream, st->split ? (long long)st->cap : 0));   // (0: the down-mix)
    else if (n > 0) CK(hipMemcpyAsync(dst, data, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st->stream));
    if (new_out && n_new > 0) {                                 // ONE copy back: row c = lane c's new samples, host row stride `cap`
        if (st->lanes.size() == 1) CK(hipMemcpyAsync(new_out, dst, (size_t)n_new * sizeof(float), hipMemcpyDeviceToHost, st->stream));
        else CK(hipMemcpy2DAsync(new_out, (size_t)cap * sizeof(float), dst, st->cap * sizeof(float), (size_t)n_new * sizeof(float), st->lanes.size(),
                                 hipMemcpyDeviceToHost, st->stream));
    }
    CK(hipStreamSynchronize(st->stream));           // ONE wait: the caller's buffer may be reused, new_out is filled, readers see the samples
    for (wlx_ring* r : st->lanes) r->resident = resident + n_new;
    st->appended = true;
    if (n_new_out) *n_new_out = n_new;
    if (dropped_out) *dropped_out = dropped;
    if (base_out) *base_out = st->lanes[0]->base;
    if (resident_out) *resident_out = resident + n_new;
    return WLX_OK;
}

// a lane of a group is a reader's handle: the group has the format and does the appending
static int refuse_lane(const char* fn, const wlx_ring* r, const char* instead) {
    return r->store->lone ? WLX_OK : set_error(WLX_ERR_STATE, "%s: the ring is a lane of a ring group%s", fn, instead);
}

// ------------------------------------------------------------------------------------------------ mono ring
extern "C" int32_t wlx_ring_create(wlx_engine* e, int64_t capacity_samples, wlx_ring** out) {
    if (!e || !out) return set_error(WLX_ERR_ARG, "null argument");
    wlx_ring_group* st = nullptr;
    CKR(store_create("wlx_ring_create", e, capacity_samples, false, 0, 0, 0, &st));
    *out = st->lanes[0];
    return WLX_OK;
}

extern "C" void wlx_ring_destroy(wlx_ring* r) {
    if (!r || !r->store->lone) return;              // a lane is borrowed: wlx_ring_group_destroy frees it
    store_free(static_cast<wlx_ring_group*>(r->store));
}

extern "C" int32_t wlx_ring_append(wlx_ring* r, const float* samples, int64_t n, int64_t max_resident, int64_t trim,
                                   int64_t* dropped_out, int64_t* base_out, int64_t* resident_out) {
    if (!r || n < 0 || (n > 0 && !samples)) return set_error(WLX_ERR_ARG, "wlx_ring_append: bad argument");
    if (n > 16000LL * 3600) return set_error(WLX_ERR_ARG, "audio chunk too long");
    CKR(refuse_lane("wlx_ring_append", r, " (wlx_ring_group_append_frames)"));
    return store_append("wlx_ring_append", r->store, false, samples, n, 0, max_resident, trim, nullptr, 0, nullptr, dropped_out, base_out,
                        resident_out);
}

// the live path's wire format (include/wlx.h): the packets are resampled into the ring by the stream form of resample.hip
extern "C" int32_t wlx_ring_set_format(wlx_ring* r, int32_t sample_format, int32_t channels, int32_t sample_rate) {
    if (!r) return set_error(WLX_ERR_ARG, "null ring");
    CKR(resample_stream_check(sample_format, channels, sample_rate));
    CKR(refuse_lane("wlx_ring_set_format", r, ", which has the format"));
    RingStore* st = r->store;
    std::lock_guard<std::mutex> lk(st->mu);
    if (st->has_format) return set_error(WLX_ERR_STATE, "wlx_ring_set_format: the ring has a format already");
    if (st->appended) return set_error(WLX_ERR_STATE, "wlx_ring_set_format: the ring has been appended to");
    CKR(resample_stream_open(st->device, sample_format, channels, sample_rate, &st->fmt));
    st->has_format = true;
    return WLX_OK;
}

extern "C" int32_t wlx_ring_append_frames(wlx_ring* r, const void* frames, int64_t n_frames, int32_t flush, int64_t max_resident,
                                          int64_t trim, float* new_out, int64_t cap, int64_t* n_new_out, int64_t* dropped_out,
                                          int64_t* base_out, int64_t* resident_out) {
    if (!r || n_frames < 0 || (n_frames > 0 && !frames)) return set_error(WLX_ERR_ARG, "wlx_ring_append_frames: bad argument");
    if (new_out && cap < 0) return set_error(WLX_ERR_ARG, "wlx_ring_append_frames: negative capacity");
    CKR(refuse_lane("wlx_ring_append_frames", r, " (wlx_ring_group_append_frames)"));
    return store_append("wlx_ring_append_frames", r->store, true, frames, n_frames, flush, max_resident, trim, new_out, cap, n_new_out,
                        dropped_out, base_out, resident_out);
}

extern "C" int32_t wlx_ring_state(wlx_ring* r, int64_t* base_out, int64_t* resident_out) {
    if (!r) return set_error(WLX_ERR_ARG, "null ring");
    std::lock_guard<std::mutex> lk(r->mu);
    if (base_out) *base_out = r->base;
    if (resident_out) *resident_out = r->resident;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------ ring group
extern "C" int32_t wlx_ring_group_create(wlx_engine* e, int64_t capacity_samples, int32_t sample_format, int32_t channels,
                                         int32_t sample_rate, wlx_ring_group** out) {
    if (!e || !out) return set_error(WLX_ERR_ARG, "null argument");
    return store_create("wlx_ring_group_create", e, capacity_samples, true, sample_format, channels, sample_rate, out);
}

extern "C" void wlx_ring_group_destroy(wlx_ring_group* g) {
    if (g) store_free(g);
}

extern "C" int32_t wlx_ring_group_lane(wlx_ring_group* g, int32_t channel, wlx_ring** out) {
    if (!g || !out) return set_error(WLX_ERR_ARG, "null argument");
    const int channels = (int)g->lanes.size();
    if (channel < 0 || channel >= channels) return set_error(WLX_ERR_ARG, "wlx_ring_group_lane: lane %d outside 0..%d", channel, channels - 1);
    *out = g->lanes[(size_t)channel];
    return WLX_OK;
}

extern "C" int32_t wlx_ring_group_append_frames(wlx_ring_group* g, const void* frames, int64_t n_frames, int32_t flush, int64_t max_resident,
                                                int64_t trim, float* new_out, int64_t cap, int64_t* n_new_out, int64_t* dropped_out,
                                                int64_t* base_out, int64_t* resident_out) {
    if (!g || n_frames < 0 || (n_frames > 0 && !frames)) return set_error(WLX_ERR_ARG, "wlx_ring_group_append_frames: bad argument");
    if (new_out && cap < 0) return set_error(WLX_ERR_ARG, "wlx_ring_group_append_frames: negative capacity");
    return store_append("wlx_ring_group_append_frames", g, true, frames, n_frames, flush, max_resident, trim, new_out, cap, n_new_out,
                        dropped_out, base_out, resident_out);
}
