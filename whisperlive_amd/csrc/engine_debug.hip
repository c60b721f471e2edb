// engine_debug.hip — the wlx_debug_* hooks of the Whisper engine (tests, scripts/trace_step.py, bench.py probes): injected-logits search, logits
// read-back, teacher-forced logits, and the three decode-step hooks (time, in-kernel trace, per-kernel profile).
#include "engine.h"
#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace wlx;

// the production search launches (launch_search, through generate_impl's loop) on caller-supplied logits: `batch` items, rows = batch * R
// per step, R = beam_size (beam mode) or num_hypotheses (sampling / greedy). Everything is checked before anything is launched or written.
extern "C" int32_t wlx_debug_search_batch(wlx_engine* e, int32_t slot, const float* logits, int32_t steps, int32_t batch,
                                          const int32_t* prompts, const int32_t* prompt_lens, int32_t prompt_stride, const wlx_gen_opts* opts,
                                          int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out, float* scores_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!logits || !prompts || !prompt_lens || !opts || !tokens_out || !n_tokens_out || !scores_out) return set_error(WLX_ERR_ARG, "null argument");
    if (batch < 1 || batch > s->B) return set_error(WLX_ERR_ARG, "batch %d out of range (slot max %d)", batch, s->B);
    if (steps < 1) return set_error(WLX_ERR_ARG, "steps %d: at least one step of logits", steps);
    CK(hipSetDevice(e->device));
    return generate_impl(e, s, batch, prompts, prompt_lens, prompt_stride, nullptr, opts, true, logits, steps, tokens_out, tokens_stride,
                         n_tokens_out, scores_out, nullptr);
}

extern "C" int32_t wlx_debug_search(wlx_engine* e, int32_t slot, const float* logits, int32_t steps,
                                    const int32_t* prompt, int32_t prompt_len, const wlx_gen_opts* opts,
                                    int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out, float* scores_out) {
    return wlx_debug_search_batch(e, slot, logits, steps, 1, prompt, &prompt_len, prompt_len, opts, tokens_out, tokens_stride, n_tokens_out, scores_out);
}

// ------------------------------------------------------------------------------------------------
// test hooks
extern "C" int32_t wlx_debug_logits_get(wlx_engine* e, int32_t slot, float* out, int32_t rows, int64_t cap_floats) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    const int V = e->spec.vocab;
    if (!out || rows < 1 || rows > s->rows_cap || (int64_t)rows * V > cap_floats) return set_error(WLX_ERR_ARG, "bad rows/cap");
    CK(hipSetDevice(e->device));
    CK(hipMemcpy2DAsync(out, (size_t)V * 4, s->logits, (size_t)s->ldl * 4, (size_t)V * 4, rows, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

extern "C" int32_t wlx_debug_decode_logits(wlx_engine* e, int32_t slot, const int32_t* tokens, int32_t n, float* out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!tokens || !out || n < 1 || n > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "bad tokens");
    if (s->enc_batch < 1) return set_error(WLX_ERR_STATE, "decode before encode");
    for (int i = 0; i < n; ++i) if (tokens[i] < 0 || tokens[i] >= e->spec.vocab) return set_error(WLX_ERR_ARG, "token out of vocabulary");
    CK(hipSetDevice(e->device));
    std::vector<short> anc(WLX_T_TEXT, 0);   // cache row 0, identity ancestry
    CKR(set_anc_rows(s, anc, 0, 1));
    CKR(prefill_tokens(e, s, 0, 0, tokens, 0, n, out, -1, 0, nullptr));
    CK(hipStreamSynchronize(s->stream));
    return WLX_OK;
}

// ---- what the three decode-step hooks share
// One synthetic decode step of `rows` rows at position t with identity history (cache content is whatever is there). Up to 16 rows: one
// item with `rows` beams (*tR = rows, *tG = 1); more: rows / R items of R beams each, as a batched decode has them. Validates (rows, t)
// and uploads the identity row tables and ancestry.
static int step_hook_setup(Slot* s, int rows, int t, int* tR, int* tG) {
    if (rows < 1 || rows > s->cache_rows || rows > s->rows_cap || t < 0 || t >= WLX_T_TEXT) return set_error(WLX_ERR_ARG, "bad arguments");
    if (rows > 16 && (rows % s->R != 0 || rows / s->R > s->B)) return set_error(WLX_ERR_ARG, "more than 16 rows: a multiple of the slot's rows per item");
    if (s->enc_batch < 1) return set_error(WLX_ERR_STATE, "decode before encode");
    *tR = rows > 16 ? s->R : rows; *tG = rows / *tR;
    std::vector<int> tk(rows, 0), ps(rows, t), ca(rows), an(rows), gi(*tG, 0);
    for (int g = 0; g < *tG; ++g) gi[g] = g % std::max(1, s->enc_batch);
    std::vector<short> anc((size_t)rows * WLX_T_TEXT);
    for (int r = 0; r < rows; ++r) { ca[r] = an[r] = r; for (int p = 0; p < WLX_T_TEXT; ++p) anc[(size_t)r * WLX_T_TEXT + p] = (short)r; }
    CKR(set_anc_rows(s, anc, 0, rows));
    return upload_rows(s, tk, ps, ca, an, gi);
}

// captures what `body` launches on the slot stream into a graph, replays it 3 times to warm up and `iters` times between the slot's
// ev0 / ev1; *ms_out = the time of the `iters` replays
template <class F>
static int time_captured(Slot* s, F&& body, int iters, float* ms_out) {
    hipStream_t st = s->stream;
    hipGraph_t graph; hipGraphExec_t exec;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    body();
    CK(hipStreamEndCapture(st, &graph));
    CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    CK(hipGraphDestroy(graph));
    for (int i = 0; i < 3; ++i) CK(hipGraphLaunch(exec, st));
    CK(hipEventRecord(s->ev0, st));
    for (int i = 0; i < iters; ++i) CK(hipGraphLaunch(exec, st));
    CK(hipEventRecord(s->ev1, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(ms_out, s->ev0, s->ev1));
    CK(hipGraphExecDestroy(exec));
    return WLX_OK;
}

extern "C" int32_t wlx_debug_time_decode_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t iters,
                                              float* avg_ms_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (iters < 1 || !avg_ms_out) return set_error(WLX_ERR_ARG, "bad arguments");
    s->busy_variant = device_is_busy(s);     // (the launch shapes a step captured now would use)
    CK(hipSetDevice(e->device));
    int tR, tG;
    CKR(step_hook_setup(s, rows, t, &tR, &tG));
    CK(hipMemsetAsync(s->st.done, 0, 4, s->stream));
    decoder_pass(e, s, s->step, rows, tR, tG, true, true);      // eager first (dynamic-LDS limits are raised outside capture)
    float ms = 0.f;
    CKR(time_captured(s, [&] { decoder_pass(e, s, s->step, rows, tR, tG, true, true); }, iters, &ms));    // (one step per graph: engine_decode.hip graph_steps_for)
    *avg_ms_out = ms / (float)iters;
    return WLX_OK;
}

// In-kernel timeline of ONE decode step (scripts/trace_step.py). Only libwlx_trace.so (-DWLX_TRACE) records anything;
// the production library reports WLX_ERR_STATE. out: [n_launches][WLX_TR_STRIDE] u64 records, names: [n_launches][48].
extern "C" int32_t wlx_debug_trace_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t with_search,
                                        uint64_t* out, int64_t cap_u64, char* names, int32_t* n_launches_out) {
#ifndef WLX_TRACE
    (void)e; (void)slot; (void)rows; (void)t; (void)with_search; (void)out; (void)cap_u64; (void)names; (void)n_launches_out;
    return set_error(WLX_ERR_STATE, "libwlx.so was built without -DWLX_TRACE (use libwlx_trace.so, scripts/trace_step.py)");
#else
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!out || !names || !n_launches_out) return set_error(WLX_ERR_ARG, "bad arguments");
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    int tR, tG;
    CKR(step_hook_setup(s, rows, t, &tR, &tG));                 // (validates before anything is allocated; reset_state uploads again)
    const size_t max_launch = 320;
    unsigned long long* buf = nullptr;
    CK(hipMalloc(&buf, max_launch * WLX_TR_STRIDE * 8));       // lives for this call only, freed on its way out
    g_trace_buf = buf; g_trace_seq = 0;
    hipGraph_t graph; hipGraphExec_t exec;
    auto reset_state = [&]() -> int {
        CKR(step_hook_setup(s, rows, t, &tR, &tG));
        CK(hipMemsetAsync(s->st.done, 0, 4, st)); CK(hipMemsetAsync(s->st.item_done, 0, 4, st));
        CK(hipMemsetAsync(s->st.n_hyp, 0, 4, st)); CK(hipMemsetAsync(s->st.n_finished, 0, 4, st));
        static const int rule0[16 * 4] = {0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0,
                                          0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0, 0, 1, -1, 0};
        CK(hipMemcpyAsync(s->st.rule, rule0, (size_t)rows * 16, hipMemcpyHostToDevice, st));
        return WLX_OK;
    };
    CKR(reset_state());
    { const int seq0 = g_trace_seq; unsigned long long* b0 = g_trace_buf; g_trace_buf = nullptr;   // eager pass (LDS limits), untraced
      decoder_pass(e, s, s->step, rows, tR, tG, true, true); g_trace_seq = seq0; g_trace_buf = b0; }
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    decoder_pass(e, s, s->step, rows, tR, tG, true, true);
    if (with_search) launch_search(e, s, rows, tR, tG, false);
    CK(hipStreamEndCapture(st, &graph));
    CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    CK(hipGraphDestroy(graph));
    const int n = g_trace_seq;
    g_trace_buf = nullptr;
    if (n > (int)max_launch) { (void)hipGraphExecDestroy(exec); (void)hipFree(buf); return set_error(WLX_ERR_ARG, "trace: %d launches exceed the trace buffer (%d)", n, (int)max_launch); }
    for (int i = 0; i < 3; ++i) { CKR(reset_state()); CK(hipGraphLaunch(exec, st)); }
    CKR(reset_state());
    CK(hipMemsetAsync(buf, 0, max_launch * WLX_TR_STRIDE * 8, st));
    CK(hipStreamSynchronize(st));
    CK(hipGraphLaunch(exec, st));
    CK(hipStreamSynchronize(st));
    CK(hipGraphExecDestroy(exec));
    if ((int64_t)n * WLX_TR_STRIDE > cap_u64) { (void)hipFree(buf); return set_error(WLX_ERR_ARG, "trace buffer too small"); }
    CK(hipMemcpyAsync(out, buf, (size_t)n * WLX_TR_STRIDE * 8, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    CK(hipFree(buf));
    for (int i = 0; i < n; ++i) { strncpy(names + (size_t)i * 48, g_trace_names[i] ? g_trace_names[i] : "?", 47); names[(size_t)i * 48 + 47] = 0; }
    *n_launches_out = n;
    return WLX_OK;
#endif
}

extern "C" int32_t wlx_debug_profile_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t iters,
                                          wlx_kernel_stat* out, int32_t cap, int32_t* n_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (iters < 1 || !out || !n_out || cap < 1) return set_error(WLX_ERR_ARG, "bad arguments");
    s->busy_variant = device_is_busy(s);     // (the launch shapes a step captured now would use)
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    int tR, tG;
    CKR(step_hook_setup(s, rows, t, &tR, &tG));
    CK(hipMemsetAsync(s->st.done, 0, 4, st));
    for (int i = 0; i < 2; ++i) decoder_pass(e, s, s->step, rows, tR, tG, true, true);                                   // warm caches / code objects
    CK(hipStreamSynchronize(st));
    Prof prof;
    prof.t = t;
    s->prof = &prof;
    decoder_pass(e, s, s->step, rows, tR, tG, true, true);                                                               // pass 1: list the launches of one step
    struct Agg { int launches = 0; double bytes = 0, us = 0; };
    std::map<std::string, Agg> agg;
    for (auto& r : prof.recs) { Agg& a = agg[r.name]; a.launches += 1; a.bytes += r.bytes; }
    // pass 2, per kernel name: a graph with just that kernel's launches of the step (back to back on the slot stream, so
    // each pays the dependent-launch boundary exactly as inside the real step), replayed `iters` times between one
    // HIP-event pair. An event pair around every single 2-5 us launch measured the events, not the kernels.
    prof.list_only = false;
    int rc = WLX_OK;
    for (auto& kv : agg) {
        prof.only = kv.first;
        float ms = 0.f;
        rc = time_captured(s, [&] { decoder_pass(e, s, s->step, rows, tR, tG, true, true); }, iters, &ms);
        if (rc != WLX_OK) break;
        kv.second.us = 1000.0 * ms / iters;                                       // all launches of this kernel in one step
    }
    s->prof = nullptr;
    if (rc != WLX_OK) return set_error(rc, "profile capture failed");
    CK(hipGetLastError());
    int n = 0;
    for (auto& kv : agg) {
        if (n >= cap) break;
        wlx_kernel_stat& o = out[n++];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", kv.first.c_str());
        o.launches_per_step = (float)kv.second.launches;
        o.avg_us = (float)(kv.second.us / kv.second.launches);
        o.total_us_per_step = (float)kv.second.us;
        o.bytes_per_launch = kv.second.bytes / kv.second.launches;
    }
    *n_out = n;
    return WLX_OK;
}
