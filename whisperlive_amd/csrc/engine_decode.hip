// engine_decode.hip — the decode half of the Whisper engine: decoder pass, prompt prefill, step graphs, search parameters and options,
// wlx_generate, language detection and word alignment (engine.hip: slots, audio, encoder; engine.h: what the files share).
#include "engine.h"
#include "grammar_table.h"
#include <sched.h>
#include <limits>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>

using namespace wlx;

// one polite spin-wait iteration (the decode loop polls a pinned word): the ISA's spin hint where there is one
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    asm volatile("" ::: "memory");
#endif
}

// ------------------------------------------------------------------------------------------------
// per-kernel profiler hook (wlx_debug_profile_step): when s->prof is set a launch of the decoder pass is either only
// listed (name as rocprofv3 prints it + its ALGORITHMIC bytes: weights / K,V it has to stream once) or filtered by name.
template <class F>
static inline void plaunch(Slot* s, const char* name, double bytes, F&& f) {
    if (!s->prof) { f(); return; }
    if (s->prof->list_only) { s->prof->recs.push_back(ProfRec{name, bytes}); return; }
    if (s->prof->only == name) f();
}
static double gemv_bytes(const GemvParams& p) { return 2.0 * (double)p.N * (double)p.K + (p.bias ? 4.0 * p.N : 0.0); }
// three or more live slots on the slot's device: the GPU is work-bound there and the decode projections pick work-saving
// launch shapes (GemvParams::busy_device). Evaluated when a step graph is captured / looked up: the variant is part of the graph key.
bool wlx::device_is_busy(const Slot* s) {
    return s->device_of >= 0 && s->device_of < 64 && g_slots_live[s->device_of].load(std::memory_order_relaxed) >= 3;
}
static void pgemv(Slot* s, const GemvParams& p0) {
    GemvParams p = p0;
    p.busy_device = s->busy_variant ? 1 : 0;
    if (!s->prof) { launch_dec_gemv(p, s->stream); return; }
    const std::string nm = dec_gemv_kernel_name(p);
    plaunch(s, nm.c_str(), gemv_bytes(p), [&] { launch_dec_gemv(p, s->stream); });
}

// final LayerNorm + vocabulary projection of `rows` residual rows at `x` into the slot's logits (plain rows, no done flag: the decoder
// pass adds its slab source and flag, probe_no_speech takes it as it is)
static GemvParams vocab_projection(const Engine* e, const Slot* s, const float* x, int rows) {
    const int d = e->spec.d_model;
    GemvParams p{};
    p.in_mode = GEMV_IN_LN; p.out_mode = GEMV_OUT_F32; p.M = rows; p.K = d; p.KT = d / 32; p.N = e->spec.vocab;
    p.Wp = e->Wvocab; p.bias = nullptr; p.X = x; p.ldx = d; p.gamma = e->dec_ln_g; p.beta = e->dec_ln_b;
    p.Y = s->logits; p.ldy = s->ldl; p.qscale = 1.f; p.xsrc = GEMV_X_PLAIN;
    return p;
}

// ------------------------------------------------------------------------------------------------
// decoder pass: embed -> L x {self-attn block, cross-attn block, MLP} -> (final LN + vocab projection)
// Row tables / ancestry must already be on the device. `rows` live rows in `groups` groups of R rows.
// `b` is the working set: the slot's `step` set (decode steps, chunked passes) or its prompt-prefill set `pf`; everything else
// (stream, KV caches, cross K/V, ancestry, profiler hook) is the slot's. `one_pass_prefill`: the pass is the one-pass prompt prefill.
void wlx::decoder_pass(Engine* e, Slot* s, const DecBufs& b, int rows, int R, int groups, bool with_logits, bool check_done, bool one_pass_prefill) {
    const wlx_spec& sp = e->spec;
    const int d = sp.d_model, F = sp.ffn, H = e->H;
    const long slab_stride = (long)b.slab_rows * d;
    hipStream_t st = s->stream;
    // The decoder pass only rewrites scratch and re-appends the same K/V at the same position when it runs once
    // more after the search has raised `done` (the host runs at most one step ahead), so the second-generation
    // kernels do not test the flag: the test was a dependent scalar load at the head of ~100 launches per step.
    const int* done = (check_done && g_decode_v1) ? s->st.done : nullptr;
    RowTables rt{b.d_token, b.d_pos, b.d_cache, b.d_ancrow, s->d_anc, s->d_intok};
    const long crs = (long)WLX_T_TEXT * d;
    // ---- the parameter sets of one layer (the first projection's residual source is filled in below)
    auto qkv_params = [&](int l, int xsrc) {
        const LayerW& w = e->dec[l];
        GemvParams p{};
        p.in_mode = GEMV_IN_LN; p.out_mode = GEMV_OUT_QKV; p.M = rows; p.K = d; p.KT = d / 32; p.N = 3 * d;
        p.Wp = w.Wqkv; p.bias = w.bqkv; p.X = b.xd; p.ldx = d; p.gamma = w.ln1_g; p.beta = w.ln1_b;
        p.Yh = b.qd; p.ldyh = d; p.d = d; p.qscale = 0.125f;
        p.Kc = s->kc + (size_t)l * s->cache_rows * crs; p.Vc = s->vc + (size_t)l * s->cache_rows * crs; p.cache_row_stride = crs;
        p.row_cache = b.d_cache; p.row_pos = b.d_pos; p.done = done;
        p.xsrc = xsrc; p.slab = b.slab; p.slab_stride = slab_stride;
        if (xsrc == GEMV_X_EMBED) {
            p.tok_emb = e->tok_emb16; p.pos_emb = e->dec_pos; p.emb_token = b.d_token; p.intok = s->d_intok;
            p.Xres = b.xd; p.ldxres = d;
        }
        return p;
    };
    auto oproj_params = [&](int l, int xsrc) {
        const LayerW& w = e->dec[l];
        GemvParams p{};
        p.in_mode = GEMV_IN_F16; p.out_mode = GEMV_OUT_RESID; p.M = rows; p.K = d; p.KT = d / 32; p.N = d;
        p.Wp = w.Wo; p.bias = w.bo; p.Xh = b.attnd; p.ldxh = d; p.Xres = b.xd; p.ldxres = d; p.qscale = 1.f; p.done = done;
        p.xsrc = xsrc; p.slab = b.slab; p.slab_stride = slab_stride;
        return p;
    };
    auto vocab_params = [&](int xsrc) {
        GemvParams p = vocab_projection(e, s, b.xd, rows);
        p.done = done; p.xsrc = xsrc; p.slab = b.slab; p.slab_stride = slab_stride;
        return p;
    };
    // ---- what this pass may use (decided once, from the shapes only — never from what a profiling filter lets through):
    // the K-split MLP output projection needs every consumer of its slabs on the lean kernel; the embedding folds into
    // layer 0's first projection under the same condition (re-measured in round 5 against the separate embedding launch: 27.80 vs 28.02 ms
    // per window, profiles/r5a_*).
    int KS = dec_gemv_slab_split(rows, F, d);
    if (rows > b.slab_rows) KS = 0;         // the partial-sum slabs of this working set hold slab_rows rows
    // batched decode steps (17..64 rows) keep the single MLP output launch (round 4, profiles/r4b_*): the split saves ~1 us
    // there but every consumer of the slabs then reads three fp32 copies of every row in its LayerNorm prologue — per 16-column
    // workgroup — and those launches are bound by load instructions per CU (60 rows, small.en: first projection 9.8 us with
    // slabs, 7.0 us without; large-v3 at 40 rows: 11.4 -> 8.7 us).
    if (rows > 16 && !b.prefill) KS = 0;
    // ... and the one-pass prompt prefill (round 6): its K-split MLP projection made every 16-column workgroup of the next layer's first projection
    // (144 x 14 workgroups at 224 rows) read THREE fp32 copies of its rows and lose the four-column-tile form: 21.8 us per launch against 11 us.
    // 224 tokens: 1.099 -> 0.955 ms (Whisper-small), 6.66 -> 5.31 ms (large-v3), profiles/r6g_prefill_time.txt. (The joint pass over a batch's
    // short prompts keeps its form: its rows must stay bit-identical to the single calls' chunked prefill.)
    if (one_pass_prefill) KS = 0;
    if (KS && !(dec_gemv_is_lean(qkv_params(0, GEMV_X_SLABS)) && dec_gemv_is_lean(oproj_params(0, GEMV_X_SLABS)))) KS = 0;
    // (batched steps, 17..64 rows: the folded form gathers ONE row per wave and trip — two trips per 16-row tile, the second behind the
    // weight stream — and has no four-tile instantiation: 13.6 us at 60 rows against 2.4 + 5.9 us for the embedding launch + the plain
    // four-tile projection, profiles/r4s_decode_step.txt.)
    // (prefill passes of more than 64 rows keep the embedding launch, as they always did: the folded form's K split over the waves — one
    // row per wave — differs from the plain LayerNorm projection's, i.e. another summation order for the prompt rows' layer-0 K / V)
    const bool fold_embed = (rows <= 16 || (b.prefill && rows <= 64)) && dec_gemv_is_lean(qkv_params(0, GEMV_X_EMBED));
    // (Measured and closed: ONE LayerNorm launch per layer phase + fp16-rows-in projections instead of the LayerNorm prologue in every
    // 16-column workgroup — for batched decode steps in round 4, for the prompt-prefill pass in round 5 (conditioned window 30.88 vs
    // 30.89 ms, profiles/r5a_*): no gain either way; the kernel left the library.)
    if (!fold_embed)
        plaunch(s, "dec_embed_kernel", (double)rows * d * (2 + 4), [&] { launch_dec_embed(e->tok_emb16, e->dec_pos, d, rt, rows, b.xd, done, st); });
    bool slabs_pending = false;             // the residual stream is xd + slabs until the next residual update writes the sum back
    for (int l = 0; l < sp.dec_layers; ++l) {
        const LayerW& w = e->dec[l];
        half_t* kc = s->kc + (size_t)l * s->cache_rows * crs;
        half_t* vc = s->vc + (size_t)l * s->cache_rows * crs;
        // LN1 + QKV, K/V appended to the self-attention cache
        {
            GemvParams pq = qkv_params(l, (l == 0 && fold_embed) ? GEMV_X_EMBED : (slabs_pending ? GEMV_X_SLABS : GEMV_X_PLAIN));
            pgemv(s, pq);
        }
        plaunch(s, "dec_self_attn2_kernel", 4.0 * rows * d * (s->prof ? s->prof->t + 1 : 1), [&] { launch_dec_self_attn(b.qd, d, kc, vc, crs, d, H, rt, rows, b.attnd, d, done, s->anc_ident, st); });
        pgemv(s, oproj_params(l, slabs_pending ? GEMV_X_SLABS : GEMV_X_PLAIN));
        slabs_pending = false;
        GemvParams p{};
        // LN2 + cross-attention query + cross-attention partials: one fused launch when the shape allows and nobody needs
        // the query rows (word alignment captures them), else projection and attention separately
        const half_t* ckl = s->ck + (size_t)l * s->B * WLX_T_AUDIO_PAD * d;
        const half_t* cvl = s->cvt + (size_t)l * s->B * d * WLX_T_AUDIO_PAD;
        // (not for the one-pass prompt prefill: with 14+ groups every (split, head, group) workgroup re-reads its head's 96 KiB of
        // query weights — 224 tokens: 1.49 ms fused, 1.32 ms as projection + attention, profiles/r3l_prefill_fused_cq.txt)
        const bool fused = !s->align && rows <= 48 && dec_cq_cross_attn_eligible(d, H, R);
        if (fused)
            plaunch(s, "dec_cq_cross_attn_kernel", 2.0 * d * d + 4.0 * groups * WLX_T_AUDIO * d, [&] {
                launch_dec_cq_cross_attn(b.xd, d, w.ln2_g, w.ln2_b, w.Wcq, w.bcq, 0.125f, d, ckl, cvl, (long)WLX_T_AUDIO_PAD * d, H, R,
                                         groups, rows, b.d_group_item, b.part_o, b.part_ml, st);
            });
        if (!fused) {
            p = GemvParams{};
            p.in_mode = GEMV_IN_LN; p.out_mode = GEMV_OUT_F16; p.M = rows; p.K = d; p.KT = d / 32; p.N = d;
            p.Wp = w.Wcq; p.bias = w.bcq; p.X = b.xd; p.ldx = d; p.gamma = w.ln2_g; p.beta = w.ln2_b;
            p.Yh = b.qd; p.ldyh = d; p.qscale = 0.125f; p.done = done;
            pgemv(s, p);
            if (s->align) {     // word alignment: raw q.k of this layer's alignment heads for the rows of this chunk
                const Slot::AlignCapture& a = *s->align;
                for (int hi = 0; hi < a.n_heads; ++hi)
                    if (a.heads[2 * hi] == l)
                        launch_dec_align_scores(b.qd, d, s->ck + ((size_t)l * s->B + a.item) * WLX_T_AUDIO_PAD * d, a.heads[2 * hi + 1], rows,
                                                a.scores + ((size_t)hi * a.n_tok + a.row0) * WLX_T_AUDIO_PAD, st);
            }
            plaunch(s, "dec_cross_attn_kernel", 4.0 * groups * WLX_T_AUDIO * d, [&] {
                launch_dec_cross_attn(b.qd, d, ckl, cvl, (long)WLX_T_AUDIO_PAD * d, H, R, groups, rows, b.d_group_item, b.part_o, b.part_ml, st);
            });
        }
        p = GemvParams{};
        p.in_mode = GEMV_IN_XATTN; p.out_mode = GEMV_OUT_RESID; p.M = rows; p.K = d; p.KT = d / 32; p.N = d;
        p.Wp = w.Wco; p.bias = w.bco; p.part_o = b.part_o; p.part_ml = b.part_ml; p.H = H; p.R = R;
        p.Xres = b.xd; p.ldxres = d; p.qscale = 1.f; p.done = done;
        if (rows > 16) {
            // batched rows: the split combine once, in its own launch, then a plain fp16-rows-in projection (decoder.hip)
            plaunch(s, "dec_xattn_combine_kernel", 0.0, [&] { launch_dec_xattn_combine(b.part_o, b.part_ml, rows, H, R, b.attnd, d, st); });
            p.in_mode = GEMV_IN_F16; p.Xh = b.attnd; p.ldxh = d;
        }
        pgemv(s, p);
        // LN3 + MLP
        p = GemvParams{};
        p.in_mode = GEMV_IN_LN; p.out_mode = GEMV_OUT_GELU_F16; p.M = rows; p.K = d; p.KT = d / 32; p.N = F;
        p.Wp = w.W1; p.bias = w.b1; p.X = b.xd; p.ldx = d; p.gamma = w.ln3_g; p.beta = w.ln3_b;
        p.Yh = b.hd; p.ldyh = F; p.qscale = 1.f; p.done = done;
        pgemv(s, p);
        p = GemvParams{};
        p.in_mode = GEMV_IN_F16; p.out_mode = GEMV_OUT_RESID; p.M = rows; p.K = F; p.KT = F / 32; p.N = d;
        p.Wp = w.W2; p.bias = w.b2; p.Xh = b.hd; p.ldxh = F; p.Xres = b.xd; p.ldxres = d; p.qscale = 1.f; p.done = done;
        // the last layer: its consumer is the vocabulary projection. While that was 1621 workgroups that would each have summed the slabs the
        // split was a loss there (+2.2 us against 1.2 us saved, profiles/r2f_*) and the last layer kept the single launch — 11-13 us at 5 rows,
        // the slowest projection of the step (profiles/r5b_*). dec_vocab_kernel (203 workgroups, one LayerNorm each) takes rows + slabs.
        const bool last_split = with_logits && dec_gemv_is_lean(vocab_params(GEMV_X_SLABS));
        if (KS && (l + 1 < sp.dec_layers || last_split)) {
            p.out_mode = GEMV_OUT_SLAB; p.KTS = p.KT / KS; p.slab = b.slab; p.slab_stride = slab_stride;
            slabs_pending = true;
        }
        pgemv(s, p);
    }
    if (with_logits) pgemv(s, vocab_params(slabs_pending ? GEMV_X_SLABS : GEMV_X_PLAIN));
}

// row tables of a pass, from a PINNED block laid out [token | pos | cache | ancrow : rows each | group_item : groups] into the working set
// `b`, on the slot stream. The block is the caller's (h_stage, h_gen or h_pf), and so is the rule for when it may be rewritten.
static int upload_row_tables(Slot* s, const DecBufs& b, const int* h, size_t rows, size_t groups) {
    CK(hipMemcpyAsync(b.d_token, h, rows * 4, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(b.d_pos, h + rows, rows * 4, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(b.d_cache, h + 2 * rows, rows * 4, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(b.d_ancrow, h + 3 * rows, rows * 4, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(b.d_group_item, h + 4 * rows, groups * 4, hipMemcpyHostToDevice, s->stream));
    return WLX_OK;
}

// upload row tables for a pass on the `step` working set through the shared staging: token/pos/cache/ancrow [rows], group_item [groups]
int wlx::upload_rows(Slot* s, const std::vector<int>& token, const std::vector<int>& pos,
                     const std::vector<int>& cache, const std::vector<int>& ancrow, const std::vector<int>& group_item) {
    const size_t rows = token.size(), ng = group_item.size();
    if (4 * rows + ng > s->h_stage_ints) return set_error(WLX_ERR_ARG, "row table too large");
    s->anc_ident = true;                                    // every row reads its history through its own ancestry row
    for (size_t i = 0; i < rows; ++i) s->anc_ident = s->anc_ident && ancrow[i] == (int)i;
    // the shared staging buffer may still be the source of an earlier pass's copies: wait (callers with a pinned area of their
    // own — wlx_generate's decode rows, the one-pass prefill — fill it and call upload_row_tables themselves)
    CK(hipStreamSynchronize(s->stream));
    int* h = s->h_stage;
    memcpy(h, token.data(), rows * 4); memcpy(h + rows, pos.data(), rows * 4);
    memcpy(h + 2 * rows, cache.data(), rows * 4); memcpy(h + 3 * rows, ancrow.data(), rows * 4);
    memcpy(h + 4 * rows, group_item.data(), ng * 4);
    return upload_row_tables(s, s->step, h, rows, ng);
}

// no_speech_prob after a prefill pass that ran WITHOUT the vocabulary projection (one-pass, joint): project the one residual row at
// <|startoftranscript|> (`x_row`) and read P(nsp_token) into *dst (the pinned result area of wlx_generate, or device memory)
static int probe_no_speech(Engine* e, Slot* s, const float* x_row, int nsp_token, float* dst) {
    launch_dec_gemv(vocab_projection(e, s, x_row, 1), s->stream);
    launch_token_prob(s->logits, s->ldl, e->spec.vocab, 1, nsp_token, s->d_tokprob, s->stream);
    CK(hipMemcpyAsync(dst, s->d_tokprob, 4, hipMemcpyDefault, s->stream));
    return WLX_OK;
}

// prefill `n` tokens of one sequence (audio item `item`, KV-cache row `crow`) starting at position pos0,
// in chunks of <= 48 rows (below); if logits_out != null the vocabulary projection runs and rows are copied out.
int wlx::prefill_tokens(Engine* e, Slot* s, int item, int crow, const int* tokens, int pos0, int n,
                        float* logits_host, int nsp_index, int nsp_token, float* nsp_out) {
    // ONE pass over the whole prompt (round 3): every window after the first carries up to 224 prompt tokens
    // (transcriber_faster_whisper.py:1480-1513) and the chunked form below costs a full ~87-launch decoder pass per 48 rows —
    // 4.6 ms for 224 tokens on Whisper-small, 18 ms on large-v3 (profiles/r3f_prefill_time.txt), 16-19 % of a window. Here
    // the pass runs ONCE over all rows: each projection is one launch of the lean kernel whose grid.z walks 48-row chunks
    // (the weight tiles are re-read from L2 by the chunks), attention and combine launches take the rows as they are.
    // Logits are only needed at the <|startoftranscript|> row (no_speech_prob); callers that want every row's logits
    // (debug hook) keep the chunked form.
    const bool one_pass = [] { const char* v = getenv("WLX_PREFILL_ONE_PASS"); return !(v && v[0] == '0'); }();   // (read per call: the A/B test toggles it)
    if (one_pass && s->pf_ok && !logits_host && !s->align && !s->prof && n > 48 && n <= WLX_T_TEXT && !g_decode_v1) {
        const int rows = n, groups = (rows + 15) / 16;
        // its own pinned staging (round 6): the shared one needed a wait for the stream first — "may still feed an earlier pass's copies" — which
        // let the GPU idle between the encoder's end and this pass while the host built and uploaded the tables. Only a SECOND one-pass prefill of
        // the same call (a batch of long prompts) has to wait: wlx_generate clears the flag, and a call returns after its own uploads were consumed.
        if (s->h_pf_used) CK(hipStreamSynchronize(s->stream));
        s->h_pf_used = true;
        int* h = s->h_pf;
        for (int i = 0; i < rows; ++i) { h[i] = tokens[i]; h[rows + i] = pos0 + i; h[2 * rows + i] = crow; h[3 * rows + i] = crow; }
        for (int g = 0; g < groups; ++g) h[4 * rows + g] = item;
        CKR(upload_row_tables(s, s->pf, h, rows, groups));
        s->anc_ident = false;                                       // every row reads its history through the prompt's cache row
        decoder_pass(e, s, s->pf, rows, 16, groups, false, false, /*one_pass_prefill=*/true);
        CK(hipGetLastError());
        if (nsp_index >= 0 && nsp_index < rows) {
            CKR(probe_no_speech(e, s, s->pf.xd + (size_t)nsp_index * e->spec.d_model, nsp_token, nsp_out));
            CK(hipGetLastError());
        }
        return WLX_OK;
    }
    // chunk size: 48 rows = three 16-row MFMA tiles = one launch of the lean projections per chunk (a 64-row chunk runs them as
    // two row chunks in grid.z); WLX_PREFILL_ROWS=16..320 (A/B, tests)
    // (read per call: tests toggle it; up to the slot's row capacity — 120 teacher-forced rows in one pass on a 24 x 5 slot)
    const int chunk = std::min(s->rows_cap, [] { const char* v = getenv("WLX_PREFILL_ROWS"); const int c = v ? atoi(v) : 48; return (c >= 16 && c <= WLX_MAX_DEC_ROWS) ? c : 48; }());
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int rows = std::min(chunk, n - c0);
        const int groups = (rows + 15) / 16;
        std::vector<int> tk(rows), ps(rows), ca(rows, crow), an(rows, crow), gi(groups, item);
        for (int i = 0; i < rows; ++i) { tk[i] = tokens[c0 + i]; ps[i] = pos0 + c0 + i; }
        CKR(upload_rows(s, tk, ps, ca, an, gi));
        const bool want_nsp = nsp_index >= c0 && nsp_index < c0 + rows;
        const bool lg = (logits_host != nullptr) || want_nsp;
        decoder_pass(e, s, s->step, rows, 16, groups, lg, false);
        CK(hipGetLastError());
        if (logits_host) {
            CK(hipMemcpy2DAsync(logits_host + (size_t)c0 * e->spec.vocab, (size_t)e->spec.vocab * 4, s->logits,
                                (size_t)s->ldl * 4, (size_t)e->spec.vocab * 4, rows, hipMemcpyDeviceToHost, s->stream));
        }
        if (want_nsp) {     // (the pass above already projected every row of the chunk: no projection launch of its own)
            launch_token_prob(s->logits + (size_t)(nsp_index - c0) * s->ldl, s->ldl, e->spec.vocab, 1, nsp_token, s->d_tokprob, s->stream);
            CK(hipMemcpyAsync(nsp_out, s->d_tokprob, 4, hipMemcpyDeviceToDevice, s->stream));
        }
    }
    return WLX_OK;
}

// identity ancestry for cache row `crow` over positions [0, upto)
int wlx::set_anc_rows(Slot* s, const std::vector<short>& anc_host, int first_row, int nrows) {
    CK(hipMemcpyAsync(s->d_anc + (size_t)first_row * WLX_T_TEXT, anc_host.data(), (size_t)nrows * WLX_T_TEXT * sizeof(short),
                      hipMemcpyHostToDevice, s->stream));
    CK(hipStreamSynchronize(s->stream));   // anc_host is caller stack memory
    return WLX_OK;
}

// token search of one step: beam mode runs the chunked scan + merge/update pair, sampling (T > 0 fallback)
// the one-workgroup-per-row kernels
void wlx::launch_search(Engine* e, Slot* s, int rows, int R, int groups, bool sampling) {
    if (sampling || g_decode_v1) {
        launch_search_rows(s->logits, s->d_sp, rows, s->st, s->stream);
        launch_search_update(s->d_sp, groups, s->st, s->stream);
    } else {
        launch_search_scan3(s->logits, s->ldl, e->spec.vocab, s->d_sp, rows, s->st, s->stream);
        launch_search_merge_update3(s->logits, s->ldl, e->spec.vocab, s->d_sp, groups, R, s->st, s->stream);
    }
}

// Steps per graph launch (round 6). The boundary between two step graphs is 8.6-8.9 us of idle GPU against 1.45 us between two kernels of one graph
// (profiles/r6ab_chunk_timeline_under_rocprof.txt): with TWO decode steps per graph every second boundary is an ordinary kernel boundary, -3.6 us per
// step. The price is how far a decode can run past its end: the host enqueues graph g + 1 when the LAST step of graph g has started (the update kernels
// mirror their step number to pinned memory), so an end of text in the first step of a graph leaves one scratch-only step behind it and one in the second
// step leaves two — 1.5 on average against 1 with one step per graph. The call itself returns at the done word either way (the results are in pinned
// memory); only work queued behind it on the same stream sees the extra 0.2 ms. So two steps are used where latency is what counts and the GPU has
// room — ONE live slot on the device, one stream's rows (<= 16) — and one step everywhere else (several clients' slots, batched rows).
static int graph_steps_for(const Slot* s, int rows) {
    if (rows > 16) return 1;
    const bool alone = s->device_of >= 0 && s->device_of < 64 && g_slots_live[s->device_of].load(std::memory_order_relaxed) <= 1;
    return alone ? 2 : 1;
}

// keyword boosting: with a table installed on the slot (wlx_bias_set) one launch between the vocabulary projection and the search adds the
// row's bias to its logits (dec_bias.hip); a slot without a table launches nothing here, so its step is the launch list it always was. In
// per-item mode (wlx_bias_set_items) the launch is dec_bias_items_kernel: the table selected for the row's item (wlx_bias_select). With a
// grammar (wlx_grammar_set) it is dec_grammar_kernel (dec_grammar.hip), which masks where the others add.
void wlx::launch_bias(Slot* s, int rows) {
    if (s->bias_mode == BIAS_ONE) launch_dec_bias(s->logits, s->d_sp, rows, s->st, s->bias, s->stream);
    else if (s->bias_mode == BIAS_ITEMS) launch_dec_bias_items(s->logits, s->d_sp, rows, s->st, s->bias_items, s->stream);
    else if (s->bias_mode == BIAS_GRAMMAR) launch_dec_grammar(s->logits, s->d_sp, rows, (int)s->ldl, s->st, s->grammar, s->stream);
}

static void launch_steps(Engine* e, Slot* s, int rows, int R, int groups, bool sampling, int nsteps) {
    for (int k = 0; k < nsteps; ++k) {
        decoder_pass(e, s, s->step, rows, R, groups, true, true);
        launch_bias(s, rows);
        launch_search(e, s, rows, R, groups, sampling);
    }
}

static int get_step_graph(Engine* e, Slot* s, int rows, int R, int groups, bool sampling, int nsteps, hipGraphExec_t* out) {
    s->busy_variant = device_is_busy(s);
    const StepGraphKey key{rows, R, groups, nsteps, s->busy_variant, sampling, s->bias_mode};
    auto it = s->graphs.find(key);
    if (it != s->graphs.end()) { *out = it->second; return WLX_OK; }
    hipGraph_t graph;
    // One eager pass first: the first launch of a kernel instantiation may have to raise its dynamic-LDS limit
    // (dec_gemv.hip g2_launch), which must not happen inside a capture. It only rewrites scratch and re-appends the K/V the
    // captured replay appends again (same rows, same positions); the search, which mutates state, is not run.
    decoder_pass(e, s, s->step, rows, R, groups, true, true);
    CK(hipGetLastError());
    CK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    launch_steps(e, s, rows, R, groups, sampling, nsteps);
    const hipError_t ce = hipStreamEndCapture(s->stream, &graph);
    if (ce != hipSuccess) {
        // An invalidated capture leaves the stream refusing every later operation ("previous error during capture"), so
        // one bad capture would end the client's session for good. Replace the stream: this call fails (the session logs
        // it and moves on to the next chunk, whisper_live/backend/base.py:134-137), the next one captures afresh.
        (void)hipGetLastError();
        hipStream_t ns = nullptr;
        bool ded = false;
        if (s->dedicated_queue) { g_dedicated_live[e->device].fetch_sub(1); s->dedicated_queue = false; }
        if (create_slot_stream(e->device, &ns, &ded) == WLX_OK) {
            s->dedicated_queue = ded;
            (void)hipStreamDestroy(s->stream);
            s->stream = ns;
        }
        return set_error(WLX_ERR_HIP, "decode-step graph capture failed: %s (slot stream replaced)", hipGetErrorString(ce));
    }
    hipGraphExec_t exec;
    CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    CK(hipGraphDestroy(graph));
    s->graphs[key] = exec;
    *out = exec;
    return WLX_OK;
}

// `nsteps` decode steps (1 or 2): one graph launch, or the same launches eagerly
static int run_step(Engine* e, Slot* s, int rows, int R, int groups, bool sampling, int nsteps = 1) {
    if (e->use_graph) {
        hipGraphExec_t exec;
        CKR(get_step_graph(e, s, rows, R, groups, sampling, nsteps, &exec));
        CK(hipGraphLaunch(exec, s->stream));
    } else {
        s->busy_variant = device_is_busy(s);
        launch_steps(e, s, rows, R, groups, sampling, nsteps);
        CK(hipGetLastError());
    }
    return WLX_OK;
}

static int fill_search_params(Engine* e, Slot* s, int batch, int R, const wlx_gen_opts* o, bool apply_ts, SearchParams* sp) {
    memset(sp, 0, sizeof(*sp));
    sp->V = e->spec.vocab; sp->ldl = s->ldl; sp->items = batch; sp->R = R; sp->rows = batch * R;
    sp->sampling = (o->sampling_temperature > 0.f || o->beam_size <= 1) ? 1 : 0;
    sp->beam = sp->sampling ? 1 : o->beam_size;
    sp->ncand = sp->sampling ? 1 : 2 * o->beam_size;
    sp->max_cand_hyp = std::max(1, (int)std::lround((double)o->beam_size * (double)o->patience));
    sp->num_hyp = std::max(1, o->num_hypotheses);
    sp->allow_early_exit = (o->length_penalty == 0.f) ? 1 : 0;
    sp->length_penalty = o->length_penalty; sp->rep_penalty = (o->repetition_penalty > 0.f) ? o->repetition_penalty : 1.f;
    sp->temperature = o->sampling_temperature; sp->no_repeat_ngram = o->no_repeat_ngram_size;
    sp->topk = (o->sampling_temperature > 0.f) ? o->sampling_topk : 1;
    sp->suppress_blank = o->suppress_blank; sp->apply_ts_rules = apply_ts ? 1 : 0;
    sp->max_initial_ts = o->max_initial_timestamp_index;
    sp->sot = o->ids.sot; sp->eot = o->ids.eot; sp->no_timestamps = o->ids.no_timestamps; sp->ts_begin = o->ids.timestamp_begin;
    sp->no_speech = o->ids.no_speech; sp->blank = o->ids.blank;
    sp->max_length = o->max_length; sp->seed = o->seed; sp->suppress_mask = s->d_suppress;
    return WLX_OK;
}

static int validate_opts(Engine* e, Slot* s, int batch, const wlx_gen_opts* o) {
    if (!o) return set_error(WLX_ERR_ARG, "null opts");
    const int V = e->spec.vocab;
    auto bad = [&](int id) { return id < 0 || id >= V; };
    if (bad(o->ids.sot) || bad(o->ids.eot) || bad(o->ids.no_timestamps) || bad(o->ids.timestamp_begin) || bad(o->ids.no_speech))
        return set_error(WLX_ERR_ARG, "token ids out of vocabulary");
    if (o->max_length < 2 || o->max_length > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "max_length must be 2..448");
    const bool sampling = (o->sampling_temperature > 0.f || o->beam_size <= 1);
    const int R = sampling ? std::max(1, o->num_hypotheses) : o->beam_size;
    if (R < 1 || R > s->R) return set_error(WLX_ERR_ARG, "beam_size/num_hypotheses %d exceeds slot rows per item %d", R, s->R);
    if (!sampling && o->num_hypotheses > o->beam_size) return set_error(WLX_ERR_ARG, "num_hypotheses > beam_size");
    if (!sampling && 2 * o->beam_size > WLX_MAX_CAND) return set_error(WLX_ERR_ARG, "beam_size too large");
    if (!sampling && std::lround((double)o->beam_size * (double)o->patience) > WLX_MAX_HYP_ASK)
        return set_error(WLX_ERR_ARG, "beam_size * patience asks for %ld finished hypotheses, the limit is %d", std::lround((double)o->beam_size * (double)o->patience), WLX_MAX_HYP_ASK);
    if (batch * R > s->rows_cap) return set_error(WLX_ERR_ARG, "too many decoder rows");
    if (o->n_suppress_tokens < 0 || (o->n_suppress_tokens > 0 && !o->suppress_tokens)) return set_error(WLX_ERR_ARG, "bad suppress_tokens");
    return WLX_OK;
}

static int upload_suppress(Engine* e, Slot* s, const wlx_gen_opts* o) {
    const int V = e->spec.vocab, words = (V + 31) / 32;
    // a session passes the same list on every call: the mask on the device is then already the right one
    if (s->suppress_valid && (int)s->last_suppress.size() == o->n_suppress_tokens &&
        (o->n_suppress_tokens == 0 || memcmp(s->last_suppress.data(), o->suppress_tokens, (size_t)o->n_suppress_tokens * 4) == 0))
        return WLX_OK;
    s->suppress_valid = false;
    std::vector<unsigned> mask(words, 0u);
    for (int i = 0; i < o->n_suppress_tokens; ++i) {
        const int id = o->suppress_tokens[i];
        if (id >= 0 && id < V) mask[id >> 5] |= 1u << (id & 31);
    }
    CK(hipMemcpyAsync(s->d_suppress, mask.data(), words * 4, hipMemcpyHostToDevice, s->stream));
    CK(hipStreamSynchronize(s->stream));
    s->last_suppress.assign(o->suppress_tokens, o->suppress_tokens + o->n_suppress_tokens);
    s->suppress_valid = true;
    return WLX_OK;
}

GenStaging wlx::gen_staging(unsigned char* base, int rows_cap, int B) {
    static_assert(sizeof(SearchParams) <= 4096, "SearchParams staging");
    size_t off = 0;
    auto take = [&](size_t bytes) { unsigned char* p = base ? base + off : nullptr; off += bytes; return p; };
    GenStaging g{};
    g.sp = reinterpret_cast<SearchParams*>(take(4096));
    g.cum = reinterpret_cast<float*>(take((size_t)rows_cap * 4));
    g.rule = reinterpret_cast<int*>(take((size_t)rows_cap * 16));
    g.nsp = reinterpret_cast<int*>(take((size_t)rows_cap * 4));
    g.plen = reinterpret_cast<int*>(take((size_t)B * 4));
    g.anc = reinterpret_cast<short*>(take((size_t)rows_cap * WLX_T_TEXT * 2 + 192));
    g.rows = reinterpret_cast<int*>(take(((size_t)rows_cap * 4 + B) * 4 + 64));
    g.bytes = (off + 63) / 64 * 64;
    return g;
}

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- per-call state: everything the host prepares goes through the slot's pinned staging (h_gen) — asynchronous
// copies with no synchronisation in between (pageable sources made every one of them a blocking, bounce-buffered copy)
// — and the zeroing is one launch. The staging is only rewritten by the next call, after this one's final wait.
static int gen_upload_state(Engine* e, Slot* s, const wlx_gen_opts* o, int batch, int R, bool sampling, bool apply_ts, const int32_t* plens, const GenStaging& g) {
    const int rows = batch * R;
    SearchState& S = s->st;
    hipStream_t st = s->stream;
    CKR(fill_search_params(e, s, batch, R, o, apply_ts, g.sp));
    CK(hipMemcpyAsync(s->d_sp, g.sp, sizeof(SearchParams), hipMemcpyHostToDevice, st));
    launch_search_reset(S, batch, rows, st);
    memset(g.anc, 0, (size_t)rows * WLX_T_TEXT * 2);
    memset(g.nsp, 0, (size_t)rows * 4);                            // (set by gen_prefill, uploaded with the decode rows)
    for (int b = 0; b < batch; ++b) {
        const int pl = plens[b];
        g.plen[b] = pl;
        for (int r = 0; r < R; ++r) {
            const int row = b * R + r;
            g.cum[row] = (sampling || r == 0) ? 0.f : -INFINITY;
            short* a = g.anc + (size_t)row * WLX_T_TEXT;
            for (int p = 0; p < pl - 1; ++p) a[p] = (short)(b * R);   // prompt K/V live in the item's first cache row
            a[pl - 1] = (short)row;
            // rule state before the first generated token: no last token, "one before last" counts as a timestamp, no timestamp yet
            g.rule[4 * row] = 0; g.rule[4 * row + 1] = 1; g.rule[4 * row + 2] = -1; g.rule[4 * row + 3] = 0;
        }
    }
    CK(hipMemcpyAsync(S.cum, g.cum, rows * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(S.rule, g.rule, (size_t)rows * 16, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(S.plen, g.plen, batch * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_anc, g.anc, (size_t)rows * WLX_T_TEXT * sizeof(short), hipMemcpyHostToDevice, st));
    return WLX_OK;
}

// ---- prefill prompt[0 .. plen-2]; no_speech_prob is read at the sot position. `nsp_rows` [rows]: the rows whose FIRST decode step
// reads it instead (sot is the prompt's last token). The route is chosen here: joint over the batch, else per item one-pass or
// chunked (prefill_tokens).
static int gen_prefill(Engine* e, Slot* s, const wlx_gen_opts* o, int batch, int R, bool sampling, const int32_t* prompts, const int32_t* plens, int pstride,
                       const int32_t* enc_items, int* nsp_rows) {
    std::vector<int> sot_at(batch, -1);
    int longest = 0, with_prompt = 0;
    for (int b = 0; b < batch; ++b) {
        const int32_t* pr = prompts + (size_t)b * pstride;
        const int pl = plens[b];
        for (int i = 0; i < pl; ++i) if (pr[i] == o->ids.sot) sot_at[b] = i;
        if (sot_at[b] == pl - 1) { for (int r = 0; r < (sampling ? R : 1); ++r) nsp_rows[b * R + r] = (r == 0) ? 1 : 0; }
        longest = std::max(longest, pl - 1);
        with_prompt += pl > 1 ? 1 : 0;
    }
    if (!(batch > 1 && with_prompt > 1 && longest <= 16 && s->pf_ok && !s->align && !s->prof && !g_decode_v1)) {
        for (int b = 0; b < batch; ++b) {
            const int pl = plens[b];
            if (pl > 1)
                CKR(prefill_tokens(e, s, (enc_items ? enc_items[b] : b), b * R, prompts + (size_t)b * pstride, 0, pl - 1, nullptr, (sot_at[b] >= 0 && sot_at[b] < pl - 1) ? sot_at[b] : -1,
                                   o->ids.no_speech, s->st.no_speech + b));
        }
        return WLX_OK;
    }
    // Batched calls with short prompts (the multilingual start sequence `[sot, lang, task]` (+ prefix) of every item of a
    // batch_inference batch): ALL items' prompt rows in ONE decoder pass — item b is row group b (16 rows, the unused ones
    // repeat the item's last prompt row: the same K / V written to the same cache position again) — instead of one full
    // pass per item, each of which streams every decoder weight (large-v3: 1.3 ms per item, 8 items per batch).
    // (the prefill working set holds WLX_T_TEXT rows = 28 items of 16 rows: a wider batch, round 5, goes in blocks of 28 items)
    const int IB = WLX_T_TEXT / 16;
    for (int b0 = 0; b0 < batch; b0 += IB) {
        const int nb = std::min(IB, batch - b0), prow = 16 * nb;
        if ((size_t)(4 * prow + nb) > s->h_stage_ints - 8) return set_error(WLX_ERR_ARG, "batch too large");
        CK(hipStreamSynchronize(s->stream));                 // the shared staging may still feed an earlier pass's copies
        int* h = s->h_stage;
        for (int bi = 0; bi < nb; ++bi) {
            const int b = b0 + bi;
            const int32_t* pr = prompts + (size_t)b * pstride;
            const int np_ = plens[b] - 1;                     // prompt rows of this item (0: a lone start token — the group idles on row 0's token at position 0... of a valid cache row)
            for (int i = 0; i < 16; ++i) {
                const int j = np_ > 0 ? std::min(i, np_ - 1) : 0;
                h[bi * 16 + i] = pr[j]; h[prow + bi * 16 + i] = j; h[2 * prow + bi * 16 + i] = b * R; h[3 * prow + bi * 16 + i] = b * R;
            }
            h[4 * prow + bi] = (enc_items ? enc_items[b] : b);
        }
        CKR(upload_row_tables(s, s->pf, h, prow, nb));
        s->anc_ident = false;
        decoder_pass(e, s, s->pf, prow, 16, nb, false, false);
        CK(hipGetLastError());
        for (int bi = 0; bi < nb; ++bi) {
            const int b = b0 + bi;
            if (!(sot_at[b] >= 0 && sot_at[b] < plens[b] - 1)) continue;
            CKR(probe_no_speech(e, s, s->pf.xd + (size_t)(bi * 16 + sot_at[b]) * e->spec.d_model, o->ids.no_speech, s->st.no_speech + b));      // (into the pinned result area)
        }
        CK(hipGetLastError());
    }
    return WLX_OK;
}

// ---- autoregressive loop: one graph replay per step. The host never lets the stream run dry: step k+1 is
// enqueued BEFORE the host knows how step k ended (the update kernels raise a pinned done word and mirror their step
// number themselves: no copies, no events), so the check costs no GPU idle time; once the word is set the one extra
// step already in flight only rewrites scratch (its search kernels return at once) and nobody waits for it: the
// results are read from pinned memory (generate_impl).
static int gen_loop(Engine* e, Slot* s, int batch, int R, bool sampling, int max_steps, const float* inj, int inj_steps, volatile int* h_done,
                    double* tg, int& steps_run) {
    const int rows = batch * R, V = e->spec.vocab;
    const bool injected_logits = inj != nullptr;
    hipStream_t st = s->stream;
    bool finished = false;
    const int gsteps = (injected_logits || !e->use_graph) ? 1 : graph_steps_for(s, rows);
    for (int step = 0; step < max_steps && !finished;) {
        int n_this = 1;
        if (injected_logits) {
            if (step >= inj_steps) break;
            // test hook: logits come from the caller; the embed kernel still records the fed tokens
            const DecBufs& sb = s->step;
            RowTables rt{sb.d_token, sb.d_pos, sb.d_cache, sb.d_ancrow, s->d_anc, s->d_intok};
            launch_dec_embed(e->tok_emb16, e->dec_pos, e->spec.d_model, rt, rows, sb.xd, nullptr, st);
            CK(hipMemcpy2DAsync(s->logits, (size_t)s->ldl * 4, inj + (size_t)step * rows * V, (size_t)V * 4, (size_t)V * 4, rows,
                                hipMemcpyHostToDevice, st));
            launch_bias(s, rows);
            launch_search(e, s, rows, R, batch, sampling);
            CK(hipGetLastError());
        } else {
            const double ta = tg ? now_us() : 0.0;
            n_this = std::min(gsteps, max_steps - step);            // (an odd step budget ends on a one-step graph)
            CKR(run_step(e, s, rows, R, batch, sampling, n_this));
            if (tg) tg[0] += now_us() - ta;
        }
        steps_run += n_this;
        step += n_this;                                             // = steps enqueued so far
        // The search kernel of the step that finishes the last item stores 1 to the pinned word h_done itself, and every update kernel
        // stores its step number to the pinned word next to it as it ends (search.hip step_mirror): the host reads how far the stream got
        // from that word. Step k+1 is enqueued BEFORE the host waits for step k-1 to have ended, so the stream never runs dry; at most two
        // steps run past the finish (scratch-only, see decoder_pass). Round 5: this replaced a hipEventRecord after every step graph +
        // hipEventSynchronize one step behind, which cost 0.31 ms per 64-step window (profiles/r5p_*: 27.59 vs 27.28 ms with no
        // synchronisation at all; polling every 2nd / 4th step had been measured in round 2 and rejected — a skipped poll lets a whole
        // step run past a real end of text).
        if (injected_logits) {
            CK(hipStreamSynchronize(st));
            finished = h_done[0] != 0;
        } else if (step >= 2) {
            const double ta = tg ? now_us() : 0.0;
            int spins = 0, rounds = 0;
            // wait until all but the LAST enqueued step have ended, i.e. the last one has started: the next launch then lands while it runs
            while (h_done[1] < step - 1 && h_done[0] == 0) {  // update kernel number `step - 1` (1-based) has not ended yet
                // a short pure spin (the word usually moves within one step, 0.1-0.4 ms for one stream), then the core is offered to
                // other runnable threads between polls (every decoding thread — batch lanes, client threads — used to burn a
                // core for the whole generate). No sleep: a timer sleep (>= 50 us of slack) could let a 113 us tiny.en step's stream run dry.
                if (rounds == 0 && spins < 4096) cpu_relax(); else sched_yield();
                if (++spins >= (1 << 16)) {                    // every few ms: is the stream still alive? (a fault must not hang the caller)
                    spins = 0; ++rounds;
                    const hipError_t q = hipStreamQuery(st);
                    if (q == hipSuccess) break;                // drained: the counter is final
                    if (q != hipErrorNotReady) return set_error(WLX_ERR_HIP, "decode loop: %s", hipGetErrorString(q));
                }
            }
            if (tg) tg[1] += now_us() - ta;
            finished = h_done[0] != 0;
        }
    }
    return WLX_OK;
}

// ---- results, from the pinned area the update kernels wrote (Slot::h_hyp): per item the best NH hypotheses by score
static void gen_read_results(const SearchState& S, int batch, int NH, int32_t* tokens_out, int tstride, int32_t* n_tokens_out, float* scores_out, float* nsp_out) {
    const int* n_hyp = S.n_hyp_host;
    const int* hyp_len = S.hyp_len;
    const float* hyp_score = S.hyp_score;
    for (int b = 0; b < batch; ++b) {
        std::vector<int> order(std::min(n_hyp[b], WLX_MAX_HYP));
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int c2) {
            return hyp_score[(size_t)b * WLX_MAX_HYP + a] > hyp_score[(size_t)b * WLX_MAX_HYP + c2];
        });
        for (int h = 0; h < NH; ++h) {
            int32_t* dst = tokens_out + ((size_t)b * NH + h) * tstride;
            if (h < (int)order.size()) {
                const int src = order[h];
                int len = hyp_len[(size_t)b * WLX_MAX_HYP + src];
                if (len > tstride) len = tstride;
                memcpy(dst, &S.hyp_tokens[((size_t)b * WLX_MAX_HYP + src) * WLX_T_TEXT], (size_t)len * 4);
                n_tokens_out[b * NH + h] = len;
                scores_out[b * NH + h] = hyp_score[(size_t)b * WLX_MAX_HYP + src];
            } else {
                n_tokens_out[b * NH + h] = 0;
                scores_out[b * NH + h] = -INFINITY;
            }
        }
        if (nsp_out) nsp_out[b] = S.no_speech[b];
    }
}

int wlx::generate_impl(Engine* e, Slot* s, int batch, const int32_t* prompts, const int32_t* plens, int pstride,
                       const int32_t* enc_items, const wlx_gen_opts* o, bool injected_logits, const float* inj, int inj_steps,
                       int32_t* tokens_out, int tstride, int32_t* n_tokens_out, float* scores_out, float* nsp_out) {
    CKR(validate_opts(e, s, batch, o));
    if (s->bias_mode == BIAS_ITEMS && batch > s->sel_n)
        return set_error(WLX_ERR_STATE, "generate: %d items, but the bias selection covers %d (wlx_bias_select)", batch, s->sel_n);
    if (s->bias_mode == BIAS_GRAMMAR && o->ids.eot != s->grammar_eot)
        return set_error(WLX_ERR_ARG, "generate: end-of-text is %d, the slot's grammar was compiled for %d (wlx_grammar_set)", o->ids.eot, s->grammar_eot);
    static const bool gen_trace = getenv("WLX_GEN_TRACE") != nullptr;
    double tg[2] = {0.0, 0.0};                                  // WLX_GEN_TRACE: host time in graph launch calls / in the polling waits
    const double tg0 = now_us();
    s->h_pf_used = false;
    const bool sampling = (o->sampling_temperature > 0.f || o->beam_size <= 1);
    const int R = sampling ? std::max(1, o->num_hypotheses) : o->beam_size;
    const int rows = batch * R, V = e->spec.vocab;
    hipStream_t st = s->stream;
    // ---- argument scan: prompt lengths and tokens, the step budget, whether the timestamp rules apply
    int max_steps = 0;
    bool apply_ts = true;
    for (int b = 0; b < batch; ++b) {
        const int pl = plens[b];
        if (pl < 1 || pl >= o->max_length) return set_error(WLX_ERR_ARG, "item %d: prompt length %d vs max_length %d", b, pl, o->max_length);
        const int32_t* pr = prompts + (size_t)b * pstride;
        for (int i = 0; i < pl; ++i) {
            if (pr[i] < 0 || pr[i] >= V) return set_error(WLX_ERR_ARG, "prompt token out of vocabulary");
            if (pr[i] == o->ids.no_timestamps) apply_ts = false;   // CT2: timestamp rules only without <|notimestamps|>
        }
        max_steps = std::max(max_steps, o->max_length - pl);
    }
    CK(hipEventRecord(s->ev0, st));
    CKR(upload_suppress(e, s, o));
    const GenStaging g = gen_staging(s->h_gen, s->rows_cap, s->B);
    CKR(gen_upload_state(e, s, o, batch, R, sampling, apply_ts, plens, g));
    if (!injected_logits) CKR(gen_prefill(e, s, o, batch, R, sampling, prompts, plens, pstride, enc_items, g.nsp));
    // ---- decode rows: every row starts on its item's last prompt token, in its own cache row. The tables are built in the call's own
    // pinned staging (h_gen: written once per call), so no wait for the stream before the loop
    for (int b = 0; b < batch; ++b) {
        const int pl = plens[b], tok = prompts[(size_t)b * pstride + pl - 1];
        for (int row = b * R; row < (b + 1) * R; ++row) { g.rows[row] = tok; g.rows[rows + row] = pl - 1; g.rows[2 * rows + row] = row; g.rows[3 * rows + row] = row; }
        g.rows[4 * rows + b] = enc_items ? enc_items[b] : b;
    }
    s->anc_ident = true;                                    // every row reads its history through its own ancestry row
    CKR(upload_row_tables(s, s->step, g.rows, rows, batch));
    CK(hipMemcpyAsync(s->st.nsp_row, g.nsp, rows * 4, hipMemcpyHostToDevice, st));
    volatile int* h_done = s->h_stage + (s->h_stage_ints - 4);
    h_done[0] = 0;
    h_done[1] = 0;                                              // the update kernels' step number (search.hip step_mirror)
    const double tg1 = now_us();
    int steps_run = 0;
    CKR(gen_loop(e, s, batch, R, sampling, max_steps, injected_logits ? inj : nullptr, inj_steps, h_done, gen_trace ? tg : nullptr, steps_run));
    const double tg2 = now_us();
    if (gen_trace) CK(hipStreamSynchronize(st));             // (only to tell the drain from the readback in the trace line)
    const double tg3 = now_us();
    // ---- results. Round 6: the update kernels store them in pinned host memory (Slot::h_hyp) and order them before the done word (search.hip
    // finish_item), so a call that saw the word reads them NOW — the step it had already enqueued behind the finish (scratch-only, ~0.4 ms) is still
    // running and is not waited for; the next call on the slot queues behind it on the stream. (Until then six copies were enqueued on the slot stream and
    // one wait covered the tail, the copies and the timing event.) A loop that ended any other way (injected logits, a step budget) waits for the stream.
    CK(hipEventRecord(s->ev1, st));
    s->gen_pending = true;
    if (h_done[0] == 0 || gen_trace) CK(hipStreamSynchronize(st));
    std::atomic_thread_fence(std::memory_order_acquire);
    gen_read_results(s->st, batch, std::max(1, o->num_hypotheses), tokens_out, tstride, n_tokens_out, scores_out, nsp_out);
    if (gen_trace) {
        float gms = 0.f;
        CK(hipEventElapsedTime(&gms, s->ev0, s->ev1));
        fprintf(stderr, "[wlx gen] steps %d: setup %.0f us | loop %.0f us (graph launch calls %.0f, event waits %.0f) | drain %.0f us | readback %.0f us | device %.0f us\n",
                steps_run, tg1 - tg0, tg2 - tg1, tg[0], tg[1], tg3 - tg2, now_us() - tg3, 1e3 * gms);
    }
    return WLX_OK;
}

extern "C" int32_t wlx_generate_ex(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* enc_items,
                                   const int32_t* prompts, const int32_t* prompt_lens, int32_t prompt_stride,
                                   const wlx_gen_opts* opts, int32_t* tokens_out, int32_t tokens_stride,
                                   int32_t* n_tokens_out, float* scores_out, float* no_speech_prob_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!prompts || !prompt_lens || !tokens_out || !n_tokens_out || !scores_out) return set_error(WLX_ERR_ARG, "null argument");
    if (batch < 1 || batch > s->B) return set_error(WLX_ERR_ARG, "batch %d out of range (slot max %d)", batch, s->B);
    if (s->enc_batch < 1) return set_error(WLX_ERR_STATE, "generate before encode");
    for (int b = 0; b < batch; ++b) {
        const int it = enc_items ? enc_items[b] : b;
        if (it < 0 || it >= s->enc_batch)
            return set_error(WLX_ERR_STATE, "generate: item %d uses encoder item %d but only %d are encoded", b, it, s->enc_batch);
    }
    CK(hipSetDevice(e->device));
    return generate_impl(e, s, batch, prompts, prompt_lens, prompt_stride, enc_items, opts, false, nullptr, 0, tokens_out,
                         tokens_stride, n_tokens_out, scores_out, no_speech_prob_out);
}

extern "C" int32_t wlx_generate(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* prompts,
                                const int32_t* prompt_lens, int32_t prompt_stride, const wlx_gen_opts* opts,
                                int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out, float* scores_out,
                                float* no_speech_prob_out) {
    return wlx_generate_ex(e, slot, batch, nullptr, prompts, prompt_lens, prompt_stride, opts, tokens_out, tokens_stride,
                           n_tokens_out, scores_out, no_speech_prob_out);
}

// ---- keyword boosting: the slot's bias table (include/wlx.h; dec_bias.hip). The device block, the state table and the pinned staging are
// allocated at the first call and stay where they are, so a step graph captured with a table replays with every later one.
static int bias_state_alloc(Slot* s) {           // the per-(cache row, position) states, shared by the single-table and the per-item mode
    if (s->bias_state) return WLX_OK;
    short* state = nullptr;
    CKR(dalloc(s->allocs, &state, (size_t)std::max(s->cache_rows, s->rows_cap) * WLX_T_TEXT, true));
    s->bias_state = state;
    return WLX_OK;
}

extern "C" int32_t wlx_bias_set(wlx_engine* e, int32_t slot, int32_t n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                                const int32_t* edge_next, float boost, int32_t n_tok, const int32_t* tok_ids, const float* tok_vals) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    // a refused table leaves the installed one whole (and allocates nothing): checked into a host copy first
    std::vector<int> block((size_t)WLX_BIAS_TABLE_INTS, 0);
    CKR(bias_table_fill(block.data(), e->spec.vocab, n_nodes, edge_off, edge_tok, edge_next, boost, n_tok, tok_ids, tok_vals));
    CK(hipSetDevice(e->device));
    CKR(bias_state_alloc(s));
    if (!s->d_bias) {
        int *blk = nullptr, *stage = nullptr;
        CKR(dalloc(s->allocs, &blk, (size_t)WLX_BIAS_TABLE_INTS, true));
        CKR(halloc(s->host_allocs, &stage, (size_t)WLX_BIAS_TABLE_INTS));
        memset(stage, 0, sizeof(int) * WLX_BIAS_TABLE_INTS);
        s->d_bias = blk; s->h_bias = stage; s->bias = bias_table_at(blk, s->bias_state);
    }
    // the staging may still feed the copy of the previous table: wait for the stream, then rewrite it
    CK(hipStreamSynchronize(s->stream));
    memcpy(s->h_bias, block.data(), sizeof(int) * WLX_BIAS_TABLE_INTS);
    CK(hipMemcpyAsync(s->d_bias, s->h_bias, sizeof(int) * WLX_BIAS_TABLE_INTS, hipMemcpyHostToDevice, s->stream));
    s->bias_mode = BIAS_ONE;
    return WLX_OK;
}

extern "C" int32_t wlx_bias_clear(wlx_engine* e, int32_t slot) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    sg_.s->bias_mode = BIAS_NONE;
    return WLX_OK;
}

// ---- per-item tables (include/wlx_bias_items.h; dec_bias.hip dec_bias_items_kernel). The pool, the selection and their pinned stagings are allocated at
// the first call and stay where they are: a step graph captured in per-item mode replays with every later set and selection.
static int bias_select_upload(Slot* s, int n, const int32_t* table_of_item) {
    // the pinned side may still feed the previous selection's copy: wait for THAT copy, not for the whole stream
    if (s->sel_pending) { CK(hipEventSynchronize(s->ev_sel)); s->sel_pending = false; }
    for (int b = 0; b < s->B; ++b) s->h_sel[b] = (table_of_item && b < n) ? table_of_item[b] : -1;
    CK(hipMemcpyAsync(s->d_sel, s->h_sel, sizeof(int) * (size_t)s->B, hipMemcpyHostToDevice, s->stream));
    CK(hipEventRecord(s->ev_sel, s->stream));
    s->sel_pending = true;
    s->sel_n = n;
    return WLX_OK;
}

extern "C" int32_t wlx_bias_set_items(wlx_engine* e, int32_t slot, int32_t n_tables, const int32_t* n_nodes, const int32_t* edge_off,
                                      const int32_t* edge_tok, const int32_t* edge_next, const float* boosts, const int32_t* n_tok,
                                      const int32_t* tok_ids, const float* tok_vals) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    // a refused set leaves whatever is installed whole (and allocates nothing): checked into a host copy first
    std::vector<int> pool;
    CKR(bias_items_fill(pool, e->spec.vocab, n_tables, n_nodes, edge_off, edge_tok, edge_next, boosts, n_tok, tok_ids, tok_vals));
    CK(hipSetDevice(e->device));
    CKR(bias_state_alloc(s));
    if (!s->d_pool) {
        int *dp = nullptr, *hp = nullptr, *ds = nullptr, *hs = nullptr;
        CKR(dalloc(s->allocs, &dp, (size_t)WLX_BIAS_POOL_INTS, true));
        CKR(dalloc(s->allocs, &ds, (size_t)s->B, true));
        CKR(halloc(s->host_allocs, &hp, (size_t)WLX_BIAS_POOL_INTS));
        CKR(halloc(s->host_allocs, &hs, (size_t)s->B));
        CK(hipEventCreateWithFlags(&s->ev_sel, hipEventDisableTiming));
        s->d_pool = dp; s->h_pool = hp; s->d_sel = ds; s->h_sel = hs;
        s->bias_items = BiasItems{dp, ds, s->bias_state};
    }
    CK(hipStreamSynchronize(s->stream));         // the pool's staging may still feed the copy of the previous set
    memcpy(s->h_pool, pool.data(), sizeof(int) * pool.size());
    CK(hipMemcpyAsync(s->d_pool, s->h_pool, sizeof(int) * pool.size(), hipMemcpyHostToDevice, s->stream));   // (the used part only)
    s->bias_tables = n_tables;
    CKR(bias_select_upload(s, s->B, nullptr));   // every item deselected: a table index of an earlier set never reaches this one
    s->bias_mode = BIAS_ITEMS;
    return WLX_OK;
}

extern "C" int32_t wlx_bias_select(wlx_engine* e, int32_t slot, int32_t n, const int32_t* table_of_item) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (s->bias_mode != BIAS_ITEMS) return set_error(WLX_ERR_STATE, "bias select: no table set installed (wlx_bias_set_items)");
    if (!table_of_item) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > s->B) return set_error(WLX_ERR_ARG, "bias select: %d items outside 1..%d", n, s->B);
    for (int b = 0; b < n; ++b)
        if (table_of_item[b] < -1 || table_of_item[b] >= s->bias_tables)
            return set_error(WLX_ERR_ARG, "bias select: item %d names table %d outside -1..%d", b, table_of_item[b], s->bias_tables - 1);
    CK(hipSetDevice(e->device));
    return bias_select_upload(s, n, table_of_item);
}

// ---- grammar-constrained decoding: the slot's DFA (include/wlx_grammar.h; dec_grammar.hip). Like the bias table: the device block and the pinned
// staging are allocated at the first call and stay where they are, the states are the slot's bias_state.
extern "C" int32_t wlx_grammar_set(wlx_engine* e, int32_t slot, int32_t eot, int32_t n_states, const int32_t* edge_off, const int32_t* edge_tok,
                                   const int32_t* edge_next, const int32_t* accept) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    // a refused grammar leaves whatever is installed whole (and allocates nothing)
    char why[200];
    if (!grammar_table_check(e->spec.vocab, eot, n_states, edge_off, edge_tok, edge_next, accept, why, sizeof(why))) return set_error(WLX_ERR_ARG, "%s", why);
    CK(hipSetDevice(e->device));
    CKR(bias_state_alloc(s));
    if (!s->d_grammar) {
        int *blk = nullptr, *stage = nullptr;
        CKR(dalloc(s->allocs, &blk, (size_t)GRAMMAR_TABLE_INTS, true));
        CKR(halloc(s->host_allocs, &stage, (size_t)GRAMMAR_TABLE_INTS));
        memset(stage, 0, sizeof(int) * GRAMMAR_TABLE_INTS);
        s->d_grammar = blk; s->h_grammar = stage; s->grammar = GrammarTable{blk, s->bias_state};
    }
    // the staging may still feed the copy of the previous grammar: wait for the stream, then rewrite it
    CK(hipStreamSynchronize(s->stream));
    grammar_table_pack(s->h_grammar, eot, n_states, edge_off, edge_tok, edge_next, accept);
    // (the used parts only: everything up to the last edge_next, and the accept flags at their fixed place)
    CK(hipMemcpyAsync(s->d_grammar, s->h_grammar, sizeof(int) * (size_t)(GRAMMAR_NEXT_AT + edge_off[n_states]), hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->d_grammar + GRAMMAR_ACCEPT_AT, s->h_grammar + GRAMMAR_ACCEPT_AT, sizeof(int) * (size_t)n_states, hipMemcpyHostToDevice, s->stream));
    s->grammar_eot = eot;
    s->bias_mode = BIAS_GRAMMAR;
    return WLX_OK;
}

extern "C" int32_t wlx_grammar_clear(wlx_engine* e, int32_t slot) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    if (sg_.s->bias_mode == BIAS_GRAMMAR) sg_.s->bias_mode = BIAS_NONE;      // (a bias table installed since stays)
    return WLX_OK;
}

extern "C" int32_t wlx_detect_language(wlx_engine* e, int32_t slot, int32_t batch, int32_t sot, const int32_t* lang_ids,
                                       int32_t n_lang, float* probs_out) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (batch < 1 || batch > s->enc_batch) return set_error(WLX_ERR_STATE, "detect_language before encode");
    if (!lang_ids || n_lang < 1 || n_lang > WLX_LANG_MAX || !probs_out) return set_error(WLX_ERR_ARG, "bad language id list");
    if (sot < 0 || sot >= e->spec.vocab) return set_error(WLX_ERR_ARG, "bad sot id");
    for (int i = 0; i < n_lang; ++i) if (lang_ids[i] < 0 || lang_ids[i] >= e->spec.vocab) return set_error(WLX_ERR_ARG, "bad language id");
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    // one decoder step on [sot] per item: row b -> cache row b*R (distinct per item)
    std::vector<int> tk(batch, sot), ps(batch, 0), ca(batch), an(batch), gi(batch);
    std::vector<short> anc((size_t)s->cache_rows * WLX_T_TEXT, 0);
    for (int b = 0; b < batch; ++b) { ca[b] = an[b] = b * s->R; gi[b] = b; anc[(size_t)(b * s->R) * WLX_T_TEXT] = (short)(b * s->R); }
    CKR(set_anc_rows(s, anc, 0, s->cache_rows));
    CKR(upload_rows(s, tk, ps, ca, an, gi));
    decoder_pass(e, s, s->step, batch, 1, batch, true, false);
    CK(hipMemcpyAsync(s->d_lang_ids, lang_ids, (size_t)n_lang * 4, hipMemcpyHostToDevice, st));
    launch_lang_probs(s->logits, s->ldl, batch, s->d_lang_ids, n_lang, s->d_probs, st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(probs_out, s->d_probs, (size_t)batch * n_lang * 4, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// word alignment: ctranslate2 Whisper.align(encoder_output, start_sequence, text_tokens, num_frames, median_filter_width)
// (transcriber_faster_whisper.py:1657-1663; CT2's source is not in the reference tree — the algorithm is the published
// one of openai/whisper timing.py find_alignment / HF generation_whisper.py _extract_token_timestamps):
//   teacher-forced decoder pass over tokens = sot_sequence + [no_timestamps] + text + [eot];
//   text_token_probs[i] = softmax(logits[n_sot + i][: eot])[text[i]];
//   per alignment head: softmax of q.k over the first num_frames/2 encoder positions; (w - mean) / std over the TOKEN axis;
//   median filter of width `median_filter_width` along time (reflect padding); mean over heads;
//   rows n_sot .. n_tokens-2; dynamic time warping on the negated matrix -> monotone (text index, time index) path.
// The decoder pass, the score capture and the token probabilities run on the device; the O(tokens x 1500) scalar
// post-processing (softmax / normalise / median / DTW) runs here on the host side of the call.
static void align_postprocess(const std::vector<float>& scores, int n_heads, int n_tok, int n_sot, int nf, int mw,
                              std::vector<int32_t>& ti, std::vector<int32_t>& fi) {
    const int TP = WLX_T_AUDIO_PAD;
    std::vector<float> w((size_t)n_heads * n_tok * nf);
    for (int h = 0; h < n_heads; ++h)
        for (int t = 0; t < n_tok; ++t) {
            const float* sr = &scores[((size_t)h * n_tok + t) * TP];
            float* wr = &w[((size_t)h * n_tok + t) * nf];
            float mx = sr[0];
            for (int f = 1; f < nf; ++f) mx = std::max(mx, sr[f]);
            double sum = 0.0;
            for (int f = 0; f < nf; ++f) { wr[f] = std::exp(sr[f] - mx); sum += wr[f]; }
            const float inv = (float)(1.0 / sum);
            for (int f = 0; f < nf; ++f) wr[f] *= inv;
        }
    // std / mean over the token axis (population std), per head and frame
    for (int h = 0; h < n_heads; ++h)
        for (int f = 0; f < nf; ++f) {
            double m = 0.0;
            for (int t = 0; t < n_tok; ++t) m += w[((size_t)h * n_tok + t) * nf + f];
            m /= n_tok;
            double v = 0.0;
            for (int t = 0; t < n_tok; ++t) { const double dlt = w[((size_t)h * n_tok + t) * nf + f] - m; v += dlt * dlt; }
            const double sd = std::sqrt(v / n_tok);
            for (int t = 0; t < n_tok; ++t) {
                float& x = w[((size_t)h * n_tok + t) * nf + f];
                x = (float)((x - m) / sd);
            }
        }
    // median filter along time, reflect padding (skipped, as in the reference implementation, when the row is too short)
    const int pad = mw / 2;
    if (mw > 1 && nf > pad) {
        std::vector<float> row(nf + 2 * pad), win(mw);
        for (size_t r = 0; r < (size_t)n_heads * n_tok; ++r) {
            float* wr = &w[r * nf];
            for (int i = 0; i < pad; ++i) { row[i] = wr[pad - i]; row[pad + nf + i] = wr[nf - 2 - i]; }
            std::copy(wr, wr + nf, row.begin() + pad);
            for (int f = 0; f < nf; ++f) {
                std::copy(row.begin() + f, row.begin() + f + mw, win.begin());
                std::nth_element(win.begin(), win.begin() + pad, win.end());
                wr[f] = win[pad];
            }
        }
    }
    // mean over heads, rows n_sot .. n_tok-2, negated: the DTW cost
    const int N = n_tok - 1 - n_sot, M = nf;
    std::vector<float> x((size_t)N * M);
    for (int i = 0; i < N; ++i)
        for (int f = 0; f < M; ++f) {
            float acc = 0.f;
            for (int h = 0; h < n_heads; ++h) acc += w[((size_t)h * n_tok + n_sot + i) * nf + f];
            x[(size_t)i * M + f] = -(acc / (float)n_heads);
        }
    // dynamic time warping (openai/whisper timing.py dtw_cpu)
    const float INF = std::numeric_limits<float>::infinity();
    std::vector<float> cost((size_t)(N + 1) * (M + 1), INF);
    std::vector<int8_t> trace((size_t)(N + 1) * (M + 1), -1);
    cost[0] = 0.f;
    for (int j = 1; j <= M; ++j)
        for (int i = 1; i <= N; ++i) {
            const float c0 = cost[(size_t)(i - 1) * (M + 1) + j - 1], c1 = cost[(size_t)(i - 1) * (M + 1) + j], c2 = cost[(size_t)i * (M + 1) + j - 1];
            float cc; int8_t tt;
            if (c0 < c1 && c0 < c2) { cc = c0; tt = 0; }
            else if (c1 < c0 && c1 < c2) { cc = c1; tt = 1; }
            else { cc = c2; tt = 2; }
            cost[(size_t)i * (M + 1) + j] = x[(size_t)(i - 1) * M + j - 1] + cc;
            trace[(size_t)i * (M + 1) + j] = tt;
        }
    for (int j = 0; j <= M; ++j) trace[j] = 2;
    for (int i = 0; i <= N; ++i) trace[(size_t)i * (M + 1)] = 1;
    int i = N, j = M;
    ti.clear(); fi.clear();
    while (i > 0 || j > 0) {
        ti.push_back(i - 1); fi.push_back(j - 1);
        const int8_t tt = trace[(size_t)i * (M + 1) + j];
        if (tt == 0) { --i; --j; } else if (tt == 1) --i; else --j;
    }
    std::reverse(ti.begin(), ti.end());
    std::reverse(fi.begin(), fi.end());
}

extern "C" int32_t wlx_align(wlx_engine* e, int32_t slot, int32_t item, const int32_t* tokens, int32_t n_tokens, int32_t n_sot,
                             int32_t num_frames, int32_t median_filter_width, const int32_t* heads, int32_t n_heads, int32_t eot,
                             int32_t* text_indices, int32_t* time_indices, int32_t path_cap, int32_t* n_path_out,
                             float* text_token_probs) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (!tokens || !heads || !text_indices || !time_indices || !n_path_out || !text_token_probs) return set_error(WLX_ERR_ARG, "null argument");
    if (item < 0 || item >= s->enc_batch) return set_error(WLX_ERR_STATE, "align: item %d not encoded", item);
    if (n_sot < 1 || n_tokens < n_sot + 3 || n_tokens > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "align: %d tokens with a start sequence of %d", n_tokens, n_sot);
    if (n_heads < 1 || n_heads > e->spec.dec_layers * e->H) return set_error(WLX_ERR_ARG, "align: bad head count");
    for (int i = 0; i < n_heads; ++i)
        if (heads[2 * i] < 0 || heads[2 * i] >= e->spec.dec_layers || heads[2 * i + 1] < 0 || heads[2 * i + 1] >= e->H)
            return set_error(WLX_ERR_ARG, "align: head (%d, %d) out of range", heads[2 * i], heads[2 * i + 1]);
    for (int i = 0; i < n_tokens; ++i) if (tokens[i] < 0 || tokens[i] >= e->spec.vocab) return set_error(WLX_ERR_ARG, "align: token out of vocabulary");
    if (eot < 1 || eot > e->spec.vocab || median_filter_width < 1 || (median_filter_width & 1) == 0) return set_error(WLX_ERR_ARG, "align: bad eot / filter width");
    int nf = num_frames / 2;
    if (nf < 1) nf = 1;
    if (nf > WLX_T_AUDIO) nf = WLX_T_AUDIO;
    const int n_text = n_tokens - n_sot - 2;
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    const size_t need = (size_t)n_heads * n_tokens * WLX_T_AUDIO_PAD;
    if (need > s->align_cap) {
        CK(hipStreamSynchronize(st));
        if (s->align_scores) CK(hipFree(s->align_scores));
        s->align_scores = nullptr; s->align_cap = 0;
        CK(hipMalloc(reinterpret_cast<void**>(&s->align_scores), need * sizeof(float)));   // grown on demand, the old one freed above: no free list
        s->align_cap = need;
    }
    const int crow = item * s->R;
    std::vector<short> anc((size_t)WLX_T_TEXT, (short)crow);
    CKR(set_anc_rows(s, anc, crow, 1));
    Slot::AlignCapture cap{s->align_scores, heads, n_heads, n_tokens, 0, item};
    std::vector<float> probs(n_tokens, 0.f);
    int rc = WLX_OK;
    s->align = &cap;
    for (int c0 = 0; c0 < n_tokens && rc == WLX_OK; c0 += 64) {
        const int rows = std::min(64, n_tokens - c0);
        const int groups = (rows + 15) / 16;
        std::vector<int> tk(rows), ps(rows), ca(rows, crow), an(rows, crow), gi(groups, item), tgt(rows, -1);
        for (int i = 0; i < rows; ++i) {
            tk[i] = tokens[c0 + i]; ps[i] = c0 + i;
            const int p = c0 + i;                       // logits at position p predict tokens[p + 1]
            if (p >= n_sot && p < n_sot + n_text) tgt[i] = tokens[p + 1];
        }
        rc = upload_rows(s, tk, ps, ca, an, gi);
        if (rc != WLX_OK) break;
        cap.row0 = c0;
        decoder_pass(e, s, s->step, rows, 16, groups, true, false);
        if (hipMemcpyAsync(s->d_align_tgt, tgt.data(), (size_t)rows * 4, hipMemcpyHostToDevice, st) != hipSuccess) { rc = WLX_ERR_HIP; break; }
        launch_token_prob_rows(s->logits, s->ldl, eot, rows, s->d_align_tgt, s->d_align_prob, st);
        if (hipMemcpyAsync(probs.data() + c0, s->d_align_prob, (size_t)rows * 4, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = WLX_ERR_HIP; break; }
        if (hipStreamSynchronize(st) != hipSuccess) { rc = WLX_ERR_HIP; break; }   // tgt / staging reuse
    }
    s->align = nullptr;
    if (rc != WLX_OK) return set_error(rc, "align: decoder pass failed");
    CK(hipGetLastError());
    std::vector<float> scores(need);
    CK(hipMemcpyAsync(scores.data(), s->align_scores, need * sizeof(float), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    std::vector<int32_t> ti, fi;
    align_postprocess(scores, n_heads, n_tokens, n_sot, nf, median_filter_width, ti, fi);
    if ((int)ti.size() > path_cap) return set_error(WLX_ERR_ARG, "align: path of %d steps exceeds the caller's capacity %d", (int)ti.size(), path_cap);
    memcpy(text_indices, ti.data(), ti.size() * 4);
    memcpy(time_indices, fi.data(), fi.size() * 4);
    *n_path_out = (int32_t)ti.size();
    for (int i = 0; i < n_text; ++i) text_token_probs[i] = probs[n_sot + i];
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// wlx_align_batch: the same alignment for a group of entries. The decoder passes run entry by entry with wlx_align's own launches (one
// entry's rows per pass: packing entries into a pass would change the row count, the GEMV dispatch and the bits of text_token_probs); what
// changes is everything around them. Every table of every chunk is written to pinned staging BEFORE the first launch, so nothing between
// the entries or chunks waits for the stream; the raw scores of all entries stay on the device, back to back, and align.hip turns them into
// cost matrices and DTW paths in one launch sequence; paths, counts and probabilities land in pinned memory and the call waits once.
namespace {

constexpr int AL_PS = 1952;             // path row of the pinned result area (>= 446 + 1500, the longest path)
constexpr int AL_CHUNKS = (WLX_T_TEXT + 63) / 64;
constexpr int AL_CHUNK_INTS = 64 * 5 + 8;       // [token | pos | cache | ancrow : rows each | group_item : groups | target : rows], rows <= 64
struct AlignStaging {
    AlignEnt* ent; int* rows; int32_t *ti, *fi, *np; float* probs;
    size_t bytes;
};
AlignStaging align_staging(unsigned char* base) {
    AlignStaging g{};
    size_t off = 0;
    auto take = [&](size_t bytes) { unsigned char* p = base + off; off += (bytes + 63) / 64 * 64; return p; };
    g.ent = reinterpret_cast<AlignEnt*>(take(sizeof(AlignEnt) * WLX_ALIGN_MAX_BATCH));
    g.rows = reinterpret_cast<int*>(take(sizeof(int) * (size_t)WLX_ALIGN_MAX_BATCH * AL_CHUNKS * AL_CHUNK_INTS));
    g.ti = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)WLX_ALIGN_MAX_BATCH * AL_PS));
    g.fi = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)WLX_ALIGN_MAX_BATCH * AL_PS));
    g.np = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * WLX_ALIGN_MAX_BATCH));
    g.probs = reinterpret_cast<float*>(take(sizeof(float) * (size_t)WLX_ALIGN_MAX_BATCH * WLX_T_TEXT));
    g.bytes = off;
    return g;
}

// a device buffer owned by name, grown on demand: WLX_ERR_NOMEM (and an empty buffer) when the larger one cannot be had
int grow_floats(Slot* s, float** buf, size_t* cap, size_t need, const char* what) {
    if (need <= *cap) return WLX_OK;
    CK(hipStreamSynchronize(s->stream));
    if (*buf) CK(hipFree(*buf));
    *buf = nullptr; *cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(buf), need * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        return set_error(WLX_ERR_NOMEM, "align: %zu bytes of %s cannot be allocated", need * sizeof(float), what);
    }
    *cap = need;
    return WLX_OK;
}

}  // namespace

extern "C" int32_t wlx_align_batch(wlx_engine* e, int32_t slot, int32_t n, const int32_t* items, const int32_t* tokens, const int32_t* n_tokens,
                                   int32_t tokens_stride, int32_t n_sot, const int32_t* num_frames, int32_t median_filter_width,
                                   const int32_t* heads, int32_t n_heads, int32_t eot, int32_t* text_indices, int32_t* time_indices,
                                   int32_t path_stride, int32_t* n_path_out, float* text_token_probs, int32_t probs_stride) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    Slot* s = sg_.s;
    if (n < 0 || n > WLX_ALIGN_MAX_BATCH) return set_error(WLX_ERR_ARG, "align: %d entries outside 0..%d", n, WLX_ALIGN_MAX_BATCH);
    if (!tokens || !n_tokens || !num_frames || !heads || !text_indices || !time_indices || !n_path_out || !text_token_probs)
        return set_error(WLX_ERR_ARG, "null argument");
    if (n_sot < 1) return set_error(WLX_ERR_ARG, "align: a start sequence of %d", n_sot);
    if (n_heads < 1 || n_heads > e->spec.dec_layers * e->H) return set_error(WLX_ERR_ARG, "align: bad head count");
    for (int i = 0; i < n_heads; ++i)
        if (heads[2 * i] < 0 || heads[2 * i] >= e->spec.dec_layers || heads[2 * i + 1] < 0 || heads[2 * i + 1] >= e->H)
            return set_error(WLX_ERR_ARG, "align: head (%d, %d) out of range", heads[2 * i], heads[2 * i + 1]);
    if (eot < 1 || eot > e->spec.vocab) return set_error(WLX_ERR_ARG, "align: bad eot");
    if (median_filter_width < 1 || median_filter_width > WLX_ALIGN_MAX_MEDIAN || (median_filter_width & 1) == 0)
        return set_error(WLX_ERR_ARG, "align: filter width %d must be odd in 1..%d", median_filter_width, WLX_ALIGN_MAX_MEDIAN);
    AlignEnt ent[WLX_ALIGN_MAX_BATCH];
    int item_of[WLX_ALIGN_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        const int item = items ? items[i] : i, nt = n_tokens[i];
        if (item < 0 || item >= s->enc_batch) return set_error(WLX_ERR_STATE, "align: entry %d: item %d not encoded", i, item);
        if (nt < n_sot + 3 || nt > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "align: entry %d: %d tokens with a start sequence of %d", i, nt, n_sot);
        if (tokens_stride < nt) return set_error(WLX_ERR_ARG, "align: tokens_stride %d below the %d tokens of entry %d", tokens_stride, nt, i);
        const int32_t* tk = tokens + (size_t)i * tokens_stride;
        for (int k = 0; k < nt; ++k) if (tk[k] < 0 || tk[k] >= e->spec.vocab) return set_error(WLX_ERR_ARG, "align: entry %d: token out of vocabulary", i);
        const int nf = std::min(std::max(num_frames[i] / 2, 1), (int)WLX_T_AUDIO);
        ent[i] = AlignEnt{};
        ent[i].n_tok = nt; ent[i].nf = nf; ent[i].N = nt - 1 - n_sot;
        item_of[i] = item;
        if (path_stride < ent[i].N + nf) return set_error(WLX_ERR_ARG, "align: path_stride %d below the longest path (%d) of entry %d", path_stride, ent[i].N + nf, i);
        if (probs_stride < nt - n_sot - 2) return set_error(WLX_ERR_ARG, "align: probs_stride %d below the %d text tokens of entry %d", probs_stride, nt - n_sot - 2, i);
    }
    if (n == 0) return WLX_OK;
    AlignPlan plan{};
    align_layout(ent, n, n_heads, &plan);
    CK(hipSetDevice(e->device));
    hipStream_t st = s->stream;
    // ---- memory, all of it before the first launch
    if (!s->h_align) {
        CKR(halloc(s->host_allocs, &s->h_align, align_staging(nullptr).bytes));
        CKR(dalloc(s->allocs, &s->d_align_ent, (size_t)WLX_ALIGN_MAX_BATCH, false));
    }
    for (hipEvent_t* ev : {&s->ev_al0, &s->ev_al1, &s->ev_al2}) if (!*ev) CK(hipEventCreate(ev));
    CKR(grow_floats(s, &s->align_scores, &s->align_cap, plan.score_floats, "alignment scores"));
    const size_t post_need = plan.stat_floats + plan.x_floats + plan.trace_words;
    CKR(grow_floats(s, &s->align_post, &s->align_post_cap, post_need, "alignment scratch"));
    float* d_stats = s->align_post;
    float* d_x = d_stats + plan.stat_floats;
    unsigned* d_trace = reinterpret_cast<unsigned*>(d_x + plan.x_floats);
    // ---- every table of the call into the pinned staging (free: the previous call on this slot ended with a wait for the stream)
    const AlignStaging g = align_staging(s->h_align);
    memcpy(g.ent, ent, sizeof(AlignEnt) * n);
    for (int i = 0; i < n; ++i) {
        const int nt = ent[i].n_tok, n_text = nt - n_sot - 2, crow = item_of[i] * s->R;
        const int32_t* tk = tokens + (size_t)i * tokens_stride;
        for (int c0 = 0, c = 0; c0 < nt; c0 += 64, ++c) {
            const int rows = std::min(64, nt - c0), groups = (rows + 15) / 16;
            int* h = g.rows + ((size_t)i * AL_CHUNKS + c) * AL_CHUNK_INTS;
            int* tgt = h + 4 * rows + groups;
            for (int r = 0; r < rows; ++r) {
                const int p = c0 + r;                       // logits at position p predict tokens[p + 1]
                h[r] = tk[p]; h[rows + r] = p; h[2 * rows + r] = crow; h[3 * rows + r] = crow;
                tgt[r] = (p >= n_sot && p < n_sot + n_text) ? tk[p + 1] : -1;
            }
            for (int gi = 0; gi < groups; ++gi) h[4 * rows + gi] = item_of[i];
        }
    }
    // ---- one launch sequence
    int rc = WLX_OK;
    auto ok = [&](hipError_t err) { if (err != hipSuccess && rc == WLX_OK) rc = WLX_ERR_HIP; return rc == WLX_OK; };
    ok(hipEventRecord(s->ev_al0, st));
    ok(hipMemcpyAsync(s->d_align_ent, g.ent, sizeof(AlignEnt) * n, hipMemcpyHostToDevice, st));
    Slot::AlignCapture cap{s->align_scores, heads, n_heads, 0, 0, 0};
    s->align = &cap;
    for (int i = 0; i < n && rc == WLX_OK; ++i) {
        const int nt = ent[i].n_tok, crow = item_of[i] * s->R;
        // identity ancestry of the entry's cache row (what wlx_align uploads: 448 times its own row)
        if (!ok(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(s->d_anc + (size_t)crow * WLX_T_TEXT), (unsigned short)crow, WLX_T_TEXT, st))) break;
        cap.scores = s->align_scores + ent[i].score_off; cap.n_tok = nt; cap.item = item_of[i];
        for (int c0 = 0, c = 0; c0 < nt && rc == WLX_OK; c0 += 64, ++c) {
            const int rows = std::min(64, nt - c0), groups = (rows + 15) / 16;
            const int* h = g.rows + ((size_t)i * AL_CHUNKS + c) * AL_CHUNK_INTS;
            s->anc_ident = rows == 1 && crow == 0;          // upload_rows' rule (ancrow[r] == r for every row) on these tables
            if (upload_row_tables(s, s->step, h, rows, groups) != WLX_OK) { rc = WLX_ERR_HIP; break; }
            cap.row0 = c0;
            decoder_pass(e, s, s->step, rows, 16, groups, true, false);
            if (!ok(hipMemcpyAsync(s->d_align_tgt, h + 4 * rows + groups, (size_t)rows * 4, hipMemcpyHostToDevice, st))) break;
            launch_token_prob_rows(s->logits, s->ldl, eot, rows, s->d_align_tgt, s->d_align_prob, st);
            ok(hipMemcpyAsync(g.probs + (size_t)i * WLX_T_TEXT + c0, s->d_align_prob, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
        }
    }
    s->align = nullptr;
    if (rc == WLX_OK) {
        ok(hipEventRecord(s->ev_al1, st));
        launch_align_cost(s->d_align_ent, n, n_heads, n_sot, median_filter_width, plan, s->align_scores, d_stats, d_x, st);
        launch_align_dtw(s->d_align_ent, n, plan.max_N, d_x, d_trace, g.ti, g.fi, AL_PS, g.np, st);
        ok(hipEventRecord(s->ev_al2, st));
    }
    const hipError_t waited = hipStreamSynchronize(st);     // the one wait of the call
    if (rc != WLX_OK) return set_error(rc, "align: a launch of the batch failed");
    CK(waited);
    CK(hipGetLastError());
    CK(hipEventElapsedTime(&s->align_pass_ms, s->ev_al0, s->ev_al1));
    CK(hipEventElapsedTime(&s->align_post_ms, s->ev_al1, s->ev_al2));
    for (int i = 0; i < n; ++i) {
        const int np = g.np[i], n_text = ent[i].n_tok - n_sot - 2;
        if (np < 0 || np > path_stride) return set_error(WLX_ERR_HIP, "align: entry %d came back with a path of %d steps", i, np);
        memcpy(text_indices + (size_t)i * path_stride, g.ti + (size_t)i * AL_PS, (size_t)np * 4);
        memcpy(time_indices + (size_t)i * path_stride, g.fi + (size_t)i * AL_PS, (size_t)np * 4);
        n_path_out[i] = np;
        for (int k = 0; k < n_text; ++k) text_token_probs[(size_t)i * probs_stride + k] = g.probs[(size_t)i * WLX_T_TEXT + n_sot + k];
    }
    return WLX_OK;
}

extern "C" int32_t wlx_debug_align_timings(wlx_engine* e, int32_t slot, float* pass_ms, float* post_ms) {
    SlotGuard sg_;
    CKR(slot_acquire(e, slot, sg_));
    if (!pass_ms || !post_ms) return set_error(WLX_ERR_ARG, "null argument");
    *pass_ms = sg_.s->align_pass_ms;
    *post_ms = sg_.s->align_post_ms;
    return WLX_OK;
}
