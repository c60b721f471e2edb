// mt_engine.hip — the M2M100 / small100 translation engine behind the wlx_mt_* entry points of include/wlx.h.
//
// Per call: the items' sources are packed by length (no pad rows), embedded (scale * shared + sinusoidal positions), run through
// the pre-norm encoder, and the cross K / V of every decoder layer is computed once from the final encoder output (one GEMM over
// all layers). The decoder then runs one eager step per generated token for batch x num_beams rows: fused q/k/v projection, KV
// append, self-attention through the beam ancestry table, cross-attention over each item's own source length, ReLU MLP, final
// LayerNorm and the tied vocabulary projection in fp32, followed by the two-stage log-softmax + top-k kernels of mt.hip. The
// candidates (2 x num_beams per row) come back to the host, where Hugging Face's beam-search bookkeeping (generation/utils.py
// _beam_search of transformers 5.x: length normaliser, early_stopping heuristics, forced EOS, no_repeat_ngram) runs in a few
// microseconds per step. All projections use the MFMA GEMM of gemm.hip; nothing is captured into a graph. Error macros, allocation
// and weight ingestion (the layer loader included) are the shared host layer of host.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "mt.h"

using namespace wlx;

namespace {

struct MtSlot {
    std::atomic<bool> busy{false};
    int B = 0, R = 0, max_src = 0, rows_cap = 0, src_cap = 0, tmax = WLX_T_TEXT;
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {};
    std::vector<void*> allocs, host_allocs;
    // encoder (packed source rows)
    float *xe = nullptr, *enc32 = nullptr;
    half_t *he = nullptr, *qkve = nullptr, *atte = nullptr, *ffe = nullptr, *ckv = nullptr;   // ckv: [src_cap][L * 2d]
    // decoder rows
    float *xd = nullptr, *logits = nullptr, *tk_scratch = nullptr, *tk_val = nullptr;
    half_t *hd = nullptr, *qkvd = nullptr, *qd = nullptr, *attd = nullptr, *ffd = nullptr, *kc = nullptr, *vc = nullptr;
    int *tk_cidx = nullptr, *tk_idx = nullptr;
    int *d_tok = nullptr, *d_pos = nullptr, *d_anc = nullptr, *d_ban = nullptr, *d_nban = nullptr;
    int *d_src_tok = nullptr, *d_src_pos = nullptr;
    MtAttnGroup *d_genc = nullptr, *d_gself = nullptr, *d_gcross = nullptr;
    int ban_ld = 0;
    // pinned host staging. An asynchronous copy reads its pinned source when it EXECUTES, so a buffer is rewritten only after the
    // stream has been synchronised past the copies that read it. The encoder has its own buffers (h_src_*, h_genc): run_generate
    // fills the decoder's h_tok / h_pos right after encode() returns, while the encoder's copies may still be queued.
    int *h_src_tok = nullptr, *h_src_pos = nullptr;
    int *h_tok = nullptr, *h_pos = nullptr, *h_anc = nullptr, *h_ban = nullptr, *h_nban = nullptr, *h_tk_idx = nullptr;
    float* h_tk_val = nullptr;
    MtAttnGroup *h_genc = nullptr, *h_gself = nullptr, *h_gcross = nullptr;
    // state of the last encode
    int n_items = 0, n_src = 0;
    std::vector<int> src_off, src_len;
    float enc_ms = 0.f, dec_ms = 0.f;
    int steps = 0;
    // wlx_mt_debug_search: host logits [steps][rows][vocab] that stand in for the network pass of run_generate's steps
    const float* inject = nullptr;
    // device search (mt_search.hip; wlx_mt_translate_many): state of one generate, allocated at the slot's first use
    bool has_search = false;
    MtSearchState sd{};
    float *d_lp = nullptr, *h_lp = nullptr;
    hipEvent_t ev_blk = nullptr;
};

}  // namespace

struct wlx_mt {
    wlx_mt_spec spec{};
    int device = 0;
    std::vector<LayerW> enc, dec;
    float *enc_ln_g = nullptr, *enc_ln_b = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr;
    half_t* E = nullptr;          // shared embedding, packed (vocab x d): token rows for the embedding, the tied output projection
    half_t* Wckv = nullptr;       // cross k / v of every decoder layer: [L * 2d][d] packed
    float* bckv = nullptr;
    float* sinpos = nullptr;      // [max_positions + 2][d]
    float embed_scale = 1.f;
    std::vector<void*> allocs;
    std::mutex mu;
    std::map<int, MtSlot*> slots;
    int next_slot = 0;
};

namespace {

// C = A W^T + b (fp16 out) or X += A W^T + b (fp32): the encoder GEMM of gemm.hip
void gemm(const half_t* A, long lda, int M, const half_t* Wp, int K, int N, const float* bias, int mode, half_t* C, long ldc,
          float* X, long ldx, hipStream_t s) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.Wp = Wp; p.KT = K / 32; p.M = M; p.N = N; p.mode = mode; p.bias = bias;
    p.C = C; p.ldc = ldc; p.X = X; p.ldx = ldx;
    launch_gemm(p, 1, s);
}

MtSlot* slot_of(wlx_mt* m, int id) {
    std::lock_guard<std::mutex> g(m->mu);
    auto it = m->slots.find(id);
    return it == m->slots.end() ? nullptr : it->second;
}

struct Busy {
    MtSlot* s;
    bool ok;
    explicit Busy(MtSlot* s_) : s(s_) { bool f = false; ok = s->busy.compare_exchange_strong(f, true); }
    ~Busy() { if (ok) s->busy.store(false); }
};

// HF create_position_ids_from_input_ids: non-pad tokens count from padding_idx + 1 (+ past), pad tokens sit at padding_idx
inline int position_of(int tok, int nonpad_before_incl, int past, int pad) { return tok != pad ? nonpad_before_incl + past + pad : pad; }

int encode(wlx_mt* m, MtSlot* s, int batch, const int32_t* src, const int32_t* lens, int stride) {
    const wlx_mt_spec& sp = m->spec;
    const int d = sp.d_model, F = sp.ffn, H = sp.n_heads, Ld = sp.dec_layers;
    if (batch < 1 || batch > s->B) return set_error(WLX_ERR_ARG, "batch %d outside 1..%d (slot max_batch)", batch, s->B);
    if (!src || !lens) return set_error(WLX_ERR_ARG, "null source");
    s->src_off.assign(batch, 0);
    s->src_len.assign(batch, 0);
    int n = 0, ng = 0;
    for (int i = 0; i < batch; ++i) {
        const int S = lens[i];
        if (S < 1 || S > s->max_src || S > stride) return set_error(WLX_ERR_ARG, "item %d: source length %d outside 1..%d", i, S, std::min(s->max_src, stride));
        s->src_off[i] = n;
        s->src_len[i] = S;
        int c = 0;
        for (int j = 0; j < S; ++j) {
            const int tok = src[(long)i * stride + j];
            if (tok < 0 || tok >= sp.vocab) return set_error(WLX_ERR_ARG, "item %d: token %d outside the vocabulary", i, tok);
            c += tok != sp.pad_id;
            s->h_src_tok[n + j] = tok;
            s->h_src_pos[n + j] = position_of(tok, c, 0, sp.pad_id);
        }
        for (int j = 0; j < S; j += 16) s->h_genc[ng++] = MtAttnGroup{n + j, std::min(16, S - j), n, S};
        n += S;
    }
    s->n_items = batch;
    s->n_src = n;
    hipStream_t st = s->st;
    CK(hipEventRecord(s->ev[0], st));
    CK(hipMemcpyAsync(s->d_src_tok, s->h_src_tok, n * sizeof(int), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_src_pos, s->h_src_pos, n * sizeof(int), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_genc, s->h_genc, ng * sizeof(MtAttnGroup), hipMemcpyHostToDevice, st));
    launch_mt_embed(s->d_src_tok, s->d_src_pos, n, m->E, d / 32, m->embed_scale, m->sinpos, d, s->xe, st);
    for (const LayerW& w : m->enc) {
        launch_layernorm_f16(s->xe, d, w.ln1_g, w.ln1_b, s->he, d, n, d, st);
        gemm(s->he, d, n, w.Wqkv, d, 3 * d, w.bqkv, GEMM_STORE_F16, s->qkve, 3 * d, nullptr, 0, st);
        launch_mt_attn(s->qkve, 3 * d, s->qkve + d, 3 * d, s->qkve + 2 * d, 3 * d, s->atte, d, s->d_genc, ng, 16, H, nullptr, 0, 0, st);
        gemm(s->atte, d, n, w.Wo, d, d, w.bo, GEMM_RESID_F32, nullptr, 0, s->xe, d, st);
        launch_layernorm_f16(s->xe, d, w.ln3_g, w.ln3_b, s->he, d, n, d, st);
        gemm(s->he, d, n, w.W1, d, F, w.b1, GEMM_STORE_F16, s->ffe, F, nullptr, 0, st);
        launch_mt_relu_f16(s->ffe, F, n, F, st);
        gemm(s->ffe, F, n, w.W2, F, d, w.b2, GEMM_RESID_F32, nullptr, 0, s->xe, d, st);
    }
    launch_layernorm_f16_f32(s->xe, d, m->enc_ln_g, m->enc_ln_b, s->he, s->enc32, d, n, d, st);
    gemm(s->he, d, n, m->Wckv, d, 2 * d * Ld, m->bckv, GEMM_STORE_F16, s->ckv, 2L * d * Ld, nullptr, 0, st);
    CK(hipGetLastError());
    CK(hipEventRecord(s->ev[1], st));
    return WLX_OK;
}

// the launches of one decoder step for `rows` rows (R per item over the slot's encoded items) at position t: logits -> s->logits.
// Every table it reads is in device memory: tokens, positions, the ancestry table and the self-attention groups of the rows
// (d_gcross: the slot's, constant over a generate).
int decode_launch(wlx_mt* m, MtSlot* s, int rows, int R, int t, const int* d_tok, const int* d_pos, const int* d_anc,
                  const MtAttnGroup* d_gself) {
    const wlx_mt_spec& sp = m->spec;
    const int d = sp.d_model, F = sp.ffn, H = sp.n_heads, Ld = sp.dec_layers, T = s->tmax;
    hipStream_t st = s->st;
    launch_mt_embed(d_tok, d_pos, rows, m->E, d / 32, m->embed_scale, m->sinpos, d, s->xd, st);
    const long cache_layer = (long)s->rows_cap * T * d;
    for (int l = 0; l < Ld; ++l) {
        const LayerW& w = m->dec[l];
        half_t* kc = s->kc + l * cache_layer;
        half_t* vc = s->vc + l * cache_layer;
        launch_layernorm_f16(s->xd, d, w.ln1_g, w.ln1_b, s->hd, d, rows, d, st);
        gemm(s->hd, d, rows, w.Wqkv, d, 3 * d, w.bqkv, GEMM_STORE_F16, s->qkvd, 3 * d, nullptr, 0, st);
        launch_mt_kv_append(s->qkvd, 3 * d, rows, d, kc, vc, T, t, st);
        launch_mt_attn(s->qkvd, 3 * d, kc, d, vc, d, s->attd, d, d_gself, rows, 1, H, d_anc, T, T, st);
        gemm(s->attd, d, rows, w.Wo, d, d, w.bo, GEMM_RESID_F32, nullptr, 0, s->xd, d, st);
        launch_layernorm_f16(s->xd, d, w.ln2_g, w.ln2_b, s->hd, d, rows, d, st);
        gemm(s->hd, d, rows, w.Wcq, d, d, w.bcq, GEMM_STORE_F16, s->qd, d, nullptr, 0, st);
        const long ldkv = 2L * d * Ld;
        launch_mt_attn(s->qd, d, s->ckv + 2L * d * l, ldkv, s->ckv + 2L * d * l + d, ldkv, s->attd, d, s->d_gcross, s->n_items, R, H,
                       nullptr, 0, 0, st);
        gemm(s->attd, d, rows, w.Wco, d, d, w.bco, GEMM_RESID_F32, nullptr, 0, s->xd, d, st);
        launch_layernorm_f16(s->xd, d, w.ln3_g, w.ln3_b, s->hd, d, rows, d, st);
        gemm(s->hd, d, rows, w.W1, d, F, w.b1, GEMM_STORE_F16, s->ffd, F, nullptr, 0, st);
        launch_mt_relu_f16(s->ffd, F, rows, F, st);
        gemm(s->ffd, F, rows, w.W2, F, d, w.b2, GEMM_RESID_F32, nullptr, 0, s->xd, d, st);
    }
    launch_layernorm_f16(s->xd, d, m->dec_ln_g, m->dec_ln_b, s->hd, d, rows, d, st);
    CK(hipMemsetAsync(s->logits, 0, (size_t)rows * sp.vocab * sizeof(float), st));
    gemm(s->hd, d, rows, m->E, d, sp.vocab, nullptr, GEMM_RESID_F32, nullptr, 0, s->logits, sp.vocab, st);
    CK(hipGetLastError());
    return WLX_OK;
}

// one decoder step with the host search: h_tok / h_pos / h_anc of the rows are set by the caller and uploaded here.
// With injected logits (wlx_mt_debug_search) the step's logits are copied in and no network pass runs.
int decode_step(wlx_mt* m, MtSlot* s, int rows, int R, int t) {
    const int T = s->tmax;
    hipStream_t st = s->st;
    if (s->inject) {
        const size_t n = (size_t)rows * m->spec.vocab;
        CK(hipMemcpyAsync(s->logits, s->inject + (size_t)t * n, n * sizeof(float), hipMemcpyHostToDevice, st));
        return WLX_OK;
    }
    for (int r = 0; r < rows; ++r) s->h_gself[r] = MtAttnGroup{r, 1, 0, t + 1};
    for (int i = 0; i < s->n_items; ++i) s->h_gcross[i] = MtAttnGroup{i * R, R, s->src_off[i], s->src_len[i]};
    CK(hipMemcpyAsync(s->d_tok, s->h_tok, rows * sizeof(int), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_pos, s->h_pos, rows * sizeof(int), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_anc, s->h_anc, (size_t)rows * T * sizeof(int), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_gself, s->h_gself, rows * sizeof(MtAttnGroup), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->d_gcross, s->h_gcross, s->n_items * sizeof(MtAttnGroup), hipMemcpyHostToDevice, st));
    return decode_launch(m, s, rows, R, t, s->d_tok, s->d_pos, s->d_anc, s->d_gself);
}

// top-k candidates of the step's rows -> pinned host h_tk_val / h_tk_idx [rows][k]; waits for the stream
int fetch_topk(wlx_mt* m, MtSlot* s, int rows, int k, bool with_bans) {
    hipStream_t st = s->st;
    if (with_bans) {
        CK(hipMemcpyAsync(s->d_nban, s->h_nban, rows * sizeof(int), hipMemcpyHostToDevice, st));
        CK(hipMemcpyAsync(s->d_ban, s->h_ban, (size_t)rows * s->ban_ld * sizeof(int), hipMemcpyHostToDevice, st));
    }
    launch_mt_topk(s->logits, rows, m->spec.vocab, with_bans ? s->d_ban : nullptr, with_bans ? s->d_nban : nullptr, s->ban_ld, k,
                   s->tk_scratch, s->tk_cidx, s->tk_val, s->tk_idx, st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(s->h_tk_val, s->tk_val, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost, st));
    CK(hipMemcpyAsync(s->h_tk_idx, s->tk_idx, (size_t)rows * k * sizeof(int), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    return WLX_OK;
}

// banned next tokens of one hypothesis (HF NoRepeatNGramLogitsProcessor over the whole sequence incl. the decoder start)
void banned_ngrams(const int* seq, int cur_len, int n, std::vector<int>& out) {
    out.clear();
    if (n <= 0 || cur_len + 1 < n) return;
    const int start = cur_len + 1 - n;
    for (int a = 0; a + n <= cur_len; ++a) {
        bool eq = true;
        for (int j = 0; j < n - 1 && eq; ++j) eq = seq[a + j] == seq[start + j];
        if (eq) out.push_back(seq[a + n - 1]);
    }
}

struct Cand { float v; int beam, tok; long flat; };

int run_generate(wlx_mt* m, MtSlot* s, const wlx_mt_gen_opts& o, int32_t* tokens_out, int tokens_stride, int32_t* n_out,
                 float* scores_out) {
    const wlx_mt_spec& sp = m->spec;
    const int B = s->n_items, R = o.num_beams, rows = B * R, T = s->tmax, ML = o.max_length, V = sp.vocab;
    const int eos = sp.eos_id, pad = sp.pad_id;
    const bool forced = o.forced_eos_token_id >= 0;
    const int K = R == 1 ? 1 : 2 * R;
    const int nng = o.no_repeat_ngram_size;
    // sequences incl. the decoder start
    std::vector<int> run(rows * ML, pad), fin(rows * ML, pad), fin_len(rows, 0);
    std::vector<float> run_score(rows, 0.f), fin_score(rows, -1.0e9f);
    std::vector<char> fin_done(rows, 0), unsat(B, 1), item_done(B, 0);
    std::vector<float> greedy_score(B, 0.f);
    for (int r = 0; r < rows; ++r) {
        run[r * ML] = sp.decoder_start_id;
        if (r % R) run_score[r] = -1.0e9f;
    }
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < T; ++j) s->h_anc[(long)r * T + j] = r;
    int cur_len = 1;
    s->steps = 0;
    CK(hipEventRecord(s->ev[2], s->st));
    std::vector<int> ban;
    while (true) {
        const int t = cur_len - 1;                 // position of the token fed in this step
        const bool force_now = forced && cur_len == ML - 1;
        if (!force_now) {
            for (int r = 0; r < rows; ++r) {
                s->h_tok[r] = run[r * ML + t];
                s->h_anc[(long)r * T + t] = r;
                s->h_pos[r] = position_of(run[r * ML + t], 1, t, pad);
            }
            CKR(decode_step(m, s, rows, R, t));
            bool any_ban = false;
            for (int r = 0; r < rows; ++r) {
                banned_ngrams(&run[r * ML], cur_len, nng, ban);
                const int nb = std::min((int)ban.size(), s->ban_ld);
                s->h_nban[r] = nb;
                for (int j = 0; j < nb; ++j) s->h_ban[(long)r * s->ban_ld + j] = ban[j];
                any_ban |= nb > 0;
            }
            CKR(fetch_topk(m, s, rows, K, any_ban));
            s->steps++;
        }
        if (R == 1) {   // greedy (HF _sample with do_sample = False)
            bool all_done = true;
            for (int b = 0; b < B; ++b) {
                int tok;
                float lp;
                if (force_now) { tok = o.forced_eos_token_id; lp = 0.f; }
                else { tok = s->h_tk_idx[b]; lp = s->h_tk_val[b]; }
                if (item_done[b]) tok = pad;
                else greedy_score[b] += lp;
                run[b * ML + cur_len] = tok;
                if (!item_done[b]) {
                    fin_len[b] = cur_len + 1;
                    if (tok == eos) item_done[b] = 1;
                }
                all_done &= item_done[b] != 0;
            }
            cur_len++;
            if (all_done || cur_len >= ML) break;
            continue;
        }
        // beam search, per item (HF _beam_search: _get_top_k_continuations, _get_running_beams_for_next_iteration,
        // _update_finished_beams, _check_early_stop_heuristic)
        const int K2 = 2 * R;
        bool any_unsat = false, all_fin = true, all_hit = true;
        std::vector<int> nrun(rows * ML), nanc((size_t)rows * T);
        std::vector<float> nscore(rows);
        for (int b = 0; b < B; ++b) {
            std::vector<Cand> c;
            c.reserve(R * K2);
            for (int bb = 0; bb < R; ++bb) {
                const int r = b * R + bb;
                if (force_now) {
                    c.push_back(Cand{0.f + run_score[r], bb, o.forced_eos_token_id, (long)bb * V + o.forced_eos_token_id});
                    continue;
                }
                for (int k = 0; k < K2; ++k) {
                    const int tok = s->h_tk_idx[r * K2 + k];
                    if (tok < 0) continue;
                    c.push_back(Cand{s->h_tk_val[r * K2 + k] + run_score[r], bb, tok, (long)bb * V + tok});
                }
            }
            std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& z) { return a.v > z.v || (a.v == z.v && a.flat < z.flat); });
            if ((int)c.size() > K2) c.resize(K2);
            const int nk = (int)c.size();
            std::vector<char> hit(nk);
            for (int k = 0; k < nk; ++k) {
                hit[k] = c[k].tok == eos || cur_len + 1 >= ML;
                all_hit &= hit[k] != 0;
            }
            // running beams of the next step
            std::vector<int> order(nk);
            std::vector<float> rv(nk);
            for (int k = 0; k < nk; ++k) { order[k] = k; rv[k] = c[k].v + (hit[k] ? -1.0e9f : 0.f); }
            std::stable_sort(order.begin(), order.end(), [&](int a, int z) { return rv[a] > rv[z]; });
            for (int bb = 0; bb < R; ++bb) {
                const int r = b * R + bb;
                if (bb >= nk) { nscore[r] = -INFINITY; std::copy(&run[r * ML], &run[r * ML] + ML, &nrun[r * ML]); continue; }
                const Cand& q = c[order[bb]];
                const int src = b * R + q.beam;
                std::copy(&run[src * ML], &run[src * ML] + ML, &nrun[r * ML]);
                nrun[r * ML + cur_len] = q.tok;
                nscore[r] = rv[order[bb]];
                for (int j = 0; j <= t; ++j) nanc[(long)r * T + j] = s->h_anc[(long)src * T + j];
            }
            // finished beams
            const float denom = (float)pow((double)cur_len, (double)o.length_penalty);
            bool full = o.early_stopping == 1;
            for (int bb = 0; bb < R; ++bb) full &= fin_done[b * R + bb] != 0;
            std::vector<float> ms(R + nk);
            std::vector<int> mseq((R + nk) * ML), mlen(R + nk);
            std::vector<char> mfin(R + nk);
            for (int bb = 0; bb < R; ++bb) {
                const int r = b * R + bb;
                ms[bb] = fin_score[r];
                std::copy(&fin[r * ML], &fin[r * ML] + ML, &mseq[bb * ML]);
                mlen[bb] = fin_len[r];
                mfin[bb] = fin_done[r];
            }
            for (int k = 0; k < nk; ++k) {
                const bool just = hit[k] && k < R;
                float v = c[k].v / denom;
                v += full ? -1.0e9f : 0.f;
                v += unsat[b] ? 0.f : -1.0e9f;
                v += just ? 0.f : -1.0e9f;
                ms[R + k] = v;
                const int src = b * R + c[k].beam;
                std::copy(&run[src * ML], &run[src * ML] + ML, &mseq[(R + k) * ML]);
                mseq[(R + k) * ML + cur_len] = c[k].tok;
                mlen[R + k] = cur_len + 1;
                mfin[R + k] = just;
            }
            std::vector<int> mo(R + nk);
            for (int i = 0; i < R + nk; ++i) mo[i] = i;
            std::stable_sort(mo.begin(), mo.end(), [&](int a, int z) { return ms[a] > ms[z]; });
            for (int bb = 0; bb < R; ++bb) {
                const int r = b * R + bb, i = mo[bb];
                fin_score[r] = ms[i];
                std::copy(&mseq[i * ML], &mseq[i * ML] + ML, &fin[r * ML]);
                fin_len[r] = mlen[i];
                fin_done[r] = mfin[i];
            }
        }
        // the ancestry rows are gathered from the OLD table (a row may be the parent of a row written before it)
        for (int r = 0; r < rows; ++r) std::copy(&nanc[(long)r * T], &nanc[(long)r * T] + t + 1, &s->h_anc[(long)r * T]);
        run.swap(nrun);
        cur_len++;
        for (int b = 0; b < B; ++b) {
            const float best_len = (o.early_stopping == 2 && o.length_penalty > 0.f) ? (float)(ML - 1) : (float)(cur_len - 1);
            const float best = nscore[b * R] / (float)pow((double)best_len, (double)o.length_penalty);
            float worst = INFINITY;
            for (int bb = 0; bb < R; ++bb) worst = std::min(worst, fin_score[b * R + bb]);
            bool anyb = false;
            for (int bb = 0; bb < R; ++bb) anyb |= best > (fin_done[b * R + bb] ? worst : -1.0e9f);
            unsat[b] = unsat[b] && anyb;
            any_unsat |= unsat[b] != 0;
            for (int bb = 0; bb < R; ++bb) all_fin &= fin_done[b * R + bb] != 0;
        }
        for (int r = 0; r < rows; ++r) run_score[r] = nscore[r];
        const bool open = !(all_fin && o.early_stopping == 1);
        if (!(any_unsat && open && !all_hit)) break;
        if (cur_len >= ML) break;
    }
    CK(hipEventRecord(s->ev[3], s->st));
    // outputs: generated tokens after the decoder start, the final EOS excluded
    for (int b = 0; b < B; ++b) {
        const int* seq;
        int len;
        float score;
        if (R == 1) { seq = &run[b * ML]; len = fin_len[b] ? fin_len[b] : cur_len; score = greedy_score[b]; }
        else { seq = &fin[b * R * ML]; len = fin_len[b * R]; score = fin_score[b * R]; }
        int n = std::max(0, len - 1);
        if (n > 0 && seq[len - 1] == eos) n--;
        n = std::min(n, tokens_stride);
        for (int j = 0; j < n; ++j) tokens_out[(long)b * tokens_stride + j] = seq[1 + j];
        n_out[b] = n;
        if (scores_out) scores_out[b] = score;
    }
    return WLX_OK;
}

// ---- the same generate with the search on the device (mt_search.hip): nothing is uploaded or downloaded per step. The host enqueues
// the iterations in blocks of `block` steps and, after each block, waits for an event and reads the pinned done word the search
// kernel stored behind the results. Iterations enqueued past the end find the group done: their decode steps compute on scratch (the logits,
// the caches at positions no later launch of this generate reads) and their search launches change nothing.
// The block length kept is 1, after measuring 1, 2, 4 and 8 on generates of 2-5 and of 31 steps (DESIGN.md §23,
// scripts/file_translate_time.py): a look at the done word costs ~4 us of a ~500 us step, a decode step enqueued past the end a whole
// step, so a block of B saves (1 - 1/B) x 0.8 % per step and wastes (B - 1) / 2 steps per group: B = 2 pays from ~125 steps on, B = 4
// from ~250. What the device search saves is the five uploads, the two downloads and the host bookkeeping of a step, not the wait.
constexpr int MT_STEP_BLOCK = 1;
int step_block_default() {
    static const int v = [] {
        const char* e = wlx_ab("WLX_MT_STEP_BLOCK");      // (another block length; read by libwlx_ab.so only: common.h)
        const int n = e ? atoi(e) : 0;
        return n >= 1 ? n : MT_STEP_BLOCK;
    }();
    return v;
}

// the search state of a slot for `rows` rows of `B` items (S.ban / S.nban are the slot's d_ban / d_nban). The buffers join the slot's
// free lists only when all of them exist: an allocation that fails midway frees what the call got, so a retry starts from nothing.
int search_alloc(MtSlot* s, int rows, int B) {
    if (s->has_search) return WLX_OK;
    std::vector<void*> A, H;
    MtSearchState S{};
    float *d_lp = nullptr, *h_lp = nullptr;
    hipEvent_t ev = nullptr;
    const size_t T = s->tmax;
    const int rc = [&]() -> int {
        for (int k = 0; k < 2; ++k) {
            CKR(dalloc(A, &S.run[k], rows * T, false));
            CKR(dalloc(A, &S.fin[k], rows * T, false));
            CKR(dalloc(A, &S.anc[k], rows * T, false));
        }
        CKR(dalloc(A, &S.run_score, rows, false));
        CKR(dalloc(A, &S.fin_score, rows, false));
        CKR(dalloc(A, &S.fin_len, rows, false));
        CKR(dalloc(A, &S.fin_done, rows, false));
        CKR(dalloc(A, &S.unsat, B, false));
        CKR(dalloc(A, &S.item_done, B, false));
        CKR(dalloc(A, &S.greedy_score, B, false));
        CKR(dalloc(A, &S.tok, rows, false));
        CKR(dalloc(A, &S.pos, rows, false));
        CKR(dalloc(A, &S.gself, rows, false));
        CKR(dalloc(A, &S.ctl, 8, true));
        CKR(dalloc(A, &d_lp, T + 1, false));
        CKR(halloc(H, &h_lp, T + 1));
        CKR(halloc(H, &S.h_done, 4));
        CKR(halloc(H, &S.h_n, B));
        CKR(halloc(H, &S.h_score, B));
        CKR(halloc(H, &S.h_tok, B * T));
        CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return WLX_OK;
    }();
    if (rc != WLX_OK) {
        for (void* p : A) (void)hipFree(p);
        for (void* p : H) (void)hipHostFree(p);
        return rc;
    }
    s->allocs.insert(s->allocs.end(), A.begin(), A.end());
    s->host_allocs.insert(s->host_allocs.end(), H.begin(), H.end());
    S.ban = s->d_ban;
    S.nban = s->d_nban;
    S.lp = d_lp;
    s->sd = S;
    s->d_lp = d_lp;
    s->h_lp = h_lp;
    s->ev_blk = ev;
    s->has_search = true;
    return WLX_OK;
}

// logits_of(i, &ptr): enqueue whatever produces the logits [rows][V] of iteration i on the slot's stream and point at them.
// Results: s->sd.h_tok [B][ML] / h_n / h_score, final when this returns. *steps_out: decode steps the search ran.
template <class LogitsFn>
int device_generate(MtSlot* s, const wlx_mt_spec& sp, const wlx_mt_gen_opts& o, int B, int block, int* steps_out, LogitsFn&& logits_of) {
    const int R = o.num_beams, rows = B * R, ML = o.max_length, K = R == 1 ? 1 : 2 * R;
    const bool forced = o.forced_eos_token_id >= 0;
    MtSearchParams P{};
    P.B = B; P.R = R; P.ML = ML; P.T = s->tmax; P.V = sp.vocab;
    P.eos = sp.eos_id; P.pad = sp.pad_id; P.start = sp.decoder_start_id; P.forced_eos = forced ? o.forced_eos_token_id : -1;
    P.nng = o.no_repeat_ngram_size; P.early_stopping = o.early_stopping; P.lp_positive = o.length_penalty > 0.f; P.ban_ld = s->ban_ld;
    const MtSearchState& S = s->sd;
    hipStream_t st = s->st;
    s->h_lp[0] = 1.f;
    for (int len = 1; len <= ML; ++len) s->h_lp[len] = (float)pow((double)len, (double)o.length_penalty);
    CK(hipMemcpyAsync(s->d_lp, s->h_lp, (ML + 1) * sizeof(float), hipMemcpyHostToDevice, st));
    volatile int* hd = S.h_done;
    hd[0] = 0; hd[1] = 0; hd[2] = 0;
    launch_mt_search_init(P, S, st);
    const bool bans = P.nng > 0;
    const int iters = ML - 1;
    for (int i = 0; i < iters; ++i) {
        const bool force_now = forced && i == ML - 2;
        if (!force_now) {
            if (bans) launch_mt_search_bans(P, S, i, st);
            const float* lg = nullptr;
            CKR(logits_of(i, &lg));
            launch_mt_topk(lg, rows, sp.vocab, bans ? S.ban : nullptr, bans ? S.nban : nullptr, s->ban_ld, K, s->tk_scratch, s->tk_cidx,
                           s->tk_val, s->tk_idx, st);
        }
        launch_mt_search_step(P, S, s->tk_val, s->tk_idx, i, force_now ? 1 : 0, st);
        if ((i + 1) % block == 0 || i == iters - 1) {
            CK(hipGetLastError());
            CK(hipEventRecord(s->ev_blk, st));
            CK(hipEventSynchronize(s->ev_blk));
            if (hd[0]) break;
        }
    }
    if (!hd[0]) return set_error(WLX_ERR_HIP, "the device search did not finish within max_length %d", ML);
    if (steps_out) *steps_out = hd[2];
    return WLX_OK;
}

int generate_on_device(wlx_mt* m, MtSlot* s, const wlx_mt_gen_opts& o, int block) {
    const int B = s->n_items, R = o.num_beams, rows = B * R;
    for (int i = 0; i < B; ++i) s->h_gcross[i] = MtAttnGroup{i * R, R, s->src_off[i], s->src_len[i]};
    CK(hipMemcpyAsync(s->d_gcross, s->h_gcross, B * sizeof(MtAttnGroup), hipMemcpyHostToDevice, s->st));
    CK(hipEventRecord(s->ev[2], s->st));
    int steps = 0;
    const MtSearchState& S = s->sd;
    CKR(device_generate(s, m->spec, o, B, block, &steps, [&](int i, const float** lg) -> int {
        *lg = s->logits;
        return decode_launch(m, s, rows, R, i, S.tok, S.pos, S.anc[i & 1], S.gself);
    }));
    CK(hipEventRecord(s->ev[3], s->st));
    s->steps += steps;
    return WLX_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int32_t wlx_mt_create(const wlx_mt_spec* spec, const wlx_tensor* w, int32_t n, int32_t device, wlx_mt** out) {
    if (!spec || !w || !out) return set_error(WLX_ERR_ARG, "null argument");
    *out = nullptr;
    const wlx_mt_spec sp = *spec;
    if (sp.d_model <= 0 || sp.d_model % 64 || sp.d_model > 2048 || sp.n_heads * 64 != sp.d_model)
        return set_error(WLX_ERR_ARG, "d_model %d / heads %d: head_dim must be 64 and d_model a multiple of 64 (<= 2048)", sp.d_model, sp.n_heads);
    if (sp.ffn <= 0 || sp.ffn % 64) return set_error(WLX_ERR_ARG, "ffn %d must be a positive multiple of 64", sp.ffn);
    if (sp.vocab <= 0 || sp.vocab % 16 || sp.vocab > WLX_MT_CHUNKS * 4096)
        return set_error(WLX_ERR_ARG, "vocab %d must be a multiple of 16 and <= %d", sp.vocab, WLX_MT_CHUNKS * 4096);
    if (sp.enc_layers < 1 || sp.dec_layers < 1 || sp.enc_layers > 64 || sp.dec_layers > 64) return set_error(WLX_ERR_ARG, "bad layer counts");
    if (sp.max_positions < 1 || sp.pad_id < 0 || sp.eos_id < 0 || sp.decoder_start_id < 0 || sp.pad_id >= sp.vocab ||
        sp.eos_id >= sp.vocab || sp.decoder_start_id >= sp.vocab)
        return set_error(WLX_ERR_ARG, "bad special ids / max_positions");
    CK(hipSetDevice(device));
    CK((hipError_t)gemm_prepare_device());
    wlx_mt* m = new wlx_mt();
    m->spec = sp;
    m->device = device;
    m->embed_scale = sp.scale_embedding ? sqrtf((float)sp.d_model) : 1.f;
    int rc = [&]() -> int {
        Weights ws;
        CKR(ws.open(w, n));
        std::vector<void*>& A = m->allocs;      // (none of this engine's allocations is zeroed: every element is written below)
        const int d = sp.d_model, F = sp.ffn, Ld = sp.dec_layers;
        int KT;
        CKR(alloc_packed(A, sp.vocab, d, &m->E, &KT, false));
        CKR(ws.pack("model.shared.weight", sp.vocab, d, m->E, KT, 0));
        // head_dim ** -0.5 is applied after the bias: folded into q_proj's weight and bias
        LayerOpts o{/*k_bias=*/true, /*q_scale=*/0.125f, /*zero=*/false};
        m->enc.resize(sp.enc_layers);
        for (int l = 0; l < sp.enc_layers; ++l)
            CKR(load_layer(ws, A, "model.encoder.layers." + std::to_string(l) + ".", d, F, o, m->enc[l]));
        CKR(ws.alloc_vec(A, "model.encoder.layer_norm.weight", d, &m->enc_ln_g, false));
        CKR(ws.alloc_vec(A, "model.encoder.layer_norm.bias", d, &m->enc_ln_b, false));
        CKR(alloc_packed(A, 2L * Ld * d, d, &m->Wckv, nullptr, false));
        CKR(dalloc(A, &m->bckv, (size_t)2 * Ld * d, false));
        o.Wckv = m->Wckv; o.bckv = m->bckv;
        m->dec.resize(Ld);
        for (o.l = 0; o.l < Ld; ++o.l)
            CKR(load_layer(ws, A, "model.decoder.layers." + std::to_string(o.l) + ".", d, F, o, m->dec[o.l]));
        CKR(ws.alloc_vec(A, "model.decoder.layer_norm.weight", d, &m->dec_ln_g, false));
        CKR(ws.alloc_vec(A, "model.decoder.layer_norm.bias", d, &m->dec_ln_b, false));
        // M2M100SinusoidalPositionalEmbedding.get_embedding, in fp32 as torch computes it
        const int npos = sp.max_positions + 2, half = d / 2;
        std::vector<float> sp_h((size_t)npos * d, 0.f);
        const float neg = (float)(-(log(10000.0) / (half - 1)));
        for (int p = 0; p < npos; ++p) {
            if (p == sp.pad_id) continue;
            for (int i = 0; i < half; ++i) {
                const float a = (float)p * expf((float)i * neg);
                sp_h[(size_t)p * d + i] = sinf(a);
                sp_h[(size_t)p * d + half + i] = cosf(a);
            }
        }
        CKR(dalloc(A, &m->sinpos, sp_h.size(), false));
        CK(hipMemcpyAsync(m->sinpos, sp_h.data(), sp_h.size() * sizeof(float), hipMemcpyHostToDevice, ws.st));
        return ws.finish();
    }();
    if (rc != WLX_OK) {
        for (void* p : m->allocs) (void)hipFree(p);
        delete m;
        return rc;
    }
    *out = m;
    return WLX_OK;
}

static void slot_free(MtSlot* s) {
    if (s->st) (void)hipStreamSynchronize(s->st);
    for (void* p : s->allocs) (void)hipFree(p);
    for (void* p : s->host_allocs) (void)hipHostFree(p);
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    if (s->ev_blk) (void)hipEventDestroy(s->ev_blk);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

extern "C" void wlx_mt_destroy(wlx_mt* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    for (auto& kv : m->slots) slot_free(kv.second);
    for (void* p : m->allocs) (void)hipFree(p);
    delete m;
}

extern "C" int32_t wlx_mt_slot_create(wlx_mt* m, int32_t max_batch, int32_t max_rows_per_item, int32_t max_src, int32_t* slot_out) {
    if (!m || !slot_out) return set_error(WLX_ERR_ARG, "null argument");
    const wlx_mt_spec& sp = m->spec;
    if (max_batch < 1 || max_batch > 64) return set_error(WLX_ERR_ARG, "max_batch %d outside 1..64", max_batch);
    if (max_rows_per_item < 1 || max_rows_per_item > 16) return set_error(WLX_ERR_ARG, "max_rows_per_item %d outside 1..16", max_rows_per_item);
    if (max_src < 1 || max_src > WLX_MT_MAX_SRC || max_src > sp.max_positions)
        return set_error(WLX_ERR_ARG, "max_src %d outside 1..%d", max_src, std::min(WLX_MT_MAX_SRC, sp.max_positions));
    CK(hipSetDevice(m->device));
    const int d = sp.d_model, F = sp.ffn, Ld = sp.dec_layers, B = max_batch, R = max_rows_per_item, T = WLX_T_TEXT;
    const long rows = (long)B * R, src = (long)B * max_src;
    const int ban_ld = T;
    const double bytes = (double)src * (d * (4.0 + 4.0 + 2 + 6 + 2) + F * 2.0 + 4.0 * d * Ld) +
                         (double)rows * (d * (4.0 + 2 + 6 + 2 + 2) + F * 2.0 + sp.vocab * 4.0 + 4.0 * Ld * T * d + T * 4.0 + ban_ld * 4.0) +
                         (double)rows * WLX_MT_CHUNKS * WLX_MT_MAXK * 12.0;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (bytes > (double)free_b)
                return set_error(WLX_ERR_NOMEM, "a translation slot of %d items x %d rows x %d source tokens needs ~%.2f GB of device memory; %.2f GB are free on device %d",
                                 B, R, max_src, bytes / 1e9, free_b / 1e9, m->device);
        } else (void)hipGetLastError();
    }
    MtSlot* s = new MtSlot();
    s->B = B; s->R = R; s->max_src = max_src; s->rows_cap = (int)rows; s->src_cap = (int)src; s->ban_ld = ban_ld;
    int rc = [&]() -> int {
        CK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
        for (auto& e : s->ev) CK(hipEventCreate(&e));
        auto& A = s->allocs;      // (not zeroed: the K / V caches alone are L x rows x 448 x d halfs)
        CKR(dalloc(A, &s->xe, src * d, false));
        CKR(dalloc(A, &s->enc32, src * d, false));
        CKR(dalloc(A, &s->he, src * d, false));
        CKR(dalloc(A, &s->qkve, src * 3 * d, false));
        CKR(dalloc(A, &s->atte, src * d, false));
        CKR(dalloc(A, &s->ffe, src * F, false));
        CKR(dalloc(A, &s->ckv, src * 2 * d * Ld, false));
        CKR(dalloc(A, &s->xd, rows * d, false));
        CKR(dalloc(A, &s->hd, rows * d, false));
        CKR(dalloc(A, &s->qkvd, rows * 3 * d, false));
        CKR(dalloc(A, &s->qd, rows * d, false));
        CKR(dalloc(A, &s->attd, rows * d, false));
        CKR(dalloc(A, &s->ffd, rows * F, false));
        CKR(dalloc(A, &s->kc, (size_t)Ld * rows * T * d, false));
        CKR(dalloc(A, &s->vc, (size_t)Ld * rows * T * d, false));
        CKR(dalloc(A, &s->logits, rows * sp.vocab, false));
        CKR(dalloc(A, &s->tk_scratch, rows * WLX_MT_CHUNKS * (2 + WLX_MT_MAXK), false));
        CKR(dalloc(A, &s->tk_cidx, rows * WLX_MT_CHUNKS * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->tk_val, rows * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->tk_idx, rows * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->d_tok, rows, false));
        CKR(dalloc(A, &s->d_pos, rows, false));
        CKR(dalloc(A, &s->d_src_tok, src, false));
        CKR(dalloc(A, &s->d_src_pos, src, false));
        CKR(dalloc(A, &s->d_anc, rows * T, false));
        CKR(dalloc(A, &s->d_ban, rows * ban_ld, false));
        CKR(dalloc(A, &s->d_nban, rows, false));
        CKR(dalloc(A, &s->d_genc, src, false));
        CKR(dalloc(A, &s->d_gself, rows, false));
        CKR(dalloc(A, &s->d_gcross, B, false));
        auto& H = s->host_allocs;
        CKR(halloc(H, &s->h_tok, rows));
        CKR(halloc(H, &s->h_pos, rows));
        CKR(halloc(H, &s->h_src_tok, src));
        CKR(halloc(H, &s->h_src_pos, src));
        CKR(halloc(H, &s->h_anc, rows * T));
        CKR(halloc(H, &s->h_ban, rows * ban_ld));
        CKR(halloc(H, &s->h_nban, rows));
        CKR(halloc(H, &s->h_tk_idx, rows * WLX_MT_MAXK));
        CKR(halloc(H, &s->h_tk_val, rows * WLX_MT_MAXK));
        CKR(halloc(H, &s->h_genc, src));
        CKR(halloc(H, &s->h_gself, rows));
        CKR(halloc(H, &s->h_gcross, B));
        return WLX_OK;
    }();
    if (rc != WLX_OK) {
        slot_free(s);
        return rc;
    }
    std::lock_guard<std::mutex> g(m->mu);
    const int id = m->next_slot++;
    m->slots[id] = s;
    *slot_out = id;
    return WLX_OK;
}

extern "C" int32_t wlx_mt_slot_destroy(wlx_mt* m, int32_t slot) {
    if (!m) return set_error(WLX_ERR_ARG, "null engine");
    MtSlot* s = nullptr;
    {
        std::lock_guard<std::mutex> g(m->mu);
        auto it = m->slots.find(slot);
        if (it == m->slots.end()) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
        s = it->second;
        bool f = false;
        if (!s->busy.compare_exchange_strong(f, true)) return set_error(WLX_ERR_STATE, "translation slot %d is busy", slot);
        m->slots.erase(it);
    }
    (void)hipSetDevice(m->device);
    slot_free(s);
    return WLX_OK;
}

static int check_opts(const wlx_mt* m, const MtSlot* s, const wlx_mt_gen_opts* o) {
    if (!o) return set_error(WLX_ERR_ARG, "null options");
    if (o->num_beams < 1 || o->num_beams > s->R) return set_error(WLX_ERR_ARG, "num_beams %d outside 1..%d (slot max_rows_per_item)", o->num_beams, s->R);
    if (2 * o->num_beams > WLX_MT_MAXK && o->num_beams > 1) return set_error(WLX_ERR_ARG, "num_beams %d > %d", o->num_beams, WLX_MT_MAXK / 2);
    const int ml_cap = std::min(WLX_T_TEXT, m->spec.max_positions);
    if (o->max_length < 2 || o->max_length > ml_cap) return set_error(WLX_ERR_ARG, "max_length %d outside 2..%d", o->max_length, ml_cap);
    if (o->early_stopping < 0 || o->early_stopping > 2) return set_error(WLX_ERR_ARG, "early_stopping must be 0 (False), 1 (True) or 2 (never)");
    if (o->no_repeat_ngram_size < 0) return set_error(WLX_ERR_ARG, "no_repeat_ngram_size < 0");
    if (o->forced_eos_token_id >= m->spec.vocab) return set_error(WLX_ERR_ARG, "forced_eos_token_id outside the vocabulary");
    return WLX_OK;
}

extern "C" int32_t wlx_mt_translate(wlx_mt* m, int32_t slot, int32_t batch, const int32_t* src_ids, const int32_t* src_lens,
                                    int32_t src_stride, const wlx_mt_gen_opts* opts, int32_t* tokens_out, int32_t tokens_stride,
                                    int32_t* n_tokens_out, float* scores_out) {
    if (!m || !tokens_out || !n_tokens_out || tokens_stride < 1) return set_error(WLX_ERR_ARG, "null argument");
    MtSlot* s = slot_of(m, slot);
    if (!s) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
    Busy busy(s);
    if (!busy.ok) return set_error(WLX_ERR_STATE, "translation slot %d is busy (a call is in flight)", slot);
    CKR(check_opts(m, s, opts));
    CK(hipSetDevice(m->device));
    CKR(encode(m, s, batch, src_ids, src_lens, src_stride));
    CKR(run_generate(m, s, *opts, tokens_out, tokens_stride, n_tokens_out, scores_out));
    CK(hipStreamSynchronize(s->st));
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, s->ev[0], s->ev[1]) == hipSuccess) s->enc_ms = a;
    if (hipEventElapsedTime(&b, s->ev[2], s->ev[3]) == hipSuccess) s->dec_ms = b;
    (void)hipGetLastError();
    return WLX_OK;
}

extern "C" int32_t wlx_mt_translate_many(wlx_mt* m, int32_t slot, int32_t n, const int32_t* src_ids, const int32_t* src_lens,
                                         int32_t src_stride, const wlx_mt_gen_opts* opts, int32_t* tokens_out, int32_t tokens_stride,
                                         int32_t* n_tokens_out, float* scores_out) {
    if (!m || !src_ids || !src_lens || !tokens_out || !n_tokens_out || tokens_stride < 1 || src_stride < 1)
        return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_MT_MANY_MAX) return set_error(WLX_ERR_ARG, "n %d outside 1..%d", n, WLX_MT_MANY_MAX);
    MtSlot* s = slot_of(m, slot);
    if (!s) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
    Busy busy(s);
    if (!busy.ok) return set_error(WLX_ERR_STATE, "translation slot %d is busy (a call is in flight)", slot);
    CKR(check_opts(m, s, opts));
    for (int i = 0; i < n; ++i) {       // everything encode() would refuse, before the first group is launched
        const int S = src_lens[i];
        if (S < 1 || S > s->max_src || S > src_stride)
            return set_error(WLX_ERR_ARG, "source %d: length %d outside 1..%d", i, S, std::min(s->max_src, (int)src_stride));
        for (int j = 0; j < S; ++j) {
            const int tok = src_ids[(long)i * src_stride + j];
            if (tok < 0 || tok >= m->spec.vocab) return set_error(WLX_ERR_ARG, "source %d: token %d outside the vocabulary", i, tok);
        }
    }
    CK(hipSetDevice(m->device));
    CKR(search_alloc(s, s->rows_cap, s->B));
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int z) { return src_lens[a] < src_lens[z]; });
    const int ML = opts->max_length, block = step_block_default();
    std::vector<int32_t> ids, lens;
    s->steps = 0;
    for (int g0 = 0; g0 < n;) {
        // a group: the next sources in length order, at most max_batch of them and no more tokens than the slot's source buffers hold
        int g1 = g0, ntok = 0, stride = 0;
        while (g1 < n && g1 - g0 < s->B && ntok + src_lens[order[g1]] <= s->src_cap) {
            ntok += src_lens[order[g1]];
            stride = std::max(stride, (int)src_lens[order[g1]]);
            ++g1;
        }
        const int B = g1 - g0;
        ids.assign((size_t)B * stride, 0);
        lens.resize(B);
        for (int k = 0; k < B; ++k) {
            const int i = order[g0 + k];
            lens[k] = src_lens[i];
            std::copy(src_ids + (long)i * src_stride, src_ids + (long)i * src_stride + lens[k], ids.begin() + (size_t)k * stride);
        }
        CKR(encode(m, s, B, ids.data(), lens.data(), stride));
        CKR(generate_on_device(m, s, *opts, block));
        const MtSearchState& S = s->sd;
        for (int k = 0; k < B; ++k) {
            const int i = order[g0 + k];
            const int cnt = std::min(S.h_n[k], (int)tokens_stride);
            for (int j = 0; j < cnt; ++j) tokens_out[(long)i * tokens_stride + j] = S.h_tok[(long)k * ML + j];
            n_tokens_out[i] = cnt;
            if (scores_out) scores_out[i] = S.h_score[k];
        }
        g0 = g1;
    }
    CK(hipStreamSynchronize(s->st));      // (the iterations enqueued past the end of the last group)
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, s->ev[0], s->ev[1]) == hipSuccess) s->enc_ms = a;
    if (hipEventElapsedTime(&b, s->ev[2], s->ev[3]) == hipSuccess) s->dec_ms = b;
    (void)hipGetLastError();
    return WLX_OK;
}

// ---- test / profiling hooks
extern "C" int32_t wlx_mt_debug_search(int32_t device, const float* logits, int32_t steps, int32_t batch, const wlx_mt_gen_opts* opts,
                                       int32_t vocab, int32_t pad_id, int32_t eos_id, int32_t start_id, int32_t ban_ld,
                                       int32_t step_block, int32_t use_device, int32_t* tokens_out, int32_t tokens_stride,
                                       int32_t* n_tokens_out, float* scores_out, int32_t* steps_run_out) {
    if (!logits || !opts || !tokens_out || !n_tokens_out || tokens_stride < 1) return set_error(WLX_ERR_ARG, "null argument");
    if (batch < 1 || batch > 64) return set_error(WLX_ERR_ARG, "batch %d outside 1..64", batch);
    if (vocab < 2 || vocab > WLX_MT_CHUNKS * 4096) return set_error(WLX_ERR_ARG, "vocab %d outside 2..%d", vocab, WLX_MT_CHUNKS * 4096);
    if (pad_id < 0 || pad_id >= vocab || eos_id < 0 || eos_id >= vocab || start_id < 0 || start_id >= vocab)
        return set_error(WLX_ERR_ARG, "special ids outside the vocabulary");
    if (ban_ld < 1 || ban_ld > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "ban_ld %d outside 1..%d", ban_ld, WLX_T_TEXT);
    if (step_block < 0) return set_error(WLX_ERR_ARG, "step_block < 0");
    wlx_mt fm;
    fm.spec.vocab = vocab; fm.spec.pad_id = pad_id; fm.spec.eos_id = eos_id; fm.spec.decoder_start_id = start_id;
    fm.spec.max_positions = WLX_T_TEXT;
    MtSlot* s = new MtSlot();
    s->B = batch; s->R = 16; s->ban_ld = ban_ld; s->n_items = batch;
    int rc = [&]() -> int {
        CKR(check_opts(&fm, s, opts));
        const int R = opts->num_beams, rows = batch * R, V = vocab, T = s->tmax;
        const int need = opts->max_length - 1 - (opts->forced_eos_token_id >= 0 ? 1 : 0);
        if (steps < 1 || steps < need) return set_error(WLX_ERR_ARG, "%d steps of logits, max_length %d may take %d", steps, opts->max_length, need);
        int ndev = 0;
        CK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return set_error(WLX_ERR_ARG, "device %d outside 0..%d", device, ndev - 1);
        CK(hipSetDevice(device));
        CK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
        for (auto& e : s->ev) CK(hipEventCreate(&e));
        s->rows_cap = rows;
        auto& A = s->allocs;
        auto& H = s->host_allocs;
        CKR(dalloc(A, &s->logits, (size_t)rows * V, false));
        CKR(dalloc(A, &s->tk_scratch, (size_t)rows * WLX_MT_CHUNKS * (2 + WLX_MT_MAXK), false));
        CKR(dalloc(A, &s->tk_cidx, (size_t)rows * WLX_MT_CHUNKS * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->tk_val, (size_t)rows * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->tk_idx, (size_t)rows * WLX_MT_MAXK, false));
        CKR(dalloc(A, &s->d_ban, (size_t)rows * ban_ld, false));
        CKR(dalloc(A, &s->d_nban, rows, false));
        if (!use_device) {
            CKR(halloc(H, &s->h_tok, rows));
            CKR(halloc(H, &s->h_pos, rows));
            CKR(halloc(H, &s->h_anc, (size_t)rows * T));
            CKR(halloc(H, &s->h_ban, (size_t)rows * ban_ld));
            CKR(halloc(H, &s->h_nban, rows));
            CKR(halloc(H, &s->h_tk_idx, (size_t)rows * WLX_MT_MAXK));
            CKR(halloc(H, &s->h_tk_val, (size_t)rows * WLX_MT_MAXK));
            s->inject = logits;
            CKR(run_generate(&fm, s, *opts, tokens_out, tokens_stride, n_tokens_out, scores_out));
            CK(hipStreamSynchronize(s->st));
            if (steps_run_out) *steps_run_out = s->steps;
            return WLX_OK;
        }
        CKR(search_alloc(s, rows, batch));
        float* dl = nullptr;
        const size_t per = (size_t)rows * V;
        CKR(dalloc(A, &dl, per * steps, false));
        CK(hipMemcpyAsync(dl, logits, per * steps * sizeof(float), hipMemcpyHostToDevice, s->st));
        int ran = 0;
        CKR(device_generate(s, fm.spec, *opts, batch, step_block > 0 ? step_block : step_block_default(), &ran,
                            [&](int i, const float** lg) -> int { *lg = dl + per * i; return WLX_OK; }));
        CK(hipStreamSynchronize(s->st));
        const MtSearchState& S = s->sd;
        for (int b = 0; b < batch; ++b) {
            const int cnt = std::min(S.h_n[b], (int)tokens_stride);
            for (int j = 0; j < cnt; ++j) tokens_out[(long)b * tokens_stride + j] = S.h_tok[(long)b * opts->max_length + j];
            n_tokens_out[b] = cnt;
            if (scores_out) scores_out[b] = S.h_score[b];
        }
        if (steps_run_out) *steps_run_out = ran;
        return WLX_OK;
    }();
    slot_free(s);
    return rc;
}

extern "C" int32_t wlx_mt_debug_encode(wlx_mt* m, int32_t slot, int32_t batch, const int32_t* src_ids, const int32_t* src_lens,
                                       int32_t src_stride, float* out, int64_t cap_floats) {
    if (!m || !out) return set_error(WLX_ERR_ARG, "null argument");
    MtSlot* s = slot_of(m, slot);
    if (!s) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
    Busy busy(s);
    if (!busy.ok) return set_error(WLX_ERR_STATE, "translation slot %d is busy", slot);
    CK(hipSetDevice(m->device));
    CKR(encode(m, s, batch, src_ids, src_lens, src_stride));
    const long need = (long)s->n_src * m->spec.d_model;
    if (cap_floats < need) return set_error(WLX_ERR_ARG, "output holds %lld floats, %ld needed", (long long)cap_floats, need);
    CK(hipMemcpyAsync(out, s->enc32, need * sizeof(float), hipMemcpyDeviceToHost, s->st));
    CK(hipStreamSynchronize(s->st));
    return WLX_OK;
}

extern "C" int32_t wlx_mt_debug_decode_logits(wlx_mt* m, int32_t slot, const int32_t* src_ids, int32_t src_len,
                                              const int32_t* dec_tokens, int32_t n, float* out) {
    if (!m || !out || !dec_tokens) return set_error(WLX_ERR_ARG, "null argument");
    MtSlot* s = slot_of(m, slot);
    if (!s) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
    Busy busy(s);
    if (!busy.ok) return set_error(WLX_ERR_STATE, "translation slot %d is busy", slot);
    if (n < 1 || n > s->tmax) return set_error(WLX_ERR_ARG, "n %d outside 1..%d", n, s->tmax);
    CK(hipSetDevice(m->device));
    CKR(encode(m, s, 1, src_ids, &src_len, src_len));
    const int V = m->spec.vocab;
    int c = 0;
    for (int j = 0; j < s->tmax; ++j) s->h_anc[j] = 0;
    for (int t = 0; t < n; ++t) {
        const int tok = dec_tokens[t];
        if (tok < 0 || tok >= V) return set_error(WLX_ERR_ARG, "token %d outside the vocabulary", tok);
        c += tok != m->spec.pad_id;
        s->h_tok[0] = tok;
        s->h_pos[0] = position_of(tok, c, 0, m->spec.pad_id);
        CKR(decode_step(m, s, 1, 1, t));
        CK(hipMemcpyAsync(out + (long)t * V, s->logits, V * sizeof(float), hipMemcpyDeviceToHost, s->st));
        CK(hipStreamSynchronize(s->st));     // (h_tok / h_pos are rewritten by the next step)
    }
    return WLX_OK;
}

extern "C" int32_t wlx_mt_debug_timings(wlx_mt* m, int32_t slot, float* encode_ms, float* decode_ms, int32_t* steps) {
    if (!m) return set_error(WLX_ERR_ARG, "null engine");
    MtSlot* s = slot_of(m, slot);
    if (!s) return set_error(WLX_ERR_ARG, "no translation slot %d", slot);
    if (encode_ms) *encode_ms = s->enc_ms;
    if (decode_ms) *decode_ms = s->dec_ms;
    if (steps) *steps = s->steps;
    return WLX_OK;
}

// ---- kernel-level test hooks (host.h HookScope): host arrays in, the production launcher unchanged on a private stream, host arrays out
extern "C" int32_t wlx_mt_debug_attn(int32_t device, const uint16_t* q, int64_t ldq, int64_t q_rows, const uint16_t* k, int64_t ldk,
                                     const uint16_t* v, int64_t ldv, int64_t kv_rows, const int32_t* groups, int32_t n_groups,
                                     int32_t max_nq, int32_t heads, const int32_t* anc, int32_t ld_anc, int32_t tmax, uint16_t* o,
                                     int64_t ldo, int64_t o_rows) {
    if (!q || !k || !v || !o || !groups) return set_error(WLX_ERR_ARG, "null argument");
    if (n_groups < 1 || heads < 1 || heads > 65535) return set_error(WLX_ERR_ARG, "n_groups %d / heads %d", n_groups, heads);
    if (max_nq < 1 || max_nq > 16) return set_error(WLX_ERR_ARG, "max_nq %d outside 1..16", max_nq);   // (4 waves x 4 rows)
    const int64_t w = 64L * heads;
    if (ldq < w || ldk < w || ldv < w || ldo < w || ldk % 8 || ldv % 8)
        return set_error(WLX_ERR_ARG, "row strides must cover heads * 64 columns (K / V strides: multiples of 8)");
    if (q_rows < 1 || kv_rows < 1 || o_rows < 1) return set_error(WLX_ERR_ARG, "empty Q / K / V / O");
    if (anc && (tmax < 1 || ld_anc < 1)) return set_error(WLX_ERR_ARG, "ancestry table with tmax %d / ld_anc %d", tmax, ld_anc);
    int64_t anc_rows = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int32_t q0 = groups[4 * g], nq = groups[4 * g + 1], k0 = groups[4 * g + 2], nk = groups[4 * g + 3];
        if (nq < 1 || nq > max_nq) return set_error(WLX_ERR_ARG, "group %d: nq %d outside 1..max_nq %d", g, nq, max_nq);
        if (q0 < 0 || (int64_t)q0 + nq > q_rows || (int64_t)q0 + nq > o_rows) return set_error(WLX_ERR_ARG, "group %d: query rows outside Q / O", g);
        if (nk < 1) return set_error(WLX_ERR_ARG, "group %d: nk %d < 1", g, nk);
        if (!anc) {
            if (k0 < 0 || (int64_t)k0 + nk > kv_rows) return set_error(WLX_ERR_ARG, "group %d: key rows [%d, %lld) outside K / V", g, k0, (long long)k0 + nk);
            continue;
        }
        if (nk > ld_anc || nk > tmax) return set_error(WLX_ERR_ARG, "group %d: nk %d exceeds ld_anc %d / tmax %d", g, nk, ld_anc, tmax);
        for (int j = 0; j < nk; ++j) {      // key j of the group: row anc[q0][j] * tmax + j
            const int64_t a = anc[(int64_t)q0 * ld_anc + j];
            if (a < 0 || a * tmax + j >= kv_rows) return set_error(WLX_ERR_ARG, "group %d: ancestry row %lld of key %d outside K / V", g, (long long)a, j);
        }
        anc_rows = std::max<int64_t>(anc_rows, (int64_t)q0 + 1);
    }
    HookScope S;
    CKR(S.begin(device));
    half_t *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    int32_t *dg = nullptr, *da = nullptr;
    CKR(S.upload(&dq, h16(q), (size_t)q_rows * ldq));
    CKR(S.upload(&dk, h16(k), (size_t)kv_rows * ldk));
    CKR(S.upload(&dv, h16(v), (size_t)kv_rows * ldv));
    CKR(S.upload(&dout, h16(o), (size_t)o_rows * ldo));
    CKR(S.upload(&dg, groups, (size_t)4 * n_groups));
    if (anc) CKR(S.upload(&da, anc, (size_t)anc_rows * ld_anc));
    static_assert(sizeof(MtAttnGroup) == 4 * sizeof(int32_t), "MtAttnGroup is four int32");
    launch_mt_attn(dq, ldq, dk, ldk, dv, ldv, dout, ldo, reinterpret_cast<const MtAttnGroup*>(dg), n_groups, max_nq, heads, da,
                   anc ? ld_anc : 0, anc ? tmax : 0, S.st);
    CKR(S.download(h16(o), dout, (size_t)o_rows * ldo));
    return S.finish();
}

extern "C" int32_t wlx_mt_debug_topk(int32_t device, const float* logits, int32_t rows, int32_t vocab, const int32_t* ban,
                                     const int32_t* nban, int32_t ban_ld, int32_t k, float* out_val, int32_t* out_idx) {
    if (!logits || !out_val || !out_idx) return set_error(WLX_ERR_ARG, "null argument");
    if (rows < 1 || rows > 65535) return set_error(WLX_ERR_ARG, "rows %d outside 1..65535", rows);
    if (k < 1 || k > WLX_MT_MAXK) return set_error(WLX_ERR_ARG, "k %d outside 1..%d", k, WLX_MT_MAXK);
    if (vocab < 16 || vocab % 16 || vocab > WLX_MT_CHUNKS * 4096)      // (the chunk kernel holds 4096 logits in LDS)
        return set_error(WLX_ERR_ARG, "vocab %d must be a multiple of 16 in 16..%d", vocab, WLX_MT_CHUNKS * 4096);
    int max_nb = 0;
    if (nban) {
        for (int r = 0; r < rows; ++r) {
            if (nban[r] < 0) return set_error(WLX_ERR_ARG, "row %d: nban %d < 0", r, nban[r]);
            max_nb = std::max(max_nb, nban[r]);
        }
        if (max_nb > 0 && (!ban || ban_ld < max_nb)) return set_error(WLX_ERR_ARG, "ban table missing or ban_ld %d < %d", ban_ld, max_nb);
    }
    HookScope S;
    CKR(S.begin(device));
    float *dl = nullptr, *scratch = nullptr, *dval = nullptr;
    int32_t *dban = nullptr, *dnban = nullptr, *cidx = nullptr, *didx = nullptr;
    CKR(S.upload(&dl, logits, (size_t)rows * vocab));
    if (nban) {
        CKR(S.upload(&dnban, nban, (size_t)rows));
        CKR(S.upload(&dban, max_nb > 0 ? ban : nullptr, max_nb > 0 ? (size_t)rows * ban_ld : 0));
    }
    CKR(S.alloc(&scratch, (size_t)rows * WLX_MT_CHUNKS * (2 + k)));
    CKR(S.alloc(&cidx, (size_t)rows * WLX_MT_CHUNKS * k));
    CKR(S.alloc(&dval, (size_t)rows * k));
    CKR(S.alloc(&didx, (size_t)rows * k));
    launch_mt_topk(dl, rows, vocab, dban, dnban, nban ? ban_ld : 0, k, scratch, cidx, dval, didx, S.st);
    CKR(S.download(out_val, dval, (size_t)rows * k));
    CKR(S.download(out_idx, didx, (size_t)rows * k));
    return S.finish();
}

extern "C" int32_t wlx_mt_debug_embed(int32_t device, const float* E, int32_t vocab, int32_t d, const int32_t* tok,
                                      const int32_t* pos, int32_t rows, float scale, const float* sinpos, int32_t n_pos, float* x) {
    if (!E || !tok || !pos || !sinpos || !x) return set_error(WLX_ERR_ARG, "null argument");
    if (vocab < 1 || d < 32 || d % 32 || rows < 1 || rows > 65535 || n_pos < 1)
        return set_error(WLX_ERR_ARG, "vocab %d / d %d (a multiple of 32) / rows %d / n_pos %d", vocab, d, rows, n_pos);
    for (int r = 0; r < rows; ++r)
        if (tok[r] < 0 || tok[r] >= vocab || pos[r] < 0 || pos[r] >= n_pos)
            return set_error(WLX_ERR_ARG, "row %d: token %d / position %d outside the tables", r, tok[r], pos[r]);
    HookScope S;
    CKR(S.begin(device));
    float *dE = nullptr, *dsin = nullptr, *dx = nullptr;
    half_t* Ep = nullptr;
    int32_t *dtok = nullptr, *dpos = nullptr;
    CKR(S.upload(&dE, E, (size_t)vocab * d));
    CKR(alloc_packed(S.allocs, vocab, d, &Ep, nullptr, false));
    launch_pack_linear(dE, vocab, d, d, Ep, d / 32, 0, S.st);      // as wlx_mt_create packs model.shared.weight
    CKR(S.upload(&dtok, tok, (size_t)rows));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&dsin, sinpos, (size_t)n_pos * d));
    CKR(S.alloc(&dx, (size_t)rows * d));
    launch_mt_embed(dtok, dpos, rows, Ep, d / 32, scale, dsin, d, dx, S.st);
    CKR(S.download(x, dx, (size_t)rows * d));
    return S.finish();
}

// the decoder self-attention cache append of one step: rows r < `rows` of the fused qkv buffer into slot t of cache row r
extern "C" int32_t wlx_mt_debug_kv_append(int32_t device, const uint16_t* qkv, int64_t ldqkv, int32_t rows, int32_t d, uint16_t* Kc,
                                          uint16_t* Vc, int32_t cache_rows, int32_t tmax, int32_t t) {
    if (!qkv || !Kc || !Vc) return set_error(WLX_ERR_ARG, "null argument");
    if (d < 8 || d % 8 || d > (1 << 16) || ldqkv < 3 * (int64_t)d || ldqkv % 8 || ldqkv > (1 << 20))
        return set_error(WLX_ERR_ARG, "d %d / ldqkv %lld: d a multiple of 8 up to 2^16, ldqkv a multiple of 8 in 3 d .. 2^20", d, (long long)ldqkv);
    if (rows < 1 || rows > cache_rows || cache_rows > 65535 || tmax < 1 || t < 0 || t >= tmax || (int64_t)cache_rows * tmax * d > (1LL << 28))
        return set_error(WLX_ERR_ARG, "rows %d / cache_rows %d / tmax %d / t %d: 1 <= rows <= cache_rows <= 65535, 0 <= t < tmax, the cache up to 2^28 halfs",
                         rows, cache_rows, tmax, t);
    const size_t n_cache = (size_t)cache_rows * tmax * d;
    HookScope S;
    CKR(S.begin(device));
    half_t *dq, *dK, *dV;
    CKR(S.upload(&dq, h16(qkv), (size_t)rows * ldqkv));
    CKR(S.upload(&dK, h16(Kc), n_cache));
    CKR(S.upload(&dV, h16(Vc), n_cache));
    launch_mt_kv_append(dq, (long)ldqkv, rows, d, dK, dV, tmax, t, S.st);
    CKR(S.download(h16(Kc), dK, n_cache));
    CKR(S.download(h16(Vc), dV, n_cache));
    return S.finish();
}

// the in-place ReLU of the MLP on columns 0 .. N of M rows of stride ld
extern "C" int32_t wlx_mt_debug_relu(int32_t device, uint16_t* y, int64_t ld, int32_t M, int32_t N) {
    if (!y) return set_error(WLX_ERR_ARG, "null argument");
    if (M < 1 || N < 8 || N % 8 || ld < N || ld % 8 || (int64_t)M * ld > (1LL << 28))
        return set_error(WLX_ERR_ARG, "M %d / N %d / ld %lld: M >= 1, N and ld multiples of 8, ld >= N, M ld up to 2^28", M, N, (long long)ld);
    HookScope S;
    CKR(S.begin(device));
    half_t* dy;
    CKR(S.upload(&dy, h16(y), (size_t)M * ld));
    launch_mt_relu_f16(dy, (long)ld, M, N, S.st);
    CKR(S.download(h16(y), dy, (size_t)M * ld));
    return S.finish();
}
