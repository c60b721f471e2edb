// kernel_hooks.hip — kernel-level test hooks of the Whisper kernels (include/wlx.h, below the TEST / PROFILING line):
//   wlx_debug_layernorm          launch_layernorm_f16 / _f16_f32 (gemm.hip)
//   wlx_debug_attn_encoder       launch_attn_encoder (attention.hip)
//   wlx_debug_dec_cross_attn     launch_dec_cross_attn + launch_dec_xattn_combine (+ launch_dec_align_scores) (decoder.hip)
//   wlx_debug_dec_self_attn      launch_dec_self_attn (decoder.hip)
//   wlx_debug_gemm               launch_gemm / launch_gemm_form, weights packed by pack.hip (gemm.hip)
//   wlx_debug_dec_gemv           launch_dec_gemv: dec_gemv2_kernel, dec_vocab_kernel, dec_gemv_kernel (dec_gemv.hip, dec_vocab.hip)
//   wlx_debug_dec_cq_cross_attn  launch_dec_cq_cross_attn (decoder.hip)
//   wlx_debug_dtw, wlx_debug_align_post   launch_align_dtw / launch_align_cost (align.hip)
//   wlx_debug_bias_apply         launch_dec_bias (dec_bias.hip)
//   wlx_debug_bias_apply_items   launch_dec_bias_items (dec_bias.hip)
//   wlx_debug_grammar_apply      launch_dec_grammar (dec_grammar.hip)
//   wlx_debug_token_prob, _token_prob_rows, _lang_probs   launch_token_prob / _token_prob_rows / launch_lang_probs (search.hip)
//   wlx_debug_dec_embed          launch_dec_embed (decoder.hip)
//   wlx_debug_prep_windows       launch_prep_windows (logmel.hip)
//   wlx_debug_f32_to_f16         launch_f32_to_f16 (pack.hip)
// The hooks' conventions are HookScope's (host.h). No engine or slot is needed, and no product code path runs differently because
// these exist.
#include "align.h"
#include "decoder.h"
#include "grammar_table.h"
#include "host.h"

using namespace wlx;

extern "C" int32_t wlx_debug_layernorm(int32_t device, const float* x, int64_t ldx, const float* gamma, const float* beta, int32_t M,
                                       int32_t d, uint16_t* out16, float* out32, int64_t ldo) {
    if (!x || !gamma || !beta || !out16) return set_error(WLX_ERR_ARG, "null argument");
    // layernorm_kernel holds a row in float4 v[8] per lane (64 lanes x 8 x 4 = 2048 columns) and moves float4 / f16x4
    if (d < 4 || d % 4 || d > 2048) return set_error(WLX_ERR_ARG, "d %d must be a multiple of 4 in 4..2048", d);
    if (M < 1 || M > (1 << 24)) return set_error(WLX_ERR_ARG, "M %d outside 1..2^24", M);
    if (ldx < d || ldo < d || ldx % 4 || ldo % 4)
        return set_error(WLX_ERR_ARG, "row strides %lld / %lld must cover d and be multiples of 4", (long long)ldx, (long long)ldo);
    HookScope S;
    CKR(S.begin(device));
    float *dx = nullptr, *dg = nullptr, *db = nullptr, *d32 = nullptr;
    half_t* d16 = nullptr;
    CKR(S.upload(&dx, x, (size_t)M * ldx));
    CKR(S.upload(&dg, gamma, (size_t)d));
    CKR(S.upload(&db, beta, (size_t)d));
    CKR(S.upload(&d16, h16(out16), (size_t)M * ldo));
    if (out32) {
        CKR(S.upload(&d32, out32, (size_t)M * ldo));
        launch_layernorm_f16_f32(dx, ldx, dg, db, d16, d32, ldo, M, d, S.st);
        CKR(S.download(out32, d32, (size_t)M * ldo));
    } else {
        launch_layernorm_f16(dx, ldx, dg, db, d16, ldo, M, d, S.st);
    }
    CKR(S.download(h16(out16), d16, (size_t)M * ldo));
    return S.finish();
}

extern "C" int32_t wlx_debug_attn_encoder(int32_t device, const uint16_t* q, int64_t ldq, int64_t isq, const uint16_t* k, int64_t ldk,
                                          int64_t isk, const uint16_t* vt, int64_t ldvt, int64_t isv, uint16_t* o, int64_t ldo,
                                          int64_t iso, int32_t T, int32_t H, int32_t items) {
    if (!q || !k || !vt || !o) return set_error(WLX_ERR_ARG, "null argument");
    if (H < 1 || H > 64 || items < 1 || items > 64) return set_error(WLX_ERR_ARG, "H %d / items %d outside 1..64", H, items);
    // Both kernels put DEPTH - 1 = 3 key tiles in flight behind the two query pieces and then wait until at most 3 tiles' worth of
    // requests is outstanding: with fewer than 3 tiles (T <= 64) that wait is already satisfied while the query pieces may still
    // be in flight. The launcher's contract is therefore T >= 65 (the encoder runs T = 1500).
    if (T < 65 || T > 32768) return set_error(WLX_ERR_ARG, "T %d outside 65..32768 (the kernels need at least three 32-key tiles)", T);
    const int64_t w = 64L * H, tpad = ((int64_t)T + 31) / 32 * 32;
    if (ldq < w || ldk < w || ldo < w) return set_error(WLX_ERR_ARG, "Q / K / O row strides must cover H * 64 columns");
    if (ldvt < tpad) return set_error(WLX_ERR_ARG, "ldvt %lld does not cover the 32-key padding (%lld columns)", (long long)ldvt, (long long)tpad);
    if (ldq % 8 || ldk % 8 || ldvt % 8 || isq % 8 || isk % 8 || isv % 8 || ldo % 4 || iso % 4)
        return set_error(WLX_ERR_ARG, "Q / K / V^T strides must be multiples of 8 halfs (16-byte loads), O strides of 4");
    if (isq < (int64_t)T * ldq || isk < (int64_t)T * ldk || isv < w * ldvt || iso < (int64_t)T * ldo)
        return set_error(WLX_ERR_ARG, "item strides must cover T rows of Q / K / O and H * 64 rows of V^T");
    HookScope S;
    CKR(S.begin(device));
    half_t *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    CKR(S.upload(&dq, h16(q), (size_t)items * isq));
    CKR(S.upload(&dk, h16(k), (size_t)items * isk));
    CKR(S.upload(&dv, h16(vt), (size_t)items * isv));
    CKR(S.upload(&dout, h16(o), (size_t)items * iso));
    launch_attn_encoder(dq, ldq, dk, ldk, dv, ldvt, dout, ldo, T, H, items, isq, isk, isv, iso, S.st);
    CKR(S.download(h16(o), dout, (size_t)items * iso));
    return S.finish();
}

extern "C" int32_t wlx_debug_dec_cross_attn(int32_t device, const uint16_t* q, int64_t ldq, const uint16_t* kp, const uint16_t* vp,
                                            int64_t item_stride, int32_t n_items, int32_t H, int32_t R, int32_t groups, int32_t rows,
                                            const int32_t* group_item, uint16_t* part_o, float* part_ml, uint16_t* out, int64_t ldo,
                                            int32_t align_item, int32_t align_head, float* align_out) {
    if (!q || !kp || !vp || !group_item || !part_o || !part_ml || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (H < 1 || H > 64 || n_items < 1) return set_error(WLX_ERR_ARG, "H %d outside 1..64 / n_items %d", H, n_items);
    if (R < 1 || R > 16) return set_error(WLX_ERR_ARG, "R %d outside 1..16 (one 16-row MFMA query tile per group)", R);
    if (groups < 1 || groups > 65535) return set_error(WLX_ERR_ARG, "groups %d outside 1..65535", groups);
    // a dead query lane of a group falls back to the group's first row, which must exist; the combine maps row m to group m / R
    if ((int64_t)rows <= (int64_t)(groups - 1) * R || (int64_t)rows > (int64_t)groups * R)
        return set_error(WLX_ERR_ARG, "rows %d outside ((groups - 1) * R, groups * R] = (%d, %d]", rows, (groups - 1) * R, groups * R);
    const int64_t w = 64L * H, image = w * WLX_T_AUDIO_PAD;
    if (ldq < w || ldo < w || ldq % 8 || ldo % 8) return set_error(WLX_ERR_ARG, "q / out row strides must cover H * 64 columns and be multiples of 8");
    if (item_stride < image || item_stride % 8)
        return set_error(WLX_ERR_ARG, "item_stride %lld below the packed image of H heads (%lld halfs) or not a multiple of 8", (long long)item_stride, (long long)image);
    for (int g = 0; g < groups; ++g)
        if (group_item[g] < 0 || group_item[g] >= n_items) return set_error(WLX_ERR_ARG, "group %d: item %d outside 0..%d", g, group_item[g], n_items - 1);
    if (align_out && (align_item < 0 || align_item >= n_items || align_head < 0 || align_head >= H))
        return set_error(WLX_ERR_ARG, "alignment scores of item %d / head %d outside the packed K", align_item, align_head);
    HookScope S;
    CKR(S.begin(device));
    half_t *dq = nullptr, *dk = nullptr, *dv = nullptr, *dpo = nullptr, *dout = nullptr;
    float *dml = nullptr, *dal = nullptr;
    int32_t* dgi = nullptr;
    const size_t n_po = (size_t)groups * H * WLX_XSPLIT * 16 * 64, n_ml = (size_t)groups * H * 16 * WLX_XSPLIT * 2;
    CKR(S.upload(&dq, h16(q), (size_t)rows * ldq));
    CKR(S.upload(&dk, h16(kp), (size_t)n_items * item_stride));
    CKR(S.upload(&dv, h16(vp), (size_t)n_items * item_stride));
    CKR(S.upload(&dgi, group_item, (size_t)groups));
    CKR(S.upload(&dpo, h16(part_o), n_po));
    CKR(S.upload(&dml, part_ml, n_ml));
    CKR(S.upload(&dout, h16(out), (size_t)rows * ldo));
    launch_dec_cross_attn(dq, ldq, dk, dv, item_stride, H, R, groups, rows, dgi, dpo, dml, S.st);
    launch_dec_xattn_combine(dpo, dml, rows, H, R, dout, ldo, S.st);
    if (align_out) {
        CKR(S.upload(&dal, align_out, (size_t)rows * WLX_T_AUDIO_PAD));
        launch_dec_align_scores(dq, ldq, dk + (int64_t)align_item * item_stride, align_head, rows, dal, S.st);
        CKR(S.download(align_out, dal, (size_t)rows * WLX_T_AUDIO_PAD));
    }
    CKR(S.download(h16(part_o), dpo, n_po));
    CKR(S.download(part_ml, dml, n_ml));
    CKR(S.download(h16(out), dout, (size_t)rows * ldo));
    return S.finish();
}

extern "C" int32_t wlx_debug_dec_self_attn(int32_t device, const uint16_t* q, int64_t ldq, const uint16_t* kc, const uint16_t* vc,
                                           int64_t cache_row_stride, int32_t cache_rows, int32_t d, int32_t H, int32_t rows,
                                           const int32_t* pos, const int32_t* ancrow, const int16_t* anc, int32_t ident_ancestry,
                                           uint16_t* out, int64_t ldo) {
    if (!q || !kc || !vc || !pos || !ancrow || !anc || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (H < 1 || H > 64 || rows < 1 || rows > 65535) return set_error(WLX_ERR_ARG, "H %d outside 1..64 / rows %d outside 1..65535", H, rows);
    const int64_t w = 64L * H;
    if (d < w || d % 8 || ldq < w || ldq % 8 || ldo < w) return set_error(WLX_ERR_ARG, "d / ldq (multiples of 8) / ldo must cover H * 64 columns");
    if (cache_rows < 1 || cache_rows > 32767) return set_error(WLX_ERR_ARG, "cache_rows %d outside 1..32767 (int16 ancestry)", cache_rows);
    int max_pos = 0;
    for (int r = 0; r < rows; ++r) max_pos = std::max(max_pos, pos[r]);
    if (max_pos >= WLX_T_TEXT) max_pos = WLX_T_TEXT - 1;    // (refused row by row below)
    if (cache_row_stride < (int64_t)(max_pos + 1) * d || cache_row_stride % 8)      // (the engine's cache rows hold all 448 positions)
        return set_error(WLX_ERR_ARG, "cache_row_stride %lld must cover positions 0..%d of d columns and be a multiple of 8", (long long)cache_row_stride, max_pos);
    if ((int64_t)cache_rows * cache_row_stride >= (1LL << 31))
        return set_error(WLX_ERR_ARG, "cache of %d rows x %lld halfs exceeds the kernel's 32-bit element offsets", cache_rows, (long long)cache_row_stride);
    for (int r = 0; r < rows; ++r) {
        if (pos[r] < 0 || pos[r] >= WLX_T_TEXT) return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..447", r, pos[r]);
        if (ancrow[r] < 0 || ancrow[r] >= cache_rows) return set_error(WLX_ERR_ARG, "row %d: ancestry row %d outside the table", r, ancrow[r]);
        if (ident_ancestry && ancrow[r] != r) return set_error(WLX_ERR_ARG, "ident_ancestry with ancrow[%d] = %d", r, ancrow[r]);
        const int16_t* ar = anc + (int64_t)ancrow[r] * WLX_T_TEXT;
        for (int p = 0; p <= pos[r]; ++p)
            if (ar[p] < 0 || ar[p] >= cache_rows) return set_error(WLX_ERR_ARG, "row %d: cache row %d at position %d outside the cache", r, ar[p], p);
    }
    HookScope S;
    CKR(S.begin(device));
    half_t *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    int32_t *dpos = nullptr, *danr = nullptr;
    int16_t* danc = nullptr;
    CKR(S.upload(&dq, h16(q), (size_t)rows * ldq));
    CKR(S.upload(&dk, h16(kc), (size_t)cache_rows * cache_row_stride));
    CKR(S.upload(&dv, h16(vc), (size_t)cache_rows * cache_row_stride));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&danr, ancrow, (size_t)rows));
    CKR(S.upload(&danc, anc, (size_t)cache_rows * WLX_T_TEXT));
    CKR(S.upload(&dout, h16(out), (size_t)rows * ldo));
    RowTables rt{};
    rt.pos = dpos; rt.ancrow = danr; rt.anc = danc;
    launch_dec_self_attn(dq, ldq, dk, dv, cache_row_stride, d, H, rt, rows, dout, ldo, nullptr, ident_ancestry != 0, S.st);
    CKR(S.download(h16(out), dout, (size_t)rows * ldo));
    return S.finish();
}

// One launch_gemm (force_form -1) or one launch on a given form. W is float32 and packed here with the production pack kernels.
extern "C" int32_t wlx_debug_gemm(int32_t device, const wlx_debug_gemm_args* a, const uint16_t* A, const float* W, const float* bias,
                                  const float* pos, uint16_t* C, float* X, uint16_t* kout, uint16_t* vt, int32_t* ran_out) {
    if (!a || !A || !W || !ran_out) return set_error(WLX_ERR_ARG, "null argument");
    const int mode = a->mode, M = a->M, N = a->N, K = a->K, KT = a->KT, Z = a->zbatch, d = a->d, rpi = a->rows_per_item;
    if (mode < 0 || mode > 5) return set_error(WLX_ERR_ARG, "mode %d outside 0..5", mode);
    if (a->force_form < -1 || a->force_form > 3) return set_error(WLX_ERR_ARG, "force_form %d outside -1..3", a->force_form);
    if (M < 1 || N < 8 || N % 8 || K < 1 || Z < 1 || Z > 64) return set_error(WLX_ERR_ARG, "M %d / N %d (a multiple of 8: 16-byte output pieces) / K %d / zbatch %d", M, N, K, Z);
    if (KT < 2 || (KT & 1) || (int64_t)KT * 32 < K) return set_error(WLX_ERR_ARG, "KT %d must be even and cover K %d (a stage is two k-tiles)", KT, K);
    if (a->conv3_cin && K != 3 * a->conv3_cin) return set_error(WLX_ERR_ARG, "conv weight: K %d != 3 * Cin %d", K, a->conv3_cin);
    if (a->lda < 8 || a->lda % 8 || a->strideA % 8) return set_error(WLX_ERR_ARG, "lda / strideA must be multiples of 8 halfs");
    // every row is read for KT * 32 columns from its start (columns past K meet zero weights), rows past M are clamped
    if ((int64_t)(Z - 1) * a->strideA + (int64_t)(M - 1) * a->lda + (int64_t)KT * 32 > a->a_len || (Z > 1 && a->strideA < 0))
        return set_error(WLX_ERR_ARG, "A (%lld halfs) does not hold KT * 32 columns behind its last row", (long long)a->a_len);
    const bool scatter = mode == GEMM_QKV || mode == GEMM_CROSS_KV;
    if (mode == GEMM_STORE_F16 || mode == GEMM_GELU_F16) {
        if (!C || a->ldc < N || a->ldc % 8 || a->strideC % 8 || a->strideC < 0 || (int64_t)(Z - 1) * a->strideC + (int64_t)(M - 1) * a->ldc + N > a->c_len)
            return set_error(WLX_ERR_ARG, "C: ldc / strideC (multiples of 8) / length do not hold [zbatch][M][N]");
    } else if (mode == GEMM_GELU_POS_F32 || mode == GEMM_RESID_F32) {
        if (!X || a->ldx < N || a->ldx % 4 || a->strideX % 4 || a->strideX < 0 || (int64_t)(Z - 1) * a->strideX + (int64_t)(M - 1) * a->ldx + N > a->x_len)
            return set_error(WLX_ERR_ARG, "X: ldx / strideX (multiples of 4) / length do not hold [zbatch][M][N]");
        if (mode == GEMM_GELU_POS_F32 && !pos) return set_error(WLX_ERR_ARG, "mode 2 needs pos [M][N]");
    } else {
        if (Z != 1) return set_error(WLX_ERR_ARG, "the scattering modes take zbatch 1");
        if (!kout || !vt || d < 64 || d % 64 || rpi < 1) return set_error(WLX_ERR_ARG, "scatter: K / V^T outputs, d %d (a multiple of 64), rows_per_item %d", d, rpi);
        const int64_t items = ((int64_t)M + rpi - 1) / rpi, tl = std::min(M, rpi);
        if (a->kv_item_stride_k % 8 || a->kv_item_stride_v % 8 || a->kv_item_stride_k < 0 || a->kv_item_stride_v < 0)
            return set_error(WLX_ERR_ARG, "item strides must be non-negative multiples of 8");
        if (mode == GEMM_QKV) {
            if (N != 3 * d) return set_error(WLX_ERR_ARG, "QKV: N %d != 3 d", N);
            if (!C || a->ldc < d || a->ldc % 8 || (int64_t)(M - 1) * a->ldc + d > a->c_len) return set_error(WLX_ERR_ARG, "q: ldc / length do not hold [M][d]");
            if (a->ldk < d || a->ldk % 8 || (items - 1) * a->kv_item_stride_k + (tl - 1) * a->ldk + d > a->k_len)
                return set_error(WLX_ERR_ARG, "K rows: ldk / item stride / length do not hold [items][rows_per_item][d]");
            if (a->ldvt < (rpi + 3) / 4 * 4 || a->ldvt % 4 || (items - 1) * a->kv_item_stride_v + (int64_t)(d - 1) * a->ldvt + (tl + 3) / 4 * 4 > a->v_len)
                return set_error(WLX_ERR_ARG, "V^T: ldvt (a multiple of 4 covering rows_per_item) / item stride / length do not hold [items][d][ldvt]");
        } else {
            if (N % (2 * d)) return set_error(WLX_ERR_ARG, "cross K/V: N %d is not a multiple of 2 d", N);
            const int64_t L = N / (2 * d), image = (int64_t)d * WLX_T_AUDIO_PAD;
            if (rpi > WLX_T_AUDIO_PAD) return set_error(WLX_ERR_ARG, "cross K/V: rows_per_item %d exceeds the 1536 keys of a packed image", rpi);
            if (a->kv_item_stride_k < image || a->kv_item_stride_v < image || a->kv_layer_stride_k % 8 || a->kv_layer_stride_v % 8 ||
                a->kv_layer_stride_k < 0 || a->kv_layer_stride_v < 0)
                return set_error(WLX_ERR_ARG, "cross K/V: item strides below a packed image of d * 1536 halfs, or layer strides not multiples of 8");
            if ((L - 1) * a->kv_layer_stride_k + (items - 1) * a->kv_item_stride_k + image > a->k_len ||
                (L - 1) * a->kv_layer_stride_v + (items - 1) * a->kv_item_stride_v + image > a->v_len)
                return set_error(WLX_ERR_ARG, "cross K/V: the packed outputs do not hold [layers][items][d * 1536]");
        }
    }
    GemmParams p{};
    p.lda = a->lda; p.strideA = a->strideA; p.KT = KT; p.M = M; p.N = N; p.mode = mode;
    p.ldc = a->ldc; p.strideC = a->strideC; p.ldx = a->ldx; p.strideX = a->strideX;
    p.d = d; p.qscale = a->qscale; p.ldk = a->ldk; p.ldvt = a->ldvt; p.rows_per_item = rpi;
    p.kv_item_stride_k = a->kv_item_stride_k; p.kv_item_stride_v = a->kv_item_stride_v;
    p.kv_layer_stride_k = a->kv_layer_stride_k; p.kv_layer_stride_v = a->kv_layer_stride_v;
    const int form_req = a->force_form;
    if (form_req >= 0 && form_req <= 2) {
        static const int wnt[3] = {2, 3, 4};
        if (scatter && d % (32 * wnt[form_req])) return set_error(WLX_ERR_ARG, "form %d: d %d is not a multiple of its %d-column tile", form_req, d, 32 * wnt[form_req]);
    } else if (form_req == 3) {
        if (Z != 1 || (N & 255) || (KT & 3) || KT < 8) return set_error(WLX_ERR_ARG, "the large-M form needs zbatch 1, N %% 256 == 0, KT %% 4 == 0, KT >= 8");
        if ((int64_t)M * a->lda * 2 >= (1LL << 31) || (int64_t)N * KT * 64 >= (1LL << 31)) return set_error(WLX_ERR_ARG, "the large-M form uses 32-bit buffer offsets");
    }
    HookScope S;
    CKR(S.begin(device));
    if (gemm_prepare_device() != 0) return set_error(WLX_ERR_HIP, "gemm_prepare_device failed");
    half_t *dA = nullptr, *dWp = nullptr, *dC = nullptr, *dK = nullptr, *dV = nullptr;
    float *dW = nullptr, *db = nullptr, *dpos = nullptr, *dX = nullptr;
    CKR(S.upload(&dA, h16(A), (size_t)a->a_len));
    CKR(S.upload(&dW, W, (size_t)N * K));
    int kt_alloc = 0;
    CKR(alloc_packed(S.allocs, N, (int64_t)KT * 32, &dWp, &kt_alloc, true));
    if (a->conv3_cin) launch_pack_conv3(dW, N, a->conv3_cin, dWp, KT, S.st);
    else launch_pack_linear(dW, N, K, K, dWp, KT, 0, S.st);
    if (bias) CKR(S.upload(&db, bias, (size_t)N));
    if (pos && mode == GEMM_GELU_POS_F32) CKR(S.upload(&dpos, pos, (size_t)M * N));
    if (C && a->c_len > 0) CKR(S.upload(&dC, h16(C), (size_t)a->c_len));
    if (X && a->x_len > 0) CKR(S.upload(&dX, X, (size_t)a->x_len));
    if (scatter) {
        CKR(S.upload(&dK, h16(kout), (size_t)a->k_len));
        CKR(S.upload(&dV, h16(vt), (size_t)a->v_len));
    }
    p.A = dA; p.Wp = dWp; p.bias = db; p.pos = dpos; p.C = dC; p.X = dX; p.Kout = dK; p.Vt = dV;
    const int form = form_req >= 0 ? form_req : gemm_form_of(p, Z);
    GemmParams ran = p;
    if (form_req < 0) {
        launch_gemm(p, Z, S.st);
        // what launch_gemm did with it: the same function on the picked form fills `ran` without launching twice — recomputed below
        if (form == 3) { ran.epi_lds = ((std::max(rpi, 0) ? rpi : 4) & 3) == 0 && (!scatter || d % 256 == 0); ran.xcd_a = ran.xcd_b = 0; }
    } else {
        launch_gemm_form(p, Z, form, &ran, S.st);
    }
    static const int wnt[3] = {2, 3, 4}, wmt[3] = {3, 3, 4};
    const bool f16_out = mode == GEMM_STORE_F16 || mode == GEMM_GELU_F16 || scatter;
    const int rp = rpi > 0 ? rpi : 4;
    int epi, xa = 0, xb = 0;
    if (form == 3) epi = f16_out && (rp & 3) == 0 && (!scatter || d % 256 == 0);
    else {
        epi = f16_out && (rp & 3) == 0 && (!scatter || d % (32 * wnt[form]) == 0);
        if (form_req >= 0) { xa = ran.xcd_a; xb = ran.xcd_b; }
        else {          // the launcher's rule, restated for the report only (gemm2_go)
            const int gx = ((N + 15) / 16 + 2 * wnt[form] - 1) / (2 * wnt[form]), gy = (M + 32 * wmt[form] - 1) / (32 * wmt[form]);
            if (Z == 1 && (gx * gy) % 8 == 0 && gx * gy >= 16) {
                double best = 1e300;
                for (int aa = 1; aa <= 8; aa <<= 1) {
                    const int bb = 8 / aa;
                    if (gy % aa || gx % bb) continue;
                    const double bytes = (double)M / aa + (double)N / bb;
                    if (bytes < best) { best = bytes; xa = aa; xb = bb; }
                }
            }
        }
    }
    ran_out[0] = form; ran_out[1] = epi; ran_out[2] = xa; ran_out[3] = xb;
    if (dC) CKR(S.download(h16(C), dC, (size_t)a->c_len));
    if (dX) CKR(S.download(X, dX, (size_t)a->x_len));
    if (scatter) {
        CKR(S.download(h16(kout), dK, (size_t)a->k_len));
        CKR(S.download(h16(vt), dV, (size_t)a->v_len));
    }
    return S.finish();
}

// One launch_dec_gemv on a GemvParams built from the arguments, as engine_decode.hip decoder_pass builds them (done = null: the lean kernels
// do not read it). W is float32 [N][K], packed here with the production pack kernel.
extern "C" int32_t wlx_debug_dec_gemv(int32_t device, const wlx_debug_dec_gemv_args* a, const float* W, const float* bias, const float* gamma,
                                      const float* beta, float* X, const uint16_t* Xh, const uint16_t* part_o, const float* part_ml,
                                      float* slab, const uint16_t* tok_emb, const float* pos_emb, const int32_t* emb_token,
                                      const int32_t* row_pos, const int32_t* row_cache, uint16_t* Yh, float* Y, float* Xres, uint16_t* Kc,
                                      uint16_t* Vc, int32_t* intok, char* name_out, int32_t name_cap) {
    if (!a || !W || !name_out || name_cap < 1) return set_error(WLX_ERR_ARG, "null argument");
    const int in = a->in_mode, out = a->out_mode, xs = a->xsrc, M = a->M, K = a->K, KT = a->KT, N = a->N, d = a->d;
    if (in < GEMV_IN_LN || in > GEMV_IN_XATTN || out < GEMV_OUT_F16 || out > GEMV_OUT_SLAB || xs < GEMV_X_PLAIN || xs > GEMV_X_EMBED)
        return set_error(WLX_ERR_ARG, "in_mode %d / out_mode %d / xsrc %d outside their enums", in, out, xs);
    if (M < 1 || M > WLX_MAX_DEC_ROWS) return set_error(WLX_ERR_ARG, "M %d outside 1..%d", M, WLX_MAX_DEC_ROWS);
    if (K < 32 || KT < 1 || K != 32 * KT) return set_error(WLX_ERR_ARG, "K %d != 32 * KT %d (the decode projections take whole k-tiles)", K, KT);
    if (N < 1 || N > (1 << 20)) return set_error(WLX_ERR_ARG, "N %d outside 1..2^20", N);
    // every epilogue but the fp32 logits stores 4-column pieces of whole 16-column tiles and reads its bias as float4
    if (out != GEMV_OUT_F32 && (!bias || (N & 15))) return set_error(WLX_ERR_ARG, "out_mode %d needs a bias and N %d a multiple of 16", out, N);
    // (fp32 rows out with a bias is no launch of the engine's: above 8192 columns the lean kernel pairs column tiles without a clamp)
    if (out == GEMV_OUT_F32 && bias && ((N & 15) || N > 8192)) return set_error(WLX_ERR_ARG, "fp32 rows out with a bias: N %d must be a multiple of 16, <= 8192", N);
    if (a->busy_device != 0 && a->busy_device != 1) return set_error(WLX_ERR_ARG, "busy_device %d", a->busy_device);
    // (the first-generation kernel's LayerNorm prologue holds one chunk of six k-tiles on each of at most eight waves)
    if (in == GEMV_IN_LN && KT > 48) return set_error(WLX_ERR_ARG, "LayerNorm prologue: K %d above 1536", K);
    if (xs != GEMV_X_PLAIN && !(in == GEMV_IN_LN || (in == GEMV_IN_F16 && out == GEMV_OUT_RESID && xs == GEMV_X_SLABS)))
        return set_error(WLX_ERR_ARG, "xsrc %d: LayerNorm prologue, or slabs under the residual epilogue of fp16 rows", xs);
    if (xs == GEMV_X_EMBED && out != GEMV_OUT_QKV) return set_error(WLX_ERR_ARG, "embedding rows feed a layer's first projection (QKV) only");
    const bool slabs_in = xs == GEMV_X_SLABS, slab_used = slabs_in || out == GEMV_OUT_SLAB;
    const int64_t rows1 = M - 1;
    // ---- inputs by mode
    if (in == GEMV_IN_LN) {
        if (!gamma || !beta) return set_error(WLX_ERR_ARG, "LayerNorm prologue without gamma / beta");
        if (!X || a->ldx < K || a->ldx % 4 || rows1 * a->ldx + K > a->x_len)
            return set_error(WLX_ERR_ARG, "X: ldx %lld (a multiple of 4 covering K) / length %lld do not hold [M][K]", (long long)a->ldx, (long long)a->x_len);
    } else if (in == GEMV_IN_F16) {
        if (!Xh || a->ldxh < K || a->ldxh % 8 || rows1 * a->ldxh + K > a->xh_len)
            return set_error(WLX_ERR_ARG, "Xh: ldxh %lld (a multiple of 8 covering K) / length %lld do not hold [M][K]", (long long)a->ldxh, (long long)a->xh_len);
    } else {
        if (!part_o || !part_ml || a->R < 1 || a->R > 16 || a->H < 1 || 64 * a->H != K)
            return set_error(WLX_ERR_ARG, "split combine: partials, R %d in 1..16, H %d * 64 == K %d", a->R, a->H, K);
        if (xs != GEMV_X_PLAIN || out != GEMV_OUT_RESID) return set_error(WLX_ERR_ARG, "split combine: plain rows, residual epilogue");
        const int64_t items = ((int64_t)M + a->R - 1) / a->R;
        if (items * a->H * WLX_XSPLIT * 16 * 64 > a->part_o_len || items * a->H * 16 * WLX_XSPLIT * 2 > a->part_ml_len)
            return set_error(WLX_ERR_ARG, "split combine: partials of %lld groups do not fit part_o / part_ml", (long long)items);
    }
    // ---- outputs by mode
    if (out == GEMV_OUT_F16 || out == GEMV_OUT_GELU_F16 || out == GEMV_OUT_QKV) {
        const int w = out == GEMV_OUT_QKV ? d : N;
        if (out == GEMV_OUT_QKV && (d < 16 || d % 16 || N != 3 * d)) return set_error(WLX_ERR_ARG, "QKV: N %d != 3 d, d %d a multiple of 16", N, d);
        if (!Yh || a->ldyh < w || a->ldyh % 4 || rows1 * a->ldyh + w > a->yh_len)
            return set_error(WLX_ERR_ARG, "Yh: ldyh %lld (a multiple of 4) / length %lld do not hold [M][%d]", (long long)a->ldyh, (long long)a->yh_len, w);
    } else if (out == GEMV_OUT_F32) {
        if (!Y || a->ldy < N || a->ldy % 4 || rows1 * a->ldy + N > a->y_len)
            return set_error(WLX_ERR_ARG, "Y: ldy %lld (a multiple of 4) / length %lld do not hold [M][N]", (long long)a->ldy, (long long)a->y_len);
    }
    if (out == GEMV_OUT_RESID || out == GEMV_OUT_SLAB) {
        if (a->ldxres < N || a->ldxres % 4) return set_error(WLX_ERR_ARG, "ldxres %lld must cover N and be a multiple of 4", (long long)a->ldxres);
        if (out == GEMV_OUT_RESID && (!Xres || rows1 * a->ldxres + N > a->xres_len)) return set_error(WLX_ERR_ARG, "Xres (%lld floats) does not hold [M][N]", (long long)a->xres_len);
    }
    if (slab_used) {
        const int64_t ld = in == GEMV_IN_LN ? a->ldx : a->ldxres, w = in == GEMV_IN_LN ? K : N;
        if (!slab || a->slab_stride < 0 || a->slab_stride % 4 || (int64_t)(WLX_FC2_KS - 1) * a->slab_stride + rows1 * ld + w > a->slab_len)
            return set_error(WLX_ERR_ARG, "slab: stride %lld (a multiple of 4) / length %lld do not hold [%d][M][%lld]", (long long)a->slab_stride, (long long)a->slab_len, WLX_FC2_KS, (long long)w);
    }
    if (out == GEMV_OUT_QKV) {
        if (!row_pos || !row_cache || !Kc || !Vc || a->cache_row_stride < d || a->cache_row_stride % 4)
            return set_error(WLX_ERR_ARG, "QKV: row tables, caches, cache_row_stride %lld (a multiple of 4)", (long long)a->cache_row_stride);
        for (int r = 0; r < M; ++r) {
            if (row_pos[r] < 0 || row_pos[r] >= WLX_T_TEXT || row_cache[r] < 0 || row_cache[r] > 32767)
                return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..447 or cache row %d outside 0..32767", r, row_pos[r], row_cache[r]);
            const int64_t end = (int64_t)row_cache[r] * a->cache_row_stride + (int64_t)row_pos[r] * d + d;
            if ((int64_t)(row_pos[r] + 1) * d > a->cache_row_stride || end > a->kc_len || end > a->vc_len)
                return set_error(WLX_ERR_ARG, "row %d: cache row %d position %d outside the caches", r, row_cache[r], row_pos[r]);
        }
    }
    if (xs == GEMV_X_EMBED) {
        if (!tok_emb || !pos_emb || !emb_token || !intok) return set_error(WLX_ERR_ARG, "embedding rows: tables, tokens, intok");
        for (int r = 0; r < M; ++r) {
            if (emb_token[r] < 0 || ((int64_t)emb_token[r] + 1) * K > a->tok_emb_len) return set_error(WLX_ERR_ARG, "row %d: token %d outside the table", r, emb_token[r]);
            if (((int64_t)row_pos[r] + 1) * K > a->pos_emb_len) return set_error(WLX_ERR_ARG, "row %d: position %d outside the table", r, row_pos[r]);
            if ((int64_t)row_cache[r] * WLX_T_TEXT + row_pos[r] >= a->intok_len) return set_error(WLX_ERR_ARG, "row %d: intok entry outside the table", r);
        }
    }
    GemvParams p{};
    p.in_mode = in; p.out_mode = out; p.xsrc = xs; p.M = M; p.K = K; p.KT = KT; p.N = N; p.busy_device = a->busy_device;
    p.KTS = out == GEMV_OUT_SLAB ? a->KTS : 0; p.H = a->H; p.R = a->R; p.d = d; p.qscale = a->qscale;
    p.ldx = a->ldx; p.ldxh = a->ldxh; p.ldyh = a->ldyh; p.ldy = a->ldy; p.ldxres = a->ldxres;
    p.cache_row_stride = a->cache_row_stride; p.slab_stride = a->slab_stride; p.done = nullptr;
    if (xs == GEMV_X_EMBED) p.ldxres = a->ldx;                      // the gathered rows land in X, where the later residual updates read them
    {   // what the engine asks before it builds such a pass: the first-generation kernel knows neither xsrc nor GEMV_OUT_SLAB
        GemvParams q = p;
        static const float dummy = 0.f;
        static float dummy_slab = 0.f;
        q.bias = bias ? &dummy : nullptr;                           // (the probe only asks whether there is one)
        q.slab = slab_used ? &dummy_slab : nullptr;
        if ((xs != GEMV_X_PLAIN || out == GEMV_OUT_SLAB) && !dec_gemv_is_lean(q))
            return set_error(WLX_ERR_ARG, "xsrc %d / out_mode %d: no lean kernel for M %d K %d N %d KTS %d", xs, out, M, K, N, a->KTS);
        // rows the first-generation kernel holds per launch are whole groups in the split combine: nothing to check; its vocabulary
        // form reads no bias. M > 64 there runs as consecutive chunks (launch_dec_gemv): still one call of the launcher.
    }
    HookScope S;
    CKR(S.begin(device));
    float *dW = nullptr, *db = nullptr, *dg = nullptr, *dbe = nullptr, *dX = nullptr, *dml = nullptr, *dsl = nullptr, *dpe = nullptr, *dY = nullptr,
          *dXr = nullptr;
    half_t *dWp = nullptr, *dXh = nullptr, *dpo = nullptr, *dte = nullptr, *dYh = nullptr, *dK = nullptr, *dV = nullptr;
    int32_t *dtok = nullptr, *dpos = nullptr, *dcache = nullptr, *dintok = nullptr;
    CKR(S.upload(&dW, W, (size_t)N * K));
    int kt_alloc = 0;
    CKR(alloc_packed(S.allocs, N, K, &dWp, &kt_alloc, true));
    launch_pack_linear(dW, N, K, K, dWp, KT, 0, S.st);
    if (bias) CKR(S.upload(&db, bias, (size_t)N));
    if (in == GEMV_IN_LN) { CKR(S.upload(&dg, gamma, (size_t)K)); CKR(S.upload(&dbe, beta, (size_t)K)); }
    const bool x_used = in == GEMV_IN_LN;
    if (x_used) CKR(S.upload(&dX, X, (size_t)a->x_len));
    if (in == GEMV_IN_F16) CKR(S.upload(&dXh, h16(Xh), (size_t)a->xh_len));
    if (in == GEMV_IN_XATTN) { CKR(S.upload(&dpo, h16(part_o), (size_t)a->part_o_len)); CKR(S.upload(&dml, part_ml, (size_t)a->part_ml_len)); }
    if (slab_used) CKR(S.upload(&dsl, slab, (size_t)a->slab_len));
    if (out == GEMV_OUT_QKV) {
        CKR(S.upload(&dpos, row_pos, (size_t)M)); CKR(S.upload(&dcache, row_cache, (size_t)M));
        CKR(S.upload(&dK, h16(Kc), (size_t)a->kc_len)); CKR(S.upload(&dV, h16(Vc), (size_t)a->vc_len));
    }
    if (xs == GEMV_X_EMBED) {
        CKR(S.upload(&dte, h16(tok_emb), (size_t)a->tok_emb_len)); CKR(S.upload(&dpe, pos_emb, (size_t)a->pos_emb_len));
        CKR(S.upload(&dtok, emb_token, (size_t)M)); CKR(S.upload(&dintok, intok, (size_t)a->intok_len));
    }
    const bool yh_used = out == GEMV_OUT_F16 || out == GEMV_OUT_GELU_F16 || out == GEMV_OUT_QKV;
    if (yh_used) CKR(S.upload(&dYh, h16(Yh), (size_t)a->yh_len));
    if (out == GEMV_OUT_F32) CKR(S.upload(&dY, Y, (size_t)a->y_len));
    if (out == GEMV_OUT_RESID) CKR(S.upload(&dXr, Xres, (size_t)a->xres_len));
    p.Wp = dWp; p.bias = db; p.X = dX; p.gamma = dg; p.beta = dbe; p.Xh = dXh; p.part_o = dpo; p.part_ml = dml;
    p.Yh = dYh; p.Y = dY; p.Xres = xs == GEMV_X_EMBED ? dX : dXr; p.Kc = dK; p.Vc = dV; p.row_cache = dcache; p.row_pos = dpos;
    p.slab = dsl; p.tok_emb = dte; p.pos_emb = dpe; p.emb_token = dtok; p.intok = dintok;
    snprintf(name_out, (size_t)name_cap, "%s", dec_gemv_kernel_name(p));
    launch_dec_gemv(p, S.st);
    if (x_used) CKR(S.download(X, dX, (size_t)a->x_len));
    if (slab_used) CKR(S.download(slab, dsl, (size_t)a->slab_len));
    if (yh_used) CKR(S.download(h16(Yh), dYh, (size_t)a->yh_len));
    if (dY) CKR(S.download(Y, dY, (size_t)a->y_len));
    if (dXr) CKR(S.download(Xres, dXr, (size_t)a->xres_len));
    if (out == GEMV_OUT_QKV) { CKR(S.download(h16(Kc), dK, (size_t)a->kc_len)); CKR(S.download(h16(Vc), dV, (size_t)a->vc_len)); }
    if (xs == GEMV_X_EMBED) CKR(S.download(intok, dintok, (size_t)a->intok_len));
    return S.finish();
}

// One launch_dec_cq_cross_attn: LayerNorm of x + query projection (Wq float32 [d][d], packed here) + the split partials of the cross attention.
extern "C" int32_t wlx_debug_dec_cq_cross_attn(int32_t device, const float* x, int64_t ldx, const float* gamma, const float* beta, const float* Wq,
                                               const float* bias, float qscale, int32_t d, const uint16_t* kp, const uint16_t* vp,
                                               int64_t item_stride, int32_t n_items, int32_t H, int32_t R, int32_t groups, int32_t rows,
                                               const int32_t* group_item, uint16_t* part_o, float* part_ml) {
    if (!x || !gamma || !beta || !Wq || !bias || !kp || !vp || !group_item || !part_o || !part_ml) return set_error(WLX_ERR_ARG, "null argument");
    if (H < 1 || H > 64 || n_items < 1 || d < 64) return set_error(WLX_ERR_ARG, "H %d outside 1..64 / n_items %d / d %d", H, n_items, d);
    if (!dec_cq_cross_attn_eligible(d, H, R)) return set_error(WLX_ERR_ARG, "the fused launch does not serve d %d / H %d / R %d", d, H, R);
    if (groups < 1 || groups > 65535) return set_error(WLX_ERR_ARG, "groups %d outside 1..65535", groups);
    // a group's dead query lanes fall back to its last live row, which must exist
    if ((int64_t)rows <= (int64_t)(groups - 1) * R || (int64_t)rows > (int64_t)groups * R)
        return set_error(WLX_ERR_ARG, "rows %d outside ((groups - 1) * R, groups * R] = (%d, %d]", rows, (groups - 1) * R, groups * R);
    if (ldx < d || ldx % 4) return set_error(WLX_ERR_ARG, "ldx %lld must cover d and be a multiple of 4", (long long)ldx);
    const int64_t image = (int64_t)d * WLX_T_AUDIO_PAD;
    if (item_stride < image || item_stride % 8)
        return set_error(WLX_ERR_ARG, "item_stride %lld below the packed image of H heads (%lld halfs) or not a multiple of 8", (long long)item_stride, (long long)image);
    for (int g = 0; g < groups; ++g)
        if (group_item[g] < 0 || group_item[g] >= n_items) return set_error(WLX_ERR_ARG, "group %d: item %d outside 0..%d", g, group_item[g], n_items - 1);
    HookScope S;
    CKR(S.begin(device));
    float *dx = nullptr, *dg = nullptr, *dbe = nullptr, *dW = nullptr, *db = nullptr, *dml = nullptr;
    half_t *dWp = nullptr, *dk = nullptr, *dv = nullptr, *dpo = nullptr;
    int32_t* dgi = nullptr;
    const size_t n_po = (size_t)groups * H * WLX_XSPLIT * 16 * 64, n_ml = (size_t)groups * H * 16 * WLX_XSPLIT * 2;
    CKR(S.upload(&dx, x, (size_t)rows * ldx));
    CKR(S.upload(&dg, gamma, (size_t)d));
    CKR(S.upload(&dbe, beta, (size_t)d));
    CKR(S.upload(&dW, Wq, (size_t)d * d));
    CKR(S.upload(&db, bias, (size_t)d));
    int kt_alloc = 0;
    CKR(alloc_packed(S.allocs, d, d, &dWp, &kt_alloc, true));
    launch_pack_linear(dW, d, d, d, dWp, d / 32, 0, S.st);
    CKR(S.upload(&dk, h16(kp), (size_t)n_items * item_stride));
    CKR(S.upload(&dv, h16(vp), (size_t)n_items * item_stride));
    CKR(S.upload(&dgi, group_item, (size_t)groups));
    CKR(S.upload(&dpo, h16(part_o), n_po));
    CKR(S.upload(&dml, part_ml, n_ml));
    launch_dec_cq_cross_attn(dx, ldx, dg, dbe, dWp, db, qscale, d, dk, dv, item_stride, H, R, groups, rows, dgi, dpo, dml, S.st);
    CKR(S.download(h16(part_o), dpo, n_po));
    CKR(S.download(part_ml, dml, n_ml));
    return S.finish();
}

// ---- word alignment's post-processing (align.hip). Both hooks take a ragged batch of up to WLX_ALIGN_MAX_BATCH entries packed back to back.
static int align_hook_paths(HookScope& S, int n, int32_t* ti, int32_t* fi, int32_t path_stride, int32_t* n_path, int32_t** dti, int32_t** dfi,
                            int32_t** dnp) {
    CKR(S.upload(dti, ti, (size_t)n * path_stride));
    CKR(S.upload(dfi, fi, (size_t)n * path_stride));
    CKR(S.upload(dnp, n_path, (size_t)n));
    return WLX_OK;
}

extern "C" int32_t wlx_debug_dtw(int32_t device, const float* x, int32_t n, const int32_t* N, const int32_t* M, int32_t* text_indices,
                                 int32_t* time_indices, int32_t path_stride, int32_t* n_path) {
    if (!x || !N || !M || !text_indices || !time_indices || !n_path) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 0 || n > WLX_ALIGN_MAX_BATCH) return set_error(WLX_ERR_ARG, "dtw: %d entries outside 0..%d", n, WLX_ALIGN_MAX_BATCH);
    if (n == 0) return WLX_OK;
    AlignEnt ent[WLX_ALIGN_MAX_BATCH];
    for (int e = 0; e < n; ++e) {
        // one thread per text row (<= 448 of them), the path buffer of the kernel holds N + M <= 2048 steps
        if (N[e] < 1 || N[e] > AL_MAX_TOK || M[e] < 1 || M[e] > AL_MAX_NF)
            return set_error(WLX_ERR_ARG, "dtw: entry %d is %d x %d, outside 1..%d x 1..%d", e, N[e], M[e], AL_MAX_TOK, AL_MAX_NF);
        if (path_stride < N[e] + M[e]) return set_error(WLX_ERR_ARG, "dtw: path_stride %d below N + M = %d of entry %d", path_stride, N[e] + M[e], e);
        ent[e] = AlignEnt{};
        ent[e].N = N[e]; ent[e].nf = M[e]; ent[e].n_tok = 0;
    }
    AlignPlan plan{};
    align_layout(ent, n, 0, &plan);
    HookScope S;
    CKR(S.begin(device));
    AlignEnt* dent = nullptr; float* dx = nullptr; unsigned* dtr = nullptr;
    int32_t *dti = nullptr, *dfi = nullptr, *dnp = nullptr;
    CKR(S.upload(&dent, ent, (size_t)n));
    CK(hipStreamSynchronize(S.st));             // (`ent` is this frame's memory)
    CKR(S.upload(&dx, x, plan.x_floats));
    CKR(S.alloc(&dtr, plan.trace_words));
    CKR(align_hook_paths(S, n, text_indices, time_indices, path_stride, n_path, &dti, &dfi, &dnp));
    launch_align_dtw(dent, n, plan.max_N, dx, dtr, dti, dfi, path_stride, dnp, S.st);
    CKR(S.download(text_indices, dti, (size_t)n * path_stride));
    CKR(S.download(time_indices, dfi, (size_t)n * path_stride));
    CKR(S.download(n_path, dnp, (size_t)n));
    return S.finish();
}

extern "C" int32_t wlx_debug_align_post(int32_t device, const float* scores, int32_t n, int32_t n_heads, const int32_t* n_tok, int32_t n_sot,
                                        const int32_t* nf, int32_t median_filter_width, float* cost_out, int32_t* text_indices,
                                        int32_t* time_indices, int32_t path_stride, int32_t* n_path) {
    if (!scores || !n_tok || !nf || !cost_out || !text_indices || !time_indices || !n_path) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 0 || n > WLX_ALIGN_MAX_BATCH) return set_error(WLX_ERR_ARG, "align_post: %d entries outside 0..%d", n, WLX_ALIGN_MAX_BATCH);
    if (n_heads < 1 || n_heads > 65535 || n_sot < 1) return set_error(WLX_ERR_ARG, "align_post: n_heads %d outside 1..65535 / n_sot %d", n_heads, n_sot);
    if (median_filter_width < 1 || median_filter_width > WLX_ALIGN_MAX_MEDIAN || (median_filter_width & 1) == 0)
        return set_error(WLX_ERR_ARG, "align_post: filter width %d must be odd in 1..%d", median_filter_width, WLX_ALIGN_MAX_MEDIAN);
    if (n == 0) return WLX_OK;
    AlignEnt ent[WLX_ALIGN_MAX_BATCH];
    for (int e = 0; e < n; ++e) {
        if (n_tok[e] < n_sot + 3 || n_tok[e] > AL_MAX_TOK) return set_error(WLX_ERR_ARG, "align_post: entry %d has %d tokens, outside %d..%d", e, n_tok[e], n_sot + 3, AL_MAX_TOK);
        if (nf[e] < 1 || nf[e] > AL_MAX_NF) return set_error(WLX_ERR_ARG, "align_post: entry %d has %d frames, outside 1..%d", e, nf[e], AL_MAX_NF);
        ent[e] = AlignEnt{};
        ent[e].n_tok = n_tok[e]; ent[e].nf = nf[e]; ent[e].N = n_tok[e] - 1 - n_sot;
        if (path_stride < ent[e].N + nf[e]) return set_error(WLX_ERR_ARG, "align_post: path_stride %d below N + nf = %d of entry %d", path_stride, ent[e].N + nf[e], e);
    }
    AlignPlan plan{};
    align_layout(ent, n, n_heads, &plan);
    HookScope S;
    CKR(S.begin(device));
    AlignEnt* dent = nullptr; float *ds = nullptr, *dstat = nullptr, *dx = nullptr; unsigned* dtr = nullptr;
    int32_t *dti = nullptr, *dfi = nullptr, *dnp = nullptr;
    CKR(S.upload(&dent, ent, (size_t)n));
    CK(hipStreamSynchronize(S.st));
    CKR(S.upload(&ds, scores, plan.score_floats));
    CKR(S.alloc(&dstat, plan.stat_floats));
    CKR(S.upload(&dx, cost_out, plan.x_floats));
    CKR(S.alloc(&dtr, plan.trace_words));
    CKR(align_hook_paths(S, n, text_indices, time_indices, path_stride, n_path, &dti, &dfi, &dnp));
    launch_align_cost(dent, n, n_heads, n_sot, median_filter_width, plan, ds, dstat, dx, S.st);
    launch_align_dtw(dent, n, plan.max_N, dx, dtr, dti, dfi, path_stride, dnp, S.st);
    CKR(S.download(cost_out, dx, plan.x_floats));
    CKR(S.download(text_indices, dti, (size_t)n * path_stride));
    CKR(S.download(time_indices, dfi, (size_t)n * path_stride));
    CKR(S.download(n_path, dnp, (size_t)n));
    return S.finish();
}

// wlx_debug_bias_apply: launch_dec_bias (dec_bias.hip) on a search state built here for one item of `rows` beams
extern "C" int32_t wlx_debug_bias_apply(int32_t device, int32_t vocab, int32_t eot, int32_t n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                                        const int32_t* edge_next, float boost, int32_t n_tok, const int32_t* tok_ids, const float* tok_vals,
                                        float* logits, int32_t rows, int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent,
                                        int32_t plen, const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out) {
    if (!logits || !tokens || !pos || !parent || !nsp_row || !prev_state || !state_out) return set_error(WLX_ERR_ARG, "null argument");
    if (vocab < 1 || vocab > (1 << 20) || ldl < vocab) return set_error(WLX_ERR_ARG, "vocab %d / ldl %lld", vocab, (long long)ldl);
    if (rows < 1 || rows > WLX_MAX_DEC_ROWS) return set_error(WLX_ERR_ARG, "rows %d outside 1..%d", rows, WLX_MAX_DEC_ROWS);
    if (plen < 1 || plen > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "plen %d outside 1..%d", plen, WLX_T_TEXT);
    // (declared before the scope: the copies below read them until the scope's last wait)
    std::vector<int> block((size_t)WLX_BIAS_TABLE_INTS, 0), zeros((size_t)rows + 4, 0), one_plen(1, plen);
    std::vector<short> anc((size_t)rows * WLX_T_TEXT, 0), state((size_t)rows * WLX_T_TEXT, 0);
    SearchParams sp{};
    CKR(bias_table_fill(block.data(), vocab, n_nodes, edge_off, edge_tok, edge_next, boost, n_tok, tok_ids, tok_vals));
    for (int r = 0; r < rows; ++r) {
        if (pos[r] < 0 || pos[r] >= WLX_T_TEXT) return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..%d", r, pos[r], WLX_T_TEXT - 1);
        if (parent[r] < 0 || parent[r] >= rows) return set_error(WLX_ERR_ARG, "row %d: parent %d outside 0..%d", r, parent[r], rows - 1);
        if (prev_state[r] < 0 || prev_state[r] >= n_nodes) return set_error(WLX_ERR_ARG, "row %d: state %d outside 0..%d", r, prev_state[r], n_nodes - 1);
        if (pos[r] >= 1) {
            anc[(size_t)r * WLX_T_TEXT + pos[r] - 1] = (short)parent[r];
            state[(size_t)parent[r] * WLX_T_TEXT + pos[r] - 1] = prev_state[r];
        }
        anc[(size_t)r * WLX_T_TEXT + pos[r]] = (short)r;
    }
    // the launch writes row r's state at pos[r]: no row may read that word as its parent's (in a decode the rows of an item share a position)
    for (int q = 0; q < rows; ++q)
        if (pos[q] >= plen && pos[q] >= 1 && pos[parent[q]] == pos[q] - 1)
            return set_error(WLX_ERR_ARG, "row %d reads the state row %d writes in this launch (position %d)", q, parent[q], pos[q] - 1);
    sp.V = vocab; sp.ldl = ldl; sp.items = 1; sp.R = rows; sp.rows = rows; sp.sampling = 0; sp.beam = rows; sp.num_hyp = 1; sp.eot = eot;
    HookScope S;
    CKR(S.begin(device));
    int *dblock = nullptr, *dzero = nullptr, *dplen = nullptr, *dtok = nullptr, *dpos = nullptr, *dnsp = nullptr;
    short *danc = nullptr, *dstate = nullptr;
    float* dl = nullptr;
    SearchParams* dsp = nullptr;
    CKR(S.upload(&dblock, block.data(), block.size()));
    CKR(S.upload(&dzero, zeros.data(), zeros.size()));
    CKR(S.upload(&dplen, one_plen.data(), (size_t)1));
    CKR(S.upload(&dtok, tokens, (size_t)rows));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&dnsp, nsp_row, (size_t)rows));
    CKR(S.upload(&danc, anc.data(), anc.size()));
    CKR(S.upload(&dstate, state.data(), state.size()));
    CKR(S.upload(&dl, logits, (size_t)rows * ldl));
    CKR(S.upload(&dsp, &sp, (size_t)1));
    SearchState st{};
    st.done = dzero; st.item_done = dzero + 1; st.row_done = dzero + 4; st.plen = dplen; st.token = dtok; st.pos = dpos; st.anc = danc; st.nsp_row = dnsp;
    launch_dec_bias(dl, dsp, rows, st, bias_table_at(dblock, dstate), S.st);
    CKR(S.download(logits, dl, (size_t)rows * ldl));
    CKR(S.download(state.data(), dstate, state.size()));
    CKR(S.finish());
    for (int r = 0; r < rows; ++r) state_out[r] = state[(size_t)r * WLX_T_TEXT + pos[r]];
    return WLX_OK;
}

// wlx_debug_bias_apply_items: launch_dec_bias_items (dec_bias.hip) on a search state built here for `items` items of R beams each
extern "C" int32_t wlx_debug_bias_apply_items(int32_t device, int32_t vocab, int32_t eot, int32_t n_tables, const int32_t* n_nodes,
                                              const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* boosts,
                                              const int32_t* n_tok, const int32_t* tok_ids, const float* tok_vals, float* logits, int32_t items,
                                              int32_t R, const int32_t* sel, int64_t ldl, const int32_t* tokens, const int32_t* pos,
                                              const int32_t* parent, const int32_t* plen, const int32_t* nsp_row, const int16_t* prev_state,
                                              int16_t* state_out) {
    if (!logits || !sel || !tokens || !pos || !parent || !plen || !nsp_row || !prev_state || !state_out) return set_error(WLX_ERR_ARG, "null argument");
    if (vocab < 1 || vocab > (1 << 20) || ldl < vocab) return set_error(WLX_ERR_ARG, "vocab %d / ldl %lld", vocab, (long long)ldl);
    if (items < 1 || items > 64 || R < 1 || (long)items * R > WLX_MAX_DEC_ROWS)
        return set_error(WLX_ERR_ARG, "%d items of %d rows: items in 1..64, at most %d rows", items, R, WLX_MAX_DEC_ROWS);
    const int rows = items * R;
    std::vector<int> pool, zeros((size_t)rows + items + 4, 0);
    std::vector<short> anc((size_t)rows * WLX_T_TEXT, 0), state((size_t)rows * WLX_T_TEXT, 0);
    SearchParams sp{};
    CKR(bias_items_fill(pool, vocab, n_tables, n_nodes, edge_off, edge_tok, edge_next, boosts, n_tok, tok_ids, tok_vals));
    for (int b = 0; b < items; ++b) {
        if (sel[b] < -1 || sel[b] >= n_tables) return set_error(WLX_ERR_ARG, "item %d names table %d outside -1..%d", b, sel[b], n_tables - 1);
        if (plen[b] < 1 || plen[b] > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "item %d: plen %d outside 1..%d", b, plen[b], WLX_T_TEXT);
    }
    for (int r = 0; r < rows; ++r) {
        if (pos[r] < 0 || pos[r] >= WLX_T_TEXT) return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..%d", r, pos[r], WLX_T_TEXT - 1);
        if (parent[r] < 0 || parent[r] >= rows) return set_error(WLX_ERR_ARG, "row %d: parent %d outside 0..%d", r, parent[r], rows - 1);
        if (prev_state[r] < 0) return set_error(WLX_ERR_ARG, "row %d: state %d is negative", r, prev_state[r]);
        if (pos[r] >= 1) {
            anc[(size_t)r * WLX_T_TEXT + pos[r] - 1] = (short)parent[r];
            state[(size_t)parent[r] * WLX_T_TEXT + pos[r] - 1] = prev_state[r];
        }
        anc[(size_t)r * WLX_T_TEXT + pos[r]] = (short)r;
    }
    // the launch writes row r's state at pos[r]: no row may read that word as its parent's
    for (int q = 0; q < rows; ++q)
        if (pos[q] >= plen[q / R] && pos[q] >= 1 && pos[parent[q]] == pos[q] - 1)
            return set_error(WLX_ERR_ARG, "row %d reads the state row %d writes in this launch (position %d)", q, parent[q], pos[q] - 1);
    sp.V = vocab; sp.ldl = ldl; sp.items = items; sp.R = R; sp.rows = rows; sp.sampling = 0; sp.beam = R; sp.num_hyp = 1; sp.eot = eot;
    HookScope S;
    CKR(S.begin(device));
    int *dpool = nullptr, *dzero = nullptr, *dplen = nullptr, *dsel = nullptr, *dtok = nullptr, *dpos = nullptr, *dnsp = nullptr;
    short *danc = nullptr, *dstate = nullptr;
    float* dl = nullptr;
    SearchParams* dsp = nullptr;
    CKR(S.upload(&dpool, pool.data(), pool.size()));
    CKR(S.upload(&dzero, zeros.data(), zeros.size()));
    CKR(S.upload(&dplen, plen, (size_t)items));
    CKR(S.upload(&dsel, sel, (size_t)items));
    CKR(S.upload(&dtok, tokens, (size_t)rows));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&dnsp, nsp_row, (size_t)rows));
    CKR(S.upload(&danc, anc.data(), anc.size()));
    CKR(S.upload(&dstate, state.data(), state.size()));
    CKR(S.upload(&dl, logits, (size_t)rows * ldl));
    CKR(S.upload(&dsp, &sp, (size_t)1));
    SearchState st{};
    st.done = dzero; st.item_done = dzero + 1; st.row_done = dzero + 1 + items; st.plen = dplen; st.token = dtok; st.pos = dpos; st.anc = danc; st.nsp_row = dnsp;
    launch_dec_bias_items(dl, dsp, rows, st, BiasItems{dpool, dsel, dstate}, S.st);
    CKR(S.download(logits, dl, (size_t)rows * ldl));
    CKR(S.download(state.data(), dstate, state.size()));
    CKR(S.finish());
    for (int r = 0; r < rows; ++r) state_out[r] = state[(size_t)r * WLX_T_TEXT + pos[r]];
    return WLX_OK;
}

// wlx_debug_grammar_apply: launch_dec_grammar (dec_grammar.hip) on a search state built here for one item of `rows` beams
extern "C" int32_t wlx_debug_grammar_apply(int32_t device, int32_t vocab, int32_t eot, int32_t n_states, const int32_t* edge_off,
                                           const int32_t* edge_tok, const int32_t* edge_next, const int32_t* accept, float* logits, int32_t rows,
                                           int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent, int32_t plen,
                                           const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out) {
    if (!logits || !tokens || !pos || !parent || !nsp_row || !prev_state || !state_out) return set_error(WLX_ERR_ARG, "null argument");
    if (vocab < 1 || vocab > (1 << 20) || ldl < vocab || ldl > (1 << 20)) return set_error(WLX_ERR_ARG, "vocab %d / ldl %lld", vocab, (long long)ldl);
    if (rows < 1 || rows > WLX_MAX_DEC_ROWS) return set_error(WLX_ERR_ARG, "rows %d outside 1..%d", rows, WLX_MAX_DEC_ROWS);
    if (plen < 1 || plen > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "plen %d outside 1..%d", plen, WLX_T_TEXT);
    char why[200];
    if (!grammar_table_check(vocab, eot, n_states, edge_off, edge_tok, edge_next, accept, why, sizeof(why))) return set_error(WLX_ERR_ARG, "%s", why);
    // (declared before the scope: the copies below read them until the scope's last wait)
    std::vector<int> block((size_t)GRAMMAR_TABLE_INTS, 0), zeros((size_t)rows + 4, 0), one_plen(1, plen);
    std::vector<short> anc((size_t)rows * WLX_T_TEXT, 0), state((size_t)rows * WLX_T_TEXT, 0);
    SearchParams sp{};
    grammar_table_pack(block.data(), eot, n_states, edge_off, edge_tok, edge_next, accept);
    for (int r = 0; r < rows; ++r) {
        if (tokens[r] < 0 || tokens[r] >= vocab) return set_error(WLX_ERR_ARG, "row %d: token %d outside the vocabulary (%d)", r, tokens[r], vocab);
        if (pos[r] < 0 || pos[r] >= WLX_T_TEXT) return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..%d", r, pos[r], WLX_T_TEXT - 1);
        if (parent[r] < 0 || parent[r] >= rows) return set_error(WLX_ERR_ARG, "row %d: parent %d outside 0..%d", r, parent[r], rows - 1);
        if (prev_state[r] < 0) return set_error(WLX_ERR_ARG, "row %d: state %d is negative", r, prev_state[r]);
        if (pos[r] >= 1) {
            anc[(size_t)r * WLX_T_TEXT + pos[r] - 1] = (short)parent[r];
            state[(size_t)parent[r] * WLX_T_TEXT + pos[r] - 1] = prev_state[r];
        }
        anc[(size_t)r * WLX_T_TEXT + pos[r]] = (short)r;
    }
    // the launch writes row r's state at pos[r]: no row may read that word as its parent's (in a decode the rows of an item share a position)
    for (int q = 0; q < rows; ++q)
        if (pos[q] >= plen && pos[q] >= 1 && pos[parent[q]] == pos[q] - 1)
            return set_error(WLX_ERR_ARG, "row %d reads the state row %d writes in this launch (position %d)", q, parent[q], pos[q] - 1);
    sp.V = vocab; sp.ldl = ldl; sp.items = 1; sp.R = rows; sp.rows = rows; sp.sampling = 0; sp.beam = rows; sp.num_hyp = 1; sp.eot = eot;
    const size_t words = (size_t)rows * ldl + WLX_DEBUG_GUARD;
    HookScope S;
    CKR(S.begin(device));
    int *dblock = nullptr, *dzero = nullptr, *dplen = nullptr, *dtok = nullptr, *dpos = nullptr, *dnsp = nullptr;
    short *danc = nullptr, *dstate = nullptr;
    float* dl = nullptr;
    SearchParams* dsp = nullptr;
    CKR(S.upload(&dblock, block.data(), block.size()));
    CKR(S.upload(&dzero, zeros.data(), zeros.size()));
    CKR(S.upload(&dplen, one_plen.data(), (size_t)1));
    CKR(S.upload(&dtok, tokens, (size_t)rows));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&dnsp, nsp_row, (size_t)rows));
    CKR(S.upload(&danc, anc.data(), anc.size()));
    CKR(S.upload(&dstate, state.data(), state.size()));
    CKR(S.upload(&dl, logits, words));
    CKR(S.upload(&dsp, &sp, (size_t)1));
    SearchState st{};
    st.done = dzero; st.item_done = dzero + 1; st.row_done = dzero + 4; st.plen = dplen; st.token = dtok; st.pos = dpos; st.anc = danc; st.nsp_row = dnsp;
    launch_dec_grammar(dl, dsp, rows, (int)ldl, st, GrammarTable{dblock, dstate}, S.st);
    CKR(S.download(logits, dl, words));
    CKR(S.download(state.data(), dstate, state.size()));
    CKR(S.finish());
    for (int r = 0; r < rows; ++r) state_out[r] = state[(size_t)r * WLX_T_TEXT + pos[r]];
    return WLX_OK;
}

// ---- the small softmax kernels of search.hip: the numbers the host thresholds (no_speech_prob, detect_language, word probabilities)
static int prob_hook_rows(const float* logits, int64_t ldl, int64_t cols, int32_t rows, const void* out) {
    if (!logits || !out) return set_error(WLX_ERR_ARG, "null argument");
    if (rows < 1 || rows > 65535) return set_error(WLX_ERR_ARG, "rows %d outside 1..65535", rows);
    if (cols < 1 || cols > (1 << 20)) return set_error(WLX_ERR_ARG, "%lld admitted ids outside 1..2^20", (long long)cols);
    if (ldl < cols || ldl > (1 << 28) || (int64_t)rows * ldl > (1 << 28))
        return set_error(WLX_ERR_ARG, "ldl %lld must cover the %lld admitted ids, rows * ldl stay within 2^28 floats", (long long)ldl, (long long)cols);
    return WLX_OK;
}

extern "C" int32_t wlx_debug_token_prob(int32_t device, const float* logits, int64_t ldl, int32_t V, int32_t rows, int32_t tok, float* out) {
    CKR(prob_hook_rows(logits, ldl, V, rows, out));
    if (tok < 0 || tok >= V) return set_error(WLX_ERR_ARG, "token %d outside 0..%d", tok, V - 1);
    HookScope S;
    CKR(S.begin(device));
    float *dl = nullptr, *dout = nullptr;
    CKR(S.upload(&dl, logits, (size_t)rows * ldl));
    CKR(S.upload(&dout, out, (size_t)rows + WLX_DEBUG_GUARD));
    launch_token_prob(dl, ldl, V, rows, tok, dout, S.st);
    CKR(S.download(out, dout, (size_t)rows + WLX_DEBUG_GUARD));
    return S.finish();
}

extern "C" int32_t wlx_debug_token_prob_rows(int32_t device, const float* logits, int64_t ldl, int32_t vlim, int32_t rows, const int32_t* toks,
                                             float* out) {
    CKR(prob_hook_rows(logits, ldl, vlim, rows, out));
    if (!toks) return set_error(WLX_ERR_ARG, "null argument");
    HookScope S;
    CKR(S.begin(device));
    float *dl = nullptr, *dout = nullptr;
    int32_t* dt = nullptr;
    CKR(S.upload(&dl, logits, (size_t)rows * ldl));
    CKR(S.upload(&dt, toks, (size_t)rows));
    CKR(S.upload(&dout, out, (size_t)rows + WLX_DEBUG_GUARD));
    launch_token_prob_rows(dl, ldl, vlim, rows, dt, dout, S.st);
    CKR(S.download(out, dout, (size_t)rows + WLX_DEBUG_GUARD));
    return S.finish();
}

extern "C" int32_t wlx_debug_lang_probs(int32_t device, const float* logits, int64_t ldl, int32_t rows, const int32_t* ids, int32_t n,
                                        float* probs) {
    CKR(prob_hook_rows(logits, ldl, 1, rows, probs));
    if (!ids) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || n > WLX_LANG_MAX) return set_error(WLX_ERR_ARG, "n %d outside 1..%d (the slot's id table)", n, WLX_LANG_MAX);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= ldl) return set_error(WLX_ERR_ARG, "id %d (entry %d) outside the row of %lld columns", ids[i], i, (long long)ldl);
    HookScope S;
    CKR(S.begin(device));
    float *dl = nullptr, *dp = nullptr;
    int32_t* di = nullptr;
    CKR(S.upload(&dl, logits, (size_t)rows * ldl));
    CKR(S.upload(&di, ids, (size_t)n));
    CKR(S.upload(&dp, probs, (size_t)rows * n + WLX_DEBUG_GUARD));
    launch_lang_probs(dl, ldl, rows, di, n, dp, S.st);
    CKR(S.download(probs, dp, (size_t)rows * n + WLX_DEBUG_GUARD));
    return S.finish();
}

// ---- the data-movement kernels of the decoder pass
extern "C" int32_t wlx_debug_dec_embed(int32_t device, const uint16_t* tok_emb, int32_t vocab, const float* pos_emb, int32_t n_pos, int32_t d,
                                       const int32_t* tokens, const int32_t* pos, int32_t rows, float* x, int32_t* intok) {
    if (!tok_emb || !pos_emb || !tokens || !pos || !x || !intok) return set_error(WLX_ERR_ARG, "null argument");
    // the kernel moves f16x4 / float4 pieces of a row
    if (d < 4 || d % 4 || d > 8192) return set_error(WLX_ERR_ARG, "d %d must be a multiple of 4 in 4..8192", d);
    if (vocab < 1 || vocab > (1 << 20)) return set_error(WLX_ERR_ARG, "vocab %d outside 1..2^20", vocab);
    if (n_pos < 1 || n_pos > WLX_T_TEXT) return set_error(WLX_ERR_ARG, "n_pos %d outside 1..%d", n_pos, WLX_T_TEXT);
    if (rows < 1 || rows > 65535) return set_error(WLX_ERR_ARG, "rows %d outside 1..65535", rows);
    if ((int64_t)vocab * d > (1 << 28) || (int64_t)rows * d > (1 << 28))
        return set_error(WLX_ERR_ARG, "vocab * d and rows * d must stay within 2^28 elements");
    for (int r = 0; r < rows; ++r) {
        if (tokens[r] < 0 || tokens[r] >= vocab) return set_error(WLX_ERR_ARG, "row %d: token %d outside 0..%d", r, tokens[r], vocab - 1);
        if (pos[r] < 0 || pos[r] >= n_pos) return set_error(WLX_ERR_ARG, "row %d: position %d outside 0..%d", r, pos[r], n_pos - 1);
    }
    std::vector<int32_t> cache((size_t)rows);                   // (declared before the scope: the copy reads it until the scope's last wait)
    for (int r = 0; r < rows; ++r) cache[r] = r;
    HookScope S;
    CKR(S.begin(device));
    half_t* dte = nullptr;
    float *dpe = nullptr, *dx = nullptr;
    int32_t *dtok = nullptr, *dpos = nullptr, *dcache = nullptr, *dintok = nullptr;
    CKR(S.upload(&dte, h16(tok_emb), (size_t)vocab * d));
    CKR(S.upload(&dpe, pos_emb, (size_t)n_pos * d));
    CKR(S.upload(&dtok, tokens, (size_t)rows));
    CKR(S.upload(&dpos, pos, (size_t)rows));
    CKR(S.upload(&dcache, cache.data(), (size_t)rows));
    CKR(S.upload(&dintok, intok, (size_t)rows * WLX_T_TEXT));
    CKR(S.upload(&dx, x, (size_t)rows * d));
    RowTables rt{};
    rt.token = dtok; rt.pos = dpos; rt.cache = dcache; rt.intok = dintok;
    launch_dec_embed(dte, dpe, d, rt, rows, dx, nullptr, S.st);
    CKR(S.download(x, dx, (size_t)rows * d));
    CKR(S.download(intok, dintok, (size_t)rows * WLX_T_TEXT));
    return S.finish();
}

extern "C" int32_t wlx_debug_prep_windows(int32_t device, const float* feats, int64_t feats_len, int64_t ld, int32_t n_mels, int64_t item_stride,
                                          int32_t items, const int32_t* seek, const int32_t* seg, uint16_t* featT, int64_t featT_stride) {
    if (!feats || !seek || !seg || !featT) return set_error(WLX_ERR_ARG, "null argument");
    // prep_window_kernel stages a block's frames in tile[128][33]; PrepWindows holds 64 windows by value
    if (n_mels < 1 || n_mels > 128) return set_error(WLX_ERR_ARG, "n_mels %d outside 1..128", n_mels);
    if (items < 1 || items > 64) return set_error(WLX_ERR_ARG, "items %d outside 1..64", items);
    if (ld < 1 || ld > (1LL << 28) || item_stride < 0 || item_stride > (1LL << 28) || feats_len < 1 || feats_len > (1LL << 28))
        return set_error(WLX_ERR_ARG, "ld %lld / item_stride %lld / feats_len %lld outside 1 (0 for the stride) .. 2^28", (long long)ld, (long long)item_stride, (long long)feats_len);
    if (featT_stride < (int64_t)(WLX_N_FRAMES + 2) * n_mels || featT_stride > (1LL << 28) || (int64_t)items * featT_stride > (1LL << 28))
        return set_error(WLX_ERR_ARG, "featT_stride %lld does not hold %d rows of %d, or items * featT_stride exceeds 2^28", (long long)featT_stride, WLX_N_FRAMES + 2, n_mels);
    PrepWindows pw{};
    for (int i = 0; i < items; ++i) {
        if (seek[i] < 0 || seg[i] < 0 || seg[i] > WLX_N_FRAMES || (int64_t)seek[i] + seg[i] > ld)
            return set_error(WLX_ERR_ARG, "item %d: window [%d, %d + %d) outside 0..3000 frames of a row of %lld", i, seek[i], seek[i], seg[i], (long long)ld);
        if ((int64_t)i * item_stride + (int64_t)(n_mels - 1) * ld + seek[i] + seg[i] > feats_len)
            return set_error(WLX_ERR_ARG, "item %d: its window ends behind feats (%lld floats)", i, (long long)feats_len);
        pw.seek[i] = seek[i]; pw.seg[i] = seg[i];
    }
    HookScope S;
    CKR(S.begin(device));
    float* df = nullptr;
    half_t* dT = nullptr;
    CKR(S.upload(&df, feats, (size_t)feats_len));
    CKR(S.upload(&dT, h16(featT), (size_t)items * featT_stride));
    launch_prep_windows(df, ld, n_mels, item_stride, pw, items, dT, featT_stride, S.st);
    CKR(S.download(h16(featT), dT, (size_t)items * featT_stride));
    return S.finish();
}

extern "C" int32_t wlx_debug_f32_to_f16(int32_t device, const float* src, int64_t n, uint16_t* dst, int64_t cap) {
    if (!src || !dst) return set_error(WLX_ERR_ARG, "null argument");
    if (n < 1 || cap < n || cap > (1LL << 28)) return set_error(WLX_ERR_ARG, "n %lld outside 1..cap, or cap %lld above 2^28", (long long)n, (long long)cap);
    HookScope S;
    CKR(S.begin(device));
    float* ds = nullptr;
    half_t* dd = nullptr;
    CKR(S.upload(&ds, src, (size_t)n));
    CKR(S.upload(&dd, h16(dst), (size_t)cap));
    launch_f32_to_f16(ds, dd, n, S.st);
    CKR(S.download(h16(dst), dd, (size_t)cap));
    return S.finish();
}
