// dec_gemv_internal.h — what the two files behind launch_dec_gemv share (dec_gemv.hip, dec_vocab.hip). Not part of decoder.h's surface.
#pragma once
#include "decoder.h"
#include <atomic>

namespace wlx {

// Workgroups that need more than the default 64 KiB of dynamic LDS (batched rows of the larger models: 30 rows x 1280 fp16 = 77 KiB of
// staged activations) raise their kernel's limit first, once. The first launch of every shape happens OUTSIDE stream capture
// (engine_decode.hip runs a decoder pass eagerly before it captures one).
#define WLX_G2_LDS_MAX (152 * 1024)
// Set when a device refused the raised limit (another GPU generation, a lower per-block LDS limit): gemv2_cfg / vocab2_ok then keep
// every shape that needs more than 64 KiB on the general kernel instead of launching something that cannot run.
extern std::atomic<bool> g_lds_optin_refused;
// the opt-in of `kernel` on the current device; `granted`: the caller's table of that instantiation (the opt-in is a property of the function ON a device)
void lds_optin(const void* kernel, std::atomic<signed char> (&granted)[64], const char* what);
// A configuration that a probe accepted and whose launch finds no instantiation is a bug in the dispatch. No other kernel runs in its
// place: launching no function leaves hipErrorInvalidDeviceFunction behind, which the engine's hipGetLastError check after the pass reports.
void dispatch_bug(const char* kernel, hipStream_t s);

// ---- the argument head (WLX_KERNARG_HEAD, default on; -DWLX_KERNARG_HEAD=0 builds the previous argument layout: the A/B library)
// A kernel's by-value struct is fetched by scalar loads the wave issues at entry, from a scalar cache that is cold at every launch: a dependent
// round trip in front of the first vector load. gfx950's command processor can instead place the LEADING kernel-argument dwords into user SGPRs at
// dispatch (-mllvm -amdgpu-kernarg-preload-count, _lib.py: dec_gemv.hip, decoder.hip and search.hip — the last two for their flat argument lists as they stand) — but only flat leading arguments, never fields of
// a by-value struct, and at most 14 dwords. So dec_gemv2_kernel (five of a decoder layer's seven launches) takes, in front of its struct, a flat
// head of exactly what its first trip of loads and its weight request read, resolved by the launcher; every other field stays in the struct, whose
// fetch (issued where hipcc places it: at entry in some forms, behind the first requests in others) is first waited on behind those requests. The head repeats fields of the struct (g2_head: the one place that fills it), so a device without
// the preload (it runs the compatibility entry, which fetches the same dwords itself) computes the same. Measured: DESIGN.md §7.3 K1 (this head), K2 / K3
// (the option alone on decoder.hip / search.hip). dec_vocab_kernel still takes one struct and gets nothing.
#ifndef WLX_KERNARG_HEAD
#define WLX_KERNARG_HEAD 1
#endif
// dec_gemv2_kernel, 14 dwords: rows = X (LayerNorm rows) / Xh (fp16 rows) / part_o (split combine); aux = slab (rows + slabs) / part_ml;
// ld = ldx / ldxh; aux_i = slab_stride / R | H << 16; dims = M | nwm << 8 | KTW << 16 | xstage << 24; kt = KT | KTS << 8 | Mtot << 16
struct GemvHead { const void* rows; const void* aux; const float* gamma; const float* beta; const half_t* wp; int ld, aux_i, dims, kt; };
static_assert(sizeof(GemvHead) == 56 && sizeof(GemvHead) % alignof(GemvParams) == 0, "14 dwords, the struct right behind them in the kernel-argument segment");
#if WLX_KERNARG_HEAD
#define WLX_G2_HEAD_PARAMS const void* h_rows, const void* h_aux, const float* h_gamma, const float* h_beta, const half_t* h_wp, int h_ld, int h_aux_i, int h_dims, int h_kt,
#define WLX_G2_HEAD_ARGS(h) (h).rows, (h).aux, (h).gamma, (h).beta, (h).wp, (h).ld, (h).aux_i, (h).dims, (h).kt,
#else
#define WLX_G2_HEAD_PARAMS
#define WLX_G2_HEAD_ARGS(h)
#endif
// the head of a launch of dec_gemv2_kernel with parameters p (launcher fields set); false: a field does not fit its head slot
bool g2_head(const GemvParams& p, GemvHead* h);
// host probe (scripts/gemv_pick_probe.cpp --heads): the head launch_dec_gemv would fill for these parameters and the parameters as launched (row chunks
// and launcher fields set); false: the vocabulary projection or the first-generation kernel runs them
bool dec_gemv_head(const GemvParams& p_any, GemvHead* h, GemvParams* launched);

// ---- dec_vocab.hip: the final LayerNorm + vocabulary projection, the three leaves of its own dispatch (vocab2_dispatch)
bool vocab2_ok(const GemvParams& p);                         // dec_vocab_kernel runs these parameters
void vocab2_launch(const GemvParams& p, hipStream_t s);      // (vocab2_ok(p) holds)
const char* vocab2_kernel_name(const GemvParams& p);         // dec_vocab_kernel<KT, KC, MT> of that launch (vocab2_ok(p) holds)

}  // namespace wlx
