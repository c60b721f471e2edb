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

// ---- dec_vocab.hip: the final LayerNorm + vocabulary projection, the three leaves of its own dispatch (vocab2_dispatch)
bool vocab2_ok(const GemvParams& p);                         // dec_vocab_kernel runs these parameters
void vocab2_launch(const GemvParams& p, hipStream_t s);      // (vocab2_ok(p) holds)
const char* vocab2_kernel_name(const GemvParams& p);         // dec_vocab_kernel<KT, KC, MT> of that launch (vocab2_ok(p) holds)

}  // namespace wlx
