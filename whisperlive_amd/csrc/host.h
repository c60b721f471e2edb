// host.h — the host support layer shared by engine.hip, mt_engine.hip and vad.hip: the error macros, the utility stream,
// device / pinned allocation into an owner's free list, the scope of a test hook call (HookScope: every wlx_*debug* hook of
// kernel_hooks.hip, mt_engine.hip, spk_engine.hip, resample.hip and flac.hip), and weight ingestion (lookup, shape check, fp32
// staging, packing, one Hugging Face transformer layer).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>
#include "../../include/wlx.h"
#include "kernels.h"

namespace wlx {

// the single writer of the thread-local message wlx_last_error() returns
int set_error(int code, const char* fmt, ...);

#define CK(call)                                                                                                      \
    do {                                                                                                              \
        hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess)                                                                                         \
            return wlx::set_error(WLX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CKR(call)                    \
    do {                             \
        int r_ = (call);             \
        if (r_ != WLX_OK) return r_; \
    } while (0)

// per-device non-blocking stream for set-up work (host.hip: the legacy stream is never used)
hipStream_t util_stream();
// host -> device on the utility stream, complete on return
int upload_sync(void* dst, const void* src, size_t bytes);

// ---- allocation into an owner's free list (the owner frees the whole list: hipFree / hipHostFree)
int alloc_bytes(std::vector<void*>& pool, void** out, size_t bytes, bool zero, bool pinned);
// device memory; `zero` clears it on the utility stream (never the null stream) and waits
template <class T>
int dalloc(std::vector<void*>& pool, T** out, size_t count, bool zero) {
    return alloc_bytes(pool, reinterpret_cast<void**>(out), std::max<size_t>(count, 1) * sizeof(T), zero, false);
}
// pinned host memory
template <class T>
int halloc(std::vector<void*>& pool, T** out, size_t count) {
    return alloc_bytes(pool, reinterpret_cast<void**>(out), std::max<size_t>(count, 1) * sizeof(T), false, true);
}
// a packed [ceil(N/16)][ceil(K/32)] fragment image (common.h) for a W[N][K]
int alloc_packed(std::vector<void*>& pool, int64_t N, int64_t K, half_t** out, int* KT_out, bool zero);

// ---- the scope of one kernel-level test hook call (wlx_*debug*): a private non-blocking stream on `device` and the device buffers of
// the call, released on every return path (wait, free, destroy). The hooks' conventions: host arrays in, ONE call of the production
// launcher on `st`, host arrays out; outputs are copied in AND out, so bytes no thread owns come back unchanged; every shape a launcher
// cannot serve is refused (WLX_ERR_ARG) before begin(), so before anything is allocated or launched.
struct HookScope {
    std::vector<void*> allocs;
    hipStream_t st = nullptr;
    ~HookScope() {
        if (st) (void)hipStreamSynchronize(st);
        for (void* p : allocs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    int begin(int device) {
        int n = 0;
        CK(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) return set_error(WLX_ERR_ARG, "device %d outside 0..%d", device, n - 1);
        CK(hipSetDevice(device));
        CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return WLX_OK;
    }
    template <class T>
    int alloc(T** d, size_t n) { return dalloc(allocs, d, n, false); }      // not cleared
    template <class T>
    int upload(T** d, const T* h, size_t n) {
        CKR(alloc(d, n));
        if (h && n) CK(hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, st));
        return WLX_OK;
    }
    template <class T>
    int download(T* h, const T* d, size_t n) {
        CK(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, st));
        return WLX_OK;
    }
    int finish() {
        CK(hipGetLastError());
        CK(hipStreamSynchronize(st));
        return WLX_OK;
    }
};
// the hooks' ABI carries fp16 as uint16_t
inline const half_t* h16(const uint16_t* p) { return reinterpret_cast<const half_t*>(p); }
inline half_t* h16(uint16_t* p) { return reinterpret_cast<half_t*>(p); }

// ---- weight ingestion: the caller's tensors by name, brought to the device and into the kernel layouts.
// All work runs on the source's own non-blocking stream; the destructor synchronises and destroys it and frees the staging
// buffer, on every exit path of the creation function that holds the object.
struct Weights {
    std::map<std::string, const wlx_tensor*> by_name;
    hipStream_t st = nullptr;
    // ONE fp32 staging buffer for host tensors (and scaled device tensors), grown to the largest: a pack kernel reads it on
    // `st` and the next copy into it is queued behind that kernel on the same stream, so it is reused without a wait. It is
    // re-allocated while loading, which is why it is owned here and not by a free list.
    float* staging = nullptr;
    size_t staging_cap = 0;

    ~Weights();
    int open(const wlx_tensor* w, int n);
    int finish();      // waits for everything queued on `st` and reports a failed launch
    int need(const std::string& name, std::initializer_list<int64_t> shape, const wlx_tensor** out) const;
    // device fp32 view of a tensor, valid until the next call. A host tensor (possibly a pageable temporary of the caller) is
    // copied to the staging buffer, complete on return. A device tensor is used in place — never written, never copied —
    // unless `scale` != 1, which multiplies a staged copy.
    int device_f32(const wlx_tensor* t, const float** out, float scale = 1.f);
    // fp32 vector [n] * scale -> dst (engine memory)
    int vec(const std::string& name, int64_t n, float* dst, float scale = 1.f);
    int alloc_vec(std::vector<void*>& pool, const std::string& name, int64_t n, float** out, bool zero);
    // W[N][K] * scale -> the packed image Wp ([NT_total][KT]) at n-tile offset nt0
    int pack(const std::string& name, int64_t N, int64_t K, half_t* Wp, int KT, int nt0, float scale = 1.f);
};

// One transformer layer in kernel layout. An encoder layer leaves the cross-attention members (ln2, Wcq, Wco, bcq, bco) null;
// ln3 is the LayerNorm in front of the MLP (final_layer_norm) in both kinds.
struct LayerW {
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr, *ln3_g = nullptr, *ln3_b = nullptr;
    half_t *Wqkv = nullptr, *Wo = nullptr, *Wcq = nullptr, *Wco = nullptr, *W1 = nullptr, *W2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *bcq = nullptr, *bco = nullptr, *b1 = nullptr, *b2 = nullptr;
};
struct LayerOpts {
    bool k_bias;       // k_proj has a bias (M2M100). Whisper's has none: that part of bqkv / bckv stays as allocated, so `zero` it
    float q_scale;     // folded into q_proj / encoder_attn.q_proj weight and bias (0.125 for M2M100; 1 for Whisper, whose kernels scale)
    bool zero;         // the layer's allocations are zeroed (Whisper) or not (M2M100)
    // decoder layer `l`: its slice of the cross K / V image and bias shared by all layers ([L][k | v]); null for an encoder layer
    half_t* Wckv = nullptr;
    float* bckv = nullptr;
    int l = 0;
};
// loads the Hugging Face layer `prefix` ("model.decoder.layers.3."; the tensor names are the same in Whisper and M2M100)
int load_layer(Weights& ws, std::vector<void*>& pool, const std::string& prefix, int d, int F, const LayerOpts& o, LayerW& w);

}  // namespace wlx
