// host.hip — the host support layer of host.h.
#include "host.h"
#include <cstdarg>
#include <cstdio>
#include <mutex>

namespace wlx {

static thread_local char g_err[512] = "";
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------------------------------------
// Nothing in this library may touch the legacy (null) stream once slots exist: while ANY stream is capturing a decode
// graph, a legacy-stream operation from another thread (hipMemset, synchronous hipMemcpy, hipDeviceSynchronize) fails with
// "would make the legacy stream depend on a capturing ... stream" AND invalidates that capture — i.e. a second client
// connecting (slot creation) used to be able to break the first client's transcription. Set-up work that is not tied to a
// slot therefore runs on a per-device non-blocking utility stream and waits for it explicitly.
hipStream_t util_stream() {
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    auto it = streams.find(dev);
    if (it != streams.end()) return it->second;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams[dev] = st;
    return st;
}
int upload_sync(void* dst, const void* src, size_t bytes) {
    hipStream_t us = util_stream();
    if (!us) return set_error(WLX_ERR_HIP, "utility stream creation failed");
    CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, us));
    CK(hipStreamSynchronize(us));
    return WLX_OK;
}

int alloc_bytes(std::vector<void*>& pool, void** out, size_t bytes, bool zero, bool pinned) {
    void* p = nullptr;
    hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return set_error(WLX_ERR_NOMEM, "%s(%zu) failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
    pool.push_back(p);
    if (zero) {
        hipStream_t us = util_stream();
        if (!us) return set_error(WLX_ERR_HIP, "utility stream creation failed");
        CK(hipMemsetAsync(p, 0, bytes, us));
        CK(hipStreamSynchronize(us));
    }
    *out = p;
    return WLX_OK;
}
int alloc_packed(std::vector<void*>& pool, int64_t N, int64_t K, half_t** out, int* KT_out, bool zero) {
    const int KT = (int)((K + 31) / 32), NT = (int)((N + 15) / 16);
    CKR(dalloc(pool, out, (size_t)NT * KT * 512, zero));
    if (KT_out) *KT_out = KT;
    return WLX_OK;
}

// ------------------------------------------------------------------------------------------------
// weight ingestion
__global__ void mt_scale_kernel(float* x, long n, float a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= a;
}
static void scale_f32(float* x, long n, float a, hipStream_t st) {
    if (a != 1.f) hipLaunchKernelGGL(mt_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, a);
}

int Weights::open(const wlx_tensor* w, int n) {
    for (int i = 0; i < n; ++i)
        if (w[i].name) by_name[w[i].name] = &w[i];
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return WLX_OK;
}
Weights::~Weights() {
    if (st) (void)hipStreamSynchronize(st);
    if (staging) (void)hipFree(staging);
    if (st) (void)hipStreamDestroy(st);
}
int Weights::finish() {
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
    return WLX_OK;
}
int Weights::need(const std::string& name, std::initializer_list<int64_t> shape, const wlx_tensor** out) const {
    auto it = by_name.find(name);
    if (it == by_name.end()) return set_error(WLX_ERR_WEIGHT, "missing weight '%s'", name.c_str());
    const wlx_tensor* t = it->second;
    if (t->ndim != (int)shape.size()) return set_error(WLX_ERR_WEIGHT, "weight '%s': ndim %d", name.c_str(), t->ndim);
    int i = 0;
    for (int64_t s : shape) {
        if (t->shape[i] != s)
            return set_error(WLX_ERR_WEIGHT, "weight '%s': dim %d is %lld, expected %lld", name.c_str(), i,
                             (long long)t->shape[i], (long long)s);
        ++i;
    }
    *out = t;
    return WLX_OK;
}
int Weights::device_f32(const wlx_tensor* t, const float** out, float scale) {
    if (t->on_device && scale == 1.f) { *out = reinterpret_cast<const float*>(t->data); return WLX_OK; }
    size_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= (size_t)t->shape[i];
    if (n > staging_cap) {
        CK(hipStreamSynchronize(st));            // (the kernels still reading the old buffer)
        if (staging) CK(hipFree(staging));
        staging = nullptr;
        staging_cap = 0;
        CK(hipMalloc(reinterpret_cast<void**>(&staging), n * sizeof(float)));   // owned here: re-allocated while loading (host.h)
        staging_cap = n;
    }
    CK(hipMemcpyAsync(staging, t->data, n * sizeof(float), t->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!t->on_device) CK(hipStreamSynchronize(st));      // (host tensors may be pageable temporaries of the caller)
    scale_f32(staging, (long)n, scale, st);
    *out = staging;
    return WLX_OK;
}
int Weights::vec(const std::string& name, int64_t n, float* dst, float scale) {
    const wlx_tensor* t;
    CKR(need(name, {n}, &t));
    CK(hipMemcpyAsync(dst, t->data, n * sizeof(float), t->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!t->on_device) CK(hipStreamSynchronize(st));
    scale_f32(dst, (long)n, scale, st);
    return WLX_OK;
}
int Weights::alloc_vec(std::vector<void*>& pool, const std::string& name, int64_t n, float** out, bool zero) {
    CKR(dalloc(pool, out, (size_t)n, zero));
    return vec(name, n, *out);
}
int Weights::pack(const std::string& name, int64_t N, int64_t K, half_t* Wp, int KT, int nt0, float scale) {
    const wlx_tensor* t;
    CKR(need(name, {N, K}, &t));
    const float* src;
    CKR(device_f32(t, &src, scale));
    launch_pack_linear(src, (int)N, (int)K, K, Wp, KT, nt0, st);
    CK(hipGetLastError());
    return WLX_OK;
}

int load_layer(Weights& ws, std::vector<void*>& pool, const std::string& p, int d, int F, const LayerOpts& o, LayerW& w) {
    auto norm = [&](const char* name, float** g, float** b) -> int {
        CKR(ws.alloc_vec(pool, p + name + ".weight", d, g, o.zero));
        return ws.alloc_vec(pool, p + name + ".bias", d, b, o.zero);
    };
    auto linear = [&](const char* name, int N, int K, half_t** W, float** b, float scale) -> int {
        int KT;
        CKR(alloc_packed(pool, N, K, W, &KT, o.zero));
        CKR(ws.pack(p + name + ".weight", N, K, *W, KT, 0, scale));
        CKR(dalloc(pool, b, (size_t)N, o.zero));
        return ws.vec(p + name + ".bias", N, *b, scale);
    };
    // q / k / v of one attention into three consecutive d-row slices of an image and its bias, from n-tile nt0 / element b0 on
    auto qkv = [&](const std::string& a, bool q, half_t* W, int nt0, float* b) -> int {
        const char* part[3] = {"q_proj", "k_proj", "v_proj"};
        for (int i = q ? 0 : 1, j = 0; i < 3; ++i, ++j) {
            const float scale = i == 0 ? o.q_scale : 1.f;
            CKR(ws.pack(p + a + part[i] + ".weight", d, d, W, d / 32, nt0 + j * (d / 16), scale));
            if (i != 1 || o.k_bias) CKR(ws.vec(p + a + part[i] + ".bias", d, b + (size_t)j * d, scale));
        }
        return WLX_OK;
    };
    CKR(norm("self_attn_layer_norm", &w.ln1_g, &w.ln1_b));
    CKR(alloc_packed(pool, 3 * d, d, &w.Wqkv, nullptr, o.zero));
    CKR(dalloc(pool, &w.bqkv, (size_t)3 * d, o.zero));
    CKR(qkv("self_attn.", true, w.Wqkv, 0, w.bqkv));
    CKR(linear("self_attn.out_proj", d, d, &w.Wo, &w.bo, 1.f));
    if (o.Wckv) {
        CKR(norm("encoder_attn_layer_norm", &w.ln2_g, &w.ln2_b));
        CKR(linear("encoder_attn.q_proj", d, d, &w.Wcq, &w.bcq, o.q_scale));
        CKR(linear("encoder_attn.out_proj", d, d, &w.Wco, &w.bco, 1.f));
        // the cross K / V projections of all layers are fused into one encoder-side GEMM
        CKR(qkv("encoder_attn.", false, o.Wckv, o.l * 2 * d / 16, o.bckv + (size_t)o.l * 2 * d));
    }
    CKR(norm("final_layer_norm", &w.ln3_g, &w.ln3_b));
    CKR(linear("fc1", F, d, &w.W1, &w.b1, 1.f));
    return linear("fc2", d, F, &w.W2, &w.b2, 1.f);
}

}  // namespace wlx

extern "C" const char* wlx_last_error(void) { return wlx::g_err; }
