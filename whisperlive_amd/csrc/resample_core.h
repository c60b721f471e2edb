// resample_core.h — what the resample kernels of resample.hip and the ragged form of put_many.hip share: the tile constants, the sample
// conversions of the five formats (rs_sample), floor division and the LDS need of a tile. One text, so that a sample converts to the
// same float32 in every kernel that reads a file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "../../include/wlx.h"

namespace wlx {

constexpr int RS_TILE = 1024;           // outputs per workgroup ...
constexpr int RS_MIN_TILE = 64;         // ... halved down to this while the tile's input span does not fit the LDS (resample_ratio)
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_RATIO = 640;       // max(up, down): 11025 Hz (640 / 441); a tap table of 12801 floats
constexpr int RS_MAX_LDS = 64 * 1024;   // taps + staged span, bytes (the default dynamic-LDS limit; two workgroups per CU at the largest)

__device__ __forceinline__ long long floor_div(long long a, long long b) {       // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// G.711 (ITU-T): one code byte -> its 16-bit linear value, in plain integer arithmetic (no table). tests/test_stream_resample_host.py
// pins the anchors: mu-law 0xFF -> 0, 0x00 -> -32124, 0x80 -> +32124; A-law 0xD5 -> +8, 0x55 -> -8, 0xAA -> +32256.
__host__ __device__ __forceinline__ int g711_mulaw(unsigned b) {
    const unsigned u = ~b & 255u;
    const int t = (int)((((u & 15u) << 3) + 132u) << ((u >> 4) & 7u));
    return (u & 128u) ? 132 - t : t - 132;
}
__host__ __device__ __forceinline__ int g711_alaw(unsigned b) {
    const unsigned a = (b ^ 0x55u) & 255u, s = (a >> 4) & 7u;
    int t = (int)((a & 15u) << 4);
    t = s == 0 ? t + 8 : (t + 0x108) << (s - 1);
    return (a & 128u) ? t : -t;
}

// the 8-bit formats are the live path's (wlx_ring_set_format); every value is exact in float32
template <int FMT>
__device__ __forceinline__ float rs_sample(const void* raw, long long idx) {
    if (FMT == WLX_PCM_S16) return (float)reinterpret_cast<const short*>(raw)[idx] * (1.0f / 32768.0f);
    if (FMT == WLX_PCM_U8) return (float)((int)reinterpret_cast<const unsigned char*>(raw)[idx] - 128) * (1.0f / 128.0f);
    if (FMT == WLX_PCM_MULAW) return (float)g711_mulaw(reinterpret_cast<const unsigned char*>(raw)[idx]) * (1.0f / 32768.0f);
    if (FMT == WLX_PCM_ALAW) return (float)g711_alaw(reinterpret_cast<const unsigned char*>(raw)[idx]) * (1.0f / 32768.0f);
    return reinterpret_cast<const float*>(raw)[idx];
}

inline size_t rs_lds_bytes(int up, int down, int half_len, int tile) {
    const long long span = ((long long)(tile - 1) * down + 2LL * half_len) / up + 2;
    return (size_t)(2 * half_len + 1 + span) * sizeof(float);
}

}  // namespace wlx
