// frontend.h — what the file front ends show each other: the host index of a FLAC stream (flac.hip) and of a telephony WAV file
// (adpcm.hip), their refusals, and the launches that need no wait. put_many.hip builds a wave of files out of them; each single-file
// entry point keeps using its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/wlx.h"
#include "adpcm_core.h"

namespace wlx {

// ---- flac.hip
// bytes [start, end), first sample, block size. `pad` is unused by the single-file kernels; the ragged form keeps the frame's entry there
struct FlacFrame { long long start, end, first; int n, pad; };
struct FlacStream {
    wlx_flac_info info{};
    std::vector<FlacFrame> frames;
};
int flac_index(const uint8_t* b, long long nbytes, FlacStream& out);      // metadata + frame table, nothing decoded
int flac_served(const FlacStream& s);                                     // WLX_ERR_ARG with the reason unless info.served
int flac_check_status(const int* status, size_t nf);                      // WLX_ERR_DATA naming the first frame that did not decode

// ---- adpcm.hip
constexpr int WAV_TAG_MS = 0x02, WAV_TAG_ALAW = 0x06, WAV_TAG_MULAW = 0x07, WAV_TAG_IMA = 0x11, WAV_TAG_EXT = 0xFFFE;
struct WavStream {
    wlx_wav_info info{};
    int kind = -1;                  // ADPCM_IMA / ADPCM_MS; -1: not an ADPCM tag
    bool layout_ok = false;         // ADPCM: bits == 4 and a block_align the formulas accept
    int n_coef = 0;
    int16_t coefs[2 * ADPCM_MAX_COEF] = {};
};
int wav_index(const uint8_t* b, long long n, WavStream& out);
int wav_served(const WavStream& w);
long long adpcm_blocks(const WavStream& w);                               // the blocks the frame count needs
// the decode launch on `st`, no wait: d_bytes = the data chunk's first adpcm_blocks(w) blocks (4-byte aligned, readable to the next
// multiple of 4), out = float32 [n_frames][channels]
int adpcm_launch_f32(const WavStream& w, const uint8_t* d_bytes, float* out, hipStream_t st);

}  // namespace wlx
