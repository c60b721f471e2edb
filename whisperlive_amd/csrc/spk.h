// spk.h — launchers of the gfx950 kernels of the speaker-embedding engine (spk.hip; engine in spk_engine.hip): the Kaldi
// filterbank front end of WeSpeaker, the ResNet convolutions as implicit GEMMs on mfma_f32_16x16x32_f16, statistics pooling
// and the embedding head. Activations are NHWC fp16 ([H = frequency][W = time][C]), accumulation is fp32.
#pragma once
#include "../../include/wlx.h"          // WLX_SPK_MAX_BATCH: items of one ragged batch (their table travels in the kernel arguments)
#include "kernels.h"

namespace wlx {

#define WLX_SPK_FRAME 400        // 25 ms at 16 kHz
#define WLX_SPK_SHIFT 160        // 10 ms
#define WLX_SPK_NFFT 512
#define WLX_SPK_BINS 256         // Kaldi's mel banks leave the Nyquist bin out
#define WLX_SPK_MIN_SAMPLES 4800 // 0.3 s: what the reference's SpeakerDiarizer refuses to embed

// frames of a snip_edges filterbank over n samples (0 below one frame)
inline int spk_frames(long n) { return n < WLX_SPK_FRAME ? 0 : 1 + (int)((n - WLX_SPK_FRAME) / WLX_SPK_SHIFT); }

// ---- every launcher takes a ragged batch: n in 1..WLX_SPK_MAX_BATCH items of different lengths in one launch, packed back to back
// without padding (a single embed is n = 1). At a stage of geometry (H, C) item i is its own [H][W_i][C] image at pixel offset
// H * sum_{j<i} W_j; a stride-s convolution gives OW_i = (W_i - 1) / s + 1 per item. An item's output does not depend on its
// neighbours, its position or n; no tap reads a neighbouring item. `widths` / `frames` / `offsets` are HOST arrays, read before the
// call returns. False = nothing launched.

// Kaldi fbank: frame t of item i = pcm[offsets[i] + 160 t .. + 400) * 2^15, DC removed, pre-emphasis 0.97, Hamming window, 512-point
// power spectrum (direct DFT against `twiddle` = cos(2 pi j / 512), j = 0..511, fp32), n_mels triangular bins `mel` [n_mels][256],
// natural log with a float32-epsilon floor -> logmel fp32 [sum frames][n_mels], rows in item order. `window` [400].
bool launch_spk_fbank_batch(const float* pcm, const long* offsets, const int* frames, int n, const float* window, const float* twiddle,
                            const float* mel, int n_mels, float* logmel, hipStream_t s);
// per item and bin, the mean over the item's own frames subtracted in place; the fp16 copy goes to out16, item i = [n_mels][frames[i]]
// at n_mels * sum_{j<i} frames[j]: the [H][W][1] image the first convolution reads
bool launch_spk_cmn_batch(float* logmel, const int* frames, int n, int n_mels, half_t* out16, hipStream_t s);

// Convolution, ks = 3 (padding 1) or 1 (padding 0), stride 1 or 2: per item in [H][W][Cin] -> out [OH][OW][Cout] with
// OH = (H - 1) / stride + 1, OW likewise. Wp: the weight w[Cout][Cin][ks][ks] packed by spk_pack_conv into MFMA fragment order
// (common.h) over k = (kh * ks + kw) * Cin + ci. out = act(conv + bias [+ resid]), resid [OH][OW][Cout]. Cin and Cout multiples
// of 32. bias [Cout] is required (zeros for a convolution without one), resid may be null. Returns false (nothing launched) for
// a shape it cannot serve (an item of more than 2^30 output pixels among them) or a null in / Wp / bias / out.
bool launch_spk_conv_batch(const half_t* in, int H, const int* widths, int n, int Cin, const half_t* Wp, const float* bias,
                           const half_t* resid, int Cout, int stride, int ks, bool relu, half_t* out, hipStream_t s);
// the same for Cin = 1, ks = 3 on the vector ALU: w fp32 [Cout][9], Cout a multiple of 4
bool launch_spk_conv_c1_batch(const half_t* in, int H, const int* widths, int n, const float* w, const float* bias, const half_t* resid,
                              int Cout, int stride, bool relu, half_t* out, hipStream_t s);
// host side: w fp32 [Cout][Cin][ks][ks] -> fragment order, ks * ks * Cin / 32 k-tiles per 16 output channels
void spk_pack_conv(const float* w, int Cout, int Cin, int ks, half_t* Wp);
inline size_t spk_packed_halfs(int Cout, int Cin, int ks) { return (size_t)(Cout / 16) * (size_t)(ks * ks * Cin / 32) * 512; }

// Statistics pooling of x, item i = [F][frames[i]][C], over its frames (frames[i] >= 2): out [n][2][C][F],
// out[i][c * F + f] = mean, out[i][C * F + c * F + f] = sqrt(var_unbiased + eps). C a multiple of 64.
bool launch_spk_pool_batch(const half_t* x, int F, const int* frames, int n, int C, float eps, float* out, hipStream_t s);
// pooled [n][D] -> emb [n][E]: emb = W pooled + b (W fp16 [E][D] row-major, D a multiple of 8), then emb /= |emb| (an all-zero row
// stays zero) unless `normalize` is false. False, before any launch: a null pointer, n < 1, E < 1, D < 8 or D % 8.
bool launch_spk_head_batch(const float* pooled, const half_t* W, const float* b, int E, int D, int n, float* emb, hipStream_t s,
                           bool normalize = true);

// ---- offline clustering (spk_cluster.hip), everything float32: every launch serves a table of 1..WLX_SPK_MANY_MAX_FILES files (one file
// is a table of one), every file 1..WLX_SPK_CLUSTER_MAX unit rows of D <= 1024 floats. File i is rows [row0, row0 + m) of ONE table X and
// owns the m x m matrix at dist + doff; the rows of all files end inside WLX_SPK_MANY_MAX_ROWS and the matrices inside
// WLX_SPK_MANY_MAX_CELLS floats (the caller lays them out without overlap). `files` is a HOST array read before the call returns: the
// table travels in the kernel arguments. A file's results do not depend on the files around it. False = nothing launched (a null
// pointer, a count or shape out of range, a threshold that is NaN or outside [0, 2], max_clusters < 0).
struct SpkClusterFile {
    size_t doff;           // first float of the file's matrix
    int row0, m;
    float threshold;       // read by launch_spk_ahc only, as max_clusters
    int max_clusters;
};
struct SpkClusterTable {
    int n;
    SpkClusterFile f[WLX_SPK_MANY_MAX_FILES];
};
// per file, dist [m][m] = 1 - X X^T, exactly symmetric, diagonal exactly 0
bool launch_spk_affinity(const float* X, const SpkClusterFile* files, int n_files, int D, float* dist, hipStream_t s);
// average-linkage clustering of every file's matrix IN PLACE, one workgroup per file (the rules: include/wlx.h wlx_spk_cluster).
// labels [rows] and heights [rows]: file i at row0 (m - 1 heights at the most); merges [2 * rows]: at 2 * row0; counts [n_files][2] =
// {n_merges, K} per file
bool launch_spk_ahc(float* dist, const SpkClusterFile* files, int n_files, int* merges, float* heights, int* labels, int* counts,
                    hipStream_t s);
// cent [rows][D]: the normalised sum of each cluster's rows, file i's K_i = counts[i][1] (read on the device) centroids at rows
// row0 .. row0 + K_i - 1
bool launch_spk_centroids(const float* X, const int* labels, const int* counts, const SpkClusterFile* files, int n_files, int D,
                          float* cent, hipStream_t s);

}  // namespace wlx
