/* wlx_spk_long.h — the long form of the offline speaker clustering in the C-ABI of libwlx.so. Included by wlx.h (inside its extern "C"
 * block, behind the types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_SPK_LONG_H
#define WLX_SPK_LONG_H

/* ---- an hour of speech: one file of up to WLX_SPK_LONG_MAX windows clustered on the device ----
 * WLX_SPK_CLUSTER_MAX windows at a 0.75 s hop are 25.6 minutes of speech; a slot item holds an hour, about 4800 windows. The entry
 * points below are wlx_spk_cluster and wlx_spk_diarize_pcm for 1 <= n <= WLX_SPK_LONG_MAX: the rules of wlx_spk_cluster word for word
 * (pair choice by the smallest (distance, i, j), j merged into i, the average-linkage update with every operation rounded on its own,
 * the stop rule with max_clusters, labels by lowest member), the same arguments, outputs, statuses, shortcuts (n = 1 / m = 1 / m = 0)
 * and refusals, one wait per call — and for n <= WLX_SPK_CLUSTER_MAX the bits the short entry points return.
 * They ALWAYS run the long kernel, whatever n: spk_ahc_long_kernel (csrc/spk_cluster.hip), one workgroup of 1024 threads with 12 n bytes
 * of dynamic LDS, behind the distance-matrix and centroid kernels of the short form. One file per call; a wave of files
 * (wlx_spk_diarize_many) keeps WLX_SPK_CLUSTER_MAX per file.
 * Cost: rows, labels, heights, merges and the pinned staging are the tables the short form shares (wlx_spk_cluster's comment); the
 * matrix is a buffer of its own, allocated by the first long call at that call's m * m floats and grown (freed and allocated anew, on
 * an idle stream) when a later call needs more: 92 MiB of HBM at 4800 windows, 256 MiB at the cap, held until wlx_spk_destroy. An
 * engine that never gets a long call never pays. dist_out of wlx_spk_diarize_pcm_long is a download of that size. */
#define WLX_SPK_LONG_MAX 8192
int32_t wlx_spk_cluster_long(wlx_spk* spk, const float* emb, int32_t n, int32_t dim, const wlx_spk_cluster_opts* opts,
                             int32_t* labels, float* centroids, int32_t* n_clusters);
int32_t wlx_spk_diarize_pcm_long(wlx_spk* spk, wlx_engine* e, int32_t slot, int32_t item, const int64_t* starts, const int64_t* n_samples,
                                 int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels, int32_t* status, float* emb_out,
                                 float* dist_out, float* centroids, int32_t* n_clusters);

/* TEST hook: ONE launch of spk_ahc_long_kernel on a matrix. wlx_spk_debug_ahc's conventions for 1 <= n <= WLX_SPK_LONG_MAX: dist [n][n]
 * symmetric (uploaded; the clustered matrix is not written back) -> labels [n]; merges [n - 1][2] and heights [n - 1], copied in and
 * out, so what no merge writes comes back unchanged; *n_merges, *n_clusters. WLX_ERR_ARG before any launch and with nothing written: a
 * null pointer, n out of range, the options as wlx_spk_cluster refuses them. */
int32_t wlx_spk_debug_ahc_long(int32_t device, const float* dist, int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels,
                               int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters);

#endif /* WLX_SPK_LONG_H */
