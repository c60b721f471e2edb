// spk_cluster.hip — offline speaker clustering on the device (launchers in spk.h; entry points in spk_engine.hip):
// the cosine-distance matrix of n <= WLX_SPK_CLUSTER_MAX unit embeddings, average-linkage (UPGMA) agglomerative clustering of that
// matrix in ONE launch of ONE workgroup, and the unit centroids of the clusters. Everything is float32: the merge threshold sits where
// fp16 noise would flip merges. The clustering is exact: tests/ compare merges, heights and labels with the NumPy float32 restatement
// (whisperlive_amd/file_diarization.py cluster_host) for equality. Every kernel works over a table of 1..WLX_SPK_MANY_MAX_FILES files
// that travels in its arguments: wlx_spk_cluster and wlx_spk_diarize_pcm launch a table of one file, wlx_spk_diarize_many
// a wave's. A file's results depend on its own rows and options only, not on the table around it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "spk.h"

namespace wlx {
namespace {

// ------------------------------------------------------------------------------------------------ distance matrix
// Dist[i][j] = 1 - dot(X_i, X_j): a 64 x 64 tile per workgroup of 256 threads (4 x 4 outputs each), K in slices of 16 through LDS.
// Every dot product is ONE chain of fmaf over k = 0 .. D-1 in order, whichever tile it lies in, and a * b = b * a: Dist[i][j] and
// Dist[j][i] have the same bits. The diagonal is written as 0, not computed. File f = blockIdx.z is rows [row0, row0 + m) of one table
// and writes its own m x m matrix at dist + doff; the grid's tiles cover the largest file and a workgroup whose tile lies outside its file
// leaves (workgroup-uniform, before any barrier).
constexpr int AFF_TILE = 64, AFF_K = 16, AFF_THREADS = 256;

__device__ __forceinline__ void spk_affinity_tile(const float* __restrict__ X, int n, int D, float* __restrict__ dist, int i0, int j0) {
    __shared__ float sa[AFF_K][AFF_TILE + 1], sb[AFF_K][AFF_TILE + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += AFF_K) {
        for (int e = threadIdx.x; e < AFF_TILE * AFF_K; e += AFF_THREADS) {
            const int r = e >> 4, k = e & 15, gk = k0 + k;
            sa[k][r] = (i0 + r < n && gk < D) ? X[(size_t)(i0 + r) * D + gk] : 0.f;
            sb[k][r] = (j0 + r < n && gk < D) ? X[(size_t)(j0 + r) * D + gk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < AFF_K; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = sa[k][ty * 4 + u], b[u] = sb[k][tx * 4 + u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < n && j < n) dist[(size_t)i * n + j] = i == j ? 0.f : 1.f - acc[u][v];
        }
}

// (the tile stays a function of its own: folded into the kernel the compiler allots 78 VGPRs, not the 80 of this form — another schedule
// of the same arithmetic, which nobody has timed)
__global__ __launch_bounds__(AFF_THREADS) void spk_affinity_kernel(const float* __restrict__ X, SpkClusterTable tab, int D,
                                                                    float* __restrict__ dist) {
    const SpkClusterFile f = tab.f[blockIdx.z];
    const int i0 = blockIdx.y * AFF_TILE, j0 = blockIdx.x * AFF_TILE;
    if (i0 >= f.m || j0 >= f.m) return;
    spk_affinity_tile(X + (size_t)f.row0 * D, f.m, D, dist + f.doff, i0, j0);
}

// ------------------------------------------------------------------------------------------------ UPGMA, one workgroup
constexpr int AHC_THREADS = 1024, AHC_WAVES = AHC_THREADS / 64;

// the Lance-Williams update of average linkage, each operation rounded on its own (no contraction into an fma): the NumPy float32
// expression (n_i * d_ki + n_j * d_kj) / (n_i + n_j) bit for bit. Plain operators under the pragma, NOT __fmul_rn / __fadd_rn: this
// ROCm's header defines those as `x * y` / `x + y` in functions of their own, compiled under hipcc's default -ffp-contract=fast, so
// after inlining the product and the sum still carry the contract flag and the backend fuses them (v_mul_f32 + v_fmac_f32, seen in the
// ISA; heights one ulp off the oracle's in the late merges). The division is hipcc's correctly rounded one (v_div_scale / v_div_fmas /
// v_div_fixup, denormals kept).
__device__ __forceinline__ float upgma(float ni, float dki, float nj, float dkj) {
#pragma clang fp contract(off)
    const float a = ni * dki, b = nj * dkj;
    const float s = a + b, t = ni + nj;
    return s / t;
}

// One wave: the nearest live neighbour ABOVE row k, the smallest (distance, j) over live j > k; (inf, n) when there is none.
__device__ __forceinline__ void ahc_scan_row(const float* dist, int n, int k, const uint16_t* size, float* nnd, uint16_t* nn, int lane) {
    const float* row = dist + (size_t)k * n;
    float bd = INFINITY;
    int bj = n;
    for (int j = k + 1 + lane; j < n; j += 64)          // (a lane sees its columns in rising order: '<' keeps the lowest on a tie)
        if (size[j]) {
            const float d = row[j];
            if (d < bd) bd = d, bj = j;
        }
    for (int off = 32; off; off >>= 1) {
        const float od = __shfl_down(bd, off);
        const int oj = __shfl_down(bj, off);
        if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    if (lane == 0) nnd[k] = bd, nn[k] = (uint16_t)bj;
}

// One workgroup per file, blockIdx.x = file: the clusterings are independent, so they run on as many CUs at once (24 KiB of LDS and 1024
// threads per workgroup: two may share a CU). File f clusters its matrix at dist + doff (n = m) under its own threshold and max_clusters;
// labels and heights are written at row0, merges at 2 * row0 (room for m each), counts at [f][2].
// dist [n][n] symmetric, clustered IN PLACE (rows and columns of merged clusters are overwritten). Clusters are named by their lowest
// member. Each round merges the pair (i, j), i < j, of live clusters with the smallest (distance, i, j); it stops at one cluster, or
// when that distance is > threshold and (max_clusters == 0 or live <= max_clusters). The minimum comes from a per-row cache of the
// nearest neighbour above the row (nn, nnd in LDS): the best pair with i as its lower member is (nnd[i], i, nn[i]), so the minimum of
// those over i is the exhaustive minimum with the tie rule. After a merge a row is rescanned (one wave per row) when its cached
// neighbour was i or j or when it is row i itself, and takes the new d(k, i) when that beats its cache; rows above j see no change.
// The loop runs at most n - 1 times and waits on nothing but __syncthreads.
// out: merges [n_merges][2], heights [n_merges], labels [n] (clusters numbered by lowest member, ascending), counts = {n_merges, K}.
__global__ __launch_bounds__(AHC_THREADS) void spk_ahc_kernel(float* __restrict__ dist, SpkClusterTable tab, int* __restrict__ merges,
                                                             float* __restrict__ heights, int* __restrict__ labels,
                                                             int* __restrict__ counts) {
    const SpkClusterFile f = tab.f[blockIdx.x];
    const int n = f.m, max_clusters = f.max_clusters;
    const float threshold = f.threshold;
    dist += f.doff, merges += 2 * (size_t)f.row0, heights += f.row0, labels += f.row0, counts += 2 * blockIdx.x;
    __shared__ uint16_t size[WLX_SPK_CLUSTER_MAX], nn[WLX_SPK_CLUSTER_MAX], parent[WLX_SPK_CLUSTER_MAX], todo[WLX_SPK_CLUSTER_MAX];
    __shared__ float nnd[WLX_SPK_CLUSTER_MAX];
    __shared__ float red_d[AHC_WAVES];
    __shared__ int red_i[AHC_WAVES];
    __shared__ int n_todo, best_i;
    __shared__ float best_d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < n; k += AHC_THREADS) size[k] = 1, parent[k] = (uint16_t)k;
    if (tid == 0) n_todo = 0;
    __syncthreads();
    for (int k = wave; k < n; k += AHC_WAVES) ahc_scan_row(dist, n, k, size, nnd, nn, lane);
    __syncthreads();
    int live = n, n_merges = 0;
    for (int round = 0; round < n - 1; ++round) {
        // the smallest (nnd[i], i) over live rows
        float bd = INFINITY;
        int bi = n;
        for (int k = tid; k < n; k += AHC_THREADS)
            if (size[k] && nnd[k] < bd) bd = nnd[k], bi = k;          // (rising k: '<' keeps the lowest row on a tie)
        for (int off = 32; off; off >>= 1) {
            const float od = __shfl_down(bd, off);
            const int oi = __shfl_down(bi, off);
            if (od < bd || (od == bd && oi < bi)) bd = od, bi = oi;
        }
        if (lane == 0) red_d[wave] = bd, red_i[wave] = bi;
        __syncthreads();
        if (wave == 0) {
            bd = lane < AHC_WAVES ? red_d[lane] : INFINITY;
            bi = lane < AHC_WAVES ? red_i[lane] : n;
            for (int off = AHC_WAVES / 2; off; off >>= 1) {
                const float od = __shfl_down(bd, off);
                const int oi = __shfl_down(bi, off);
                if (od < bd || (od == bd && oi < bi)) bd = od, bi = oi;
            }
            if (lane == 0) best_d = bd, best_i = bi;
        }
        __syncthreads();
        bd = best_d, bi = best_i;
        if (bi >= n) break;                                            // (no finite pair: every thread reads the same values)
        const int bj = nn[bi];
        if (bj >= n) break;
        if (bd > threshold && (max_clusters == 0 || live <= max_clusters)) break;
        const float ni = (float)size[bi], nj = (float)size[bj];
        __syncthreads();                                               // every thread holds the pair and its sizes before they change
        const float *ri = dist + (size_t)bi * n, *rj = dist + (size_t)bj * n;
        for (int k = tid; k < n; k += AHC_THREADS) {
            if (k == bi || k == bj || !size[k]) continue;
            const float d = upgma(ni, ri[k], nj, rj[k]);
            dist[(size_t)bi * n + k] = d;
            dist[(size_t)k * n + bi] = d;
            if (k < bi) {
                const int c = nn[k];
                if (c == bi || c == bj) todo[atomicAdd(&n_todo, 1)] = (uint16_t)k;
                else if (d < nnd[k] || (d == nnd[k] && bi < c)) nnd[k] = d, nn[k] = (uint16_t)bi;
            } else if (k < bj && nn[k] == bj) {
                todo[atomicAdd(&n_todo, 1)] = (uint16_t)k;
            }
        }
        if (tid == 0) {
            merges[2 * n_merges] = bi, merges[2 * n_merges + 1] = bj;
            heights[n_merges] = bd;
            size[bi] = (uint16_t)(size[bi] + size[bj]), size[bj] = 0, parent[bj] = (uint16_t)bi;
            todo[atomicAdd(&n_todo, 1)] = (uint16_t)bi;
        }
        ++n_merges, --live;
        __syncthreads();
        const int nt = n_todo;                                         // at most one entry per live row: <= n
        for (int t = wave; t < nt; t += AHC_WAVES) ahc_scan_row(dist, n, todo[t], size, nnd, nn, lane);
        __syncthreads();
        if (tid == 0) n_todo = 0;                                      // (the next pushes come two barriers later)
    }
    __syncthreads();
    // number the live clusters by lowest member (nn is free now), then every row follows its parents to a live one
    for (int k = tid; k < n; k += AHC_THREADS)
        if (size[k]) {
            int r = 0;
            for (int q = 0; q < k; ++q) r += size[q] != 0;
            nn[k] = (uint16_t)r;
        }
    __syncthreads();
    for (int k = tid; k < n; k += AHC_THREADS) {
        int r = k;
        while (!size[r]) r = parent[r];                                // (parent[r] < r: ends at a live row after at most n steps)
        labels[k] = nn[r];
    }
    if (tid == 0) counts[0] = n_merges, counts[1] = live;
}

// ------------------------------------------------------------------------------------------------ centroids
// grid (cluster, file): cluster c = blockIdx.x of file f = blockIdx.y (blocks past K = counts[f][1], and past m, leave): the sum of its
// members' rows in member order, divided by its norm, to row row0 + c of cent
__global__ __launch_bounds__(256) void spk_centroid_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                           const int* __restrict__ counts, SpkClusterTable tab, int D,
                                                           float* __restrict__ cent) {
    const SpkClusterFile f = tab.f[blockIdx.y];
    const int c = blockIdx.x, n = f.m;
    if (c >= n || c >= counts[2 * blockIdx.y + 1]) return;
    X += (size_t)f.row0 * D, labels += f.row0, cent += (size_t)f.row0 * D;
    __shared__ float red[256];
    float sq = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
        for (int m = 0; m < n; ++m)
            if (labels[m] == c) s += X[(size_t)m * D + d];
        cent[(size_t)c * D + d] = s;
        sq = fmaf(s, s, sq);
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const float norm = sqrtf(red[0]);
    if (norm > 0.f)
        for (int d = threadIdx.x; d < D; d += 256) cent[(size_t)c * D + d] /= norm;      // (each thread rereads what it wrote itself)
}

bool cluster_shape_ok(int n, int D) { return n >= 1 && n <= WLX_SPK_CLUSTER_MAX && D >= 1 && D <= 1024; }

}  // namespace

// the table of a launch: every file 1..WLX_SPK_CLUSTER_MAX rows of D <= 1024, rows and matrices inside the caps
static bool cluster_table(const SpkClusterFile* files, int n_files, int D, bool with_opts, SpkClusterTable& tab, int& max_m) {
    if (!files || n_files < 1 || n_files > WLX_SPK_MANY_MAX_FILES) return false;
    size_t cells = 0;
    long rows = 0;
    max_m = 0;
    tab.n = n_files;
    for (int i = 0; i < n_files; ++i) {
        const SpkClusterFile& f = files[i];
        if (!cluster_shape_ok(f.m, D) || f.row0 < 0) return false;
        if (with_opts && (!(f.threshold >= 0.f && f.threshold <= 2.f) || f.max_clusters < 0)) return false;
        rows = std::max(rows, (long)f.row0 + f.m);
        cells = std::max(cells, f.doff + (size_t)f.m * f.m);
        max_m = std::max(max_m, f.m);
        tab.f[i] = f;
    }
    return rows <= WLX_SPK_MANY_MAX_ROWS && cells <= WLX_SPK_MANY_MAX_CELLS;
}

bool launch_spk_affinity(const float* X, const SpkClusterFile* files, int n_files, int D, float* dist, hipStream_t s) {
    SpkClusterTable tab;
    int max_m;
    if (!X || !dist || !cluster_table(files, n_files, D, false, tab, max_m)) return false;
    const int t = (max_m + AFF_TILE - 1) / AFF_TILE;
    spk_affinity_kernel<<<dim3(t, t, n_files), AFF_THREADS, 0, s>>>(X, tab, D, dist);
    return true;
}

bool launch_spk_ahc(float* dist, const SpkClusterFile* files, int n_files, int* merges, float* heights, int* labels, int* counts,
                    hipStream_t s) {
    SpkClusterTable tab;
    int max_m;
    if (!dist || !merges || !heights || !labels || !counts || !cluster_table(files, n_files, 1, true, tab, max_m)) return false;
    spk_ahc_kernel<<<n_files, AHC_THREADS, 0, s>>>(dist, tab, merges, heights, labels, counts);
    return true;
}

bool launch_spk_centroids(const float* X, const int* labels, const int* counts, const SpkClusterFile* files, int n_files, int D,
                          float* cent, hipStream_t s) {
    SpkClusterTable tab;
    int max_m;
    if (!X || !labels || !counts || !cent || !cluster_table(files, n_files, D, false, tab, max_m)) return false;
    spk_centroid_kernel<<<dim3(max_m, n_files), 256, 0, s>>>(X, labels, counts, tab, D, cent);
    return true;
}

}  // namespace wlx
