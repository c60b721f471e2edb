// spk_cluster.hip — offline speaker clustering on the device (launchers in spk.h; entry points in spk_engine.hip):
// the cosine-distance matrix of n <= WLX_SPK_CLUSTER_MAX unit embeddings, average-linkage (UPGMA) agglomerative clustering of that
// matrix in ONE launch of ONE workgroup, and the unit centroids of the clusters. Everything is float32: the merge threshold sits where
// fp16 noise would flip merges. The clustering is exact: tests/ compare merges, heights and labels with the NumPy float32 restatement
// (whisperlive_amd/file_diarization.py cluster_host) for equality. Every kernel works over a table of 1..WLX_SPK_MANY_MAX_FILES files
// that travels in its arguments: wlx_spk_cluster and wlx_spk_diarize_pcm launch a table of one file, wlx_spk_diarize_many
// a wave's. A file's results depend on its own rows and options only, not on the table around it.
// The long form (spk_ahc_long_kernel and the *_long launchers) clusters ONE file of up to WLX_SPK_LONG_MAX rows by the
// same rules, with the same bits.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
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

// ------------------------------------------------------------------------------------------------ UPGMA, long form
// spk_ahc_long_kernel: the same clustering for ONE file of up to WLX_SPK_LONG_MAX rows, still one workgroup of 1024 threads that waits
// on nothing but __syncthreads and loops at most n - 1 times. Same rules, same arithmetic (upgma above), same results bit for bit; what
// differs is how the work is laid out, because at these sizes the matrix (256 MiB at the cap) lives in HBM, not in the L2:
//  * state in DYNAMIC LDS, 12 n bytes (96 KiB at the cap, past the 64 KiB default: the launcher raises the limit): nnd float[n], then
//    size, nn, the work list and the list of live rows as uint16_t[n] each. `parent` is read by the labelling alone and lives in global
//    memory until then.
//  * `list`: the live rows in ascending order, possibly with dead entries between them (size == 0, skipped). It is compacted by a
//    workgroup prefix sum whenever the live count has fallen to half its length (at most 13 times), so the minimum reduction, the update
//    and the rescans walk ~1.5 live entries per live row instead of n.
//  * the update holds a thread's columns in registers: all loads of rows i and j first (up to AHC_LONG_COLS per row and thread, issued
//    together: one memory latency per round, not one per column), then the arithmetic and the stores.
//  * row i's new nearest neighbour comes out of those registers — the smallest (d, k) over its live k > i, by wave shuffle and one LDS
//    step — not from a rescan that reads back what was just stored. Every thread folds the 16 wave results itself and carries the
//    result into the next round's reduction (`fresh_d` stands for nnd[i] there: thread 0's store to LDS may not have landed), so a
//    round whose work list is empty has no rescan phase and no barrier for it.
constexpr int AHC_LONG_COLS = WLX_SPK_LONG_MAX / AHC_THREADS;

// one wave, all rows live: the first scan of row k, eight loads in flight per lane
__device__ __forceinline__ void ahc_long_first_row(const float* dist, int n, int k, float* nnd, uint16_t* nn, int lane) {
    const float* row = dist + (size_t)k * n;
    float bd = INFINITY;
    int bj = n;
    for (int j0 = k + 1 + lane; j0 < n; j0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = j0 + 64 * u < n ? row[j0 + 64 * u] : INFINITY;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (v[u] < bd) bd = v[u], bj = j0 + 64 * u;                  // (rising j per lane: '<' keeps the lowest on a tie)
    }
    for (int off = 32; off; off >>= 1) {
        const float od = __shfl_down(bd, off);
        const int oj = __shfl_down(bj, off);
        if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    if (lane == 0) nnd[k] = bd, nn[k] = (uint16_t)bj;
}

// one wave: ahc_scan_row over the list — the entries above k start at the first list position whose row is > k — four loads in flight
__device__ __forceinline__ void ahc_long_scan_row(const float* dist, int n, int k, const uint16_t* list, int L, const uint16_t* size,
                                                  float* nnd, uint16_t* nn, int lane) {
    const float* row = dist + (size_t)k * n;
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    float bd = INFINITY;
    int bj = n;
    for (int t0 = lo + lane; t0 < L; t0 += 64 * 4) {
        float v[4];
        int j[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 64 * u;
            j[u] = t < L ? list[t] : n;
            v[u] = (t < L && size[j[u]]) ? row[j[u]] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v[u] < bd) bd = v[u], bj = j[u];                         // (the list ascends: rising j per lane)
    }
    for (int off = 32; off; off >>= 1) {
        const float od = __shfl_down(bd, off);
        const int oj = __shfl_down(bj, off);
        if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    if (lane == 0) nnd[k] = bd, nn[k] = (uint16_t)bj;
}

// the whole workgroup: list[0 .. L) without its dead entries, order kept, through `tmp`; returns the new length. A thread owns a run of
// consecutive entries, the runs' live counts are summed by an inclusive wave scan and the 16 wave totals.
__device__ __forceinline__ int ahc_long_compact(uint16_t* list, uint16_t* tmp, const uint16_t* size, int L, int* wave_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (L + AHC_THREADS - 1) / AHC_THREADS, t0 = min(L, tid * per), t1 = min(L, t0 + per);
    int cnt = 0;
    for (int t = t0; t < t1; ++t) cnt += size[list[t]] != 0;
    int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off);
        if (lane >= off) inc += v;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int at = inc - cnt, total = 0;
    for (int w = 0; w < AHC_WAVES; ++w) {
        const int v = wave_tot[w];
        if (w < wave) at += v;
        total += v;
    }
    for (int t = t0; t < t1; ++t) {
        const uint16_t k = list[t];
        if (size[k]) tmp[at++] = k;
    }
    __syncthreads();
    for (int t = tid; t < total; t += AHC_THREADS) list[t] = tmp[t];
    __syncthreads();
    return total;
}

// dist [n][n] symmetric, clustered IN PLACE; parent: n entries of scratch; out as spk_ahc_kernel's: merges [n_merges][2], heights
// [n_merges], labels [n], counts = {n_merges, K}
__global__ __launch_bounds__(AHC_THREADS) void spk_ahc_long_kernel(float* __restrict__ dist, int n, float threshold, int max_clusters,
                                                                  uint16_t* __restrict__ parent, int* __restrict__ merges,
                                                                  float* __restrict__ heights, int* __restrict__ labels,
                                                                  int* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char ahc_long_lds[];
    float* nnd = reinterpret_cast<float*>(ahc_long_lds);
    uint16_t *size = reinterpret_cast<uint16_t*>(nnd + n), *nn = size + n, *todo = nn + n, *list = todo + n;
    __shared__ float red_d[AHC_WAVES], row_d[AHC_WAVES];
    __shared__ int red_i[AHC_WAVES], row_k[AHC_WAVES], wave_tot[AHC_WAVES];
    __shared__ int n_todo, best_i;
    __shared__ float best_d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < n; k += AHC_THREADS) size[k] = 1, list[k] = (uint16_t)k;
    if (tid == 0) n_todo = 0;
    __syncthreads();
    for (int k = wave; k < n; k += AHC_WAVES) ahc_long_first_row(dist, n, k, nnd, nn, lane);
    __syncthreads();
    int live = n, L = n, n_merges = 0, fresh_i = n;
    float fresh_d = INFINITY;
    for (int round = 0; round < n - 1; ++round) {
        if (2 * live <= L) L = ahc_long_compact(list, todo, size, L, wave_tot);      // (the work list is empty between rounds)
        // the smallest (nnd[i], i) over live rows
        float bd = INFINITY;
        int bi = n;
        for (int t = tid; t < L; t += AHC_THREADS) {
            const int k = list[t];
            if (!size[k]) continue;
            const float d = k == fresh_i ? fresh_d : nnd[k];
            if (d < bd) bd = d, bi = k;                                  // (rising k: '<' keeps the lowest row on a tie)
        }
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
        const int cols = (L + AHC_THREADS - 1) / AHC_THREADS;          // <= AHC_LONG_COLS
        int kk[AHC_LONG_COLS];
        float di[AHC_LONG_COLS], dj[AHC_LONG_COLS];
#pragma unroll
        for (int c = 0; c < AHC_LONG_COLS; ++c) {
            kk[c] = -1;
            if (c < cols) {
                const int t = tid + c * AHC_THREADS, k = t < L ? list[t] : bi;
                if (k != bi && k != bj && size[k]) kk[c] = k, di[c] = ri[k], dj[c] = rj[k];
            }
        }
        float rd = INFINITY;                                           // row i's nearest neighbour above it, from this thread's columns
        int rk = n;
#pragma unroll
        for (int c = 0; c < AHC_LONG_COLS; ++c) {
            const int k = kk[c];
            if (k < 0) continue;
            const float d = upgma(ni, di[c], nj, dj[c]);
            dist[(size_t)bi * n + k] = d;
            dist[(size_t)k * n + bi] = d;
            if (k < bi) {
                const int c0 = nn[k];
                if (c0 == bi || c0 == bj) todo[atomicAdd(&n_todo, 1)] = (uint16_t)k;
                else if (d < nnd[k] || (d == nnd[k] && bi < c0)) nnd[k] = d, nn[k] = (uint16_t)bi;
            } else {
                if (d < rd) rd = d, rk = k;                              // (rising k per thread)
                if (k < bj && nn[k] == bj) todo[atomicAdd(&n_todo, 1)] = (uint16_t)k;
            }
        }
        for (int off = 32; off; off >>= 1) {
            const float od = __shfl_down(rd, off);
            const int ok = __shfl_down(rk, off);
            if (od < rd || (od == rd && ok < rk)) rd = od, rk = ok;
        }
        if (lane == 0) row_d[wave] = rd, row_k[wave] = rk;
        if (tid == 0) {
            merges[2 * n_merges] = bi, merges[2 * n_merges + 1] = bj;
            heights[n_merges] = bd;
            size[bi] = (uint16_t)(size[bi] + size[bj]), size[bj] = 0, parent[bj] = (uint16_t)bi;
        }
        ++n_merges, --live;
        __syncthreads();
        rd = row_d[0], rk = row_k[0];                                  // (row_d is next written two barriers on)
        for (int w = 1; w < AHC_WAVES; ++w) {
            const float od = row_d[w];
            const int ok = row_k[w];
            if (od < rd || (od == rd && ok < rk)) rd = od, rk = ok;
        }
        fresh_d = rd, fresh_i = bi;
        if (tid == 0) nnd[bi] = rd, nn[bi] = (uint16_t)rk;             // (nn[bi] is next read two barriers on, nnd[bi] through fresh_d)
        const int nt = n_todo;                                         // at most one entry per live row other than i: < n
        if (nt) {
            for (int t = wave; t < nt; t += AHC_WAVES) ahc_long_scan_row(dist, n, todo[t], list, L, size, nnd, nn, lane);
            __syncthreads();
            if (tid == 0) n_todo = 0;                                  // (the next pushes come two barriers later)
        }
    }
    __syncthreads();
    // the compacted list numbers the live clusters by lowest member (nn is free now); parent comes into LDS (the work list's space)
    // so that the walk to a live row does not pay a memory latency per step
    L = ahc_long_compact(list, todo, size, L, wave_tot);
    for (int t = tid; t < L; t += AHC_THREADS) nn[list[t]] = (uint16_t)t;
    for (int k = tid; k < n; k += AHC_THREADS)
        if (!size[k]) todo[k] = parent[k];
    __syncthreads();
    for (int k = tid; k < n; k += AHC_THREADS) {
        int r = k;
        while (!size[r]) r = todo[r];                                  // (parent[r] < r: ends at a live row after at most n steps)
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

// ---- the long form: ONE file of 1..WLX_SPK_LONG_MAX rows at row 0 with a matrix of its own. The distance matrix and the centroids are
// the kernels above on a table of one file that only the cap of cluster_table would refuse (their offsets are 64-bit already).
static SpkClusterTable long_table(int m) {
    SpkClusterTable tab;
    tab.n = 1;
    tab.f[0] = SpkClusterFile{0, 0, m, 0.f, 0};
    return tab;
}
static bool long_shape_ok(int m, int D) { return m >= 1 && m <= WLX_SPK_LONG_MAX && D >= 1 && D <= 1024; }

bool launch_spk_affinity_long(const float* X, int m, int D, float* dist, hipStream_t s) {
    if (!X || !dist || !long_shape_ok(m, D)) return false;
    const int t = (m + AFF_TILE - 1) / AFF_TILE;
    spk_affinity_kernel<<<dim3(t, t, 1), AFF_THREADS, 0, s>>>(X, long_table(m), D, dist);
    return true;
}

bool launch_spk_ahc_long(float* dist, int n, float threshold, int max_clusters, uint16_t* parent, int* merges, float* heights, int* labels,
                         int* counts, hipStream_t s) {
    if (!dist || !parent || !merges || !heights || !labels || !counts || !long_shape_ok(n, 1)) return false;
    if (!(threshold >= 0.f && threshold <= 2.f) || max_clusters < 0) return false;
    // 12 n bytes of dynamic LDS, over the 64 KiB default from n = 5462 on: the limit is raised once per device
    static std::atomic<signed char> raised[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (!raised[dev].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&spk_ahc_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                12 * WLX_SPK_LONG_MAX) != hipSuccess)
            return false;
        raised[dev].store(1, std::memory_order_release);
    }
    spk_ahc_long_kernel<<<1, AHC_THREADS, (size_t)12 * n, s>>>(dist, n, threshold, max_clusters, parent, merges, heights, labels, counts);
    return true;
}

bool launch_spk_centroids_long(const float* X, const int* labels, const int* counts, int m, int D, float* cent, hipStream_t s) {
    if (!X || !labels || !counts || !cent || !long_shape_ok(m, D)) return false;
    spk_centroid_kernel<<<dim3(m, 1), 256, 0, s>>>(X, labels, counts, long_table(m), D, cent);
    return true;
}

}  // namespace wlx
