// dec_lm.hip — n-gram language-model fusion: the one launch between the vocabulary projection and the token search of a decode step
// whose slot points at a model (wlx_lm_set). A step of a slot without one does not launch it. Two kernels share one body
// (lm_fuse_row): dec_lm_kernel under the slot's one descriptor, dec_lm_items_kernel under the pool entry selected for the row's item
// (wlx_lm_set_items / wlx_lm_select), described above it.
//
// The model is a backoff automaton over token ids, built on the host (whisperlive_amd/lm.py) and checked by lm_table.h: state 0 is the
// empty context with the dense unigram arrays; state n > 0 carries its sorted explicit edges (token, log-probability, next state), a
// backoff link to a strictly shorter context and that link's weight. Alphabet A = the text tokens 0 .. eot - 1 and eot.
//
// Semantics per row (whisperlive_amd/lm.py restates them in float64). State at position p:
//   - the start state while the fed token is a prompt token (p < plen or p < 1);
//   - the parent's state at p - 1 where the fed token is >= eot (specials and timestamps are transparent);
//   - otherwise `next` of the token's edge at the first level of the parent's backoff chain that has one, unigram_next[token] where none has.
//   A parent's state outside 0 .. n_states - 1 reads as the start state.
// Score s(v) in state n with chain n = c0 .. ck = 0: the edge's logp at the first level cj that has one plus the weights of c0 .. c(j-1),
// unigram_logp[v] plus all the chain's weights where none has. Fusion: l'(v) = l(v) + w s(v) - c over A, c = LSE_A(l + w s) - LSE_A(l).
// A row with st.nsp_row[r] > 0 writes its state and keeps its logits; a row without a finite logit in A keeps them too; ids above eot and
// the pad columns keep their bits.
//
// Unlike the bias, grammar and pattern launches this one is DENSE: every token of A gets a score in every context, and the normaliser
// needs two reductions over the row. Shape: ONE workgroup of 1024 threads per decoder row; the row is read once and written once.
//   1. every thread requests its share of the row — two 16-byte pieces per chunk of NGLM_CHUNK ids, up to 64 values — before anything
//      else: the loads are in flight while wave 0 resolves the state;
//   2. wave 0 resolves the row's state and gathers the chain (at most four contexts, their edge ranges and the weights above them) into
//      LDS. Every search in an edge list is a WAVE-wide 64-ary search (lm_lower_bound): one dependent load per factor of 64, four for
//      the largest list the caps allow, where a binary search would chain twenty-two;
//   3. the (level, chunk boundary) searches — where each level's edge list crosses a multiple of NGLM_CHUNK — are dealt over the sixteen
//      waves and left in LDS, so the chunk loop below does no search at all;
//   4. per chunk of 8192 ids, 32 KB of LDS: filled with unigram + all weights (16-byte loads: the unigram array is padded to whole
//      chunks), then level by level from the shortest context to the longest the level's edges of the chunk are scattered over it (a
//      barrier behind every level that had edges: the longer context wins), then each thread takes its 8 scores and forms l + w s in
//      place of the 8 raw logits it holds. Both log-sum-exps run online per thread (max and sum, rescaled per chunk);
//   5. the fused values of the whole row stay in registers — compile-time indexing, the chunk loop fully unrolled; at most 64 a thread
//      for a vocabulary of 65536 — so after one workgroup reduction (wave shuffles, sixteen partials through LDS) c is subtracted and the
//      row is stored with 16-byte stores. No second pass over global memory, no scratch.
#include "decoder.h"
#include "host.h"
#include "lm_table.h"

namespace wlx {

#define NGLM_THREADS 1024
#define NGLM_WAVES (NGLM_THREADS / 64)
#define NGLM_CHUNK 8192                                         // ids whose scores are in LDS at a time
#define NGLM_MAX_CHUNKS (NGLM_MAX_VOCAB / NGLM_CHUNK)           // 8
#define NGLM_PIECES (NGLM_CHUNK / 4 / NGLM_THREADS)             // 16-byte pieces per thread and chunk: 2
#define NGLM_LEVELS (NGLM_MAX_ORDER - 1)                        // contexts of a chain (the unigram level is dense)

// first index in [lo, hi) whose token is >= t, hi where none is: the tokens ascend. Wave-wide: the 64 lanes probe 64 evenly spaced
// entries, the ballot cuts the range by 64 per dependent load. lo, hi, t and the result are uniform in the wave; all lanes take part.
__device__ __forceinline__ int lm_lower_bound(const int* __restrict__ tokv, int lo, int hi, int t, int lane) {
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int i = lo + lane * step;
        const int k = __popcll(__ballot(i < hi && tokv[i] < t));        // (the lanes below t are a prefix)
        if (k == 0) return lo;
        const int nlo = lo + (k - 1) * step + 1;
        hi = min(hi, lo + k * step);
        lo = nlo;
    }
    const int i = lo + lane;
    return lo + __popcll(__ballot(i < hi && tokv[i] < t));
}

// (m, s): the maximum and the sum of exp(x - m) of the values seen so far; (-inf, 0) while there is none
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    if (nm == -INFINITY) return;
    s = s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}
__device__ __forceinline__ void lse_add8(float& m, float& s, const float (&x)[8]) {
    float cm = x[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) cm = fmaxf(cm, x[i]);
    if (cm == -INFINITY) return;
    const float nm = fmaxf(m, cm);
    // (the hardware exponential: with the library's expf the 112 calls a thread makes were a fifth of the launch's time at 5 rows,
    // 38 -> 31 us, one workgroup being alone on its CU; its error, 2^-22 relative near the maximum, averages out in a sum of thousands)
    float a = s * __expf(m - nm);
#pragma unroll
    for (int i = 0; i < 8; ++i) a += __expf(x[i] - nm);
    s = a; m = nm;
}

// The fusion of ONE row, shared by the two kernels below: `r` the decoder row, `item` its item, `d` the RESOLVED descriptor (by value:
// in SGPRs, every field uniform in the workgroup), `state` the slot's context states. The callers have returned for a finished call, a
// finished item and a row outside the beam; every return in here depends on the row and the descriptor alone, so the workgroup is whole
// at each barrier.
__device__ __forceinline__ void lm_fuse_row(float* __restrict__ logits, const SearchState& st, const LmDesc d, int* __restrict__ state_of, const int r,
                                            const int item, const int eot, const long ldl) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = st.pos[r], plen = st.plen[item], tok = st.token[r];
    if (p < 0 || p >= WLX_T_TEXT) return;
    if (eot < 1 || eot >= NGLM_MAX_VOCAB) return;
    const bool raw = st.nsp_row[r] > 0;         // the row's RAW distribution defines no_speech_prob: its state is written, its logits stay
    __shared__ __attribute__((aligned(16))) float s_sc[NGLM_CHUNK];
    __shared__ int s_bnd[NGLM_LEVELS][NGLM_MAX_CHUNKS + 1];     // level j's edges of chunk c are [s_bnd[j][c], s_bnd[j][c + 1])
    __shared__ float s_above[NGLM_LEVELS + 1];                  // the weights above level j; [nlev]: all of the chain
    __shared__ int s_nlev;
    __shared__ float s_red[NGLM_WAVES][4];
    const int nch = eot / NGLM_CHUNK + 1;       // chunks that hold a token of A
    float* lrow = logits + (long)r * ldl;
    const bool wide = (ldl & 3) == 0 && (reinterpret_cast<unsigned long long>(logits) & 15ull) == 0;
    // ---- 1. the thread's share of the row: piece q of chunk c covers ids c * NGLM_CHUNK + (q * 1024 + tid) * 4 .. + 3. A piece that
    // starts at or below eot lies below ldl (a multiple of 4 above eot); an id above eot is carried as it is and stored back unchanged
    float val[NGLM_MAX_CHUNKS][4 * NGLM_PIECES];
    if (!raw) {
#pragma unroll
        for (int c = 0; c < NGLM_MAX_CHUNKS; ++c) {
#pragma unroll
            for (int q = 0; q < NGLM_PIECES; ++q) {
                const int col = c * NGLM_CHUNK + (q * NGLM_THREADS + tid) * 4;
                float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (col <= eot) {
                    if (wide) v = *reinterpret_cast<const float4*>(lrow + col);
                    else {
                        v.x = lrow[col];
                        if (col + 1 <= eot) v.y = lrow[col + 1];
                        if (col + 2 <= eot) v.z = lrow[col + 2];
                        if (col + 3 <= eot) v.w = lrow[col + 3];
                    }
                }
                val[c][4 * q] = v.x; val[c][4 * q + 1] = v.y; val[c][4 * q + 2] = v.z; val[c][4 * q + 3] = v.w;
            }
        }
    }
    // the descriptor's FIRST use, behind the requests for the row: in the per-item kernel its fetch depends on the selection, and up to
    // here nothing has waited for it. (generate refuses another eot: never indexes past the unigram arrays. Uniform in the workgroup.)
    if (eot != d.eot) return;
    // (and the unigram scores of chunk 0, which depend on nothing else: one chunk ahead from here on)
    float4 un[NGLM_PIECES];
#pragma unroll
    for (int q = 0; q < NGLM_PIECES; ++q) un[q] = *reinterpret_cast<const float4*>(d.unigram_logp + (q * NGLM_THREADS + tid) * 4);
    // ---- 2. wave 0: the row's state, then its chain
    if (wave == 0) {
        int state = d.start;
        if (p >= plen && p >= 1) {              // a generated position: the parent's state, advanced by a text token
            int ps = state_of[(long)st.anc[(long)r * WLX_T_TEXT + p - 1] * WLX_T_TEXT + p - 1];
            if (ps < 0 || ps >= d.n_states) ps = d.start;       // (a state another model left behind: never indexes past this one)
            state = ps;
            if ((unsigned)tok < (unsigned)eot) {
                int s = ps, found = -1;
                for (int lvl = 0; lvl < NGLM_LEVELS && s > 0; ++lvl) {
                    const int lo = d.edge_off[s], hi = d.edge_off[s + 1];
                    const int i = lm_lower_bound(d.tok, lo, hi, tok, lane);
                    if (i < hi && d.tok[i] == tok) { found = d.next[i]; break; }
                    s = d.backoff_state[s];
                }
                state = found >= 0 ? found : d.unigram_next[tok];
                if (state < 0 || state >= d.n_states) state = 0;
            }
        }
        if (lane == 0) state_of[(long)r * WLX_T_TEXT + p] = state;
        if (!raw && lane == 0) {
            int n = 0, s = state;
            float acc = 0.f;
            for (; n < NGLM_LEVELS && s > 0; ++n) {
                s_bnd[n][0] = d.edge_off[s]; s_bnd[n][nch] = d.edge_off[s + 1];
                s_above[n] = acc;
                acc += d.backoff_weight[s];
                s = d.backoff_state[s];
            }
            s_above[n] = acc;
            s_nlev = n;
        }
    }
    if (raw) return;
    __syncthreads();
    // ---- 3. where each level's edge list crosses a chunk boundary: (level, boundary) tasks dealt over the waves
    const int nlev = s_nlev;
    for (int task = wave; task < nlev * (nch - 1); task += NGLM_WAVES) {
        const int j = task / (nch - 1), c = task - j * (nch - 1) + 1;
        const int b = lm_lower_bound(d.tok, s_bnd[j][0], s_bnd[j][nch], c * NGLM_CHUNK, lane);
        if (lane == 0) s_bnd[j][c] = b;
    }
    const float w = d.w, all_above = s_above[nlev];
    float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f;   // LSE_A(l), LSE_A(l + w s)
    // ---- 4. chunk by chunk through LDS
#pragma unroll
    for (int c = 0; c < NGLM_MAX_CHUNKS; ++c) {
        if (c < nch) {                          // (uniform)
            const int c0 = c * NGLM_CHUNK;
            __syncthreads();                    // the boundaries are written; the reads of the chunk before are over
#pragma unroll
            for (int q = 0; q < NGLM_PIECES; ++q) {
                const int k = (q * NGLM_THREADS + tid) * 4;
                float4 u = un[q];
                u.x += all_above; u.y += all_above; u.z += all_above; u.w += all_above;
                *reinterpret_cast<float4*>(s_sc + k) = u;
                // the next chunk's unigram scores are requested now: they arrive under this chunk's scatter and reductions
                if (c + 1 < nch) un[q] = *reinterpret_cast<const float4*>(d.unigram_logp + c0 + NGLM_CHUNK + k);
            }
            __syncthreads();
#pragma unroll
            for (int j = NGLM_LEVELS - 1; j >= 0; --j) {        // the shortest context first: a longer one overwrites it
                if (j < nlev) {
                    const int lo = s_bnd[j][c], hi = s_bnd[j][c + 1];
                    if (lo < hi) {              // (uniform)
                        const float above = s_above[j];
                        for (int i = lo + tid; i < hi; i += NGLM_THREADS) {
                            const unsigned k = (unsigned)(d.tok[i] - c0);
                            if (k < (unsigned)NGLM_CHUNK) s_sc[k] = d.logp[i] + above;
                        }
                        __syncthreads();
                    }
                }
            }
            float xr[4 * NGLM_PIECES], xf[4 * NGLM_PIECES];     // the raw and the fused values inside A, -inf outside
#pragma unroll
            for (int q = 0; q < NGLM_PIECES; ++q) {
                const int k = (q * NGLM_THREADS + tid) * 4;
                const float4 sc = *reinterpret_cast<const float4*>(s_sc + k);
                const float s4[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool in_a = c0 + k + i <= eot;
                    const float l = val[c][4 * q + i];
                    const float f = __fadd_rn(l, __fmul_rn(w, s4[i]));  // (two roundings, like the formula: no fused multiply-add)
                    xr[4 * q + i] = in_a ? l : -INFINITY;
                    xf[4 * q + i] = in_a ? f : -INFINITY;
                    if (in_a) val[c][4 * q + i] = f;
                }
            }
            lse_add8(m1, s1, xr);
            lse_add8(m2, s2, xf);
        }
    }
    // ---- 5. the workgroup's two log-sum-exps, then the stores
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lse_merge(m1, s1, __shfl_xor(m1, off), __shfl_xor(s1, off));
        lse_merge(m2, s2, __shfl_xor(m2, off), __shfl_xor(s2, off));
    }
    if (lane == 0) { s_red[wave][0] = m1; s_red[wave][1] = s1; s_red[wave][2] = m2; s_red[wave][3] = s2; }
    __syncthreads();
    m1 = m2 = -INFINITY; s1 = s2 = 0.f;
    for (int k = 0; k < NGLM_WAVES; ++k) {      // (every thread the same order: c is one number in the workgroup)
        lse_merge(m1, s1, s_red[k][0], s_red[k][1]);
        lse_merge(m2, s2, s_red[k][2], s_red[k][3]);
    }
    if (m1 == -INFINITY || !(s1 > 0.f) || !(s2 > 0.f)) return;  // no finite logit in A: the row is left alone
    const float cnorm = (m2 + logf(s2)) - (m1 + logf(s1));
#pragma unroll
    for (int c = 0; c < NGLM_MAX_CHUNKS; ++c) {
#pragma unroll
        for (int q = 0; q < NGLM_PIECES; ++q) {
            const int col = c * NGLM_CHUNK + (q * NGLM_THREADS + tid) * 4;
            if (col <= eot) {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = col + i <= eot ? val[c][4 * q + i] - cnorm : val[c][4 * q + i];
                if (wide) *reinterpret_cast<float4*>(lrow + col) = make_float4(o[0], o[1], o[2], o[3]);
                else {
                    lrow[col] = o[0];
                    if (col + 1 <= eot) lrow[col + 1] = o[1];
                    if (col + 2 <= eot) lrow[col + 2] = o[2];
                    if (col + 3 <= eot) lrow[col + 3] = o[3];
                }
            }
        }
    }
}

__global__ __launch_bounds__(NGLM_THREADS) void dec_lm_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp, SearchState st,
                                                              LmFusion lm) {
    if (*st.done) return;                       // scratch steps behind the end of the call
    const int r = blockIdx.x;
    const int R = spp->R, eot = spp->eot;
    const long ldl = spp->ldl;
    const int item = r / R, rb = r - item * R;
    if (st.item_done[item]) return;
    if (spp->sampling) { if (rb >= spp->num_hyp || st.row_done[r]) return; }
    else if (rb >= spp->beam) return;
    lm_fuse_row(logits, st, *lm.desc, lm.state, r, item, eot, ldl);
}

// The per-item form (wlx_lm_set_items / wlx_lm_select): the grid is (row of the item, item), so a workgroup finds its item
// without a division, and the descriptor is entry sel[item] of the slot's pool. Both sit at fixed addresses and are read from memory:
// one captured step graph serves any pool and any selection. A workgroup whose item has no entry (sel < 0) returns before it has asked
// for one word of the row: such an item pays the dispatch of its empty workgroups and writes neither a state nor a logit.
// The entry is fetched through the SCALAR cache: sel[item] and pool[sel] are uniform in the workgroup, so the 80 bytes land in SGPRs (two
// s_load) and cost no VGPR — the kernel holds the whole row in registers, 115 VGPRs of the 128 that 1024 threads leave, and a descriptor
// fetched by one lane and broadcast would need twenty readlanes or spill. The fetch depends on sel, which the exit needs anyway, and is
// asked for here, in front of the call; lm_fuse_row first reads a field of it BEHIND its requests for the row (step 1), so the entry
// arrives under the row's loads and wave 0's state walk starts where it starts in dec_lm_kernel: the entry is no new link in the chain.
__global__ __launch_bounds__(NGLM_THREADS) void dec_lm_items_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp, SearchState st,
                                                                    LmItems li) {
    const int item = blockIdx.y, rb = blockIdx.x;
    // everything the exits read is asked for at once (each word is there whatever the others hold), so the selection is no link of its
    // own in front of them: one wait where dec_lm_kernel's exits, written one behind the other, wait four times
    const int done = *st.done, e = li.sel[item], idone = st.item_done[item];
    const int R = spp->R, eot = spp->eot, sampling = spp->sampling, width = sampling ? spp->num_hyp : spp->beam;
    const long ldl = spp->ldl;
    if (done) return;                           // scratch steps behind the end of the call
    if (e < 0 || e >= NGLM_MAX_ENTRIES) return; // not fused (and never past the pool)
    if (idone || rb >= R || rb >= width) return;
    const int r = item * R + rb;
    if (sampling && st.row_done[r]) return;
    lm_fuse_row(logits, st, li.pool[e], li.state, r, item, eot, ldl);
}

void launch_dec_lm(float* logits, const SearchParams* sp_dev, int rows, const SearchState& st, const LmFusion& lm, hipStream_t s) {
    hipLaunchKernelGGL(dec_lm_kernel, dim3(rows), dim3(NGLM_THREADS), 0, s, logits, sp_dev, st, lm);
}

void launch_dec_lm_items(float* logits, const SearchParams* sp_dev, int items, int R, const SearchState& st, const LmItems& li, hipStream_t s) {
    hipLaunchKernelGGL(dec_lm_items_kernel, dim3(R, items), dim3(NGLM_THREADS), 0, s, logits, sp_dev, st, li);
}

}  // namespace wlx
