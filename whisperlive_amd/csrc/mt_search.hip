// mt_search.hip — the search of the translation engine on the device: the per-step bookkeeping of mt_engine.hip run_generate
// (Hugging Face's _beam_search: _get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams,
// _check_early_stop_heuristic; greedy search; NoRepeatNGramLogitsProcessor) as kernels over state that lives on the device for the
// whole generate (mt.h MtSearchState). The kernels use the host code's constants and its float operations in its order: one add per
// candidate, one division by a host-made length-penalty term, three adds of 0 / -1e9 — no multiplication, so nothing contracts, and
// the division must be the correctly rounded one (this file is not to be built with fast-math or approximate division: checked below
// and, bit for bit against the host search, by tests/test_gpu_mt_search_kernels.py).
//
// Orders are made by RANK, not by sorting: an element's place is the number of elements that precede it in the host code's order
// (value descending, then beam * V + token ascending for the candidate merge; value descending, then position ascending — the stable
// order — for the running and finished beams). Those orders are total, so the ranks are a permutation and equal std::sort's result.
//
// Termination: every item's workgroup ORs its stop flags into one word and counts itself in; the workgroup that arrives last owns the
// group's decision. When the generate is over it stores the results to pinned host memory, fences at system scope, and stores the
// done words — a release store, the pattern of search.hip finish_item. Nothing waits on a flag: the host reads the done word after an
// event. Later launches find ctl[0] set and return. Values that are not ordered (NaN) give garbage tokens, as on the host, but every
// index a rank fills has a valid default, so nothing is read out of bounds.
#include "mt.h"

#ifdef __FAST_MATH__
#error "mt_search.hip needs IEEE division and addition: build it without -ffast-math"
#endif

namespace wlx {

#define MTS_THREADS 256
#define MTS_MAXC (16 * WLX_MT_MAXK)     // candidates of one item: R rows x 2 R, R <= 16
#define MTS_NEG (-1.0e9f)

__device__ __forceinline__ int mts_position(int tok, int t, int pad) { return tok != pad ? 1 + t + pad : pad; }

__global__ __launch_bounds__(64) void mt_search_init_kernel(MtSearchParams P, MtSearchState S) {
    const int r = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < P.ML; j += 64) {
        const int v = j == 0 ? P.start : P.pad;
        S.run[0][(long)r * P.ML + j] = v;
        S.run[1][(long)r * P.ML + j] = v;
        S.fin[0][(long)r * P.ML + j] = P.pad;
        S.fin[1][(long)r * P.ML + j] = P.pad;
    }
    for (int j = tid; j < P.T; j += 64) {
        S.anc[0][(long)r * P.T + j] = r;
        S.anc[1][(long)r * P.T + j] = r;
    }
    if (tid != 0) return;
    S.run_score[r] = (r % P.R) ? MTS_NEG : 0.f;
    S.fin_score[r] = MTS_NEG;
    S.fin_len[r] = 0;
    S.fin_done[r] = 0;
    S.tok[r] = P.start;
    S.pos[r] = mts_position(P.start, 0, P.pad);
    S.gself[r] = MtAttnGroup{r, 1, 0, 1};
    S.nban[r] = 0;
    if (r % P.R == 0) {
        const int b = r / P.R;
        S.unsat[b] = 1;
        S.item_done[b] = 0;
        S.greedy_score[b] = 0.f;
    }
    if (r == 0) {
        S.ctl[0] = 0; S.ctl[1] = 0; S.ctl[2] = 0; S.ctl[3] = 1; S.ctl[4] = 0;
    }
}

// one wave per row: the tokens that would complete an n-gram already in the sequence, in the order of their first positions
__global__ __launch_bounds__(64) void mt_search_bans_kernel(MtSearchParams P, MtSearchState S, int i) {
    if (S.ctl[0]) return;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int cur_len = i + 1, n = P.nng;
    if (n <= 0 || cur_len + 1 < n) {
        if (lane == 0) S.nban[r] = 0;
        return;
    }
    const int* seq = S.run[P.R == 1 ? 0 : (i & 1)] + (long)r * P.ML;
    const int start = cur_len + 1 - n;
    int count = 0;
    for (int base = 0; base + n <= cur_len; base += 64) {
        const int a = base + lane;
        bool eq = a + n <= cur_len;
        for (int j = 0; j < n - 1 && eq; ++j) eq = seq[a + j] == seq[start + j];
        const unsigned long long mask = __ballot(eq);
        const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (eq && at < P.ban_ld) S.ban[(long)r * P.ban_ld + at] = seq[a + n - 1];
        count += __popcll(mask);
    }
    if (lane == 0) S.nban[r] = min(count, P.ban_ld);
}

__global__ __launch_bounds__(MTS_THREADS) void mt_search_step_kernel(MtSearchParams P, MtSearchState S,
                                                                     const float* __restrict__ tk_val,
                                                                     const int* __restrict__ tk_idx, int i, int force_now) {
    if (S.ctl[0]) return;
    __shared__ float cv[MTS_MAXC];
    __shared__ int cbeam[MTS_MAXC], ctok[MTS_MAXC];
    __shared__ int sel[WLX_MT_MAXK], order[WLX_MT_MAXK], tb[WLX_MT_MAXK], tt[WLX_MT_MAXK], hit[WLX_MT_MAXK];
    __shared__ float tv[WLX_MT_MAXK], rv[WLX_MT_MAXK];
    __shared__ float ms[16 + WLX_MT_MAXK];
    __shared__ int mlen[16 + WLX_MT_MAXK], mfin[16 + WLX_MT_MAXK];
    __shared__ float nscore[16], nfs[16];
    __shared__ int nfd[16], nfl[16], nfsrc[16];
    __shared__ int s_nvalid, s_last, s_done, s_ncl, s_steps;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = P.R, ML = P.ML, T = P.T, t = i, cur_len = i + 1;
    int bits = 0;       // thread 0: bit 0 = the item keeps the generate going (unsat / not done), bit 1 = not all finished, bit 2 = not all hit

    if (R == 1) {       // greedy (HF _sample with do_sample = False)
        if (tid == 0) {
            int tok;
            float lp;
            if (force_now) { tok = P.forced_eos; lp = 0.f; }
            else { tok = tk_idx[b]; lp = tk_val[b]; }
            int idn = S.item_done[b];
            if (idn) tok = P.pad;
            else S.greedy_score[b] += lp;
            S.run[0][(long)b * ML + cur_len] = tok;
            if (!idn) {
                S.fin_len[b] = cur_len + 1;
                if (tok == P.eos) { idn = 1; S.item_done[b] = 1; }
            }
            bits = idn ? 0 : 1;
            const int feed = tok < 0 ? P.pad : tok;
            S.tok[b] = feed;
            S.pos[b] = mts_position(feed, t + 1, P.pad);
            S.gself[b] = MtAttnGroup{b, 1, 0, min(t + 2, T)};
        }
    } else {
        const int K2 = 2 * R, p = i & 1, q = p ^ 1, r0 = b * R;
        const int* run_p = S.run[p];
        int* run_q = S.run[q];
        const int nc = force_now ? R : R * K2;
        if (tid == 0) s_nvalid = 0;
        __syncthreads();
        // ---- top-k continuations: the item's candidates
        for (int c = tid; c < nc; c += MTS_THREADS) {
            const int bb = force_now ? c : c / K2;
            const int r = r0 + bb;
            int tok;
            float v;
            if (force_now) { tok = P.forced_eos; v = 0.f + S.run_score[r]; }
            else { tok = tk_idx[(long)r * K2 + (c - bb * K2)]; v = tk_val[(long)r * K2 + (c - bb * K2)] + S.run_score[r]; }
            cv[c] = v; cbeam[c] = bb; ctok[c] = tok;
            if (tok >= 0) atomicAdd(&s_nvalid, 1);
        }
        for (int m = tid; m < R; m += MTS_THREADS) {      // the finished beams as they stand
            ms[m] = S.fin_score[r0 + m];
            mlen[m] = S.fin_len[r0 + m];
            mfin[m] = S.fin_done[r0 + m];
            nfs[m] = ms[m]; nfl[m] = mlen[m]; nfd[m] = mfin[m]; nfsrc[m] = m;      // (defaults: see sel / order below)
        }
        // The ranks below are a permutation only while the values are ordered. A NaN logit (the host's std::sort is undefined there
        // too) would leave places unwritten, and they index LDS and global rows: every place starts at a valid index.
        for (int k = tid; k < WLX_MT_MAXK; k += MTS_THREADS) { sel[k] = 0; order[k] = k; }
        __syncthreads();
        const int nk = min(s_nvalid, K2);
        for (int c = tid; c < nc; c += MTS_THREADS) {
            if (ctok[c] < 0) continue;
            const float v = cv[c];
            const int bb = cbeam[c], tok = ctok[c];
            int rank = 0;
            for (int j = 0; j < nc; ++j) {
                if (ctok[j] < 0) continue;
                const float vj = cv[j];
                rank += (vj > v || (vj == v && (cbeam[j] < bb || (cbeam[j] == bb && ctok[j] < tok)))) ? 1 : 0;
            }
            if (rank < K2) sel[rank] = c;
        }
        __syncthreads();
        if (tid < nk) {
            const int c = sel[tid];
            tv[tid] = cv[c]; tb[tid] = cbeam[c]; tt[tid] = ctok[c];
            const int h = (ctok[c] == P.eos || cur_len + 1 >= ML) ? 1 : 0;
            hit[tid] = h;
            rv[tid] = cv[c] + (h ? MTS_NEG : 0.f);
        }
        __syncthreads();
        // ---- running beams of the next iteration (stable order on rv) and the merge keys of the finished beams
        if (tid < nk) {
            int rank = 0;
            for (int j = 0; j < nk; ++j) rank += (rv[j] > rv[tid] || (rv[j] == rv[tid] && j < tid)) ? 1 : 0;
            order[rank] = tid;
            bool full = P.early_stopping == 1;
            for (int bb = 0; bb < R; ++bb) full &= mfin[bb] != 0;
            const bool just = hit[tid] && tid < R;
            float v = tv[tid] / S.lp[cur_len];
            v += full ? MTS_NEG : 0.f;
            v += S.unsat[b] ? 0.f : MTS_NEG;
            v += just ? 0.f : MTS_NEG;
            ms[R + tid] = v;
            mlen[R + tid] = cur_len + 1;
            mfin[R + tid] = just ? 1 : 0;
        }
        __syncthreads();
        if (tid < R + nk) {
            int rank = 0;
            for (int j = 0; j < R + nk; ++j) rank += (ms[j] > ms[tid] || (ms[j] == ms[tid] && j < tid)) ? 1 : 0;
            if (rank < R) { nfs[rank] = ms[tid]; nfl[rank] = mlen[tid]; nfd[rank] = mfin[tid]; nfsrc[rank] = tid; }
        }
        __syncthreads();
        // ---- the rows of the next iteration: sequences, ancestry (gathered from the OLD table), finished sequences
        for (int bb = 0; bb < R; ++bb) {
            const int r = r0 + bb;
            if (bb >= nk) {
                for (int j = tid; j < ML; j += MTS_THREADS) run_q[(long)r * ML + j] = run_p[(long)r * ML + j];
                for (int j = tid; j <= t; j += MTS_THREADS) S.anc[q][(long)r * T + j] = 0;
                if (tid == 0) nscore[bb] = -INFINITY;
            } else {
                const int k = order[bb], src = r0 + tb[k];
                for (int j = tid; j < ML; j += MTS_THREADS) run_q[(long)r * ML + j] = j == cur_len ? tt[k] : run_p[(long)src * ML + j];
                for (int j = tid; j <= t; j += MTS_THREADS) S.anc[q][(long)r * T + j] = S.anc[p][(long)src * T + j];
                if (tid == 0) nscore[bb] = rv[k];
            }
            if (tid == 0 && t + 1 < T) S.anc[q][(long)r * T + t + 1] = r;
            const int msrc = nfsrc[bb];
            int* fq = S.fin[q] + (long)r * ML;
            if (msrc < R) {
                const int* fp = S.fin[p] + (long)(r0 + msrc) * ML;
                for (int j = tid; j < ML; j += MTS_THREADS) fq[j] = fp[j];
            } else {
                const int k = msrc - R;
                const int* rp = run_p + (long)(r0 + tb[k]) * ML;
                for (int j = tid; j < ML; j += MTS_THREADS) fq[j] = j == cur_len ? tt[k] : rp[j];
            }
        }
        __syncthreads();
        if (tid < R) {
            const int r = r0 + tid;
            S.fin_score[r] = nfs[tid];
            S.fin_len[r] = nfl[tid];
            S.fin_done[r] = nfd[tid];
            S.run_score[r] = nscore[tid];
            const int tok = run_q[(long)r * ML + cur_len];      // (this thread's view: written above, behind the barrier)
            const int feed = tok < 0 ? P.pad : tok;
            S.tok[r] = feed;
            S.pos[r] = mts_position(feed, t + 1, P.pad);
            S.gself[r] = MtAttnGroup{r, 1, 0, min(t + 2, T)};
        }
        if (tid == 0) {     // early-stop heuristic of the item, with cur_len already advanced
            const int best_len = (P.early_stopping == 2 && P.lp_positive) ? ML - 1 : cur_len;
            const float best = nscore[0] / S.lp[best_len];
            float worst = INFINITY;
            for (int bb = 0; bb < R; ++bb) worst = nfs[bb] < worst ? nfs[bb] : worst;
            bool anyb = false, all_fin = true, all_hit = true;
            for (int bb = 0; bb < R; ++bb) {
                anyb |= best > (nfd[bb] ? worst : MTS_NEG);
                all_fin &= nfd[bb] != 0;
            }
            for (int k = 0; k < nk; ++k) all_hit &= hit[k] != 0;
            const int un = (S.unsat[b] && anyb) ? 1 : 0;
            S.unsat[b] = un;
            bits = un | (all_fin ? 0 : 2) | (all_hit ? 0 : 4);
        }
    }

    // ---- arrival: this item's state is stored; the last workgroup decides for the group
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        if (bits) atomicOr(&S.ctl[2], bits);
        __threadfence();
        s_last = atomicAdd(&S.ctl[1], 1) == P.B - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid == 0) {
        const int flags = atomicExch(&S.ctl[2], 0);
        atomicExch(&S.ctl[1], 0);
        const int ncl = cur_len + 1;
        const int steps = S.ctl[4] + (force_now ? 0 : 1);
        S.ctl[3] = ncl;
        S.ctl[4] = steps;
        bool done;
        if (R == 1) done = !(flags & 1) || ncl >= ML;
        else {
            const bool any_unsat = flags & 1, all_fin = !(flags & 2), all_hit = !(flags & 4);
            const bool open = !(all_fin && P.early_stopping == 1);
            done = !(any_unsat && open && !all_hit) || ncl >= ML;
        }
        s_done = done; s_ncl = ncl; s_steps = steps;
    }
    __syncthreads();
    if (!s_done) return;
    // ---- results: generated tokens after the decoder start, the final EOS excluded
    const int qf = (i & 1) ^ 1;
    for (int b2 = 0; b2 < P.B; ++b2) {
        const int* seq;
        int len;
        float score;
        if (R == 1) { seq = S.run[0] + (long)b2 * ML; len = S.fin_len[b2] ? S.fin_len[b2] : s_ncl; score = S.greedy_score[b2]; }
        else { seq = S.fin[qf] + (long)b2 * R * ML; len = S.fin_len[b2 * R]; score = S.fin_score[b2 * R]; }
        int n = max(0, len - 1);
        if (n > 0 && seq[len - 1] == P.eos) n--;
        for (int j = tid; j < n; j += MTS_THREADS) S.h_tok[(long)b2 * ML + j] = seq[1 + j];
        if (tid == 0) { S.h_n[b2] = n; S.h_score[b2] = score; }
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        S.ctl[0] = 1;
        S.h_done[1] = s_ncl;
        S.h_done[2] = s_steps;
        __threadfence_system();
        __hip_atomic_store(S.h_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

void launch_mt_search_init(const MtSearchParams& P, const MtSearchState& S, hipStream_t s) {
    hipLaunchKernelGGL(mt_search_init_kernel, dim3(P.B * P.R), dim3(64), 0, s, P, S);
}

void launch_mt_search_bans(const MtSearchParams& P, const MtSearchState& S, int i, hipStream_t s) {
    hipLaunchKernelGGL(mt_search_bans_kernel, dim3(P.B * P.R), dim3(64), 0, s, P, S, i);
}

void launch_mt_search_step(const MtSearchParams& P, const MtSearchState& S, const float* tk_val, const int* tk_idx, int i,
                           int force_now, hipStream_t s) {
    hipLaunchKernelGGL(mt_search_step_kernel, dim3(P.B), dim3(MTS_THREADS), 0, s, P, S, tk_val, tk_idx, i, force_now);
}

}  // namespace wlx
