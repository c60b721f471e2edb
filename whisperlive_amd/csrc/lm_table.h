// lm_table.h — the host side of an n-gram language model (wlx_lm_create; dec_lm.hip) that needs no device: the check of the backoff
// automaton a caller hands in. Plain C++ without a device call, so a stand-alone program can run it under the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace wlx {

constexpr int NGLM_MAX_ORDER = 5;               // include/wlx_lm.h WLX_LM_MAX_ORDER: a chain is at most four contexts and the unigram level
constexpr int NGLM_MAX_STATES = 1 << 20;        // WLX_LM_MAX_STATES
constexpr int NGLM_MAX_EDGES = 1 << 22;         // WLX_LM_MAX_EDGES
constexpr int NGLM_MAX_VOCAB = 65536;           // WLX_LM_MAX_VOCAB: a row's fused values stay in the registers of one workgroup
constexpr int NGLM_MAX_MODELS = 8;              // WLX_LM_MAX_MODELS
constexpr int NGLM_MAX_ENTRIES = 64;            // include/wlx_lm_items.h WLX_LM_SET_MAX_ENTRIES: (model, weight) entries of a slot's pool

// the format of include/wlx_lm.h, violation by violation: true, or false with the reason in `msg`. Reads nothing past what the counts
// checked so far allow.
inline bool lm_table_check(int V, int eot, int order, int n_states, int start_state, const int32_t* edge_off, const int32_t* backoff_state,
                           const float* backoff_weight, const int32_t* edge_tok, const float* edge_logp, const int32_t* edge_next,
                           const float* unigram_logp, const int32_t* unigram_next, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b, long c) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b, c); return false; };
    if (V < 1 || V > NGLM_MAX_VOCAB) return fail("lm: a vocabulary of %ld outside 1..%ld (vocab)", V, NGLM_MAX_VOCAB, 0);
    if (eot < 1 || eot >= V) return fail("lm: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1, 0);
    if (order < 1 || order > NGLM_MAX_ORDER) return fail("lm: order %ld outside 1..%ld", order, NGLM_MAX_ORDER, 0);
    if (n_states < 1 || n_states > NGLM_MAX_STATES) return fail("lm: %ld states outside 1..%ld", n_states, NGLM_MAX_STATES, 0);
    if (!edge_off || !backoff_state || !backoff_weight || !unigram_logp || !unigram_next) return fail("lm: null argument", 0, 0, 0);
    if (start_state < 0 || start_state >= n_states) return fail("lm: start state %ld outside 0..%ld", start_state, (long)n_states - 1, 0);
    if (edge_off[0] != 0 || edge_off[1] != 0) return fail("lm: state 0 is the empty context and has no explicit edges (edge_off[0..1] must be 0)", 0, 0, 0);
    for (int n = 0; n < n_states; ++n)
        if (edge_off[n + 1] < edge_off[n] || edge_off[n + 1] > NGLM_MAX_EDGES)
            return fail("lm: state %ld ends at edge %ld (offsets ascend, at most %ld edges)", n, edge_off[n + 1], NGLM_MAX_EDGES);
    const int n_edges = edge_off[n_states];
    if (n_edges > 0 && (!edge_tok || !edge_logp || !edge_next)) return fail("lm: null argument", 0, 0, 0);
    for (int v = 0; v <= eot; ++v) {
        if (!std::isfinite(unigram_logp[v])) return fail("lm: the unigram score of token %ld is not finite", v, 0, 0);
        if (unigram_next[v] < 0 || unigram_next[v] >= n_states)
            return fail("lm: token %ld leads from the empty context to state %ld outside 0..%ld (next)", v, unigram_next[v], (long)n_states - 1);
    }
    // a backoff link leads to a strictly shorter context: every chain reaches state 0, within order - 1 links
    if (backoff_state[0] != -1 && backoff_state[0] != 0) return fail("lm: state 0 backs off to %ld (it is the end of every chain)", backoff_state[0], 0, 0);
    std::vector<int8_t> depth((size_t)n_states, -1);
    depth[0] = 0;
    for (int n = 1; n < n_states; ++n) {
        if (!std::isfinite(backoff_weight[n])) return fail("lm: the backoff weight of state %ld is not finite", n, 0, 0);
        if (backoff_state[n] < 0 || backoff_state[n] >= n_states)
            return fail("lm: state %ld backs off to state %ld outside 0..%ld (backoff)", n, backoff_state[n], (long)n_states - 1);
    }
    for (int n = 1; n < n_states; ++n) {
        int hops = 0, s = n;
        while (depth[s] < 0 && hops < order) { s = backoff_state[s]; ++hops; }
        if (depth[s] < 0 || depth[s] + hops > order - 1)
            return fail("lm: the backoff chain of state %ld does not reach the empty context within %ld links (a backoff leads to a strictly shorter context)",
                        n, (long)order - 1, 0);
        int d = depth[s] + hops;
        for (s = n; depth[s] < 0; s = backoff_state[s]) depth[s] = (int8_t)d--;
    }
    for (int n = 1; n < n_states; ++n)
        for (int i = edge_off[n]; i < edge_off[n + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] > eot) return fail("lm: edge token %ld of state %ld outside 0..%ld (the text tokens and eot)", edge_tok[i], n, eot);
            if (i > edge_off[n] && edge_tok[i] <= edge_tok[i - 1]) return fail("lm: the edge tokens of state %ld do not ascend", n, 0, 0);
            if (!std::isfinite(edge_logp[i])) return fail("lm: the score of edge %ld (state %ld) is not finite", i, n, 0);
            if (edge_next[i] < 0 || edge_next[i] >= n_states)
                return fail("lm: edge %ld leads to state %ld outside 0..%ld (next)", i, edge_next[i], (long)n_states - 1);
        }
    return true;
}

}  // namespace wlx
