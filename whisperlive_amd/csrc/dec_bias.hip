// dec_bias.hip — keyword boosting: the one launch between the vocabulary projection and the token search of a decode step whose slot
// has a bias table installed (wlx_bias_set). A step of a slot without a table does not launch it. A slot that holds a SET of
// tables, one selected per item of the decode group (wlx_bias_set_items / wlx_bias_select), launches dec_bias_items_kernel
// (below) in its place.
//
// The table is an Aho-Corasick automaton over token ids, closed on the host (whisperlive_amd/biasing.py): node n carries the sorted
// list of its explicit edges (token, next node) — every token that leads from n to a node other than the root, through n's own
// children or its failure chain; any other token leads to the root (node 0). A node that ends a phrase carries the root's edges.
// Row r at position p is in state next(state of its parent row at p - 1, token fed at p); the parent row is anc[r][p - 1], the KV-cache
// row that holds position p - 1 of the hypothesis now living in r, so the state follows the beam's re-ordering like the fed tokens
// (intok) do: it is kept per (cache row, position) and a row re-used after a re-order cannot overwrite what a sibling still reads.
// The logits of the row then take `boost` on every edge token of its node, and after that the values of the token list (logit_bias).
#include "decoder.h"
#include "host.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace wlx {

// one wave per decoder row
__global__ __launch_bounds__(64) void dec_bias_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp, SearchState st,
                                                      BiasTable bt) {
    if (*st.done) return;                       // scratch steps behind the end of the call
    const int r = blockIdx.x;
    const int R = spp->R, eot = spp->eot;
    const long ldl = spp->ldl;
    const int item = r / R, rb = r - item * R;
    if (st.item_done[item]) return;
    if (spp->sampling) { if (rb >= spp->num_hyp || st.row_done[r]) return; }
    else if (rb >= spp->beam) return;
    const int lane = threadIdx.x;
    const int p = st.pos[r], plen = st.plen[item], tok = st.token[r];
    if (p < 0 || p >= WLX_T_TEXT) return;
    const int n_nodes = bt.hdr[0], n_tok = bt.hdr[2];
    const float boost = __int_as_float(bt.hdr[3]);
    // ---- the row's node: the root while the fed token is a prompt token (the first generated position) or a special / timestamp
    int state = 0;
    if (p >= plen && p >= 1 && tok < eot) {
        const int parent = st.anc[(long)r * WLX_T_TEXT + p - 1];
        int ps = bt.state[(long)parent * WLX_T_TEXT + p - 1];
        if (ps < 0 || ps >= n_nodes) ps = 0;    // (a state another table left behind: never indexes past this one)
        const int lo = bt.edge_off[ps], hi = bt.edge_off[ps + 1];
        for (int base = lo; base < hi; base += 64) {        // (uniform trip count: lo, hi are the same in every lane)
            const int i = base + lane;
            const unsigned long long hit = __ballot(i < hi && bt.edge_tok[i] == tok);
            if (hit) { state = bt.edge_next[base + __ffsll((long long)hit) - 1]; break; }
        }
    }
    if (lane == 0) bt.state[(long)r * WLX_T_TEXT + p] = (short)state;
    // a row whose RAW distribution defines no_speech_prob inside the search keeps its logits as they are
    if (st.nsp_row[r] > 0) return;
    float* lrow = logits + (long)r * ldl;
    const int e0 = bt.edge_off[state], e1 = bt.edge_off[state + 1];
    for (int i = e0 + lane; i < e1; i += 64) lrow[bt.edge_tok[i]] += boost;        // distinct tokens within a node: no two lanes share an address
    __syncthreads();                            // a list token may be an edge token: the second add reads what the first one stored
    for (int i = lane; i < n_tok; i += 64) lrow[bt.tok_ids[i]] += bt.tok_vals[i];   // distinct tokens (checked by wlx_bias_set)
}

int bias_table_fill(int* block, int V, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, float boost,
                    int n_tok, const int32_t* tok_ids, const float* tok_vals) {
    if (n_nodes < 1 || n_nodes > WLX_BIAS_MAX_NODES) return set_error(WLX_ERR_ARG, "bias table: %d nodes outside 1..%d", n_nodes, WLX_BIAS_MAX_NODES);
    if (n_tok < 0 || n_tok > WLX_BIAS_MAX_TOKENS) return set_error(WLX_ERR_ARG, "bias table: %d logit_bias entries outside 0..%d", n_tok, WLX_BIAS_MAX_TOKENS);
    if (!edge_off || (n_tok > 0 && (!tok_ids || !tok_vals))) return set_error(WLX_ERR_ARG, "bias table: null argument");
    if (!std::isfinite(boost)) return set_error(WLX_ERR_ARG, "bias table: boost is not finite");
    if (edge_off[0] != 0) return set_error(WLX_ERR_ARG, "bias table: edge_off[0] must be 0");
    for (int n = 0; n < n_nodes; ++n)
        if (edge_off[n + 1] < edge_off[n] || edge_off[n + 1] > WLX_BIAS_MAX_EDGES)
            return set_error(WLX_ERR_ARG, "bias table: node %d ends at edge %d (offsets ascend, at most %d edges)", n, edge_off[n + 1], WLX_BIAS_MAX_EDGES);
    const int n_edges = edge_off[n_nodes];
    if (n_edges > 0 && (!edge_tok || !edge_next)) return set_error(WLX_ERR_ARG, "bias table: null argument");
    for (int n = 0; n < n_nodes; ++n)
        for (int i = edge_off[n]; i < edge_off[n + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] >= V) return set_error(WLX_ERR_ARG, "bias table: edge token %d outside the vocabulary (%d)", edge_tok[i], V);
            if (i > edge_off[n] && edge_tok[i] <= edge_tok[i - 1]) return set_error(WLX_ERR_ARG, "bias table: the edge tokens of node %d do not ascend", n);
            if (edge_next[i] < 1 || edge_next[i] >= n_nodes) return set_error(WLX_ERR_ARG, "bias table: edge %d leads to node %d outside 1..%d", i, edge_next[i], n_nodes - 1);
        }
    std::vector<int32_t> seen(tok_ids, tok_ids + n_tok);
    std::sort(seen.begin(), seen.end());
    for (int i = 0; i < n_tok; ++i) {
        if (tok_ids[i] < 0 || tok_ids[i] >= V) return set_error(WLX_ERR_ARG, "bias table: logit_bias token %d outside the vocabulary (%d)", tok_ids[i], V);
        if (!std::isfinite(tok_vals[i])) return set_error(WLX_ERR_ARG, "bias table: the logit_bias value of token %d is not finite", tok_ids[i]);
        if (i > 0 && seen[i] == seen[i - 1]) return set_error(WLX_ERR_ARG, "bias table: logit_bias names token %d twice", seen[i]);
    }
    const BiasTable t = bias_table_at(block, nullptr);
    int* hdr = block;
    hdr[0] = n_nodes; hdr[1] = n_edges; hdr[2] = n_tok; memcpy(&hdr[3], &boost, 4);
    memcpy(const_cast<int*>(t.edge_off), edge_off, (size_t)(n_nodes + 1) * 4);
    if (n_edges) { memcpy(const_cast<int*>(t.edge_tok), edge_tok, (size_t)n_edges * 4); memcpy(const_cast<int*>(t.edge_next), edge_next, (size_t)n_edges * 4); }
    if (n_tok) { memcpy(const_cast<int*>(t.tok_ids), tok_ids, (size_t)n_tok * 4); memcpy(const_cast<float*>(t.tok_vals), tok_vals, (size_t)n_tok * 4); }
    return WLX_OK;
}

void launch_dec_bias(float* logits, const SearchParams* sp_dev, int rows, const SearchState& st, const BiasTable& bt, hipStream_t s) {
    hipLaunchKernelGGL(dec_bias_kernel, dim3(rows), dim3(64), 0, s, logits, sp_dev, st, bt);
}

// ---- per-item tables (wlx_bias_set_items / wlx_bias_select). The same launch shape and the same early returns; the row's
// table is the one selected for its item of the decode group. A table is stored in the COMPACT form: node 0's list is the root's (its
// children), node n != 0 keeps only its own edges — the entries of its closed list that are not the root's entry for that token. The walk
// looks in the parent node's own list, then in the root's; the adds take the unflagged own edges, then the root's list (an own edge whose
// token the root's list names too is flagged: the root pass boosts it). Every token so gets the one add the closed table gives it.
__global__ __launch_bounds__(64) void dec_bias_items_kernel(float* __restrict__ logits, const SearchParams* __restrict__ spp, SearchState st,
                                                            BiasItems bi) {
    if (*st.done) return;
    const int r = blockIdx.x;
    const int R = spp->R, eot = spp->eot;
    const long ldl = spp->ldl;
    const int item = r / R, rb = r - item * R;
    if (st.item_done[item]) return;
    if (spp->sampling) { if (rb >= spp->num_hyp || st.row_done[r]) return; }
    else if (rb >= spp->beam) return;
    const int lane = threadIdx.x;
    const int p = st.pos[r], plen = st.plen[item], tok = st.token[r];
    if (p < 0 || p >= WLX_T_TEXT) return;
    const int t = bi.sel[item];
    if (t < 0) {                                // no table for this item: the root, and the row's logits stay as they are
        if (lane == 0) bi.state[(long)r * WLX_T_TEXT + p] = 0;
        return;
    }
    const int* hdr = bi.pool + t * BIAS_HDR_INTS;
    const int* off = bi.pool + hdr[0];
    const int* etok = bi.pool + hdr[1];
    const int* enext = bi.pool + hdr[2];
    const int n_nodes = hdr[5], n_tok = hdr[6];
    const float boost = __int_as_float(hdr[7]);
    const int r1 = off[1];                      // the root's list is [0, r1)
    int state = 0;
    if (p >= plen && p >= 1 && tok < eot) {
        const int parent = st.anc[(long)r * WLX_T_TEXT + p - 1];
        int ps = bi.state[(long)parent * WLX_T_TEXT + p - 1];
        if (ps < 0 || ps >= n_nodes) ps = 0;    // (a state another table left behind: never indexes past this one)
        bool found = false;
        if (ps != 0) {                          // the own list first: it overrides the root's entry for the same token
            const int lo = off[ps], hi = off[ps + 1];
            for (int base = lo; base < hi; base += 64) {    // (uniform trip count)
                const int i = base + lane;
                const unsigned long long hit = __ballot(i < hi && etok[i] == tok);
                if (hit) { state = enext[base + __ffsll((long long)hit) - 1] & (WLX_BIAS_EDGE_SHARED - 1); found = true; break; }
            }
        }
        if (!found)
            for (int base = 0; base < r1; base += 64) {
                const int i = base + lane;
                const unsigned long long hit = __ballot(i < r1 && etok[i] == tok);
                if (hit) { state = enext[base + __ffsll((long long)hit) - 1] & (WLX_BIAS_EDGE_SHARED - 1); break; }
            }
    }
    if (lane == 0) bi.state[(long)r * WLX_T_TEXT + p] = (short)state;
    if (st.nsp_row[r] > 0) return;
    float* lrow = logits + (long)r * ldl;
    if (state != 0) {                           // (in the root the own list IS the root's: the pass below takes it)
        const int e0 = off[state], e1 = off[state + 1];
        for (int i = e0 + lane; i < e1; i += 64)
            if (!(enext[i] & WLX_BIAS_EDGE_SHARED)) lrow[etok[i]] += boost;
    }
    // the root's tokens are none of the unflagged own ones: no two adds of the two passes share an address
    for (int i = lane; i < r1; i += 64) lrow[etok[i]] += boost;
    __syncthreads();
    const int* ids = bi.pool + hdr[3];
    const float* vals = reinterpret_cast<const float*>(bi.pool + hdr[4]);
    for (int i = lane; i < n_tok; i += 64) lrow[ids[i]] += vals[i];
}

int bias_items_fill(std::vector<int>& pool, int V, int n_tables, const int32_t* n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                    const int32_t* edge_next, const float* boosts, const int32_t* n_tok, const int32_t* tok_ids, const float* tok_vals) {
    if (n_tables < 1 || n_tables > WLX_BIAS_SET_MAX_TABLES) return set_error(WLX_ERR_ARG, "bias set: %d tables outside 1..%d", n_tables, WLX_BIAS_SET_MAX_TABLES);
    if (!n_nodes || !edge_off || !boosts || !n_tok) return set_error(WLX_ERR_ARG, "bias set: null argument");
    long nodes = 0, edges = 0, toks = 0;
    for (int t = 0; t < n_tables; ++t) {
        if (n_nodes[t] < 1 || n_nodes[t] > WLX_BIAS_MAX_NODES) return set_error(WLX_ERR_ARG, "bias set: table %d has %d nodes, outside 1..%d", t, n_nodes[t], WLX_BIAS_MAX_NODES);
        if (n_tok[t] < 0 || n_tok[t] > WLX_BIAS_MAX_TOKENS) return set_error(WLX_ERR_ARG, "bias set: table %d has %d logit_bias entries, outside 0..%d", t, n_tok[t], WLX_BIAS_MAX_TOKENS);
        if (!std::isfinite(boosts[t])) return set_error(WLX_ERR_ARG, "bias set: the boost of table %d is not finite", t);
        const int32_t* off = edge_off + nodes + t;
        if (off[0] != 0) return set_error(WLX_ERR_ARG, "bias set: the edge offsets of table %d must start at 0", t);
        for (int n = 0; n < n_nodes[t]; ++n)
            if (off[n + 1] < off[n] || off[n + 1] > WLX_BIAS_SET_MAX_EDGES)
                return set_error(WLX_ERR_ARG, "bias set: node %d of table %d ends at edge %d (offsets ascend, at most %d edges in all)", n, t, off[n + 1], WLX_BIAS_SET_MAX_EDGES);
        nodes += n_nodes[t]; edges += off[n_nodes[t]]; toks += n_tok[t];
        if (nodes > WLX_BIAS_SET_MAX_NODES) return set_error(WLX_ERR_ARG, "bias set: more than %d nodes in all", WLX_BIAS_SET_MAX_NODES);
        if (edges > WLX_BIAS_SET_MAX_EDGES) return set_error(WLX_ERR_ARG, "bias set: more than %d edges in all", WLX_BIAS_SET_MAX_EDGES);
        if (toks > WLX_BIAS_SET_MAX_TOKENS) return set_error(WLX_ERR_ARG, "bias set: more than %d logit_bias entries in all", WLX_BIAS_SET_MAX_TOKENS);
    }
    if ((edges > 0 && (!edge_tok || !edge_next)) || (toks > 0 && (!tok_ids || !tok_vals))) return set_error(WLX_ERR_ARG, "bias set: null argument");
    const int off_at = WLX_BIAS_SET_MAX_TABLES * BIAS_HDR_INTS, etok_at = off_at + (int)nodes + n_tables, enext_at = etok_at + (int)edges,
              ids_at = enext_at + (int)edges, vals_at = ids_at + (int)toks;
    pool.assign((size_t)vals_at + toks, 0);
    long nb = 0, eb = 0, tb = 0;
    for (int t = 0; t < n_tables; ++t) {
        const int32_t* off = edge_off + nb + t;
        const int32_t *etok = edge_tok + eb, *enext = edge_next + eb, *ids = tok_ids + tb;
        const float* vals = tok_vals + tb;
        const int nn = n_nodes[t], ne = off[nn], nt = n_tok[t], r1 = off[1];
        for (int n = 0; n < nn; ++n)
            for (int i = off[n]; i < off[n + 1]; ++i) {
                const int nx = enext[i] & (WLX_BIAS_EDGE_SHARED - 1);
                const bool shared = (enext[i] & WLX_BIAS_EDGE_SHARED) != 0;
                if (etok[i] < 0 || etok[i] >= V) return set_error(WLX_ERR_ARG, "bias set: edge token %d of table %d outside the vocabulary (%d)", etok[i], t, V);
                if (i > off[n] && etok[i] <= etok[i - 1]) return set_error(WLX_ERR_ARG, "bias set: the edge tokens of node %d of table %d do not ascend", n, t);
                if ((enext[i] & ~(WLX_BIAS_EDGE_SHARED | (WLX_BIAS_EDGE_SHARED - 1))) || nx < 1 || nx >= nn)
                    return set_error(WLX_ERR_ARG, "bias set: edge %d of table %d leads to node %d outside 1..%d", i, t, nx, nn - 1);
                // the flag says exactly whether the root's list names the token: the two boost passes then never meet on a token
                const bool in_root = n != 0 && std::binary_search(etok, etok + r1, etok[i]);
                if (shared != in_root) return set_error(WLX_ERR_ARG, "bias set: edge %d of table %d: the shared flag must be set exactly where the root's list has the token", i, t);
            }
        std::vector<int32_t> seen(ids, ids + nt);
        std::sort(seen.begin(), seen.end());
        for (int i = 0; i < nt; ++i) {
            if (ids[i] < 0 || ids[i] >= V) return set_error(WLX_ERR_ARG, "bias set: logit_bias token %d of table %d outside the vocabulary (%d)", ids[i], t, V);
            if (!std::isfinite(vals[i])) return set_error(WLX_ERR_ARG, "bias set: the logit_bias value of token %d of table %d is not finite", ids[i], t);
            if (i > 0 && seen[i] == seen[i - 1]) return set_error(WLX_ERR_ARG, "bias set: table %d names logit_bias token %d twice", t, seen[i]);
        }
        int* hdr = pool.data() + (size_t)t * BIAS_HDR_INTS;
        hdr[0] = off_at + (int)nb + t; hdr[1] = etok_at + (int)eb; hdr[2] = enext_at + (int)eb; hdr[3] = ids_at + (int)tb; hdr[4] = vals_at + (int)tb;
        hdr[5] = nn; hdr[6] = nt; memcpy(&hdr[7], &boosts[t], 4);
        memcpy(pool.data() + hdr[0], off, (size_t)(nn + 1) * 4);
        if (ne) { memcpy(pool.data() + hdr[1], etok, (size_t)ne * 4); memcpy(pool.data() + hdr[2], enext, (size_t)ne * 4); }
        if (nt) { memcpy(pool.data() + hdr[3], ids, (size_t)nt * 4); memcpy(pool.data() + hdr[4], vals, (size_t)nt * 4); }
        nb += nn; eb += ne; tb += nt;
    }
    return WLX_OK;
}

void launch_dec_bias_items(float* logits, const SearchParams* sp_dev, int rows, const SearchState& st, const BiasItems& bi, hipStream_t s) {
    hipLaunchKernelGGL(dec_bias_items_kernel, dim3(rows), dim3(64), 0, s, logits, sp_dev, st, bi);
}

}  // namespace wlx
