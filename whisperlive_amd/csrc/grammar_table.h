// grammar_table.h — the host side of a grammar table (wlx_grammar_set; dec_grammar.hip) that needs no device: the check of the DFA a caller
// hands in, and its layout in the block of ints the kernel walks. Plain C++: tests/grammar_table_check.cpp runs it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace wlx {

constexpr int GRAMMAR_MAX_STATES = 4096;        // include/wlx_grammar.h WLX_GRAMMAR_MAX_STATES: a state fits the short the bias states use
constexpr int GRAMMAR_MAX_EDGES = 16384;        // WLX_GRAMMAR_MAX_EDGES
// the block: [4] header (n_states, n_edges, eot, 0), edge_off [MAX_STATES + 1], edge_tok [MAX_EDGES], edge_next [MAX_EDGES], accept [MAX_STATES]
constexpr int GRAMMAR_HDR_INTS = 4;
constexpr int GRAMMAR_OFF_AT = GRAMMAR_HDR_INTS;
constexpr int GRAMMAR_TOK_AT = GRAMMAR_OFF_AT + GRAMMAR_MAX_STATES + 1;
constexpr int GRAMMAR_NEXT_AT = GRAMMAR_TOK_AT + GRAMMAR_MAX_EDGES;
constexpr int GRAMMAR_ACCEPT_AT = GRAMMAR_NEXT_AT + GRAMMAR_MAX_EDGES;
constexpr int GRAMMAR_TABLE_INTS = GRAMMAR_ACCEPT_AT + GRAMMAR_MAX_STATES;

// the format of include/wlx_grammar.h, violation by violation: true, or false with the reason in `msg`. Reads nothing past what the
// counts checked so far allow (edge_off[n + 1] only after edge_off[n] passed, an edge only below the last offset).
inline bool grammar_table_check(int V, int eot, int n_states, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                                const int32_t* accept, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b, long c) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b, c); return false; };
    if (V < 1 || eot < 1 || eot >= V) return fail("grammar: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1, 0);
    if (n_states < 1 || n_states > GRAMMAR_MAX_STATES) return fail("grammar: %ld states outside 1..%ld", n_states, GRAMMAR_MAX_STATES, 0);
    if (!edge_off || !accept) return fail("grammar: null argument", 0, 0, 0);
    if (edge_off[0] != 0) return fail("grammar: edge_off[0] must be 0", 0, 0, 0);
    for (int n = 0; n < n_states; ++n)
        if (edge_off[n + 1] < edge_off[n] || edge_off[n + 1] > GRAMMAR_MAX_EDGES)
            return fail("grammar: state %ld ends at edge %ld (offsets ascend, at most %ld edges)", n, edge_off[n + 1], GRAMMAR_MAX_EDGES);
    if (edge_off[n_states] > 0 && (!edge_tok || !edge_next)) return fail("grammar: null argument", 0, 0, 0);
    for (int n = 0; n < n_states; ++n) {
        if (accept[n] != 0 && accept[n] != 1) return fail("grammar: accept[%ld] is %ld, not 0 or 1", n, accept[n], 0);
        for (int i = edge_off[n]; i < edge_off[n + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] >= eot)
                return fail("grammar: edge token %ld of state %ld is no text token (0..%ld, below end-of-text)", edge_tok[i], n, (long)eot - 1);
            if (i > edge_off[n] && edge_tok[i] <= edge_tok[i - 1]) return fail("grammar: the edge tokens of state %ld do not ascend", n, 0, 0);
            if (edge_next[i] < 0 || edge_next[i] >= n_states)
                return fail("grammar: edge %ld leads to state %ld outside 0..%ld", i, edge_next[i], (long)n_states - 1);
        }
    }
    return true;
}

// a CHECKED table into a block of GRAMMAR_TABLE_INTS ints -> the ints in use from the block's start up to the last edge_next; the accept
// region (at its fixed place) is n_states ints more
inline void grammar_table_pack(int* block, int eot, int n_states, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                               const int32_t* accept) {
    const int n_edges = edge_off[n_states];
    block[0] = n_states; block[1] = n_edges; block[2] = eot; block[3] = 0;
    memcpy(block + GRAMMAR_OFF_AT, edge_off, sizeof(int) * (size_t)(n_states + 1));
    if (n_edges) {
        memcpy(block + GRAMMAR_TOK_AT, edge_tok, sizeof(int) * (size_t)n_edges);
        memcpy(block + GRAMMAR_NEXT_AT, edge_next, sizeof(int) * (size_t)n_edges);
    }
    memcpy(block + GRAMMAR_ACCEPT_AT, accept, sizeof(int) * (size_t)n_states);
}

}  // namespace wlx
