// grammar_pool.h — the host side of a POOL of grammar tables (wlx_grammar_set_items; dec_grammar.hip dec_grammar_items_kernel) that needs
// no device: the check of the set a caller hands in, and its layout in the block of ints the kernel walks. Plain C++, on top of
// grammar_table.h (every table of a set is a table of wlx_grammar_set): tests/grammar_pool_check.cpp runs it under the host sanitizers.
#pragma once
#include "grammar_table.h"

namespace wlx {

constexpr int GRAMMAR_SET_MAX_TABLES = 64;      // include/wlx_grammar_items.h WLX_GRAMMAR_SET_MAX_TABLES
constexpr int GRAMMAR_SET_MAX_STATES = 16384;   // WLX_GRAMMAR_SET_MAX_STATES, over all tables
constexpr int GRAMMAR_SET_MAX_EDGES = 65536;    // WLX_GRAMMAR_SET_MAX_EDGES, over all tables
// the pool: one header of GRAMMAR_POOL_HDR_INTS ints per table SLOT (so the arrays start at fixed places, whatever the set holds):
// (state base, edge base, n_states, n_edges); then, each at its fixed place and packed back to back over the tables,
// edge_off [states + tables] (n_states + 1 per table, LOCAL to the table's edges), edge_tok [edges], edge_next [edges] (local state
// numbers), accept [states]. Table t of state base sb and edge base eb: its offsets start at OFF_AT + sb + t, its edges at TOK_AT + eb
// and NEXT_AT + eb, its accept flags at ACCEPT_AT + sb.
constexpr int GRAMMAR_POOL_HDR_INTS = 4;
constexpr int GRAMMAR_POOL_OFF_AT = GRAMMAR_SET_MAX_TABLES * GRAMMAR_POOL_HDR_INTS;
constexpr int GRAMMAR_POOL_TOK_AT = GRAMMAR_POOL_OFF_AT + GRAMMAR_SET_MAX_STATES + GRAMMAR_SET_MAX_TABLES;
constexpr int GRAMMAR_POOL_NEXT_AT = GRAMMAR_POOL_TOK_AT + GRAMMAR_SET_MAX_EDGES;
constexpr int GRAMMAR_POOL_ACCEPT_AT = GRAMMAR_POOL_NEXT_AT + GRAMMAR_SET_MAX_EDGES;
constexpr int GRAMMAR_POOL_INTS = GRAMMAR_POOL_ACCEPT_AT + GRAMMAR_SET_MAX_STATES;

// the format of include/wlx_grammar_items.h, violation by violation: true with the totals in *states_out / *edges_out, or false with the
// reason in `msg`. A table's arrays are read only after the tables before it passed and the totals so far are within the caps, and
// within a table grammar_table_check reads nothing past what the counts checked so far allow.
inline bool grammar_pool_check(int V, int eot, int n_tables, const int32_t* n_states, const int32_t* edge_off, const int32_t* edge_tok,
                               const int32_t* edge_next, const int32_t* accept, int* states_out, int* edges_out, char* msg, size_t msg_len) {
    auto fail = [&](const char* fmt, long a, long b) { if (msg && msg_len) snprintf(msg, msg_len, fmt, a, b); return false; };
    if (V < 1 || eot < 1 || eot >= V) return fail("grammar set: eot %ld outside 1..%ld (the vocabulary)", eot, (long)V - 1);
    if (n_tables < 1 || n_tables > GRAMMAR_SET_MAX_TABLES) return fail("grammar set: %ld tables outside 1..%ld", n_tables, GRAMMAR_SET_MAX_TABLES);
    if (!n_states || !edge_off || !accept) return fail("grammar set: null argument", 0, 0);
    long states = 0, edges = 0;
    for (int t = 0; t < n_tables; ++t) {
        const int ns = n_states[t];
        if (ns < 1 || ns > GRAMMAR_MAX_STATES) return fail("grammar set: table %ld has %ld states", t, ns);
        if (states + ns > GRAMMAR_SET_MAX_STATES) return fail("grammar set: more than %ld states in all (at table %ld)", GRAMMAR_SET_MAX_STATES, t);
        const int32_t* off = edge_off + states + t;
        char why[160] = "";
        // (the tokens and nexts of this table start at `edges`; they are read only where this table has edges)
        if (!grammar_table_check(V, eot, ns, off, edge_tok ? edge_tok + edges : nullptr, edge_next ? edge_next + edges : nullptr, accept + states,
                                 why, sizeof(why))) {
            if (msg && msg_len) snprintf(msg, msg_len, "grammar set: table %d: %s", t, why);
            return false;
        }
        states += ns;
        edges += off[ns];
        if (edges > GRAMMAR_SET_MAX_EDGES) return fail("grammar set: more than %ld edges in all (at table %ld)", GRAMMAR_SET_MAX_EDGES, t);
    }
    if (states_out) *states_out = (int)states;
    if (edges_out) *edges_out = (int)edges;
    return true;
}

// a CHECKED set into a block of GRAMMAR_POOL_INTS ints. The used parts: [0, OFF_AT + states + n_tables), `edges` ints at TOK_AT and at
// NEXT_AT, `states` ints at ACCEPT_AT; the headers of the table slots behind n_tables are zeroed (n_states 0: no table)
inline void grammar_pool_pack(int* block, int n_tables, const int32_t* n_states, const int32_t* edge_off, const int32_t* edge_tok,
                              const int32_t* edge_next, const int32_t* accept) {
    int sb = 0, eb = 0;
    memset(block, 0, sizeof(int) * (size_t)GRAMMAR_POOL_OFF_AT);
    for (int t = 0; t < n_tables; ++t) {
        const int ns = n_states[t];
        const int32_t* off = edge_off + sb + t;
        const int ne = off[ns];
        int* hdr = block + t * GRAMMAR_POOL_HDR_INTS;
        hdr[0] = sb; hdr[1] = eb; hdr[2] = ns; hdr[3] = ne;
        memcpy(block + GRAMMAR_POOL_OFF_AT + sb + t, off, sizeof(int) * (size_t)(ns + 1));
        if (ne) {
            memcpy(block + GRAMMAR_POOL_TOK_AT + eb, edge_tok + eb, sizeof(int) * (size_t)ne);
            memcpy(block + GRAMMAR_POOL_NEXT_AT + eb, edge_next + eb, sizeof(int) * (size_t)ne);
        }
        memcpy(block + GRAMMAR_POOL_ACCEPT_AT + sb, accept + sb, sizeof(int) * (size_t)ns);
        sb += ns; eb += ne;
    }
}

}  // namespace wlx
