/* wlx_bias_items.h — the per-item part of keyword boosting in the C-ABI of libwlx.so. Included by wlx.h (inside its extern "C" block,
 * behind the types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_BIAS_ITEMS_H
#define WLX_BIAS_ITEMS_H

/* ---- keyword boosting per item: a SET of tables on the slot, one selected per item of a decode group ----
 * wlx_bias_set_items installs up to WLX_BIAS_SET_MAX_TABLES tables and puts the slot into per-item mode: every decode step then runs ONE
 * launch of dec_bias_items_kernel (csrc/dec_bias.hip) where the single-table mode runs dec_bias_kernel, with the same semantics per row
 * (above), the table being the one selected for the row's item. wlx_bias_set returns the slot to single-table mode; wlx_bias_clear
 * clears either mode.
 * A table is given in the COMPACT form of the same automaton: node 0's list is the root's (its children); node n != 0 lists only its
 * OWN edges, the entries of its closed list that are not identical to the root's entry for that token (the token is not in the
 * root's list, or is there with another next node). An own edge whose token the root's list names too has WLX_BIAS_EDGE_SHARED set
 * in its edge_next. Transition from node n on token t: n's own list, else the root's list, else the root; a token >= eot: the root.
 * Bias of a row in node n: `boost` on every own edge token WITHOUT the flag, `boost` on every token of the root's list (n = 0: the
 * root's list once), then the token list — every token gets exactly the adds the closed table of wlx_bias_set gives it, bit for bit.
 * Layout, tables back to back: n_nodes[t] and n_tok[t] per table; edge_off holds n_nodes[t] + 1 offsets per table, LOCAL to the
 * table (each run starts at 0); edge_tok / edge_next hold each table's edges (node 0's first), ascending by token within a node;
 * boosts[t]; tok_ids / tok_vals hold each table's n_tok[t] entries. A state is a node number local to its table.
 * The set is checked into a host copy first. WLX_ERR_ARG, whatever is installed left whole: n_tables outside
 * 1..WLX_BIAS_SET_MAX_TABLES; a table with n_nodes outside 1..WLX_BIAS_MAX_NODES or n_tok outside 0..WLX_BIAS_MAX_TOKENS; more than
 * WLX_BIAS_SET_MAX_NODES nodes, WLX_BIAS_SET_MAX_EDGES edges or WLX_BIAS_SET_MAX_TOKENS token-list entries in all; offsets of a table
 * that do not start at 0 and ascend; edge tokens of a node that do not ascend; a next node outside 1..n_nodes[t] - 1 or other bits
 * in edge_next; a flag that is not set exactly where the root's list has the token; a token outside the vocabulary; a token named
 * twice in one table's tok_ids; a boost or value that is not finite.
 * The pool, its pinned staging and the selection live in buffers of the slot at fixed addresses (allocated at the first call), so
 * captured step graphs replay across sets and selections; only the used part of the pool is copied, asynchronously on the slot's
 * stream. After the call EVERY item is deselected (-1) for max_batch items: generate calls decode unbiased until wlx_bias_select.
 * wlx_bias_select: table_of_item[b] (-1: none) is the table of item b of the FOLLOWING generate calls — b is the position in the
 * call's batch (the decode group), not the encoder item of wlx_generate_ex — until the next select, set or clear. WLX_ERR_ARG: n
 * outside 1..max_batch, an entry outside -1..n_tables - 1; WLX_ERR_STATE: the slot is not in per-item mode. In per-item mode a
 * generate (or wlx_debug_search[_batch]) whose batch exceeds the selected n is refused with WLX_ERR_STATE. */
#define WLX_BIAS_SET_MAX_TABLES 64
#define WLX_BIAS_SET_MAX_NODES 16384
#define WLX_BIAS_SET_MAX_EDGES 65536
#define WLX_BIAS_SET_MAX_TOKENS 4096
#define WLX_BIAS_EDGE_SHARED 0x40000000
int32_t wlx_bias_set_items(wlx_engine* e, int32_t slot, int32_t n_tables, const int32_t* n_nodes, const int32_t* edge_off,
                           const int32_t* edge_tok, const int32_t* edge_next, const float* boosts, const int32_t* n_tok,
                           const int32_t* tok_ids, const float* tok_vals);
int32_t wlx_bias_select(wlx_engine* e, int32_t slot, int32_t n, const int32_t* table_of_item);

/* ONE launch of the per-item kernel (dec_bias_items_kernel), wlx_debug_bias_apply's conventions: a set as wlx_bias_set_items takes it
 * (checked the same way), `items` items of R rows each (items in 1..64, items * R <= 320, beam mode), sel[items] the table of each item
 * (-1: none), plen[items] the prompt length of each item; tokens / pos / parent / nsp_row / prev_state / state_out per row, parent
 * being a row of the whole launch. prev_state may be ANY node number 0..32767: one past the selected table's nodes is what another
 * table left behind and is read as the root. */
int32_t wlx_debug_bias_apply_items(int32_t device, int32_t vocab, int32_t eot, int32_t n_tables, const int32_t* n_nodes, const int32_t* edge_off,
                                   const int32_t* edge_tok, const int32_t* edge_next, const float* boosts, const int32_t* n_tok,
                                   const int32_t* tok_ids, const float* tok_vals, float* logits, int32_t items, int32_t R, const int32_t* sel,
                                   int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent, const int32_t* plen,
                                   const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out);

#endif /* WLX_BIAS_ITEMS_H */
