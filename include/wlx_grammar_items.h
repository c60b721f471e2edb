/* wlx_grammar_items.h — the per-item part of grammar-constrained decoding in the C-ABI of libwlx.so. Included by wlx.h (inside its
 * extern "C" block, behind the types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_GRAMMAR_ITEMS_H
#define WLX_GRAMMAR_ITEMS_H

/* ---- a grammar per item: a POOL of DFAs on the slot, one selected per item of a decode group ----
 * wlx_grammar_set_items installs up to WLX_GRAMMAR_SET_MAX_TABLES tables and puts the slot into per-item grammar mode: every decode
 * step then runs ONE launch of dec_grammar_items_kernel (csrc/dec_grammar.hip) where the single-grammar mode runs dec_grammar_kernel,
 * with the same semantics per row (wlx_grammar.h), the table being the one selected for the row's item. An item without a table (-1)
 * decodes unconstrained: its logits are not touched, its state is written as 0.
 * Layout, tables back to back, each in the exact format of wlx_grammar_set: n_states[t] per table; edge_off holds n_states[t] + 1
 * offsets per table, LOCAL to the table (each run starts at 0); edge_tok / edge_next hold each table's edges (state 0's first), the
 * tokens ascending within a state and all below `eot`, edge_next any state 0..n_states[t] - 1 of THAT table; accept holds n_states[t]
 * values 0 or 1 per table. A state is a number local to its table (so it fits the array the bias modes share); a state the row's
 * parent holds that is out of range for the SELECTED table counts as the start state.
 * The set is checked into a host copy first. WLX_ERR_ARG, before any upload and with whatever is installed left whole: n_tables outside
 * 1..WLX_GRAMMAR_SET_MAX_TABLES; a table past WLX_GRAMMAR_MAX_STATES or WLX_GRAMMAR_MAX_EDGES, or with any violation wlx_grammar_set
 * refuses; more than WLX_GRAMMAR_SET_MAX_STATES states or WLX_GRAMMAR_SET_MAX_EDGES edges over all tables; eot outside 1..vocab - 1; a
 * null array.
 * The pool, its pinned staging and the selection live in buffers of the slot at fixed addresses (allocated at the first call), so
 * captured step graphs replay across sets and selections; only the used part of the pool is copied, asynchronously on the slot's
 * stream. After the call EVERY item is deselected (-1) for max_batch items: generate calls decode unconstrained until
 * wlx_grammar_select.
 * wlx_grammar_select: wlx_bias_select's contract. table_of_item[b] (-1: none) is the table of item b of the FOLLOWING generate calls —
 * b is the position in the call's batch — until the next select, set or clear. WLX_ERR_ARG: n outside 1..max_batch, an entry outside
 * -1..n_tables - 1, a null array; WLX_ERR_STATE: the slot is not in per-item grammar mode. In that mode a generate (or
 * wlx_debug_search[_batch]) whose batch exceeds the selected n is refused with WLX_ERR_STATE, and one whose opts->ids.eot differs from
 * the pool's `eot` with WLX_ERR_ARG.
 * ONE mode at a time, and the last set call decides: wlx_grammar_set, wlx_bias_set and wlx_bias_set_items take the slot out of this
 * mode (the pool stays on the device but is not applied), wlx_grammar_clear and wlx_bias_clear clear it. A grammar together with
 * keyword boosting on one slot is not served. */
#define WLX_GRAMMAR_SET_MAX_TABLES 64
#define WLX_GRAMMAR_SET_MAX_STATES 16384
#define WLX_GRAMMAR_SET_MAX_EDGES 65536
int32_t wlx_grammar_set_items(wlx_engine* e, int32_t slot, int32_t eot, int32_t n_tables, const int32_t* n_states, const int32_t* edge_off,
                              const int32_t* edge_tok, const int32_t* edge_next, const int32_t* accept);
int32_t wlx_grammar_select(wlx_engine* e, int32_t slot, int32_t n, const int32_t* table_of_item);

/* ONE launch of the per-item kernel (launch_dec_grammar_items). wlx_debug_bias_apply_items' conventions: a set as
 * wlx_grammar_set_items takes it (checked the same way against `vocab` and `eot`), `items` items of R rows each (items in 1..64,
 * items * R <= 320, beam mode), sel[items] the table of each item (-1: none), plen[items] the prompt length of each item; tokens / pos /
 * parent / nsp_row / prev_state / state_out per row, parent being a row of the whole launch. wlx_debug_grammar_apply's conventions:
 * logits [items * R][ldl] float32 (vocab <= ldl <= 2^20) FOLLOWED BY WLX_DEBUG_GUARD words, all copied in AND out; prev_state may be ANY
 * number 0..32767. Every refusal (WLX_ERR_ARG) comes before any launch, with logits and state_out untouched. */
int32_t wlx_debug_grammar_apply_items(int32_t device, int32_t vocab, int32_t eot, int32_t n_tables, const int32_t* n_states,
                                      const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const int32_t* accept,
                                      float* logits, int32_t items, int32_t R, const int32_t* sel, int64_t ldl, const int32_t* tokens,
                                      const int32_t* pos, const int32_t* parent, const int32_t* plen, const int32_t* nsp_row,
                                      const int16_t* prev_state, int16_t* state_out);

#endif /* WLX_GRAMMAR_ITEMS_H */
