/* wlx_pattern_items.h — the per-item part of regular-expression grammars in the C-ABI of libwlx.so. Included by wlx.h (inside its
 * extern "C" block, behind the types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_PATTERN_ITEMS_H
#define WLX_PATTERN_ITEMS_H

/* ---- a pattern per item: a POOL of byte DFAs on the slot, one selected per item of a decode group ----
 * wlx_pattern_set_items installs up to WLX_PATTERN_SET_MAX_TABLES tables and puts the slot into per-item pattern mode: every decode
 * step then runs ONE launch of dec_pattern_items_kernel (csrc/dec_pattern.hip) where the single-pattern mode runs dec_pattern_kernel,
 * with the same semantics per row (wlx_pattern.h), the table being the one selected for the row's item. The launch has one workgroup
 * per (item, tile of the vocabulary), which stages the item's table and the tile's bytes once for all beam rows of the item. An item
 * without a table (-1) decodes unconstrained: its logits are not touched, its states are written as 0.
 * Layout, tables back to back, each in the exact format of wlx_pattern_set: n_states[t] and n_classes[t] per table; byte_class holds
 * 256 bytes per table; trans holds n_states[t] * n_classes[t] cells per table and accept n_states[t] bytes per table, concatenated
 * without pads (the library aligns each table's cells on 16 bytes in its own copy). A state is a number local to its table (so it fits
 * the array all modes share); a state the row's parent holds that is out of range for the SELECTED table counts as the start state.
 * The vocabulary bytes are the engine's (wlx_pattern_vocab_set): WLX_ERR_STATE without them.
 * The set is checked into a host copy first. WLX_ERR_ARG, before any upload and with whatever is installed left whole: n_tables outside
 * 1..WLX_PATTERN_SET_MAX_TABLES; a table with any violation wlx_pattern_set refuses (WLX_PATTERN_MAX_STATES, 256 classes,
 * WLX_PATTERN_MAX_CELLS, a class or a transition out of range, an accept value other than 0 or 1); more than
 * WLX_PATTERN_SET_MAX_CELLS cells or WLX_PATTERN_SET_MAX_STATES states over all tables; eot outside 1..vocab - 1 or different from the
 * vocabulary bytes' eot; a null array.
 * The pool, its pinned staging and the selection live in buffers of the slot at fixed addresses (allocated at the first call), so
 * captured step graphs replay across sets and selections; only the used parts of the pool are copied, asynchronously on the slot's
 * stream. After the call EVERY item is deselected (-1) for max_batch items: generate calls decode unconstrained until
 * wlx_pattern_select.
 * wlx_pattern_select: wlx_grammar_select's contract. table_of_item[b] (-1: none) is the table of item b of the FOLLOWING generate
 * calls — b is the position in the call's batch — until the next select, set or clear. WLX_ERR_ARG: n outside 1..max_batch, an entry
 * outside -1..n_tables - 1, a null array; WLX_ERR_STATE: the slot is not in per-item pattern mode. In that mode a generate (or
 * wlx_debug_search[_batch]) whose batch exceeds the selected n is refused with WLX_ERR_STATE, and one whose opts->ids.eot differs from
 * the pool's `eot` with WLX_ERR_ARG.
 * ONE mode at a time, and the last set call decides: every other set call (wlx_pattern_set, wlx_grammar_set[_items],
 * wlx_bias_set[_items]) takes the slot out of this mode (the pool stays on the device but is not applied), wlx_pattern_clear and
 * wlx_bias_clear clear it. A pattern together with keyword boosting or a phrase list on one slot is not served. */
#define WLX_PATTERN_SET_MAX_TABLES 64
#define WLX_PATTERN_SET_MAX_CELLS 393216
#define WLX_PATTERN_SET_MAX_STATES 65536
int32_t wlx_pattern_set_items(wlx_engine* e, int32_t slot, int32_t eot, int32_t n_tables, const int32_t* n_states, const int32_t* n_classes,
                              const uint8_t* byte_class, const uint16_t* trans, const uint8_t* accept);
int32_t wlx_pattern_select(wlx_engine* e, int32_t slot, int32_t n, const int32_t* table_of_item);

/* ONE launch of the per-item kernel (launch_dec_pattern_items). wlx_debug_grammar_apply_items' conventions for the rows: `items` items
 * of R rows each (items in 1..64, R in 1..16, items * R <= 320, beam mode), sel[items] the table of each item (-1: none), plen[items]
 * the prompt length of each item; tokens / pos / parent / nsp_row / prev_state / state_out per row, parent being a row of the whole
 * launch. wlx_debug_pattern_apply's conventions for the rest: a set as wlx_pattern_set_items takes it and vocabulary bytes as
 * wlx_pattern_vocab_set takes them (both checked the same way against `vocab` and `eot`), logits [items * R][ldl] float32
 * (vocab <= ldl <= 2^20) FOLLOWED BY WLX_DEBUG_GUARD words, all copied in AND out; prev_state may be ANY number 0..32767. Every refusal
 * (WLX_ERR_ARG) comes before any launch, with logits and state_out untouched. */
int32_t wlx_debug_pattern_apply_items(int32_t device, int32_t vocab, int32_t eot, int32_t n_tables, const int32_t* n_states,
                                      const int32_t* n_classes, const uint8_t* byte_class, const uint16_t* trans, const uint8_t* accept,
                                      const int32_t* tok_off, const uint8_t* bytes, float* logits, int32_t items, int32_t R,
                                      const int32_t* sel, int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent,
                                      const int32_t* plen, const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out);

#endif /* WLX_PATTERN_ITEMS_H */
