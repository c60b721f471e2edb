/* wlx_lm_items.h — the per-item part of n-gram language-model fusion in the C-ABI of libwlx.so. Included by wlx.h (inside its
 * extern "C" block, behind the types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_LM_ITEMS_H
#define WLX_LM_ITEMS_H

/* ---- a model and a weight per item: a POOL of (model, weight) entries on the slot, one selected per item of a decode group
 *  ----
 * wlx_lm_set_items installs up to WLX_LM_SET_MAX_ENTRIES entries and puts the slot into per-item fusion mode: every decode step then
 * runs ONE launch of dec_lm_items_kernel (csrc/dec_lm.hip) where the single-model mode runs dec_lm_kernel, with the same semantics per
 * row (wlx_lm.h) and the same arithmetic in the same order: a row of an item whose entry is (lm, w) gets, bit for bit, what wlx_lm_set(lm,
 * w) would give it. The launch has one workgroup per (item, row of the item); an item without an entry (-1) is not fused: its workgroups
 * return before they load anything, its logits and its states are not written.
 * An entry is models[i], a model of THIS engine (wlx_lm_create; the models stay the engine's, at most WLX_LM_MAX_MODELS), and
 * weights[i] (finite, > 0): two entries may name one model at different weights. The slot keeps a small descriptor per entry — the
 * model's arrays and the weight — in a pool at a fixed device address and the selection at another, and the kernel reads both from
 * memory: captured step graphs replay across pools and selections. The states live in the array wlx_lm_set uses; a state the row's
 * parent holds that is out of range for the SELECTED entry's model (another model wrote it) reads as that model's start state.
 * WLX_ERR_ARG, before any upload and with whatever is installed left whole: n_entries outside 1..WLX_LM_SET_MAX_ENTRIES, an entry that
 * names no live model, a weight that is not finite or not above 0, entries whose models were built for different end-of-text ids, a
 * null array. After the call EVERY item is deselected (-1) for max_batch items: generate calls decode unfused until wlx_lm_select.
 * wlx_lm_destroy refuses (WLX_ERR_STATE) a model that an entry of a slot's pool names, until wlx_lm_clear or wlx_bias_clear.
 * wlx_lm_select: wlx_grammar_select's contract. sel[b] (-1: none) is the entry of item b of the FOLLOWING generate calls — b is the
 * position in the call's batch — until the next select, set or clear. WLX_ERR_ARG: batch outside 1..max_batch, an entry outside
 * -1..n_entries - 1, a null array; WLX_ERR_STATE: the slot is not in per-item fusion mode. In that mode a generate (or
 * wlx_debug_search[_batch]) whose batch exceeds the selected one is refused with WLX_ERR_STATE, and one whose opts->ids.eot differs from
 * the entries' with WLX_ERR_ARG.
 * ONE mode at a time, and the last set call decides: every other set call (wlx_lm_set, wlx_pattern_set[_items],
 * wlx_grammar_set[_items], wlx_bias_set[_items]) takes the slot out of this mode (the pool stays on the device but is not applied),
 * wlx_lm_clear and wlx_bias_clear clear it. A model together with keyword boosting or a grammar on one slot is not served. */
#define WLX_LM_SET_MAX_ENTRIES 64
int32_t wlx_lm_set_items(wlx_engine* e, int32_t slot, int32_t n_entries, const int32_t* models, const float* weights);
int32_t wlx_lm_select(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* sel);

/* ONE launch of the per-item kernel (launch_dec_lm_items). wlx_debug_pattern_apply_items' conventions for the rows: `items` items of R
 * rows each (items in 1..64, R in 1..16, items * R <= 320), sel[items] the entry of each item (-1: none), plen[items] the prompt length
 * of each item; tokens / pos / parent / nsp_row / row_done / prev_state / state_out per row, parent being a row of the whole launch.
 * `sampling` != 0: the rows are the hypotheses of a sampling call and a row with row_done[r] != 0 is finished (left alone); otherwise beam
 * mode, row_done is not read by the kernel. wlx_debug_lm_apply's conventions for the rest: n_models (1..WLX_LM_MAX_MODELS) tables as
 * wlx_lm_create takes them, back to back — order / n_states / start_state per model; edge_off holds n_states[m] + 1 offsets per model,
 * each model's starting at 0; backoff_state / backoff_weight n_states[m] entries per model; edge_tok / edge_logp / edge_next each
 * model's edges; unigram_logp / unigram_next `vocab` entries per model — every one checked like wlx_lm_create's against `vocab` and `eot`;
 * n_entries entries (entry_model[i] in 0..n_models - 1, entry_weight[i]); logits [items * R][ldl] float32 (vocab <= ldl <= 2^20) FOLLOWED
 * BY WLX_DEBUG_GUARD words, all copied in AND out. prev_state may be ANY number >= 0. state_out is copied in AND out as well: the word
 * of a row the launch does not write comes back as it went in. Every refusal (WLX_ERR_ARG) comes before any launch, with logits and
 * state_out untouched. */
int32_t wlx_debug_lm_apply_items(int32_t device, int32_t vocab, int32_t eot, int32_t n_models, const int32_t* order, const int32_t* n_states,
                                 const int32_t* start_state, const int32_t* edge_off, const int32_t* backoff_state, const float* backoff_weight,
                                 const int32_t* edge_tok, const float* edge_logp, const int32_t* edge_next, const float* unigram_logp,
                                 const int32_t* unigram_next, int32_t n_entries, const int32_t* entry_model, const float* entry_weight,
                                 float* logits, int32_t items, int32_t R, int32_t sampling, const int32_t* sel, int64_t ldl,
                                 const int32_t* tokens, const int32_t* pos, const int32_t* parent, const int32_t* plen, const int32_t* nsp_row,
                                 const int32_t* row_done, const int32_t* prev_state, int32_t* state_out);

#endif /* WLX_LM_ITEMS_H */
