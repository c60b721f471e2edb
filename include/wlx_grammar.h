/* wlx_grammar.h — grammar-constrained decoding in the C-ABI of libwlx.so. Included by wlx.h (inside its extern "C" block, behind the
 * types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_GRAMMAR_H
#define WLX_GRAMMAR_H

/* ---- a closed phrase list in the decode step: a DFA over token ids on the slot (the host compiler is
 * whisperlive_amd/grammar.py) ----
 * While a grammar is installed every decode step of the slot (wlx_generate / wlx_generate_ex in beam and sampling mode, and the
 * wlx_debug_search hooks) runs ONE more launch (csrc/dec_grammar.hip dec_grammar_kernel) between the vocabulary projection and the
 * token search, where keyword boosting runs its own. It sets to -inf, BEFORE anything of the search reads them, every logit of a text
 * token (id < eot) that is no edge token of the row's state, and the logit of eot unless the state accepts; edge tokens, ids above
 * eot (specials, timestamps) and the columns behind the vocabulary keep their bits. No logit is computed: a word is what it was, or
 * 0xff800000. Normalisation, suppress mask, timestamp rules, penalties and sampling all see the masked row, and the scores are those
 * of the masked distribution. A grammar whose state allows only tokens that the call's suppress list removes leaves a row without
 * any finite logit, which is outside the search's contract: compile the grammar from tokens the call does not suppress.
 * Format: state n (0 = the start state) owns the edges [edge_off[n], edge_off[n + 1]) of (edge_tok, edge_next), the tokens
 * ascending within a state and all below eot; edge_next is any state 0..n_states - 1 (0 is a legal target); accept[n] is 0 or 1.
 * State of a row at position p: the start state while the fed token is a prompt token (p below the prompt length: the first
 * generated position); the state of its parent row at p - 1 where the fed token is >= eot (a timestamp inside a phrase is
 * transparent; the bias walk returns to its root there); else next(parent's state, token), the start state where the parent's state
 * has no edge for the token (a caller-forced prefix) — and a parent's state outside 0..n_states - 1, which another grammar or a bias
 * table left behind, counts as the start state. The states live per (cache row, position) in the array the bias modes use and follow
 * the beam's re-ordering. A row whose raw distribution defines no_speech_prob inside the search is not masked at that step (its state
 * is written): no_speech_prob is the same with and without a grammar. One grammar serves every item of the decode group.
 * `eot` is the end-of-text id the table is checked against; a generate whose opts->ids.eot differs is refused with WLX_ERR_ARG.
 * The table and the pinned staging of the upload live in buffers of the slot at fixed addresses (allocated at the first call):
 * captured step graphs stay valid across calls and across grammars. The upload is asynchronous on the slot's stream.
 * ONE mode at a time, and the last set call decides, as wlx_bias_set over wlx_bias_set_items does: wlx_grammar_set takes the slot out
 * of either keyword mode (the table or set stays on the device but is not applied), wlx_bias_set / wlx_bias_set_items take it out of
 * grammar mode. A grammar together with keyword boosting on one slot is not served.
 * WLX_ERR_ARG, whatever is installed left whole: eot outside 1..vocab - 1; n_states outside 1..WLX_GRAMMAR_MAX_STATES; more than
 * WLX_GRAMMAR_MAX_EDGES edges; offsets that do not start at 0 and ascend; edge tokens of a state that do not ascend; a token below 0
 * or >= eot (so also every token outside the vocabulary); an edge_next outside 0..n_states - 1; an accept value other than 0 or 1; a
 * null array.
 * wlx_grammar_clear: a slot in grammar mode decodes without the launch again — its step is the launch list of a slot that never had
 * a grammar; a slot in another mode is left as it is (wlx_bias_clear clears every mode, this one included). */
#define WLX_GRAMMAR_MAX_STATES 4096
#define WLX_GRAMMAR_MAX_EDGES 16384
int32_t wlx_grammar_set(wlx_engine* e, int32_t slot, int32_t eot, int32_t n_states, const int32_t* edge_off, const int32_t* edge_tok,
                        const int32_t* edge_next, const int32_t* accept);
int32_t wlx_grammar_clear(wlx_engine* e, int32_t slot);

/* ONE launch of the grammar kernel (launch_dec_grammar), wlx_debug_bias_apply's conventions and arguments with `accept` in place of
 * the boost and the token list: a table as wlx_grammar_set takes it (checked the same way against `vocab` and `eot`), `rows` decoder
 * rows of ONE item in beam mode (1..320), logits [rows][ldl] float32 (vocab <= ldl <= 2^20) FOLLOWED BY WLX_DEBUG_GUARD words, all
 * copied in AND out: a store past the last row shows in the guard. tokens[r] in 0..vocab - 1. prev_state may be ANY number 0..32767:
 * one past the table's states is what another table left behind and is read as the start state. Every refusal (WLX_ERR_ARG) comes
 * before any launch, with logits and state_out untouched. */
int32_t wlx_debug_grammar_apply(int32_t device, int32_t vocab, int32_t eot, int32_t n_states, const int32_t* edge_off, const int32_t* edge_tok,
                                const int32_t* edge_next, const int32_t* accept, float* logits, int32_t rows, int64_t ldl,
                                const int32_t* tokens, const int32_t* pos, const int32_t* parent, int32_t plen, const int32_t* nsp_row,
                                const int16_t* prev_state, int16_t* state_out);

#endif /* WLX_GRAMMAR_H */
