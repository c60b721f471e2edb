/* wlx_pattern.h — regular-expression grammars in the C-ABI of libwlx.so. Included by wlx.h (inside its extern "C" block, behind the
 * types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_PATTERN_H
#define WLX_PATTERN_H

/* ---- a regular expression in the decode step: a DFA over the BYTES of the text on the slot (the host compiler is
 * whisperlive_amd/pattern.py) ----
 * A phrase-list grammar (wlx_grammar.h) is a DFA over token ids and admits the tokenisations its compiler enumerated. A pattern is a
 * DFA over bytes: while one is installed every decode step of the slot runs ONE more launch (csrc/dec_pattern.hip dec_pattern_kernel)
 * between the vocabulary projection and the token search, which decides for every row and every text token whether the token's byte
 * string can be walked from the row's state — every tokenisation of a text of the language is admitted, and `\d{8}` is nine states,
 * not 10^8 phrases. No logit is computed: a word is what it was, or 0xff800000.
 * The vocabulary's bytes are engine-wide and go up once (wlx_pattern_vocab_set): tok_off[eot + 1], starting at 0 and ascending, and the
 * concatenated byte strings of the text tokens 0 .. eot - 1 (bytes[tok_off[t] .. tok_off[t + 1])). A token without bytes is never
 * allowed. WLX_ERR_ARG: eot outside 1..vocab - 1, offsets that do not start at 0 and ascend, a token longer than
 * WLX_PATTERN_MAX_TOKEN_BYTES, more than WLX_PATTERN_MAX_VOCAB_BYTES bytes, a null array. A second call with identical contents does
 * nothing; one with different contents is WLX_ERR_STATE (captured step graphs and installed tables rely on the first).
 * The table: byte_class[256] maps a byte to a class 0 .. n_classes - 1; trans[n_states][n_classes] is the next state, 0xFFFF = dead;
 * accept[n] is 0 or 1; state 0 is the start state.
 * State of a row at position p: the start state while the fed token is a prompt token (p below the prompt length, or p < 1); the state
 * of its parent row at p - 1 where the fed token is >= eot (specials and timestamps are transparent); otherwise the walk of the token's
 * bytes from the parent's state — the start state where that walk dies or the token has no bytes (a caller-forced prefix). A parent's
 * state outside 0 .. n_states - 1, left behind by another mode, reads as the start state. The states live per (cache row, position) in
 * the array the bias and grammar modes use and follow the beam's re-ordering.
 * A row whose raw distribution defines no_speech_prob inside the search is not masked at that step (its state is written). Otherwise a
 * text token t < eot keeps its logit iff it has at least one byte and its walk from the row's state does not die; eot keeps its logit
 * iff the state accepts; ids above eot and the columns behind the vocabulary keep their bits. A state from which the call's suppress
 * list removes every allowed token leaves a row without a finite logit, which is outside the search's contract (the host compiler trims
 * states without a completion and Pattern.dead_states finds the rest).
 * wlx_pattern_set: the device block and its pinned staging live in buffers of the slot at fixed addresses (allocated at the first
 * call): captured step graphs stay valid across calls and across patterns. The upload is asynchronous on the slot's stream. ONE mode at
 * a time and the last set call decides, as documented in wlx_grammar.h: wlx_pattern_set takes the slot out of the keyword and grammar
 * modes, their set calls take it out of pattern mode. WLX_ERR_STATE: the engine has no vocabulary bytes yet. WLX_ERR_ARG, whatever is
 * installed left whole: n_states outside 1..WLX_PATTERN_MAX_STATES; n_classes outside 1..256; n_states * n_classes above
 * WLX_PATTERN_MAX_CELLS; a class >= n_classes; a transition that is neither 0xFFFF nor < n_states; an accept value other than 0 or 1; a
 * null array; eot different from the vocabulary bytes' eot. A generate whose opts->ids.eot differs is refused with WLX_ERR_ARG.
 * wlx_pattern_clear: a slot in pattern mode decodes without the launch again — its step is the launch list of a slot that never had a
 * pattern; a slot in another mode is left as it is (wlx_bias_clear clears every mode, this one included). */
#define WLX_PATTERN_MAX_STATES 4096
#define WLX_PATTERN_MAX_CELLS 24576
#define WLX_PATTERN_MAX_TOKEN_BYTES 255
#define WLX_PATTERN_MAX_VOCAB_BYTES (1 << 22)
int32_t wlx_pattern_vocab_set(wlx_engine* e, int32_t eot, const int32_t* tok_off, const uint8_t* bytes);
int32_t wlx_pattern_set(wlx_engine* e, int32_t slot, int32_t eot, int32_t n_states, int32_t n_classes, const uint8_t* byte_class,
                        const uint16_t* trans, const uint8_t* accept);
int32_t wlx_pattern_clear(wlx_engine* e, int32_t slot);

/* ONE launch of the pattern kernel (launch_dec_pattern), wlx_debug_grammar_apply's conventions: a table as wlx_pattern_set takes it and
 * vocabulary bytes as wlx_pattern_vocab_set takes them (both checked the same way against `vocab` and `eot`), `rows` decoder rows of ONE
 * item in beam mode (1..320), logits [rows][ldl] float32 (vocab <= ldl <= 2^20) FOLLOWED BY WLX_DEBUG_GUARD words, all copied in AND
 * out: a store past the last row shows in the guard. tokens[r] in 0..vocab - 1. prev_state may be ANY number 0..32767. Every refusal
 * (WLX_ERR_ARG) comes before any launch, with logits and state_out untouched. */
int32_t wlx_debug_pattern_apply(int32_t device, int32_t vocab, int32_t eot, int32_t n_states, int32_t n_classes, const uint8_t* byte_class,
                                const uint16_t* trans, const uint8_t* accept, const int32_t* tok_off, const uint8_t* bytes, float* logits,
                                int32_t rows, int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent, int32_t plen,
                                const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out);

#endif /* WLX_PATTERN_H */
