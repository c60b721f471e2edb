/* wlx_lm.h — n-gram language-model fusion in the C-ABI of libwlx.so. Included by wlx.h (inside its extern "C" block, behind the
 * types it declares): include wlx.h, not this file. WLX_ABI_VERSION stays 1: symbols are only added. */
#ifndef WLX_LM_H
#define WLX_LM_H

/* ---- a backoff n-gram model over token ids, fused into the search (shallow fusion; the host builder is
 * whisperlive_amd/lm.py) ----
 * Keyword boosting is a hint and a grammar a guarantee; this is a prior. While a model is set on a slot every decode step of the slot
 * runs ONE more launch (csrc/dec_lm.hip dec_lm_kernel) between the vocabulary projection and the token search.
 * The model belongs to the ENGINE (at most WLX_LM_MAX_MODELS of them): one model serves every slot, a slot only points at it.
 * Alphabet A: the text tokens 0 .. eot - 1 and eot, which stands for end of sentence. Scores are natural-log float32.
 * The table: states are contexts. State 0 is the empty context: it has no explicit edges, its scores are the dense unigram_logp[vocab]
 * (finite for every token of A; entries above eot are ignored) and its transitions unigram_next[vocab]. State n > 0 carries the edges
 * [edge_off[n], edge_off[n + 1]) — tok ascending within the state, logp the log-probability of the token in that context, next the
 * state after it (the longest known suffix) — and backs off to backoff_state[n], a strictly shorter context, at the price
 * backoff_weight[n]; every chain reaches state 0 within order - 1 links. start_state is the context of the sentence start.
 * State of a row at position p: start_state while the fed token is a prompt token (p below the prompt length, or p < 1); the state of
 * its parent row at p - 1 where the fed token is >= eot (specials and timestamps are transparent); otherwise the parent's state advanced
 * by the token: `next` of the token's edge at the first level of the parent's chain that has one, unigram_next[token] where none has. A
 * parent's state outside 0 .. n_states - 1 reads as start_state. The states live per (cache row, position) in an int32 array of the
 * slot's own and follow the beam's re-ordering.
 * Score s(v), v in A, in state n with chain n = c0, c1 .. ck = 0: logp of v's edge at the first level cj that has one plus the backoff
 * weights of c0 .. c(j-1); unigram_logp[v] plus all the chain's weights where none has.
 * Fusion with weight w > 0: l'(v) = l(v) + w s(v) - c for v in A, c = LSE_A(l + w s) - LSE_A(l): the model moves probability among
 * the text tokens and eot, and the mass of A against the timestamps and specials stays what the acoustic model gave. Ids above eot and
 * the columns behind the vocabulary keep their bits; -inf stays -inf; a row without a finite logit in A is left alone; the row whose raw
 * distribution defines no_speech_prob keeps its logits (its state is written).
 * wlx_lm_create: copies the table to the device, complete on return. WLX_ERR_ARG, nothing created: order outside 1..WLX_LM_MAX_ORDER,
 * n_states outside 1..WLX_LM_MAX_STATES, more than WLX_LM_MAX_EDGES edges, a vocabulary above WLX_LM_MAX_VOCAB, eot outside
 * 1..vocab - 1, offsets that do not start at 0 and ascend, edges on state 0, edge tokens outside A or not ascending, a score or weight
 * that is not finite, a next / backoff / start state outside the table, a backoff chain longer than order - 1 links, a null array.
 * WLX_ERR_STATE: the engine holds WLX_LM_MAX_MODELS models already.
 * wlx_lm_destroy: WLX_ERR_STATE while a slot points at the model.
 * wlx_lm_set: the slot points at model `lm` with weight `weight` (finite, > 0). A small descriptor of the slot at a fixed device
 * address names the model's arrays and the weight, and the kernel reads it from memory: captured step graphs serve any model and any
 * weight. ONE mode at a time and the last set call decides, as documented in wlx_grammar.h. A generate whose opts->ids.eot differs from
 * the model's is refused with WLX_ERR_ARG. A model and a weight PER ITEM of a decode group is wlx_lm_set_items (wlx_lm_items.h).
 * wlx_lm_clear: a slot in this mode (or in the per-item one) decodes without the launch again — its step is the launch list of a slot that never had a model —
 * and points at no model; a slot in another mode only stops pointing at one (wlx_bias_clear clears every mode, this one included). */
#define WLX_LM_MAX_ORDER 5
#define WLX_LM_MAX_STATES (1 << 20)
#define WLX_LM_MAX_EDGES (1 << 22)
#define WLX_LM_MAX_VOCAB 65536
#define WLX_LM_MAX_MODELS 8
int32_t wlx_lm_create(wlx_engine* e, int32_t eot, int32_t order, int32_t n_states, int32_t start_state, const int32_t* edge_off,
                      const int32_t* backoff_state, const float* backoff_weight, const int32_t* edge_tok, const float* edge_logp,
                      const int32_t* edge_next, const float* unigram_logp, const int32_t* unigram_next, int32_t* lm_out);
int32_t wlx_lm_destroy(wlx_engine* e, int32_t lm);
int32_t wlx_lm_set(wlx_engine* e, int32_t slot, int32_t lm, float weight);
int32_t wlx_lm_clear(wlx_engine* e, int32_t slot);

/* ONE launch of the fusion kernel (launch_dec_lm), wlx_debug_pattern_apply's conventions: a table as wlx_lm_create takes it (checked the
 * same way against `vocab` and `eot`), `rows` decoder rows of ONE item in beam mode (1..320), logits [rows][ldl] float32
 * (vocab <= ldl <= 2^20) FOLLOWED BY WLX_DEBUG_GUARD words, all copied in AND out: a store past the last row shows in the guard.
 * tokens[r] in 0..vocab - 1. prev_state may be ANY number >= 0. Every refusal (WLX_ERR_ARG) comes before any launch, with logits and
 * state_out untouched. */
int32_t wlx_debug_lm_apply(int32_t device, int32_t vocab, int32_t eot, int32_t order, int32_t n_states, int32_t start_state,
                           const int32_t* edge_off, const int32_t* backoff_state, const float* backoff_weight, const int32_t* edge_tok,
                           const float* edge_logp, const int32_t* edge_next, const float* unigram_logp, const int32_t* unigram_next,
                           float weight, float* logits, int32_t rows, int64_t ldl, const int32_t* tokens, const int32_t* pos,
                           const int32_t* parent, int32_t plen, const int32_t* nsp_row, const int32_t* prev_state, int32_t* state_out);

#endif /* WLX_LM_H */
