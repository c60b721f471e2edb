"""NumPy restatement of what dec_grammar_kernel (csrc/dec_grammar.hip) does with a grammar table (include/wlx_grammar.h): the walk to a
row's state and the mask of its logits, on the arrays wlx_grammar_set takes. No arithmetic touches a logit, so the comparison with the
device is on the uint32 view of the rows: a word is what it was, or NEG_INF."""
import numpy as np

NEG_INF = np.uint32(0xff800000)


def next_state(g, parent_state: int, token: int, pos: int, plen: int) -> int:
    """state of a row fed `token` at position `pos` of a prompt of `plen` tokens, whose parent row was in `parent_state` at pos - 1"""
    if pos < plen or pos < 1:
        return 0
    ps = int(parent_state)
    if ps < 0 or ps >= g.n_states:
        ps = 0                                  # what another table left behind
    if token >= g.eot:
        return ps                               # specials and timestamps are transparent
    a, b = int(g.edge_off[ps]), int(g.edge_off[ps + 1])
    hit = np.nonzero(g.edge_tok[a:b] == token)[0]
    return int(g.edge_next[a + hit[0]]) if hit.size else 0


def mask_row(g, row: np.ndarray, state: int) -> np.ndarray:
    """the mask on one float32 logits row, in place: text tokens that are no edge of `state`, and end-of-text unless it accepts"""
    assert row.dtype == np.float32
    bits = row.view(np.uint32)
    keep = np.zeros(g.eot + 1, bool)
    keep[g.edge_tok[int(g.edge_off[state]):int(g.edge_off[state + 1])]] = True
    keep[g.eot] = bool(g.accept[state])
    bits[:g.eot + 1][~keep] = NEG_INF
    return row


def apply(g, logits: np.ndarray, tokens, pos, parent, plen: int, nsp_row, prev_state):
    """one launch as wlx_debug_grammar_apply describes it: (logits out [rows][ldl], state_out [rows]); `logits` is not changed"""
    out = np.array(logits, dtype=np.float32, copy=True)
    states = np.zeros(len(tokens), np.int16)
    for r in range(len(tokens)):
        s = next_state(g, prev_state[r], int(tokens[r]), int(pos[r]), plen)
        states[r] = s
        if nsp_row[r] <= 0:
            mask_row(g, out[r], s)
    return out, states
