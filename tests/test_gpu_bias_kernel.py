"""GPU (-m gpu): ONE launch of dec_bias_kernel (csrc/dec_bias.hip) through wlx_debug_bias_apply against the NumPy restatement
whisperlive_amd/biasing.py: logits and states bit for bit. Boosts and values are exact in float32 (0.5, 2.0, -4.0), so the device's single
add per pass equals NumPy's."""
import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import biasing as B

pytestmark = pytest.mark.gpu

VOCAB, EOT, LDL = 1000, 900, 1008          # ldl > vocab: the pad columns must come back untouched


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def apply_gpu(table, logits, tokens, pos, parent, plen, nsp, prev_state, vocab=VOCAB, eot=EOT):
    lib = _lib.load()
    rows, ldl = logits.shape
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    tokens, pos, parent, nsp = i32(tokens), i32(pos), i32(parent), i32(nsp)
    prev = np.ascontiguousarray(prev_state, dtype=np.int16)
    state = np.full(rows, -1, np.int16)
    off, tok, nxt, ids = i32(table.edge_off), i32(table.edge_tok), i32(table.edge_next), i32(table.tok_ids)
    vals = np.ascontiguousarray(table.tok_vals, dtype=np.float32)
    _lib.check(lib.wlx_debug_bias_apply(0, vocab, eot, table.n_nodes, _p(off, C.c_int32), _p(tok, C.c_int32), _p(nxt, C.c_int32),
                                        float(table.boost), ids.size, _p(ids, C.c_int32), _p(vals, C.c_float), _p(out, C.c_float), rows, ldl,
                                        _p(tokens, C.c_int32), _p(pos, C.c_int32), _p(parent, C.c_int32), plen, _p(nsp, C.c_int32),
                                        _p(prev, C.c_int16), _p(state, C.c_int16)))
    return out, state


def apply_ref(table, logits, tokens, pos, plen, nsp, prev_state):
    out = logits.copy()
    states = np.zeros(len(tokens), np.int16)
    for r, tk in enumerate(tokens):
        s = table.next_state(int(prev_state[r]), int(tk)) if pos[r] >= plen else 0
        states[r] = s
        if not nsp[r]:
            table.bias_row(out[r, :table.vocab], s)
    return out, states


def _logits(rows, seed):
    return (np.random.default_rng(seed).standard_normal((rows, LDL)) * 3).astype(np.float32)


@pytest.fixture(scope="module")
def fan(gpu):
    """a table whose nodes have 0 .. 65 explicit edges: phrases [t, c] for c in a fan under first tokens 10 (1 child), 11 (63), 12 (64),
    13 (65) — the node after 10 / 11 / 12 / 13 carries its children plus the root's four edges — and a logit_bias list that names an edge
    token (200), token 0 and vocab - 1"""
    phrases = [[10, 200]] + [[11, 300 + i] for i in range(59)] + [[12, 400 + i] for i in range(60)] + [[13, 500 + i] for i in range(61)]
    t = B.compile_bias(phrases, 0.5, {200: 2.0, 0: -4.0, VOCAB - 1: 2.0, 10: -4.0}, vocab=VOCAB, eot=EOT)
    n = lambda path: t.paths.index(tuple(path))
    sizes = {len(t.edges(n(p))[0]) for p in ([10], [11], [12], [13])}
    assert sizes == {5, 63, 64, 65} and len(t.edges(0)[0]) == 4, sizes
    return t, n


def test_edge_counts_at_the_lane_stride_boundaries(fan):
    """parents in nodes with 4, 5, 63, 64 and 65 edges; the fed token is the first, the last, one in the second stride, or none of the
    node's edges; the new node then has 4 (a phrase end: the root's), 63, 64, 65 edges to boost"""
    t, n = fan
    cases = [(0, 10), (0, 13), (0, 77), (n([10]), 200), (n([10]), 12), (n([11]), 300), (n([11]), 358), (n([12]), 400), (n([12]), 459),
             (n([12]), 13), (n([13]), 500), (n([13]), 560), (n([13]), 559), (n([13]), 10), (n([13]), 899), (n([13]), 900), (n([13]), 999)]
    rows = len(cases)
    lg = _logits(rows, 1)
    tokens, prev = [c[1] for c in cases], [c[0] for c in cases]
    pos, parent, nsp = [7] * rows, list(range(rows)), [0] * rows
    got, gs = apply_gpu(t, lg, tokens, pos, parent, 3, nsp, prev)
    ref, rs = apply_ref(t, lg, tokens, pos, 3, nsp, prev)
    assert gs.tolist() == rs.tolist()
    assert rs[-2] == 0 and rs[-1] == 0 and rs[3] == n([10, 200])             # >= eot resets; a phrase end is reached
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got[:, VOCAB:], lg[:, VOCAB:])


def test_a_node_without_edges_and_an_empty_token_list(gpu):
    t = B.compile_bias([], 2.0, {}, vocab=VOCAB, eot=EOT)                   # the root alone, 0 edges, 0 list entries
    lg = _logits(5, 2)
    got, gs = apply_gpu(t, lg, [1, 2, 3, 4, 5], [4] * 5, list(range(5)), 2, [0] * 5, [0] * 5)
    assert np.array_equal(got, lg) and gs.tolist() == [0] * 5
    one = B.compile_bias([[7]], 2.0, {}, vocab=VOCAB, eot=EOT)            # the root with exactly one edge
    assert len(one.edges(0)[0]) == 1
    got, gs = apply_gpu(one, lg, [1, 7, 3, 4, 5], [4] * 5, list(range(5)), 2, [0] * 5, [0] * 5)
    ref, rs = apply_ref(one, lg, [1, 7, 3, 4, 5], [4] * 5, 2, [0] * 5, [0] * 5)
    assert gs.tolist() == rs.tolist() == [0, 1, 0, 0, 0] and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (got[:, 7] == lg[:, 7] + np.float32(2.0)).all()


def test_list_token_equal_to_an_edge_token_takes_both_adds_in_order(fan):
    """the root boosts token 10 by 0.5 and the list then adds -4.0 to it: (x + 0.5) + -4.0 in float32, at x = 2^23 + 1 where the order
    shows (0.5 first rounds up to 2^23 + 2; -4.0 first would leave 2^23 - 2.5 exact); token 200 takes both in node [10]; tokens 0 and
    vocab - 1 with ldl > vocab"""
    t, n = fan
    lg = _logits(2, 3)
    x = np.float32(8388609.0)
    lg[:, 10] = x
    lg[:, 0], lg[:, VOCAB - 1] = np.float32(0.1), np.float32(-0.3)
    got, gs = apply_gpu(t, lg, [77, 10], [5, 5], [0, 1], 1, [0, 0], [0, 0])
    ref, rs = apply_ref(t, lg, [77, 10], [5, 5], 1, [0, 0], [0, 0])
    assert gs.tolist() == rs.tolist() == [0, n([10])]
    first = np.float32(np.float32(x + np.float32(0.5)) + np.float32(-4.0))
    assert first == np.float32(8388606.0) != np.float32(np.float32(x + np.float32(-4.0)) + np.float32(0.5))
    assert got[0, 10] == first and got[1, 10] == first
    assert got[1, 200] == np.float32(np.float32(lg[1, 200] + np.float32(0.5)) + np.float32(2.0))
    assert got[0, 0] == np.float32(np.float32(0.1) + np.float32(-4.0)) and got[0, VOCAB - 1] == np.float32(np.float32(-0.3) + np.float32(2.0))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("rows", [1, 5, 16, 17])
def test_row_counts_parents_positions_and_the_untouched_row(fan, rows):
    """1, 5, 16 and 17 rows; every row's parent is ANOTHER row (a rotation) whose state differs from the row's own; the first generated
    position (pos = plen - 1: the root whatever the parent says), positions 446 and 447, and a row that defines no_speech_prob: its state is
    stored, its logits stay (447: the next test)"""
    t, n = fan
    rng = np.random.default_rng(rows)
    nodes = [0, n([10]), n([11]), n([12]), n([13])]
    plen = 4
    pos = [int(rng.choice([plen - 1, plen + 1, 100, 446])) for _ in range(rows)]     # (no two adjacent: a row's state at p is not another's parent state)
    # rows that share a parent at the same position must agree on its state: the state is a function of (parent, position)
    parent = [(r + 1) % rows for r in range(rows)]
    prev = [nodes[(parent[r] + pos[r]) % 5] for r in range(rows)]
    tokens = [int(rng.choice([10, 11, 12, 13, 200, 300, 459, 560, 5, 950])) for _ in range(rows)]
    nsp = [1 if r == 0 else 0 for r in range(rows)]
    lg = _logits(rows, 10 + rows)
    got, gs = apply_gpu(t, lg, tokens, pos, parent, plen, nsp, prev)
    ref, rs = apply_ref(t, lg, tokens, pos, plen, nsp, prev)
    assert gs.tolist() == rs.tolist()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got[0], lg[0])
    for r in range(rows):
        if pos[r] == plen - 1:
            assert gs[r] == 0


def test_positions_446_and_447_and_the_first_generated_position(fan):
    t, n = fan
    lg = _logits(3, 4)
    got, gs = apply_gpu(t, lg, [200, 200, 200], [446, 447, 2], [0, 1, 0], 3, [0, 0, 0], [n([10])] * 3)
    ref, rs = apply_ref(t, lg, [200, 200, 200], [446, 447, 2], 3, [0, 0, 0], [n([10])] * 3)
    assert gs.tolist() == rs.tolist() == [n([10, 200]), n([10, 200]), 0]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_refusals(gpu):
    t = B.compile_bias([[1, 2]], 0.5, {3: 2.0}, vocab=VOCAB, eot=EOT)
    lg = _logits(1, 5)
    with pytest.raises(_lib.WlxError) as ei:
        apply_gpu(t, lg, [1], [448], [0], 1, [0], [0])
    assert ei.value.code == _lib.ERR_ARG
    bad = B.compile_bias([[1, 2]], 0.5, {3: 2.0}, vocab=VOCAB, eot=EOT)
    bad.edge_next = bad.edge_next.copy(); bad.edge_next[0] = bad.n_nodes
    with pytest.raises(_lib.WlxError) as ei:
        apply_gpu(bad, lg, [1], [4], [0], 1, [0], [0])
    assert ei.value.code == _lib.ERR_ARG and "node" in str(ei.value)
