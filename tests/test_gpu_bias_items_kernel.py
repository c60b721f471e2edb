"""GPU (-m gpu): ONE launch of dec_bias_items_kernel (csrc/dec_bias.hip) through wlx_debug_bias_apply_items: a set of COMPACT tables
(biasing.compile_compact / BiasSet), one selected per item. Logits and states are compared bit for bit with the CLOSED-form NumPy oracle
(biasing.BiasTable.next_state / bias_row on the uncapped closure, compile_bias(max_edges=None)); an item without a table keeps its rows and
takes state 0. Boosts and values are exact in float32 (0.5, 1.5, 2.0, -4.0), so the device's single add per pass equals NumPy's."""
import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd import biasing as B

pytestmark = pytest.mark.gpu

VOCAB, EOT, LDL = 600, 560, 608            # ldl > vocab: the pad columns must come back untouched


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Pair:
    """one phrase list in both forms: `compact` goes to the device, `closed` (no edge cap) is the oracle"""

    def __init__(self, phrases, boost, logit_bias=None):
        self.compact = B.compile_compact(phrases, boost, logit_bias, vocab=VOCAB, eot=EOT)
        self.closed = B.compile_bias(phrases, boost, logit_bias, vocab=VOCAB, eot=EOT, max_edges=None)
        assert self.compact.paths == self.closed.paths

    def n(self, path):
        return self.closed.paths.index(tuple(path))

    def own(self, path):
        return len(self.compact.edges(self.n(path))[0])


def apply_gpu(tables, sel, R, logits, tokens, pos, parent, plen, nsp, prev_state, packed=None):
    lib = _lib.load()
    rows, ldl = logits.shape
    items = len(sel)
    assert rows == items * R
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    tokens, pos, parent, nsp, sel, plen = i32(tokens), i32(pos), i32(parent), i32(nsp), i32(sel), i32(plen)
    prev = np.ascontiguousarray(prev_state, dtype=np.int16)
    state = np.full(rows, -1, np.int16)
    nn, off, tok, nxt, boosts, nt, ids, vals = packed if packed is not None else B.BiasSet(tables).packed()
    _lib.check(lib.wlx_debug_bias_apply_items(0, VOCAB, EOT, len(nn), _p(nn, C.c_int32), _p(off, C.c_int32), _p(tok, C.c_int32), _p(nxt, C.c_int32),
                                              _p(boosts, C.c_float), _p(nt, C.c_int32), _p(ids, C.c_int32), _p(vals, C.c_float), _p(out, C.c_float),
                                              items, R, _p(sel, C.c_int32), ldl, _p(tokens, C.c_int32), _p(pos, C.c_int32), _p(parent, C.c_int32),
                                              _p(plen, C.c_int32), _p(nsp, C.c_int32), _p(prev, C.c_int16), _p(state, C.c_int16)))
    return out, state


def apply_ref(closed, sel, R, logits, tokens, pos, plen, nsp, prev_state):
    """the closed-form oracle: `closed[i]` is the closed table of set entry i"""
    out = logits.copy()
    states = np.zeros(len(tokens), np.int16)
    for r, tk in enumerate(tokens):
        t = sel[r // R]
        if t < 0:
            continue
        tab = closed[t]
        ps = int(prev_state[r]) if 0 <= int(prev_state[r]) < tab.n_nodes else 0           # a stale state past the table: the root
        s = tab.next_state(ps, int(tk)) if pos[r] >= plen[r // R] else 0
        states[r] = s
        if not nsp[r]:
            tab.bias_row(out[r, :VOCAB], s)
    return out, states


def both(pairs, sel, R, lg, tokens, pos, parent, plen, nsp, prev):
    got, gs = apply_gpu([p.compact for p in pairs], sel, R, lg, tokens, pos, parent, plen, nsp, prev)
    ref, rs = apply_ref([p.closed for p in pairs], sel, R, lg, tokens, pos, plen, nsp, prev)
    assert gs.tolist() == rs.tolist()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got[:, VOCAB:], lg[:, VOCAB:])
    return got, gs


def _logits(rows, seed):
    return (np.random.default_rng(seed).standard_normal((rows, LDL)) * 3).astype(np.float32)


@pytest.fixture(scope="module")
def fan(gpu):
    """own lists of 0 / 1 / 63 / 64 / 65 edges under a root list of 4: phrases [t, c] for c in a fan under first tokens 10 (1 child),
    11 (63), 12 (64), 13 (65); the node after [10, 200] ends a phrase and has no own edge. The token list names an own-edge token
    (200), a root-edge token (10), token 0 and vocab - 1."""
    phrases = [[10, 200]] + [[11, 300 + i] for i in range(63)] + [[12, 400 + i] for i in range(64)] + [[13, 480 + i] for i in range(65)]
    p = Pair(phrases, 0.5, {200: 2.0, 0: -4.0, VOCAB - 1: 2.0, 10: -4.0})
    assert [p.own(x) for x in ([10, 200], [10], [11], [12], [13])] == [0, 1, 63, 64, 65] and p.own([]) == 4
    return p


@pytest.fixture(scope="module")
def ab(gpu):
    """two tables with different boosts whose first tokens overlap; A has a token in both lists with a different next ([7, 7, 9]: in
    node [7] token 7 leads to [7, 7], in the root to [7])"""
    a = Pair([[7, 7, 9], [7, 30], [21, 22, 23], [22, 40], [50]], 1.5, {30: 2.0, 3: -4.0})
    b = Pair([[7, 8], [21, 7], [60]], 0.5, {7: 2.0})
    return a, b


def test_four_items_with_tables_a_none_b_a(ab):
    """4 items at R = 5, tables (A, none, B, A): every row's parent is ANOTHER row of its item (a rotation), parent states beyond the
    root; the rows of the item without a table are bitwise unchanged with state 0"""
    a, b = ab
    R, sel, plen = 5, [0, -1, 1, 0], [3, 1, 4, 2]
    rows = 4 * R
    pos = [p for p in (9, 5, 11, 6) for _ in range(R)]
    parent = [it * R + (j + 1) % R for it in range(4) for j in range(R)]
    nodes = {0: [0, a.n([7]), a.n([7, 7]), a.n([21, 22]), a.n([21])], 1: [0, b.n([7]), b.n([21]), 0, b.n([7])]}
    prev = [nodes.get(sel[r // R], [3, 1, 2, 4, 1])[parent[r] % R] for r in range(rows)]
    tokens = [7, 9, 30, 40, 22,   7, 21, 50, 60, 8,   8, 7, 60, 21, 555,   7, 7, 9, 23, 570]
    got, gs = both([a, b], sel, R, _logits(rows, 1), tokens, pos, parent, plen, [0] * rows, prev)
    lg = _logits(rows, 1)
    assert np.array_equal(got[R:2 * R].view(np.uint32), lg[R:2 * R].view(np.uint32)) and gs[R:2 * R].tolist() == [0] * R
    assert len(set(gs.tolist())) > 4                                        # states beyond the root were reached, in both tables
    assert not np.array_equal(got[:R], lg[:R]) and not np.array_equal(got[2 * R:3 * R], lg[2 * R:3 * R])


def test_own_lists_at_the_lane_stride_boundaries(fan):
    """parents in nodes whose own list has 0, 1, 63, 64 and 65 edges; the fed token is the first, the last, one in the second stride or
    none of the own edges, a root token (found in the second search), a token >= eot; the new node then boosts 0 .. 65 own edges"""
    t = fan
    n = t.n
    cases = [(0, 10), (0, 13), (0, 77), (n([10]), 200), (n([10]), 12), (n([10, 200]), 10), (n([10, 200]), 200), (n([11]), 300), (n([11]), 362),
             (n([12]), 400), (n([12]), 463), (n([12]), 13), (n([13]), 480), (n([13]), 544), (n([13]), 543), (n([13]), 10), (n([13]), 559),
             (n([13]), 560), (n([13]), 599)]
    rows = len(cases)
    tokens, prev = [c[1] for c in cases], [c[0] for c in cases]
    got, gs = both([t], [0], rows, _logits(rows, 2), tokens, [7] * rows, list(range(rows)), [3], [0] * rows, prev)
    assert gs[3] == n([10, 200]) and gs[-1] == 0 and gs[-2] == 0 and gs[13] == n([13, 544]) and gs[15] == n([10])


@pytest.mark.parametrize("k", [0, 1, 64, 65])
def test_root_lists_of_0_1_64_65(gpu, k):
    """a root list of k edges (k one-token phrases; with k > 0 one of them goes on, so a node with an own list exists): walks from the
    root and from that node over the root's first, last and second-stride token, and a miss"""
    phrases = [[100 + i] for i in range(k)] + ([[100, 300]] if k else [])
    t = Pair(phrases, 2.0, {5: -4.0})
    assert t.own([]) == k
    node = t.n([100]) if k else 0
    tokens = [100, 100 + max(k - 1, 0), 100 + k, 300, 163, 164, 5, 100]
    prev = [0, 0, 0, node, node, node, node, node]
    rows = len(tokens)
    both([t], [0], rows, _logits(rows, 3 + k), tokens, [6] * rows, list(range(rows)), [2], [0] * rows, prev)


def test_a_token_in_both_lists_takes_the_own_edge_and_one_boost(ab):
    a, _ = ab
    lg = _logits(2, 4)
    got, gs = both([a], [0], 2, lg, [7, 7], [5, 5], [1, 0], [1], [0, 0], [0, a.n([7])])
    assert gs.tolist() == [a.n([7]), a.n([7, 7])]                            # row 1: the own edge of [7] on token 7, not the root's
    # in node [7] token 7 is an own edge AND a root edge: one add of the boost
    assert got[0, 7] == np.float32(lg[0, 7] + np.float32(1.5))
    tok, _, shared = a.compact.edges(a.n([7]))
    assert shared[tok.tolist().index(7)] and not shared[tok.tolist().index(30)]


def test_list_token_equal_to_an_edge_token_takes_both_adds_in_order(fan):
    """token 10 (a root edge) and token 200 (an own edge of [10]) are logit_bias tokens too: (x + boost) + value in float32, at
    x = 2^23 + 1 where the order shows"""
    t = fan
    lg = _logits(2, 5)
    x = np.float32(8388609.0)
    lg[:, 10] = x
    lg[1, 200] = x
    got, gs = both([t], [0], 2, lg, [77, 10], [5, 5], [0, 1], [1], [0, 0], [0, 0])
    assert gs.tolist() == [0, t.n([10])]
    first = np.float32(np.float32(x + np.float32(0.5)) + np.float32(-4.0))
    assert first != np.float32(np.float32(x + np.float32(-4.0)) + np.float32(0.5))
    assert got[0, 10] == first and got[1, 10] == first
    assert got[1, 200] == np.float32(np.float32(x + np.float32(0.5)) + np.float32(2.0))


@pytest.mark.parametrize("items,R", [(1, 1), (1, 5), (4, 4), (1, 17)])
def test_row_counts_positions_and_the_untouched_row(fan, ab, items, R):
    """1 / 5 / 16 / 17 rows; parents are other rows of the same item; the first generated position (the root whatever the parent says),
    positions 446 and 447; a row that defines no_speech_prob keeps its logits and stores its state"""
    t, (a, _) = fan, ab
    rows = items * R
    rng = np.random.default_rng(rows)
    sel = [(0, 1, -1, 0)[i % 4] for i in range(items)]
    plen = [4] * items
    item_pos = [(3, 447, 100, 446)[(i + rows) % 4] for i in range(items)]
    pos = [item_pos[r // R] for r in range(rows)]
    parent = [(r // R) * R + (r % R + 1) % R for r in range(rows)]
    nodes = [[0, t.n([10]), t.n([11]), t.n([12]), t.n([13])], [0, a.n([7]), a.n([7, 7]), a.n([21]), a.n([21, 22])]]
    prev = [nodes[max(sel[r // R], 0)][(parent[r] + pos[r]) % 5] for r in range(rows)]
    tokens = [int(rng.choice([10, 11, 12, 13, 200, 300, 463, 544, 7, 9, 22, 30, 5, 570])) for _ in range(rows)]
    nsp = [1 if r == 0 else 0 for r in range(rows)]
    lg = _logits(rows, 10 + rows)
    got, gs = both([t, a], sel, R, lg, tokens, pos, parent, plen, nsp, prev)
    assert np.array_equal(got[0], lg[0])
    for r in range(rows):
        if pos[r] == 3:
            assert gs[r] == 0


def test_positions_446_447_and_the_first_generated_one(fan):
    t = fan
    node = t.n([10])
    lg = _logits(3, 6)
    got, gs = both([t], [0, 0, 0], 1, lg, [200, 200, 200], [446, 447, 2], [0, 1, 2], [3, 3, 3], [0, 0, 0], [node] * 3)
    assert gs.tolist() == [t.n([10, 200]), t.n([10, 200]), 0]


def test_a_stale_parent_state_past_the_selected_table_is_the_root(fan, ab):
    """the parent's state was left by the large table; the item now selects the small one: the state is read as the root"""
    t, (_, b) = fan, ab
    stale = t.closed.n_nodes - 1
    assert stale >= b.closed.n_nodes
    got, gs = both([t, b], [1, 1], 1, _logits(2, 7), [8, 7], [5, 5], [0, 1], [1, 1], [0, 0], [stale, stale])
    assert gs.tolist() == [0, b.n([7])]


def test_refusals(fan, ab):
    t, (a, b) = fan, ab
    lg = _logits(1, 8)
    args = ([0], 1, lg, [1], [4], [0], [1], [0], [0])
    with pytest.raises(_lib.WlxError) as ei:                                  # a table index past the set
        apply_gpu([a.compact], [1], *args[1:])
    assert ei.value.code == _lib.ERR_ARG
    packed = list(B.BiasSet([a.compact]).packed())
    flagged = int(np.flatnonzero(packed[3] & _lib.BIAS_EDGE_SHARED)[0])
    bad = [x.copy() for x in packed]
    bad[3][flagged] &= ~_lib.BIAS_EDGE_SHARED                                 # the flag taken off an edge the root's list names too
    with pytest.raises(_lib.WlxError) as ei:
        apply_gpu(None, *args, packed=bad)
    assert ei.value.code == _lib.ERR_ARG and "flag" in str(ei.value)
    bad = [x.copy() for x in packed]
    bad[3][0] = a.compact.n_nodes                                             # a next node past the table
    with pytest.raises(_lib.WlxError) as ei:
        apply_gpu(None, *args, packed=bad)
    assert ei.value.code == _lib.ERR_ARG and "node" in str(ei.value)
    with pytest.raises(_lib.WlxError) as ei:                                  # position 448
        apply_gpu([a.compact], [0], 1, lg, [1], [448], [0], [1], [0], [0])
    assert ei.value.code == _lib.ERR_ARG
