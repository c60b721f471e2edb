"""GPU (-m gpu): ONE launch of dec_grammar_items_kernel (csrc/dec_grammar.hip) through wlx_debug_grammar_apply_items against
tests/grammar_ref.py applied item by item with that item's table: the uint32 view of the logits (guard words and pad columns included)
and the states, bit for bit (no arithmetic, so no tolerance). One pool serves every case: the seven-state fan of
tests/test_gpu_grammar_kernel.py; a two-state table whose start state has an edge on either side of every 2048-id tile edge (a parent
state valid for the fan is out of range here); a one-state table. Items select them in a cycle that names a table twice and leaves
items without one; the rows are the fan's walk cases (prompt positions, transparent tokens, states out of range, an nsp_row row)."""
import ctypes as C

import numpy as np
import pytest

from tests import grammar_ref as GR
from tests.test_gpu_grammar_kernel import PLEN, POS, SHAPES, _i32, _p, cases, fan, logits_for
from whisperlive_amd import _lib
from whisperlive_amd.grammar import Grammar

pytestmark = pytest.mark.gpu
SEL = [0, 1, -1, 2, 1, 0, -1]                   # the table of item b is SEL[b % 7]


def table(vocab, eot, lists, nexts, accept):
    off = np.concatenate([[0], np.cumsum([len(t) for t in lists])])
    return Grammar(vocab=vocab, eot=eot, edge_off=_i32(off), edge_tok=_i32(np.concatenate(lists)), edge_next=_i32(np.concatenate(nexts)), accept=_i32(accept))


def pool(vocab, eot):
    """the fan; state 0 with the first and the last text id and both neighbours of every tile edge, state 1 with four tokens; one state"""
    t0 = sorted({0, eot - 1} | {t for k in range(1, eot // 2048 + 1) for t in (k * 2048 - 1, k * 2048) if t < eot})
    return [fan(vocab, eot), table(vocab, eot, [t0, [5, 6, 7, 8]], [np.arange(len(t0)) % 2, [0] * 4], [1, 0]), table(vocab, eot, [[3]], [[0]], [1])]


def call(tables, vocab, eot, flat, items, R, sel, ldl, tokens, pos, parent, plen, nsp, prev_state, state, n_tables=None, null=None):
    """the hook on a flat logits buffer of items * R * ldl + GUARD words (changed in place) -> the status"""
    cat = lambda name: _i32(np.concatenate([getattr(t, name) for t in tables]))
    a = dict(ns=_i32([t.n_states for t in tables]), off=cat("edge_off"), tok=cat("edge_tok"), nxt=cat("edge_next"), acc=cat("accept"), sel=_i32(sel),
             tokens=_i32(tokens), pos=_i32(pos), parent=_i32(parent), plen=_i32(plen), nsp=_i32(nsp))
    a[null] = None
    p = lambda k: _p(a[k], C.c_int32)
    return _lib.load().wlx_debug_grammar_apply_items(
        0, vocab, eot, len(tables) if n_tables is None else n_tables, p("ns"), p("off"), p("tok"), p("nxt"), p("acc"), _p(flat, C.c_float), items, R,
        p("sel"), ldl, p("tokens"), p("pos"), p("parent"), p("plen"), p("nsp"), _p(np.ascontiguousarray(prev_state, dtype=np.int16), C.c_int16),
        _p(state, C.c_int16))


@pytest.mark.parametrize("items,R", [(1, 1), (2, 5), (20, 16), (64, 5)])
@pytest.mark.parametrize("vocab,ldl,eot", SHAPES)
def test_the_launch_equals_the_reference_item_by_item(gpu, vocab, ldl, eot, items, R):
    tables = pool(vocab, eot)
    cs, rows = cases(tables[0]), items * R
    pick = [cs[r % len(cs)] for r in range(rows)]
    prev, tokens, pos, nsp = ([c[k] for c in pick] for k in range(4))
    parent = list(range(rows))                  # rows of a run of equal parent states inside an item name the first row of the run
    for r in range(1, rows):
        if prev[r] == prev[r - 1] and pos[r] == pos[r - 1] and r % R:
            parent[r] = parent[r - 1]
    sel = [SEL[b % len(SEL)] for b in range(items)]
    plen = [POS + 1 if b % 5 == 3 else PLEN for b in range(items)]     # (some items still inside their prompt: the start state everywhere)
    src = logits_for(vocab, ldl, rows)
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    _lib.check(call(tables, vocab, eot, flat, items, R, sel, ldl, tokens, pos, parent, plen, nsp, prev, state))
    ref, want = src.copy(), np.zeros(rows, np.int16)               # (an item without a table: its bits stay, its states are 0)
    ref2 = ref[:rows * ldl].reshape(rows, ldl)
    for b in range(items):
        if sel[b] >= 0:
            q = slice(b * R, (b + 1) * R)
            ref2[q], want[q] = GR.apply(tables[sel[b]], ref2[q], tokens[q], pos[q], parent[q], plen[b], nsp[q], prev[q])
    assert state.tolist() == want.tolist() and want[:min(R, 15)].tolist() == [c[4] for c in cs[:R]]     # item 0 is under the fan: its own walk cases
    bad = np.nonzero(flat.view(np.uint32) != ref.view(np.uint32))[0]                               # guard words and pad columns included
    assert bad.size == 0, ([divmod(int(i), ldl) for i in bad[:8]], [hex(int(flat.view(np.uint32)[i])) for i in bad[:8]])
    changed = (flat.view(np.uint32) != src.view(np.uint32))[:rows * ldl].reshape(rows, ldl)
    assert not changed[:, eot + 1:].any() and changed.any(axis=1).tolist() == [sel[r // R] >= 0 and nsp[r] <= 0 for r in range(rows)]


def test_every_refusal_comes_before_any_launch(gpu):
    vocab, ldl, eot, items, R, rows = 20000, 20000, 19000, 2, 2, 4
    tables, src = pool(vocab, eot), logits_for(20000, 20000, 4)
    ok = dict(sel=[0, 1], tokens=[6, 7, 8, 5], pos=[POS] * rows, parent=[0, 1, 2, 3], plen=[PLEN] * items, nsp=[0] * rows, prev_state=[0] * rows)
    loops = lambda n_states, n_edges: table(vocab, eot, [np.arange(n_edges)] + [[]] * (n_states - 1), [np.zeros(n_edges)], [0] * n_states)
    bad = pool(vocab, eot)[1]
    bad.edge_next[0] = 2                                                                           # a state only the fan has
    cases_ = [dict(ts=[tables[2]] * 65), dict(n_tables=0), dict(ts=[loops(4000, 1)] * 5), dict(ts=[loops(1, 16000)] * 5),   # each table within its own limits
              dict(sel=[0, 3]), dict(sel=[-2, 0]), dict(ts=[tables[0], bad, tables[2]]), dict(items=65),
              dict(pos=[POS, POS + 1, POS, POS], parent=[0, 0, 2, 3])]                              # a row that reads the state another row writes
    cases_ += [dict(null=name) for name in ("ns", "off", "tok", "nxt", "acc", "sel", "tokens", "pos", "parent", "plen", "nsp")]
    for kw in cases_ + [{}]:
        flat, state = src.copy(), np.full(rows, -1, np.int16)
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        rc = call(kw.get("ts", tables), vocab, eot, flat, kw.get("items", items), R, a["sel"], ldl, a["tokens"], a["pos"], a["parent"], a["plen"], a["nsp"],
                  a["prev_state"], state, n_tables=kw.get("n_tables"), null=kw.get("null"))
        if kw:
            assert rc == _lib.ERR_ARG and np.array_equal(flat.view(np.uint32), src.view(np.uint32)) and np.all(state == -1), kw.keys()
    assert rc == 0 and state.tolist() == [3, 4, 0, 0]                                               # the same arguments unchanged are served
