"""GPU (-m gpu): ONE launch of dec_grammar_kernel (csrc/dec_grammar.hip) through wlx_debug_grammar_apply against the NumPy restatement
tests/grammar_ref.py: the uint32 view of the logits (guard words and pad columns included) and the states, bit for bit. The kernel does
no arithmetic, so there is no tolerance: a word is what it was, or 0xff800000.

Shapes: the multilingual vocabulary with the engine's row stride (51865 / 51872: 16-byte pieces, 26 tiles of 2048 ids, a ragged last
one) and 1003 / 1003 (rows that are not 16-byte aligned: the one-word path); end-of-text as the last id and well inside; 1, 5 and 320
rows; states with 0, 1, 64, 65 and 300 edges whose tokens run from 0 to eot - 1 across every tile."""
import ctypes as C

import numpy as np
import pytest

from tests import grammar_ref as GR
from whisperlive_amd import _lib
from whisperlive_amd.grammar import Grammar

pytestmark = pytest.mark.gpu

GUARD = _lib.DEBUG_GUARD
PLEN, POS = 3, 7


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def call(g, flat, rows, ldl, tokens, pos, parent, plen, nsp, prev_state, state, vocab=None, eot=None, n_states=None, nulls=()):
    """the hook on a flat logits buffer of rows * ldl + GUARD words (changed in place) -> the status"""
    lib = _lib.load()
    a = dict(off=_i32(g.edge_off), tok=_i32(g.edge_tok), nxt=_i32(g.edge_next), acc=_i32(g.accept), tokens=_i32(tokens), pos=_i32(pos),
             parent=_i32(parent), nsp=_i32(nsp))
    prev = np.ascontiguousarray(prev_state, dtype=np.int16)
    for k in nulls:
        a[k] = None
    return lib.wlx_debug_grammar_apply(0, g.vocab if vocab is None else vocab, g.eot if eot is None else eot,
                                       g.n_states if n_states is None else n_states, _p(a["off"], C.c_int32), _p(a["tok"], C.c_int32),
                                       _p(a["nxt"], C.c_int32), _p(a["acc"], C.c_int32), _p(flat, C.c_float), rows, ldl,
                                       _p(a["tokens"], C.c_int32), _p(a["pos"], C.c_int32), _p(a["parent"], C.c_int32), plen,
                                       _p(a["nsp"], C.c_int32), _p(prev, C.c_int16), _p(state, C.c_int16))


def fan(vocab, eot):
    """state 0: the start state, six edges (tokens 0 and eot - 1 among them) into states 1 .. 6 with 0, 1, 64, 65, 300 and 0 edges; the
    tokens of a state run evenly from 0 to eot - 1, so every tile of the row holds some and the first and the last text id are edges"""
    def spread(k):
        return np.unique(np.linspace(0, eot - 1, k).astype(np.int64)).astype(np.int32)
    lists = [np.array([0, 5, 6, 7, 8, eot - 1], np.int32), spread(0), np.array([eot - 1], np.int32), spread(64), spread(65), spread(300), spread(0)]
    nexts = [np.array([1, 2, 3, 4, 5, 6], np.int32)] + [(np.arange(len(t)) % 7).astype(np.int32) for t in lists[1:]]
    assert [len(t) for t in lists] == [6, 0, 1, 64, 65, 300, 0]
    off = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    return Grammar(vocab=vocab, eot=eot, edge_off=off, edge_tok=np.concatenate(lists).astype(np.int32),
                   edge_next=np.concatenate(nexts).astype(np.int32), accept=np.array([1, 1, 0, 0, 1, 0, 0], np.int32))


def cases(g):
    """(parent's state, fed token, position, nsp_row) per row, and the state each must reach"""
    eot, special = g.eot, min(g.vocab - 1, g.eot + 3)
    rows = [(0, 6, POS, 0, 3),                  # 64 edges, not accepting
            (0, 7, POS, 0, 4),                  # 65 edges, accepting
            (0, 8, POS, 0, 5),                  # 300 edges
            (0, 0, POS, 0, 1),                  # token 0 is an edge; the new state has NO edge and accepts: only end-of-text survives
            (0, eot - 1, POS, 0, 6),            # token eot - 1 is an edge; no edge and not accepting: nothing of [0, eot] survives
            (0, 5, POS, 0, 2),                  # one edge (eot - 1), end-of-text masked
            (3, 5, PLEN - 1, 0, 0),             # a prompt position: the start state whatever the parent held
            (4, eot, POS, 0, 4),                # end-of-text fed: the parent's state
            (5, special, POS, 0, 5),            # a special / timestamp fed: the parent's state
            (2, 9, POS, 0, 0),                  # a text token the parent's state has no edge for: the start state
            (4000, 6, POS, 0, 3),               # a parent state out of range counts as the start state
            (32767, eot + 0, POS, 0, 0),        # ... also where the token is transparent
            (0, 8, POS, 1, 5),                  # nsp_row: the bits stay, the state is written
            (5, int(g.edges(5)[0][299]), POS, 0, 299 % 7),    # the last of 300 edges (the second stride of the walk)
            (4, int(g.edges(4)[0][64]), POS, 0, 64 % 7)]
    return rows


SHAPES = [(51865, 51872, 51864), (51865, 51872, 50257), (1003, 1003, 1002), (1003, 1003, 900)]
_INPUT = {}


def logits_for(vocab, ldl, rows):
    """seeded rows with a few words whose bits a float operation would not keep (-0.0, a NaN payload, +inf, a denormal), shared by the cases of a shape"""
    key = (ldl, rows)
    if key not in _INPUT:
        rng = np.random.default_rng(ldl + rows)
        flat = (rng.standard_normal(rows * ldl + GUARD, dtype=np.float32) * np.float32(3.0))
        u = flat.view(np.uint32)
        u[0::997] = 0x80000000
        u[1::1499] = 0x7fc12345
        u[2::2503] = 0x7f800000
        u[3::3001] = 0x00000001
        u[rows * ldl:] = 0xdeadbeef
        _INPUT[key] = flat
    return _INPUT[key]


def run_case(vocab, ldl, eot, rows):
    g = fan(vocab, eot)
    cs = cases(g)
    pick = [cs[r % len(cs)] for r in range(rows)]
    prev = [c[0] for c in pick]
    tokens, pos, nsp, want = [c[1] for c in pick], [c[2] for c in pick], [c[3] for c in pick], [c[4] for c in pick]
    # rows that share a parent: every row of a run of equal parent states names the first row of the run (the hook keeps one state per parent)
    parent = list(range(rows))
    for r in range(1, rows):
        if prev[r] == prev[r - 1] and pos[r] == pos[r - 1]:
            parent[r] = parent[r - 1]
    src = logits_for(vocab, ldl, rows)
    flat = src.copy()
    state = np.full(rows, -1, np.int16)
    _lib.check(call(g, flat, rows, ldl, tokens, pos, parent, PLEN, nsp, prev, state))
    ref, rs = GR.apply(g, src[:rows * ldl].reshape(rows, ldl), tokens, pos, parent, PLEN, nsp, prev)
    assert rs.tolist() == want[:rows] and state.tolist() == rs.tolist()
    got = flat.view(np.uint32)
    assert np.array_equal(got[rows * ldl:], src.view(np.uint32)[rows * ldl:])                   # the guard words
    got2, ref2, in2 = got[:rows * ldl].reshape(rows, ldl), ref.view(np.uint32), src.view(np.uint32)[:rows * ldl].reshape(rows, ldl)
    bad = np.argwhere(got2 != ref2)
    assert bad.size == 0, (bad[:8].tolist(), [hex(int(got2[tuple(b)])) for b in bad[:8]])
    assert np.array_equal(got2[:, eot + 1:], in2[:, eot + 1:])                                  # ids above end-of-text and the pad columns
    return g, pick, got2, in2


@pytest.mark.parametrize("rows", [1, 5, 320])
@pytest.mark.parametrize("vocab,ldl,eot", SHAPES)
def test_the_launch_equals_the_reference_bit_for_bit(gpu, vocab, ldl, eot, rows):
    g, pick, got, src = run_case(vocab, ldl, eot, rows)
    for r, (_ps, _tok, _pos, nsp, want) in enumerate(pick[:15]):
        if nsp:
            assert np.array_equal(got[r], src[r])                                               # the row that defines no_speech_prob
            continue
        kept = np.nonzero(got[r, :eot + 1] != GR.NEG_INF)[0]
        allowed = set(g.edges(want)[0].tolist()) | ({eot} if g.accept[want] else set())
        # (an input word may be -inf by itself only where the seeded row says so: none is)
        assert set(kept.tolist()) == allowed, (r, want, sorted(set(kept.tolist()) ^ allowed)[:8])
        assert np.array_equal(got[r, kept], src[r, kept])


def test_every_refusal_comes_before_any_launch(gpu):
    vocab, ldl, eot, rows = 1003, 1008, 900, 4
    g = fan(vocab, eot)
    src = logits_for(vocab, ldl, rows)
    ok = dict(tokens=[6, 7, 8, 5], pos=[POS] * rows, parent=[0, 1, 2, 3], plen=PLEN, nsp=[0] * rows, prev_state=[0] * rows)

    def refused(what, table=None, **kw):
        t = table if table is not None else g
        flat, state = src.copy(), np.full(rows, -1, np.int16)
        extra = {k: kw.pop(k) for k in ("vocab", "eot", "n_states", "nulls", "rows", "ldl") if k in kw}
        a = dict(ok, **kw)
        rc = call(t, flat, extra.pop("rows", rows), extra.pop("ldl", ldl), a["tokens"], a["pos"], a["parent"], a["plen"], a["nsp"], a["prev_state"],
                  state, **extra)
        assert rc == _lib.ERR_ARG, (what, rc)
        assert np.array_equal(flat.view(np.uint32), src.view(np.uint32)) and np.all(state == -1), what

    def changed(**kw):
        t = fan(vocab, eot)
        for k, (i, v) in kw.items():
            arr = getattr(t, k).copy()
            arr[i] = v
            setattr(t, k, arr)
        return t

    refused("an edge token that is end-of-text", changed(edge_tok=(5, eot)))
    refused("an edge token that is a special", changed(edge_tok=(5, eot + 5)))
    refused("an edge token outside the vocabulary", changed(edge_tok=(5, vocab)))
    refused("a negative edge token", changed(edge_tok=(0, -1)))
    refused("edge tokens that do not ascend", changed(edge_tok=(2, 5)))
    refused("a next state past the last", changed(edge_next=(3, 7)))
    refused("a negative next state", changed(edge_next=(3, -1)))
    refused("accept 2", changed(accept=(1, 2)))
    refused("accept -1", changed(accept=(0, -1)))
    refused("offsets that do not start at 0", changed(edge_off=(0, 1)))
    refused("offsets that descend", changed(edge_off=(3, 2)))
    refused("more than 16384 edges", changed(edge_off=(7, 16385)))
    refused("no state", n_states=0)
    refused("4097 states", n_states=4097)
    refused("end-of-text outside the vocabulary", eot=vocab)
    refused("end-of-text below an edge token", eot=800)
    for name in ("off", "acc", "tok", "nxt", "tokens", "pos", "parent", "nsp"):
        refused(f"null {name}", nulls=(name,))
    refused("no rows", rows=0)
    refused("321 rows", rows=321)
    refused("ldl below the vocabulary", ldl=vocab - 1)
    refused("plen 0", plen=0)
    refused("plen 449", plen=449)
    refused("a position out of range", pos=[POS, 448, POS, POS])
    refused("a negative position", pos=[POS, -1, POS, POS])
    refused("a parent out of range", parent=[0, 4, 2, 3])
    refused("a fed token outside the vocabulary", tokens=[6, vocab, 8, 5])
    refused("a negative parent state", prev_state=[0, -1, 0, 0])
    refused("a row that reads the state another row writes in this launch", pos=[POS, POS + 1, POS, POS], parent=[0, 0, 2, 3])
    # and the same arguments unchanged are served
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    _lib.check(call(g, flat, rows, ldl, ok["tokens"], ok["pos"], ok["parent"], PLEN, ok["nsp"], ok["prev_state"], state))
    assert state.tolist() == [3, 4, 5, 2]
