"""GPU (-m gpu): ONE launch of dec_pattern_kernel (csrc/dec_pattern.hip) through wlx_debug_pattern_apply against a plain Python loop over
bytes: the uint32 view of the logits (guard words and pad columns included) and the states, bit for bit. The kernel does no arithmetic,
so there is no tolerance: a word is what it was, or 0xff800000.

Semantics per row (the kernel's header comment). State at position p: the start state while the fed token is a prompt token (p < plen or
p < 1); the parent's state at p - 1 where the fed token is >= eot; otherwise the walk of the token's bytes from the parent's state; the
start state where that walk dies or the token has no bytes. A parent's state outside 0 .. n_states - 1 reads as the start state. A row
with nsp_row > 0 writes its state and keeps its logits raw. Otherwise a text token t < eot keeps its logit iff it has at least one byte
and its walk from the row's state does not die; eot keeps its logit iff the state accepts; ids above eot and the pad columns keep
their bits.

Shapes: 51865 / 51872 (16-byte pieces, 26 tiles) and 1003 / 1003 (the one-word path); end-of-text as the last id and well inside; 1, 5
and 320 rows. The seeded vocabulary has tokens of 0, 1, 2, 3, 4, 5, 8, 15, 16, 17 and 255 bytes around the ids 0, 2047, 2048 and
eot - 1, and a tile whose bytes exceed one 16 KiB staging piece, with a token planted across the piece's end that must survive."""
import ctypes as C

import numpy as np
import pytest

from whisperlive_amd import _lib

pytestmark = pytest.mark.gpu

GUARD, DEAD, NEG_INF = _lib.DEBUG_GUARD, 0xFFFF, 0xff800000
PLEN, POS, PIECE = 3, 7, 16384
LENGTHS = [0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 255]
NOTHING_ACC, NOTHING_REJ = 5, 6                 # states of the "cap" table that allow nothing: one accepts, one does not


class Table:
    def __init__(self, kind):
        if kind == "one":                       # 1 state x 1 class: every byte loops, the state accepts
            self.cls, self.trans, self.accept = np.zeros(256, np.uint8), np.zeros((1, 1), np.uint16), np.ones(1, np.uint8)
            return
        n = 4096                                # x 6 classes = 24576 cells, the cap: a b c d e, everything else
        self.cls = np.full(256, 5, np.uint8)
        self.cls[[97, 98, 99, 100, 101]] = [0, 1, 2, 3, 4]
        s = np.arange(n)
        self.trans = np.full((n, 6), DEAD, np.uint16)
        self.trans[:, 0] = (s * 7 + 1) % n
        self.trans[:, 1] = s
        self.trans[::2, 2] = (s[::2] + 3) % n
        self.trans[:, 4] = 0
        self.trans[[NOTHING_ACC, NOTHING_REJ]] = DEAD
        self.accept = (s % 3 == 0).astype(np.uint8)
        self.accept[[NOTHING_ACC, NOTHING_REJ]] = [1, 0]

    n_states = property(lambda self: self.trans.shape[0])
    n_classes = property(lambda self: self.trans.shape[1])


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def vocabulary(eot):
    """(tok_off, bytes): seeded; bytes mostly from `abcde`; LENGTHS around the ids 0, 2047, 2048 and eot - 1; planted tokens 1 = `a`,
    3 = `abb` (survives wherever `a` does), 5 = `bbbbd` (dies on its last byte); long tokens in the tile of id 2048 (or in tile 0 of a
    small vocabulary), and the token across the first piece's end all `b` (survives from every state that allows anything)"""
    rng = np.random.default_rng(eot)
    n = rng.choice([1, 2, 3, 4, 5, 8], eot, p=[.1, .2, .25, .2, .15, .1])
    lo = 2048 if eot > 4096 else 0
    n[lo:lo + 2048] = rng.integers(8, 40, min(2048, eot - lo))
    for first, lengths in ((0, LENGTHS), (2037, LENGTHS), (2048, LENGTHS[-2::-1] + [255]), (eot - 9, LENGTHS)):   # 0 / 255 / 17 / 16 bytes at the four ids
        for k, ln in enumerate(lengths):
            i = first + k
            if 0 <= i < eot:
                n[i] = ln
    while True:                                 # (one byte more in a token in front of it until the piece's end falls INSIDE a token)
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        if (int(off[lo]) & ~15) + PIECE not in off:
            break
        n[lo + 20] += 1
    by = rng.choice(np.frombuffer(b"abcdez", np.uint8), int(off[-1]), p=[.35, .35, .1, .1, .05, .05])
    for t, text in ((1, b"a"), (3, b"abb"), (5, b"bbbbd")):
        by[off[t]:off[t + 1]] = np.frombuffer(text, np.uint8)
    cut = (int(off[lo]) & ~15) + PIECE          # the first byte of the tile's second staging piece
    t = int(np.searchsorted(off, cut, side="right")) - 1
    assert off[lo + min(2048, eot - lo)] > cut and off[t] < cut < off[t + 1], "a token straddles the staging piece"
    by[off[t]:off[t + 1]] = 98
    return off, by, t


def walk(tb, state, data):
    if not hasattr(tb, "rows"):
        tb.rows, tb.classes = tb.trans.tolist(), tb.cls.tolist()       # (plain lists: the loop below runs over every byte of a vocabulary)
    for b in data:
        state = tb.rows[state][tb.classes[b]]
        if state == DEAD:
            return -1
    return state


def next_state(tb, off, by, eot, ps, tok, p):
    if p < PLEN or p < 1:
        return 0
    if not 0 <= ps < tb.n_states:
        ps = 0
    if tok >= eot:
        return ps
    data = by[off[tok]:off[tok + 1]]
    return max(walk(tb, ps, data.tolist()), 0) if len(data) else 0


def keep_mask(tb, off, by, eot, ldl, state):
    """bool [ldl]: the words of a row in `state` that keep their bits"""
    keep = np.ones(ldl, bool)
    data, at = by.tolist(), off.tolist()
    for t in range(eot):
        keep[t] = at[t + 1] > at[t] and walk(tb, state, data[at[t]:at[t + 1]]) >= 0
    keep[eot] = bool(tb.accept[state])
    return keep


def rows_for(tb, eot, vocab, rows):
    """(parent's state, fed token, position, nsp_row) per row"""
    cs = [(0, 3, POS, 0), (3, 3, PLEN - 1, 0),                  # a walk that lives; a prompt position
          (4, eot, POS, 0), (NOTHING_ACC, min(vocab - 1, eot + 3), POS, 0),     # end-of-text and a timestamp: the parent's state
          (NOTHING_REJ, eot, POS, 0), (2, 5, POS, 0), (2, 0, POS, 0),           # nothing survives; a walk that dies; an empty token
          (tb.n_states, 3, POS, 0), (32767, eot, POS, 0),       # a parent's state another mode left behind
          (0, 3, POS, 1), (tb.n_states - 1, eot, POS, 0), (9, 1, POS, 0)]       # nsp_row; the table's last state; one byte
    return [cs[r % len(cs)] for r in range(rows)]


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def call(tb, off, by, flat, rows, ldl, vocab, eot, tokens, pos, parent, plen, nsp, prev, state, n_states=None, n_classes=None, nulls=()):
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    a = dict(cls=np.ascontiguousarray(tb.cls), trans=np.ascontiguousarray(tb.trans), acc=np.ascontiguousarray(tb.accept), off=i32(off),
             by=np.ascontiguousarray(by, dtype=np.uint8), tokens=i32(tokens), pos=i32(pos), parent=i32(parent), nsp=i32(nsp))
    a.update({k: None for k in nulls})
    prev = np.ascontiguousarray(prev, dtype=np.int16)
    return _lib.load().wlx_debug_pattern_apply(
        0, vocab, eot, tb.n_states if n_states is None else n_states, tb.n_classes if n_classes is None else n_classes, _p(a["cls"], C.c_uint8),
        _p(a["trans"], C.c_uint16), _p(a["acc"], C.c_uint8), _p(a["off"], C.c_int32), _p(a["by"], C.c_uint8), _p(flat, C.c_float), rows, ldl,
        _p(a["tokens"], C.c_int32), _p(a["pos"], C.c_int32), _p(a["parent"], C.c_int32), plen, _p(a["nsp"], C.c_int32), _p(prev, C.c_int16),
        _p(state, C.c_int16))


def logits_for(ldl, rows):
    """seeded rows with words whose bits a float operation would not keep (-0.0, a NaN payload, +inf, a denormal)"""
    rng = np.random.default_rng(ldl + rows)
    flat = rng.standard_normal(rows * ldl + GUARD, dtype=np.float32) * np.float32(3.0)
    u = flat.view(np.uint32)
    u[0::997], u[1::1499], u[2::2503], u[3::3001] = 0x80000000, 0x7fc12345, 0x7f800000, 0x00000001
    u[rows * ldl:] = 0xdeadbeef
    return flat


@pytest.mark.parametrize("kind", ["one", "cap"])
@pytest.mark.parametrize("rows", [1, 5, 320])
@pytest.mark.parametrize("vocab,ldl,eot", [(51865, 51872, 51864), (51865, 51872, 50257), (1003, 1003, 1002), (1003, 1003, 900)])
def test_the_launch_equals_the_byte_loop_bit_for_bit(gpu, vocab, ldl, eot, rows, kind):
    tb = cached(kind, lambda: Table(kind))
    off, by, straddler = cached(eot, lambda: vocabulary(eot))
    pick = rows_for(tb, eot, vocab, rows)
    prev, tokens, pos, nsp = ([c[k] for c in pick] for k in range(4))
    parent = [(r + 1) % rows for r in range(rows)]              # every row reads ANOTHER row's state through the ancestry
    src = cached(("logits", ldl, rows), lambda: logits_for(ldl, rows))
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    _lib.check(call(tb, off, by, flat, rows, ldl, vocab, eot, tokens, pos, parent, PLEN, nsp, prev, state))
    want = [next_state(tb, off, by, eot, *c[:3]) for c in pick]
    assert state.tolist() == want
    got, ref = flat.view(np.uint32), src.view(np.uint32).copy()
    for r, s in enumerate(want):
        if not nsp[r]:
            keep = cached(("keep", kind, eot, ldl, s), lambda: keep_mask(tb, off, by, eot, ldl, s))
            ref[r * ldl:(r + 1) * ldl][~keep] = NEG_INF
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(int(i) // ldl, int(i) % ldl, hex(int(got[i]))) for i in bad[:8]]
    # what the case is for: the token across the piece's end lives wherever anything does; only end-of-text after NOTHING_ACC
    live = cached(("keep", kind, eot, ldl, want[0]), lambda: None)
    assert live[straddler] and live[3] and not live[0] and (kind == "one" or not live[5])
    if kind == "cap" and rows >= 5:
        assert want[3] == NOTHING_ACC and np.all(got[3 * ldl:3 * ldl + eot] == NEG_INF) and got[3 * ldl + eot] == ref[3 * ldl + eot]
        assert want[4] == NOTHING_REJ and np.all(got[4 * ldl:4 * ldl + eot + 1] == NEG_INF)


REFUSALS = {
    "no state": dict(n_states=0), "4097 states": dict(n_states=4097), "no class": dict(n_classes=0), "257 classes": dict(n_classes=257),
    "24577 cells": dict(n_states=3073, n_classes=8), "a class past the last": dict(edit=("cls", 7, 6)),
    "a transition past the last state": dict(edit=("trans", (1, 1), 4096)), "accept 2": dict(edit=("accept", 1, 2)),
    "end-of-text outside the vocabulary": dict(eot=1008), "offsets that do not start at 0": dict(edit=("off", 0, 1)),
    "offsets that descend": dict(edit=("off", 4, 0)), "a token of 256 bytes": dict(edit=("off", slice(7, None), 256)),
    "more than 2^22 vocabulary bytes": dict(vocab=51865, ldl=51872, eot=51864, off_all=255),
    **{f"null {k}": dict(nulls=(k,)) for k in ("cls", "trans", "acc", "off", "by", "tokens", "pos", "parent", "nsp")},
    "no rows": dict(rows=0), "321 rows": dict(rows=321), "ldl below the vocabulary": dict(ldl=1002), "plen 0": dict(plen=0),
    "a position out of range": dict(pos=[POS, 448, POS, POS]), "a parent out of range": dict(parent=[0, 4, 2, 3]),
    "a fed token outside the vocabulary": dict(tokens=[3, 1003, 3, 3]), "a negative parent state": dict(prev=[0, -1, 0, 0]),
    "a row that reads the state another row writes": dict(pos=[POS, POS + 1, POS, POS], parent=[0, 0, 2, 3]),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_every_refusal_comes_before_any_launch(gpu, what):
    vocab, ldl, eot, rows = 1003, 1008, 1002, 4
    kw = dict(REFUSALS[what])
    tb, (off, by, _t) = Table("cap"), vocabulary(eot)
    off = off.copy()
    if "edit" in kw:
        name, at, value = kw.pop("edit")
        arr = off if name == "off" else getattr(tb, name)
        arr[at] = value if name != "off" or isinstance(at, int) else arr[at] - arr[at][0] + off[at.start - 1] + value
    if "off_all" in kw:
        off = (np.arange(kw["eot"] + 1) * kw.pop("off_all")).astype(np.int32)
    vocab = kw.pop("vocab", vocab)
    src = logits_for(kw.get("ldl", ldl), rows)
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    a = dict(rows=rows, ldl=ldl, eot=eot, tokens=[3] * rows, pos=[POS] * rows, parent=[0, 1, 2, 3], plen=PLEN, nsp=[0] * rows, prev=[0] * rows)
    extra = {k: kw.pop(k) for k in ("n_states", "n_classes", "nulls") if k in kw}
    a.update(kw)
    rc = call(tb, off, by, flat, a["rows"], a["ldl"], vocab, a["eot"], a["tokens"], a["pos"], a["parent"], a["plen"], a["nsp"], a["prev"], state, **extra)
    assert rc == _lib.ERR_ARG, (what, rc)
    assert np.array_equal(flat.view(np.uint32), src.view(np.uint32)) and np.all(state == -1), what
