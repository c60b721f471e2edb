"""GPU (-m gpu): ONE launch of dec_pattern_items_kernel (csrc/dec_pattern.hip) through wlx_debug_pattern_apply_items against the Python
loop over bytes of tests/test_gpu_pattern_kernel.py applied item by item with that item's table: the uint32 view of the logits (guard
words and pad columns included) and the states, bit for bit (no arithmetic, so no tolerance).

The pool, in this order: the 1 x 1 table (behind it the next table's cells would start misaligned if the packer did not pad), a 37 x 3
table, the table at exactly 24576 cells (which therefore does not start at offset 0). Every item takes its rows out of rows_for's cases
from another start, `parent` a rotation inside the item; among them an nsp_row row between masked rows: a skipped row INSIDE the row
loop of a workgroup. An item without a table keeps its bits and has its states written as 0."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_pattern_kernel import DEAD, NEG_INF, PLEN, Table, _p, cached, keep_mask, logits_for, next_state, rows_for, vocabulary
from whisperlive_amd import _lib

pytestmark = pytest.mark.gpu
ONE, MID, CAP = 0, 1, 2


def mid_table():
    tb = Table("one")
    n = 37
    s = np.arange(n)
    tb.cls = np.full(256, 2, np.uint8)
    tb.cls[[97, 98]] = [0, 1]
    tb.trans = np.full((n, 3), DEAD, np.uint16)
    tb.trans[:, 0], tb.trans[:, 1] = (s * 5 + 1) % n, s
    tb.accept = (s % 2).astype(np.uint8)
    return tb


def pool():
    return cached("pool", lambda: [Table("one"), mid_table(), Table("cap")])


def call(tables, off, by, flat, items, R, sel, ldl, vocab, eot, tokens, pos, parent, plen, nsp, prev, state, n_tables=None, nulls=()):
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    cat = lambda name, t: np.ascontiguousarray(np.concatenate([np.asarray(getattr(tb, name), t).ravel() for tb in tables]))
    a = dict(ns=i32([tb.trans.shape[0] for tb in tables]), nc=i32([tb.trans.shape[1] for tb in tables]), cls=cat("cls", np.uint8),
             trans=cat("trans", np.uint16), acc=cat("accept", np.uint8), off=i32(off), by=np.ascontiguousarray(by, dtype=np.uint8), sel=i32(sel),
             tokens=i32(tokens), pos=i32(pos), parent=i32(parent), plen=i32(plen), nsp=i32(nsp))
    a.update({k: None for k in nulls})
    prev = np.ascontiguousarray(prev, dtype=np.int16)
    p32 = lambda k: _p(a[k], C.c_int32)
    return _lib.load().wlx_debug_pattern_apply_items(
        0, vocab, eot, len(tables) if n_tables is None else n_tables, p32("ns"), p32("nc"), _p(a["cls"], C.c_uint8), _p(a["trans"], C.c_uint16),
        _p(a["acc"], C.c_uint8), p32("off"), _p(a["by"], C.c_uint8), _p(flat, C.c_float), items, R, p32("sel"), ldl, p32("tokens"), p32("pos"),
        p32("parent"), p32("plen"), p32("nsp"), _p(prev, C.c_int16), _p(state, C.c_int16))


SHAPES = [(1, 1, [CAP]), (1, 5, [CAP]), (3, 5, [CAP, -1, ONE]), (2, 16, [CAP, MID]), (64, 5, [ONE, MID, CAP, -1] * 16)]


@pytest.mark.parametrize("items,R,sel", SHAPES, ids=[f"{i}x{r}" for i, r, _s in SHAPES])
@pytest.mark.parametrize("vocab,ldl,eot", [(51865, 51872, 51864), (1003, 1003, 900)])
def test_the_launch_equals_the_byte_loop_item_by_item(gpu, vocab, ldl, eot, items, R, sel):
    tables, rows = pool(), items * R
    off, by, straddler = cached(eot, lambda: vocabulary(eot))
    pick = []
    for b in range(items):                      # item b: R of the twelve cases from case 9 b on (the nsp_row case is case 9)
        cs = rows_for(tables[max(sel[b], 0)], eot, vocab, 12)
        pick += [cs[(9 * b + k) % 12] for k in range(R)]
    prev, tokens, pos, nsp = ([c[k] for c in pick] for k in range(4))
    parent = [r - r % R + (r % R + 1) % R for r in range(rows)]         # a rotation within each item
    src = cached(("logits", ldl, rows), lambda: logits_for(ldl, rows))
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    _lib.check(call(tables, off, by, flat, items, R, sel, ldl, vocab, eot, tokens, pos, parent, [PLEN] * items, nsp, prev, state))
    want, ref = [0] * rows, src.view(np.uint32).copy()
    for r in range(rows):
        t = sel[r // R]
        if t < 0:
            continue                            # an item without a table: its bits stay, its states are 0
        want[r] = s = next_state(tables[t], off, by, eot, *pick[r][:3])
        if not nsp[r]:
            kind = {ONE: "one", CAP: "cap"}.get(t, "mid")      # (the masks of `one` and `cap` are those of tests/test_gpu_pattern_kernel.py)
            keep = cached(("keep", kind, eot, ldl, s), lambda: keep_mask(tables[t], off, by, eot, ldl, s))
            ref[r * ldl:(r + 1) * ldl][~keep] = NEG_INF
    assert state.tolist() == want
    got = flat.view(np.uint32)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(int(i) // ldl, int(i) % ldl, hex(int(got[i]))) for i in bad[:8]]
    # what the case is for: the token across the piece's end lives in every selected item; rows are masked exactly where they should be
    changed = (got != src.view(np.uint32))[:rows * ldl].reshape(rows, ldl)
    assert changed.any(axis=1).tolist() == [sel[r // R] >= 0 and not nsp[r] for r in range(rows)] and not changed[:, eot + 1:].any()
    for b in range(items):
        assert sel[b] < 0 or any(got[r * ldl + straddler] != NEG_INF and changed[r].any() for r in range(b * R, (b + 1) * R)), b
    if R >= 12:
        assert nsp[9] and not changed[9].any() and changed[8].any() and changed[10].any()      # the raw row between two masked rows


def shaped(n, c):
    tb = Table("one")
    tb.cls, tb.trans, tb.accept = np.zeros(256, np.uint8), np.zeros((n, c), np.uint16), np.zeros(n, np.uint8)
    return tb


def edited(name, at, value):
    tb = mid_table()
    getattr(tb, name)[at] = value
    return [Table("one"), tb, Table("one")]


REFUSALS = {
    "no table": dict(n_tables=0), "65 tables": dict(ts=lambda: [Table("one")] * 65), "a pool over the cell cap": dict(ts=lambda: [Table("cap")] * 17),
    "a table over its own cap": dict(ts=lambda: [Table("one"), shaped(3073, 8)]), "a class out of range in the second table": dict(ts=lambda: edited("cls", 7, 3)),
    "a transition out of range in the second table": dict(ts=lambda: edited("trans", (1, 1), 37)), "a selection past the last table": dict(sel=[3, 0]),
    "a selection below -1": dict(sel=[-2, 0]), "321 rows": dict(items=107, R=3), "17 rows an item": dict(items=1, R=17),
    **{f"null {k}": dict(nulls=(k,)) for k in ("ns", "nc", "cls", "trans", "acc", "off", "by", "sel", "tokens", "pos", "parent", "plen", "nsp")},
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_every_refusal_comes_before_any_launch(gpu, what):
    vocab, ldl, eot = 1003, 1008, 1002
    kw = dict(REFUSALS[what])
    items, R = kw.get("items", 2), kw.get("R", 2)
    rows = items * R
    tables = kw["ts"]() if "ts" in kw else pool()
    off, by, _t = cached(eot, lambda: vocabulary(eot))
    src = logits_for(ldl, rows)
    flat, state = src.copy(), np.full(rows, -1, np.int16)
    rc = call(tables, off, by, flat, items, R, kw.get("sel", [ONE, MID] * items)[:items], ldl, vocab, eot, [3] * rows, [7] * rows, list(range(rows)),
              [PLEN] * items, [0] * rows, [0] * rows, state, n_tables=kw.get("n_tables"), nulls=kw.get("nulls", ()))
    assert rc == _lib.ERR_ARG, (what, rc)
    assert np.array_equal(flat.view(np.uint32), src.view(np.uint32)) and np.all(state == -1), what
