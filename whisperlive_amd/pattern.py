"""Regular-expression grammars, host side: a regular expression compiled into the DFA over the BYTES of the text that the decode step
walks on the device (include/wlx_pattern.h wlx_pattern_set, csrc/dec_pattern.hip), and the byte strings of a byte-level
BPE vocabulary that it walks them over (wlx_pattern_vocab_set).

A phrase-list grammar (grammar.py) is a DFA over token ids: it admits the tokenisations its compiler enumerated and needs a state per
phrase prefix. A pattern's automaton runs over bytes, so every tokenisation of a text of the language is admitted and `\\d{8}` is nine
states. The match is a FULL match of a window's text; `leading_space=True` compiles `" ?(regex)"`, because Whisper's first text token
carries a space.

Syntax: literals (a non-ASCII character stands for its UTF-8 bytes), `.` (any byte), the escapes `\\d \\w \\s \\D \\W \\S` (ASCII sets) `\\n \\t \\r
\\xHH` and an escaped punctuation character, ASCII classes `[a-z0-9_]` with ranges and negation `[^...]` (a negated class, like `\\D \\W \\S`,
matches one ASCII byte it does not exclude or one whole non-ASCII character), grouping `(...)` and `(?:...)`, `|`, the
quantifiers `? * +`, `{m}`, `{m,}`, `{m,n}`. Refused with a ValueError that names the construct: anchors (`^ $ \\b \\B \\A \\Z`),
back-references, look-around, named groups and flags, lazy and possessive quantifiers, a non-ASCII character inside a class.

Pipeline: Thompson construction -> subset construction over the classes of bytes the expression tells apart -> minimisation -> TRIMMING
(every state that cannot reach an accepting state becomes dead, so a row that survives always has a completion) -> byte classes (bytes
with identical columns share a class). Limits: wlx_pattern.h's, named in the ValueError that reports them."""
from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import (PATTERN_DEAD, PATTERN_MAX_CELLS, PATTERN_MAX_STATES, PATTERN_MAX_TOKEN_BYTES, PATTERN_MAX_VOCAB_BYTES, PATTERN_SET_MAX_CELLS,
                   PATTERN_SET_MAX_STATES, PATTERN_SET_MAX_TABLES)

DEAD = PATTERN_DEAD
MAX_REPEAT = 1000               # the largest count of a `{m,n}`
_SUBSET_CAP = 4 * PATTERN_MAX_STATES    # states of the automaton before minimisation

_DIGIT = frozenset(range(48, 58))
_WORD = frozenset(range(48, 58)) | frozenset(range(65, 91)) | frozenset(range(97, 123)) | {95}
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_ASCII = frozenset(range(128))
_SHORT = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _ASCII - _DIGIT, "W": _ASCII - _WORD, "S": _ASCII - _SPACE}
_CTRL = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0}
_NEGATED = {"D": _DIGIT, "W": _WORD, "S": _SPACE}
_CONT = ("set", frozenset(range(0x80, 0xC0)))
# one non-ASCII character as its UTF-8 bytes: what a negated class or \D \W \S matches besides the ASCII bytes it does not exclude
_WIDE = ("alt", [("cat", [("set", frozenset(range(0xC2, 0xE0))), _CONT]), ("cat", [("set", frozenset(range(0xE0, 0xF0))), _CONT, _CONT]),
                 ("cat", [("set", frozenset(range(0xF0, 0xF5))), _CONT, _CONT, _CONT])])


# ---------------------------------------------------------------------------------------------------- the vocabulary's bytes
def _unicode_to_byte() -> Dict[str, int]:
    """the inverse of the GPT-2 byte <-> unicode alphabet of byte-level BPE vocabularies: printable bytes stand for themselves, the rest
    are the code points from 256 on, in byte order"""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    out, n = {chr(b): b for b in keep}, 0
    for b in range(256):
        if b not in keep:
            out[chr(256 + n)] = b
            n += 1
    return out


_U2B = _unicode_to_byte()
_vocab_cache: Dict[Tuple[int, int], Tuple[object, np.ndarray, np.ndarray]] = {}


def token_bytes(tokenizer, eot: int) -> Tuple[np.ndarray, np.ndarray]:
    """(tok_off int32 [eot + 1], bytes uint8) of the text tokens 0 .. eot - 1 of a byte-level BPE vocabulary, as wlx_pattern_vocab_set
    takes them. `tokenizer`: anything with `id_to_token(id)`, or with `.tokenizer` / `.tok` that has it. A token that is missing, has a
    character outside the byte alphabet, or is longer than 255 bytes is stored EMPTY: a token without bytes is never allowed under a
    pattern. Cached per tokenizer: the same arrays come back, which is what lets an engine see that it holds them already."""
    inner = tokenizer
    for name in ("tokenizer", "tok"):
        if not hasattr(inner, "id_to_token") and hasattr(inner, name):
            inner = getattr(inner, name)
    if not hasattr(inner, "id_to_token"):
        raise ValueError("token_bytes needs a tokenizer with id_to_token (a byte-level BPE vocabulary)")
    key = (id(inner), int(eot))
    hit = _vocab_cache.get(key)
    if hit is not None and hit[0] is inner:
        return hit[1], hit[2]
    off = np.zeros(int(eot) + 1, np.int32)
    parts: List[bytes] = []
    for t in range(int(eot)):
        s = inner.id_to_token(t)
        b = b""
        if s:
            try:
                b = bytes(_U2B[ch] for ch in s)
            except KeyError:
                b = b""
        if len(b) > PATTERN_MAX_TOKEN_BYTES:
            b = b""
        parts.append(b)
        off[t + 1] = off[t] + len(b)
    if int(off[-1]) > PATTERN_MAX_VOCAB_BYTES:
        raise ValueError(f"the vocabulary's text tokens have {int(off[-1])} bytes (at most {PATTERN_MAX_VOCAB_BYTES} vocabulary bytes)")
    by = np.frombuffer(b"".join(parts), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    _vocab_cache[key] = (inner, off, by)
    return off, by


# ---------------------------------------------------------------------------------------------------- the parser
# AST: ("set", frozenset of bytes) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
class _Parser:
    def __init__(self, regex: str, ignore_case: bool):
        self.s, self.i, self.ic = regex, 0, ignore_case

    def fail(self, what: str):
        raise ValueError(f"pattern {self.s!r}: {what} (at offset {self.i}) is not served")

    def peek(self) -> str:
        return self.s[self.i] if self.i < len(self.s) else ""

    def fold(self, bs: Iterable[int]) -> FrozenSet[int]:
        out = set(bs)
        if self.ic:
            out |= {b ^ 32 for b in out if 65 <= (b & ~32) <= 90}
        return frozenset(out)

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail("an unmatched ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "?":
                m, n = 0, 1
            elif c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "{":
                j = self.s.find("}", self.i)
                body = self.s[self.i + 1:j] if j > 0 else ""
                lo, sep, hi = body.partition(",")
                if not lo.isdigit() or (sep and hi and not hi.isdigit()):
                    self.fail("a '{' that opens no count {m}, {m,} or {m,n}")
                m, n = int(lo), (int(lo) if not sep else (int(hi) if hi else None))
                if m > MAX_REPEAT or (n is not None and (n > MAX_REPEAT or n < m)):
                    self.fail(f"the count {{{body}}} (0 <= m <= n <= {MAX_REPEAT})")
                self.i = j
            else:
                return node
            self.i += 1
            if self.peek() == "?":
                self.fail("a lazy quantifier")
            if self.peek() == "+":
                self.fail("a possessive quantifier")
            node = ("rep", node, m, n)

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.s[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("look-around")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("a named group")
                else:
                    self.fail("an inline flag or group extension '(?'")
            node = self.alt()
            if self.peek() != ")":
                self.fail("a '(' without its ')'")
            self.i += 1
            return node
        if c in ("^", "$"):
            self.fail(f"the anchor '{c}' (a pattern is always a full match)")
        if c in ("*", "+", "?", "{"):
            self.fail(f"a quantifier '{c}' with nothing to repeat")
        if c == "[":
            bs, wide = self.cls()
            return ("alt", [("set", bs), _WIDE]) if wide else ("set", bs)
        if c == ".":
            self.i += 1
            return ("set", _ALL)
        if c == "\\":
            wide = self.s[self.i + 1:self.i + 2] in _NEGATED
            bs = self.escape(False)
            return ("alt", [("set", bs), _WIDE]) if wide else ("set", bs)
        self.i += 1
        raw = c.encode("utf-8")
        if len(raw) == 1:
            return ("set", self.fold(raw))
        return ("cat", [("set", frozenset([b])) for b in raw])

    def escape(self, in_class: bool) -> FrozenSet[int]:
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in _SHORT:
            return _SHORT[c]
        if c in _CTRL and not (c == "0" and self.peek().isdigit()):
            return frozenset([_CTRL[c]])
        if c == "x":
            h = self.s[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.fail("an incomplete \\xHH escape")
            self.i += 2
            return frozenset([int(h, 16)])
        if c.isdigit():
            self.i -= 1
            self.fail("a back-reference")
        if c in "bBAZz" and not in_class:
            self.i -= 1
            self.fail(f"the anchor '\\{c}' (a pattern is always a full match)")
        if c.isalnum() or ord(c) > 127:
            self.i -= 1
            self.fail(f"the escape '\\{c}'")
        return frozenset([ord(c)])

    def cls(self) -> Tuple[FrozenSet[int], bool]:
        """-> (the ASCII bytes of the class, whether it also matches any one non-ASCII character)"""
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        out, first, wide = set(), True, False
        while True:
            c = self.peek()
            if c == "":
                self.fail("a '[' without its ']'")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            wide = wide or (c == "\\" and self.s[self.i + 1:self.i + 2] in _NEGATED)
            lo = self.member()
            if self.peek() == "-" and self.s[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.member()
                if len(lo) != 1 or len(hi) != 1 or min(hi) < min(lo):
                    self.fail("a class range whose ends are not two ascending characters")
                out |= set(range(min(lo), min(hi) + 1))
            else:
                out |= lo
        out = self.fold(out)
        return frozenset(_ASCII - out if negate else out), wide != negate

    def member(self) -> FrozenSet[int]:
        c = self.peek()
        if c == "\\":
            return self.escape(True)
        if ord(c) > 127:
            self.fail("a non-ASCII character inside a class")
        self.i += 1
        return frozenset([ord(c)])


# ---------------------------------------------------------------------------------------------------- Thompson construction
class _Nfa:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[FrozenSet[int], int]]] = []

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > 200000:
            raise ValueError(f"the pattern expands past 200000 automaton nodes before determinisation (at most {PATTERN_MAX_STATES} states)")
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        a, b = self.new(), self.new()
        if kind == "set":
            self.edges[a].append((node[1], b))
        elif kind == "cat":
            cur = a
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[cur].append(x)
                cur = y
            self.eps[cur].append(b)
        elif kind == "alt":
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[a].append(x)
                self.eps[y].append(b)
        else:
            _, sub, m, n = node
            cur = a
            for _i in range(m):
                x, y = self.build(sub)
                self.eps[cur].append(x)
                cur = y
            if n is None:
                x, y = self.build(sub)
                self.eps[cur] += [x, b]
                self.eps[y] += [x, b]
            else:
                for _i in range(n - m):
                    x, y = self.build(sub)
                    self.eps[cur] += [x, b]
                    cur = y
                self.eps[cur].append(b)
        return a, b

    def closure(self, states: Iterable[int]) -> FrozenSet[int]:
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


@dataclass
class Pattern:
    """What wlx_pattern_set takes: state 0 is the start state, trans[state, byte_class[byte]] the next state or DEAD (0xFFFF)."""
    regex: str
    byte_class: np.ndarray          # uint8 [256]
    trans: np.ndarray               # uint16 [n_states, n_classes]
    accept: np.ndarray              # uint8 [n_states], 0 or 1
    ignore_case: bool = False
    leading_space: bool = True
    _dead_cache: Dict[tuple, List[int]] = field(default_factory=dict, repr=False, compare=False)

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.trans.shape[1])

    def step(self, state: int, data: Union[int, bytes]) -> int:
        """the state after the byte(s) `data` from `state`, -1 where the walk dies"""
        for b in (bytes([data]) if isinstance(data, int) else bytes(data)):
            state = int(self.trans[state, self.byte_class[b]])
            if state == DEAD:
                return -1
        return state

    def accepts(self, text: Union[str, bytes]) -> bool:
        """is `text` (its UTF-8 bytes) in the language? A full match from the start state."""
        s = self.step(0, text.encode("utf-8") if isinstance(text, str) else text)
        return s >= 0 and bool(self.accept[s])

    def allowed(self, state: int, tok_off: np.ndarray, tok_bytes: np.ndarray) -> np.ndarray:
        """the ids of the text tokens (ascending) whose bytes can be walked from `state`: what the device leaves finite there"""
        off = np.asarray(tok_off, np.int64)
        n = off[1:] - off[:-1]
        cls = self.byte_class[np.asarray(tok_bytes, np.uint8)].astype(np.int64)
        ids = np.nonzero(n > 0)[0]
        cur = np.full(ids.shape, int(state), np.int64)
        k, done = 0, [np.zeros(0, np.int64)]
        while ids.size:                                         # byte k of every token still alive: almost all die at k = 0
            cur = self.trans[cur, cls[off[ids] + k]].astype(np.int64)
            live = cur != DEAD
            ids, cur = ids[live], cur[live]
            k += 1
            more = n[ids] > k
            done.append(ids[~more])
            ids, cur = ids[more], cur[more]
        return np.sort(np.concatenate(done))

    def dead_states(self, tok_off: np.ndarray, tok_bytes: np.ndarray, suppressed: Iterable[int], blank: Optional[int] = None) -> List[int]:
        """the states a row could not leave: every token allowed there is in `suppressed` (for the start state also `blank`, which
        suppress_blank removes at the first generated position) — or none is allowed at all and the state does not accept. Cached per
        (eot, suppress set, blank)."""
        sup = tuple(sorted({int(t) for t in suppressed}))
        key = (int(np.asarray(tok_off).shape[0]) - 1, sup, blank)
        hit = self._dead_cache.get(key)
        if hit is not None:
            return hit
        sup_a = np.asarray(sup, np.int64)
        out = []
        for s in range(self.n_states):
            ids = self.allowed(s, tok_off, tok_bytes)
            left = ids[~np.isin(ids, sup_a)]
            if s == 0 and blank is not None:
                left = left[left != blank]
            if (ids.size and not left.size) or (not ids.size and not self.accept[s]):
                out.append(s)
        self._dead_cache[key] = out
        return out


def compile_pattern(regex: str, *, ignore_case: bool = False, leading_space: bool = True) -> Pattern:
    """Compile `regex` into a Pattern (module docstring). ValueError names the construct that is not served or the limit that is broken
    (4096 states, 24576 cells = states x byte classes)."""
    if not isinstance(regex, str) or not regex:
        raise ValueError("a pattern is a non-empty regular expression string")
    ast = _Parser(regex, ignore_case).parse()
    if leading_space:
        ast = ("cat", [("rep", ("set", frozenset([32])), 0, 1), ast])
    nfa = _Nfa()
    start, final = nfa.build(ast)
    # the classes of bytes the expression tells apart: bytes that lie in the same edge sets
    sets = sorted({bs for es in nfa.edges for bs, _t in es}, key=sorted)
    sig: Dict[Tuple[int, ...], int] = {}
    atom_of = [0] * 256
    for b in range(256):
        atom_of[b] = sig.setdefault(tuple(i for i, bs in enumerate(sets) if b in bs), len(sig))
    n_atoms = len(sig)
    rep = [atom_of.index(a) for a in range(n_atoms)]            # one byte per atom
    # ---- subset construction, breadth first
    s0 = nfa.closure([start])
    index: Dict[FrozenSet[int], int] = {s0: 0}
    order = [s0]
    rows: List[List[int]] = []
    at = 0
    while at < len(order):
        cur = order[at]
        at += 1
        row = []
        for a in range(n_atoms):
            b = rep[a]
            tgt = {t for n in cur for bs, t in nfa.edges[n] if b in bs}
            if not tgt:
                row.append(-1)
                continue
            nxt = nfa.closure(tgt)
            k = index.get(nxt)
            if k is None:
                if len(order) >= _SUBSET_CAP:
                    raise ValueError(f"pattern {regex!r}: more than {_SUBSET_CAP} states before minimisation (at most {PATTERN_MAX_STATES} states)")
                k = index[nxt] = len(order)
                order.append(nxt)
            row.append(k)
        rows.append(row)
    T = np.asarray(rows, np.int64).reshape(len(order), n_atoms)
    acc = np.asarray([final in s for s in order], bool)
    # ---- trimming: a state that cannot reach an accepting state is dead
    live = acc.copy()
    dist = np.where(acc, 0, -1)                 # bytes to the nearest accepting state: states that differ in it are never equivalent
    rounds = 0
    while True:
        grown = live | ((T >= 0) & live[np.maximum(T, 0)]).any(axis=1)
        if (grown == live).all():
            break
        rounds += 1
        dist[grown & ~live] = rounds
        live = grown
    if not live[0]:
        raise ValueError(f"pattern {regex!r}: the language is empty (no text matches)")
    T = np.where((T >= 0) & live[np.maximum(T, 0)], T, -1)
    # ---- minimisation: Moore's refinement over the live states (-1 is the dead class), seeded with the distance to acceptance — which
    # tells the states of a counter like \\d{1000} apart at once, where acceptance alone would need a round per state
    part = np.where(live, dist.astype(np.int64), -1)
    while True:
        nxt_part = np.where(T >= 0, part[np.maximum(T, 0)], -1)
        keys = np.concatenate([part[:, None], nxt_part], axis=1)
        _u, inv = np.unique(keys, axis=0, return_inverse=True)
        new = np.where(live, inv.reshape(-1), -1)
        if len(set(new[live].tolist())) == len(set(part[live].tolist())):
            break
        part = new
    # number the classes breadth first from the start state: state 0 is the start state
    first_of: Dict[int, int] = {}
    for s in range(len(order)):
        if live[s]:
            first_of.setdefault(int(part[s]), s)
    number: Dict[int, int] = {int(part[0]): 0}
    queue = [int(part[0])]
    for c in queue:
        for t in T[first_of[c]]:
            if t >= 0 and int(part[t]) not in number:
                number[int(part[t])] = len(number)
                queue.append(int(part[t]))
    n_states = len(number)
    if n_states > PATTERN_MAX_STATES:
        raise ValueError(f"pattern {regex!r}: {n_states} states (at most {PATTERN_MAX_STATES} states)")
    M = np.full((n_states, n_atoms), DEAD, np.int64)
    accept = np.zeros(n_states, np.uint8)
    for c, k in number.items():
        src = first_of[c]
        accept[k] = 1 if acc[src] else 0
        for a in range(n_atoms):
            if T[src, a] >= 0:
                M[k, a] = number[int(part[T[src, a]])]
    # ---- byte classes: bytes with identical columns share a class
    _cols, col_cls = np.unique(M.T, axis=0, return_inverse=True)
    col_cls = col_cls.reshape(-1)
    n_classes = int(col_cls.max()) + 1
    if n_states * n_classes > PATTERN_MAX_CELLS:
        raise ValueError(f"pattern {regex!r}: {n_states} states x {n_classes} byte classes = {n_states * n_classes} cells "
                         f"(at most {PATTERN_MAX_CELLS} cells)")
    trans = np.full((n_states, n_classes), DEAD, np.uint16)
    for a in range(n_atoms):
        trans[:, col_cls[a]] = M[:, a].astype(np.uint16)
    byte_class = np.asarray([col_cls[atom_of[b]] for b in range(256)], np.uint8)
    return Pattern(regex=regex, byte_class=byte_class, trans=np.ascontiguousarray(trans), accept=accept, ignore_case=bool(ignore_case),
                   leading_space=bool(leading_space))


# ---- the calling thread's pattern (WhisperModelHIP.grammar(pattern=)): every generate of the thread installs it on its slot
_tls = threading.local()


def current() -> Optional[Pattern]:
    return getattr(_tls, "pattern", None)


class scope:
    """context manager: `pattern` is the calling thread's pattern inside the block (None: none); scopes nest, other threads are untouched"""

    def __init__(self, pattern: Optional[Pattern]):
        self.pattern = pattern

    def __enter__(self):
        self._prev = current()
        _tls.pattern = self.pattern
        return self.pattern

    def __exit__(self, *exc):
        _tls.pattern = self._prev
        return False


def install(slot, pattern: Optional[Pattern], vocab: Optional[Tuple[int, np.ndarray, np.ndarray]] = None) -> None:
    """Bring `slot` to `pattern` (None: no pattern). `vocab` = (eot, tok_off, bytes) of token_bytes: the engine's vocabulary bytes go up
    at the first install. The slot remembers what it holds, so a session that decodes under the same pattern call after call uploads it
    once. A slot that cannot take a pattern (no `set_pattern`) with one asked for is an error, never a silent unconstrained decode.
    Installing a pattern takes the slot out of its keyword and grammar modes (one mode at a time): what it held there is forgotten."""
    if getattr(slot, "_pattern", None) is pattern:
        return
    if pattern is None:
        slot.clear_pattern()
    else:
        if not hasattr(slot, "set_pattern"):
            raise RuntimeError("a pattern asked for, but this slot has no set_pattern")
        eng = getattr(slot, "engine", None)
        if vocab is not None and hasattr(eng, "set_pattern_vocab"):
            eng.set_pattern_vocab(*vocab)
        slot.set_pattern(pattern)
        slot._bias_table = slot._grammar = None
    slot._pattern = pattern


# ---- a pattern PER ITEM (include/wlx_pattern_items.h wlx_pattern_set_items / wlx_pattern_select)
class PatternSet:
    """Up to 64 compiled Patterns packed into the pool of wlx_pattern_set_items. `add` returns the pattern's index, storing one that is
    already there (the same object, or equal tables) once; ValueError names the limit a new pattern would pass and leaves the set as it
    was. `version` moves with every stored pattern: a slot uploads a set again only when it has grown (install_items)."""

    def __init__(self, patterns: Iterable[Pattern] = ()):
        self.tables: List[Pattern] = []
        self._index: Dict[bytes, int] = {}
        self.n_states = self.n_cells = 0
        self.version = 0
        for p in patterns:
            self.add(p)

    def __len__(self) -> int:
        return len(self.tables)

    @staticmethod
    def _key(p: Pattern) -> bytes:
        parts = ((p.byte_class, np.uint8), (p.trans, np.uint16), (p.accept, np.uint8))
        return np.asarray(p.trans.shape, np.int64).tobytes() + b"".join(np.ascontiguousarray(a, t).tobytes() for a, t in parts)

    def index(self, p: Pattern) -> Optional[int]:
        return self._index.get(self._key(p))

    def _refusal(self, p: Pattern) -> Optional[str]:
        if not isinstance(p, Pattern):
            return "a PatternSet holds compiled patterns (compile_pattern)"
        cells = p.n_states * p.n_classes
        if p.n_states > PATTERN_MAX_STATES:
            return f"a pattern has {p.n_states} states (at most {PATTERN_MAX_STATES} states per pattern)"
        if cells > PATTERN_MAX_CELLS:
            return f"a pattern has {cells} cells (at most {PATTERN_MAX_CELLS} cells per pattern)"
        if len(self.tables) + 1 > PATTERN_SET_MAX_TABLES:
            return f"the set would hold {len(self.tables) + 1} patterns (at most {PATTERN_SET_MAX_TABLES} patterns in one set)"
        if self.n_cells + cells > PATTERN_SET_MAX_CELLS:
            return f"the set would hold {self.n_cells + cells} cells (at most {PATTERN_SET_MAX_CELLS} cells in one set)"
        if self.n_states + p.n_states > PATTERN_SET_MAX_STATES:
            return f"the set would hold {self.n_states + p.n_states} states (at most {PATTERN_SET_MAX_STATES} states in one set)"
        return None

    def fits(self, p: Pattern) -> bool:
        """`add(p)` would succeed (a pattern already stored always fits)"""
        return (isinstance(p, Pattern) and self._key(p) in self._index) or self._refusal(p) is None

    def add(self, p: Pattern) -> int:
        if isinstance(p, Pattern):
            i = self._index.get(self._key(p))
            if i is not None:
                return i
        why = self._refusal(p)
        if why:
            raise ValueError(why)
        self._index[self._key(p)] = len(self.tables)
        self.tables.append(p)
        self.n_states += p.n_states
        self.n_cells += p.n_states * p.n_classes
        self.version += 1
        return len(self.tables) - 1

    def packed(self):
        """the arrays of wlx_pattern_set_items: (n_states [T], n_classes [T], byte_class [T * 256], trans [cells], accept [states]), the
        tables back to back without pads"""
        ts = self.tables
        cat = lambda xs, t: np.ascontiguousarray(np.concatenate([np.asarray(x, t).ravel() for x in xs]) if xs else np.zeros(0, t), dtype=t)
        return (np.asarray([p.n_states for p in ts], np.int32), np.asarray([p.n_classes for p in ts], np.int32),
                cat([p.byte_class for p in ts], np.uint8), cat([p.trans for p in ts], np.uint16), cat([p.accept for p in ts], np.uint8))


def current_items() -> Optional["item_scope"]:
    return getattr(_tls, "items", None)


class item_scope:
    """context manager: `patterns[i]` (a Pattern, or None: that item decodes unconstrained) is the pattern of prompt i of every generate
    call the calling thread makes inside the block; scopes nest, other threads are untouched. `pattern_set`: the set the patterns go into
    (a job passes one set for all its decode groups, so a slot uploads it once); without one the scope owns a set of its own."""

    def __init__(self, patterns: Sequence[Optional[Pattern]], pattern_set: Optional[PatternSet] = None):
        self.patterns = list(patterns)
        self.pattern_set = pattern_set if pattern_set is not None else PatternSet()

    def __enter__(self):
        self._prev = current_items()
        _tls.items = self
        return self

    def __exit__(self, *exc):
        _tls.items = self._prev
        return False


def install_items(slot, patterns: Sequence[Optional[Pattern]], pattern_set: PatternSet,
                  vocab: Optional[Tuple[int, np.ndarray, np.ndarray]] = None) -> List[int]:
    """Bring `slot` to the per-item route for a generate call over `patterns` (one per prompt, None: unconstrained): every pattern is
    stored in `pattern_set` (ValueError names a pool limit), the slot uploads the set unless it holds it already, and the table index of
    every prompt is returned (-1: none) for Slot.select_patterns per decode group. A call none of whose prompts has a pattern keeps a
    slot that holds THIS set in per-item mode with every item deselected (the kernel then touches no logit), and clears any other slot.
    `vocab` as for `install`. A slot that cannot take a set (no `set_patterns`) with one asked for is an error, never a silent
    unconstrained decode."""
    idx = [-1 if p is None else pattern_set.add(p) for p in patterns]
    if getattr(slot, "_pattern", None) is pattern_set and getattr(slot, "_pattern_set_version", None) == pattern_set.version:
        return idx
    if all(i < 0 for i in idx):
        if getattr(slot, "_pattern", None) is not None:
            install(slot, None)
        return idx
    if not hasattr(slot, "set_patterns"):
        raise RuntimeError("a pattern per item asked for, but this slot has no set_patterns")
    eng = getattr(slot, "engine", None)
    if vocab is not None and hasattr(eng, "set_pattern_vocab"):
        eng.set_pattern_vocab(*vocab)
    slot.set_patterns(pattern_set)
    slot._pattern, slot._pattern_set_version, slot._bias_table, slot._grammar = pattern_set, pattern_set.version, None, None
    return idx
