"""Grammar-constrained decoding, host side: a closed phrase list compiled into the DFA over token ids that the decode step walks on the
device (include/wlx_grammar.h wlx_grammar_set, csrc/dec_grammar.hip).

The language is ``(phrase)*`` with ``repeat=True`` and ``phrase | empty`` without, over TEXT tokens only: specials and timestamps are
transparent to the walk, so a phrase may carry a timestamp in its middle. A phrase given as text is taken in the two forms keyword
boosting uses (biasing.encode_phrases: with and without the leading space); a token list as it is.

The compiler builds the trie of the phrases' token sequences, adds an empty move from every phrase end back to the root when `repeat` is
set, and determinises by subset construction — the device then never has to choose between continuing the longer phrase and starting the
next one: with the phrases ``a``, ``a b c``, ``b d`` the state after ``a`` holds both "inside a b c" and "at the root", and ``a b d`` is
reachable. Two reductions keep the table small without a full minimisation: every trie leaf (a phrase end with nothing behind it) is one
and the same END state, and END disappears from a subset that holds the root, which accepts and restarts already — so 1000 one-token
phrases are ONE state with 1000 edges onto itself. The start state accepts: a silent window is an empty transcript.

For a row in state n the kernel sets to -inf every logit of a text token that is no edge token of n, and the logit of end-of-text unless
accept[n]; ids above end-of-text keep their bits (the search's own rules decide about timestamps). tests/grammar_ref.py restates that.
"""
from __future__ import annotations

import threading
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import GRAMMAR_MAX_EDGES, GRAMMAR_MAX_STATES
from .biasing import encode_phrases

_END = -1       # every trie leaf in a subset: a phrase has ended and nothing continues it


@dataclass
class Grammar:
    """What wlx_grammar_set takes: state 0 is the start state."""
    vocab: int
    eot: int
    edge_off: np.ndarray            # int32 [n_states + 1]
    edge_tok: np.ndarray            # int32 [n_edges], ascending within a state, every token < eot
    edge_next: np.ndarray           # int32 [n_edges], 0 .. n_states - 1
    accept: np.ndarray              # int32 [n_states], 0 or 1
    repeat: bool = True
    phrases: List[Tuple[int, ...]] = field(default_factory=list)

    @property
    def n_states(self) -> int:
        return int(self.edge_off.shape[0]) - 1

    @property
    def n_edges(self) -> int:
        return int(self.edge_tok.shape[0])

    def edges(self, state: int) -> Tuple[np.ndarray, np.ndarray]:
        a, b = int(self.edge_off[state]), int(self.edge_off[state + 1])
        return self.edge_tok[a:b], self.edge_next[a:b]

    def step(self, state: int, token: int) -> int:
        """the state after text token `token`, -1 where `state` has no edge for it"""
        tok, nxt = self.edges(state)
        i = int(np.searchsorted(tok, token))
        return int(nxt[i]) if i < tok.shape[0] and tok[i] == token else -1

    def dead_states(self, suppressed: Iterable[int], blank: Optional[int] = None) -> List[int]:
        """the states with edges whose EVERY edge token is in `suppressed` (for the start state also `blank`, which suppress_blank removes
        at the first generated position): a row there would keep no finite text logit"""
        sup = np.fromiter((int(t) for t in suppressed), np.int64)
        gone = np.isin(self.edge_tok, sup)
        out = []
        for n in range(self.n_states):
            a, b = int(self.edge_off[n]), int(self.edge_off[n + 1])
            g = gone[a:b] | (self.edge_tok[a:b] == blank) if (n == 0 and blank is not None) else gone[a:b]
            if b > a and bool(g.all()):
                out.append(n)
        return out


def accepts(dfa: Grammar, tokens: Sequence[int]) -> bool:
    """is the text of `tokens` in the language? Tokens >= eot (specials, timestamps) are skipped, as the device's walk skips them."""
    state = 0
    for t in tokens:
        if t >= dfa.eot:
            continue
        state = dfa.step(state, int(t))
        if state < 0:
            return False
    return bool(dfa.accept[state])


def compile_grammar(tokenizer, phrases: Iterable[Union[str, Sequence[int]]], repeat: bool = True, *, vocab: Optional[int] = None,
                    eot: Optional[int] = None) -> Grammar:
    """Compile a closed phrase list into a Grammar (module docstring). `tokenizer`: anything with `encode(text) -> ids` (and `.eot`
    where `eot` is not given); token lists need none. ValueError: an empty list; a phrase with no text token (empty, or a token that is
    a special or a timestamp, or outside the vocabulary); a DFA of more than 4096 states or 16384 edges (the limit is named)."""
    if eot is None:
        eot = getattr(tokenizer, "eot", None)
    if vocab is None or eot is None:
        raise ValueError("compile_grammar needs the vocabulary size and the <|endoftext|> id (vocab=, eot= or a tokenizer with .eot)")
    vocab, eot = int(vocab), int(eot)
    if phrases is None:
        raise ValueError("a grammar needs at least one phrase (an empty list allows nothing)")
    seqs = encode_phrases(phrases, tokenizer)
    if not seqs:
        raise ValueError("a grammar needs at least one phrase (an empty list allows nothing)")
    # ---- the trie
    children: List[Dict[int, int]] = [{}]
    terminal: List[bool] = [False]
    for seq in seqs:
        n = 0
        for t in seq:
            if not 0 <= t < vocab:
                raise ValueError(f"phrase token {t} outside the vocabulary (every token < vocab = {vocab})")
            if t >= eot:
                raise ValueError(f"phrase token {t} is a special or timestamp token (>= eot = {eot}): a phrase needs text tokens only")
            nxt = children[n].get(t)
            if nxt is None:
                nxt = children[n][t] = len(children)
                children.append({})
                terminal.append(False)
            n = nxt
        terminal[n] = True

    def canon(nodes) -> FrozenSet[int]:
        s = {(_END if not children[n] else n) for n in nodes}
        if repeat and (_END in s or any(n >= 0 and terminal[n] for n in s)):
            s.add(0)                        # the empty move from a phrase end back to the root
        if 0 in s:
            s.discard(_END)                 # the root accepts and has every continuation END stands for (none)
        return frozenset(s)

    # ---- subset construction, breadth first from {root}
    start = canon([0])
    index: Dict[FrozenSet[int], int] = {start: 0}
    order: List[FrozenSet[int]] = [start]
    lists: List[Dict[int, int]] = []
    queue = deque([start])
    n_edges = 0
    while queue:
        cur = queue.popleft()
        moves: Dict[int, List[int]] = {}
        for n in cur:
            if n >= 0:
                for t, c in children[n].items():
                    moves.setdefault(t, []).append(c)
        out: Dict[int, int] = {}
        for t, targets in moves.items():
            nxt = canon(targets)
            k = index.get(nxt)
            if k is None:
                if len(order) >= GRAMMAR_MAX_STATES:
                    raise ValueError(f"the grammar needs more than {GRAMMAR_MAX_STATES} states (at most {GRAMMAR_MAX_STATES} states)")
                k = index[nxt] = len(order)
                order.append(nxt)
                queue.append(nxt)
            out[t] = k
        n_edges += len(out)
        if n_edges > GRAMMAR_MAX_EDGES:
            raise ValueError(f"the grammar needs more than {GRAMMAR_MAX_EDGES} edges (at most {GRAMMAR_MAX_EDGES} edges)")
        lists.append(out)
    edge_off = np.zeros(len(order) + 1, np.int32)
    edge_tok = np.zeros(n_edges, np.int32)
    edge_next = np.zeros(n_edges, np.int32)
    at = 0
    for k, d in enumerate(lists):
        for t in sorted(d):
            edge_tok[at], edge_next[at] = t, d[t]
            at += 1
        edge_off[k + 1] = at
    accept = np.array([1 if (0 in s or _END in s or any(n >= 0 and terminal[n] for n in s)) else 0 for s in order], np.int32)
    return Grammar(vocab=vocab, eot=eot, edge_off=edge_off, edge_tok=edge_tok, edge_next=edge_next, accept=accept, repeat=bool(repeat),
                   phrases=seqs)


# ---- the calling thread's grammar (WhisperModelHIP.grammar): every generate of the thread installs it on its slot
_tls = threading.local()


def current() -> Optional[Grammar]:
    return getattr(_tls, "grammar", None)


class scope:
    """context manager: `grammar` is the calling thread's grammar inside the block (None: none); scopes nest, other threads are untouched"""

    def __init__(self, grammar: Optional[Grammar]):
        self.grammar = grammar

    def __enter__(self):
        self._prev = current()
        _tls.grammar = self.grammar
        return self.grammar

    def __exit__(self, *exc):
        _tls.grammar = self._prev
        return False


def install(slot, grammar: Optional[Grammar]) -> None:
    """Bring `slot` to `grammar` (None: no grammar). The slot remembers what it holds, so a session that decodes under the same grammar
    call after call uploads it once. A slot that cannot take a grammar (no `set_grammar`) with one asked for is an error, never a silent
    unconstrained decode. Installing a grammar takes the slot out of its keyword mode (one mode at a time): what it held there is forgotten."""
    if getattr(slot, "_grammar", None) is grammar:
        return
    if grammar is None:
        slot.clear_grammar()
    else:
        if not hasattr(slot, "set_grammar"):
            raise RuntimeError("a grammar asked for, but this slot has no set_grammar")
        slot.set_grammar(grammar)
        slot._bias_table = None
    slot._grammar = grammar
