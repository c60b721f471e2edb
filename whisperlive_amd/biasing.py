"""Keyword boosting, host side: phrases and per-token values compiled into the bias table the decode step reads on the device
(include/wlx.h wlx_bias_set, csrc/dec_bias.hip), and the NumPy restatement of what the kernel does with it.

Semantics. `phrases` become an Aho-Corasick automaton over token ids. A string is encoded the way `hotwords` is, as
``" " + phrase.strip()``, and once more without the leading space when that gives other tokens; a token list is taken as it is;
duplicates are dropped. Node 0 is the root (nothing matched). After a generated token the row's node is the longest suffix of what
it generated that is a prefix of some phrase — the failure links are closed here, so every node carries the sorted list of its
explicit edges ``(token, next node)``: every token that leads to a node other than the root, through the node's own children first,
then through its failure chain. Any other token leads to the root. A node that ends a phrase restarts the walk: its failure link is
the root, so it carries its own children (a longer phrase it is a prefix of still completes) and the root's edges. A token ``>= eot``
(specials, timestamps) sends every node to the root and is never an edge.

For a row in node n the kernel adds, before anything of the search reads the row (pre-softmax, like OpenAI's ``logit_bias``):
``boost`` on every edge token of n, one float32 add; then ``value`` on every ``logit_bias`` token, one float32 add. A bonus given on
a partial match is not taken back when the match breaks, and the scores (``avg_logprob``) are those of the biased distribution.

The default boost is NOT tuned: no real checkpoint was at hand when this was written (DESIGN.md §25 says so, as §22 does for the
clustering threshold)."""
from __future__ import annotations

import math
import threading
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import BIAS_MAX_EDGES, BIAS_MAX_NODES, BIAS_MAX_TOKENS

DEFAULT_BOOST = 2.0          # unpinned (see the module docstring)


@dataclass
class BiasTable:
    """What wlx_bias_set takes, plus what the host needs to restate the kernel: `paths[n]` is the token tuple that leads from the
    root to node n, `terminal[n]` whether it ends a phrase."""
    vocab: int
    eot: int
    boost: np.float32
    edge_off: np.ndarray            # int32 [n_nodes + 1]
    edge_tok: np.ndarray            # int32 [n_edges], ascending within a node
    edge_next: np.ndarray           # int32 [n_edges]
    tok_ids: np.ndarray             # int32 [n_tok]
    tok_vals: np.ndarray            # float32 [n_tok]
    paths: List[Tuple[int, ...]] = field(default_factory=lambda: [()])
    terminal: List[bool] = field(default_factory=lambda: [False])
    phrases: List[Tuple[int, ...]] = field(default_factory=list)

    @property
    def n_nodes(self) -> int:
        return int(self.edge_off.shape[0]) - 1

    @property
    def n_edges(self) -> int:
        return int(self.edge_tok.shape[0])

    @property
    def empty(self) -> bool:
        """nothing would ever be added: a slot decodes without the bias launch"""
        return self.n_edges == 0 and self.tok_ids.shape[0] == 0

    def edges(self, state: int) -> Tuple[np.ndarray, np.ndarray]:
        a, b = int(self.edge_off[state]), int(self.edge_off[state + 1])
        return self.edge_tok[a:b], self.edge_next[a:b]

    def next_state(self, state: int, token: int) -> int:
        """the node after `token` was fed to a row whose parent was in `state`"""
        if token >= self.eot:
            return 0
        tok, nxt = self.edges(state)
        i = int(np.searchsorted(tok, token))
        return int(nxt[i]) if i < tok.shape[0] and tok[i] == token else 0

    def bias_row(self, row: np.ndarray, state: int) -> np.ndarray:
        """the kernel's two adds on a float32 logits row (in place), in its order"""
        assert row.dtype == np.float32
        tok, _ = self.edges(state)
        row[tok] += self.boost
        row[self.tok_ids] += self.tok_vals
        return row

    def apply(self, state: int, token: int) -> Tuple[int, np.ndarray]:
        """(state', delta row): the node after `token` and what the logits row of that node gains, as float32 [vocab] (the sum of the
        two adds; `bias_row` applies them one after the other, which is what is bit-identical to the device)."""
        s = self.next_state(state, token)
        return s, self.bias_row(np.zeros(self.vocab, np.float32), s)


def _finite(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} {x!r} is not a number")
    v = float(x)
    if not math.isfinite(v) or abs(v) > float(np.finfo(np.float32).max):
        raise ValueError(f"{what} {x!r} is not a finite float32")
    return v


def encode_phrases(phrases: Iterable[Union[str, Sequence[int]]], tokenizer=None) -> List[Tuple[int, ...]]:
    """phrases -> distinct token tuples: a string as `hotwords` is encoded (" " + phrase.strip()) and, where the tokens differ,
    without the leading space; a token list as it is"""
    if isinstance(phrases, (str, bytes)):
        raise ValueError("phrases must be a list of strings or token lists, not one string")
    out: List[Tuple[int, ...]] = []
    for ph in phrases:
        if isinstance(ph, str):
            if tokenizer is None:
                raise ValueError("a phrase given as text needs a tokenizer")
            text = ph.strip()
            if not text:
                raise ValueError("empty phrase")
            forms = [tuple(int(t) for t in tokenizer.encode(" " + text)), tuple(int(t) for t in tokenizer.encode(text))]
        else:
            try:
                forms = [tuple(int(t) for t in ph)]
            except (TypeError, ValueError):
                raise ValueError(f"phrase {ph!r} is neither text nor a list of token ids") from None
            if any(isinstance(t, (bool, float)) for t in ph):
                raise ValueError(f"phrase {ph!r}: token ids are integers")
        for f in forms:
            if not f:
                raise ValueError(f"phrase {ph!r} has no tokens")
            if f not in out:
                out.append(f)
    return out


def compile_bias(phrases: Optional[Iterable[Union[str, Sequence[int]]]] = None, boost: Optional[float] = None,
                 logit_bias: Optional[Dict[int, float]] = None, tokenizer=None, vocab: Optional[int] = None,
                 eot: Optional[int] = None) -> BiasTable:
    """Compile phrases and per-token values into a BiasTable (see the module docstring). `tokenizer`: anything with `encode(text) ->
    ids` (and `eot`, unless `eot` is given); `vocab`: the model's vocabulary size. ValueError names the cap that was exceeded: more
    than 4096 nodes, 16384 edges after the closure or 1024 logit_bias entries; a token outside the vocabulary; a phrase token that is a
    special or a timestamp (>= eot); a boost or value that is not finite."""
    if eot is None:
        eot = getattr(tokenizer, "eot", None)
    if vocab is None or eot is None:
        raise ValueError("compile_bias needs the vocabulary size and the <|endoftext|> id (vocab=, eot= or a tokenizer with .eot)")
    vocab, eot = int(vocab), int(eot)
    boost_f = np.float32(_finite(DEFAULT_BOOST if boost is None else boost, "boost"))
    seqs = encode_phrases(phrases or [], tokenizer)
    # ---- trie
    children: List[Dict[int, int]] = [{}]
    paths: List[Tuple[int, ...]] = [()]
    terminal: List[bool] = [False]
    for seq in seqs:
        n = 0
        for t in seq:
            if not 0 <= t < vocab:
                raise ValueError(f"phrase token {t} outside the vocabulary (every token < vocab = {vocab})")
            if t >= eot:
                raise ValueError(f"phrase token {t} is a special or timestamp token (>= eot = {eot}): phrases are text tokens")
            if t not in children[n]:
                if len(children) >= BIAS_MAX_NODES:
                    raise ValueError(f"the phrases need more than {BIAS_MAX_NODES} nodes (at most 4096 nodes: 256 phrases x 16 tokens)")
                children[n][t] = len(children)
                children.append({})
                paths.append(paths[n] + (t,))
                terminal.append(False)
            n = children[n][t]
        terminal[n] = True
    # ---- failure links, breadth first (the standard ones: a node's failure chain does not stop at a node that ends a phrase, the state
    # is the longest suffix that is a phrase prefix), then the closed edge lists: the list of the failure node — of the root for a node
    # that ends a phrase, which restarts the walk — overridden by the node's own children
    n_nodes = len(children)
    fail = [0] * n_nodes
    queue = deque(children[0].values())
    while queue:
        n = queue.popleft()
        for t, c in children[n].items():
            fail[c] = _std_goto(children, fail, fail[n], t)
            queue.append(c)
    std: List[Optional[Dict[int, int]]] = [None] * n_nodes      # the standard closure (what a failure chain through the node sees)
    for n in sorted(range(n_nodes), key=lambda i: len(paths[i])):          # (a failure node is shallower than its node)
        d = dict(std[fail[n]]) if n else {}
        d.update(children[n])
        std[n] = d
    closed: List[Dict[int, int]] = []
    for n in range(n_nodes):
        d = dict(std[0]) if terminal[n] else (dict(std[fail[n]]) if n else {})
        d.update(children[n])
        closed.append(d)
    n_edges = sum(len(d) for d in closed)
    if n_edges > BIAS_MAX_EDGES:
        raise ValueError(f"the phrases close to {n_edges} edges (at most {BIAS_MAX_EDGES} edges after the failure closure)")
    edge_off = np.zeros(n_nodes + 1, np.int32)
    edge_tok = np.zeros(n_edges, np.int32)
    edge_next = np.zeros(n_edges, np.int32)
    at = 0
    for n, d in enumerate(closed):
        for t in sorted(d):
            edge_tok[at], edge_next[at] = t, d[t]
            at += 1
        edge_off[n + 1] = at
    # ---- logit_bias
    lb = dict(logit_bias or {})
    if len(lb) > BIAS_MAX_TOKENS:
        raise ValueError(f"logit_bias has {len(lb)} entries (at most {BIAS_MAX_TOKENS} logit_bias entries)")
    ids: Dict[int, float] = {}
    for k, v in lb.items():
        if isinstance(k, (bool, float)):
            raise ValueError(f"logit_bias token {k!r} is not a token id")
        try:
            t = int(k)
        except (TypeError, ValueError):
            raise ValueError(f"logit_bias token {k!r} is not a token id") from None
        if not 0 <= t < vocab:
            raise ValueError(f"logit_bias token {t} outside the vocabulary (every token < vocab = {vocab})")
        if t in ids:
            raise ValueError(f"logit_bias names token {t} twice")
        ids[t] = _finite(v, f"the logit_bias value of token {t}")
    order = sorted(ids)
    return BiasTable(vocab=vocab, eot=eot, boost=boost_f, edge_off=edge_off, edge_tok=edge_tok, edge_next=edge_next,
                     tok_ids=np.asarray(order, np.int32), tok_vals=np.asarray([ids[t] for t in order], np.float32),
                     paths=paths, terminal=terminal, phrases=seqs)


def _std_goto(children, fail, n: int, t: int) -> int:
    """the standard Aho-Corasick transition from node n on token t (failure links of the nodes above already set)"""
    while True:
        c = children[n].get(t)
        if c is not None:
            return c
        if n == 0:
            return 0
        n = fail[n]


# ---- the calling thread's table (WhisperModelHIP.keyword_bias): every generate of the thread installs it on its slot
_tls = threading.local()


def current() -> Optional[BiasTable]:
    return getattr(_tls, "table", None)


class scope:
    """context manager: `table` is the calling thread's bias table inside the block (None: no table); scopes nest"""

    def __init__(self, table: Optional[BiasTable]):
        self.table = table

    def __enter__(self):
        self._prev = current()
        _tls.table = self.table
        return self.table

    def __exit__(self, *exc):
        _tls.table = self._prev
        return False


def install(slot, table: Optional[BiasTable]) -> None:
    """Bring `slot` to `table` (None or an empty table: no bias). The slot remembers what it holds, so a session that passes the same
    table call after call uploads it once. A slot that cannot take a table (no `set_bias`) with one asked for is an error, never a
    silent decode without it."""
    want = None if table is None or table.empty else table
    if getattr(slot, "_bias_table", None) is want:
        return
    if want is None:
        slot.clear_bias()
    else:
        if not hasattr(slot, "set_bias"):
            raise RuntimeError("keyword bias asked for, but this slot has no set_bias")
        slot.set_bias(want)
    slot._bias_table = want
