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
clustering threshold).

Per item and per session (include/wlx_bias_items.h wlx_bias_set_items / wlx_bias_select): `compile_compact` builds the COMPACT form of
the same automaton — node 0's list is the root's (its children), node n != 0 keeps only its own edges, the entries of its closed list
that are not identical to the root's entry for that token; an own edge whose token the root's list names too is flagged
(`edge_shared`): the root pass boosts that token, the own pass must not. Transition: the node's own list, else the root's list, else
the root. The root's list is so stored once per table, not once per node: a list of a thousand keywords is a thousand edges. A
`BiasSet` packs up to 64 compact tables into the pool a slot holds; `item_scope` names, for the calling thread, the table of every
prompt of the generate calls made inside it."""
from __future__ import annotations

import math
import threading
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import (BIAS_EDGE_SHARED, BIAS_MAX_EDGES, BIAS_MAX_NODES, BIAS_MAX_TOKENS, BIAS_SET_MAX_EDGES, BIAS_SET_MAX_NODES,
                   BIAS_SET_MAX_TABLES, BIAS_SET_MAX_TOKENS)

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
                 eot: Optional[int] = None, max_edges: Optional[int] = BIAS_MAX_EDGES) -> BiasTable:
    """Compile phrases and per-token values into a BiasTable (see the module docstring). `tokenizer`: anything with `encode(text) ->
    ids` (and `eot`, unless `eot` is given); `vocab`: the model's vocabulary size. ValueError names the cap that was exceeded: more
    than 4096 nodes, 16384 edges after the closure or 1024 logit_bias entries; a token outside the vocabulary; a phrase token that is a
    special or a timestamp (>= eot); a boost or value that is not finite. `max_edges=None` builds the closure without the edge cap:
    a table wlx_bias_set would refuse, kept as the oracle of the compact form (compile_compact)."""
    vocab, eot, boost_f, seqs = _compile_args(phrases, boost, tokenizer, vocab, eot)
    children, paths, terminal, fail = _trie(seqs, vocab, eot)
    n_nodes = len(children)
    # ---- the closed edge lists: the list of the failure node — of the root for a node that ends a phrase, which restarts the walk —
    # overridden by the node's own children
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
    if max_edges is not None and n_edges > max_edges:
        raise ValueError(f"the phrases close to {n_edges} edges (at most {max_edges} edges after the failure closure)")
    edge_off, edge_tok, edge_next = _pack_edges(closed)
    tok_ids, tok_vals = _token_list(logit_bias, vocab)
    return BiasTable(vocab=vocab, eot=eot, boost=boost_f, edge_off=edge_off, edge_tok=edge_tok, edge_next=edge_next,
                     tok_ids=tok_ids, tok_vals=tok_vals, paths=paths, terminal=terminal, phrases=seqs)


def _compile_args(phrases, boost, tokenizer, vocab, eot):
    if eot is None:
        eot = getattr(tokenizer, "eot", None)
    if vocab is None or eot is None:
        raise ValueError("compile_bias needs the vocabulary size and the <|endoftext|> id (vocab=, eot= or a tokenizer with .eot)")
    boost_f = np.float32(_finite(DEFAULT_BOOST if boost is None else boost, "boost"))
    return int(vocab), int(eot), boost_f, encode_phrases(phrases or [], tokenizer)


def _trie(seqs, vocab: int, eot: int):
    """the phrases' trie and its failure links: (children, paths, terminal, fail)"""
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
    # is the longest suffix that is a phrase prefix)
    n_nodes = len(children)
    fail = [0] * n_nodes
    queue = deque(children[0].values())
    while queue:
        n = queue.popleft()
        for t, c in children[n].items():
            fail[c] = _std_goto(children, fail, fail[n], t)
            queue.append(c)
    return children, paths, terminal, fail


def _pack_edges(lists: List[Dict[int, int]]):
    """per-node {token: next} -> (edge_off, edge_tok, edge_next), tokens ascending within a node"""
    n_edges = sum(len(d) for d in lists)
    edge_off = np.zeros(len(lists) + 1, np.int32)
    edge_tok = np.zeros(n_edges, np.int32)
    edge_next = np.zeros(n_edges, np.int32)
    at = 0
    for n, d in enumerate(lists):
        for t in sorted(d):
            edge_tok[at], edge_next[at] = t, d[t]
            at += 1
        edge_off[n + 1] = at
    return edge_off, edge_tok, edge_next


def _token_list(logit_bias, vocab: int):
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
    return np.asarray(order, np.int32), np.asarray([ids[t] for t in order], np.float32)


def _std_goto(children, fail, n: int, t: int) -> int:
    """the standard Aho-Corasick transition from node n on token t (failure links of the nodes above already set)"""
    while True:
        c = children[n].get(t)
        if c is not None:
            return c
        if n == 0:
            return 0
        n = fail[n]


@dataclass
class CompactTable:
    """One table of wlx_bias_set_items: the compact form (module docstring), and its NumPy restatement. `edge_next` holds plain node
    numbers; `edge_shared[i]`: edge i is an own edge whose token the root's list has too (the bit WLX_BIAS_EDGE_SHARED of the C-ABI's
    edge_next: `packed_next`)."""
    vocab: int
    eot: int
    boost: np.float32
    edge_off: np.ndarray            # int32 [n_nodes + 1]; node 0's list is the root's
    edge_tok: np.ndarray            # int32 [n_edges], ascending within a node
    edge_next: np.ndarray           # int32 [n_edges]
    edge_shared: np.ndarray         # bool [n_edges]
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
        return self.n_edges == 0 and self.tok_ids.shape[0] == 0

    @property
    def packed_next(self) -> np.ndarray:
        return (self.edge_next | np.where(self.edge_shared, BIAS_EDGE_SHARED, 0)).astype(np.int32)

    def key(self) -> bytes:
        """the table's content: two tables with the same key are stored once in a BiasSet"""
        k = getattr(self, "_key", None)
        if k is None:
            k = b"|".join([np.asarray([self.vocab, self.eot], np.int64).tobytes(), np.float32(self.boost).tobytes(), self.edge_off.tobytes(),
                           self.edge_tok.tobytes(), self.packed_next.tobytes(), self.tok_ids.tobytes(), self.tok_vals.tobytes()])
            self._key = k
        return k

    def edges(self, state: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        a, b = int(self.edge_off[state]), int(self.edge_off[state + 1])
        return self.edge_tok[a:b], self.edge_next[a:b], self.edge_shared[a:b]

    def next_state(self, state: int, token: int) -> int:
        """the node's own list, else the root's list, else the root; a token >= eot: the root"""
        if token >= self.eot:
            return 0
        for n in ((state, 0) if state else (0,)):
            tok, nxt, _ = self.edges(n)
            i = int(np.searchsorted(tok, token))
            if i < tok.shape[0] and tok[i] == token:
                return int(nxt[i])
        return 0

    def bias_row(self, row: np.ndarray, state: int) -> np.ndarray:
        """the kernel's adds on a float32 logits row (in place), in its order: the unflagged own edges, the root's list, the token list"""
        assert row.dtype == np.float32
        if state:
            tok, _, shared = self.edges(state)
            row[tok[~shared]] += self.boost
        row[self.edges(0)[0]] += self.boost
        row[self.tok_ids] += self.tok_vals
        return row

    def apply(self, state: int, token: int) -> Tuple[int, np.ndarray]:
        s = self.next_state(state, token)
        return s, self.bias_row(np.zeros(self.vocab, np.float32), s)

    def own_set(self) -> "BiasSet":
        """the one-table set of this table (keyword_bias(compact=True): selected for every item), built once"""
        bs = getattr(self, "_own_set", None)
        if bs is None:
            bs = self._own_set = BiasSet([self])
        return bs


def compile_compact(phrases: Optional[Iterable[Union[str, Sequence[int]]]] = None, boost: Optional[float] = None,
                    logit_bias: Optional[Dict[int, float]] = None, tokenizer=None, vocab: Optional[int] = None,
                    eot: Optional[int] = None) -> CompactTable:
    """compile_bias's arguments, phrases, encoding rules and failure links -> the compact form, built directly (the closure is never
    expanded: the work is the sum of the own lists). ValueError as compile_bias, but for the edges: a table's edges are capped only
    by the pool of the set it goes into (65536 edges)."""
    vocab, eot, boost_f, seqs = _compile_args(phrases, boost, tokenizer, vocab, eot)
    children, paths, terminal, fail = _trie(seqs, vocab, eot)
    n_nodes = len(children)
    root = children[0]
    # own(n) = what the failure node's standard closure holds BEYOND the root's list (nothing for a node that ends a phrase, whose walk
    # restarts at the root), overridden by n's children. A child of n != 0 is never the root's entry (it is a deeper node), and an entry
    # that differs from the root's stays different down the failure chain or is overridden by a child: no entry needs a second look.
    std_own: List[Optional[Dict[int, int]]] = [None] * n_nodes
    own: List[Dict[int, int]] = [dict(root)] + [{} for _ in range(n_nodes - 1)]
    std_own[0] = {}
    n_edges = len(root)
    for n in sorted(range(1, n_nodes), key=lambda i: len(paths[i])):
        d = dict(std_own[fail[n]])
        d.update(children[n])
        std_own[n] = d
        own[n] = dict(children[n]) if terminal[n] else d
        n_edges += len(own[n])
        if n_edges > BIAS_SET_MAX_EDGES:
            raise ValueError(f"the phrases need more than {BIAS_SET_MAX_EDGES} edges in the compact form (at most {BIAS_SET_MAX_EDGES} edges in one set)")
    edge_off, edge_tok, edge_next = _pack_edges(own)
    shared = np.zeros(edge_tok.shape[0], bool)
    r1 = int(edge_off[1])
    if r1 and edge_tok.shape[0] > r1:
        shared[r1:] = np.isin(edge_tok[r1:], edge_tok[:r1])
    tok_ids, tok_vals = _token_list(logit_bias, vocab)
    return CompactTable(vocab=vocab, eot=eot, boost=boost_f, edge_off=edge_off, edge_tok=edge_tok, edge_next=edge_next, edge_shared=shared,
                        tok_ids=tok_ids, tok_vals=tok_vals, paths=paths, terminal=terminal, phrases=seqs)


def compact_of(table) -> Optional[CompactTable]:
    """the compact form of a table: itself, or a BiasTable's phrases, boost and token list compiled again (once per table object)"""
    if table is None or isinstance(table, CompactTable):
        return table
    c = getattr(table, "_compact", None)
    if c is None:
        c = table._compact = compile_compact(table.phrases, float(table.boost), dict(zip(table.tok_ids.tolist(), table.tok_vals.tolist())),
                                             vocab=table.vocab, eot=table.eot)
    return c


class BiasSet:
    """Up to 64 compact tables packed into the pool of wlx_bias_set_items. `add` returns the table's index, storing a table that is
    already there (the same object, or equal content) once; ValueError names the cap a new table would exceed and leaves the set as it
    was. `version` moves with every stored table: a slot uploads a set again only when it has grown (install_set)."""

    def __init__(self, tables: Iterable[CompactTable] = ()):
        self.tables: List[CompactTable] = []
        self._index: Dict[bytes, int] = {}
        self.n_nodes = self.n_edges = self.n_tok = 0
        self.version = 0
        for t in tables:
            self.add(t)

    def __len__(self) -> int:
        return len(self.tables)

    @property
    def vocab(self) -> Optional[int]:
        return self.tables[0].vocab if self.tables else None

    def index(self, table: CompactTable) -> Optional[int]:
        return self._index.get(table.key())

    def _refusal(self, table: CompactTable) -> Optional[str]:
        if not isinstance(table, CompactTable):
            return "a BiasSet holds compact tables (compile_compact, compact_of)"
        if self.tables and (table.vocab, table.eot) != (self.tables[0].vocab, self.tables[0].eot):
            return "the tables of a set are compiled for one vocabulary"
        if table.n_nodes > BIAS_MAX_NODES:
            return f"a table has {table.n_nodes} nodes (at most {BIAS_MAX_NODES} nodes per table)"
        if table.tok_ids.shape[0] > BIAS_MAX_TOKENS:
            return f"a table has {table.tok_ids.shape[0]} logit_bias entries (at most {BIAS_MAX_TOKENS} logit_bias entries per table)"
        if len(self.tables) + 1 > BIAS_SET_MAX_TABLES:
            return f"the set would hold {len(self.tables) + 1} tables (at most {BIAS_SET_MAX_TABLES} tables in one set)"
        if self.n_nodes + table.n_nodes > BIAS_SET_MAX_NODES:
            return f"the set would hold {self.n_nodes + table.n_nodes} nodes (at most {BIAS_SET_MAX_NODES} nodes in one set)"
        if self.n_edges + table.n_edges > BIAS_SET_MAX_EDGES:
            return f"the set would hold {self.n_edges + table.n_edges} edges (at most {BIAS_SET_MAX_EDGES} edges in one set)"
        if self.n_tok + table.tok_ids.shape[0] > BIAS_SET_MAX_TOKENS:
            return f"the set would hold {self.n_tok + table.tok_ids.shape[0]} logit_bias entries (at most {BIAS_SET_MAX_TOKENS} logit_bias entries in one set)"
        return None

    def fits(self, table: CompactTable) -> bool:
        """`add(table)` would succeed (a table already stored always fits)"""
        return (isinstance(table, CompactTable) and table.key() in self._index) or self._refusal(table) is None

    def add(self, table: CompactTable) -> int:
        if isinstance(table, CompactTable):
            i = self._index.get(table.key())
            if i is not None:
                return i
        why = self._refusal(table)
        if why:
            raise ValueError(why)
        self._index[table.key()] = len(self.tables)
        self.tables.append(table)
        self.n_nodes += table.n_nodes
        self.n_edges += table.n_edges
        self.n_tok += int(table.tok_ids.shape[0])
        self.version += 1
        return len(self.tables) - 1

    def packed(self):
        """the arguments of wlx_bias_set_items: (n_nodes [T], edge_off [nodes + T] local per table, edge_tok, edge_next with the flag
        bit, boosts [T], n_tok [T], tok_ids, tok_vals)"""
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).ravel() for x in xs]) if xs else np.zeros(0, dt), dtype=dt)
        ts = self.tables
        return (np.asarray([t.n_nodes for t in ts], np.int32), cat([t.edge_off for t in ts], np.int32), cat([t.edge_tok for t in ts], np.int32),
                cat([t.packed_next for t in ts], np.int32), np.asarray([t.boost for t in ts], np.float32),
                np.asarray([t.tok_ids.shape[0] for t in ts], np.int32), cat([t.tok_ids for t in ts], np.int32), cat([t.tok_vals for t in ts], np.float32))

    def next_state(self, table: int, state: int, token: int) -> int:
        """the kernel's walk for an item that selects `table` (-1: none — the root)"""
        return 0 if table < 0 else self.tables[table].next_state(state if 0 <= state < self.tables[table].n_nodes else 0, token)

    def bias_row(self, table: int, row: np.ndarray, state: int) -> np.ndarray:
        return row if table < 0 else self.tables[table].bias_row(row, state)


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


# ---- the calling thread's table PER ITEM: one entry per prompt of the generate calls made inside the scope
def current_items() -> Optional["item_scope"]:
    return getattr(_tls, "items", None)


class item_scope:
    """context manager: `tables[i]` (a CompactTable, a BiasTable — taken in its compact form — or None: no bias for that item) is the
    table of prompt i of every generate call the calling thread makes inside the block; scopes nest, other threads are untouched.
    `bias_set`: the set the tables go into (a job passes one set for all its decode groups, so a slot uploads it once); without one the
    scope owns a set of its own."""

    def __init__(self, tables: Sequence, bias_set: Optional[BiasSet] = None):
        self.tables = list(tables)
        self.bias_set = bias_set if bias_set is not None else BiasSet()

    def __enter__(self):
        self._prev = current_items()
        _tls.items = self
        return self

    def __exit__(self, *exc):
        _tls.items = self._prev
        return False


def install_items(slot, tables: Sequence, bias_set: BiasSet, fallback=None) -> Optional[List[int]]:
    """Bring `slot` to the per-item route for a generate call over `tables` (one per prompt; None: `fallback`, the thread's single
    table, or no bias): every table is stored in `bias_set` (ValueError names a pool cap), the slot uploads the set unless it holds it
    already, and the table index of every prompt is returned (-1: none) for Slot.select_bias per decode group. None: no prompt has
    anything to add — the slot is cleared like `install(slot, None)`, unless it already holds `bias_set`: then every item is deselected."""
    want = [compact_of(t if t is not None else fallback) for t in tables]
    idx = [-1 if (t is None or t.empty) else bias_set.add(t) for t in want]
    if all(i < 0 for i in idx):
        # nothing to add for this call. A slot that already holds THIS set stays in per-item mode with every item deselected (the kernel
        # then touches no logit), so a job whose biased and unbiased groups alternate uploads its set once; any other slot is cleared
        if getattr(slot, "_bias_table", None) is bias_set and getattr(slot, "_bias_set_version", None) == bias_set.version:
            return idx
        if getattr(slot, "_bias_table", None) is not None:
            install(slot, None)
        return None
    if not hasattr(slot, "set_bias_items"):
        raise RuntimeError("per-item keyword bias asked for, but this slot has no set_bias_items")
    if getattr(slot, "_bias_table", None) is not bias_set or getattr(slot, "_bias_set_version", None) != bias_set.version:
        slot.set_bias_items(bias_set)
        slot._bias_table, slot._bias_set_version = bias_set, bias_set.version
    return idx
