"""N-gram language-model fusion (include/wlx_lm.h; csrc/dec_lm.hip): the host side. A backoff n-gram model over TOKEN
ids — read from an ARPA file written from tokenised text, or counted from a small corpus — becomes the automaton the decode step
walks: a state per context, sorted explicit edges, backoff links. `score_row`, `next_state` and `fuse_row` restate the kernel in
float64: they are the oracle of its tests.

Alphabet A: the text tokens 0 .. eot - 1 and eot (end of sentence). Scores are natural logarithms."""
from __future__ import annotations

import math
import os
import threading
from collections import defaultdict
from typing import Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib

# The fusion weight where the caller names none. NOT tuned: there is no real checkpoint and no domain corpus in this repository to tune
# it on; 0.3 is the usual starting point of shallow fusion in the literature.
DEFAULT_WEIGHT = 0.3
BOS = -1        # the sentence start inside a context tuple: never predicted, never fed


class NgramLM:
    """The automaton, as wlx_lm_create takes it. State 0 is the empty context (dense `unigram_logp` / `unigram_next`); state n > 0 has
    the edges [edge_off[n], edge_off[n + 1]) (`edge_tok` ascending, `edge_logp`, `edge_next`), backs off to `backoff_state[n]` at the
    price `backoff_weight[n]`. ValueError names the cap a model breaks."""

    def __init__(self, vocab: int, eot: int, order: int, start_state: int, edge_off, backoff_state, backoff_weight, edge_tok, edge_logp,
                 edge_next, unigram_logp, unigram_next):
        self.vocab, self.eot, self.order, self.start_state = int(vocab), int(eot), int(order), int(start_state)
        self.edge_off = np.ascontiguousarray(edge_off, dtype=np.int32)
        self.backoff_state = np.ascontiguousarray(backoff_state, dtype=np.int32)
        self.backoff_weight = np.ascontiguousarray(backoff_weight, dtype=np.float32)
        self.edge_tok = np.ascontiguousarray(edge_tok, dtype=np.int32)
        self.edge_logp = np.ascontiguousarray(edge_logp, dtype=np.float32)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32)
        self.unigram_logp = np.ascontiguousarray(unigram_logp, dtype=np.float32)
        self.unigram_next = np.ascontiguousarray(unigram_next, dtype=np.int32)
        if not 1 <= self.order <= _lib.LM_MAX_ORDER:
            raise ValueError(f"lm: order {self.order} outside 1..{_lib.LM_MAX_ORDER}")
        if not 1 <= self.vocab <= _lib.LM_MAX_VOCAB:
            raise ValueError(f"lm: a vocab of {self.vocab} outside 1..{_lib.LM_MAX_VOCAB}")
        if not 1 <= self.eot < self.vocab:
            raise ValueError(f"lm: eot {self.eot} outside 1..{self.vocab - 1} (the vocab)")
        if not 1 <= self.n_states <= _lib.LM_MAX_STATES:
            raise ValueError(f"lm: {self.n_states} states outside 1..{_lib.LM_MAX_STATES}")
        if self.n_edges > _lib.LM_MAX_EDGES:
            raise ValueError(f"lm: {self.n_edges} edges, at most {_lib.LM_MAX_EDGES}")
        if self.unigram_logp.size != self.vocab or self.unigram_next.size != self.vocab:
            raise ValueError(f"lm: the unigram arrays hold {self.unigram_logp.size} / {self.unigram_next.size} entries, the vocab has {self.vocab}")
        if not np.all(np.isfinite(self.unigram_logp[:self.eot + 1])):
            raise ValueError("lm: a unigram score inside the alphabet is not finite")

    @property
    def n_states(self) -> int:
        return self.backoff_state.size

    @property
    def n_edges(self) -> int:
        return self.edge_tok.size

    def packed(self):
        """the eight arrays in wlx_lm_create's order"""
        return (self.edge_off, self.backoff_state, self.backoff_weight, self.edge_tok, self.edge_logp, self.edge_next, self.unigram_logp,
                self.unigram_next)

    # ---- the float64 oracle
    def chain(self, state: int):
        """the contexts of `state`'s backoff chain (without the empty one) and the summed weights above each, then above the unigram level"""
        levels, above, acc = [], [], 0.0
        while state > 0:
            levels.append(state)
            above.append(acc)
            acc += float(self.backoff_weight[state])
            state = int(self.backoff_state[state])
        return levels, above, acc

    def score_row(self, state: int) -> np.ndarray:
        """s(v) for every v of A in `state`, float64 [eot + 1]"""
        levels, above, acc = self.chain(state)
        s = self.unigram_logp[:self.eot + 1].astype(np.float64) + acc
        for n, b in zip(reversed(levels), reversed(above)):         # the shortest context first: a longer one overwrites it
            lo, hi = self.edge_off[n], self.edge_off[n + 1]
            s[self.edge_tok[lo:hi]] = self.edge_logp[lo:hi].astype(np.float64) + b
        return s

    def next_state(self, state: int, tok: int) -> int:
        """the state after feeding `tok` in `state`: a token >= eot is transparent"""
        if not 0 <= state < self.n_states:
            state = self.start_state
        if tok >= self.eot:
            return state
        while state > 0:
            lo, hi = self.edge_off[state], self.edge_off[state + 1]
            i = lo + int(np.searchsorted(self.edge_tok[lo:hi], tok))
            if i < hi and self.edge_tok[i] == tok:
                return int(self.edge_next[i])
            state = int(self.backoff_state[state])
        return int(self.unigram_next[tok])

    def fuse_row(self, logits: np.ndarray, state: int, weight: float) -> np.ndarray:
        """l'(v) = l(v) + w s(v) - c over A with c = LSE_A(l + w s) - LSE_A(l), float64; everything behind eot as it was; a row without
        a finite logit in A as it was"""
        out = np.asarray(logits, dtype=np.float64).copy()
        a = out[:self.eot + 1]
        if not np.any(np.isfinite(a)):
            return out
        f = a + float(weight) * self.score_row(state)
        out[:self.eot + 1] = f - (_lse(f) - _lse(a))
        return out

    # ---- builders
    @classmethod
    def from_tables(cls, vocab: int, eot: int, order: int, unigram: np.ndarray, probs: Dict[Tuple[int, ...], Dict[int, float]],
                    bows: Dict[Tuple[int, ...], float]) -> "NgramLM":
        """`unigram` [eot + 1] ln-probabilities; probs[context][token] ln-probabilities of the explicit n-grams (contexts of 1 .. order - 1
        ids, BOS for the sentence start); bows[context] ln backoff weights. The states are the contexts, closed under suffix."""
        contexts = {c for c in probs if c} | {c for c, b in bows.items() if c and b != 0.0}
        if order > 1:
            contexts.add((BOS,))
        for c in list(contexts):
            if len(c) > order - 1:
                raise ValueError(f"lm: an n-gram of {len(c) + 1} ids in a model of order {order}")
            for k in range(1, len(c)):
                contexts.add(c[k:])
        index = {c: i + 1 for i, c in enumerate(sorted(contexts, key=lambda c: (len(c), c)))}
        index[()] = 0

        def longest(c):
            c = c[-(order - 1):] if order > 1 else ()
            while c not in index:
                c = c[1:]
            return index[c]
        n = len(index)
        off, boff, bw = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        tok, logp, nxt = [], [], []
        for c, i in sorted(index.items(), key=lambda kv: kv[1]):
            if i:
                boff[i], bw[i] = index[c[1:]], bows.get(c, 0.0)
                for t, p in sorted(probs.get(c, {}).items()):
                    tok.append(t); logp.append(p); nxt.append(0 if t == eot else longest(c + (t,)))
            off[i + 1] = len(tok)
        uni = np.zeros(vocab, np.float64)
        uni[:eot + 1] = unigram
        unext = np.zeros(vocab, np.int32)
        for v in range(eot):
            unext[v] = index.get((v,), 0)
        return cls(vocab, eot, order, index.get((BOS,), 0), off, boff, bw, tok, logp, nxt, uni, unext)

    @classmethod
    def from_arpa(cls, path_or_text: Union[str, os.PathLike], *, eot: int, vocab: Optional[int] = None) -> "NgramLM":
        """An ARPA file (a path, or its text) whose words are TOKEN ids as decimal strings plus <s>, </s> and <unk>: what any toolkit
        writes from a corpus of tokenised text. log10 scores become ln; </s> is `eot`; the tokens of A without a unigram share the <unk>
        mass uniformly, so every token stays finite. A word-level file (any other word) is a ValueError."""
        text = str(path_or_text)
        if "\\data\\" not in text:
            with open(path_or_text, "r", encoding="utf-8") as f:
                text = f.read()
        vocab = int(vocab) if vocab is not None else eot + 1
        ln10 = math.log(10.0)

        def word(w):
            if w == "<s>":
                return BOS
            if w == "</s>":
                return eot
            if w == "<unk>":
                return None
            if not w.isdigit():
                raise ValueError(f"lm: the ARPA word {w!r} is not a token id: word-level ARPA files are out of scope (write the model from tokenised text)")
            if int(w) >= eot:
                raise ValueError(f"lm: the ARPA token {w} is outside the text tokens 0..{eot - 1}")
            return int(w)
        grams, bows, order, n, unk = defaultdict(dict), {}, 0, 0, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:line.index("-")])
                order = max(order, n)
                continue
            parts = line.split()
            if n < 1 or len(parts) < n + 1:
                raise ValueError(f"lm: cannot read the ARPA line {line!r}")
            p, ids = float(parts[0]) * ln10, [word(w) for w in parts[1:n + 1]]
            bow = float(parts[n + 1]) * ln10 if len(parts) > n + 1 else 0.0
            if None in ids:
                if n == 1:
                    unk = p
                continue                        # (an n-gram through <unk> names no token: skipped)
            if BOS in ids[1:] or eot in ids[:-1]:
                continue
            if ids[-1] != BOS:
                grams[tuple(ids[:-1])][ids[-1]] = p
            if bow != 0.0 and ids[-1] != eot:
                bows[tuple(ids)] = bow
        if order < 1:
            raise ValueError("lm: no n-grams in the ARPA text")
        uni = np.full(eot + 1, np.nan)
        for t, p in grams.pop((), {}).items():
            uni[t] = p
        missing = np.isnan(uni)
        if missing.any():
            if unk is None or not math.isfinite(unk) or unk < -90:
                raise ValueError(f"lm: {int(missing.sum())} tokens have no unigram and the ARPA file has no <unk> mass to share among them")
            uni[missing] = unk - math.log(int(missing.sum()))
        return cls.from_tables(vocab, eot, order, uni, grams, bows)

    @classmethod
    def from_corpus(cls, texts: Iterable[Union[str, Sequence[int]]], tokenizer, order: int = 3, *, eot: Optional[int] = None,
                    vocab: Optional[int] = None) -> "NgramLM":
        """Counted from `texts` (strings, through tokenizer.encode, or token lists) with INTERPOLATED Witten-Bell smoothing — no
        count-of-counts, so a corpus of a few sentences works: P(w | c) = (n(c, w) + T(c) P(w | c')) / (n(c) + T(c)), T(c) the distinct
        continuations of c, down to a uniform distribution over A. Stored in backoff form: the explicit scores are the interpolated
        ones, the backoff weight of c is ln(T(c) / (n(c) + T(c)))."""
        eot = int(eot if eot is not None else tokenizer.eot)
        vocab = int(vocab) if vocab is not None else eot + 1
        if not 1 <= order <= _lib.LM_MAX_ORDER:
            raise ValueError(f"lm: order {order} outside 1..{_lib.LM_MAX_ORDER}")
        counts = defaultdict(lambda: defaultdict(int))
        for t in texts:
            ids = [i for i in (tokenizer.encode(t) if isinstance(t, str) else list(t)) if 0 <= i < eot]
            sent = [BOS] + ids + [eot]
            for i in range(1, len(sent)):
                for k in range(0, min(order - 1, i) + 1):
                    counts[tuple(sent[i - k:i])][sent[i]] += 1
        if not counts:
            raise ValueError("lm: an empty corpus")
        n_a = eot + 1
        c0 = counts[()]
        n0, t0 = sum(c0.values()), len(c0)
        uni = np.full(n_a, (t0 / n_a) / (n0 + t0))
        for w, c in c0.items():
            uni[w] += c / (n0 + t0)

        def p_of(ctx, w):                       # the interpolated probability, recursively through the shorter contexts
            if not ctx:
                return uni[w]
            if ctx not in counts:
                return p_of(ctx[1:], w)
            d = counts[ctx]
            n, t = sum(d.values()), len(d)
            return (d.get(w, 0) + t * p_of(ctx[1:], w)) / (n + t)
        probs, bows = {}, {}
        for ctx, d in counts.items():
            if not ctx:
                continue
            n, t = sum(d.values()), len(d)
            probs[ctx] = {w: math.log(p_of(ctx, w)) for w in d}
            bows[ctx] = math.log(t / (n + t))
        return cls.from_tables(vocab, eot, order, np.log(uni), probs, bows)


def _lse(x: np.ndarray) -> float:
    m = np.max(x)
    return float(m + np.log(np.sum(np.exp(x - m))))


# ---- the calling thread's model (WhisperModelHIP.language_model): every generate of the thread sets it on its slot
_tls = threading.local()


def current() -> Optional[Tuple[NgramLM, float]]:
    return getattr(_tls, "lm", None)


class scope:
    """context manager: (`lm`, `weight`) is the calling thread's language model inside the block (None: none); scopes nest, other threads
    are untouched"""

    def __init__(self, lm: Optional[NgramLM], weight: float = DEFAULT_WEIGHT):
        if lm is not None:
            if not isinstance(lm, NgramLM):
                raise ValueError("lm: an NgramLM is expected (NgramLM.from_arpa, NgramLM.from_corpus); a model per file or per item is out of scope")
            if not (math.isfinite(weight) and weight > 0):
                raise ValueError(f"lm: the weight {weight} must be finite and above 0")
        self.value = None if lm is None else (lm, float(weight))

    def __enter__(self):
        self._prev = current()
        _tls.lm = self.value
        return self.value

    def __exit__(self, *exc):
        _tls.lm = self._prev
        return False


def install(slot, value: Optional[Tuple[NgramLM, float]]) -> None:
    """Bring `slot` to (`lm`, weight) (None: no model). The slot remembers what it holds: a session that decodes under the same model call
    after call sets it once, and the model itself goes to the engine once (Engine.create_lm). A slot that cannot take a model (no
    `set_lm`) with one asked for is an error, never a silent unfused decode."""
    if getattr(slot, "_lm", None) == value:
        return
    if value is None:
        slot.clear_lm()
    else:
        if not hasattr(slot, "set_lm"):
            raise RuntimeError("a language model asked for, but this slot has no set_lm")
        slot.set_lm(value[0], value[1])
        slot._bias_table = slot._grammar = slot._pattern = None
    slot._lm = value


# ---- a model and a weight PER ITEM (include/wlx_lm_items.h wlx_lm_set_items / wlx_lm_select)
class LmSet:
    """Up to 64 (model, weight) entries: the pool of wlx_lm_set_items. `add` returns the entry's index, storing a pair that is already
    there (the same model object at the same weight) once; the models themselves are stored once each (`models`, at most 8: the engine
    holds that many), so one model at two weights is two entries over one model. ValueError names the limit a new entry would pass and
    leaves the set as it was. `version` moves with every stored entry: a slot uploads a set again only when it has grown
    (install_items)."""

    def __init__(self, entries: Iterable[Tuple[NgramLM, float]] = ()):
        self.models: list = []
        self.entries: list = []                 # (index into `models`, weight)
        self._index: Dict[Tuple[int, float], int] = {}
        self.version = 0
        for m, w in entries:
            self.add(m, w)

    def __len__(self) -> int:
        return len(self.entries)

    def _model(self, lm: NgramLM) -> Optional[int]:
        return next((i for i, m in enumerate(self.models) if m is lm), None)

    def _refusal(self, lm, weight) -> Optional[str]:
        if not isinstance(lm, NgramLM):
            return "an LmSet holds NgramLM models (NgramLM.from_arpa, NgramLM.from_corpus)"
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not (math.isfinite(weight) and weight > 0):
            return f"lm: the weight {weight} must be finite and above 0"
        if self.models and (lm.eot, lm.vocab) != (self.models[0].eot, self.models[0].vocab):
            return (f"lm: a model for end-of-text {lm.eot} in a vocabulary of {lm.vocab} next to one for {self.models[0].eot} in "
                    f"{self.models[0].vocab}: the models of one set serve one vocabulary")
        if len(self.entries) + 1 > _lib.LM_SET_MAX_ENTRIES:
            return f"the set would hold {len(self.entries) + 1} entries (at most {_lib.LM_SET_MAX_ENTRIES} entries in one set)"
        if self._model(lm) is None and len(self.models) + 1 > _lib.LM_MAX_MODELS:
            return f"the set would hold {len(self.models) + 1} models (at most {_lib.LM_MAX_MODELS} models in one set)"
        return None

    def index(self, lm: NgramLM, weight: float) -> Optional[int]:
        m = self._model(lm)
        return None if m is None else self._index.get((m, float(weight)))

    def fits(self, lm: NgramLM, weight: float) -> bool:
        """`add(lm, weight)` would succeed (an entry already stored always fits)"""
        return self._refusal(lm, weight) is None or (isinstance(lm, NgramLM) and self.index(lm, weight) is not None)

    def add(self, lm: NgramLM, weight: float = DEFAULT_WEIGHT) -> int:
        if isinstance(lm, NgramLM) and isinstance(weight, (int, float)) and self.index(lm, weight) is not None:
            return self.index(lm, weight)
        why = self._refusal(lm, weight)
        if why:
            raise ValueError(why)
        m = self._model(lm)
        if m is None:
            self.models.append(lm)
            m = len(self.models) - 1
        self._index[(m, float(weight))] = len(self.entries)
        self.entries.append((m, float(weight)))
        self.version += 1
        return len(self.entries) - 1


def current_items() -> Optional["item_scope"]:
    return getattr(_tls, "items", None)


class item_scope:
    """context manager: `values[i]` — an (NgramLM, weight) pair, or None: that item is not fused — is the model of prompt i of every
    generate call the calling thread makes inside the block; scopes nest, other threads are untouched. `lm_set`: the set the pairs go
    into (a job passes one set for all its decode groups, so a slot uploads it once); without one the scope owns a set of its own."""

    def __init__(self, values: Sequence[Optional[Tuple[NgramLM, float]]], lm_set: Optional[LmSet] = None):
        self.values = list(values)
        self.lm_set = lm_set if lm_set is not None else LmSet()

    def __enter__(self):
        self._prev = current_items()
        _tls.items = self
        return self

    def __exit__(self, *exc):
        _tls.items = self._prev
        return False


def install_items(slot, values: Sequence[Optional[Tuple[NgramLM, float]]], lm_set: LmSet) -> list:
    """Bring `slot` to the per-item route for a generate call over `values` (one per prompt, None: not fused): every pair is stored in
    `lm_set` (ValueError names a limit), the slot uploads the set unless it holds it already, and the entry index of every prompt is
    returned (-1: none) for Slot.select_lms per decode group. A call none of whose prompts has a model keeps a slot that holds THIS set
    in per-item mode with every item deselected (the kernel then touches nothing), and clears any other slot. A slot that cannot take a
    set (no `set_lms`) with one asked for is an error, never a silent unfused decode."""
    idx = [-1 if v is None else lm_set.add(v[0], v[1]) for v in values]
    if getattr(slot, "_lm", None) is lm_set and getattr(slot, "_lm_set_version", None) == lm_set.version:
        return idx
    if all(i < 0 for i in idx):
        if getattr(slot, "_lm", None) is not None:
            install(slot, None)
        return idx
    if not hasattr(slot, "set_lms"):
        raise RuntimeError("a language model per item asked for, but this slot has no set_lms")
    slot.set_lms(lm_set)
    slot._lm, slot._lm_set_version, slot._bias_table, slot._grammar, slot._pattern = lm_set, lm_set.version, None, None, None
    return idx
