"""Injected-logits cases for the device search (tests/test_gpu_search_batch.py) and their oracle answers: plain numpy, no GPU, nothing
but oracle.decoding. Every case is a seeded logits array [steps, items * R, vocab] (R = beam_size in beam mode, num_hypotheses when
sampling; item b owns rows [b * R, (b + 1) * R)), one prompt per item and the generate options; the answer of item b is

    odec.generate(odec.InjectedLogits(lg[:, b * R:(b + 1) * R]), prompt_b, opts, row_base=b * R)

tests/test_search_cases_host.py shows on the oracle alone that each case has the property it was built for and that its decisions are
`MARGIN` apart, so a GPU mismatch is never a near-tie. Seeds are fixed here; a seed whose case is not separated is replaced, the margin
never widened.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import decoding as odec

MARGIN = 1e-3            # what the suite allows between GPU and oracle scores of this hook (tests/test_gpu_parity.py)
VOCAB = {"micro": 2310, "full": 51865}   # tests/helpers.py MICRO (one text + one timestamp scan chunk); the multilingual vocabulary (26 chunks, ragged last text chunk)


def token_ids(vocab: int) -> odec.TokenIds:
    """tests/helpers.py token_ids_for (not imported: that module needs the package)"""
    tb = vocab - 1501
    return odec.TokenIds(sot=tb - 106, eot=tb - 107, no_timestamps=tb - 1, timestamp_begin=tb, no_speech=tb - 2, blank=220 if vocab > 1000 else 7)


def suppress_list(ids: odec.TokenIds) -> List[int]:
    """tests/helpers.py default_suppress"""
    tb = ids.timestamp_begin
    return sorted({1, 2, 7, 8, 9, 10, 14, 25, tb - 5, tb - 6, ids.sot, tb - 3, tb - 4})


def prompt_of(ids: odec.TokenIds, n: int, no_timestamps: bool = False) -> List[int]:
    """a prompt of n tokens that ends on <|startoftranscript|> (with no_timestamps: on <|startoftranscript|><|notimestamps|>)"""
    tail = [ids.sot, ids.no_timestamps] if no_timestamps else [ids.sot]
    assert n >= len(tail)
    return [3 + 2 * i for i in range(n - len(tail))] + tail


@dataclass
class Case:
    name: str
    vocab: str                               # "micro" | "full"
    R: int                                   # rows per item
    plens: Sequence[int]                     # prompt length per item
    kw: dict                                 # generate options (without ids / suppress_tokens)
    seed: int
    kind: str = "gauss"                      # "gauss" | "quant"
    peaky: float = 4.0
    eot: Sequence[float] = (6.0,)            # per item: added to the end-of-text logit from the second step on (-inf-like: never ends on it)
    fav: float = 0.0                         # > 0: six text ids favoured at every step (repetitions for the penalties to act on)
    same_as: Dict[int, int] = field(default_factory=dict)   # item -> the item whose logits it repeats
    no_timestamps: bool = False
    note: str = ""

    @property
    def V(self) -> int:
        return VOCAB[self.vocab]

    @property
    def ids(self) -> odec.TokenIds:
        return token_ids(self.V)

    @property
    def items(self) -> int:
        return len(self.plens)

    @property
    def prompts(self) -> List[List[int]]:
        return [prompt_of(self.ids, n, self.no_timestamps) for n in self.plens]

    @property
    def steps(self) -> int:
        return self.kw["max_length"] - min(self.plens)

    @property
    def gen_kw(self) -> dict:
        """keyword arguments of Slot.debug_search / debug_search_batch and of GenOptions (plus ids)"""
        return dict(self.kw, suppress_tokens=suppress_list(self.ids))

    def opts(self) -> odec.GenOptions:
        return odec.GenOptions(ids=self.ids, **self.gen_kw)

    def logits(self) -> np.ndarray:
        ids, V, R = self.ids, self.V, self.R
        rows = self.items * R
        rng = np.random.default_rng(self.seed)
        lg = rng.standard_normal((self.steps, rows, V), dtype=np.float32) * np.float32(self.peaky)
        if self.kind == "quant":
            # tests/test_gpu_lean_family.py test_search_on_injected_logits_full_vocabulary: a coarse grid (equal values inside every row, broken
            # by the smaller id), the best candidates planted in one lane of one scan chunk and as neighbours, nearly empty chunks
            lg = np.round(lg * 4.0) / 4.0
            tb = ids.timestamp_begin
            for t in range(self.steps):
                base = int(rng.integers(1000, V - 9000)) if V > 12000 else int(rng.integers(10, tb // 4))
                lg[t, :, base:min(base + 4096, tb - 120):256] += 9.0
                lg[t, :, base + 7:base + 19] += 8.75
            if self.steps > 7:
                lg[5:7, :, (3000 if V > 12000 else 300):ids.eot - 200] = -np.inf
        lg[:, :, ids.timestamp_begin:] += 2.0
        if self.fav > 0:
            lg[:, :, [31, 57, 123, 300, 411, 640]] += np.float32(self.fav)
        for b in range(self.items):
            boost = self.eot[b % len(self.eot)]
            lg[:, b * R:(b + 1) * R, ids.eot] += np.float32(boost)
        for b, src in self.same_as.items():
            lg[:, b * R:(b + 1) * R] = lg[:, src * R:(src + 1) * R]
        return lg

    def item_logits(self, lg: np.ndarray, b: int) -> np.ndarray:
        return np.ascontiguousarray(lg[:, b * self.R:(b + 1) * self.R])


def _beam_kw(beam, L, **more):
    return dict(dict(beam_size=beam, patience=1.0, max_length=L, length_penalty=1.0), **more)


NEVER = -25.0      # end-of-text boost of an item that must run into its step budget
EARLY = 40.0       # ... of an item whose every row ends the moment end-of-text is allowed (the second step)
_L = {"micro": 9 + 10, "full": 9 + 6}        # max_length of the batched cases: prompts of 1 / 4 / 9 tokens -> 18 / 15 / 10 (14 / 11 / 6) steps


# a case whose first seed left two deciding scores closer than MARGIN got another one (scanned upwards in steps of 100)
_RESEED: Dict[str, int] = {'beam6-quant-full': 2106, 'beam7-gauss-full': 1107, 'beam8-quant-full': 2108, 'beam9-quant-full': 2209, 'beam12-gauss-full': 1212, 'beam12-quant-full': 2212, 'beam12-initial-ts5-full': 3112, 'beam9-no-timestamps-full': 3109, 'batch2x5-full': 4125, 'batch5x5-full': 4355, 'batch2x16-full': 4136,
                          'beam16-patience2-full': 4216, 'beam16-patience2-micro': 4716, 'beam6-gauss-micro': 1206, 'beam7-quant-micro': 2207, 'beam8-gauss-micro': 1308, 'beam8-quant-micro': 2108, 'beam9-gauss-micro': 1109, 'beam9-quant-micro': 2109, 'beam12-gauss-micro': 1112, 'beam12-quant-micro': 2312, 'beam16-gauss-micro': 2416, 'beam16-quant-micro': 4316, 'beam12-initial-ts5-micro': 3212, 'beam9-no-timestamps-micro': 4009, 'batch2x5-micro': 4125, 'batch3x5-micro': 4135, 'batch5x5-micro': 4355, 'batch2x16-micro': 5136, 'batch3x5-repetition-penalty': 6101, 'batch3x5-no-repeat-ngram': 6202, 'batch3x5-length-penalty0': 6103}


def _cases() -> Dict[str, Case]:
    out: List[Case] = []
    for vocab in ("micro", "full"):
        L1 = 1 + (24 if vocab == "micro" else 12)
        # ---- a. one item, beam widths 6 .. 16
        for beam in (6, 7, 8, 9, 12, 16):
            out.append(Case(f"beam{beam}-gauss-{vocab}", vocab, beam, [1], _beam_kw(beam, L1), seed=1000 + beam))
            out.append(Case(f"beam{beam}-quant-{vocab}", vocab, beam, [1], _beam_kw(beam, L1), seed=2000 + beam, kind="quant", peaky=3.0,
                            eot=(5.0 if beam % 2 else 0.0,)))
        out.append(Case(f"beam16-patience2-{vocab}", vocab, 16, [1], _beam_kw(16, L1 + (4 if vocab == "micro" else 3), patience=2.0, num_hypotheses=16),
                        seed=3016, eot=(13.0 if vocab == "micro" else 22.0,), peaky=6.0, note="32 finished hypotheses: the whole store"))
        out.append(Case(f"beam12-initial-ts5-{vocab}", vocab, 12, [1], _beam_kw(12, L1, max_initial_timestamp_index=5), seed=3012,
                        note="six allowed ids at the first step: exhausted candidate lists"))
        out.append(Case(f"beam9-no-timestamps-{vocab}", vocab, 9, [2], _beam_kw(9, L1 + 1), seed=3009, no_timestamps=True))
        # ---- b. several items in one call: prompt lengths 1 / 4 / 9, an item that runs into the step budget, one that ends at the second step
        L = _L[vocab]
        for items, beam in ((2, 5), (3, 5), (5, 5), (3, 8), (2, 16)):
            plens = [1, 4, 9, 4, 1][:items]
            out.append(Case(f"batch{items}x{beam}-{vocab}", vocab, beam, plens, _beam_kw(beam, L), seed=4000 + 10 * items + beam,
                            eot=(NEVER, EARLY, 7.0, 5.0, 8.0)))
        # ---- c. sampling / greedy rows
        Ls = 1 + (20 if vocab == "micro" else 11)
        samp = dict(beam_size=1, num_hypotheses=5, sampling_temperature=0.6, sampling_topk=0, max_length=Ls + 3, seed=1234)
        se = (6.0, 3.0, 7.0) if vocab == "micro" else (13.0, 11.0, 14.0)      # (the full vocabulary's best of 50 k text ids sits near 4.3 sigma)
        out.append(Case(f"sample3x5-{vocab}", vocab, 5, [1, 1, 4], samp, seed=5001, peaky=3.0, eot=se[:1], same_as={1: 0}))
        out.append(Case(f"sample3x5-topk1-{vocab}", vocab, 5, [1, 1, 4], dict(samp, sampling_topk=1), seed=5002, peaky=3.0, eot=se))
        out.append(Case(f"greedy4-{vocab}", vocab, 1, [1, 4, 9, 2], dict(beam_size=1, max_length=L), seed=5003, peaky=3.0, eot=(NEVER, EARLY, 6.0, 4.0)))
    # ---- b. options, three items of five beams (micro: the rules do not depend on the vocabulary)
    L = _L["micro"]
    eo = (NEVER, EARLY, 6.0)
    out.append(Case("batch3x5-repetition-penalty", "micro", 5, [1, 4, 9], _beam_kw(5, L, repetition_penalty=1.3), seed=6001, eot=eo, fav=7.0, peaky=2.0))
    out.append(Case("batch3x5-no-repeat-ngram", "micro", 5, [1, 4, 9], _beam_kw(5, L, no_repeat_ngram_size=2), seed=6002, eot=eo, fav=7.0, peaky=2.0))
    out.append(Case("batch3x5-length-penalty0", "micro", 5, [1, 4, 9], _beam_kw(5, L, length_penalty=0.0, num_hypotheses=3), seed=6003, eot=(NEVER, EARLY, 4.0)))
    out.append(Case("batch3x5-keep-blank", "micro", 5, [1, 4, 9], _beam_kw(5, L, suppress_blank=False), seed=6004, eot=eo))
    # ---- the open question of the hypothesis store: round(16 * 2.5) = 40 hypotheses asked for, 32 slots
    out.append(Case("beam16-patience2.5-micro", "micro", 16, [1], _beam_kw(16, 1 + 30, patience=2.5, num_hypotheses=16), seed=9016, eot=(9.0,)))
    for c in out:
        c.seed = _RESEED.get(c.name, c.seed)
    return {c.name: c for c in out}


CASES: Dict[str, Case] = _cases()


@dataclass
class Answer:
    results: List[odec.GenResult]            # per item
    margin: float                            # the smallest decisive score difference of the case (inf: none decisive)
    where: str                               # what that difference is between
    n_hyps: List[int]                        # finished hypotheses per item (beam mode)
    max_new: List[int]                       # step budget per item


class _Watch:
    """Observer of odec.generate: the smallest difference between two scores whose order decides the result, whenever the two come from
    DIFFERENT beam rows (inside one row the candidates are ordered by value and id, ties included: the value-desc / id-asc rule)."""

    def __init__(self, beam: int, num_hyp: int, eot: int):
        self.B, self.NH, self.eot = beam, num_hyp, eot
        self.margin, self.where, self.n_hyps = float("inf"), "", 0

    def _pair(self, a, c, what):
        if a[1] == c[1] or not (np.isfinite(a[0]) or np.isfinite(c[0])):
            return
        d = float(abs(np.float64(a[0]) - np.float64(c[0]))) if np.isfinite(a[0]) and np.isfinite(c[0]) else float("inf")
        if d < self.margin:
            self.margin, self.where = d, what

    def __call__(self, ev):
        if "hyps" in ev:
            self.n_hyps = len(ev["hyps"])
            sc = sorted((s for s, _ in ev["hyps"] if np.isfinite(s)), reverse=True)[: self.NH + 1]
            for i in range(len(sc) - 1):                       # the order of the hypotheses returned, and the first one left out
                if sc[i] == sc[i + 1]:                         # bit-equal: the same parent row and equal logits, ordered by id on both sides
                    continue
                if sc[i] - sc[i + 1] < self.margin:
                    self.margin, self.where = float(sc[i] - sc[i + 1]), f"finished hypotheses {i} / {i + 1}"
            return
        B, cands, step, last = self.B, ev["cands"], ev["step"], ev["is_last"]
        nc = 2 * B
        if len(cands) > nc:
            self._pair(cands[nc - 1], cands[nc], f"step {step}: last merged candidate / first rejected")
        fin = [last or c[3] == self.eot for c in cands[: nc + 1]]
        if fin[B - 1] or fin[B]:
            self._pair(cands[B - 1], cands[B], f"step {step}: last candidate that may finish / the next")
        act = [k for k in range(min(nc, len(cands))) if not fin[k]]
        for i in range(min(B, len(act) - 1)):                  # the order of the beams that go on (their row = their logits), and the first one left out
            self._pair(cands[act[i]], cands[act[i + 1]], f"step {step}: continuing beams {i} / {i + 1}")


@functools.lru_cache(maxsize=None)
def answer(name: str) -> Answer:
    """the oracle's results for every item of a case, with the separation of its decisions"""
    c = CASES[name]
    lg = c.logits()
    o = c.opts()
    beam_mode = not (o.sampling_temperature > 0 or o.beam_size <= 1)
    res, margin, where, nh, mn = [], float("inf"), "", [], []
    for b, prompt in enumerate(c.prompts):
        w = _Watch(c.R, max(1, o.num_hypotheses), c.ids.eot) if beam_mode else None
        res.append(odec.generate(odec.InjectedLogits(c.item_logits(lg, b)), prompt, o, row_base=b * c.R, observer=w))
        mn.append(o.max_length - len(prompt))
        if w is not None:
            nh.append(w.n_hyps)
            if w.margin < margin:
                margin, where = w.margin, f"item {b}, {w.where}"
    return Answer(res, margin, where, nh, mn)


def first_step_allowed(name: str, item: int = 0) -> int:
    """how many ids the rules leave at an item's first step"""
    c = CASES[name]
    row = c.logits()[0, item * c.R]
    v, _, _ = odec.process_logits(row, [], c.opts(), c.ids.no_timestamps not in c.prompts[item])
    return int(np.isfinite(v).sum())
