"""Scripted decode searches: injected logits that STEER the search (csrc/search.hip) into the corners of every token rule, instead of waiting
for a random walk to get there (tests/search_cases.py). Plain numpy, no GPU.

A case is a `script` (the ids boosted step by step), the generate options, a prompt and `expect`: "verbatim" (the script is legal: the best
hypothesis is the script) or None (some scripted id is illegal where it stands: the search must go elsewhere). Every row of a case has the same
logits, so the score of a hypothesis depends on its tokens only.

The first half of this file is the REFERENCE and does not import the oracle: `rules_f64` restates the logits processors in float64 from the
published definition (OpenAI whisper/decoding.py SuppressBlank, SuppressTokens, ApplyTimestampRules, and the CTranslate2 options listed in
SURVEY.md Appendix A.5), `score_f64` sums float64 log-probabilities, `violations` is a predicate on an output sequence alone. The second half
holds the cases and runs them through oracle/decoding.py; tests/test_search_scripts_host.py shows that the two statements agree and that every
deciding pair of scores of every case is more than `MARGIN` apart, tests/test_gpu_search_scripted.py runs the cases on the device.

Seeds are fixed; a seed whose case was not separated (or whose noise pushed a legal script off its path) was replaced, scanning upwards in steps
of 100 (`_RESEED`), the margin never widened."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

GAP = 10.0               # boost of the scripted id over unit noise: wins every step, and the scores stay well away from 0.0
FAR = -1.0e4             # "-inf-like": a finite logit whose exp underflows to 0 against anything in the row


# ====================================================================================================================== reference (no oracle)
def scripted_logits(script: Sequence[int], rows: int, V: int, ids, gap: float, seed: int, identical_rows: bool = True) -> np.ndarray:
    """[len(script) + 1, rows, V] float32: unit Gaussian noise, +gap on the scripted id of each step, +gap on end-of-text at the step after."""
    rng = np.random.default_rng(seed)
    S = len(script) + 1
    if identical_rows:
        lg = np.repeat(rng.standard_normal((S, 1, V), dtype=np.float32), rows, axis=1)
    else:
        lg = rng.standard_normal((S, rows, V), dtype=np.float32)
    for t, tok in enumerate(script):
        lg[t, :, tok] += np.float32(gap)
    lg[S - 1, :, ids.eot] += np.float32(gap)
    return np.ascontiguousarray(lg)


def _lse64(x: np.ndarray) -> float:
    x = x[np.isfinite(x)]
    if x.size == 0:
        return -np.inf
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def _rules(logits_row, history, opts, apply_ts):
    """(masked float64 logits, log-sum-exp, timestamp mass - best text log-probability or None where the mass rule has nothing to compare)"""
    ids = opts.ids
    v = np.asarray(logits_row, dtype=np.float64).copy()
    V = v.shape[0]
    history = [int(t) for t in history]
    n_gen = len(history)
    # 1. repetition penalty (CTranslate2 / CTRL): every id generated so far; a positive logit is divided, a negative one multiplied
    pen = float(opts.repetition_penalty)
    if pen != 1.0:
        for t in set(history):
            v[t] = v[t] * pen if v[t] < 0 else v[t] / pen
    # 2. no-repeat-ngram: an id that would complete an n-gram already in the history
    n = int(opts.no_repeat_ngram_size)
    if n > 0 and n_gen >= n - 1:
        prefix = tuple(history[n_gen - (n - 1):]) if n > 1 else ()
        for j in range(n_gen - n + 1):
            if tuple(history[j:j + n - 1]) == prefix:
                v[history[j + n - 1]] = -np.inf
    # 3. suppress_tokens
    for t in opts.suppress_tokens:
        if 0 <= t < V:
            v[t] = -np.inf
    # 4. suppress_blank: at the first generated position
    if n_gen == 0 and opts.suppress_blank:
        if ids.blank >= 0:
            v[ids.blank] = -np.inf
        v[ids.eot] = -np.inf
    mass_gap = None
    # 5. timestamp rules (OpenAI ApplyTimestampRules)
    if apply_ts:
        tb = ids.timestamp_begin
        v[ids.no_timestamps] = -np.inf
        last_ts = n_gen >= 1 and history[-1] >= tb
        before_ts = n_gen < 2 or history[-2] >= tb
        if last_ts:
            if before_ts:
                v[tb:] = -np.inf            # a pair is closed (or the opening timestamp stands alone): text or the end must follow
            else:
                v[:ids.eot] = -np.inf       # one timestamp after text: its partner or the end must follow
        stamps = [t for t in history if t >= tb]
        if stamps:
            floor = stamps[-1] if (last_ts and not before_ts) else stamps[-1] + 1      # may repeat only to close its pair
            v[tb:floor] = -np.inf
        if n_gen == 0:
            v[:tb] = -np.inf
            if opts.max_initial_timestamp_index is not None and opts.max_initial_timestamp_index >= 0:
                v[tb + opts.max_initial_timestamp_index + 1:] = -np.inf
        # 6. if the probability mass on timestamps exceeds every single text token, it is a timestamp
        logp = v - _lse64(v)
        ts_mass = _lse64(logp[tb:])
        best_text = logp[:tb].max() if tb > 0 else -np.inf
        if np.isfinite(ts_mass) and np.isfinite(best_text):
            mass_gap = float(ts_mass - best_text)
        if ts_mass > best_text:
            v[:tb] = -np.inf
    return v, _lse64(v), mass_gap


def rules_f64(logits_row, history, opts, apply_ts) -> Tuple[np.ndarray, float]:
    """The logits processors on one row after `history` (the ids generated so far), float64: masked logits and their log-sum-exp."""
    v, lse, _ = _rules(logits_row, history, opts, apply_ts)
    return v, lse


def score_f64(tokens: Sequence[int], ended_on_eot: bool, logits: np.ndarray, opts, apply_ts: bool = True) -> float:
    """Sum of the float64 log-softmax of each emitted token (and of end-of-text where the hypothesis ended on it) / max(len, 1) ** length_penalty.
    `logits` is [steps, V]: the one row every beam sees (identical rows only)."""
    total = 0.0
    seq = list(tokens) + ([opts.ids.eot] if ended_on_eot else [])
    for t, tok in enumerate(seq):
        v, lse = rules_f64(logits[t], seq[:t], opts, apply_ts)
        total += v[tok] - lse
    return float(total / max(len(tokens), 1) ** float(opts.length_penalty))


def violations(tokens: Sequence[int], ids, opts, apply_ts: bool) -> List[str]:
    """What an OUTPUT sequence (prompt and end-of-text excluded) breaks; needs neither logits nor oracle."""
    out = []
    toks = [int(t) for t in tokens]
    tb = ids.timestamp_begin
    is_ts = [t >= tb for t in toks]
    sup = set(int(t) for t in opts.suppress_tokens)
    for i, t in enumerate(toks):
        if t in sup:
            out.append(f"suppressed id {t} at {i}")
    if toks and opts.suppress_blank and toks[0] in (ids.blank, ids.eot):
        out.append(f"blank or end-of-text first ({toks[0]})")
    n = int(opts.no_repeat_ngram_size)
    if n > 0:
        seen = {}
        for i in range(len(toks) - n + 1):
            g = tuple(toks[i:i + n])
            if g in seen:
                out.append(f"{n}-gram {g} at {seen[g]} repeated at {i}")
            seen.setdefault(g, i)
    if not apply_ts:
        return out
    if toks:
        if not is_ts[0]:
            out.append(f"first token {toks[0]} is not a timestamp")
        elif opts.max_initial_timestamp_index is not None and 0 <= opts.max_initial_timestamp_index < toks[0] - tb:
            out.append(f"first timestamp index {toks[0] - tb} past max_initial_timestamp_index {opts.max_initial_timestamp_index}")
    prev_ts = None
    for i, t in enumerate(toks):
        if t == ids.no_timestamps:
            out.append(f"<|notimestamps|> at {i}")
        if is_ts[i]:
            if prev_ts is not None and t < prev_ts:
                out.append(f"timestamp decreases at {i}: {t - tb} after {prev_ts - tb}")
            elif prev_ts is not None and t == prev_ts and not is_ts[i - 1]:
                out.append(f"timestamp at {i} not strictly greater after text: {t - tb}")
            if i >= 1 and is_ts[i - 1] and (i == 1 or is_ts[i - 2]):     # (nothing stands before the opening timestamp: it counts as closed)
                out.append(f"three timestamps in a row at {i}" if i >= 2 else "timestamp directly after the opening timestamp")
            prev_ts = t
        elif t < ids.eot and i >= 2 and is_ts[i - 1] and not is_ts[i - 2]:
            out.append(f"text at {i} after a single timestamp that follows text")
    return out


# ====================================================================================================================== cases (oracle side)
from oracle import decoding as odec                                             # noqa: E402
from tests.search_cases import MARGIN, VOCAB, _Watch, prompt_of, suppress_list, token_ids    # noqa: E402

# what float32 costs the oracle's scores against score_f64, largest over all cases and returned hypotheses (measured; the host test holds the
# cases to it), and what the device is allowed: 8 x that (it sums in another order and uses __expf / __logf), never more than the 1e-3 * max(1, |s|)
# of the random-logits tests
ORACLE_SCORE_ERR = 1.6e-6      # measured 1.58e-6 (finish-length-penalty0.0: a sum of three log-probabilities, not divided)
DEVICE_SCORE_TOL = 8 * ORACLE_SCORE_ERR


def device_tol(score: float) -> float:
    return min(DEVICE_SCORE_TOL, 1e-3 * max(1.0, abs(score)))


@dataclass
class Script:
    name: str
    vocab: str                                # "micro" | "full"
    script: List[int]
    expect: Optional[str]                     # "verbatim" | None
    kw: dict = field(default_factory=dict)    # generate options over beam 5 / patience 1 / length_penalty 1 (without ids / suppress_tokens / max_length)
    plen: int = 1
    no_timestamps: bool = False               # the prompt ends on <|notimestamps|>: timestamp rules off
    gap: float = GAP
    edits: Sequence[tuple] = ()               # changes to single steps of scripted_logits, see logits()
    max_length: Optional[int] = None          # default: plen + len(script) + 1 (the end-of-text step is the last one); plen + len(script): no end-of-text offered
    at: Dict[int, object] = field(default_factory=dict)   # position -> what the best hypothesis has there: an id, "ts", "text", or ("not", id)
    n_returned: Optional[int] = None          # hypotheses returned
    n_finished: Optional[int] = None          # hypotheses finished when the search stopped (seen on the oracle only)
    before: Optional[Tuple[List[int], List[int]]] = None  # the first sequence is returned ahead of the second
    seed: int = 0
    note: str = ""

    @property
    def V(self) -> int:
        return VOCAB[self.vocab]

    @property
    def ids(self) -> odec.TokenIds:
        return token_ids(self.V)

    @property
    def prompt(self) -> List[int]:
        return prompt_of(self.ids, self.plen, self.no_timestamps)

    @property
    def apply_ts(self) -> bool:
        return not self.no_timestamps

    @property
    def gen_kw(self) -> dict:
        d = dict(beam_size=5, patience=1.0, length_penalty=1.0)
        d.update(self.kw)
        d["max_length"] = self.max_length if self.max_length is not None else self.plen + len(self.script) + 1
        d["suppress_tokens"] = suppress_list(self.ids)
        return d

    def opts(self) -> odec.GenOptions:
        return odec.GenOptions(ids=self.ids, **self.gen_kw)

    @property
    def beam_mode(self) -> bool:
        k = self.gen_kw
        return not (k.get("sampling_temperature", 0.0) > 0 or k["beam_size"] <= 1)

    @property
    def R(self) -> int:
        k = self.gen_kw
        return k["beam_size"] if self.beam_mode else max(1, k.get("num_hypotheses", 1))

    @property
    def max_new(self) -> int:
        return self.gen_kw["max_length"] - self.plen

    def logits(self) -> np.ndarray:
        """scripted_logits, cut or padded to max_new steps (a padding step: noise with end-of-text far above everything, so whatever is still running
        ends there), then the edits of single steps:
          ("set", step, id, value)                  logit := value
          ("rel", step, id, ref, delta)             logit := logit of `ref` + delta
          ("shift", step, delta)                    every logit += delta (before a "set" in the same step: the set ids stand out of the rest)
          ("mass", step, text_id, value, first, count, delta)
                                                    text_id := value (the best text id); every timestamp := FAR, but `count` of them from index
                                                    `first` := value - log(count) + delta (spread by +-0.3 around it), so logsumexp(timestamps) - max(text) = delta"""
        ids, V, R = self.ids, self.V, self.R
        lg = scripted_logits(self.script, R, V, ids, self.gap, self.seed)
        S = self.max_new
        if S <= lg.shape[0]:
            lg = np.ascontiguousarray(lg[:S])
        else:
            pad = np.repeat(np.random.default_rng(self.seed + 1).standard_normal((S - lg.shape[0], 1, V), dtype=np.float32), R, axis=1)
            pad[:, :, ids.eot] += np.float32(25.0)
            lg = np.ascontiguousarray(np.concatenate([lg, pad], axis=0))
        for e in self.edits:
            kind, t = e[0], e[1]
            if kind == "set":
                lg[t, :, e[2]] = np.float32(e[3])
            elif kind == "rel":
                lg[t, :, e[2]] = lg[t, :, e[3]] + np.float32(e[4])
            elif kind == "shift":
                lg[t] += np.float32(e[2])
            elif kind == "mass":
                _, _, text_id, value, first, count, delta = e
                tb = ids.timestamp_begin
                lg[t, :, text_id] = np.float32(value)
                lg[t, :, tb:] = np.float32(FAR)
                off = np.linspace(0.3, -0.3, count)          # 0.015 between neighbours: no two beams tie; the mass stays what it was
                off -= np.log(np.exp(off).mean())
                lg[t, :, tb + first:tb + first + count] = (value - np.log(count) + delta + off).astype(np.float32)
            else:
                raise ValueError(kind)
        return lg


def _build() -> Dict[str, Script]:
    out: List[Script] = []
    add = out.append
    m = token_ids(VOCAB["micro"])
    tb, eot = m.timestamp_begin, m.eot

    def ts(i, base=tb):
        return base + i

    # ---------------------------------------------------------------- legal scripts: verbatim
    add(Script("legal-opener-text-pair-text-pair", "micro", [ts(0), 100, 101, ts(7), ts(7), 102, ts(20), ts(20)], "verbatim"))
    add(Script("legal-pair-text-pair-text-pair", "micro", [ts(0), 100, ts(7), ts(7), 101, 102, ts(20), ts(20), 103, ts(33), ts(33)], "verbatim"))
    add(Script("legal-last-timestamp-id", "micro", [ts(0), 100, ts(1500), ts(1500)], "verbatim"))
    for mi in (0, 5, 50):
        add(Script(f"legal-initial-ts-at-limit{mi}", "micro", [ts(mi), 100, ts(mi + 3), ts(mi + 3)], "verbatim", kw=dict(max_initial_timestamp_index=mi)))
    opener = [ts(0)] + [100 + i for i in range(9)]
    add(Script("legal-runs-into-max-length", "micro", opener, "verbatim", max_length=1 + len(opener), note="no end-of-text offered: the last step keeps its token"))
    add(Script("legal-one-token", "micro", [ts(0)], "verbatim"))
    add(Script("legal-long-prompt", "micro", [ts(2), 100, 101, ts(9), ts(9)], "verbatim", plen=9))

    # ---------------------------------------------------------------- illegal scripts: one id illegal where it stands
    add(Script("illegal-text-first", "micro", [100, 101, ts(5), ts(5)], None, at={0: "ts"}))
    add(Script("illegal-initial-ts-past-limit50", "micro", [ts(51), 100, ts(60), ts(60)], None, at={0: ("not", ts(51))}))
    add(Script("illegal-initial-ts-past-limit5", "micro", [ts(6), 100, ts(60), ts(60)], None, kw=dict(max_initial_timestamp_index=5), at={0: ("not", ts(6))}))
    add(Script("illegal-initial-ts-past-limit0", "micro", [ts(1), 100, ts(60), ts(60)], None, kw=dict(max_initial_timestamp_index=0), at={0: ts(0)}))
    add(Script("illegal-decreasing-timestamp", "micro", [ts(10), 100, ts(5), ts(5)], None, at={0: ts(10), 1: 100, 2: ("not", ts(5))}))
    add(Script("illegal-equal-timestamp-after-pair-and-text", "micro", [ts(0), 100, ts(7), ts(7), 101, ts(7), ts(7)], None,
               at={3: ts(7), 4: 101, 5: ("not", ts(7))}))
    add(Script("illegal-equal-timestamp-after-opener-and-text", "micro", [ts(4), 100, ts(4), ts(4)], None, at={1: 100, 2: ("not", ts(4))}))
    add(Script("illegal-third-timestamp", "micro", [ts(0), 100, ts(7), ts(7), ts(9), 101, ts(12), ts(12)], None, at={3: ts(7), 4: ("not", ts(9))}))
    add(Script("illegal-second-timestamp-at-once", "micro", [ts(0), ts(0), 100, ts(5), ts(5)], None, at={1: "text"}))
    add(Script("illegal-text-after-single-timestamp", "micro", [ts(0), 100, ts(7), 101, ts(9), ts(9)], None, at={2: ts(7), 3: ("not", 101)}))
    add(Script("illegal-notimestamps-scripted", "micro", [ts(0), m.no_timestamps, 100, ts(5), ts(5)], None, at={1: ("not", m.no_timestamps)}))
    add(Script("illegal-eot-first", "micro", [eot, 100, ts(5), ts(5)], None, at={0: "ts"}))
    add(Script("illegal-suppressed-id", "micro", [ts(0), 100, 14, 101, ts(5), ts(5)], None, at={1: 100, 2: ("not", 14)}))
    add(Script("illegal-suppressed-special", "micro", [ts(0), 100, tb - 5, 101, ts(5), ts(5)], None, at={2: ("not", tb - 5)}))

    # ---------------------------------------------------------------- the timestamp-mass rule, 0.05 either side of its threshold
    mass_script = [ts(0), 100, 101, ts(60), ts(60)]
    add(Script("mass-above-text-masked", "micro", mass_script, None, edits=[("mass", 2, 101, 12.0, 10, 40, +0.05)], at={2: "ts"}))
    add(Script("mass-below-text-kept", "micro", mass_script, "verbatim", edits=[("mass", 2, 101, 12.0, 10, 40, -0.05)], at={2: 101}))

    # ---------------------------------------------------------------- a <|notimestamps|> prompt: the same timestamp-heavy scripts, rules off
    nt = dict(no_timestamps=True, plen=2)
    add(Script("norules-text-first", "micro", [100, 101, ts(5), ts(5)], "verbatim", **nt))
    add(Script("norules-decreasing-and-triple", "micro", [ts(51), 100, ts(5), ts(5), ts(5), 101, ts(3)], "verbatim", **nt))
    add(Script("norules-notimestamps-scripted", "micro", [ts(1500), m.no_timestamps, 100], "verbatim", **nt))
    add(Script("norules-text-after-single-timestamp", "micro", [100, ts(7), 101, ts(7), ts(7), ts(7)], "verbatim", no_timestamps=True, plen=4))
    add(Script("norules-mass-above-text-kept", "micro", [100, 101, 102], "verbatim", edits=[("mass", 1, 101, 12.0, 10, 40, +0.05)], at={1: 101}, **nt))
    add(Script("norules-blank-first", "micro", [m.blank, 100, 101], None, at={0: ("not", m.blank)}, **nt))
    add(Script("norules-blank-first-kept", "micro", [m.blank, 100, 101], "verbatim", kw=dict(suppress_blank=False), **nt))
    add(Script("norules-eot-first", "micro", [eot, 100, 101], None, at={0: "text"}, **nt))

    # ---------------------------------------------------------------- no_repeat_ngram_size 1, 2, 3
    def ng(n):
        return dict(kw=dict(no_repeat_ngram_size=n), **nt)
    add(Script("ngram2-history-shorter", "micro", [100], "verbatim", **ng(2)))
    add(Script("ngram3-history-shorter", "micro", [100, 100, 100], "verbatim", **ng(3), note="ngen 1 < n - 1; at ngen 2 there is no earlier trigram"))
    add(Script("ngram1-repeat-masked", "micro", [100, 101, 100, 102], None, at={1: 101, 2: ("not", 100)}, **ng(1)))
    add(Script("ngram2-repeat-masked", "micro", [100, 101, 102, 100, 101, 103], None, at={3: 100, 4: ("not", 101)}, **ng(2)))
    add(Script("ngram3-repeat-masked", "micro", [100, 101, 102, 103, 100, 101, 102], None, at={5: 101, 6: ("not", 102)}, **ng(3)))
    add(Script("ngram3-fourth-equal-token-masked", "micro", [100, 100, 100, 100], None, at={2: 100, 3: ("not", 100)}, **ng(3)))
    add(Script("ngram3-only-last-token-matches", "micro", [100, 101, 102, 103, 101, 102, 104], "verbatim", **ng(3)))
    add(Script("ngram2-first-token-repeats", "micro", [100, 101, 100, 102], "verbatim", **ng(2)))
    add(Script("ngram3-repeat-spans-pair", "micro", [100, ts(5), ts(5), 101, 102, ts(5), ts(5), 101], None, at={6: ts(5), 7: ("not", 101)}, **ng(3)))
    add(Script("ngram1-closing-timestamp-masked", "micro", [ts(0), 100, ts(5), ts(5)], None, kw=dict(no_repeat_ngram_size=1), at={2: ts(5), 3: ("not", ts(5))},
               note="rules on: the partner of a pair is a repeated 1-gram"))
    add(Script("ngram2-repeat-spans-pair-rules-on", "micro", [ts(0), 100, ts(5), ts(5), 100, ts(5), ts(9)], None, kw=dict(no_repeat_ngram_size=2),
               at={4: 100, 5: ("not", ts(5))}))

    # ---------------------------------------------------------------- repetition_penalty 1.3 and 0.8 (values set by hand at the deciding step)
    rp = [100, 101, 100, 102]
    add(Script("penalty1.3-lead-removed", "micro", rp, None, kw=dict(repetition_penalty=1.3), edits=[("set", 2, 100, 10.0), ("set", 2, 150, 8.5)],
               at={2: 150}, note="10 / 1.3 = 7.69 < 8.5", **nt))
    add(Script("penalty1.0-lead-kept", "micro", rp, "verbatim", edits=[("set", 2, 100, 10.0), ("set", 2, 150, 8.5)], **nt))
    add(Script("penalty1.3-negative-made-worse", "micro", rp, None, kw=dict(repetition_penalty=1.3),
               edits=[("shift", 2, -12.0), ("set", 2, 100, -1.0), ("set", 2, 150, -1.2)], at={2: 150}, note="-1.0 * 1.3 = -1.3 < -1.2", **nt))
    add(Script("penalty1.0-negative-kept", "micro", rp, "verbatim", edits=[("shift", 2, -12.0), ("set", 2, 100, -1.0), ("set", 2, 150, -1.2)], **nt))
    add(Script("penalty0.8-promotes", "micro", rp, "verbatim", kw=dict(repetition_penalty=0.8), edits=[("set", 2, 100, 8.0), ("set", 2, 150, 9.0)],
               at={2: 100}, note="8 / 0.8 = 10 > 9", **nt))
    add(Script("penalty1.0-not-promoted", "micro", rp, None, edits=[("set", 2, 100, 8.0), ("set", 2, 150, 9.0)], at={2: 150}, **nt))
    add(Script("penalty1.3-rules-on-timestamp", "micro", [ts(0), 100, ts(5), ts(5), 101], None, kw=dict(repetition_penalty=1.3),
               edits=[("set", 3, ts(5), 10.0), ("set", 3, ts(6), 8.5)], at={2: ts(5), 3: ts(6)}, note="the partner of a pair is a repeated id too"))

    # ---------------------------------------------------------------- finishing
    # end-of-text 4 below the scripted id from the second step on: of all candidates that end, only the best beam's is among the top `beam`, so one
    # hypothesis (a prefix of the script) finishes per step and the count of finished hypotheses is the step number
    def one_per_step(n):
        return [("rel", t, eot, s, -4.0) for t, s in enumerate(fin_script[:n]) if t >= 1]
    fin_script = [ts(0)] + [100 + i for i in range(15)]
    for beam, pat, nh, stop in ((3, 1.5, 3, 5), (5, 0.5, 5, 3), (5, 2.5, 5, 13)):
        # stops after lround(beam * patience) = `stop` hypotheses (round-half-even would give stop - 1). Longer prefixes score higher (the -4 is divided
        # by the length), so the returned set shows the last step
        add(Script(f"finish-beam{beam}-patience{pat}", "micro", fin_script, None, kw=dict(beam_size=beam, patience=pat, num_hypotheses=nh),
                   edits=one_per_step(len(fin_script)), n_returned=min(nh, stop), n_finished=stop, before=(fin_script[:stop], fin_script[:stop - 1]),
                   note=f"{stop} finished hypotheses"))
    add(Script("finish-all-beams-in-one-step", "micro", [ts(0), 100, 101], "verbatim", kw=dict(num_hypotheses=5), edits=[("set", 3, eot, 30.0)], n_returned=5))
    lp_script = [ts(0), 100, 101, 102, 103, 104]
    for lp, first in ((0.0, "short"), (0.6, "long"), (2.0, "long")):
        a, b = lp_script[:2], lp_script
        add(Script(f"finish-length-penalty{lp}", "micro", lp_script, "verbatim" if first == "long" else None, kw=dict(length_penalty=lp, num_hypotheses=5),
                   edits=[("rel", 2, eot, 101, -0.5)], n_returned=5, before=(a, b) if first == "short" else (b, a),
                   note="a two-token hypothesis ends at the third step with the better sum; the full script ends later"))

    # ---------------------------------------------------------------- greedy and sampling rows (search_rows_kernel / search_update_kernel)
    by_name = {s.name: s for s in out}
    for base in ("legal-opener-text-pair-text-pair", "legal-last-timestamp-id", "legal-runs-into-max-length",
                 "illegal-equal-timestamp-after-pair-and-text", "illegal-third-timestamp", "illegal-text-after-single-timestamp",
                 "mass-above-text-masked", "mass-below-text-kept", "ngram2-repeat-masked", "penalty1.3-lead-removed"):
        s = by_name[base]
        for tag, more in (("greedy", dict(beam_size=1)), ("topk1", dict(beam_size=1, sampling_temperature=0.4, sampling_topk=1))):
            add(Script(f"{base}-{tag}", s.vocab, s.script, s.expect, kw=dict(s.kw, **more), plen=s.plen, no_timestamps=s.no_timestamps, edits=s.edits,
                       max_length=s.max_length, at=s.at))

    # ---------------------------------------------------------------- full vocabulary: 25 text chunks (the last one ragged: ids 49152 .. 50363) + 1 timestamp chunk
    f = token_ids(VOCAB["full"])
    ftb = f.timestamp_begin
    lo, hi = 300, 49152 + 700                 # a text id of the first chunk / of the ragged last text chunk
    fk = dict(vocab="full", gap=13.0)

    def fts(i):
        return ftb + i
    add(Script("full-legal-pairs", script=[fts(0), lo, hi, fts(7), fts(7), 2048 + 5, fts(1500), fts(1500)], expect="verbatim", **fk))
    add(Script("full-legal-initial-ts-at-limit5", script=[fts(5), hi, hi + 1, 20000, fts(6), fts(6)], expect="verbatim", kw=dict(max_initial_timestamp_index=5), plen=4, **fk))
    add(Script("full-illegal-equal-timestamp", script=[fts(0), hi, fts(7), fts(7), lo, fts(7), fts(7)], expect=None, at={4: lo, 5: ("not", fts(7))}, **fk))
    add(Script("full-illegal-text-after-single-timestamp", script=[fts(50), lo, fts(1499), hi, fts(1500), fts(1500)], expect=None, at={2: fts(1499), 3: ("not", hi)}, **fk))
    for where, tid in (("first-chunk", lo), ("last-text-chunk", hi)):
        sc = [fts(0), 30000, tid, fts(60), fts(60)]
        add(Script(f"full-mass-above-{where}", script=sc, expect=None, edits=[("mass", 2, tid, 16.0, 1461, 40, +0.05)], at={2: "ts"}, **fk))
        add(Script(f"full-mass-below-{where}", script=sc, expect="verbatim", edits=[("mass", 2, tid, 16.0, 1461, 40, -0.05)], at={2: tid}, **fk))

    # ---------------------------------------------------------------- the items of the batched call: one max_length, prompts of 1 / 4 / 9 tokens
    L = 9 + 9
    add(Script("batch-item-short", "micro", [ts(3), 100], "verbatim", plen=1, max_length=L, note="ends at the third of 17 steps"))
    add(Script("batch-item-illegal", "micro", [ts(0), 100, ts(7), ts(7), 101, ts(7), ts(7), 102, ts(30)], None, plen=4, max_length=L, at={5: ("not", ts(7))}))
    add(Script("batch-item-to-max-length", "micro", [ts(50), 100, 101, ts(60), ts(60), 102, 103, 104, 105], "verbatim", plen=9, max_length=L))

    for s in out:
        s.seed = _RESEED.get(s.name, 7000 + zlib.crc32(s.name.encode()) % 90)
    assert len({s.name for s in out}) == len(out)
    return {s.name: s for s in out}


BATCHES: Dict[str, List[str]] = {"batch-three-scripts": ["batch-item-short", "batch-item-illegal", "batch-item-to-max-length"]}

_RESEED: Dict[str, int] = {'legal-initial-ts-at-limit0': 7146, 'illegal-equal-timestamp-after-opener-and-text': 7187, 'illegal-third-timestamp': 7152, 'norules-eot-first': 7242,
                          'penalty1.0-negative-kept': 7140, 'penalty1.3-rules-on-timestamp': 7159, 'finish-length-penalty0.0': 7114, 'finish-length-penalty2.0': 7122,
                          'full-mass-above-last-text-chunk': 7236, 'full-mass-below-last-text-chunk': 7126}

SCRIPTS: Dict[str, Script] = _build()


class _Recorder(odec.LogitsProvider):
    """InjectedLogits that also keeps every row's history at every step (the rows the processors saw)."""

    def __init__(self, logits: np.ndarray):
        self.logits, self.i = logits, 0
        self.hist: List[List[int]] = []
        self.seen: List[Tuple[int, int, List[int]]] = []      # (step, row, history)

    def prefill(self, tokens):
        return None

    def step(self, tokens, parents):
        if self.i == 0:
            self.hist = [[] for _ in tokens]
        else:
            self.hist = [self.hist[p] + [int(t)] for p, t in zip(parents, tokens)]
        for r, h in enumerate(self.hist):
            self.seen.append((self.i, r, list(h)))
        out = self.logits[self.i][: len(tokens)]
        self.i += 1
        return out


@dataclass
class Answer:
    result: odec.GenResult
    margin: float                            # the smallest decisive score difference (inf: none decisive)
    where: str
    n_hyps: int                              # finished hypotheses (beam mode)
    seen: List[Tuple[int, int, List[int]]]   # (step, row, history) of every row the oracle processed


@functools.lru_cache(maxsize=None)
def answer(name: str) -> Answer:
    s = SCRIPTS[name]
    o = s.opts()
    rec = _Recorder(s.logits())
    w = _Watch(s.R, max(1, o.num_hypotheses), s.ids.eot) if s.beam_mode else None
    res = odec.generate(rec, s.prompt, o, observer=w)
    return Answer(res, w.margin if w else float("inf"), w.where if w else "", w.n_hyps if w else 0, rec.seen)


def ended_on_eot(s: Script, tokens: Sequence[int]) -> bool:
    """a hypothesis shorter than the step budget ended on end-of-text (the last step keeps its token unless that is end-of-text)"""
    return len(tokens) < s.max_new


def expectation_failures(s: Script, seqs: List[List[int]]) -> List[str]:
    """what the returned hypotheses (best first) miss of the case's `expect`, `at`, `n_returned` and `before`"""
    out = []
    if not seqs:
        return ["nothing returned"]
    best = seqs[0]
    tb = s.ids.timestamp_begin
    if s.expect == "verbatim" and best != list(s.script):
        out.append(f"best {best} is not the script {list(s.script)}")
    if s.expect is None and best == list(s.script):
        out.append("an illegal script came back verbatim")
    for pos, want in s.at.items():
        got = best[pos] if pos < len(best) else None
        ok = (got is not None and got >= tb) if want == "ts" else (got is not None and got < s.ids.eot) if want == "text" else \
            (got != want[1]) if isinstance(want, tuple) else (got == want)
        if not ok:
            out.append(f"position {pos}: {got}, wanted {want}")
    if s.n_returned is not None and len(seqs) != s.n_returned:
        out.append(f"{len(seqs)} hypotheses returned, wanted {s.n_returned}")
    if s.before is not None:
        a, b = list(s.before[0]), list(s.before[1])
        if a not in seqs or (b in seqs and seqs.index(b) < seqs.index(a)):
            out.append(f"{a} is not returned ahead of {b}: {seqs}")
    return out
