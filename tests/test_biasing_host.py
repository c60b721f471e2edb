"""CPU tests of keyword boosting's host side (whisperlive_amd/biasing.py): the compiled automaton against a brute-force "longest suffix
that is a phrase prefix" walk, the caps, the C-ABI bindings against include/wlx.h, the thread-local scope of WhisperModelHIP.keyword_bias
on the scripted engine of tests/fakes.py, and the parsing of the REST form fields and the WebSocket options."""
import ctypes as C
import os
import re
import threading
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd import biasing as B
from whisperlive_amd.tokenizer import Tokenizer, synthetic_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 2310
TOK = Tokenizer(synthetic_tokenizer(V), False)
EOT = TOK.eot


# ---- the brute-force restatement: the state is a token tuple
def brute_next(phrases, state, token, eot):
    if token >= eot:
        return ()
    prefixes = {p[:k] for p in phrases for k in range(1, len(p) + 1)}
    seq = tuple(state) + (token,)
    if tuple(state) in set(phrases):           # a phrase ended here: the walk restarts, but a longer phrase it begins still grows
        cands = [seq, (token,)]
    else:
        cands = [seq[k:] for k in range(len(seq))]
    return next((c for c in cands if c in prefixes), ())


def brute_boosted(phrases, state, eot, vocab_tokens):
    return sorted(t for t in vocab_tokens if brute_next(phrases, state, t, eot) != ())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_automaton_equals_the_brute_force_walk_on_random_streams(seed):
    rng = np.random.default_rng(seed)
    alphabet = [5, 6, 7, 8]
    phrases = []
    for _ in range(12):
        p = tuple(int(x) for x in rng.choice(alphabet, size=int(rng.integers(1, 6))))
        if p not in phrases:
            phrases.append(p)
    t = B.compile_bias([list(p) for p in phrases], 0.5, vocab=V, eot=EOT)
    assert t.phrases == phrases
    state, bstate = 0, ()
    stream = [int(x) for x in rng.choice(alphabet + [9, EOT, EOT + 40], size=600, p=[0.22, 0.22, 0.22, 0.22, 0.06, 0.03, 0.03])]
    for tok in stream:
        state, bstate = t.next_state(state, tok), brute_next(phrases, bstate, tok, EOT)
        assert t.paths[state] == bstate, (tok, t.paths[state], bstate)
        assert t.edges(state)[0].tolist() == brute_boosted(phrases, bstate, EOT, alphabet + [9])
        tok_, nxt = t.edges(state)
        assert (np.diff(tok_) > 0).all() and ((nxt >= 1) & (nxt < t.n_nodes)).all()
        s2, delta = t.apply(0, tok)
        assert s2 == t.next_state(0, tok) and delta.dtype == np.float32 and delta.shape == (V,)
        assert sorted(np.nonzero(delta)[0].tolist()) == t.edges(s2)[0].tolist()


def test_overlap_prefix_duplicate_and_reset_cases():
    a, b, c, d = 11, 12, 13, 14
    t = B.compile_bias([[a, b, c], [b, d]], 2.0, vocab=V, eot=EOT)
    s = 0
    for tok in (a, b, d):                       # history a b d completes `b d` through the failure link of `a b`
        s = t.next_state(s, tok)
    assert t.paths[s] == (b, d) and t.terminal[s]
    assert t.edges(t.paths.index((a, b)))[0].tolist() == sorted([c, d, a, b])
    assert t.edges(s)[0].tolist() == t.edges(0)[0].tolist() == [a, b]         # a phrase end behaves like the root
    # a phrase that is a prefix of another: it ends (root's edges) and the longer one still completes
    t = B.compile_bias([[a, b], [a, b, c]], 2.0, vocab=V, eot=EOT)
    ab = t.paths.index((a, b))
    assert t.terminal[ab] and t.edges(ab)[0].tolist() == [a, c] and t.paths[t.next_state(ab, c)] == (a, b, c)
    # duplicates are dropped; a string is encoded with and without the leading space
    t = B.compile_bias([[a, b], [a, b], "hello", " hello "], 2.0, tokenizer=TOK, vocab=V)
    sp, ns = tuple(TOK.encode(" hello")), tuple(TOK.encode("hello"))
    assert t.phrases == [(a, b)] + ([sp] if sp == ns else [sp, ns]) and t.eot == EOT
    # a special or a timestamp resets every state and is never an edge
    t = B.compile_bias([[a, b, c]], 2.0, vocab=V, eot=EOT)
    ab = t.paths.index((a, b))
    assert t.next_state(ab, EOT) == 0 and t.next_state(ab, TOK.timestamp_begin + 7) == 0 and t.next_state(ab, c) != 0
    assert (t.edge_tok < EOT).all()
    # logit_bias applies in every state, after the boost, as one float32 add each
    t = B.compile_bias([[a, b]], 0.5, {b: 2.0, "7": -4.0}, vocab=V, eot=EOT)
    row = np.zeros(V, np.float32)
    t.bias_row(row, t.paths.index((a,)))
    assert row[b] == 2.5 and row[7] == -4.0 and row[a] == 0.5 and np.count_nonzero(row) == 3
    assert B.compile_bias([], None, {}, vocab=V, eot=EOT).empty and float(B.compile_bias([[a]], None, vocab=V, eot=EOT).boost) == B.DEFAULT_BOOST


def test_every_cap_and_every_non_finite_value_raises():
    ok = dict(vocab=V, eot=EOT)
    with pytest.raises(ValueError, match="4096 nodes"):
        B.compile_bias([[5] * 4096], 1.0, **ok)
    assert B.compile_bias([[5] * 4095], 1.0, **ok).n_nodes == 4096
    # the closure: every node that ends a phrase carries the root's edges, so 100 one-token phrases are 100 + 100 * 100 edges ...
    assert B.compile_bias([[20 + i] for i in range(100)], 1.0, **ok).n_edges == 100 + 100 * 100
    # ... and 256 root edges carried by 384 nodes are past the cap
    many = [[20 + i] for i in range(128)] + [[200 + i, 400 + i] for i in range(128)]
    with pytest.raises(ValueError, match="16384 edges"):
        B.compile_bias(many, 1.0, **ok)
    with pytest.raises(ValueError, match="1024 logit_bias"):
        B.compile_bias([], 1.0, {i: 0.5 for i in range(1025)}, **ok)
    B.compile_bias([], 1.0, {i: 0.5 for i in range(1024)}, **ok)
    for bad in ([[V]], [[-1]], [[EOT]], [[TOK.timestamp_begin]], [[]], [""], ["  "], [[1.5]], [None], "one string"):
        with pytest.raises(ValueError):
            B.compile_bias(bad, 1.0, tokenizer=TOK, **ok)
    for bad in ({V: 1.0}, {-1: 1.0}, {3: float("nan")}, {3: float("inf")}, {3: 1e39}, {3: "x"}, {"x": 1.0}, {3: True}, {3: 1.0, "3": 2.0}):
        with pytest.raises(ValueError):
            B.compile_bias([], 1.0, bad, **ok)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, "2", True):
        with pytest.raises(ValueError):
            B.compile_bias([[5]], bad, **ok)
    with pytest.raises(ValueError):
        B.compile_bias(["text"], 1.0, **ok)                                    # text without a tokenizer
    with pytest.raises(ValueError):
        B.compile_bias([[5]], 1.0)                                             # no vocabulary


def test_bindings_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlx.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(wlx_(?:debug_)?bias_[a-z_]+)\s*\(", src))) == ["wlx_bias_clear", "wlx_bias_set", "wlx_debug_bias_apply"]
    for name, const in (("WLX_BIAS_MAX_NODES", _lib.BIAS_MAX_NODES), ("WLX_BIAS_MAX_EDGES", _lib.BIAS_MAX_EDGES), ("WLX_BIAS_MAX_TOKENS", _lib.BIAS_MAX_TOKENS)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == const
    _lib.build()
    lib = _lib.load()
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    i32p, f32p, i16p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int16)
    ctype = {"wlx_engine*": vp, "int32_t": i32, "int64_t": i64, "float": f32, "const int32_t*": i32p, "const float*": f32p, "float*": f32p,
             "const int16_t*": i16p, "int16_t*": i16p}
    for name in ("wlx_bias_set", "wlx_bias_clear", "wlx_debug_bias_apply"):
        args = re.search(rf"int32_t {name}\((.*?)\);", src, flags=re.S).group(1)
        types = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in args.split(",")]
        assert getattr(lib, name).argtypes == types, name
        assert getattr(lib, name).restype is i32 and name in _lib.EXPORTS
    # refused without a device: a null engine
    assert lib.wlx_bias_clear(None, 0) == _lib.ERR_ARG and lib.wlx_bias_set(None, 0, 1, None, None, None, 1.0, 0, None, None) == _lib.ERR_ARG


class BiasSlot(FakeSlot):
    def set_bias(self, table):
        self.calls.append(("set_bias", table))

    def clear_bias(self):
        self.calls.append(("clear_bias",))


class BiasEngine(FakeEngine):
    slot_type = BiasSlot


def _model(engine):
    from whisperlive_amd.transcriber import WhisperModelHIP
    return WhisperModelHIP("fake", engine=engine, hf_tokenizer=synthetic_tokenizer(V))


def test_keyword_bias_is_scoped_to_the_calling_thread():
    eng = BiasEngine()
    eng.default_tokens = [50, 51]
    m = _model(eng)
    pcm = np.zeros(16000, np.float32)
    kw = dict(language="en", temperature=0.0, vad_filter=False)
    gate, seen, errs = threading.Barrier(2), {}, []

    def worker(name, phrase):
        try:
            with m.keyword_bias(phrases=[phrase], boost=0.5) as table:
                gate.wait(timeout=10)
                m.transcribe(pcm, **kw)
                gate.wait(timeout=10)
                m.transcribe(pcm, **kw)
                seen[name] = (table, m._slot())
            m.transcribe(pcm, **kw)                                  # outside: cleared
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=("a", [5, 6])), threading.Thread(target=worker, args=("b", [7, 8, 9]))]
    [t.start() for t in ts]
    [t.join(timeout=20) for t in ts]
    assert not errs, errs
    (ta, sa), (tb, sb) = seen["a"], seen["b"]
    assert sa is not sb and ta.phrases == [(5, 6)] and tb.phrases == [(7, 8, 9)]
    for table, slot in ((ta, sa), (tb, sb)):
        bias_calls = [c for c in slot.calls if c[0] in ("set_bias", "clear_bias")]
        assert bias_calls == [("set_bias", table), ("clear_bias",)], bias_calls      # installed once for two calls, then cleared
        names = [c[0] for c in slot.calls if c[0] in ("set_bias", "clear_bias", "generate")]
        assert names == ["set_bias", "generate", "generate", "clear_bias", "generate"]
    # the main thread never had a table: its slot is left alone; a refused table raises before the block
    # (the main thread takes over a slot one of the ended threads left: its history is that thread's, so count from here)
    mine = m._slot()
    n0 = len(mine.calls)
    m.transcribe(pcm, **kw)
    assert m._slot() is mine and not [c for c in mine.calls[n0:] if c[0] in ("set_bias", "clear_bias")]
    with pytest.raises(ValueError, match="vocabulary"):
        m.keyword_bias(phrases=[[V + 5]])
    # the arguments of transcribe are the same scope; nesting restores the outer table; a slot that cannot take a table is an error
    m.transcribe(pcm, **kw, keywords=[[5, 6]], keywords_boost=2.0)
    assert [c[0] for c in mine.calls[n0:] if c[0] in ("set_bias", "clear_bias")] == ["set_bias"]
    with m.keyword_bias(phrases=[[5]]) as outer:
        with m.keyword_bias(phrases=[[6]]):
            pass
        assert B.current() is outer
    assert B.current() is None
    plain = _model(FakeEngine())
    with plain.keyword_bias(phrases=[[5]]):
        with pytest.raises(RuntimeError, match="set_bias"):
            plain.transcribe(pcm, **kw)


def test_rest_fields_and_websocket_options():
    from whisperlive_amd import rest as R
    from whisperlive_amd.serve_client import ServeClientHIP, keyword_options
    m = _model(BiasEngine())
    assert R.keyword_scope(m, [], None) is None
    sc = R.keyword_scope(m, ["hello there", "acme"], "2.0")
    assert float(sc.table.boost) == 2.0 and tuple(TOK.encode(" acme")) in sc.table.phrases
    assert float(R.keyword_scope(m, ["acme"], None).table.boost) == B.DEFAULT_BOOST
    for kws, boost, word in ((["acme"], "nan", "keywords_boost"), (["acme"], "x", "keywords_boost"), (["acme"], "inf", "keywords_boost"),
                             ([], "2.0", "keywords_boost"), ([" "], None, "empty"), (["a" * 5000], None, "4096 nodes")):
        with pytest.raises(R._HttpError) as ei:
            R.keyword_scope(m, kws, boost)
        assert ei.value.status == 400 and word in ei.value.payload["error"], ei.value.payload
    with pytest.raises(R._HttpError):
        R.keyword_scope(object(), ["acme"], None)
    assert float(keyword_options(m, ["acme", "hello"], 0.5).table.boost) == 0.5
    for kws, boost in ((None, 1.0), ("acme", None), ([], None), ([""], None), ([3], None), (["acme"], "2"), (["acme"], float("nan")), (["acme"], True)):
        with pytest.raises(ValueError):
            keyword_options(m, kws, boost)
    # a session without the options is untouched; one with them holds its scope; a refused value ends it with the cap named
    sock = MagicMock()
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False)
    assert c._bias is None
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False, keywords=["acme"], keywords_boost=2.0)
    assert float(c._bias.table.boost) == 2.0
    sock = MagicMock()
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False, keywords=["a" * 5000])
    assert not hasattr(c, "transcriber") and sock.close.called and "4096 nodes" in sock.send.call_args[0][0]
