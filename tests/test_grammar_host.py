"""CPU tests of grammar-constrained decoding's host side: whisperlive_amd/grammar.py (the compiled DFA against a brute-force enumeration of
the language, the named shapes, every refusal), tests/grammar_ref.py on hand-made tables, the C-ABI bindings against include/wlx_grammar.h,
csrc/grammar_table.h under the host sanitizers (tests/grammar_table_check.cpp), and the routes on the scripted engine of tests/fakes.py:
the thread's scope, transcribe(grammar=), the REST form fields, the session's first message and transcribe_many's one grammar."""
import ctypes as C
import itertools
import json
import os
import re
import shutil
import subprocess
import threading
from unittest.mock import MagicMock

import numpy as np
import pytest

from tests import grammar_ref as GR
from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd import grammar as G
from whisperlive_amd.tokenizer import Tokenizer, synthetic_tokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = next((c for c in (shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")) if c), None)
V = 2310
TOK = Tokenizer(synthetic_tokenizer(V), False)
EOT = TOK.eot


def compile_ids(phrases, repeat=True, vocab=V, eot=EOT):
    return G.compile_grammar(None, phrases, repeat, vocab=vocab, eot=eot)


def language(phrases, repeat, max_len):
    """brute force: every token string of at most max_len tokens that is a concatenation of phrases (one phrase or none without repeat)"""
    phrases = [tuple(p) for p in phrases]
    out = {()}
    if not repeat:
        return out | {p for p in phrases if len(p) <= max_len}
    frontier = {()}
    while frontier:
        new = {s + p for s in frontier for p in phrases if len(s + p) <= max_len} - out
        out |= new
        frontier = new
    return out


def check_table(g):
    assert g.edge_off[0] == 0 and np.all(np.diff(g.edge_off) >= 0) and g.edge_off[-1] == g.n_edges
    assert 1 <= g.n_states <= _lib.GRAMMAR_MAX_STATES and g.n_edges <= _lib.GRAMMAR_MAX_EDGES
    for n in range(g.n_states):
        tok, nxt = g.edges(n)
        assert np.all(np.diff(tok) > 0) and np.all((tok >= 0) & (tok < g.eot)) and np.all((nxt >= 0) & (nxt < g.n_states))
    assert set(g.accept.tolist()) <= {0, 1} and g.accept[0] == 1          # a silent window is an empty transcript
    for a in (g.edge_off, g.edge_tok, g.edge_next, g.accept):
        assert a.dtype == np.int32


NAMED = {
    "a / a b c / b d": [[11], [11, 12, 13], [12, 14]],
    "shared prefixes": [[20, 21, 22], [20, 21, 23], [20, 24], [25, 21, 22]],
    "a prefix of another": [[30, 31], [30, 31, 32, 33], [30]],
    "a phrase inside a repetition of another": [[40, 40], [40, 40, 40]],
    "the end of one is the start of another": [[50, 51], [51, 52], [51]],
}


@pytest.mark.parametrize("name", sorted(NAMED))
@pytest.mark.parametrize("repeat", [True, False])
def test_accepts_equals_the_brute_force_language(name, repeat):
    phrases = NAMED[name]
    g = compile_ids(phrases, repeat)
    check_table(g)
    assert g.repeat is repeat and g.phrases == [tuple(p) for p in phrases]
    alphabet = sorted({t for p in phrases for t in p}) + [99]            # (99: a token of no phrase)
    L = 6
    lang = language(phrases, repeat, L)
    for n in range(L + 1):
        for s in itertools.product(alphabet, repeat=n):
            assert G.accepts(g, s) == (s in lang), (name, repeat, s)


def test_the_device_never_prefers_the_longer_phrase():
    g = compile_ids(NAMED["a / a b c / b d"])
    assert G.accepts(g, [11, 12, 14]) and G.accepts(g, [11, 12, 13]) and G.accepts(g, [11, 11, 12, 14, 11])
    assert not G.accepts(g, [11, 12]) and not G.accepts(g, [12]) and not G.accepts(g, [13])
    # specials and timestamps are transparent, also in the middle of a phrase
    assert G.accepts(g, [EOT + 120, 11, EOT + 130, 12, 14, EOT + 140, EOT]) and not G.accepts(g, [11, EOT + 130, 12])
    once = compile_ids(NAMED["a / a b c / b d"], repeat=False)
    assert G.accepts(once, [11]) and G.accepts(once, [12, 14]) and G.accepts(once, []) and not G.accepts(once, [11, 12, 14])
    # without repeat a finished phrase that nothing continues is ONE state without edges: only end-of-text survives there
    ends = [n for n in range(once.n_states) if once.edge_off[n] == once.edge_off[n + 1]]
    assert len(ends) == 1 and once.accept[ends[0]] == 1


def test_a_thousand_one_token_phrases_are_one_state():
    g = compile_ids([[t] for t in range(300, 1300)], vocab=51865, eot=50257)
    check_table(g)
    assert g.n_states == 1 and g.n_edges == 1000 and np.all(g.edge_next == 0) and g.edge_tok.tolist() == list(range(300, 1300))
    once = compile_ids([[t] for t in range(300, 1300)], repeat=False, vocab=51865, eot=50257)
    assert once.n_states == 2 and once.n_edges == 1000 and np.all(once.edge_next == 1) and once.accept.tolist() == [1, 1]


def test_text_phrases_take_both_space_forms():
    g = G.compile_grammar(TOK, ["yes", "no", "operator please"], vocab=V)
    check_table(g)
    for text in ("yes", " yes", " operator please", "operator please", " no yes", " yes operator please no"):
        assert G.accepts(g, TOK.encode(text)), text
    assert not G.accepts(g, TOK.encode(" maybe")) and not G.accepts(g, TOK.encode(" operator"))
    assert g.eot == EOT and g.vocab == V


def test_every_refusal():
    for phrases, word in (([], "at least one phrase"), (None, "at least one phrase"), ([[]], "no tokens"),
                          ([[EOT]], "text tokens only"), ([[5, EOT + 200]], "text tokens only"), ([[V]], "vocabulary"), ([[-1]], "vocabulary"),
                          ("yes", "not one string"), ([[1.5]], "integers"), ([object()], "neither text")):
        with pytest.raises(ValueError, match=word):
            compile_ids(phrases)
    with pytest.raises(ValueError, match="needs a tokenizer"):
        compile_ids(["yes"])
    with pytest.raises(ValueError, match="empty phrase"):
        G.compile_grammar(TOK, ["yes", "  "], vocab=V)
    with pytest.raises(ValueError, match="vocabulary size"):
        G.compile_grammar(None, [[5]])
    # the limits are named: 4097 states (a chain of 4096 tokens behind the start state), 16385 edges (all of them out of the start state)
    with pytest.raises(ValueError, match="at most 4096 states"):
        compile_ids([[5 + (i % 7) for i in range(4097)]])
    assert compile_ids([[5 + (i % 7) for i in range(4096)]]).n_states == 4096
    with pytest.raises(ValueError, match="at most 16384 edges"):
        compile_ids([[t] for t in range(16385)], vocab=51865, eot=50257)
    assert compile_ids([[t] for t in range(16384)], vocab=51865, eot=50257).n_edges == 16384


def test_the_reference_walk_and_mask():
    g = compile_ids(NAMED["a / a b c / b d"])          # states: 0 start, 1 after a, 2 after b, 3 after a b
    s_a, s_b = g.step(0, 11), g.step(0, 12)
    s_ab = g.step(s_a, 12)
    assert (s_a, s_b) != (0, 0) and g.accept[s_a] == 1 and g.accept[s_b] == 0 and g.step(s_ab, 14) == 0 and g.step(s_ab, 13) == 0
    plen = 3
    assert GR.next_state(g, s_a, 12, 2, plen) == 0                      # a prompt position: the start state
    assert GR.next_state(g, s_a, 12, 3, plen) == s_ab
    assert GR.next_state(g, s_a, EOT + 150, 3, plen) == s_a             # a timestamp keeps the parent's state
    assert GR.next_state(g, s_a, EOT, 3, plen) == s_a
    assert GR.next_state(g, s_a, 77, 3, plen) == 0                      # no edge: the start state
    assert GR.next_state(g, 4000, 11, 3, plen) == s_a                   # a state out of range counts as the start state
    assert GR.next_state(g, 0, 11, 0, 0) == 0                           # position 0 has no parent
    rng = np.random.default_rng(0)
    row = rng.standard_normal(V + 2).astype(np.float32)
    raw = row.view(np.uint32).copy()
    out = GR.mask_row(g, row.copy(), s_b).view(np.uint32)
    kept = np.ones(V + 2, bool)
    kept[:EOT + 1] = False
    kept[14] = True                                                     # the one edge of `b`; end-of-text is masked: the state does not accept
    assert np.array_equal(out[kept], raw[kept]) and np.all(out[~kept] == GR.NEG_INF)
    out = GR.mask_row(g, row.copy(), s_a).view(np.uint32)
    assert out[EOT] == raw[EOT] and out[11] == raw[11] and out[12] == raw[12] and out[13] == GR.NEG_INF
    lg = rng.standard_normal((3, V)).astype(np.float32)
    got, st = GR.apply(g, lg, [12, 12, EOT + 9], [3, 3, 3], [0, 1, 2], plen, [0, 1, 0], [s_a, s_a, s_b])
    assert st.tolist() == [s_ab, s_ab, s_b] and np.array_equal(got[1].view(np.uint32), lg[1].view(np.uint32))
    assert np.isneginf(got[0][:EOT + 1]).sum() == EOT + 1 - 2 and np.isneginf(got[2][:EOT + 1]).sum() == EOT


def test_bindings_match_the_header():
    text = open(os.path.join(ROOT, "include", "wlx_grammar.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(wlx_[a-z_0-9]+)\s*\(", src))) == sorted(_lib.EXPORTS_GRAMMAR)
    assert '#include "wlx_grammar.h"' in open(os.path.join(ROOT, "include", "wlx.h")).read()
    for name, const in (("WLX_GRAMMAR_MAX_STATES", _lib.GRAMMAR_MAX_STATES), ("WLX_GRAMMAR_MAX_EDGES", _lib.GRAMMAR_MAX_EDGES)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == const
    hdr = open(os.path.join(ROOT, "whisperlive_amd", "csrc", "grammar_table.h")).read()
    assert f"GRAMMAR_MAX_STATES = {_lib.GRAMMAR_MAX_STATES};" in hdr and f"GRAMMAR_MAX_EDGES = {_lib.GRAMMAR_MAX_EDGES};" in hdr
    assert "dec_grammar.hip" in _lib.SOURCES and "WLX_ABI_VERSION stays 1" in text
    _lib.build()
    lib = _lib.load()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    i32p, f32p, i16p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int16)
    ctype = {"wlx_engine*": vp, "int32_t": i32, "int64_t": i64, "const int32_t*": i32p, "float*": f32p, "const int16_t*": i16p, "int16_t*": i16p}
    for name in _lib.EXPORTS_GRAMMAR:
        args = re.search(rf"int32_t {name}\((.*?)\);", src, flags=re.S).group(1)
        types = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in args.split(",")]
        assert getattr(lib, name).argtypes == types, name
        assert getattr(lib, name).restype is i32
    assert lib.wlx_abi_version() == 1
    # refused without a device: a null engine
    assert lib.wlx_grammar_clear(None, 0) == _lib.ERR_ARG and lib.wlx_grammar_set(None, 0, 5, 1, None, None, None, None) == _lib.ERR_ARG


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_table_check_under_the_sanitizers(tmp_path):
    exe = tmp_path / "grammar_table_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "grammar_table_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr[-3000:])
    assert run.returncode == 0 and "grammar_table_check: 0 failures" in run.stdout, (run.stdout, run.stderr[-3000:])


# ---- the scripted engine
class GrammarSlot(FakeSlot):
    def set_grammar(self, grammar):
        self.calls.append(("set_grammar", grammar))

    def clear_grammar(self):
        self.calls.append(("clear_grammar",))

    def set_bias(self, table):
        self.calls.append(("set_bias", table))

    def clear_bias(self):
        self.calls.append(("clear_bias",))


class GrammarEngine(FakeEngine):
    slot_type = GrammarSlot


def _model(engine):
    from whisperlive_amd.transcriber import WhisperModelHIP
    return WhisperModelHIP("fake", engine=engine, hf_tokenizer=synthetic_tokenizer(V))


NAMES = ("set_grammar", "clear_grammar", "set_bias", "clear_bias", "generate")
PCM = np.zeros(16000, np.float32)
KW = dict(language="en", temperature=0.0, vad_filter=False)


def test_the_grammar_is_scoped_to_the_calling_thread():
    eng = GrammarEngine()
    eng.default_tokens = [50, 51]
    m = _model(eng)
    gate, seen, errs = threading.Barrier(2), {}, []

    def worker(name, phrase):
        try:
            with m.grammar(phrases=[phrase]) as g:
                gate.wait(timeout=10)
                m.transcribe(PCM, **KW)
                gate.wait(timeout=10)
                m.transcribe(PCM, **KW)
                seen[name] = (g, m._slot())
            m.transcribe(PCM, **KW)                                  # outside: cleared
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=("a", [55, 56])), threading.Thread(target=worker, args=("b", [57, 64, 65]))]
    [t.start() for t in ts]
    [t.join(timeout=20) for t in ts]
    assert not errs, errs
    (ga, sa), (gb, sb) = seen["a"], seen["b"]
    assert sa is not sb and ga.phrases == [(55, 56)] and gb.phrases == [(57, 64, 65)]
    for g, slot in ((ga, sa), (gb, sb)):
        calls = [c for c in slot.calls if c[0] in NAMES]
        assert [c[0] for c in calls] == ["set_grammar", "generate", "generate", "clear_grammar", "generate"] and calls[0][1] is g
    # the main thread never had a grammar: its slot is left alone (it takes over a slot an ended thread left: count from here)
    mine = m._slot()
    n0 = len(mine.calls)
    m.transcribe(PCM, **KW)
    assert [c[0] for c in mine.calls[n0:] if c[0] in NAMES] == ["generate"]
    # transcribe(grammar=, grammar_repeat=) is the same scope for one call
    m.transcribe(PCM, **KW, grammar=[[55], [56, 57]], grammar_repeat=False)
    calls = [c for c in mine.calls[n0:] if c[0] in NAMES]
    assert [c[0] for c in calls] == ["generate", "set_grammar", "generate"] and calls[1][1].repeat is False and calls[1][1].phrases == [(55,), (56, 57)]
    # one mode at a time: a keyword table after a grammar clears the grammar first, a grammar after a table replaces it
    m.transcribe(PCM, **KW, keywords=[[55, 56]])
    m.transcribe(PCM, **KW, grammar=[[55]])
    m.transcribe(PCM, **KW)
    assert [c[0] for c in mine.calls[n0:] if c[0] in NAMES][3:] == ["clear_grammar", "set_bias", "generate", "set_grammar", "generate", "clear_grammar", "generate"]
    # both at once is refused on the host, whichever way they meet; scopes nest; a refused list raises before the block
    with pytest.raises(ValueError, match="one of them"):
        m.transcribe(PCM, **KW, grammar=[[55]], keywords=[[56]])
    with m.keyword_bias(phrases=[[56]]):
        with m.grammar(phrases=[[55]]):
            with pytest.raises(ValueError, match="one of them"):
                m.transcribe(PCM, **KW)
    with m.grammar(phrases=[[55]]) as outer:
        with m.grammar(phrases=[[56]]):
            pass
        assert G.current() is outer
    assert G.current() is None
    with pytest.raises(ValueError, match="at least one phrase"):
        m.grammar(phrases=[])
    # a token the call suppresses cannot be a grammar token (a state whose every token is suppressed would have nothing left to emit)
    with pytest.raises(ValueError, match="suppresses"):
        m.transcribe(PCM, **KW, grammar=[[55], [56, 57]], suppress_tokens=[57])
    m.transcribe(PCM, **KW, grammar=[[55], [56, 57], [56, 64]], suppress_tokens=[57])          # (a state that keeps another token: 57 is merely unreachable)
    g = compile_ids([[55], [56, 57], [220]])
    assert g.dead_states([57]) == [g.step(0, 56)] and g.dead_states([55, 56]) == [] and g.dead_states([55, 56], blank=220) == [0]
    # a slot that cannot take a grammar is an error, never an unconstrained decode
    plain = _model(FakeEngine())
    with plain.grammar(phrases=[[55]]):
        with pytest.raises(RuntimeError, match="set_grammar"):
            plain.transcribe(PCM, **KW)


def test_the_rest_fields_reach_the_model():
    from tests.test_rest import FILE, ScriptedTranscriber, Served
    from whisperlive_amd import rest as R
    m = _model(GrammarEngine())
    assert R.grammar_scope(m, [], None) is None
    sc = R.grammar_scope(m, ["yes", "operator please"], "false")
    assert sc.grammar.repeat is False and tuple(TOK.encode(" operator please")) in sc.grammar.phrases and tuple(TOK.encode("yes")) in sc.grammar.phrases
    assert R.grammar_scope(m, ["yes"], None).grammar.repeat is True and R.grammar_scope(m, ["yes"], "true").grammar.repeat is True
    for phrases, repeat, kws, word in ((["yes"], "maybe", None, "grammar_repeat must be a boolean"), ([], "true", None, "grammar_repeat needs"),
                                       ([" "], None, None, "empty"), (["yes"], None, ["acme"], "cannot be combined with keywords"),
                                       (["a b c d e f g h " * 600], None, None, "4096 states")):
        with pytest.raises(R._HttpError) as ei:
            R.grammar_scope(m, phrases, repeat, kws)
        assert ei.value.status == 400 and word in ei.value.payload["error"], ei.value.payload
    with pytest.raises(R._HttpError):
        R.grammar_scope(object(), ["yes"], None)

    class Recording(ScriptedTranscriber):
        """what the request's thread decodes under while transcribe runs"""
        def grammar(self, phrases=None, repeat=True):
            return G.scope(G.compile_grammar(TOK, phrases, repeat, vocab=V))

        def transcribe(self, audio, **kw):
            self.under = G.current()
            return super().transcribe(audio, **kw)

    t = Recording()
    with Served(t) as s:
        st, _, body = s.post([FILE, ("grammar", "yes"), ("grammar", "no"), ("grammar[]", "operator please"), ("grammar_repeat", "false")])
        assert st == 200, body
        assert t.under is not None and t.under.repeat is False
        assert {tuple(TOK.encode(" " + p)) for p in ("yes", "no", "operator please")} <= set(t.under.phrases)
        t.under = "unset"
        st, _, body = s.post([FILE])
        assert st == 200 and t.under is None
        for fields, word in (([("grammar", "yes"), ("keywords", "acme")], "cannot be combined with keywords"),
                             ([("grammar", "yes"), ("stream", "true")], "cannot be combined with stream"),
                             ([("grammar_repeat", "true")], "grammar_repeat needs"), ([("grammar", "yes"), ("grammar_repeat", "2")], "boolean")):
            st, _, body = s.post([FILE] + fields)
            assert st == 400 and word in json.loads(body)["error"], body


def test_the_session_keys_reach_the_model():
    from whisperlive_amd.serve_client import ServeClientHIP, grammar_options
    eng = GrammarEngine()
    eng.default_tokens = [50, 51]
    m = _model(eng)
    assert grammar_options(m, ["yes", "no"], None).grammar.repeat is True and grammar_options(m, ["yes"], False).grammar.repeat is False
    for phrases, repeat, kws in ((None, True, None), ("yes", None, None), ([], None, None), ([""], None, None), ([3], None, None),
                                 (["yes"], "true", None), (["yes"], 1, None), (["yes"], None, ["acme"])):
        with pytest.raises(ValueError):
            grammar_options(m, phrases, repeat, kws)
    sock = MagicMock()
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False)
    assert c._grammar is None and c._bias is None
    c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False, grammar=["yes", "no"], grammar_repeat=False)
    assert c._grammar.grammar.repeat is False and c._bias is None
    # the session decodes on its own slot under its grammar, with or without a batch worker on the device
    slot = m._slot()
    n0 = len(slot.calls)
    worker = MagicMock()
    ServeClientHIP.BATCH_WORKERS[c.device_index] = worker
    try:
        c.transcribe_audio(PCM)
    finally:
        del ServeClientHIP.BATCH_WORKERS[c.device_index]
    calls = [x for x in slot.calls[n0:] if x[0] in NAMES]
    assert [x[0] for x in calls] == ["set_grammar", "generate"] and calls[0][1] is c._grammar.grammar and not worker.submit.called
    assert G.current() is None
    # a refused list ends the session with the limit named; so does a grammar next to keywords
    for kw, word in ((dict(grammar=["a b c d e f g h " * 600]), "4096 states"), (dict(grammar=["yes"], keywords=["acme"]), "keywords"),
                     (dict(grammar_repeat=True), "needs grammar")):
        sock = MagicMock()
        c = ServeClientHIP(sock, client_uid="u", model="x.en", transcriber=m, use_vad=False, start_thread=False, **kw)
        assert not hasattr(c, "transcriber") and sock.close.called and word in sock.send.call_args[0][0], sock.send.call_args
    # the server hands both keys of the first message to the session
    src = open(os.path.join(ROOT, "whisperlive_amd", "server.py")).read()
    assert src.count('grammar=options.get("grammar"), grammar_repeat=options.get("grammar_repeat")') == 2


def test_transcribe_many_takes_one_grammar_for_all_files():
    from whisperlive_amd import many_files as MF
    g = compile_ids([[55]])
    seen = []

    def job():
        for i in range(3):
            seen.append(G.current())
            yield i, [], None

    out = []
    for item in MF._under_grammar(job(), g):
        assert G.current() is None                                  # the scope is left before a file is handed out
        out.append(item[0])
    assert out == [0, 1, 2] and seen == [g, g, g] and G.current() is None
    src = open(os.path.join(ROOT, "whisperlive_amd", "many_files.py")).read()
    assert 'kwargs.pop("grammar", None)' in src and "_under_grammar(job, pipe.model.compile_grammar(grammar, grammar_repeat))" in src
