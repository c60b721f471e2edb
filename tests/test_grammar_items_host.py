"""No GPU: the host side of a grammar per item. GrammarSet packing against hand-made tables and its named refusals, the
C-ABI bindings against include/wlx_grammar_items.h, the pool check of csrc/grammar_pool.h under the host sanitizers (a stand-alone
program, tests/grammar_pool_check.cpp, run as a child process), and transcribe_many(grammars=...) on the scripted engine of
tests/fakes.py: one set per wave, a selection per decode group, a refused list costs only its file."""
import io
import json
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from tests.fakes import FrontEndEngine, FrontEndSlot
from tests.test_grammar_host import CXX, HERE, ROOT
from whisperlive_amd import _lib
from whisperlive_amd import grammar as G
from whisperlive_amd.batched import BatchedInferencePipeline
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP
from whisperlive_amd.vad import EnergyGateModel

V, EOT, SR = 2310, 2305, 16000


def compile_ids(phrases, repeat=True):
    return G.compile_grammar(None, phrases, repeat, vocab=V, eot=EOT)


def test_a_set_packs_its_grammars_back_to_back_and_names_its_limits():
    a, b, one = compile_ids([[11], [11, 12, 13], [12, 14]]), compile_ids([[7, 8]], repeat=False), compile_ids([[5]])
    s = G.GrammarSet([a, b])
    assert (s.add(a), s.add(compile_ids([[7, 8]], repeat=False)), s.add(one), s.add(b)) == (0, 1, 2, 1) and len(s) == 3 and s.version == 3
    ns, off, tok, nxt, acc = s.packed()
    assert all(x.dtype == np.int32 and x.flags.c_contiguous for x in (ns, off, tok, nxt, acc)) and (s.vocab, s.eot) == (V, EOT)
    assert ns.tolist() == [a.n_states, b.n_states, 1] and (s.n_states, s.n_edges) == (int(ns.sum()), tok.size)
    assert off.tolist() == a.edge_off.tolist() + b.edge_off.tolist() + [0, 1]          # local to each table: every run starts at 0
    assert tok.tolist() == a.edge_tok.tolist() + b.edge_tok.tolist() + [5] and nxt.tolist() == a.edge_next.tolist() + b.edge_next.tolist() + [0]
    assert acc.tolist() == a.accept.tolist() + b.accept.tolist() + [1] and s.index(one) == 2 and s.index(compile_ids([[6]])) is None
    # the limits: 1801 states a table, one state with 2300 - k edges, one-token tables
    for tables, word in (([compile_ids([[x, 1000 + x % 7, 2000 + k] for x in range(900)]) for k in range(10)], "16384 states in one set"),
                         ([compile_ids([[y] for y in range(k, 2300)]) for k in range(30)], "65536 edges in one set"),
                         ([compile_ids([[k + 1]]) for k in range(65)], "64 grammars in one set"),
                         ([one, G.compile_grammar(None, [[5]], vocab=V, eot=EOT - 1)], "one vocabulary"), ([one, [[5]]], "compiled grammars")):
        s = G.GrammarSet()
        with pytest.raises(ValueError, match=word):
            for t in tables:
                s.add(t)
        assert s.n_states <= _lib.GRAMMAR_SET_MAX_STATES and s.n_edges <= _lib.GRAMMAR_SET_MAX_EDGES and not s.fits(t) and s.fits(s.tables[0])


def test_bindings_match_the_header():
    main = open(os.path.join(ROOT, "include", "wlx.h")).read()
    assert '#include "wlx_grammar_items.h"' in main and int(re.search(r"#define WLX_ABI_VERSION (\d+)", main).group(1)) == 1
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlx_grammar_items.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(wlx_[a-z_0-9]+)\s*\(", src))) == sorted(_lib.EXPORTS_GRAMMAR_ITEMS)
    pool = open(os.path.join(ROOT, "whisperlive_amd", "csrc", "grammar_pool.h")).read()
    for name in ("GRAMMAR_SET_MAX_TABLES", "GRAMMAR_SET_MAX_STATES", "GRAMMAR_SET_MAX_EDGES"):
        const = getattr(_lib, name)
        assert int(re.search(rf"#define WLX_{name} (\d+)", src).group(1)) == const and f"{name} = {const};" in pool
    _lib.build()
    lib = _lib.load()
    for name in _lib.EXPORTS_GRAMMAR_ITEMS:         # as many arguments as the header declares; refused without a device: a null engine
        assert len(getattr(lib, name).argtypes) == re.search(rf"int32_t {name}\((.*?)\);", src, flags=re.S).group(1).count(",") + 1
    assert lib.wlx_grammar_select(None, 0, 1, None) == _lib.ERR_ARG and lib.wlx_grammar_set_items(None, 0, 5, 1, None, None, None, None, None) == _lib.ERR_ARG


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_pool_check_under_the_sanitizers(tmp_path):
    exe = tmp_path / "grammar_pool_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "grammar_pool_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "grammar_pool_check: 0 failures" in run.stdout, (run.stdout, run.stderr[-3000:])


# ---- the scripted engine
class ItemsSlot(FrontEndSlot):
    def set_grammar(self, grammar):
        self.calls.append(("set_grammar", grammar))

    def clear_grammar(self):
        self.calls.append(("clear_grammar",))

    def set_grammars(self, grammar_set):
        self.calls.append(("set_grammars", grammar_set))

    def select_grammars(self, indices):
        self.calls.append(("select_grammars", list(indices)))


class ItemsEngine(FrontEndEngine):
    slot_type = ItemsSlot


NAMES = ("set_grammar", "clear_grammar", "set_grammars", "select_grammars", "generate")
KW = dict(language="en", vad_filter=False, clip_timestamps=[{"start": 0, "end": SR}], batch_size=2)
FILES = [np.zeros(SR, np.float32)] * 4


def _model(engine_type=ItemsEngine):
    eng = engine_type(WhisperSpec(80, 128, 2, 1, 1, 512, V))
    eng.default_tokens = [300, 301, 302]
    return WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(V), max_batch=6, vad_model=EnergyGateModel())


def _pipe(engine_type=ItemsEngine):
    hip = _model(engine_type)
    return BatchedInferencePipeline(hip), hip._slot()


def test_transcribe_many_selects_the_grammar_of_each_chunks_file():
    pipe, slot = _pipe()
    yes, acct = [[55], [56, 57]], [[64, 65]]
    out = pipe.transcribe_many(FILES, grammars=[yes, None, acct, yes], grammars_repeat=[True, True, False, True], **KW)
    assert all(len(segs) == 1 for segs, _info in out)
    calls = [c for c in slot.calls if c[0] in NAMES]
    # one upload for the wave (equal lists are one table), a selection per decode group of two chunks
    assert [c[0] for c in calls] == ["set_grammars", "select_grammars", "generate", "select_grammars", "generate"], calls
    gset = calls[0][1]
    assert len(gset) == 2 and gset.tables[0].phrases == [(55,), (56, 57)] and gset.tables[1].repeat is False
    assert calls[1][1] == [0, -1] and calls[3][1] == [1, 0] and G.current_items() is None
    # a job without grammars on the same slot clears the mode; all-None is such a job
    n0 = len(slot.calls)
    pipe.transcribe_many(FILES[:2], grammars=[None, None], **KW)
    assert [c[0] for c in slot.calls[n0:] if c[0] in NAMES] == ["clear_grammar", "generate"]


def test_a_refused_list_costs_only_its_file_and_the_combinations_are_value_errors():
    pipe, _slot = _pipe()
    files, too_many = FILES[:3], ["a b c d e f g h " * 600]
    out = pipe.transcribe_many(files, grammars=[[[55]], too_many, [[56, 57]]], suppress_tokens=[57], **KW)
    assert len(out[0][0]) == 1 and out[0][1] is not None
    assert isinstance(out[1][0], ValueError) and "4096 states" in str(out[1][0]) and out[1][1] is None
    assert isinstance(out[2][0], ValueError) and "suppresses" in str(out[2][0])            # the dead-state rule against the job's suppress_tokens
    assert "at least one phrase" in str(pipe.transcribe_many(files, grammars=[[], None, None], **KW)[0][0])
    one = [[[55]]] * 3
    for kw, word in ((dict(grammars=[[[55]], too_many, None], on_error="raise"), "4096 states"), (dict(grammars=one, grammar=[[55]]), "one of them"),
                     (dict(grammars=one, keywords=["acme"]), "keywords"), (dict(grammars=one, logit_bias={5: 1.0}), "logit_bias"),
                     (dict(grammars=one[:2]), "one entry per file"), (dict(grammars=one, grammars_repeat=[True]), "grammars_repeat")):
        with pytest.raises(ValueError, match=word):
            pipe.transcribe_many(files, **kw, **KW)
    # a slot that cannot take a set is an error, never an unconstrained decode
    with pytest.raises(RuntimeError, match="set_grammars"):
        _pipe(FrontEndEngine)[0].transcribe_many(files, grammars=[[[55]], None, None], **KW)


def test_an_upload_with_a_grammar_joins_the_pool_and_answers_like_the_unpooled_route():
    from tests.test_rest import Served
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes((np.random.default_rng(1).standard_normal(2 * SR) * 6000).astype("<i2").tobytes())
    base = [("file", ("a.wav", buf.getvalue())), ("response_format", "verbose_json")]
    fields = base + [("grammar", "yes"), ("grammar", "no"), ("grammar_repeat", "false")]
    answers, calls = {}, {}
    for pooled in (False, True):
        m = _model()
        with Served(m, model_factory=lambda model, device_index, **kw: m, file_batch_size=2, file_batch_window_ms=20 if pooled else 0) as s:
            for f in (fields, base, fields + [("keywords", "acme")]):
                answers[pooled, len(f)] = s.post(f)
            assert (s.server.batcher.jobs if pooled else s.server.batcher) == (2 if pooled else None)
        calls[pooled] = [c for slot in m._slots for c in slot.calls if c[0] in NAMES]
    assert [c[0] for c in calls[False]] == ["set_grammar", "generate", "clear_grammar", "generate"] and calls[False][0][1].repeat is False
    assert [c[0] for c in calls[True]] == ["set_grammars", "select_grammars", "generate", "clear_grammar", "generate"], calls[True]
    assert calls[True][0][1].tables[0].phrases == calls[False][0][1].phrases and calls[True][0][1].tables[0].repeat is False and calls[True][1][1] == [0]
    # the two routes answer the same bytes, and a grammar next to keywords is a 400 on both
    assert answers[True, 5][0] == 200 and answers[True, 5][2] == answers[False, 5][2] and json.loads(answers[True, 5][2])["segments"][0]["tokens"] == [300, 301, 302]
    assert answers[True, 6][0] == answers[False, 6][0] == 400 and answers[True, 6][2] == answers[False, 6][2]
