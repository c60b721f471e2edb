"""No GPU: the host side of a pattern per item. PatternSet packing and its named refusals, the pool functions of
csrc/pattern_table.h under the host sanitizers (a stand-alone program, tests/pattern_pool_check.cpp, run as a child process), and
transcribe_many(grammar_patterns=...) on the scripted engine of tests/fakes.py: a set per wave, a selection per decode group."""
import os
import subprocess

import numpy as np
import pytest

from tests.fakes import FrontEndEngine, FrontEndSlot
from tests.test_grammar_host import CXX, HERE
from tests.test_grammar_items_host import FILES, KW, _pipe
from whisperlive_amd import _lib
from whisperlive_amd import pattern as P


def test_a_set_packs_its_patterns_back_to_back_and_names_its_limits():
    a, b, one = P.compile_pattern(r"\d{8}"), P.compile_pattern(r"(yes|no)", ignore_case=True), P.compile_pattern(r".*", leading_space=False)
    s = P.PatternSet([a, b])
    assert (s.add(a), s.add(P.compile_pattern(r"(yes|no)", ignore_case=True)), s.add(one), s.add(b)) == (0, 1, 2, 1) and len(s) == 3 and s.version == 3
    ns, nc, cls, trans, acc = s.packed()
    assert [x.dtype for x in (ns, nc, cls, trans, acc)] == [np.int32, np.int32, np.uint8, np.uint16, np.uint8] and all(x.flags.c_contiguous for x in (cls, trans, acc))
    assert ns.tolist() == [a.n_states, b.n_states, one.n_states] and nc.tolist() == [a.n_classes, b.n_classes, one.n_classes]
    assert (s.n_states, s.n_cells) == (int(ns.sum()), int((ns * nc).sum())) == (acc.size, trans.size) and cls.size == 3 * 256
    assert cls[256:512].tolist() == b.byte_class.tolist() and trans[a.trans.size:a.trans.size + b.trans.size].tolist() == b.trans.ravel().tolist()
    assert acc[a.n_states:a.n_states + b.n_states].tolist() == b.accept.tolist() and s.index(one) == 2 and s.index(P.compile_pattern("x")) is None
    def made(n, c, k):                                                  # distinct tables of n states x c classes, each within a table's limits
        trans = np.zeros((n, c), np.uint16)
        trans[0, 0] = k
        return P.Pattern("made", np.arange(256, dtype=np.uint8) % c, trans, np.zeros(n, np.uint8))
    for tables, word in (([made(4096, 1, k) for k in range(17)], "65536 states in one set"), ([made(4096, 6, k) for k in range(17)], "393216 cells in one set"),
                         ([made(1, 1, 0)] + [made(2, 1, k) for k in range(64)], "64 patterns in one set"), ([one, r"\d"], "compiled patterns")):
        s = P.PatternSet()
        with pytest.raises(ValueError, match=word):
            for t in tables:
                s.add(t)
        assert s.n_states <= _lib.PATTERN_SET_MAX_STATES and s.n_cells <= _lib.PATTERN_SET_MAX_CELLS and not s.fits(t) and s.fits(s.tables[0])


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_pool_check_under_the_sanitizers(tmp_path):
    exe = tmp_path / "pattern_pool_check"
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "pattern_pool_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pattern_pool_check: 0 failures" in run.stdout, (run.stdout, run.stderr[-3000:])


# ---- the scripted engine
NAMES = ("set_pattern", "clear_pattern", "set_patterns", "select_patterns", "generate")
record = lambda name: lambda self, *a: self.calls.append((name, *(list(x) if name == "select_patterns" else x for x in a)))
ItemsSlot = type("ItemsSlot", (FrontEndSlot,), {name: record(name) for name in NAMES[:4]})


class ItemsEngine(FrontEndEngine):
    slot_type = ItemsSlot


def test_transcribe_many_selects_the_pattern_of_each_chunks_file():
    pipe, slot = _pipe(ItemsEngine)
    out = pipe.transcribe_many(FILES, grammar_patterns=[r"yes|no", None, r"\d{8}", r"YES|NO"], grammar_patterns_ignore_case=[True, False, False, True], **KW)
    assert all(len(segs) == 1 for segs, _info in out)
    calls = [c for c in slot.calls if c[0] in NAMES]
    # one upload for the wave (expressions with equal tables are one table), a selection per decode group of two chunks
    assert [c[0] for c in calls] == ["set_patterns", "select_patterns", "generate", "select_patterns", "generate"], calls
    assert len(calls[0][1]) == 2 and calls[0][1].tables[1].regex == r"\d{8}"
    assert calls[1][1] == [0, -1] and calls[3][1] == [1, 0] and P.current_items() is None


def test_a_refused_expression_costs_only_its_file_and_the_combinations_are_value_errors():
    pipe, _slot = _pipe(ItemsEngine)
    files = FILES[:3]
    out = pipe.transcribe_many(files, grammar_patterns=[r" w355", "(", r" w35[67]"], suppress_tokens=[356, 357], **KW)
    assert len(out[0][0]) == 1 and out[0][1] is not None
    assert isinstance(out[1][0], ValueError) and out[1][1] is None
    assert isinstance(out[2][0], ValueError) and "suppresses" in str(out[2][0])            # the dead-state rule against the job's suppress_tokens
    one = [r"\d"] * 3
    for kw, word in ((dict(grammar_patterns=[r"\d", "(", None], on_error="raise"), "without its"), (dict(grammar_patterns=one, grammar_pattern=r"\d"), "one of them"),
                     (dict(grammar_patterns=one, grammar=[[55]]), "phrase list"), (dict(grammar_patterns=one, grammars=[[[55]]] * 3), "phrase list"),
                     (dict(grammar_patterns=one, keywords=["acme"]), "keywords"), (dict(grammar_patterns=one, logit_bias={5: 1.0}), "logit_bias"),
                     (dict(grammar_patterns=one[:2]), "one entry per file"), (dict(grammar_patterns=r"\d"), "one entry per file"),
                     (dict(grammar_patterns=one, grammar_patterns_ignore_case=[True]), "grammar_patterns_ignore_case")):
        with pytest.raises(ValueError, match=word):
            pipe.transcribe_many(files, **kw, **KW)
    # a slot that cannot take a set is an error, never an unconstrained decode
    with pytest.raises(RuntimeError, match="set_patterns"):
        _pipe(FrontEndEngine)[0].transcribe_many(files, grammar_patterns=[r"\d", None, None], **KW)
