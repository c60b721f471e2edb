"""No GPU, DESIGN.md §34: LmSet, transcribe_many(lms=, lm_weights=) on tests/fakes.py, the REST batcher pooling uploads of different lm_weight."""
import threading

import pytest

from tests.fakes import FrontEndEngine, FrontEndSlot
from tests.test_grammar_items_host import FILES, KW, V, _pipe
from whisperlive_amd import _lib
from whisperlive_amd import lm as L

NAMES = ("set_lm", "clear_lm", "set_lms", "select_lms", "generate")
record = lambda name: lambda self, *a: self.calls.append((name, *(list(x) if name == "select_lms" else x for x in a)))
ItemsSlot = type("ItemsSlot", (FrontEndSlot,), {name: record(name) for name in NAMES[:4]})
ItemsEngine = type("ItemsEngine", (FrontEndEngine,), {"slot_type": ItemsSlot})


def lm_for(pipe, corpus, order=2):
    return L.NgramLM.from_corpus(corpus, None, order=order, eot=pipe.model.token_ids.eot, vocab=V)


def test_a_set_stores_a_model_once_and_names_its_caps():
    ms = [L.NgramLM.from_corpus([[k + 1, 2]], None, order=2, eot=9) for k in range(_lib.LM_MAX_MODELS + 1)]
    s = L.LmSet([(ms[0], 0.3), (ms[1], 0.5)])
    assert (s.add(ms[0], 0.3), s.add(ms[0], 0.7), s.add(ms[1], 0.5)) == (0, 2, 1) and len(s) == 3 and len(s.models) == 2 and s.version == 3
    assert s.entries == [(0, 0.3), (1, 0.5), (0, 0.7)] and s.index(ms[0], 0.7) == 2 and s.index(ms[2], 0.3) is None
    cases = (([(m, 0.3) for m in ms], "8 models in one set"), ([(ms[0], 0.01 * (k + 1)) for k in range(65)], "64 entries in one set"),
             ([(ms[0], 0.3), (ms[1], 0.0)], "finite and above 0"), ([(ms[0], 0.3), ("x", 0.3)], "NgramLM"),
             ([(ms[0], 0.3), (L.NgramLM.from_corpus([[1]], None, order=1, eot=7), 0.3)], "one vocabulary"))
    for entries, word in cases:
        s = L.LmSet()
        with pytest.raises(ValueError, match=word):
            for e in entries:
                s.add(*e)
        assert len(s) == len(entries) - 1 and not s.fits(*e) and s.fits(*entries[0])


def test_transcribe_many_selects_the_entry_of_each_chunks_file():
    pipe, slot = _pipe(ItemsEngine)
    a, b = lm_for(pipe, [[300, 301]]), lm_for(pipe, [[301, 302]], order=1)
    out = pipe.transcribe_many(FILES, lms=[a, None, b, a], lm_weights=[0.3, None, 0.5, 0.3], **KW)
    assert all(len(segs) == 1 for segs, _info in out)
    calls = [c for c in slot.calls if c[0] in NAMES]
    # one upload for the wave (an equal pair is one entry), a selection per decode group of two chunks
    assert [c[0] for c in calls] == ["set_lms", "select_lms", "generate", "select_lms", "generate"], calls
    assert calls[0][1].models == [a, b] and calls[0][1].entries == [(0, 0.3), (1, 0.5)]
    assert calls[1][1] == [0, -1] and calls[3][1] == [1, 0] and L.current_items() is None
    # one weight for all files; then a job without models on the same slot clears the mode
    n0 = len(slot.calls)
    pipe.transcribe_many(FILES[:2], lms=[a, b], lm_weights=0.8, **KW)
    pipe.transcribe_many(FILES[:2], lms=[None, None], **KW)
    later = [c for c in slot.calls[n0:] if c[0] in NAMES]
    assert [c[0] for c in later] == ["set_lms", "select_lms", "generate", "clear_lm", "generate"] and later[0][1].entries == [(0, 0.8), (1, 0.8)]


def test_a_refused_entry_costs_only_its_file_and_the_combinations_are_value_errors():
    pipe, _slot = _pipe(ItemsEngine)
    a, files = lm_for(pipe, [[300, 301]]), FILES[:3]
    other = L.NgramLM.from_corpus([[1, 2]], None, order=2, eot=9, vocab=V)
    out = pipe.transcribe_many(files, lms=[a, other, a], lm_weights=[0.3, 0.3, -1.0], **KW)
    assert len(out[0][0]) == 1 and out[0][1] is not None
    assert isinstance(out[1][0], ValueError) and "end-of-text" in str(out[1][0]) and out[1][1] is None
    assert isinstance(out[2][0], ValueError) and "weight" in str(out[2][0])
    three = [a] * 3
    for kw, word in ((dict(lms=[a, other, None], on_error="raise"), "end-of-text"), (dict(lms=three, lm=a), "one of them"),
                     (dict(lms=three, keywords=["acme"]), "keyword boosting is out of scope"), (dict(lms=three, logit_bias={5: 1.0}), "out of scope"),
                     (dict(lms=three, grammar=[[55]]), "grammar is out of scope"), (dict(lms=three, grammars=[[[55]]] * 3), "out of scope"),
                     (dict(lms=three, grammar_pattern=r"\d"), "out of scope"), (dict(lms=three, grammar_patterns=[r"\d"] * 3), "out of scope"),
                     (dict(lms=three[:2]), "one entry per file"), (dict(lms=a), "one entry per file"), (dict(lms=three, lm_weights=[0.3]), "lm_weights"),
                     (dict(lm_weights=0.3), "goes with lms"), (dict(lm=[a]), "out of scope")):
        with pytest.raises(ValueError, match=word):
            pipe.transcribe_many(files, **kw, **KW)
    # a slot that cannot take a set is an error, never an unfused decode
    with pytest.raises(RuntimeError, match="set_lms"):
        _pipe(FrontEndEngine)[0].transcribe_many(files, lms=[a, None, None], **KW)


def test_the_file_batcher_pools_uploads_that_differ_in_lm_weight():
    from whisperlive_amd import rest as R
    jobs, model = [], object()

    class Pipe:
        def iter_many(self, audios, **kw):
            jobs.append(kw)
            for i in range(len(audios)):
                yield i, [f"seg{i}"], object()

    fb = R.FileBatcher(lambda tr: Pipe(), batch_size=2, window_s=30.0)         # (a job closes when it is full: nothing waits the window out)
    try:
        tr, out = object(), {}

        def up(name, weight):
            per_file = dict(language=None, initial_prompt=None, hotwords=None, diarize=False, max_speakers=0, lm=(model, weight))
            out[name] = fb.submit(tr, name.encode(), per_file, dict(temperature=0.0))
        ts = [threading.Thread(target=up, args=a) for a in (("x", 0.3), ("y", 0.9))]
        [t.start() for t in ts]
        [t.join(timeout=20) for t in ts]
    finally:
        fb.close()
    assert len(out) == 2 and fb.jobs == len(jobs) == 1
    assert jobs[0]["lms"] == [model, model] and sorted(jobs[0]["lm_weights"]) == [0.3, 0.9] and "keywords" not in jobs[0] and "grammars" not in jobs[0]
