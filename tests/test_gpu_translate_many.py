"""GPU tests of wlx_mt_translate_many (a whole transcript as one job, the search on the device) against wlx_mt_translate (the
host search), at the fixture config with seeded weights as tests/test_gpu_translation.py builds them: the transformers recording,
one source, more sources than two batches with mixed lengths, repeated calls, every refusal, and HipTranslator.translate_many."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from whisperlive_amd.mt_weights import MTGenOptions, MTSpec, random_mt_weights

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "mt_golden.json")))
FIX = MTSpec(**GOLD["spec"])
MAX_BATCH, MAX_SRC = 8, 128


def opts_of(c):
    return MTGenOptions(num_beams=c["num_beams"], max_length=c["max_length"], early_stopping=c["early_stopping"],
                        length_penalty=c["length_penalty"], no_repeat_ngram_size=c.get("no_repeat_ngram_size", 0),
                        forced_eos_token_id=c.get("forced_eos_token_id"))


def strip(seq, spec):
    s = seq[1:]
    if spec.eos_id in s:
        s = s[:s.index(spec.eos_id)]
    return s


def bits(scores):
    return np.asarray(scores, np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module")
def eng():
    from whisperlive_amd.translation import HipMTEngine
    w = random_mt_weights(FIX, seed=GOLD["seed"], peaked=GOLD["peaked"])
    e = HipMTEngine(FIX, w, device=0, max_batch=MAX_BATCH, max_rows=5, max_src=MAX_SRC)
    yield e
    e.close()


def mixed_sources():
    """2 * max_batch + 1 sources: one token, max_src tokens, the recording's eight, duplicates, in no length order"""
    rng = np.random.default_rng(21)
    g = GOLD["sources"]
    longest = [2000] + [int(x) for x in rng.integers(4, 1900, size=MAX_SRC - 2)] + [FIX.eos_id]
    mid = [2001] + [int(x) for x in rng.integers(4, 1900, size=40)] + [FIX.eos_id]
    srcs = [g[5], [FIX.eos_id], g[0], longest, g[7], g[2], g[2], mid, g[1], g[6], [FIX.eos_id], g[3], longest, g[4], mid[:20] + [FIX.eos_id],
            g[0], g[5]]
    assert len(srcs) == 2 * MAX_BATCH + 1 and min(map(len, srcs)) == 1 and max(map(len, srcs)) == MAX_SRC
    return srcs


@pytest.fixture(scope="module")
def singles(eng):
    """wlx_mt_translate of every distinct source alone, per option set (computed once, shared)"""
    cache = {}

    def get(src, o):
        key = (tuple(src), repr(o))
        if key not in cache:
            t, s = eng.translate_ids([src], o)
            cache[key] = (t[0], s[0])
        return cache[key]
    return get


@pytest.mark.parametrize("case", [c["name"] for c in GOLD["cases"]])
def test_many_matches_transformers_golden(eng, case):
    c = next(x for x in GOLD["cases"] if x["name"] == case)
    toks, scores = eng.translate_ids_many(GOLD["sources"], opts_of(c))
    for i, r in enumerate(c["results"]):
        assert toks[i] == strip(r["sequence"], FIX), (case, i)
        if r["score"] is not None:
            assert abs(scores[i] - r["score"]) <= 2e-3 * max(1.0, abs(r["score"])), (case, i, scores[i], r["score"])
    # the eight sources are in length order: one group, the composition of the batched host-search call — the same bits
    ht, hs = eng.translate_ids(GOLD["sources"], opts_of(c))
    assert toks == ht and bits(scores) == bits(hs)


@pytest.mark.parametrize("beams", [1, 5])
def test_one_source(eng, singles, beams):
    o = MTGenOptions(num_beams=beams, max_length=40, early_stopping=True, length_penalty=1.0)
    for src in (GOLD["sources"][3], [FIX.eos_id]):
        toks, scores = eng.translate_ids_many([src], o)
        t, s = singles(src, o)
        assert toks == [t] and bits(scores) == bits([s])


@pytest.mark.parametrize("o", [MTGenOptions(num_beams=5, max_length=40, early_stopping=True, length_penalty=1.0),
                               MTGenOptions(num_beams=1, max_length=30),
                               MTGenOptions(num_beams=4, max_length=24, early_stopping=False, length_penalty=0.6, no_repeat_ngram_size=2,
                                            forced_eos_token_id=2)], ids=["beam5", "greedy", "beam4_ngram_forced"])
def test_more_than_two_batches_in_input_order(eng, singles, o):
    srcs = mixed_sources()
    toks, scores = eng.translate_ids_many(srcs, o)
    assert len(toks) == len(srcs)
    # each entry: the single call on that source (tokens; the score to the bound batch == singles holds in test_gpu_translation.py)
    for i, src in enumerate(srcs):
        t, s = singles(src, o)
        assert toks[i] == t, i
        assert abs(scores[i] - s) <= 1e-4, (i, scores[i], s)
    # and, bit for bit, wlx_mt_translate on each group's composition: stable length order, groups of max_batch
    order = sorted(range(len(srcs)), key=lambda i: len(srcs[i]))
    for k in range(0, len(order), MAX_BATCH):
        grp = order[k:k + MAX_BATCH]
        ht, hs = eng.translate_ids([srcs[i] for i in grp], o)
        assert [toks[i] for i in grp] == ht
        assert bits([scores[i] for i in grp]) == bits(hs)
    # a second call on the same slot: the same bits (no state of the first call survives), also after a different job in between
    eng.translate_ids_many(srcs[:3], MTGenOptions(num_beams=2, max_length=9, no_repeat_ngram_size=1))
    toks2, scores2 = eng.translate_ids_many(srcs, o)
    assert toks2 == toks and bits(scores2) == bits(scores)


def test_refusals_write_nothing(eng):
    from whisperlive_amd import _lib
    lib = eng.lib
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    good = eng._opts(MTGenOptions(num_beams=5, max_length=20, early_stopping=True))
    ids, lens, stride = eng._pack([GOLD["sources"][0], GOLD["sources"][2]])

    def call(n=2, ids=ids, lens=lens, stride=stride, opts=good, toks="buf", cnt="buf", null_src=False, slot=None):
        t = np.full((4, 20), -7, np.int32)
        c = np.full(4, -7, np.int32)
        s = np.full(4, -7.0, np.float32)
        rc = lib.wlx_mt_translate_many(eng.h, eng.slot if slot is None else slot, n, None if null_src else ids.ctypes.data_as(i32p),
                                       lens.ctypes.data_as(i32p) if lens is not None else None, stride,
                                       C.byref(opts) if opts is not None else None, t.ctypes.data_as(i32p) if toks else None, 20,
                                       c.ctypes.data_as(i32p) if cnt else None, s.ctypes.data_as(f32p))
        if rc != 0:
            assert (t == -7).all() and (c == -7).all() and (s == -7.0).all(), "a refused call wrote to its outputs"
        return rc

    assert call(null_src=True) == _lib.ERR_ARG
    assert call(lens=None) == _lib.ERR_ARG
    assert call(toks=None) == _lib.ERR_ARG
    assert call(cnt=None) == _lib.ERR_ARG
    assert call(opts=None) == _lib.ERR_ARG
    assert call(n=0) == _lib.ERR_ARG
    assert call(n=_lib.MT_MANY_MAX + 1) == _lib.ERR_ARG
    assert call(lens=np.array([3, 0], np.int32)) == _lib.ERR_ARG
    long_ids = np.zeros((2, MAX_SRC + 1), np.int32) + 5
    assert call(ids=long_ids, lens=np.array([3, MAX_SRC + 1], np.int32), stride=MAX_SRC + 1) == _lib.ERR_ARG
    bad_tok = ids.copy()
    bad_tok[1, 1] = FIX.vocab
    assert call(ids=bad_tok) == _lib.ERR_ARG
    for bad in (MTGenOptions(num_beams=6, max_length=20), MTGenOptions(num_beams=5, max_length=1), MTGenOptions(num_beams=5, max_length=449)):
        assert call(opts=eng._opts(bad)) == _lib.ERR_ARG
    es = eng._opts(MTGenOptions(num_beams=5, max_length=20))
    es.early_stopping = 3
    assert call(opts=es) == _lib.ERR_ARG
    assert call(slot=12345) == _lib.ERR_ARG
    # a busy slot: another thread is inside a call on it (it retries if this thread's probe got the slot first)
    import threading
    srcs = mixed_sources() * 2
    o = MTGenOptions(num_beams=5, max_length=100, early_stopping="never", length_penalty=1.0)
    started, codes, errs = threading.Event(), [], []

    def long_job():
        started.set()
        while True:
            try:
                eng.translate_ids_many(srcs, o)
                return
            except _lib.WlxError as e:
                if e.code != _lib.ERR_STATE:
                    errs.append(e)
                    return
    th = threading.Thread(target=long_job)
    th.start()
    started.wait()
    while th.is_alive() and _lib.ERR_STATE not in codes:
        codes.append(call())
    th.join()
    assert not errs, errs
    assert _lib.ERR_STATE in codes and set(codes) <= {0, _lib.ERR_STATE}, codes
    assert call() == 0      # the slot is free again


def test_translator_translate_many_equals_a_loop_of_translate(eng):
    from whisperlive_amd.mt_tokenizer import M2M100SPTokenizer
    from whisperlive_amd.translation import HipTranslator
    tok = M2M100SPTokenizer(os.path.join(HERE, "golden", "mt_tok"))
    tr = HipTranslator(None, engine=eng, tokenizer=tok, options=MTGenOptions(num_beams=5, max_length=40, early_stopping=True))
    texts = ["Hello world.", "", "   ", "And so, my fellow Americans, ask not what your country can do for you.", "Yes.", "Hello world.",
             "One two three four five six seven eight nine ten eleven twelve.", "Thank you.", "What time is it?", "Good morning.", "No."]
    many = tr.translate_many(texts, "de")
    assert many == [tr.translate([t], "de")[0] for t in texts]
    assert many[1] == "" and many[2] == "   " and many[0] == many[5] and many[0] != ""
