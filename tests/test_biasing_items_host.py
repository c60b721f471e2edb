"""CPU tests of per-item keyword boosting's host side (whisperlive_amd/biasing.py): the compact form against the closed
table (compile_bias without the edge cap) on seeded random phrase sets, the flag, long lists, BiasSet packing / caps / deduplication,
item_scope, the C-ABI bindings against include/wlx_bias_items.h, and the routes on the scripted engine of tests/fakes.py: generate installs a set
once and selects per group, the per-file spread of transcribe_many and the wave that closes on a pool cap, the file endpoint's pooling
decision, and the batch worker's scope."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from tests.fakes import FakeEngine, FakeSlot
from whisperlive_amd import _lib
from whisperlive_amd import biasing as B
from whisperlive_amd.tokenizer import synthetic_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, EOT = 40, 32


def both(phrases, boost=0.5, lb=None, vocab=V, eot=EOT):
    return (B.compile_compact(phrases, boost, lb, vocab=vocab, eot=eot), B.compile_bias(phrases, boost, lb, vocab=vocab, eot=eot, max_edges=None))


def assert_same(compact, closed, seed=0):
    """every (state, token) leads to the same node; every state's bias is the same bits; the flag sits exactly where the root has the token"""
    rng = np.random.default_rng(seed)
    assert compact.paths == closed.paths and compact.n_nodes == closed.n_nodes
    root = compact.edges(0)[0]
    assert not compact.edges(0)[2].any()
    for s in range(closed.n_nodes):
        for t in range(compact.vocab):
            assert compact.next_state(s, t) == closed.next_state(s, t), (s, t)
        row = (rng.standard_normal(compact.vocab) * 3).astype(np.float32)
        assert np.array_equal(compact.bias_row(row.copy(), s).view(np.uint32), closed.bias_row(row.copy(), s).view(np.uint32)), s
        tok, nxt, shared = compact.edges(s)
        if s:
            assert (shared == np.isin(tok, root)).all(), s
            # an own edge is an entry of the closed list that is not the root's entry for that token
            ctok, cnxt = closed.edges(s)
            rnxt = dict(zip(root.tolist(), compact.edges(0)[1].tolist()))
            want = {(a, b) for a, b in zip(ctok.tolist(), cnxt.tolist()) if rnxt.get(a) != b}
            assert set(zip(tok.tolist(), nxt.tolist())) == want, s
    assert (compact.packed_next & (_lib.BIAS_EDGE_SHARED - 1) == compact.edge_next).all()
    assert ((compact.packed_next & _lib.BIAS_EDGE_SHARED) != 0).tolist() == compact.edge_shared.tolist()


@pytest.mark.parametrize("seed", range(6))
def test_compact_equals_closed_on_random_phrase_sets(seed):
    rng = np.random.default_rng(seed)
    for trial in range(25):
        alphabet = 5 if trial % 2 else 30                       # a small alphabet: overlaps, shared first tokens, phrases inside phrases
        phrases = [[int(x) for x in rng.integers(0, alphabet, size=int(rng.integers(1, 5)))] for _ in range(int(rng.integers(0, 9)))]
        lb = {int(t): float(rng.choice([0.5, -4.0, 2.0])) for t in rng.choice(V, size=int(rng.integers(0, 4)), replace=False)}
        assert_same(*both(phrases, 0.5, lb), seed=trial)


def test_compact_equals_closed_on_the_named_shapes():
    assert_same(*both([[1, 2, 3], [1, 2], [2, 3, 4], [3], [1, 5], [1, 2, 3, 6]]))     # a prefix of another, one ending inside another, shared first tokens
    assert_same(*both([[7, 7, 9], [7, 3]]))                                            # a token in both lists with another next
    assert_same(*both([[t] for t in range(0, 30, 2)]))                                 # single-token phrases only
    assert_same(*both([]))
    c, x = both([[7, 7, 9], [7, 3]])
    n = c.paths.index((7,))
    tok, nxt, shared = c.edges(n)
    assert tok.tolist() == [3, 7] and shared.tolist() == [False, True] and nxt[1] == c.paths.index((7, 7))


def test_a_long_list_compiles_compact_and_is_refused_closed():
    phrases = [[t] for t in range(1000)]
    c = B.compile_compact(phrases, 1.0, vocab=2000, eot=1500)
    assert c.n_nodes == 1001 and c.n_edges == 1000
    with pytest.raises(ValueError, match="16384 edges"):
        B.compile_bias(phrases, 1.0, vocab=2000, eot=1500)
    # 4096 nodes under 1000 first tokens: built directly, no closure
    deep = [[t, 1000 + t, 1100 + (t % 7)] for t in range(1000)] + [[t, 1200 + t] for t in range(1000)]
    d = B.compile_compact(deep, 1.0, vocab=4000, eot=3000)
    assert d.n_nodes == 1 + 4000 - 0 and d.n_edges == 4000
    with pytest.raises(ValueError, match="4096 nodes"):
        B.compile_compact(deep + [[5, 6, 7, 8] * 30], 1.0, vocab=4000, eot=3000)


def test_set_packing_deduplication_and_caps():
    a, _ = both([[1, 2], [3]], 0.5, {4: 2.0})
    b, _ = both([[1, 2, 3]], 1.5)
    a2, _ = both([[1, 2], [3]], 0.5, {4: 2.0})                   # equal content, another object
    s = B.BiasSet([a, b, a, a2])
    assert len(s) == 2 and s.index(a2) == 0 and s.add(b) == 1 and s.version == 2
    nn, off, tok, nxt, boosts, nt, ids, vals = s.packed()
    assert nn.tolist() == [a.n_nodes, b.n_nodes] and off.tolist() == a.edge_off.tolist() + b.edge_off.tolist()
    assert tok.tolist() == a.edge_tok.tolist() + b.edge_tok.tolist() and nxt.tolist() == a.packed_next.tolist() + b.packed_next.tolist()
    assert boosts.tolist() == [0.5, 1.5] and nt.tolist() == [1, 0] and ids.tolist() == [4] and vals.tolist() == [2.0]
    assert s.next_state(-1, 3, 1) == 0 and s.next_state(1, 999, 1) == b.next_state(0, 1)      # no table; a stale state is the root
    # ---- the caps, each named
    big = lambda k: B.compile_compact([[t, 2000 + k] for t in range(1500)], 1.0, vocab=4000, eot=3900)       # 3001 nodes, 3000 edges
    nodes = B.BiasSet([big(k) for k in range(5)])
    assert nodes.n_nodes == 15005 and not nodes.fits(big(9)) and nodes.fits(big(0))
    with pytest.raises(ValueError, match="16384 nodes in one set"):
        nodes.add(big(9))
    assert len(nodes) == 5 and nodes.version == 5                # a refused table leaves the set as it was
    tokens = B.BiasSet([B.compile_compact([], 1.0, {t: 1.0 for t in range(k, 1024 + k)}, vocab=4000, eot=3900) for k in range(4)])
    with pytest.raises(ValueError, match="4096 logit_bias entries in one set"):
        tokens.add(B.compile_compact([], 1.0, {7: 1.0}, vocab=4000, eot=3900))
    many = B.BiasSet([B.compile_compact([[k + 1]], 1.0, vocab=4000, eot=3900) for k in range(64)])
    with pytest.raises(ValueError, match="64 tables in one set"):
        many.add(B.compile_compact([[70]], 1.0, vocab=4000, eot=3900))
    with pytest.raises(ValueError, match="one vocabulary"):
        B.BiasSet([a]).add(B.compile_compact([[1]], 1.0, vocab=50, eot=45))
    with pytest.raises(ValueError, match="compact"):
        B.BiasSet([B.compile_bias([[1]], 1.0, vocab=V, eot=EOT)])


def test_the_edge_cap_of_a_set():
    # edges without as many nodes (a table's own children alone would meet the node cap first): failure links copy a fan into every
    # node of a chain — own lists that are not children
    chain = [[5] * 20] + [[5, t] for t in range(100, 1200)]
    c, x = both(chain, 1.0, None, 4000, 3950)
    assert c.n_edges > 15 * c.n_nodes and c.n_edges < x.n_edges
    s = B.BiasSet()
    with pytest.raises(ValueError, match="65536 edges in one set"):
        for k in range(64):
            s.add(B.compile_compact(chain + [[6, k + 7]], 1.0, vocab=4000, eot=3950))
    assert 0 < len(s) < 64 and s.n_edges <= 65536 and s.n_nodes < 16384
    with pytest.raises(ValueError, match="65536 edges"):       # one table past the pool's edges is refused when it is compiled
        B.compile_compact([[5] * 70] + [[5, t] for t in range(100, 1200)], 1.0, vocab=4000, eot=3950)


def test_item_scope_nests_and_is_per_thread():
    a, _ = both([[1]])
    assert B.current_items() is None
    with B.item_scope([a, None]) as outer:
        assert B.current_items() is outer and outer.tables == [a, None] and isinstance(outer.bias_set, B.BiasSet)
        shared = B.BiasSet()
        with B.item_scope([None], shared) as inner:
            assert B.current_items() is inner and inner.bias_set is shared
        assert B.current_items() is outer
        seen = []
        t = threading.Thread(target=lambda: seen.append(B.current_items()))
        t.start(); t.join()
        assert seen == [None]
    assert B.current_items() is None


def test_bindings_match_the_header():
    main = open(os.path.join(ROOT, "include", "wlx.h")).read()
    assert '#include "wlx_bias_items.h"' in main and int(re.search(r"#define WLX_ABI_VERSION (\d+)", main).group(1)) == 1
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlx_bias_items.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(wlx_[a-z_0-9]+)\s*\(", src))) == sorted(_lib.EXPORTS_BIAS_ITEMS)
    for name, const in (("WLX_BIAS_SET_MAX_TABLES", _lib.BIAS_SET_MAX_TABLES), ("WLX_BIAS_SET_MAX_NODES", _lib.BIAS_SET_MAX_NODES),
                        ("WLX_BIAS_SET_MAX_EDGES", _lib.BIAS_SET_MAX_EDGES), ("WLX_BIAS_SET_MAX_TOKENS", _lib.BIAS_SET_MAX_TOKENS),
                        ("WLX_BIAS_EDGE_SHARED", _lib.BIAS_EDGE_SHARED)):
        assert int(re.search(rf"#define {name} (\w+)", src).group(1), 0) == const
    _lib.build()
    lib = _lib.load()
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    i32p, f32p, i16p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int16)
    ctype = {"wlx_engine*": vp, "int32_t": i32, "int64_t": i64, "float": f32, "const int32_t*": i32p, "const float*": f32p, "float*": f32p,
             "const int16_t*": i16p, "int16_t*": i16p}
    for name in ("wlx_bias_set_items", "wlx_bias_select", "wlx_debug_bias_apply_items"):
        args = re.search(rf"int32_t {name}\((.*?)\);", src, flags=re.S).group(1)
        types = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in args.split(",")]
        assert getattr(lib, name).argtypes == types, name
        assert getattr(lib, name).restype is i32 and name in _lib.EXPORTS_BIAS_ITEMS
    assert lib.wlx_bias_select(None, 0, 1, None) == _lib.ERR_ARG
    assert lib.wlx_bias_set_items(None, 0, 1, None, None, None, None, None, None, None, None) == _lib.ERR_ARG


# ---- the scripted engine
class ItemsSlot(FakeSlot):
    def set_bias(self, table):
        self.calls.append(("set_bias", table))

    def clear_bias(self):
        self.calls.append(("clear_bias",))

    def set_bias_items(self, bias_set):
        self.calls.append(("set_bias_items", bias_set, len(bias_set)))

    def select_bias(self, indices):
        self.calls.append(("select_bias", list(indices)))


class ItemsEngine(FakeEngine):
    slot_type = ItemsSlot


def _model(engine):
    from whisperlive_amd.transcriber import WhisperModelHIP
    return WhisperModelHIP("fake", engine=engine, hf_tokenizer=synthetic_tokenizer(2310))


def _bias_calls(slot, n0=0):
    return [c for c in slot.calls[n0:] if c[0] in ("set_bias", "clear_bias", "set_bias_items", "select_bias", "generate")]


def test_generate_installs_once_and_selects_per_group():
    eng = ItemsEngine()
    eng.default_tokens = [50, 51]
    m = _model(eng)
    pcm = np.zeros(16000, np.float32)
    kw = dict(language="en", temperature=0.0, vad_filter=False)
    a = m.compile_keywords([[5, 6]], 0.5, compact=True)
    b = m.compile_keywords([[7]], 1.5, compact=True)
    shared = B.BiasSet([a, b])
    slot = m._slot()
    with B.item_scope([b], shared):
        m.transcribe(pcm, **kw)
        m.transcribe(pcm, **kw)
    calls = _bias_calls(slot)
    assert [c[0] for c in calls] == ["set_bias_items", "select_bias", "generate", "select_bias", "generate"], calls
    assert calls[0][1] is shared and calls[1][1] == [1]
    # an entry None falls back to the thread's table, which becomes one more table of the set (one more upload: the set has grown)
    n0 = len(slot.calls)
    with m.keyword_bias(phrases=[[9, 9]], boost=2.0) as thread_table:
        with B.item_scope([None], shared):
            m.transcribe(pcm, **kw)
    calls = _bias_calls(slot, n0)
    assert [c[0] for c in calls] == ["set_bias_items", "select_bias", "generate"] and calls[1][1] == [2] and len(shared) == 3
    assert shared.tables[2].phrases == thread_table.phrases and float(shared.tables[2].boost) == 2.0
    # nothing to add for any item on a slot that holds this very set: it stays in per-item mode, every item deselected (no upload when
    # biased and unbiased groups of a job alternate); under another set the slot is cleared; without a scope nothing changes
    n0 = len(slot.calls)
    with B.item_scope([None], shared):
        m.transcribe(pcm, **kw)
    with B.item_scope([b], shared):
        m.transcribe(pcm, **kw)
    calls = _bias_calls(slot, n0)
    assert [c[0] for c in calls] == ["select_bias", "generate", "select_bias", "generate"] and calls[0][1] == [-1] and calls[2][1] == [1]
    n0 = len(slot.calls)
    with B.item_scope([None]):
        m.transcribe(pcm, **kw)
    assert [c[0] for c in _bias_calls(slot, n0)] == ["clear_bias", "generate"]
    n0 = len(slot.calls)
    m.transcribe(pcm, **kw, keywords=[[5, 6]])
    assert [c[0] for c in _bias_calls(slot, n0)] == ["set_bias", "generate"]
    # compact=True: a one-table set selected for every item; a list the closed form refuses
    n0 = len(slot.calls)
    long_list = [[t] for t in range(300)]
    with pytest.raises(ValueError, match="edges"):
        m.keyword_bias(phrases=long_list)
    m.transcribe(pcm, **kw, keywords=long_list, keywords_compact=True)
    calls = _bias_calls(slot, n0)
    assert [c[0] for c in calls] == ["set_bias_items", "select_bias", "generate"] and calls[0][2] == 1 and calls[1][1] == [0]
    # a wrong number of tables is an error, and so is a slot that cannot take a set
    with B.item_scope([a, b], shared):
        with pytest.raises(ValueError, match="2 tables for 1 prompts"):
            m.transcribe(pcm, **kw)
    plain = _model(FakeEngine())
    with B.item_scope([a]):
        with pytest.raises(RuntimeError, match="set_bias_items"):
            plain.transcribe(pcm, **kw)


def test_per_file_tables_of_a_job_and_the_wave_that_closes_on_a_pool_cap():
    from whisperlive_amd import many_files as MF
    m = _model(ItemsEngine())
    t = MF.per_file_tables(m, dict(keywords=[[[5, 6]], None, [[7]], [[5, 6]]], keywords_boost=[0.5, None, 1.5, 0.5], logit_bias=None), 4)
    assert t[1] is None and t[0] is t[3] and t[0].phrases == [(5, 6)] and float(t[2].boost) == 1.5
    one = MF.per_file_tables(m, dict(keywords=[[5, 6], [7]], keywords_boost=None, logit_bias={3: 1.0}), 3)        # token lists: ONE list for every file
    assert one[0] is one[1] is one[2] and one[0].phrases == [(5, 6), (7,)] and one[0].tok_ids.tolist() == [3]
    assert MF.per_file_tables(m, dict(keywords=None, keywords_boost=None, logit_bias=None), 2) == [None, None]
    with pytest.raises(ValueError, match="one entry per file"):
        MF.per_file_tables(m, dict(keywords=[[[5]], None], keywords_boost=None, logit_bias=None), 3)
    with pytest.raises(ValueError, match="keywords_boost needs keywords"):
        MF.per_file_tables(m, dict(keywords=None, keywords_boost=1.0, logit_bias=None), 2)
    # a refused table costs only its file
    r = MF.per_file_tables(m, dict(keywords=[[[5]], [[2309]], None], keywords_boost=None, logit_bias=None), 3)
    assert isinstance(r[1], ValueError) and "special or timestamp" in str(r[1]) and r[0] is not None and r[2] is None
    # the wave rule: 5 tables of 3001 nodes fit the pool's 16384 nodes, the sixth distinct one does not; a repeated table costs nothing
    big = [B.compile_compact([[x, 2000 + k] for x in range(1500)], 1.0, vocab=2310, eot=2305) for k in range(7)]
    tables = [big[0], big[1], None, big[0], big[2], big[3], big[4], big[5], big[6]]
    wave, bset = MF.fit_tables(list(range(9)), tables)
    assert wave == [0, 1, 2, 3, 4, 5, 6] and len(bset) == 5
    wave, bset = MF.fit_tables([7, 8], tables)
    assert wave == [7, 8] and len(bset) == 2
    assert MF.fit_tables([2], tables) == ([2], None)
    wave, bset = MF.fit_tables([0, 1], [ValueError("x"), big[1]])
    assert wave == [0, 1] and len(bset) == 1


def test_the_file_batcher_pools_uploads_with_keywords():
    from whisperlive_amd import rest as R
    assert R.pool_upload(True, False, None, None) and not R.pool_upload(False, False, None, None)
    assert not R.pool_upload(True, True, None, None) and not R.pool_upload(True, False, ["ann"], None)
    jobs = []

    class Pipe:
        def iter_many(self, audios, **kw):
            jobs.append(kw)
            for i in range(len(audios)):
                yield i, [f"seg{i}"], object()

    fb = R.FileBatcher(lambda tr: Pipe(), batch_size=4, window_s=0.3)
    try:
        tr, out = object(), {}

        def up(name, kws, boost):
            per_file = dict(language=None, initial_prompt=None, hotwords=None, diarize=False, max_speakers=0, keywords=kws, keywords_boost=boost)
            out[name] = fb.submit(tr, name.encode(), per_file, dict(temperature=0.0))
        ts = [threading.Thread(target=up, args=a) for a in (("x", ["acme"], 3.0), ("y", None, None), ("z", ["zeta", "eta"], None))]
        [t.start() for t in ts]
        [t.join(timeout=20) for t in ts]
    finally:
        fb.close()
    assert len(out) == 3 and fb.jobs == len(jobs)
    pooled = [j for j in jobs if len(j["language"]) > 1]
    assert pooled, jobs                                               # uploads with different keywords shared a job
    for j in jobs:
        if "keywords" in j:
            assert len(j["keywords"]) == len(j["language"]) == len(j["keywords_boost"])
    flat = sorted((repr(k), b) for j in jobs for k, b in zip(j.get("keywords", [None] * len(j["language"])), j.get("keywords_boost", [None] * len(j["language"]))))
    assert flat == sorted([(repr(["acme"]), 3.0), (repr(None), None), (repr(["zeta", "eta"]), None)])


def test_the_batch_worker_decodes_a_group_under_an_item_scope():
    from whisperlive_amd.batching import BatchInferenceWorker, BatchRequest
    a, _ = both([[1]])
    b, _ = both([[2]])
    reqs = [BatchRequest(audio=np.zeros(4, np.float32), bias_table=a), BatchRequest(audio=np.zeros(4, np.float32)),
            BatchRequest(audio=np.zeros(4, np.float32), bias_table=b)]
    bset = B.BiasSet()
    with BatchInferenceWorker._bias_scope(reqs, bset) as scope:
        assert B.current_items() is scope and scope.tables == [a, None, b] and scope.bias_set is bset
    with BatchInferenceWorker._bias_scope([reqs[2]], bset) as scope:          # a re-decoded subset carries its own tables
        assert scope.tables == [b]
    with BatchInferenceWorker._bias_scope(reqs[1:2], None):
        assert B.current_items() is None
    assert BatchRequest(audio=None).bias_table is None
    # the worker keeps one set per lane: the same sessions batch after batch find their tables in it (no new version, no upload)
    w = BatchInferenceWorker(type("T", (), {"max_batch": 4})(), max_batch_size=4)
    s1 = w._bias_set_for(reqs)
    v = s1.version
    assert w._bias_set_for(reqs[:1]) is s1 and w._bias_set_for(reqs) is s1 and s1.version == v and len(s1) == 2
    assert w._bias_set_for(reqs[1:2]) is None
