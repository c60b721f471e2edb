"""GPU tests (-m gpu) of wlx_align_batch on the tiny seeded engine of test_align_parity: five encoded items, six entries (one item
aligned twice) with text lengths 1, 2, 17, 63 and 70 (the last crosses the 64-row chunk of the teacher-forced pass) and a different
num_frames each, one of them with nf <= 3.

* text_token_probs are bit-identical to wlx_align's entry by entry (the same pass, the same kernels);
* every path is monotone from (0, 0) to (N - 1, nf - 1) and its cost ON THE ORACLE'S MATRIX is within 0.5 % of the optimum
  (test_align_parity's rule and figure: fp16 attention can move a step, DTW is discontinuous);
* an entry's path, count and probabilities are bit-identical alone and in a batch, in any order;
* the slot is left as wlx_align leaves it: a generate straight after gives the same tokens; a stale item and a busy slot are refused."""
import threading

import numpy as np
import pytest

from tests import helpers as H
from oracle import alignment as oal
from oracle import logmel as olm
from oracle import model as omodel

pytestmark = pytest.mark.gpu

TEXT_LENS = [1, 2, 17, 63, 70, 17]
ITEMS = [0, 1, 2, 3, 4, 2]
CLIP_SECONDS = [5, 6, 7, 8, 6]
MW = 7


def _pcm(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1730 * t + 1.0) + 0.05 * rng.standard_normal(n)
    x *= (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def setup(gpu):
    """engine, a slot holding five encoded items, the six entries, and per entry wlx_align's result and the oracle's (computed once)"""
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.weights import random_weights
    spec = H.TINY_EN
    w = random_weights(spec, seed=7)
    eng = HipWhisperEngine(spec, w)
    oracle = omodel.WhisperOracle(H.oracle_spec(spec), H.f16_weights(w))
    ids = H.token_ids_for(spec.vocab)
    slot = eng.create_slot(5, 5)
    Ts = [slot.logmel(_pcm(sec * 16000, 40 + i), item=i) for i, sec in enumerate(CLIP_SECONDS)]
    feats = [slot.features(item=i) for i in range(5)]
    slot.encode(5, seek=[0] * 5, seg=[t - 1 for t in Ts])
    encs = [oracle.encode(olm.pad_or_trim(feats[i][:, : Ts[i] - 1])[None]) for i in range(5)]
    heads = [(l, h) for l in range(spec.dec_layers // 2, spec.dec_layers) for h in range(spec.n_heads)]
    sot_seq = [ids.sot]
    num_frames = [Ts[0] - 1, 6, Ts[2] - 1, Ts[3] - 1, Ts[4] - 1, 301]      # entry 1: nf = 3 (the median is skipped); entry 5: item 2 again, cut short
    entries = []
    for e, (n_text, item) in enumerate(zip(TEXT_LENS, ITEMS)):
        text = np.random.default_rng(100 + e).integers(300, ids.eot - 1, size=n_text).tolist()
        tokens = sot_seq + [ids.no_timestamps] + text + [ids.eot]
        single = slot.align(tokens, len(sot_seq), num_frames[e], heads, ids.eot, median_filter_width=MW, item=item)
        rti, rfi, _, matrix = oal.align(oracle, encs[item], sot_seq, ids.no_timestamps, text, ids.eot, num_frames[e], heads, MW)
        entries.append(dict(tokens=tokens, item=item, num_frames=num_frames[e], single=single, ref_path=(rti, rfi), matrix=matrix))
    yield dict(spec=spec, eng=eng, slot=slot, ids=ids, heads=heads, n_sot=len(sot_seq), entries=entries)
    slot.close()
    eng.close()


def run_batch(s, order):
    en = [s["entries"][i] for i in order]
    return s["slot"].align_batch([x["tokens"] for x in en], s["n_sot"], [x["num_frames"] for x in en], s["heads"], s["ids"].eot,
                                 median_filter_width=MW, items=[x["item"] for x in en])


def test_batch_against_wlx_align(setup):
    s = setup
    res = run_batch(s, range(6))
    for e, ((ti, fi, probs), ent) in enumerate(zip(res, s["entries"])):
        np.testing.assert_array_equal(probs.view(np.uint32), ent["single"][2].view(np.uint32), err_msg=f"entry {e}")
        matrix = ent["matrix"]
        N, M = matrix.shape
        assert N == TEXT_LENS[e] + 1 and M == max(1, min(1500, ent["num_frames"] // 2))
        assert ti[0] == 0 and fi[0] == 0 and ti[-1] == N - 1 and fi[-1] == M - 1, e
        dt, df = np.diff(ti), np.diff(fi)
        assert ((dt == 0) | (dt == 1)).all() and ((df == 0) | (df == 1)).all() and ((dt + df) >= 1).all(), e
        cost = lambda a, b: float((-matrix)[a, b].sum())
        c_got, c_ref = cost(ti, fi), cost(*ent["ref_path"])
        print("align_batch entry", e, "N x M", N, M, "cost", c_got, "optimum", c_ref, "wlx_align's", cost(ent["single"][0], ent["single"][1]))
        assert c_got <= c_ref + 5e-3 * abs(c_ref) + 1e-3, (e, c_got, c_ref)


def test_batch_invariance(setup):
    s = setup
    base = run_batch(s, range(6))
    for order in ([5, 4, 3, 2, 1, 0], [3, 0, 5, 1, 4, 2]):
        got = run_batch(s, order)
        for k, e in enumerate(order):
            for a, b in zip(got[k], base[e]):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (order, e)
    for e in range(6):
        alone = run_batch(s, [e])[0]
        for a, b in zip(alone, base[e]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), e


def test_generate_after_align_batch_and_timings(setup):
    s = setup
    slot, ids = s["slot"], s["ids"]
    kw = dict(beam_size=5, max_length=1 + 12, suppress_tokens=H.default_suppress(ids))
    before = slot.generate([[ids.sot]] * 5, H.engine_ids(ids), **kw)
    run_batch(s, range(6))
    pass_ms, post_ms = slot.align_timings()
    assert pass_ms > 0 and post_ms > 0
    after = slot.generate([[ids.sot]] * 5, H.engine_ids(ids), **kw)
    for a, b in zip(before, after):
        assert a.sequences_ids == b.sequences_ids and a.scores == b.scores


def test_refusals(setup):
    from whisperlive_amd import _lib
    s = setup
    slot, ids, ent = s["slot"], s["ids"], s["entries"][2]
    call = lambda **kw: slot.align_batch(**{**dict(token_lists=[ent["tokens"]], n_sot=s["n_sot"], num_frames=[ent["num_frames"]], heads=s["heads"],
                                                   eot=ids.eot, median_filter_width=MW, items=[2]), **kw})
    with pytest.raises(_lib.WlxError) as ei:
        call(items=[5])                                     # the slot holds five encoded items
    assert ei.value.code == _lib.ERR_STATE
    for bad in (dict(median_filter_width=6), dict(median_filter_width=17), dict(token_lists=[ent["tokens"][:3]]),
                dict(heads=[(s["spec"].dec_layers, 0)]), dict(eot=0), dict(token_lists=[[s["spec"].vocab] + ent["tokens"][1:]]),
                dict(token_lists=[ent["tokens"]] * 65, num_frames=[100] * 65, items=[0] * 65)):
        with pytest.raises(_lib.WlxError) as ei:
            call(**bad)
        assert ei.value.code == _lib.ERR_ARG, bad
    assert slot.align_batch([], s["n_sot"], [], s["heads"], ids.eot) == []


def test_busy_slot_is_refused(setup):
    """a slot serves one call at a time: while a long generate runs on it in another thread, wlx_align_batch returns WLX_ERR_STATE"""
    from whisperlive_amd import _lib
    s = setup
    slot, ids = s["slot"], s["ids"]
    started, stop = threading.Event(), threading.Event()

    def decode_loop():
        kw = dict(beam_size=5, max_length=300, suppress_tokens=H.default_suppress(ids) + [ids.eot])
        while not stop.is_set():
            try:
                started.set()
                slot.generate([[ids.sot]] * 5, H.engine_ids(ids), **kw)
            except _lib.WlxError as err:                    # (the align call got the slot first)
                assert err.code == _lib.ERR_STATE

    th = threading.Thread(target=decode_loop)
    th.start()
    seen = False
    try:
        started.wait()
        for _ in range(400):
            try:
                run_batch(s, [0])
            except _lib.WlxError as err:
                assert err.code == _lib.ERR_STATE
                seen = True
                break
    finally:
        stop.set()
        th.join()
    assert seen
