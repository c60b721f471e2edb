"""GPU tests of the translation engine's device search (csrc/mt_search.hip) through wlx_mt_debug_search: the same seeded logits go
to the production top-k launches and then to the host bookkeeping of wlx_mt_translate (use_device=0) and to the device search of
wlx_mt_translate_many (use_device=1). Tokens, counts and decode steps must be equal and the scores equal BIT FOR BIT: the device
search uses the host code's float operations in its order, with a correctly rounded division.

Vocabulary 97 (not a multiple of the 64 top-k chunks); (batch, beams) over (1, 1), (3, 1), (1, 4), (2, 5), (3, 4). The logits are
peaked on the CPU so that no case is trivial: what the cases need (an early finish, a run to max_length, a full ban list, ties) is
asserted on the HOST result or on the inputs, never on the device result.

"A step where all 2R candidates are EOS": a beam contributes its EOS token once, so at most R of an item's 2R merged candidates
can be EOS; what the host code's `all_hit` branch sees is a step where all 2R candidates are HITS, which happens at
cur_len + 1 >= max_length. test_all_candidates_hit covers that step (max_length 3: the second step hits everywhere) together with
EOS on top of every beam."""
from __future__ import annotations

import numpy as np
import pytest

from whisperlive_amd.mt_weights import MTGenOptions, MTSpec

from .mt_oracle import M2M100Oracle

pytestmark = pytest.mark.gpu
V, PAD, EOS, START = 97, 1, 2, 0
SHAPES = [(1, 1), (3, 1), (1, 4), (2, 5), (3, 4)]
MULTI = [s for s in SHAPES if s[0] > 1]


def search(logits, batch, o, use_device, ban_ld=448, step_block=0):
    from whisperlive_amd.translation import mt_debug_search
    return mt_debug_search(logits, batch, o, PAD, EOS, START, ban_ld=ban_ld, step_block=step_block, use_device=use_device)


def make_logits(batch, beams, steps, seed, eos_from=None, spread=1.0, peaks=()):
    """normal logits [steps][batch * beams][V]; EOS at -30 except for the items of `eos_from` (item -> first step with EOS at +30 on
    all of its rows); `peaks`: tokens lifted by 6 on every row"""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((steps, batch * beams, V)) * spread).astype(np.float32)
    lg[:, :, EOS] = -30.0
    lg[:, :, PAD] = -30.0
    for tok in peaks:
        lg[:, :, tok] += 6.0
    for item, s0 in (eos_from or {}).items():
        lg[s0:, item * beams:(item + 1) * beams, EOS] = 30.0
    return lg


def both(logits, batch, o, **kw):
    """host and device search on the same logits -> the host result, after asserting that the device result is identical"""
    ht, hs, hn = search(logits, batch, o, False, **{k: v for k, v in kw.items() if k != "step_block"})
    dt, ds, dn = search(logits, batch, o, True, **kw)
    assert dt == ht, (o, dt, ht)
    assert ds.view(np.uint32).tolist() == hs.view(np.uint32).tolist(), (o, ds, hs)
    assert dn == hn, (o, dn, hn)
    return ht, hs, hn


def variants(batch, beams, steps, seed, **kw):
    """logits sets that between them hold an early finish and a run to max_length: one call for several items (item 0 ends at step
    2, the last item never), two calls for one item"""
    if batch > 1:
        return [make_logits(batch, beams, steps, seed, eos_from={0: 2}, **kw)]
    return [make_logits(batch, beams, steps, seed, eos_from={0: 2}, **kw), make_logits(batch, beams, steps, seed + 1, **kw)]


def check_early_and_full(results, ML, forced=False):
    """on HOST results [(tokens, scores, steps)]: some item finished early and some item ran to max_length"""
    lens = [len(t) for toks, _, _ in results for t in toks]
    full = ML - 2 if forced else ML - 1        # (a forced final EOS is stripped from the output)
    assert min(lens) < full - 1, lens
    assert max(lens) == full, lens


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_max_length_6_forced_eos(batch, beams):
    o = MTGenOptions(num_beams=beams, max_length=6, early_stopping=True, length_penalty=1.0, forced_eos_token_id=EOS)
    res = [both(lg, batch, o) for lg in variants(batch, beams, 5, 100 + batch * 10 + beams)]
    check_early_and_full(res, 6, forced=True)
    # the forced step takes no decode step
    assert max(r[2] for r in res) == 4


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_max_length_70_crosses_64_steps(batch, beams):
    """the ancestry table, the parity buffers and the step blocks (4, and the library's) past 64 steps"""
    o = MTGenOptions(num_beams=beams, max_length=70, early_stopping=False, length_penalty=1.0)
    res = []
    for lg in variants(batch, beams, 69, 200 + batch * 10 + beams):
        res.append(both(lg, batch, o, step_block=4))
        again = search(lg, batch, o, True, step_block=0)
        assert again[0] == res[-1][0] and again[1].view(np.uint32).tolist() == res[-1][1].view(np.uint32).tolist()
        odd = search(lg, batch, o, True, step_block=7)
        assert odd[0] == res[-1][0] and odd[2] == res[-1][2]
    check_early_and_full(res, 70)
    assert max(r[2] for r in res) == 69


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_early_stopping_modes_and_length_penalties(batch, beams):
    """early_stopping False / True / "never" x length_penalty 0, 0.6, 1.3, on logits whose EOS competes (items finish at different
    steps, and finished hypotheses are overtaken or not depending on the penalty)"""
    ML = 14
    rng = np.random.default_rng(300 + batch * 10 + beams)
    lg = make_logits(batch, beams, ML - 1, 310 + batch * 10 + beams, spread=2.0)
    lg[:, :, EOS] = rng.normal(3.0, 2.0, size=lg.shape[:2]).astype(np.float32)      # around the top of 97 logits of spread 2
    lg[:, (batch - 1) * beams:, EOS] = -30.0                                          # the last item runs on
    long_lg = make_logits(batch, beams, ML - 1, 320 + batch * 10 + beams, spread=2.0)
    res = []
    for es in (False, True, "never"):
        for lp in (0.0, 0.6, 1.3):
            o = MTGenOptions(num_beams=beams, max_length=ML, early_stopping=es, length_penalty=lp)
            res.append(both(lg, batch, o))
            if batch == 1:
                res.append(both(long_lg, batch, o))
    e = make_logits(batch, beams, ML - 1, 330 + batch * 10 + beams, eos_from={0: 2})
    res.append(both(e, batch, MTGenOptions(num_beams=beams, max_length=ML, early_stopping=True, length_penalty=1.0)))
    check_early_and_full(res, ML)


def banned(seq, n):
    cur = len(seq)
    if n <= 0 or cur + 1 < n:
        return []
    key = tuple(seq[cur + 1 - n:cur])
    return [seq[a + n - 1] for a in range(cur - n + 1) if tuple(seq[a:a + n - 1]) == key]


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_no_repeat_ngram_2_with_a_full_ban_list(batch, beams):
    """logits peaked on four tokens: without the processor the best hypotheses would repeat bigrams at once. ban_ld = 2, so the
    ban lists of the rows are cut (the same cut on both sides); ban_ld = 448 uncut."""
    ML = 24
    peaks = (5, 6, 7, 8)
    res, free = [], []
    for lg in variants(batch, beams, ML - 1, 400 + batch * 10 + beams, peaks=peaks):
        for ban_ld in (2, 448):
            o = MTGenOptions(num_beams=beams, max_length=ML, early_stopping=True, length_penalty=1.0, no_repeat_ngram_size=2)
            res.append(both(lg, batch, o, ban_ld=ban_ld))
            if ban_ld == 448:       # the uncut result repeats no bigram, and the hypothesis' own history filled a ban list of >= 2
                for t in res[-1][0]:
                    seq = [START] + t
                    grams = list(zip(seq, seq[1:]))
                    assert len(grams) == len(set(grams)), seq
        free += search(lg, batch, MTGenOptions(num_beams=beams, max_length=ML, early_stopping=True), False)[0]
    assert any(len(set(zip([START] + t, t))) < len(t) for t in free), free      # without the processor bigrams WOULD repeat
    longest = max((t for r in res for t in r[0]), key=len)
    seq = [START] + longest
    assert max(len(banned(seq[:k], 2)) for k in range(1, len(seq))) >= 2
    check_early_and_full(res, ML)


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_tied_logits(batch, beams):
    """logits from {0, 1, 2}, the same row for every beam of a step: exactly equal values across tokens and, from the second step,
    across beams — the (value, beam * V + token) rule of the candidate merge and the stable orders behind it"""
    ML = 10
    rng = np.random.default_rng(500 + batch * 10 + beams)
    row = rng.integers(0, 3, size=(ML - 1, batch, 1, V)).astype(np.float32)
    lg = np.broadcast_to(row, (ML - 1, batch, beams, V)).reshape(ML - 1, batch * beams, V).copy()
    assert len(np.unique(lg)) == 3
    lg[:, :, PAD] = -30.0
    late = lg.copy()
    late[:, :, EOS] = -30.0
    lg[:2, :, EOS] = -30.0
    lg[:, :, EOS] = -30.0
    lg[2:, :beams, EOS] = 3.0           # item 0 ends at step 2; the other items run on among tied tokens
    res = []
    for es, lp in ((True, 1.0), (False, 0.6), ("never", 1.3)):
        o = MTGenOptions(num_beams=beams, max_length=ML, early_stopping=es, length_penalty=lp)
        res.append(both(lg, batch, o))
        res.append(both(late, batch, o))
    check_early_and_full(res, ML)


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_all_candidates_hit(batch, beams):
    """max_length 3: at the second step every candidate is a hit (cur_len + 1 >= max_length) and the search stops on `all_hit`;
    with EOS on top of every beam at that step too"""
    o = MTGenOptions(num_beams=beams, max_length=3, early_stopping=False, length_penalty=1.0)
    for seed, eos_from in ((600, None), (601, {b: 1 for b in range(batch)})):
        lg = make_logits(batch, beams, 2, seed + batch * 10 + beams, eos_from=eos_from)
        toks, _, steps = both(lg, batch, o)
        assert steps == 2
        assert all(len(t) == (1 if eos_from else 2) for t in toks), toks


@pytest.mark.parametrize("batch,beams", MULTI)
def test_item_finishing_at_step_2_beside_one_to_max_length(batch, beams):
    """(greedy: the finished item is fed pad until the group ends)"""
    ML = 20
    o = MTGenOptions(num_beams=beams, max_length=ML, early_stopping=True, length_penalty=1.0)
    lg = make_logits(batch, beams, ML - 1, 700 + batch * 10 + beams, eos_from={0: 2})
    toks, _, steps = both(lg, batch, o)
    assert len(toks[0]) == 2 and len(toks[-1]) == ML - 1 and steps == ML - 1


@pytest.mark.parametrize("batch,beams", SHAPES)
def test_against_the_oracle_search(batch, beams):
    """tests/mt_oracle.py's generate() over logits that depend on (item, step) only: the same tokens, scores to float32 rounding"""
    ML = 12
    spec = MTSpec(d_model=64, n_heads=1, enc_layers=1, dec_layers=1, ffn=64, vocab=V, max_positions=448, pad_id=PAD, eos_id=EOS,
                  decoder_start_id=START)
    orc = M2M100Oracle(spec, {})
    rng = np.random.default_rng(800 + batch * 10 + beams)
    per_item = (rng.standard_normal((ML - 1, batch, V)) * 2.0).astype(np.float32)
    per_item[:, :, PAD] = -30.0
    per_item[:, :, EOS] = rng.normal(2.0, 2.0, size=(ML - 1, batch)).astype(np.float32)
    per_item[:, batch - 1, EOS] = -30.0
    lg = np.repeat(per_item, beams, axis=1)
    import torch
    step = lambda i, seq: torch.from_numpy(per_item[len(seq) - 1, i])      # noqa: E731
    for es, lp in ((True, 1.0), (False, 0.6)):
        o = MTGenOptions(num_beams=beams, max_length=ML, early_stopping=es, length_penalty=lp)
        toks, scores, _ = both(lg, batch, o)
        ref, ref_scores = (orc._greedy if beams == 1 else orc._beam)([[0]] * batch, o, step)
        assert toks == ref
        for a, r in zip(scores, ref_scores):      # (the bound tests/test_gpu_translation.py holds the same kernels' scores to)
            assert abs(float(a) - r) <= 2e-3 * max(1.0, abs(r)), (a, r)


def test_refusals():
    from whisperlive_amd._lib import ERR_ARG, WlxError
    o = MTGenOptions(num_beams=2, max_length=6)
    lg = make_logits(1, 2, 5, 1)
    for kw, opts, logits in ((dict(ban_ld=0), o, lg), (dict(), MTGenOptions(num_beams=17, max_length=6), make_logits(1, 17, 5, 1)),
                             (dict(), o, lg[:3])):
        with pytest.raises(WlxError) as e:
            search(logits, 1, opts, True, **kw)
        assert e.value.code == ERR_ARG
