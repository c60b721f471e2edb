"""GPU tests of the translation kernels of csrc/mt.hip, one launch each through the wlx_mt_debug_attn / _topk / _embed hooks,
against the float64 references of tests/mt_kernel_ref.py on the same fp16-rounded (attention, embedding) or fp32 (top-k) inputs.
The bounds are derived in the docstrings of mt_kernel_ref.attn_bound / topk_bound / embed_bound; tests/test_mt_kernel_ref.py
checks on the host, for every input set here, that the nearest plausible wrong answer lies outside them."""
from __future__ import annotations

import numpy as np
import pytest

from . import mt_kernel_ref as R

pytestmark = pytest.mark.gpu


def _check_attn(c):
    rc, o = R.run_attn(c)
    assert rc == 0
    a = (c["q"], c["k"], c["v"], c["groups"], c["heads"], c["anc"], c["ld_anc"], c["tmax"])
    ref, _ = R.attn_ref(*a)
    bound = R.attn_bound(*a)
    got = {(i, h): o[i, 64 * h:64 * h + 64] for (i, h) in ref}
    assert all(np.isfinite(g.astype(np.float64)).all() for g in got.values())
    excess = R.attn_excess(got, ref, bound)
    assert excess <= 1.0, excess
    # rows no group owns, and the columns past the heads, come back as they went in
    owned = np.zeros(o.shape, bool)
    for (i, h) in ref:
        owned[i, 64 * h:64 * h + 64] = True
    assert (o.view(np.uint16)[~owned] == c["o"].view(np.uint16)[~owned]).all()


@pytest.mark.parametrize("max_nq", sorted(R.ATTN_LAYOUTS))
@pytest.mark.parametrize("pattern", R.ATTN_PATTERNS)
def test_attn_tiles(pattern, max_nq):
    """every nk of (1, 2, 63, 64, 65, 127, 128, 129, 447, 448, 1000, 1024) as ragged groups of one launch (k0 packed; every nq
    of 1..max_nq, nq = max_nq at nk >= 129; max_nq 1 / 4 / 5 / 16: both templates, every wave), heads 1 / 6 / 16, row strides
    wider than heads x 64 (fused-qkv 3d, cross K / V 6d, odd widths) with garbage of +-1000 in the unread columns. Scores rise or fall across the tiles (the running max
    moves in every tile / only in the first), are near-uniform, or one key at 0, 63, 64 or nk - 1 dominates by +4.
    Bound per element (mt_kernel_ref.attn_bound): U16 |O| + 2^-25 + (1 + U16) 2 (eps_p + (nk + 2) U32) S, the fp16 rounding of
    the output plus the fp32 dot products, __expf and accumulation; no GPU figure enters it."""
    _check_attn(R.attn_tile_case(pattern, max_nq))


@pytest.mark.parametrize("t1", [1, 64, 65, 200, 448])
def test_attn_ancestry(t1):
    """decoder self-attention at step t1 - 1 of 2 items x 5 beams (tmax 448) through ancestry tables that switch beams at tile
    boundaries and inside tiles; bound as in test_attn_tiles"""
    _check_attn(R.attn_ancestry_case(t1))


def _check_topk(x, k, ban, nban):
    rc, val, idx = R.run_topk(x, k, ban, nban)
    assert rc == 0
    rv, ri = R.topk_ref(x, k, ban, nban)
    assert (idx == ri).all(), [(r, idx[r].tolist(), ri[r].tolist()) for r in np.nonzero((idx != ri).any(1))[0][:3]]
    live = ri >= 0
    assert np.isneginf(val[~live]).all()
    err = np.abs(val.astype(np.float64) - np.where(live, rv, 0))[live]
    bound = np.broadcast_to(R.topk_bound(x)[:, None], rv.shape)[live]
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("k", R.TOPK_KS)
@pytest.mark.parametrize("vocab", R.TOPK_VOCABS)
def test_topk(vocab, k):
    """vocab 16 / 80 (empty trailing chunks) / 2112 / 4000 / 128112 / 262144 (the LDS limit), k 1 / 2 / 10 / 32, 80 rows (16
    at 262144) with logit spreads from +-1 to +-80. Ties within one thread's stride, across the waves of a chunk, across chunks
    and at the row maximum; bans (odd rows) on the argmax, on chunk boundaries, repeated, and on one row all but k - 1 tokens.
    Indices exact (value descending, smaller index on a tie; -1 / -inf past the eligible tokens); log-probabilities against
    logit - logsumexp(all logits, banned included) in float64 within mt_kernel_ref.topk_bound: the fp32 rounding of x - logZ
    and M + log Z, the chunk and merge sums, and __expf / __logf to 2 ulp."""
    x, ban, nban, k = R.topk_case(vocab, k)
    _check_topk(x, k, ban, nban)


@pytest.mark.parametrize("vocab", [80, 128112])
def test_topk_without_ban_table(vocab):
    """nban == nullptr: no row banned (as the engine calls it without no_repeat_ngram)"""
    x, _, _, k = R.topk_case(vocab, 32, seed=1)
    _check_topk(x, k, None, None)


@pytest.mark.parametrize("vocab,d,scaled", R.EMBED_CASES)
def test_embed(vocab, d, scaled):
    """tokens 15 / 16 / 17 (pack-tile edges), vocab - 1, the pad token at the pad position, position max_positions + 1, with and
    without scale_embedding; E packed by the engine's launch_pack_linear call. Bound: two fp32 roundings,
    2 U32 (|scale e| + |p|) (mt_kernel_ref.embed_bound)"""
    E, tok, pos, scale, sinpos = R.embed_case(vocab, d, scaled)
    rc, x = R.run_embed(E, tok, pos, scale, sinpos)
    assert rc == 0
    ref = R.embed_ref(E, tok, pos, scale, sinpos)
    assert (np.abs(x - ref) <= R.embed_bound(E, tok, pos, scale, sinpos)).all()
    assert (x[tok == 1] == sinpos[pos[tok == 1]]).all()     # the pad row of E is zero
