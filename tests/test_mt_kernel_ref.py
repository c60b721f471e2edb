"""CPU tests of tests/mt_kernel_ref.py, the float64 references of the translation kernels: each reference against the arithmetic
it restates (M2M100Oracle._attn, torch.log_softmax + topk, M2M100Oracle.embed), the sensitivity guards of every input set of
tests/test_gpu_mt_kernels.py (the nearest plausible wrong answer lies outside the bound the GPU test applies), and the shape
checks of the wlx_mt_debug_* hooks, which refuse before touching a device."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from whisperlive_amd.mt_weights import MTSpec

from . import mt_kernel_ref as R
from .mt_oracle import M2M100Oracle, positions


def _oracle(heads, w):
    spec = MTSpec(d_model=64 * heads, n_heads=heads, enc_layers=1, dec_layers=1, ffn=64, vocab=64)
    o = M2M100Oracle.__new__(M2M100Oracle)
    o.spec = spec
    o.w = {k: torch.from_numpy(v) for k, v in w.items()}
    return o


def test_attn_ref_matches_oracle_attention_arithmetic():
    """_attn with identity projections (q_proj = 8 I undoes the 1/8 scale, k / v read the two halves of [k | v]) is the
    attention the kernel computes"""
    rng = np.random.default_rng(0)
    heads, nq, nk = 3, 5, 77
    d = 64 * heads
    q = R._f16(rng.standard_normal((nq, d)) * 0.5)
    k = R._f16(rng.standard_normal((nk, d)))
    v = R._f16(rng.standard_normal((nk, d)))
    eye, zero = np.eye(d, dtype=np.float32), np.zeros((d, d), np.float32)
    w = {"a.q_proj.weight": 8 * eye, "a.k_proj.weight": np.hstack([eye, zero]), "a.v_proj.weight": np.hstack([zero, eye]),
         "a.out_proj.weight": eye}
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        w[f"a.{n}.bias"] = np.zeros(d, np.float32)
    orc = _oracle(heads, w)
    got = orc._attn(torch.from_numpy(q.astype(np.float32)), torch.from_numpy(np.hstack([k, v]).astype(np.float32)), "a").numpy()
    ref, _ = R.attn_ref(q, k, v, [(0, nq, 0, nk)], heads)
    for (i, h), o in ref.items():
        np.testing.assert_allclose(got[i, 64 * h:64 * h + 64], o, rtol=1e-5, atol=1e-5)     # (torch: fp32)


def test_attn_ref_follows_the_ancestry_table():
    rng = np.random.default_rng(1)
    tmax, rows, nk = 8, 3, 6
    k = R._f16(rng.standard_normal((rows * tmax, 64)))
    v = R._f16(rng.standard_normal((rows * tmax, 64)))
    q = R._f16(rng.standard_normal((rows, 64)))
    anc = rng.integers(0, rows, (rows, tmax)).astype(np.int32)
    ref, _ = R.attn_ref(q, k, v, [(r, 1, 0, nk) for r in range(rows)], 1, anc, tmax, tmax)
    for r in range(rows):
        kr = anc[r, :nk] * tmax + np.arange(nk)
        alone, _ = R.attn_ref(q[r:r + 1], k[kr], v[kr], [(0, 1, 0, nk)], 1)
        np.testing.assert_allclose(ref[(r, 0)], alone[(0, 0)], rtol=1e-15)


@pytest.mark.parametrize("bans", [False, True])
def test_topk_ref_matches_torch_log_softmax_topk(bans):
    rng = np.random.default_rng(2)
    x = rng.permutation(np.arange(4 * 96, dtype=np.float32)).reshape(4, 96) * 0.37 - 40     # distinct: no ties for torch
    ban = np.array([[int(np.argmax(x[r])), 5, 5, 90] for r in range(4)], np.int32)
    nban = np.array([4, 0, 2, 1], np.int32)
    val, idx = R.topk_ref(x, 10, ban if bans else None, nban if bans else None)
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1)
    if bans:
        for r in range(4):
            lp[r, torch.from_numpy(ban[r, :nban[r]]).long()] = float("-inf")
    tv, ti = torch.topk(lp, 10)
    assert (idx == ti.numpy()).all()
    np.testing.assert_allclose(val, tv.numpy(), rtol=0, atol=1e-12)


def test_topk_ref_tie_rule_padding_and_logz_over_banned_tokens():
    x = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0, -1.0, 0.5]], np.float32)
    lz = float(np.log(np.exp(x[0].astype(np.float64)).sum()))
    val, idx = R.topk_ref(x, 4)
    assert idx.tolist() == [[1, 2, 4, 3]]
    val, idx = R.topk_ref(x, 4, larger_index_on_tie=True)
    assert idx.tolist() == [[4, 2, 1, 3]]
    ban = np.array([[1, 2, 4, 3, 0, 5, 5]], np.int32)
    val, idx = R.topk_ref(x, 4, ban, np.array([7], np.int32))
    assert idx.tolist() == [[7, 6, -1, -1]]
    assert np.isneginf(val[0, 2:]).all()
    np.testing.assert_allclose(val[0, :2], [0.5 - lz, -1.0 - lz], rtol=0, atol=1e-12)


def test_embed_ref_matches_oracle_embedding():
    spec = MTSpec(d_model=128, n_heads=2, enc_layers=1, dec_layers=1, ffn=64, vocab=48, max_positions=40)
    rng = np.random.default_rng(3)
    E = rng.standard_normal((48, 128)).astype(np.float32)
    E[spec.pad_id] = 0
    orc = M2M100Oracle(spec, {"model.shared.weight": E}, fp16_matrices=True)
    ids = [0, 17, 1, 47, 16, 15, 2]
    got = orc.embed(ids).numpy()
    ref = R.embed_ref(E, ids, positions(ids, spec.pad_id), np.float32(orc.scale), orc.pos.numpy())
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ guards of the GPU test inputs
@pytest.mark.parametrize("max_nq", sorted(R.ATTN_LAYOUTS))
@pytest.mark.parametrize("pattern", R.ATTN_PATTERNS)
def test_guard_attn_tile_case(pattern, max_nq):
    """the launch has every nq of 1..max_nq, and the answer with the last key of a tile left out lies outside
    test_attn_tiles' bound on the same inputs"""
    c = R.attn_tile_case(pattern, max_nq)
    assert {g[1] for g in c["groups"]} == set(range(1, max_nq + 1))          # every wave of the launch owns rows
    assert any(g[1] == max_nq and g[3] >= 129 for g in c["groups"])
    a = (c["q"], c["k"], c["v"], c["groups"], c["heads"])
    ref, _ = R.attn_ref(*a)
    bound = R.attn_bound(*a)
    assert R.attn_excess(R.attn_wrong_drop_tile_end(*a), ref, bound) > 1.0


@pytest.mark.parametrize("t1", [1, 64, 65, 200, 448])
def test_guard_attn_ancestry_case(t1):
    """a tile gathered from the neighbouring beam, and every row read through row 0's ancestry, lie outside
    test_attn_ancestry's bound (t1 = 1: one key, whose beam is the only thing that can be wrong)"""
    c = R.attn_ancestry_case(t1)
    a = (c["q"], c["k"], c["v"], c["groups"], c["heads"], c["anc"], c["ld_anc"], c["tmax"])
    ref, _ = R.attn_ref(*a)
    bound = R.attn_bound(*a)
    assert R.attn_excess(R.attn_wrong_neighbour_tile(*a, c["n_rows"]), ref, bound) > 1.0
    assert R.attn_excess(R.attn_wrong_first_row_ancestry(c), ref, bound) > 1.0
    if t1 > 1:
        assert R.attn_excess(R.attn_wrong_drop_tile_end(*a), ref, bound) > 1.0


@pytest.mark.parametrize("k", R.TOPK_KS)
@pytest.mark.parametrize("vocab", R.TOPK_VOCABS)
def test_guard_topk_case(vocab, k):
    """ties to the larger index change the index lists test_topk asserts; logZ over the unbanned logits only moves a
    log-probability outside its bound"""
    x, ban, nban, k = R.topk_case(vocab, k)
    val, idx = R.topk_ref(x, k, ban, nban)
    _, idx_t = R.topk_ref(x, k, ban, nban, larger_index_on_tie=True)
    assert (idx_t != idx).any()
    val_m, _ = R.topk_ref(x, k, ban, nban, mask_bans_in_logz=True)
    live = np.isfinite(val)
    excess = np.abs(np.where(live, val_m, 0) - np.where(live, val, 0)) / R.topk_bound(x)[:, None]
    assert excess.max() > 1.0
    if vocab <= 80:                             # row 7: fewer than k eligible tokens
        assert (idx[7] == -1).any() and (idx[7] >= 0).sum() == min(k - 1, vocab)


@pytest.mark.parametrize("vocab,d,scaled", R.EMBED_CASES)
def test_guard_embed_case(vocab, d, scaled):
    """the neighbouring token row and the neighbouring position row lie outside test_embed's bound"""
    E, tok, pos, scale, sinpos = R.embed_case(vocab, d, scaled)
    ref = R.embed_ref(E, tok, pos, scale, sinpos)
    bound = R.embed_bound(E, tok, pos, scale, sinpos)
    for t, p in ((tok ^ 1, pos), (tok, np.minimum(pos + 1, len(sinpos) - 1))):
        wrong = R.embed_ref(E, t, p, scale, sinpos)
        assert (np.abs(wrong - ref) > bound).any(axis=1).sum() >= len(tok) - 2


@pytest.mark.parametrize("d,rows,tmax,t,wide", R.KV_CASES)
def test_guard_kv_case(d, rows, tmax, t, wide):
    """K and V swapped, slot t +- 1, cache row r + 1 and (where the buffer is wider and has more than one row) the source read at
    stride 3 d all differ in bits from the reference test_kv_append compares with; the reference itself writes the K / V thirds to
    slot t of rows 0 .. rows and leaves every other element as preset"""
    c = R.kv_case(d, rows, tmax, t, wide)
    kc, vc = R.kv_append_ref(c)
    q = c["qkv"].reshape(rows, c["ldqkv"])
    assert np.array_equal(kc[:rows, t], q[:, d:2 * d]) and np.array_equal(vc[:rows, t], q[:, 2 * d:3 * d])
    untouched = np.ones(kc.shape, bool)
    untouched[:rows, t] = False
    assert np.array_equal(kc[untouched], c["kc"][untouched]) and np.array_equal(vc[untouched], c["vc"][untouched])
    assert not np.array_equal(kc[:rows, t], c["kc"][:rows, t])                  # the preset differs from what is appended
    wrongs = R.kv_wrong_answers(c)
    assert {"swap", "row+1"} <= set(wrongs) and (tmax == 1 or {"t-1", "t+1"} & set(wrongs)) and (("ld=3d" in wrongs) == (wide and rows > 1))
    for name, (wk, wv) in wrongs.items():
        assert not np.array_equal(wk, kc) and not np.array_equal(wv, vc), name
    assert np.abs(q[:, :d].view(np.float16).astype(np.float32)).min() == 1000.0     # the Q third is garbage


@pytest.mark.parametrize("M,N,ld", R.RELU_CASES)
def test_guard_relu_case(M, N, ld):
    """the reference agrees with torch.relu on the live columns (no NaN among the inputs) except that it returns +0.0 for -0.0 as
    the kernel's compare does; a ReLU that keeps -0.0, one over all ld columns and one that skips the last 8-wide vector of a row
    differ in bits from it"""
    y = R.relu_case(M, N, ld)
    f = y.view(np.float16)
    assert not np.isnan(f.astype(np.float32)).any() and 0x8000 in y[:, :N] and 0x7c00 in y[:, :N] and 0xfc00 in y[:, :N]
    assert (y[0, :8] == R.RELU_SPECIALS[:8]).all() and (y[M - 1, N - 1] == 0x8000 or (M, N) == (1, 8))     # (one vector in all: the first eight)
    ref = R.relu_ref(y, N)
    want = torch.relu(torch.from_numpy(f[:, :N].astype(np.float32))).numpy().astype(np.float16).view(np.uint16)
    want[want == 0x8000] = 0                                                    # (torch keeps the sign of -0.0)
    assert np.array_equal(ref[:, :N], want) and np.array_equal(ref[:, N:], y[:, N:])
    assert not np.array_equal(R.relu_ref(y, N, keep_negative_zero=True), ref)
    assert not np.array_equal(R.relu_ref(y, N - 8), ref) if N > 8 else ref[0, 0] == 0
    if ld > N:
        assert (y[:, N:] & 0x8000).any() and not np.array_equal(R.relu_ref(y, ld), ref)


# ------------------------------------------------------------------ shape checks of the hooks (host side, no device touched)
@pytest.fixture(scope="module")
def lib():
    from whisperlive_amd import _lib
    _lib.build()
    return _lib.load()


def _attn_args(**kw):
    rng = np.random.default_rng(4)
    c = dict(q=R._f16(rng.standard_normal((20, 64))), k=R._f16(rng.standard_normal((40, 64))), v=R._f16(rng.standard_normal((40, 64))),
             o=np.zeros((20, 64), np.float16), groups=[(0, 4, 0, 40)], max_nq=4, heads=1, anc=None, ld_anc=0, tmax=0)
    c.update(kw)
    return c


@pytest.mark.parametrize("bad", [
    dict(max_nq=17, groups=[(0, 17, 0, 40)]),                 # more rows than four waves of four
    dict(max_nq=0),
    dict(max_nq=4, groups=[(0, 5, 0, 40)]),                   # nq > max_nq: rows past 4 would be dropped
    dict(max_nq=8, groups=[(0, 9, 0, 40)]),
    dict(groups=[(0, 4, 1, 40)]),                             # key rows past K / V
    dict(groups=[(0, 4, 0, 0)]),
    dict(groups=[(17, 4, 0, 8)]),                             # query rows past Q / O
    dict(heads=2),                                            # strides narrower than heads * 64
    dict(groups=[(0, 1, 0, 9)], anc=np.full((1, 8), 0, np.int32), ld_anc=8, tmax=8),   # nk > tmax / ld_anc
    dict(groups=[(0, 1, 0, 8)], anc=np.full((1, 8), 5, np.int32), ld_anc=8, tmax=8),   # ancestry row 5 * 8 + j >= 40
    dict(groups=[(0, 1, 0, 8)], anc=np.full((1, 8), -1, np.int32), ld_anc=8, tmax=8),
])
def test_attn_hook_rejects_shapes_the_launcher_cannot_serve(lib, bad):
    rc, _ = R.run_attn(_attn_args(**bad))
    assert rc == 1, lib.wlx_last_error()


@pytest.mark.parametrize("vocab,k,nban", [(64, 0, None), (64, 33, None), (72, 4, None), (64 * 4096 + 16, 4, None),
                                          (64, 4, [3]), (64, 4, [-1])])
def test_topk_hook_rejects_shapes_the_launcher_cannot_serve(lib, vocab, k, nban):
    x = np.zeros((1, vocab), np.float32)
    ban = np.zeros((1, 2), np.int32)
    rc, _, _ = R.run_topk(x, k, ban if nban else None, np.array(nban, np.int32) if nban else None)
    assert rc == 1, lib.wlx_last_error()


def test_embed_hook_rejects_tokens_and_positions_outside_the_tables(lib):
    E = np.zeros((32, 64), np.float32)
    sp = np.zeros((10, 64), np.float32)
    for tok, pos in (([32], [0]), ([-1], [0]), ([0], [10]), ([0], [-1])):
        rc, _ = R.run_embed(E, np.array(tok), np.array(pos), 1.0, sp)
        assert rc == 1, lib.wlx_last_error()
    rc, _ = R.run_embed(np.zeros((32, 48), np.float32), np.array([0]), np.array([0]), 1.0, np.zeros((10, 48), np.float32))
    assert rc == 1
