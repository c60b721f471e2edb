"""GPU tests of the translation engine's row kernels (csrc/mt.hip), one launch each through wlx_mt_debug_kv_append
(mt_kv_append_kernel, the only writer of the decoder self-attention cache) and wlx_mt_debug_relu (mt_relu_kernel, in place on the
fused FFN layout). Both move bits: the results are compared as uint16 with the references of tests/mt_kernel_ref.py, including
every element the kernel must leave alone — no tolerance. tests/test_mt_kernel_ref.py shows that the nearest wrong answers differ
from those references on the same inputs."""
from __future__ import annotations

import numpy as np
import pytest

from . import mt_kernel_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,rows,tmax,t,wide", R.KV_CASES)
def test_kv_append(d, rows, tmax, t, wide):
    """destination (r tmax + t) d and source qkv + r ldqkv + d / + 2 d: slot t of cache rows 0 .. rows holds the K / V thirds bit for
    bit and every other element of both caches (other slots, the spare row) keeps its preset. K and V swapped, slot t +- 1, row
    r + 1 or a source stride of 3 d under a wider buffer would each differ (test_guard_kv_case); the +-1000 of the Q third and of the
    padding columns must not appear."""
    c = R.kv_case(d, rows, tmax, t, wide)
    rc, kc, vc = R.run_kv_append(c)
    assert rc == 0
    want_k, want_v = R.kv_append_ref(c)
    for name, got, want in (("K", kc, want_k), ("V", vc, want_v)):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name} cache: {len(bad)} elements differ, the first at (row, slot, column) {tuple(bad[0])}"


def _kv_small():
    return R.kv_case(64, 2, 5, 2, True)


@pytest.mark.parametrize("what,over", [
    ("d % 8", dict(d=60)), ("d = 0", dict(d=0)), ("ldqkv < 3 d", dict(ldqkv=3 * 64 - 8)), ("ldqkv % 8", dict(ldqkv=3 * 64 + 4)),
    ("t = -1", dict(t=-1)), ("t = tmax", dict(t=5)), ("tmax = 0", dict(tmax=0, t=0)), ("rows > cache_rows", dict(rows=4)),
    ("rows = 0", dict(rows=0)), ("null qkv", dict(qkv=None)), ("null Kc", dict(kc=None)), ("null Vc", dict(vc=None))])
def test_kv_append_refusals(what, over):
    """(rows = 4 against 3 cache rows would write past the cache; the hook only ever reads `rows` rows of qkv, so the two-row buffer
    is never read past either: the call is refused before any copy)"""
    c = _kv_small()
    rc, kc, vc = R.run_kv_append(c)
    assert rc == 0 and np.array_equal(kc, R.kv_append_ref(c)[0])
    rc, kc, vc = R.run_kv_append(c, **over)
    assert rc == 1, what
    assert (kc is None or np.array_equal(kc, c["kc"])) and (vc is None or np.array_equal(vc, c["vc"])), what


@pytest.mark.parametrize("M,N,ld", R.RELU_CASES)
def test_relu(M, N, ld):
    """M N / 8 vectors below 256, above it and off its multiples; ld > N as the fused layouts launch it. Bit for bit: negative values,
    -inf, negative subnormals and -0.0 become +0.0; +inf, positive subnormals and normals stay; the columns N .. ld, negative values
    among them, come back untouched. NaN is left out: the kernel's `v > 0 ? v : 0` maps it to 0 where torch.relu keeps it, and no
    product input is NaN."""
    y = R.relu_case(M, N, ld)
    rc, got = R.run_relu(y, N)
    assert rc == 0
    want = R.relu_ref(y, N)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} elements differ, the first at (row, column) {tuple(bad[0])}: {got[tuple(bad[0])]:#06x} for {want[tuple(bad[0])]:#06x}"
    assert np.array_equal(got[:, N:], y[:, N:])


@pytest.mark.parametrize("what,over", [("N % 8", dict(N=60)), ("N = 0", dict(N=0)), ("ld < N", dict(N=72)), ("ld % 8", dict(ld=68, M=2)),
                                       ("M = 0", dict(M=0)), ("null y", dict(y=None, ld=64, M=3))])
def test_relu_refusals(what, over):
    y = R.relu_case(3, 64, 64)
    a = dict(y=y, N=64)
    rc, got = R.run_relu(**a)
    assert rc == 0 and np.array_equal(got, R.relu_ref(y, 64))
    a.update(over)
    rc, got = R.run_relu(**a)
    assert rc == 1, what
    assert got is None or np.array_equal(got, y), what
