"""CPU tests of the long form of the offline clustering: include/wlx_spk_long.h against the binding table, the symbols in the library,
and the route FileDiarizer.cluster_windows takes by window count and by what the embedder has."""
import ctypes
import os
import re

import numpy as np
import pytest

from whisperlive_amd import _lib
from whisperlive_amd.file_diarization import FileDiarizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_names_are_the_binding_table_and_the_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlx_spk_long.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(wlx_[a-z_0-9]+)\s*\(", src))) == sorted(_lib.EXPORTS_SPK_LONG)
    assert int(re.search(r"#define\s+WLX_SPK_LONG_MAX\s+(\d+)", src).group(1)) == _lib.SPK_LONG_MAX == 8192
    assert '#include "wlx_spk_long.h"' in open(os.path.join(ROOT, "include", "wlx.h")).read()
    lib = ctypes.CDLL(str(_lib.build()))
    assert all(hasattr(lib, name) for name in _lib.EXPORTS_SPK_LONG)


class Resident:
    slot, item = object(), 0


class Scripted:
    """an embedder that records which route was taken; embed_resident gives two orthogonal rows in turn"""

    def __init__(self):
        self.calls = []

    def diarize_resident(self, slot, item, ranges, threshold, max_clusters):
        self.calls.append("short")
        return np.zeros(len(ranges), np.int32), np.ones((1, 2), np.float32)

    def embed_resident(self, slot, item, ranges):
        self.calls.append("host")
        return [np.eye(2, dtype=np.float32)[i % 2] for i in range(len(ranges))]


class ScriptedLong(Scripted):
    def diarize_resident_long(self, slot, item, ranges, threshold, max_clusters):
        self.calls.append("long")
        return np.zeros(len(ranges), np.int32), np.ones((1, 2), np.float32)


@pytest.mark.parametrize("embedder,n,route", [(ScriptedLong, 2048, "short"), (ScriptedLong, 2049, "long"), (ScriptedLong, 8192, "long"),
                                              (ScriptedLong, 8193, "host"), (Scripted, 2049, "host")])
def test_cluster_windows_route(embedder, n, route, monkeypatch):
    from whisperlive_amd import file_diarization as FD
    # (the oracle is not what is under test here: at 8193 rows it would take a quarter of a minute)
    monkeypatch.setattr(FD, "cluster_host", lambda X, thr, cap: FD.Clustering(np.arange(len(X), dtype=np.int32) % 2, None, None, X[:2]))
    e = embedder()
    labels, centroids = FileDiarizer(e).cluster_windows(Resident(), [(80 * i, 24000, i) for i in range(n)])
    assert e.calls == [route] and len(labels) == n and centroids is not None
