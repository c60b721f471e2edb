"""CPU tests of the host side of batched word alignment: add_word_timestamps' align_many_fn route gives the words of the align_fn
route with ONE call for all windows that have text, and the four new C-ABI symbols agree between include/wlx.h, the binding's export
list and its argtypes."""
import copy
import ctypes as C
import os
import re

import numpy as np

from whisperlive_amd import word_timing as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT = 1000


class FakeTokenizer:
    """one word per token; token t spells ' w<t>', ids >= EOT are specials"""
    eot = EOT

    def split_to_word_tokens(self, tokens):
        return [f" w{t}" if t < EOT else "" for t in tokens], [[t] for t in tokens]


def fake_align(text_tokens, num_frames, window):
    """a deterministic per-window alignment: token k enters at frame 3 * k + window, two path steps per token"""
    n = len(text_tokens) + 1
    ti = np.repeat(np.arange(n), 2)
    fi = np.minimum(3 * ti + window + np.tile([0, 1], n), max(1, num_frames // 2) - 1 + 3 * n)
    probs = np.asarray([0.5 + 0.001 * (t % 97) + 0.01 * window for t in text_tokens], dtype=np.float64)
    return ti, fi, probs


def windows():
    mk = lambda seek, toks, a, b: dict(seek=seek, tokens=toks, start=a, end=b)
    return [[mk(0, [5, 6, 7, EOT + 3], 0.0, 1.2), mk(0, [8, 9], 1.2, 2.0)],
            [mk(3000, [EOT + 1, EOT + 2], 30.0, 30.5)],                          # nothing but specials: no alignment for this window
            [mk(6000, [11, 12, 13, 14, 15], 60.0, 62.5)]]


def test_align_many_route_gives_the_words_of_the_align_fn_route_in_one_call():
    tok = FakeTokenizer()
    args = (tok,), (1500, 50, 100, "\"'“¿([{-", "\"'.。,，!！?？:：”)]}、", 0.0)
    a = windows()
    calls = []

    def align_fn(text_tokens, num_frames, window):
        calls.append(window)
        return fake_align(text_tokens, num_frames, window)

    last_a = wt.add_word_timestamps(a, *args[0], align_fn, *args[1])
    assert calls == [0, 2]
    b = windows()
    many_calls = []

    def align_many_fn(requests):
        many_calls.append(copy.deepcopy(requests))
        return [fake_align(*rq) for rq in requests]

    def never(*_):
        raise AssertionError("align_fn called although align_many_fn was given")

    last_b = wt.add_word_timestamps(b, *args[0], never, *args[1], align_many_fn=align_many_fn)
    assert len(many_calls) == 1
    assert many_calls[0] == [([5, 6, 7, 8, 9], 1500, 0), ([11, 12, 13, 14, 15], 1500, 2)]
    assert a == b and last_a == last_b
    assert all("words" in sub for w in b for sub in w) and b[1][0]["words"] == [] and len(b[2][0]["words"]) == 5


def test_align_many_is_not_called_without_text():
    tok = FakeTokenizer()
    segs = [[dict(seek=0, tokens=[EOT + 1], start=0.0, end=1.0)]]
    called = []
    wt.add_word_timestamps(segs, tok, None, 1500, 50, 100, "", "", 0.0, align_many_fn=lambda rq: called.append(rq) or [])
    assert called == [] and segs[0][0]["words"] == []


# ---- ABI: header, export list and argtypes of the new symbols
NEW = ("wlx_align_batch", "wlx_debug_dtw", "wlx_debug_align_post", "wlx_debug_align_timings")


def header_prototypes():
    src = open(os.path.join(ROOT, "include", "wlx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(wlx_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def ctype_of(decl: str):
    decl = re.sub(r"\bconst\b", "", decl).strip()
    stars = decl.count("*")
    base = re.match(r"[a-z_0-9]+", decl).group(0)
    if stars == 0:
        return {"int32_t": C.c_int32, "int64_t": C.c_int64}[base]
    assert stars == 1, decl
    return {"int32_t": C.POINTER(C.c_int32), "float": C.POINTER(C.c_float), "wlx_engine": C.c_void_p}[base]


def test_new_symbols_agree_between_header_binding_list_and_argtypes():
    from whisperlive_amd import _lib
    protos = header_prototypes()
    path = _lib.build()
    lib = C.CDLL(str(path))
    src = open(os.path.join(ROOT, "whisperlive_amd", "_lib.py")).read()
    ns = dict(vp=C.c_void_p, i32=C.c_int32, i64=C.c_int64, f32p=C.POINTER(C.c_float), i32p=C.POINTER(C.c_int32))
    for name in NEW:
        assert name in protos, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
        m = re.search(r"lib\.%s\.argtypes = (\[[^\]]*\])" % name, src)
        assert m, name
        bound = eval(m.group(1), dict(ns))
        want = [ctype_of(a) for a in protos[name]]
        assert bound == want, (name, bound, want)
    hdr = open(os.path.join(ROOT, "include", "wlx.h")).read()
    assert re.search(r"#define\s+WLX_ALIGN_MAX_BATCH\s+64\b", hdr) and _lib.ALIGN_MAX_BATCH == 64
    assert re.search(r"#define\s+WLX_ALIGN_MAX_MEDIAN\s+15\b", hdr) and _lib.ALIGN_MAX_MEDIAN == 15
