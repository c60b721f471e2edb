"""Host tests of the argument head's build (whisperlive_amd/_lib.py, csrc/dec_gemv_internal.h WLX_KERNARG_HEAD).
What the compiler made: every dec_gemv2_kernel of the built library reports a non-zero kernel-argument preload length in its kernel
descriptor (14 dwords: the whole head), so do the flat-list kernels of the step (decoder.hip, search.hip), nothing else does, and dec_gemv.hip compiled as the A/B build
(-DWLX_KERNARG_HEAD=0, no preload option) reports zero everywhere (tests/kernarg_preload_reader.py reads the descriptors).
What the build asks for: the preload option goes to those three translation units only, the A/B build carries it nowhere,
and a compiler that rejects one of the two hidden options loses that one alone (the compiler is replaced by a recorder there)."""
import subprocess
from pathlib import Path

import pytest

from whisperlive_amd import _lib

from . import kernarg_preload_reader as R


def test_every_decode_projection_kernel_is_preloaded_and_nothing_else():
    lib = _lib.build()
    if _lib._preload_ok is False:
        pytest.fail("this hipcc rejected the preload option: the library was built without it")
    lens = R.file_preload_lengths(lib)
    g2 = {k: v for k, v in lens.items() if "16dec_gemv2_kernelI" in k}       # (mangled: the instantiations of the template)
    assert len(g2) >= 100, len(g2)
    assert all(v == 14 for v in g2.values()), sorted(set(g2.values()))
    # the flat-list kernels of the step (decoder.hip, search.hip: compiled with the option, argument lists as they stand)
    for listed in ("dec_self_attn2_kernel", "dec_cq_cross_attn_kernel", "search_scan3_kernel", "search_merge_update3_kernel"):
        hit = {k: v for k, v in lens.items() if listed in k}
        assert hit and all(v > 0 for v in hit.values()), (listed, hit)
    # nothing outside those three translation units: the vocabulary projection (one by-value struct), encoder, VAD, MT, speaker kernels
    ours = ("dec_embed_kernel", "dec_cross_attn_kernel", "dec_xattn_combine_kernel", "dec_align_scores_kernel", "dec_self_attn2_kernel",
            "dec_cq_cross_attn_kernel", "search_", "token_prob", "lang_probs_kernel")
    other = {k: v for k, v in lens.items() if k not in g2 and v and not any(o in k for o in ours)}
    assert not other, other
    assert all(v == 0 for k, v in lens.items() if "dec_vocab_kernel" in k)


def test_the_ab_object_preloads_nothing(tmp_path):
    cached = _lib.CSRC / ".obj" / "base_WLX_KERNARG_HEAD-0" / "dec_gemv.hip.o"
    src = _lib.CSRC / "dec_gemv.hip"
    deps = [src] + list(_lib.CSRC.glob("*.h"))
    if cached.exists() and all(cached.stat().st_mtime >= d.stat().st_mtime for d in deps):
        obj = cached
    else:                                        # (device code only: the descriptors are all the test reads)
        obj = tmp_path / "dec_gemv_nohead.co"
        subprocess.run([_lib._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-DWLX_KERNARG_HEAD=0",
                        "-c", str(src), "-o", str(obj)], check=True, capture_output=True)
    blob = obj.read_bytes()
    lens = R.file_preload_lengths(obj) or R.preload_lengths(blob)               # (a host object with its bundle, or the bare code object)
    assert len(lens) >= 100 and not any(lens.values()), {k: v for k, v in lens.items() if v}


def _recorded_build(monkeypatch, tmp_path, defines, reject=()):
    (tmp_path / "dummy.h").write_text("")
    monkeypatch.setattr(_lib, "CSRC", tmp_path)
    monkeypatch.setattr(_lib, "_hipcc", lambda: "hipcc")
    monkeypatch.setattr(_lib, "_extra_ok", None)
    monkeypatch.setattr(_lib, "_preload_ok", None)
    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(list(cmd))
        for flag in reject:
            if any(flag in a for a in cmd):
                return subprocess.CompletedProcess(cmd, 1, "", "clang (LLVM option parsing): Unknown command line argument '-%s=1'" % flag)
        Path(cmd[cmd.index("-o") + 1]).write_bytes(b"")
        return subprocess.CompletedProcess(cmd, 0, "", "")

    monkeypatch.setattr(_lib.subprocess, "run", fake_run)
    _lib._compile(tmp_path / "lib.so", defines, force=True)
    return {Path(c[c.index("-c") + 1]).name: c for c in cmds if "-c" in c}


def test_preload_option_goes_to_the_decode_projections_only(monkeypatch, tmp_path):
    by_src = _recorded_build(monkeypatch, tmp_path, ())
    assert set(by_src) == set(_lib.SOURCES)
    flag = _lib.KERNARG_PRELOAD[1]
    assert flag.startswith("-amdgpu-kernarg-preload-count=") and 1 <= int(flag.split("=")[1]) <= 14   # 16 user SGPRs less the kernel-argument pointer
    for src, cmd in by_src.items():
        assert (flag in cmd) == (src in _lib.KERNARG_PRELOAD_SOURCES), src
    assert set(_lib.KERNARG_PRELOAD_SOURCES) == {"dec_gemv.hip", "decoder.hip", "search.hip"}


def test_the_ab_build_has_no_preload(monkeypatch, tmp_path):
    by_src = _recorded_build(monkeypatch, tmp_path, ["WLX_KERNARG_HEAD=0"])
    for src, cmd in by_src.items():
        assert "-DWLX_KERNARG_HEAD=0" in cmd, src
        assert not any("kernarg-preload" in a for a in cmd), src


@pytest.mark.parametrize("reject,kept", [("amdgpu-kernarg-preload-count", "amdgpu-mfma-vgpr-form"), ("amdgpu-mfma-vgpr-form", "amdgpu-kernarg-preload-count")])
def test_a_rejected_option_goes_alone(monkeypatch, tmp_path, capsys, reject, kept):
    by_src = _recorded_build(monkeypatch, tmp_path, (), reject=(reject,))      # (the last command per source: the build that went through)
    assert not any(reject in a for c in by_src.values() for a in c)
    assert any(kept in a for a in by_src["dec_gemv.hip"])
    assert reject in capsys.readouterr().out
