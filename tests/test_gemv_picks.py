"""Host-only (-m "not gpu"): which `dec_gemv2_kernel` / `dec_vocab_kernel` instantiation the launcher picks for every decode projection
of the Whisper family — the rules of `csrc/dec_gemv.hip gemv2_cfg` as round 6 left them (DESIGN.md §7.3 logs G5, G7-G10), pinned so that
a change of the search loop shows up here before it shows up as a slower step or, as it did once that round, as a launch past its bound.

`scripts/gemv_pick_probe.cpp` is compiled for the HOST (hipcc, no device code) and linked against the production `libwlx.so`.
`wlx::dec_gemv_kernel_name` is the name leaf of `dec_gemv.hip gemv2_dispatch` / `dec_vocab.hip vocab2_dispatch`, the one walk per family that the eligibility
probe (`dec_gemv_is_lean`, `dec_gemv_slab_split`) and the launch go through as well: it prints the template arguments
<CH, LNV, IN, OUT, NTB, MT, XS> of the instantiation that runs. CH = k-tiles per wave (so K / 32 / CH waves stream the weights),
IN 0 = LayerNorm-fronted, 1 = fp16 rows in, 2 = split combine. No kernel is launched and no GPU is needed.

Two layers: 27 named picks of the Whisper models (EXPECTED), and the probe's `--sweep` — every (in, out, xsrc) combination, the ones the
lean kernels refuse included, over 63 row counts, the family's and four other widths, with and without bias / busy device / slab pointer /
K slices — compared point for point with `tests/golden/gemv_pick_sweep.txt.gz`: the answers of the commit before the dispatch became one
walk, recorded by linking the probe against that commit's library. A change of a pick is then a change of that file, made on purpose
(`gemv_pick_probe --sweep | gzip -9n`)."""
import gzip
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

# what one stream's step (<= 8 rows, Mtot == 0) runs, per projection
EXPECTED = {
    # fp16 rows in (attention output projection; K-split MLP output projection; the one that also adds the slabs): few waves, long K slices (G5)
    "small o-proj M5": "dec_gemv2_kernel<12, 1, 1, 3, 1, 1, 0>",
    "small fc2 slab M5": "dec_gemv2_kernel<12, 1, 1, 5, 1, 1, 0>",
    "small o-proj slabs M5": "dec_gemv2_kernel<12, 1, 1, 3, 1, 1, 1>",
    "medium o-proj M5": "dec_gemv2_kernel<8, 1, 1, 3, 1, 1, 0>",
    "medium fc2 slab M5": "dec_gemv2_kernel<8, 1, 1, 5, 1, 1, 0>",
    "large o-proj M5": "dec_gemv2_kernel<10, 1, 1, 3, 1, 1, 0>",
    "large fc2 slab M5": "dec_gemv2_kernel<10, 1, 1, 5, 1, 1, 0>",
    "base o-proj M5": "dec_gemv2_kernel<8, 1, 1, 3, 1, 1, 0>",
    "tiny o-proj M5": "dec_gemv2_kernel<12, 1, 1, 3, 1, 1, 0>",
    # the split combine keeps four waves of six / eight of five (G5: wider lost)
    "small xattn M5": "dec_gemv2_kernel<6, 1, 2, 3, 1, 1, 0>",
    "large xattn M5": "dec_gemv2_kernel<5, 1, 2, 3, 1, 1, 0>",
    # LayerNorm-fronted on PLAIN rows: four waves (G7, G8, G10)
    "small mlp-up M5": "dec_gemv2_kernel<6, 3, 0, 1, 1, 1, 0>",
    "medium mlp-up M5": "dec_gemv2_kernel<8, 4, 0, 1, 1, 1, 0>",
    "large mlp-up M5": "dec_gemv2_kernel<10, 5, 0, 1, 2, 1, 0>",
    "large q-proj M5": "dec_gemv2_kernel<10, 5, 0, 0, 1, 1, 0>",
    # a layer's first projection (rows + slabs / embedding rows): one row per wave for K = 768, four waves with both rows of a wave
    # requested together for K = 1024 / 1280 (G9)
    "small qkv slabs M5": "dec_gemv2_kernel<4, 3, 0, 4, 1, 1, 1>",
    "small qkv embed M5": "dec_gemv2_kernel<4, 3, 0, 4, 1, 1, 2>",
    "medium qkv slabs M5": "dec_gemv2_kernel<8, 4, 0, 4, 1, 1, 1>",
    "large qkv slabs M5": "dec_gemv2_kernel<10, 5, 0, 4, 1, 1, 1>",
    # batched rows (row tiles, Mtot > 0) and 9..16 rows of the LayerNorm-fronted launches keep the narrow slices
    "small o-proj M60": "dec_gemv2_kernel<6, 1, 1, 3, 1, 1, 0>",
    "small fc2 slab M60": "dec_gemv2_kernel<6, 1, 1, 5, 1, 1, 0>",
    "small mlp-up M60": "dec_gemv2_kernel<6, 3, 0, 1, 4, 1, 0>",
    "large mlp-up M16": "dec_gemv2_kernel<5, 5, 0, 1, 2, 1, 0>",
    "large qkv slabs M16": "dec_gemv2_kernel<5, 5, 0, 4, 1, 1, 1>",
    # 16 rows of an UNSPLIT K = 4096 projection: eight waves of eight k-tiles twice over (sixteen waves would pass the 512-thread bound
    # of the wide instantiations: 'unspecified launch failure', profiles/r6ap_*)
    "medium fc2 resid M16": "dec_gemv2_kernel<8, 1, 1, 3, 1, 1, 0>",
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not found")
    from whisperlive_amd import _lib
    lib = _lib.build()                                       # (fresh in-tree library: returned as it is)
    exe = tmp_path_factory.mktemp("probe") / "gemv_pick_probe"
    cmd = [hipcc, "-std=c++17", "-O1", str(ROOT / "scripts" / "gemv_pick_probe.cpp"), "-o", str(exe),
           f"-L{lib.parent}", f"-l:{lib.name}", f"-Wl,-rpath,{lib.parent}"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def picks(probe):
    out = subprocess.run([str(probe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        what, rest = line[:24].strip(), line[24:]
        got[what] = (rest.split("  ")[-1].strip(), "lean=1" in rest, rest)
    return got


def test_every_probed_projection_runs_on_the_lean_kernel(picks):
    assert len(picks) >= len(EXPECTED)
    for what, (name, lean, rest) in picks.items():
        assert lean and name.startswith("dec_gemv2_kernel<"), (what, rest)


@pytest.mark.parametrize("what", sorted(EXPECTED))
def test_pick(picks, what):
    assert what in picks, sorted(picks)
    assert picks[what][0] == EXPECTED[what], (what, picks[what][2])


def test_k_split_of_the_mlp_output_projection(picks):
    """two K slices for one stream's rows and for row tiles; none for the 16-row unsplit case the probe lists"""
    assert "slab_split=2" in picks["small fc2 slab M5"][2] and "slab_split=2" in picks["large fc2 slab M5"][2]
    assert "slab_split=0" in picks["medium fc2 resid M16"][2]


# ---------------------------------------------------------------- the whole decision space
GOLDEN = ROOT / "tests" / "golden" / "gemv_pick_sweep.txt.gz"


def _parse_sweep(text):
    """-> (row counts, {series key: [(slab_split, lean, kernel name) per row count]}); the line format: scripts/gemv_pick_probe.cpp"""
    lines = text.splitlines()
    assert lines and lines[0].startswith("M "), lines[:1]
    ms = [int(m) for m in lines[0].split()[1:]]
    at = {m: i for i, m in enumerate(ms)}
    series = {}
    for line in lines[1:]:
        key, *runs = line.split("|")
        answers = []
        for run in runs:
            span, answer = run.split(":", 1)
            first, last = (int(m) for m in span.split("-"))
            split, lean, name = answer.split(",", 2)
            answers += [(int(split), int(lean), name)] * (at[last] - at[first] + 1)
        assert len(answers) == len(ms) and key not in series, line
        series[key] = answers
    return ms, series


def _point(key, m):
    i, o, x, k, n, *flags = key.split()
    return f"(in={i}, out={o}, xsrc={x}, M={m}, K={k}, N={n}, flags={' '.join(flags)})"


@pytest.fixture(scope="module")
def sweep(probe):
    out = subprocess.run([str(probe), "--sweep"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return _parse_sweep(out.stdout)


def test_sweep_equals_the_recorded_answers(sweep):
    ms, got = sweep
    with gzip.open(GOLDEN, "rt") as f:
        want_ms, want = _parse_sweep(f.read())
    assert ms == want_ms
    assert list(got) == list(want), sorted(set(got) ^ set(want))[:5]
    assert len(want) >= 54 * 9 * 7 * 8                                   # every combination x width x shape x flag set is in the file
    for key, answers in want.items():
        if got[key] == answers:
            continue
        for m, g, w in zip(ms, got[key], answers):
            assert g == w, f"{_point(key, m)}: (slab_split, lean, kernel) is {g}, recorded {w}"


def test_sweep_lean_answer_and_kernel_name_agree(sweep):
    """what engine_decode.hip decoder_pass asks before it builds a pass (lean?) and what the profiling hook filters by (the name) are one answer"""
    ms, got = sweep
    n_lean = 0
    for key, answers in got.items():
        for m, (split, lean, name) in zip(ms, answers):
            if lean:
                n_lean += 1
                assert name.startswith(("dec_gemv2_kernel<", "dec_vocab_kernel<")), (_point(key, m), name)
            else:
                assert name.startswith("dec_gemv_kernel<"), (_point(key, m), name)
    assert n_lean > 10000                                                # (the sweep does reach the lean kernels)


def test_sweep_slab_split_implies_a_lean_k_split_launch(sweep):
    """dec_gemv_slab_split(M, K, N) = KS != 0 promises that fp16 rows in -> GEMV_OUT_SLAB with KTS = K / 32 / KS runs on the lean kernel:
    the engine splits the MLP output projection on that answer, and the first-generation kernel does not know GEMV_OUT_SLAB"""
    ms, got = sweep
    n_split = 0
    for key, answers in got.items():
        i, o, x, k, n, b, u, s, kts = key.split()
        if (i, o, x, b) != ("1", "5", "0", "b1"):                        # (GEMV_IN_F16, GEMV_OUT_SLAB, GEMV_X_PLAIN, with a bias)
            continue
        for m, (split, lean, name) in zip(ms, answers):
            if split and kts == f"k{int(k) // 32 // split}":
                n_split += 1
                assert lean and name.startswith("dec_gemv2_kernel<") and ", 1, 5, " in name, (_point(key, m), split, lean, name)
    assert n_split > 100
    for key, answers in got.items():                                     # the split is a function of (M, K, N) alone
        ref = got[" ".join(["1", "5", "0"] + key.split()[3:5] + ["b1", "u0", "s0", "k0"])]
        assert [a[0] for a in answers] == [a[0] for a in ref], key
