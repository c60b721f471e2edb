"""bench.py's measurement plumbing that can be checked without a GPU: the FETCH_SIZE reduction with its in-pass calibration (VERDICT r04
weak 4: the factor was 'calibrated' on the wrong kernel and nothing asserted on it), the decode-step byte model, the CPU-baseline leg on
a tiny model (median of several runs on pinned threads, fp32 and int8 ports)."""
import os

import numpy as np
import pytest

import bench


def test_fetch_reduction_calibrates_on_the_vocabulary_projection_and_refuses_a_bad_factor():
    vocab_bytes = 2.0 * 51864 * 768                     # Whisper-small.en: 79.66 MB streamed once per launch
    raw_vocab = vocab_bytes / 2048.0                    # what FETCH_SIZE reports (KiB) when 128-byte requests are tallied at 64 B
    per = {
        "void wlx::dec_vocab_kernel<24, 6, 1, true>(wlx::VocabParams)": [raw_vocab * 13, 13],
        "void wlx::dec_gemv2_kernel<6, 1, 1, 5, 1, 1, 0>(wlx::GemvParams)": [2461.0 * 143, 143],      # round 4 calibrated on THIS one: 31.6
        "_ZN3wlx24dec_cq_cross_attn_kernelILi3ELi4EEEvPKfl": [3205.0 * 156, 156],
    }
    got, src, extra = bench.reduce_fetch_pass(per, "dec_cq_cross_attn_kernel", vocab_bytes)
    assert abs(got - 3205.0 * 2048.0) < 1.0 and "156 launches" in src
    cal = extra["calibration"]
    assert "dec_vocab_kernel" in cal["kernel"] and abs(cal["bytes_per_raw_kib_over_1024"] - 2.0) < 1e-9 and cal["launches"] == 13
    # a pass in which the conversion does not hold (e.g. the counter tallies full requests): the figure is withheld, with the reason
    per_bad = dict(per)
    per_bad["void wlx::dec_vocab_kernel<24, 6, 1, true>(wlx::VocabParams)"] = [2.0 * raw_vocab * 13, 13]
    got, src, extra = bench.reduce_fetch_pass(per_bad, "dec_cq_cross_attn_kernel", vocab_bytes)
    assert got is None and "outside [1.8, 2.2]" in src and abs(extra["calibration"]["bytes_per_raw_kib_over_1024"] - 1.0) < 1e-9
    # no vocabulary projection in the pass: not calibrated, not reported
    got, src, extra = bench.reduce_fetch_pass({k: v for k, v in per.items() if "vocab" not in k}, "dec_cq_cross_attn_kernel", vocab_bytes)
    assert got is None and "not calibrated" in src
    got, src, _ = bench.reduce_fetch_pass(per, "no_such_kernel", vocab_bytes)
    assert got is None and "no FETCH_SIZE rows" in src


def test_decode_step_bytes_matches_survey_8d():
    from whisperlive_amd.specs import get_spec
    sp = get_spec("small.en")
    b = bench.decode_step_bytes(sp, 5, 33)
    # 277.9 MB of weights + 55.3 MB of cross K/V + the self-attention cache at t
    weights = 2 * (12 * (6 * 768 * 768 + 2 * 768 * 3072) + 51864 * 768)
    assert abs(weights - 277.9e6) / 277.9e6 < 0.01
    assert b == weights + 2 * 12 * 2 * 1500 * 768 + 2 * 12 * 2 * 33 * 768 * 5
    assert 333e6 < b < 340e6
    assert abs(bench.encoder_flops(sp) - 386.6e9) / 386.6e9 < 0.01


def test_cpu_baseline_leg_on_a_tiny_model():
    from oracle import logmel as olm
    from whisperlive_amd.specs import WhisperSpec
    from whisperlive_amd.weights import random_weights
    spec = WhisperSpec(n_mels=80, d_model=128, n_heads=2, enc_layers=1, dec_layers=1, ffn=512, vocab=2310)
    w = bench.f16_rounded(random_weights(spec, seed=0))
    ids = bench.token_ids(spec.vocab)
    pcm = olm.speech_like_pcm(30.0, seed=1)
    aff = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
    base, toks = bench.cpu_baseline(spec, w, pcm, ids, 6, 6, threads=2, repeats=3)
    # 3 runs, more (at most 6) while the last three disagree by more than 15 %; the figure is the median of the LAST three
    assert base["kind"] == "port" and 3 <= base["runs"] <= 6 and len(base["window_s_all_runs"]) == base["runs"] and base["cores"] == 2
    assert base["value"] == pytest.approx(30.0 / sorted(base["window_s_all_runs"][-3:])[1], rel=2e-2)      # the MEDIAN of the last three
    assert base["runs"] == 6 or base["spread"] <= 0.15
    assert f"median of the last 3 of {base['runs']} runs on 2 pinned threads" in base["sample"] and "measured in full" in base["sample"] and len(toks) == 6
    q8, toks8 = bench.cpu_baseline(spec, w, pcm, ids, 3, 6, threads=2, int8="fbgemm")
    assert q8["kind"] == "port-int8" and "scaled to 6" in q8["sample"] and len(toks8) == 3
    if aff is not None:
        assert os.sched_getaffinity(0) == aff          # the pinning is undone


def test_dump_outputs_writes_every_window_and_caps_the_dense_arrays(tmp_path):
    """--dump-outputs: tokens / scores / no-speech probabilities of every window in float64, log-mel and encoder output of the
    first windows that fit the budget in float32, the whole dump under 64 MB"""
    class Slot:
        def features(self, b):
            return np.full((80, 3001), b, np.float32)

        def encoder_output(self, b):
            return np.full((1500, 768), -b, np.float32)
    sl = Slot()
    results = [([7, 8, 9][: 1 + b % 3], -0.25 * b, 0.01 * b) for b in range(16)]
    bench.dump_outputs(str(tmp_path), results, [(sl, b) for b in range(16)], 3)
    got = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert set(got) == {"tokens", "scores", "no_speech_prob", "logmel", "encoder_output"}
    assert got["tokens"].dtype == got["scores"].dtype == np.float64 and got["tokens"].shape == (16, 3)
    assert got["tokens"][0].tolist() == [7, -1, -1] and got["tokens"][2].tolist() == [7, 8, 9] and got["scores"][4] == -1.0
    k = got["logmel"].shape[0]
    assert 0 < k < 16 and got["encoder_output"].shape == (k, 1500, 768) and got["logmel"].dtype == np.float32
    assert got["logmel"][k - 1, 0, 0] == k - 1 and got["encoder_output"][k - 1, 0, 0] == 1 - k
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 64e6
    bench.dump_outputs(str(tmp_path / "c5"), results, [], 0)              # config 5: no resident windows
    assert sorted(p.stem for p in (tmp_path / "c5").iterdir()) == ["no_speech_prob", "scores", "tokens"]
