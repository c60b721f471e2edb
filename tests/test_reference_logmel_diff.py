"""Differential test of the log-mel ORACLE against the reference's own in-tree statement of the recipe
(VERDICT r05 "next round" 4a).

``whisper_live/transcriber/tensorrt_utils.py`` holds the one piece of feature arithmetic the reference repository itself
owns: ``log_mel_spectrogram(audio, n_mels, padding=...)`` (:130-194: right pad, ``torch.stft`` with a periodic Hann
window, drop the last frame, ``|X|^2``, mel projection, ``log10(clamp(., 1e-10))``, the ``max - 8`` floor, ``(x + 4) / 4``)
and ``pad_or_trim`` (:80-104). It is plain torch-CPU; with its un-vendored imports (``kaldialign``, ``soundfile``, ``av``,
``whisper_live.utils``) stubbed in ``sys.modules`` the file loads UNMODIFIED by path. Its filterbank comes from a
``mel_filters.npz`` that is not in the checkout (``docker/Dockerfile.tensorrt:21`` downloads it): the record was made with one from
``oracle.logmel.mel_filters`` (pinned separately to ``transformers.audio_utils.mel_filter_bank`` in
tests/test_oracle_golden.py) in ``mel_filters_dir``, so what is compared is everything BUT the filterbank:
framing / reflect padding, window, STFT, frame drop, power, projection, log, floor, scale.

Required, for 80 and 128 mels on five lengths including sub-window and ragged ones: both the float32 restatement
(``precise=False``) and the float64 oracle the HIP kernel is tested against (tests/test_gpu_parity.py::test_logmel_parity,
2e-4) equal the reference to max-abs <= 1e-4 with the 99.9th percentile of the absolute differences <= 2e-5.
Measured here: max 1.3e-5 ... 6.4e-5, 99.9th percentile 6e-6 ... 1.6e-5 — the reference's float32 ``torch.stft`` carries its
own rounding noise of that size in a handful of low-power bins per window (3 ... 95 of 240 080 ... 384 128 values sit more
than 2e-5 from the float64 answer; the float32 and float64 restatements agree with each other to 1.2e-5), which is why the
bound on the maximum is 1e-4 and not 2e-5. ``pad_or_trim`` must be equal bit for bit on numpy and torch inputs.

The reference's side is recorded (tests/golden/make_ref_logmel_diff_golden.py; only data is stored): the full maps are too
large to keep, so the test computes them with ``reference_recipe`` — the same torch float32 operations in the same order — and
pins that restatement to the record (exact values at 4096 seeded positions per map, its float64 sum and sum of squares) before
the oracle is compared with it; ``pad_or_trim`` is held to the SHA-256 of the reference's output bytes."""
from __future__ import annotations

import hashlib
import os

import numpy as np
import pytest

from oracle import logmel as olm
from whisperlive_amd.synthetic import speech_like_pcm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_logmel_diff_golden.npz")
LENGTHS = [480000, 176000, 721234 % 480000 + 7, 16000, 4321]      # 30 s, jfk-length, ragged, 1 s, 0.27 s
PAD_CASES = [(t, length) for length in (3000, 1000) for t in (0, 1, 999, 1000, 2999, 3000, 3001, 4500)]
N_PINNED = 4096


def case_pcm(n):
    pcm = speech_like_pcm(n / 16000.0, seed=1234 + n % 97)[:n]
    assert pcm.shape[0] == n
    return pcm


def logmel_cases():
    """(key, pcm, n_mels, padding): the recipe cases, then padding=0 on a numpy input of 3 s (the TensorRT backend's own call)"""
    for n_mels in (80, 128):
        for n in LENGTHS:
            yield f"mel{n_mels}_{n}", case_pcm(n), n_mels, 160
    yield "default_padding", speech_like_pcm(3.0, seed=5), 80, 0


def pad_or_trim_input(t):
    rng = np.random.default_rng(t)
    return rng.standard_normal((80, t)).astype(np.float32), rng.standard_normal(t * 7).astype(np.float32)


def summary(m):
    """what the record keeps of one log-mel map"""
    idx = np.random.default_rng(m.size).choice(m.size, size=min(N_PINNED, m.size), replace=False)
    m64 = m.astype(np.float64)
    return {"shape": np.asarray(m.shape, np.int64), "sum": np.float64(m64.sum()), "sumsq": np.float64((m64 ** 2).sum()),
            "idx": idx.astype(np.int64), "values": m.reshape(-1)[idx]}


def reference_recipe(pcm, n_mels, padding):
    """Whisper's log-mel as the reference's tensorrt_utils.log_mel_spectrogram computes it, in torch float32: a numpy input
    padded / trimmed to 30 s, right pad, STFT with a periodic Hann window, last frame dropped, power, mel projection,
    log10 of the clamp at 1e-10, the max - 8 floor, (x + 4) / 4"""
    import torch
    if padding == 0:
        pcm = olm.pad_or_trim(pcm, 480000)
    x = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.float32))
    if padding > 0:
        x = torch.nn.functional.pad(x, (0, padding))
    with torch.no_grad():
        spec = torch.stft(x, 400, 160, window=torch.hann_window(400), return_complex=True)
        power = spec[..., :-1].abs() ** 2
        mel = torch.from_numpy(olm.mel_filters(n_mels)) @ power
        log_spec = torch.clamp(mel, min=1e-10).log10()
        log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
        return ((log_spec + 4.0) / 4.0).numpy()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def ref(golden):
    """the reference's map of every case: the restatement, held to the record of the reference's own output"""
    pytest.importorskip("torch")
    out = {}
    for key, pcm, n_mels, padding in logmel_cases():
        m = reference_recipe(pcm, n_mels, padding)
        assert m.dtype == np.float32 and m.shape == tuple(golden[f"{key}_shape"]), key
        np.testing.assert_allclose(m.reshape(-1)[golden[f"{key}_idx"]], golden[f"{key}_values"], rtol=0, atol=1e-6, err_msg=key)
        s = summary(m)
        assert abs(s["sum"] - golden[f"{key}_sum"]) <= 1e-6 * m.size and abs(s["sumsq"] - golden[f"{key}_sumsq"]) <= 1e-6 * m.size, key
        out[key] = m
    return out


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("n", LENGTHS)
def test_oracle_logmel_equals_reference_recipe(ref, n_mels, n):
    pcm = case_pcm(n)
    got_ref = ref[f"mel{n_mels}_{n}"]
    f32 = olm.log_mel_spectrogram(pcm, n_mels, padding=160, precise=False)
    f64 = olm.log_mel_spectrogram(pcm, n_mels, padding=160, precise=True)
    assert got_ref.shape == f32.shape == f64.shape == (n_mels, (n + 160) // 160)
    assert got_ref.dtype == np.float32
    e32 = float(np.abs(got_ref - f32).max())
    e64 = float(np.abs(got_ref - f64).max())
    assert e32 <= 1e-4, f"float32 restatement vs tensorrt_utils.log_mel_spectrogram: {e32}"
    assert e64 <= 1e-4, f"float64 oracle vs tensorrt_utils.log_mel_spectrogram: {e64}"
    q32 = float(np.quantile(np.abs(got_ref - f32), 0.999))
    q64 = float(np.quantile(np.abs(got_ref - f64), 0.999))
    assert q32 <= 2e-5 and q64 <= 2e-5, f"99.9th percentile of |reference - oracle|: f32 {q32}, f64 {q64}"


def test_reference_default_padding_path(ref):
    """padding=0 (the TensorRT backend's own call) and a numpy input, which the reference first pads / trims to 30 s."""
    pcm = speech_like_pcm(3.0, seed=5)
    got = ref["default_padding"]
    want = olm.log_mel_spectrogram(np.pad(pcm, (0, 480000 - pcm.shape[0])), 80, padding=0, precise=False)
    assert got.shape == want.shape == (80, 3000)
    assert float(np.abs(got - want).max()) <= 2e-5


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@pytest.mark.parametrize("length", [3000, 1000])
@pytest.mark.parametrize("t", [0, 1, 999, 1000, 2999, 3000, 3001, 4500])
def test_pad_or_trim_equals_reference(golden, t, length):
    a, b = pad_or_trim_input(t)
    got = olm.pad_or_trim(a, length)
    assert got.shape == (80, length) and got.dtype == np.float32
    # bit-equal to the reference's answer on a numpy and on a torch input
    assert np.array_equal(_sha(got), golden[f"pad_{t}_{length}_np"]) and np.array_equal(_sha(got), golden[f"pad_{t}_{length}_torch"])
    # the default axis / length of the reference are the audio ones (N_SAMPLES); the feature call sites pass 3000 frames
    assert np.array_equal(_sha(olm.pad_or_trim(b, 480000)), golden[f"pad_{t}_{length}_audio"])
