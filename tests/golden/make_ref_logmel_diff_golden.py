"""Generate tests/golden/ref_logmel_diff_golden.npz: what the reference's OWN log-mel code answers in the cases of
tests/test_reference_logmel_diff.py.

Run with a checkout of the reference:  python tests/golden/make_ref_logmel_diff_golden.py REFERENCE_ROOT

whisper_live/transcriber/tensorrt_utils.py is loaded by path with its un-vendored imports stubbed (as make_ref_logmel_golden.py
does), its filterbank written from oracle.logmel.mel_filters. The full maps are too large to store, so per log-mel case the
fixture keeps the map's shape, its float64 sum and sum of squares and its exact values at 4096 seeded positions (the test pins
its torch restatement of the recipe to them); per pad_or_trim case the SHA-256 of the reference's output bytes. Only DATA is stored."""
import hashlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import logmel as olm  # noqa: E402
from tests.test_reference_logmel_diff import GOLDEN, LENGTHS, PAD_CASES, logmel_cases, pad_or_trim_input, summary  # noqa: E402


def load_reference(path):
    for name in ("kaldialign", "soundfile", "av", "whisper_live", "whisper_live.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["whisper_live"].__path__ = []
    sys.modules["whisper_live.utils"].resample = None
    spec = importlib.util.spec_from_file_location("_ref_tensorrt_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "whisper_live", "transcriber", "tensorrt_utils.py"))
    d = tempfile.mkdtemp()
    np.savez_compressed(os.path.join(d, "mel_filters.npz"), mel_80=olm.mel_filters(80), mel_128=olm.mel_filters(128))
    out = {}
    with torch.no_grad():
        for key, pcm, n_mels, padding in logmel_cases():
            a = torch.from_numpy(pcm) if padding else pcm                   # numpy input: the reference pads / trims it to 30 s
            got = ref.log_mel_spectrogram(a, n_mels, padding=padding, mel_filters_dir=d).numpy()
            assert got.dtype == np.float32
            for k, v in summary(got).items():
                out[f"{key}_{k}"] = v
        for t, length in PAD_CASES:
            a, b = pad_or_trim_input(t)
            out[f"pad_{t}_{length}_np"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(ref.pad_or_trim(a, length)).tobytes()).digest(), np.uint8)
            out[f"pad_{t}_{length}_torch"] = np.frombuffer(hashlib.sha256(ref.pad_or_trim(torch.from_numpy(a), length).numpy().tobytes()).digest(), np.uint8)
            out[f"pad_{t}_{length}_audio"] = np.frombuffer(hashlib.sha256(ref.pad_or_trim(b).tobytes()).digest(), np.uint8)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes", len(LENGTHS), "lengths")


if __name__ == "__main__":
    main()
