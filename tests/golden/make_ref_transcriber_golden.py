"""Generate tests/golden/ref_transcriber_golden.json.gz: what the reference's OWN transcriber code answers in the 320 seeded
cases of tests/test_reference_transcriber_diff.py.

Run with a checkout of the reference:  python tests/golden/make_ref_transcriber_golden.py REFERENCE_ROOT

The reference's transcriber module (whisper_live/transcriber/transcriber_faster_whisper.py) is loaded by path with its
un-vendored imports (ctranslate2, faster_whisper.*) stubbed in ``sys.modules``; ``WhisperModel.__new__`` gives an instance whose
``transcribe`` is the reference's own, driven by the test's scripted stand-in for ``model.generate`` / ``detect_language`` /
``align`` / the VAD probabilities. Only DATA is stored: per seed the error (type, message), the call log at the numerical
boundary, the segments, the ``TranscriptionInfo`` fields and the transcription options, as JSON."""
from __future__ import annotations

import gzip
import importlib.util
import json
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_reference_transcriber_diff import GOLDEN, N_CASES, Script, run_case  # noqa: E402
from whisperlive_amd import vad as wvad  # noqa: E402
from whisperlive_amd import word_timing as wwt  # noqa: E402
from whisperlive_amd.tokenizer import LANGUAGE_CODES, Tokenizer  # noqa: E402

REF_FILE = os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "whisper_live", "transcriber", "transcriber_faster_whisper.py")


# ------------------------------------------------------------------------------------------------------------------
# reference side: module loaded by path with the un-vendored imports stubbed
def _load_reference(script_holder):
    names = ["ctranslate2", "faster_whisper", "faster_whisper.audio", "faster_whisper.feature_extractor",
             "faster_whisper.tokenizer", "faster_whisper.utils", "faster_whisper.vad"]
    saved = {n: sys.modules.get(n) for n in names}
    ct2 = types.ModuleType("ctranslate2")

    class StorageView:
        @staticmethod
        def from_array(a):
            return a
    ct2.StorageView = StorageView
    ct2.models = types.SimpleNamespace(Whisper=object, WhisperGenerationResult=object)
    fw = types.ModuleType("faster_whisper")
    audio = types.ModuleType("faster_whisper.audio")

    def pad_or_trim(array, length=3000, axis=-1):
        n = array.shape[axis]
        if n > length:
            return array.take(indices=range(length), axis=axis)
        if n < length:
            w = [(0, 0)] * array.ndim
            w[axis] = (0, length - n)
            return np.pad(array, w)
        return array
    audio.pad_or_trim = pad_or_trim
    audio.decode_audio = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("no decoder in the test"))
    fe = types.ModuleType("faster_whisper.feature_extractor")
    fe.FeatureExtractor = object
    tokm = types.ModuleType("faster_whisper.tokenizer")
    tokm.Tokenizer = Tokenizer
    tokm._LANGUAGE_CODES = LANGUAGE_CODES
    utils = types.ModuleType("faster_whisper.utils")
    utils.download_model = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("offline"))
    utils.format_timestamp = lambda s, *a, **k: f"{s:.3f}"
    utils.get_logger = lambda: logging.getLogger("faster_whisper")
    utils.get_end = wwt.last_word_end
    vadm = types.ModuleType("faster_whisper.vad")
    vadm.VadOptions = wvad.VadOptions
    vadm.SpeechTimestampsMap = wvad.SpeechTimestampsMap
    vadm.collect_chunks = wvad.collect_chunks
    vadm.get_speech_timestamps = lambda audio_, opts=None, **kw: wvad.get_speech_timestamps(
        audio_, opts, model=script_holder["vad"])
    mods = dict(zip(names, [ct2, fw, audio, fe, tokm, utils, vadm]))
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location("_ref_transcriber_under_test", REF_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


class _RefFeatureExtractor:
    """attributes the reference reads (:656-665,1058,1115-1126) + a frame-count-only __call__"""
    n_fft, hop_length, chunk_length, sampling_rate = 400, 160, 30, 16000
    n_samples, nb_max_frames, time_per_frame = 480000, 3000, 0.01

    def __call__(self, waveform, padding=160, chunk_length=None):
        # column j carries j + 1, so the scripted encoder can read (seek, window size) back from what it is handed
        t = (len(waveform) + padding) // 160
        return np.broadcast_to(np.arange(1, t + 1, dtype=np.float32), (80, t)).copy()


class _RefCT2:
    """ctranslate2.models.Whisper as the reference calls it, answering from the script"""
    device, device_index = "cuda", [0]

    def __init__(self, script: Script, hf_tok, multilingual: bool):
        self.s, self.hf, self.is_multilingual = script, hf_tok, multilingual
        bt = Tokenizer(hf_tok, False)
        self.langs = bt.language_token_ids()
        self.non_speech = set(bt.non_speech_tokens)

    def encode(self, features, to_cpu=False):
        f = np.asarray(features)
        assert f.shape == (1, 80, 3000)                   # pad_or_trim'ed window, batch axis added (:1344-1348)
        row = f[0, 0]
        self.s.log.append(("encode", int(row[0]) - 1, int(np.count_nonzero(row))))
        return object()

    def generate(self, enc, prompts, **kw):
        assert len(prompts) == 1
        prompt = list(prompts[0])
        sup = sorted(set(kw.get("suppress_tokens") or ()))
        beam = kw.get("beam_size", 5)
        temp = 0.0 if beam > 1 else (float(kw.get("sampling_temperature", 1.0)) if kw.get("sampling_topk", 1) != 1 else 0.0)
        self.s.log.append(("generate", prompt, beam, float(kw.get("patience", 1)), kw.get("num_hypotheses", 1),
                           float(kw["length_penalty"]), float(kw["repetition_penalty"]), kw["no_repeat_ngram_size"],
                           kw["max_length"], bool(kw["suppress_blank"]), tuple(sup), kw["max_initial_timestamp_index"],
                           round(temp, 6)))
        toks, score, nsp = self.s.generate(prompt, kw["max_length"] - len(prompt))
        return [types.SimpleNamespace(sequences_ids=[toks], scores=[score], no_speech_prob=nsp)]

    def detect_language(self, enc):
        self.s.log.append(("detect_language",))
        p = self.s.lang_probs()
        pairs = [(f"<|{c}|>", float(np.float32(x))) for (c, _i), x in zip(self.langs, p)]
        return [sorted(pairs, key=lambda x: -x[1])]

    def align(self, enc, start_sequence, text_tokens, num_frames, median_filter_width=7):
        out = []
        for toks in text_tokens:
            if not toks:
                # the reference still calls align for a window without text tokens and then discards the result
                # (:1670-1678 "return on eot only"); the HIP host skips that device call — the one tolerated difference
                out.append(types.SimpleNamespace(alignments=[], text_token_probs=[]))
                continue
            self.s.log.append(("align", list(start_sequence), list(toks), int(num_frames), median_filter_width))
            pairs, probs = self.s.align(len(toks), num_frames)
            out.append(types.SimpleNamespace(alignments=pairs, text_token_probs=probs))
        return out


def _make_reference(refmod, script, hf_tok, multilingual):
    m = refmod.WhisperModel.__new__(refmod.WhisperModel)
    m.logger = logging.getLogger("faster_whisper")
    m.model = _RefCT2(script, hf_tok, multilingual)
    m.hf_tokenizer = hf_tok
    m.feat_kwargs = {}
    m.feature_extractor = _RefFeatureExtractor()
    m.input_stride = 2
    m.num_samples_per_token = 320
    m.frames_per_second = 100
    m.tokens_per_second = 50
    m.time_precision = 0.02
    m.max_length = 448
    return m




def main():
    holder = {"vad": None}
    refmod = _load_reference(holder)
    refmod._script_holder = holder

    def make_model(script, hf, multilingual_model, vad_model):
        holder["vad"] = vad_model
        return _make_reference(refmod, script, hf, multilingual_model)
    cases = [run_case(seed, make_model) for seed in range(N_CASES)]
    with gzip.open(GOLDEN, "wt", encoding="utf-8") as f:
        json.dump(cases, f, separators=(",", ":"))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
