"""Result-level check with REAL weights and REAL audio — the reference's only transcript-level pin
(tests/test_server.py:73-118: `base.en` on assets/jfk.flac, word error rate < 0.05 after text normalisation).

Neither weights nor a tokenizer exist in the build container, so this test is gated on the environment
and skips cleanly without the artefacts:

    WLX_MODEL_DIR   (optional since round 5: without it the product's own look-up is used — $WLX_MODEL_ROOT, then the Hugging Face cache
                    for base.en / small.en / tiny.en ..., whisperlive_amd/artifacts.py — so a box with a warmed cache runs this unattended)
                    a model directory the loaders understand: CTranslate2 (model.bin + tokenizer.json / vocabulary.*,
                    e.g. Systran/faster-whisper-base.en — what the reference serves) or Hugging Face
                    (model.safetensors + tokenizer.json), whisperlive_amd/weights.py::load_model_dir
    WLX_WAV         (optional) a WAV / FLAC file; default: the reference's assets/jfk.flac as tests/golden/jfk_16k.npz
    WLX_REF_TEXT    (optional) the expected transcript of WLX_WAV; default: the reference test's ground truth for jfk
    WLX_MAX_WER     (optional) default 0.05, the reference's bound

The word error rate is computed here (Levenshtein distance over normalised words: lower-case, punctuation stripped,
whitespace collapsed — the parts of whisper's EnglishTextNormalizer that matter for this sentence; jiwer and
whisper.normalizers are not installable offline). Needs the GPU: the transcript comes from libwlx.so."""
import os
import re

import numpy as np
import pytest

JFK_TEXT = ("And so my fellow Americans, ask not, what your country can do for you. "
            "Ask what you can do for your country!")          # tests/test_server.py:92 of the reference



def _find_model_dir():
    """WLX_MODEL_DIR, else whatever the product's own look-up finds WITHOUT a download (whisperlive_amd/artifacts.py: $WLX_MODEL_ROOT, the
    Hugging Face cache) for the reference test's model and its neighbours — so the test runs unattended on any box that has the cache."""
    d = os.environ.get("WLX_MODEL_DIR")
    if d:
        return d
    try:
        from whisperlive_amd.artifacts import ArtifactNotFound, resolve_model
    except ImportError:
        return None
    for name in ("base.en", "small.en", "tiny.en", "base", "small", "tiny"):
        try:
            return resolve_model(name, local_files_only=True)
        except ArtifactNotFound:
            continue
    return None


def _find_wav():
    w = os.environ.get("WLX_WAV")
    if w:
        return w
    fx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_16k.npz")     # the same clip, decoded (tests/golden/make_jfk_fixture.py)
    return fx if os.path.isfile(fx) else None


MODEL_DIR = _find_model_dir()
WAV = _find_wav()


def normalise(text: str):
    return re.sub(r"[^a-z0-9' ]+", " ", text.lower()).split()


def word_error_rate(ref: str, hyp: str) -> float:
    r, h = normalise(ref), normalise(hyp)
    d = np.arange(len(h) + 1)
    for i in range(1, len(r) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(h) + 1):
            cur = d[j]
            d[j] = min(d[j] + 1, d[j - 1] + 1, prev + (r[i - 1] != h[j - 1]))
            prev = cur
    return float(d[len(h)]) / max(1, len(r))


def test_word_error_rate_helper():
    assert word_error_rate(JFK_TEXT, JFK_TEXT.upper().replace(",", "")) == 0.0
    assert word_error_rate("a b c d", "a x c") == 0.5                      # one substitution + one deletion over 4 words
    assert word_error_rate("a b", "a b c") == 0.5


@pytest.mark.gpu
@pytest.mark.skipif(not (MODEL_DIR and os.path.isdir(MODEL_DIR)), reason="no Whisper weights: WLX_MODEL_DIR not set and nothing in $WLX_MODEL_ROOT / the Hugging Face cache (SURVEY.md §8c)")
@pytest.mark.skipif(WAV is None, reason="no audio: set WLX_WAV (the reference's assets/jfk.flac is not present)")
@pytest.mark.parametrize("vad", [False, True])
def test_transcript_of_real_audio_with_real_weights(gpu, vad):
    from whisperlive_amd.transcriber import WhisperModelHIP
    from whisperlive_amd.artifacts import silero_candidates
    if vad and not silero_candidates():
        pytest.skip("VAD leg needs Silero weights (WLX_SILERO_VAD_NPZ / WLX_SILERO_VAD_ONNX, ~/.cache/whisper-live/silero_vad.onnx or an installed faster_whisper)")
    model = WhisperModelHIP(MODEL_DIR, device="cuda", device_index=0)
    audio = WAV
    if WAV.endswith(".npz"):
        z = np.load(WAV)
        audio = z["pcm"].astype(np.float32)
    try:
        segments, info = model.transcribe(audio, language="en" if not model.model.is_multilingual else None,
                                          vad_filter=vad, vad_parameters={"threshold": 0.5} if vad else None)
        text = " ".join(s.text.strip() for s in (segments or []))
        ref = os.environ.get("WLX_REF_TEXT") or JFK_TEXT
        wer = word_error_rate(ref, text)
        print(f"[real weights] {MODEL_DIR} on {WAV}: '{text}'  WER {wer:.3f}  language {info.language}")
        assert wer < float(os.environ.get("WLX_MAX_WER", "0.05")), (text, wer)
        assert all(0.0 <= s.start <= s.end <= info.duration + 0.5 for s in segments)
    finally:
        model.close()
