"""GPU tests of the speaker-embedding engine (wlx_spk_*) and the diarization built on it: the whole ResNet34 against the CPU
restatement of tests/spk_oracle.py on seeded weights (no WeSpeaker checkpoint exists offline: PARITY UNPINNED, as the oracle's
header says), labels against the reference-pinned clustering on the oracle's embeddings, repeatability, independence of calls,
concurrency with a running ASR decode, and the server end to end."""
from __future__ import annotations

import json
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from whisperlive_amd import spk_weights
from whisperlive_amd.diarization import SpeakerDiarizer, SpeakerEmbedderHIP

from . import spk_oracle as O

pytestmark = pytest.mark.gpu

SPEC = spk_weights.RESNET34
WEIGHT_SEED = 11


def voice_pcm(voice: int, seconds: float, seed: int) -> np.ndarray:
    """seeded synthetic 'voice': a harmonic series at the voice's pitch under the voice's three formants, gated on and off at the
    voice's own rate and duty cycle, plus noise. The front end removes each bin's mean over time, so what tells voices apart is
    their modulation: voices differ in pitch, formants, gating rate and duty; takes of one voice in phases and noise."""
    f0 = (95.0, 160.0, 230.0, 130.0)[voice]
    formants = ((650, 1100, 2500), (400, 1900, 2700), (300, 900, 3100), (800, 1400, 2300))[voice]
    rng = np.random.default_rng(1000 * voice + seed)
    n = int(round(seconds * 16000))
    t = np.arange(n) / 16000.0
    sig = np.zeros(n)
    for h in range(1, int(3800 / f0)):
        f = h * f0
        gain = sum(np.exp(-0.5 * ((f - fc) / 120.0) ** 2) for fc in formants) + 0.02
        sig += gain * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    rate, duty = ((0.0, 1.0), (3.0, 0.5), (11.0, 0.3), (6.0, 0.7))[voice]
    if rate:
        sig *= ((t * rate + rng.uniform(0, 1)) % 1.0 < duty)
    sig += rng.normal(0, 0.002 * np.abs(sig).max(), n)
    return (0.5 * sig / np.abs(sig).max()).astype(np.float32)


# 12 segments of three voices. Chosen on the CPU (oracle embeddings only): the widest gap of the sorted pairwise similarities is
# >= 0.02 and the clustering at its midpoint goes through both the new-speaker and the match branch (asserted in the test).
SEGMENTS = [(0, 2.0, 1), (1, 1.5, 2), (0, 3.1, 3), (2, 0.9, 4), (1, 2.6, 5), (2, 2.2, 6), (0, 0.7, 7), (1, 4.0, 8), (2, 1.3, 9),
            (0, 1.1, 10), (2, 3.3, 11), (1, 0.6, 12)]


@pytest.fixture(scope="module")
def net():
    w = spk_weights.fold(spk_weights.random_weights(SPEC, seed=WEIGHT_SEED), SPEC)
    eng = SpeakerEmbedderHIP(SPEC, w, device=0)
    yield eng, w
    eng.close()


@pytest.mark.parametrize("seconds", [0.3, 2.5, 11.0, 45.0])
def test_whole_network_against_the_oracle(net, seconds):
    """Full ResNet34 on seeded weights. e_emul = rel-rms between the oracle with every stored activation rounded to fp16 and the
    plain fp32 oracle (both on the CPU, same folded tensors); the HIP embedding must lie within max(2e-3, 2 e_emul) of the fp32
    oracle, the factor 2 for the accumulation order. The bound never sees the GPU's output. The printed figures of an MI355X run
    are kept in profiles/spk_network_error.txt."""
    eng, w = net
    pcm = voice_pcm(int(seconds) % 4, seconds, seed=int(seconds * 10))
    assert len(pcm) == int(round(seconds * 16000))
    ref = O.embed(SPEC, w, pcm)
    e_emul = O.rel_rms(O.embed(SPEC, w, pcm, fp16_activations=True), ref)
    bound = max(2e-3, 2 * e_emul)
    got = eng.embed(pcm)
    err = O.rel_rms(got, ref)
    fb, nn = eng.timings()
    print(f"spk network {seconds:5.1f} s: e_emul {e_emul:.3e} bound {bound:.3e} hip error {err:.3e} cosine {float(got @ ref):.6f} "
          f"device ms fbank {fb:.3f} net {nn:.3f}")
    assert got.shape == (256,) and np.isfinite(got).all() and abs(float(np.linalg.norm(got)) - 1) <= 1e-5
    assert err <= bound, (err, bound)


def test_short_and_long_audio_statuses(net):
    eng, _ = net
    assert eng.embed(np.zeros(4799, np.float32) + 0.1) is None            # under 0.3 s: the distinct status, no embedding
    assert eng.embed(voice_pcm(0, 0.3, 1)) is not None
    from whisperlive_amd import _lib
    import ctypes as C
    big = np.zeros(45 * 16000 + 1, np.float32)
    out = np.zeros(256, np.float32)
    f32p = C.POINTER(C.c_float)
    assert eng.lib.wlx_spk_embed(eng.h, big.ctypes.data_as(f32p), len(big), out.ctypes.data_as(f32p)) == 1     # WLX_ERR_ARG
    assert _lib.ERR_TOO_SHORT == 6
    # one sample under the minimum: the status is the return value and `out` is not written; exactly the minimum is served
    edge = voice_pcm(0, 0.3, 1)
    out[:] = 7.0
    assert len(edge) == 4800 and eng.lib.wlx_spk_embed(eng.h, edge.ctypes.data_as(f32p), 4799, out.ctypes.data_as(f32p)) == 6
    assert (out == 7.0).all()
    assert eng.lib.wlx_spk_embed(eng.h, edge.ctypes.data_as(f32p), 4800, out.ctypes.data_as(f32p)) == 0
    assert (out.view(np.uint32) == eng.embed(edge).view(np.uint32)).all()


def _oracle_labels(w, pcms, threshold, max_speakers=10):
    embs = [O.embed(SPEC, w, p) if len(p) >= 4800 else None for p in pcms]
    feed = [e for e in embs if e is not None]            # (the diarizer never asks for a segment under 0.3 s)
    d = SpeakerDiarizer(similarity_threshold=threshold, max_speakers=max_speakers, embedder=lambda pcm, sr: feed.pop(0))
    return [d.identify_speaker(p) for p in pcms], [e for e in embs if e is not None]


def _widest_gap_threshold(embs):
    E = np.stack(embs).astype(np.float64)
    sims = np.sort((E @ E.T)[np.triu_indices(len(embs), 1)])
    k = int(np.argmax(np.diff(sims)))
    return 0.5 * (sims[k] + sims[k + 1]), float(sims[k + 1] - sims[k])


def test_labels_equal_the_oracle_pipeline(net):
    """12 seeded segments through SpeakerDiarizer on the HIP embedder against the same (reference-pinned, tests/test_spk_host.py)
    clustering on the oracle's embeddings; threshold at the midpoint of the widest gap of the oracle's pairwise similarities"""
    eng, w = net
    pcms = [voice_pcm(v, s, seed) for v, s, seed in SEGMENTS]
    _, embs = _oracle_labels(w, pcms, 0.5)
    thr, gap = _widest_gap_threshold(embs)
    assert gap >= 0.02, gap                                  # a condition on the committed inputs
    want, _ = _oracle_labels(w, pcms, thr)
    assert len(set(want)) >= 2 and len(set(want)) < len(want), want      # new-speaker and match branches both occur
    d = SpeakerDiarizer(similarity_threshold=thr, embedder=eng)
    got = [d.identify_speaker(p) for p in pcms]
    print(f"labels: threshold {thr:.4f} (gap {gap:.4f}) -> {got}")
    assert got == want


def test_same_segment_twice_is_bit_identical_and_calls_are_independent(net):
    eng, _ = net
    short, long_ = voice_pcm(1, 0.5, 3), voice_pcm(2, 20.0, 4)
    a = eng.embed(short)
    assert (eng.embed(short).view(np.uint32) == a.view(np.uint32)).all()
    b = eng.embed(long_)
    assert (eng.embed(long_).view(np.uint32) == b.view(np.uint32)).all()
    # a short segment after a long one: nothing of the long one is left in the buffers
    assert (eng.embed(short).view(np.uint32) == a.view(np.uint32)).all()
    assert not (a.view(np.uint32) == b.view(np.uint32)).all()


def test_asr_tokens_unchanged_by_concurrent_embeds(net):
    """modelled on test_asr_tokens_unchanged_by_concurrent_translation: a Whisper decode with embeds running on the same GPU"""
    from oracle import logmel as olm
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    eng, _ = net
    spec = SPECS["tiny.en"]
    asr = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = asr.create_slot(1, 5)
    try:
        pcm = olm.speech_like_pcm(6.0, seed=1234)
        tb = spec.vocab - 1501
        ids = TokenIds(tb - 106, tb - 107, tb - 1, tb, tb - 2, 220)
        kw = dict(beam_size=5, patience=1.0, max_length=1 + 24, suppress_tokens=[1, 2, 7, ids.sot])

        def run():
            T = slot.logmel(pcm)
            slot.encode(1, seek=[0], seg=[T - 1])
            return slot.generate([[ids.sot]], ids, **kw)[0].sequences_ids[0]
        solo = run()
        seg = voice_pcm(0, 3.0, 5)
        emb_solo = eng.embed(seg)
        stop = threading.Event()
        errs, embs = [], []

        def embed_loop():
            try:
                while not stop.is_set():
                    embs.append(eng.embed(seg))
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = threading.Thread(target=embed_loop)
        th.start()
        try:
            together = [run() for _ in range(3)]
        finally:
            stop.set()
            th.join(timeout=120)
        assert not errs, errs
        assert all(t == solo for t in together)
        assert embs and all((e.view(np.uint32) == emb_solo.view(np.uint32)).all() for e in embs)
    finally:
        slot.close()
        asr.close()


class _OneSecondTranscriber:
    """stands in for Whisper: commits pieces of 1.0, 0.2, 1.7, 0.8, 1.3 seconds, one per call and only once the chunk holds the whole
    piece and some tail (until then it reports one in-progress segment), so the boundaries do not depend on packet timing and the
    server's own slicing of frames_np decides what the embedder hears"""
    LENGTHS = (1.0, 0.2, 1.7, 0.8, 1.3)

    def __init__(self):
        self.calls = self.commits = 0

    def transcribe(self, audio, **kw):
        self.calls += 1
        dur = audio.shape[0] / 16000.0
        info = SimpleNamespace(language="en", language_probability=0.99)
        cut = self.LENGTHS[self.commits % len(self.LENGTHS)]
        if dur < cut + 0.05:
            return [SimpleNamespace(start=0.0, end=dur, text=f" pending{self.calls}", no_speech_prob=0.0, words=None)], info
        self.commits += 1
        return [SimpleNamespace(start=0.0, end=cut, text=f" s{self.commits}", no_speech_prob=0.0, words=None),
                SimpleNamespace(start=cut, end=dur, text=f" tail{self.calls}", no_speech_prob=0.0, words=None)], info


def test_server_end_to_end_labels_equal_the_oracle_pipeline(tmp_path, net):
    """the real server, the seeded embedder weights as a checkpoint in a temporary directory, a protocol client with
    enable_diarization: every completed segment of >= 0.3 s carries the speaker the oracle pipeline assigns, shorter ones none"""
    from whisperlive_amd import diarization, ws
    from whisperlive_amd.serve_client import ServeClientHIP
    from whisperlive_amd.server import TranscriptionServer
    _, w = net
    sd = spk_weights.random_weights(SPEC, seed=WEIGHT_SEED)
    ckpt = tmp_path / "wespeaker-seeded"
    ckpt.mkdir()
    torch.save({"state_dict": {"resnet." + k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt / "pytorch_model.bin")
    pcm = np.concatenate([voice_pcm(0, 1.0, 21), voice_pcm(1, 1.9, 22), voice_pcm(0, 0.8, 23), voice_pcm(2, 1.3, 24),
                          voice_pcm(1, 1.5, 25)])
    bounds, t0 = [], 0.0
    for n in _OneSecondTranscriber.LENGTHS:
        bounds.append((t0, t0 + n))
        t0 += n
    pieces = [pcm[int(a * 16000):int(b * 16000)] for a, b in bounds]
    _, embs = _oracle_labels(w, pieces, 0.5)
    thr, gap = _widest_gap_threshold(embs)
    assert gap >= 0.02, gap
    want, _ = _oracle_labels(w, pieces, thr)
    assert want[1] is None and sum(x is not None for x in want) == 4

    srv, ready = TranscriptionServer(), threading.Event()
    srv.diarization_model = str(ckpt)
    ServeClientHIP.MODELS.clear()
    t = threading.Thread(target=srv.run, args=("127.0.0.1",), daemon=True,
                         kwargs=dict(port=0, ready=ready, single_model=True, model_factory=lambda m, d: _OneSecondTranscriber()))
    t.start()
    assert ready.wait(10)
    try:
        c = ws.connect(f"ws://127.0.0.1:{srv.port}")
        c.send(json.dumps(dict(uid="e2e", language="en", task="transcribe", model="small.en", use_vad=False, enable_diarization=True,
                               diarization_threshold=thr, max_speakers=10)))
        assert json.loads(c.recv(timeout=30.0))["message"] == "SERVER_READY"
        stream = np.concatenate([pcm, np.zeros(16000, np.float32)])          # (a second of tail so the last piece is committed)
        for i in range(0, stream.shape[0], 4096):
            c.send(stream[i: i + 4096].tobytes())
        done = {}
        for _ in range(600):
            msg = json.loads(c.recv(timeout=60.0))
            for s in msg.get("segments", []):
                if s.get("completed"):
                    done[s["start"]] = s
            if len(done) >= len(bounds):
                break
        c.send(b"END_OF_AUDIO")
        c.close()
        segs = [done[k] for k in sorted(done, key=float)][:len(bounds)]
        print("e2e:", [(s["start"], s["end"], s.get("speaker")) for s in segs], "oracle", want)
        assert [(float(s["start"]), float(s["end"])) for s in segs] == [(round(a, 3), round(b, 3)) for a, b in bounds]
        assert [s.get("speaker") for s in segs] == want
        assert isinstance(diarization.shared_embedder(str(ckpt), 0), SpeakerEmbedderHIP)
    finally:
        srv.shutdown()
        t.join(5)
        ServeClientHIP.MODELS.clear()
        diarization.close_shared()
