"""Host-side tests of the diarization feature (no GPU): the two restatements of tests/spk_oracle.py against independent
arithmetic, the BatchNorm fold, the checkpoint loader, the clustering against label sequences and centroids RECORDED FROM THE
REFERENCE'S OWN SpeakerDiarizer (tests/golden/ref_diarizer_golden.json, written by tests/golden/make_ref_diarizer_golden.py), the
artefact look-up order, and the server wiring with a fake embedder and a fake transcriber."""
from __future__ import annotations

import json
import logging
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from whisperlive_amd import artifacts, spk_weights, ws
from whisperlive_amd.diarization import SpeakerDiarizer
from whisperlive_amd.serve_client import ServeClientHIP
from whisperlive_amd.server import TranscriptionServer
from whisperlive_amd.synthetic import speech_like_pcm

from . import spk_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_diarizer_golden.json")
SMALL = spk_weights.SpkSpec(n_mels=16, planes=32, blocks=(1, 1, 1, 1), embed_dim=32, max_seconds=5)


# ---- the restatements ------------------------------------------------------------------------------------------------
def test_fbank_frame_against_a_direct_dft():
    """one frame of the float64 filterbank against an O(N^2) DFT written out term by term, with the Kaldi steps (scale, DC,
    pre-emphasis against the previous sample, Hamming, zero-padding to 512, power, triangular bins, log) restated in plain loops"""
    pcm = speech_like_pcm(0.5, seed=3)
    t = 7
    x = [float(v) * 32768.0 for v in pcm[160 * t:160 * t + 400]]
    mean = sum(x) / 400
    x = [v - mean for v in x]
    y = [x[0] - 0.97 * x[0]] + [x[i] - 0.97 * x[i - 1] for i in range(1, 400)]
    y = [v * (0.54 - 0.46 * np.cos(2 * np.pi * i / 399)) for i, v in enumerate(y)]
    n = np.arange(400)
    power = np.zeros(256)
    for k in range(256):
        re = float(np.sum(np.asarray(y) * np.cos(2 * np.pi * k * n / 512)))
        im = float(np.sum(np.asarray(y) * np.sin(2 * np.pi * k * n / 512)))
        power[k] = re * re + im * im
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    lo, hi = mel(20.0), mel(8000.0)
    ref = np.zeros(80)
    for b in range(80):
        left, centre, right = (lo + (b + j) * (hi - lo) / 81 for j in range(3))
        e = 0.0
        for k in range(256):
            m = mel(k * 16000.0 / 512)
            if left < m < right:
                e += power[k] * ((m - left) / (centre - left) if m <= centre else (right - m) / (right - centre))
        ref[b] = np.log(max(e, np.finfo(np.float32).eps))
    got = O.fbank(pcm)
    assert got.shape == (1 + (len(pcm) - 400) // 160, 80)
    assert np.abs(got[t] - ref).max() <= 1e-9
    assert np.abs(O.features(pcm).mean(axis=0)).max() <= 1e-12


def test_fp32_filterbank_restatement_is_well_inside_the_gpu_bound():
    """what fp32 DFT and mel stages cost against float64 on speech-like audio: two orders below the 2e-3 log units the GPU test
    allows the kernel (measured here: about 1e-4), so that bound needs no widening"""
    pcm = speech_like_pcm(7.3, seed=73)
    err = float(np.abs(O.fbank(pcm, dtype=np.float32) - O.fbank(pcm)).max())
    assert err <= 1e-3, err


@pytest.mark.parametrize("spec", [SMALL, spk_weights.SpkSpec(n_mels=24, planes=32, blocks=(2, 1, 2, 1), embed_dim=16)])
def test_fold_matches_unfolded_batchnorm(spec):
    """folded convolutions (before the fp16 rounding) give what conv + BatchNorm in eval mode gives, to float32 round-off"""
    sd = spk_weights.random_weights(spec, seed=5)
    feats = O.features(speech_like_pcm(1.0, seed=9), spec.n_mels).astype(np.float32)
    with torch.no_grad():
        ref = O.unfolded(spec, sd)(torch.from_numpy(feats)).numpy()
    got = O.folded_forward(spec, spk_weights.fold(sd, spec, round_fp16=False), feats)
    assert O.rel_rms(got, ref) <= 2e-5
    w16 = spk_weights.fold(sd, spec)
    for k, v in w16.items():
        assert v.dtype == np.float32
        if k.endswith(".weight"):
            assert (v.astype(np.float16).astype(np.float32) == v).all(), k
    assert O.rel_rms(O.folded_forward(spec, w16, feats), ref) <= 5e-3       # fp16 weights: 2^-11 per weight, not round-off


def test_spec_names_the_resnet34_tensors():
    names = spk_weights.state_shapes(spk_weights.RESNET34)
    assert names["conv1.weight"] == (32, 1, 3, 3) and names["seg_1.weight"] == (256, 5120)
    assert names["layer4.0.shortcut.0.weight"] == (256, 128, 1, 1) and "layer1.0.shortcut.0.weight" not in names
    assert sum(1 for n in names if n.endswith("conv1.weight") and n.startswith("layer")) == 16
    folded = {n for n, *_ in spk_weights.RESNET34.convs()}
    assert len(folded) == 1 + 32 + 3


# ---- loader ----------------------------------------------------------------------------------------------------------
class _Foreign:
    """stands for the Lightning objects a published checkpoint carries beside its tensors"""
    def __init__(self):
        self.x = 3


def test_loader_reads_plain_nested_and_safetensors_identically(tmp_path):
    from safetensors.numpy import save_file
    sd = spk_weights.random_weights(SMALL, seed=1)
    tsd = {"resnet." + k: torch.from_numpy(v) for k, v in sd.items()}
    tsd["resnet.bn1.num_batches_tracked"] = torch.tensor(7)
    torch.save(tsd, tmp_path / "plain.bin")
    torch.save({"state_dict": tsd, "epoch": 3, "pyannote.audio": {"versions": {"torch": "2"}}}, tmp_path / "nested.ckpt")
    torch.save({"state_dict": tsd, "hyper_parameters": _Foreign()}, tmp_path / "foreign.ckpt")
    save_file({"resnet." + k: v for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    want = spk_weights.fold(sd, SMALL)
    for f in ("plain.bin", "nested.ckpt", "foreign.ckpt", "model.safetensors", ""):
        spec, got = spk_weights.load(str(tmp_path / f), max_seconds=5)
        assert spec == SMALL, f
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), (f, k)


def test_loader_reads_parameters_beside_foreign_objects(tmp_path):
    """a state dict that holds Parameters (pickled through torch._utils._rebuild_parameter) in a checkpoint that needs the
    restricted reader: the tensors arrive, none is dropped"""
    sd = spk_weights.random_weights(SMALL, seed=2)
    tsd = {"resnet." + k: torch.nn.Parameter(torch.from_numpy(v), requires_grad=False) for k, v in sd.items()}
    torch.save({"state_dict": tsd, "hyper_parameters": _Foreign()}, tmp_path / "params.ckpt")
    _, got = spk_weights.load(str(tmp_path / "params.ckpt"), max_seconds=5)
    want = spk_weights.fold(sd, SMALL)
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)


def test_loader_never_runs_pickled_code(tmp_path):
    """a checkpoint whose pickle names a callable: neither reader calls it"""
    marker = tmp_path / "ran"

    class Evil:
        def __reduce__(self):
            return (os.mkdir, (str(marker),))

    sd = {k: torch.from_numpy(v) for k, v in spk_weights.random_weights(SMALL, seed=1).items()}
    torch.save({"state_dict": sd, "extra": Evil()}, tmp_path / "evil.ckpt")
    got = spk_weights.read_state_dict(str(tmp_path / "evil.ckpt"))
    assert not marker.exists() and "conv1.weight" in got


def test_loader_names_a_missing_key_and_a_wrong_shape():
    sd = spk_weights.random_weights(SMALL, seed=1)
    bad = dict(sd)
    del bad["layer2.0.shortcut.1.running_var"]
    with pytest.raises(KeyError, match=r"layer2\.0\.shortcut\.1\.running_var"):
        spk_weights.fold(bad, SMALL)
    bad = dict(sd)
    bad["layer3.0.conv2.weight"] = bad["layer3.0.conv2.weight"][:, :-1]
    with pytest.raises(ValueError, match=r"layer3\.0\.conv2\.weight.*\(128, 127, 3, 3\)"):
        spk_weights.fold(bad, SMALL)
    with pytest.raises(KeyError, match="seg_1.weight"):
        spk_weights.spec_from_state({k: v for k, v in sd.items() if k != "seg_1.weight"})


# ---- clustering against the reference's own class --------------------------------------------------------------------
N_SCENARIOS = 200
DIM = 4


def scenario(i: int):
    """seeded inputs of clustering scenario i: constructor arguments and a list of operations ("identify", vector | None),
    ("enroll", name, vector | None), ("reset",). Vectors are unit float64: draws around 2..6 base directions with a spread chosen
    per scenario, so that matches, new speakers and the speaker cap all occur."""
    rng = np.random.default_rng(10_000 + i)
    kw = dict(similarity_threshold=float(rng.choice([0.55, 0.55, 0.3, 0.75])), max_speakers=int(rng.choice([10, 10, 1, 2, 3])))
    if rng.random() < 0.35:
        kw["speaker_names"] = ["alice", "bob", "carol"][: int(rng.integers(1, 4))]
    bases = rng.standard_normal((int(rng.integers(2, 7)), DIM))
    spread = float(rng.choice([0.05, 0.25, 0.6]))

    def vec():
        v = bases[int(rng.integers(len(bases)))] + spread * np.linalg.norm(bases[0]) * rng.standard_normal(DIM)
        return v / np.linalg.norm(v)

    ops = []
    for _ in range(int(rng.integers(6, 17))):
        u = rng.random()
        if u < 0.06:
            ops.append(("reset",))
        elif u < 0.16:
            ops.append(("enroll", str(rng.choice(["dana", "alice", "SPEAKER_01"])), None if rng.random() < 0.2 else vec()))
        else:
            ops.append(("identify", None if rng.random() < 0.1 else vec()))
    return kw, ops


def replay(diarizer, ops, feed):
    """run `ops` on a diarizer whose embeddings come from `feed` (a list the embedding hook pops from); returns the outputs"""
    out = []
    audio = np.zeros(4800, dtype=np.float32)
    for op in ops:
        if op[0] == "reset":
            diarizer.reset()
            out.append("reset")
        elif op[0] == "enroll":
            feed.append(op[2])
            out.append(bool(diarizer.enroll_speaker(op[1], audio)))
        else:
            feed.append(op[1])
            out.append(diarizer.identify_speaker(audio))
    return out


def test_clustering_equals_the_reference_on_recorded_sequences():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["n"] == N_SCENARIOS >= 200 and len(gold["scenarios"]) == N_SCENARIOS
    seen = set()
    for i, g in enumerate(gold["scenarios"]):
        kw, ops = scenario(i)
        feed = []
        d = SpeakerDiarizer(embedder=lambda pcm, sr: feed.pop(0), **kw)
        out = replay(d, ops, feed)
        assert out == g["out"], (i, out, g["out"])
        assert list(d.speakers) == list(g["centroids"]), i
        for name, c in g["centroids"].items():
            assert np.abs(d.speakers[name] - np.asarray(c)).max() <= 1e-6, (i, name)
        # which branches this scenario went through, read off the RECORDED outputs
        labels, known = [], set()
        for op, o in zip(ops, g["out"]):
            if op[0] == "reset":
                seen.add("reset")
                known = set()
            elif op[0] == "enroll":
                seen.add("enroll" if o else "enroll_none")
                if o:
                    known.add(op[1])
            elif o is None:
                seen.add("none")
            else:
                if o in known:
                    seen.add("match_or_cap")
                    if len(known) >= kw["max_speakers"]:
                        seen.add("at_cap")
                else:
                    seen.add("new")
                    if not o.startswith("SPEAKER_"):
                        seen.add("named")
                known.add(o)
                labels.append(o)
    assert seen >= {"reset", "enroll", "enroll_none", "none", "match_or_cap", "at_cap", "new", "named"}, seen


def test_diarizer_surface():
    d = SpeakerDiarizer(embedder=lambda pcm, sr: np.eye(4)[0])
    assert (d.similarity_threshold, d.max_speakers, d.speaker_names) == (0.55, 10, [])
    assert d.identify_speaker(np.zeros(4799, np.float32)) is None            # under 0.3 s: no embedding, no speaker
    assert d.identify_speaker(np.zeros(4800, np.float32)) == "SPEAKER_00"
    assert d.enroll_speaker("x", np.zeros(100, np.float32)) is False
    d.reset()
    assert d.speakers == {} and d.identify_speaker(np.zeros(4800, np.float32)) == "SPEAKER_00"


# ---- artefact look-up ------------------------------------------------------------------------------------------------
def test_diarization_model_lookup_order(tmp_path, monkeypatch):
    monkeypatch.delenv("WLX_MODEL_ROOT", raising=False)
    monkeypatch.delenv("WLX_DIARIZATION_MODEL", raising=False)
    calls = []

    def snap(found):
        def f(repo, cache_dir, local_only):
            calls.append((repo, local_only))
            return found.get(local_only)
        return f

    def ckpt(d):
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "pytorch_model.bin"), "wb").close()
        return str(d)

    name = artifacts.DIARIZATION_MODEL
    assert name == "pyannote/wespeaker-voxceleb-resnet34-LM"
    # 1. an existing file or directory wins, the hub is not asked
    direct = ckpt(tmp_path / "direct")
    assert artifacts.resolve_diarization_model(direct, snapshot=snap({})) == direct
    f = os.path.join(direct, "pytorch_model.bin")
    assert artifacts.resolve_diarization_model(f, snapshot=snap({})) == f and calls == []
    # 2. $WLX_MODEL_ROOT/<name>, then its basename
    root = tmp_path / "root"
    monkeypatch.setenv("WLX_MODEL_ROOT", str(root))
    by_base = ckpt(root / "wespeaker-voxceleb-resnet34-LM")
    assert artifacts.resolve_diarization_model(snapshot=snap({})) == by_base
    by_name = ckpt(root / "pyannote" / "wespeaker-voxceleb-resnet34-LM")
    assert artifacts.resolve_diarization_model(name, snapshot=snap({})) == by_name and calls == []
    monkeypatch.delenv("WLX_MODEL_ROOT")
    # 3. the cache before any download; 4. the download only where allowed
    cached, fetched = ckpt(tmp_path / "cached"), ckpt(tmp_path / "fetched")
    assert artifacts.resolve_diarization_model(snapshot=snap({True: cached, False: fetched})) == cached
    assert calls == [(name, True)]
    calls.clear()
    monkeypatch.setenv("WLX_NO_DOWNLOAD", "1")
    assert artifacts.resolve_diarization_model(snapshot=snap({False: fetched})) is None and calls == [(name, True)]
    calls.clear()
    monkeypatch.setenv("WLX_NO_DOWNLOAD", "0")
    monkeypatch.delenv("HF_HUB_OFFLINE", raising=False)
    assert artifacts.resolve_diarization_model(snapshot=snap({False: fetched})) == fetched
    assert calls == [(name, True), (name, False)]
    assert artifacts.resolve_diarization_model(local_files_only=True, snapshot=snap({False: fetched})) is None
    # $WLX_DIARIZATION_MODEL replaces the default name; a bare word that is no directory is not a hub id
    calls.clear()
    monkeypatch.setenv("WLX_DIARIZATION_MODEL", "someone/other-model")
    assert artifacts.resolve_diarization_model(snapshot=snap({True: cached})) == cached and calls == [("someone/other-model", True)]
    assert artifacts.resolve_diarization_model("nothing-here", snapshot=snap({True: cached})) is None


# ---- server wiring ---------------------------------------------------------------------------------------------------
class TwoVoiceTranscriber:
    """one completed segment of 1 s per call and a tail, like tests/test_server.py's ScriptedTranscriber"""

    def transcribe(self, audio, **kw):
        dur = audio.shape[0] / 16000.0
        seg = [SimpleNamespace(start=0.0, end=min(dur, 1.0), text=" seg", no_speech_prob=0.0, words=None),
               SimpleNamespace(start=min(dur, 1.0), end=dur, text=" tail", no_speech_prob=0.0, words=None)]
        return seg, SimpleNamespace(language="en", language_probability=0.99)


def loudness_embedder(pcm, sr):
    """fake embedder: loud audio and quiet audio point in orthogonal directions"""
    return np.eye(4)[0] if float(np.abs(pcm).mean()) > 0.1 else np.eye(4)[1]


@pytest.fixture
def running_server():
    started = []

    def start(**attrs):
        srv, ready = TranscriptionServer(), threading.Event()
        for k, v in attrs.items():
            setattr(srv, k, v)
        t = threading.Thread(target=srv.run, args=("127.0.0.1",), daemon=True,
                             kwargs=dict(port=0, ready=ready, single_model=True, model_factory=lambda model, dev: TwoVoiceTranscriber()))
        t.start()
        assert ready.wait(10)
        started.append((srv, t))
        return srv

    ServeClientHIP.MODELS.clear()
    yield start
    for srv, t in started:
        srv.shutdown()
        t.join(5)
    ServeClientHIP.MODELS.clear()


OPTS = dict(uid="d1", language="en", task="transcribe", model="small.en", use_vad=False, send_last_n_segments=10,
            no_speech_thresh=0.45, clip_audio=False, same_output_threshold=10)


def _completed_segments(srv, opts, n_want=2):
    c = ws.connect(f"ws://127.0.0.1:{srv.port}")
    c.send(json.dumps(opts))
    assert json.loads(c.recv(timeout=10.0))["message"] == "SERVER_READY"
    t = np.arange(16000) * 0.05
    pcm = np.concatenate([0.5 * np.sign(np.sin(t)), 0.01 * np.sin(t), 0.5 * np.sign(np.sin(t)), 0.01 * np.sin(t)]).astype(np.float32)
    for i in range(0, pcm.shape[0], 4096):
        c.send(pcm[i: i + 4096].tobytes())
    done = {}
    for _ in range(400):
        msg = json.loads(c.recv(timeout=10.0))
        for s in msg.get("segments", []):
            if s.get("completed"):
                done[s["start"]] = s
        if len(done) >= n_want:
            break
    c.send(b"END_OF_AUDIO")
    c.close()
    return [done[k] for k in sorted(done, key=float)]


def test_server_labels_completed_segments_for_a_diarizing_client(running_server, tmp_path):
    ckpt = tmp_path / "pytorch_model.bin"
    ckpt.write_bytes(b"")
    made = []

    def factory(path, device):
        made.append((path, device))
        return loudness_embedder

    srv = running_server(diarization_model=str(ckpt), embedder_factory=factory)
    segs = _completed_segments(srv, dict(OPTS, enable_diarization=True, diarization_threshold=0.5, max_speakers=4), n_want=3)
    assert made == [(str(ckpt), 0)]
    assert [s["speaker"] for s in segs[:3]] == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_00"]
    # a client that does not ask gets no key
    segs = _completed_segments(srv, dict(OPTS, uid="d2"), n_want=2)
    assert all("speaker" not in s for s in segs)


def test_server_without_a_resolvable_model_runs_unlabelled_with_the_old_warning(running_server, tmp_path, caplog, monkeypatch):
    monkeypatch.delenv("WLX_MODEL_ROOT", raising=False)
    srv = running_server(diarization_model=str(tmp_path / "absent"))
    with caplog.at_level(logging.WARNING):
        segs = _completed_segments(srv, dict(OPTS, enable_diarization=True), n_want=2)
    assert segs and all("speaker" not in s for s in segs)
    assert "enable_diarization: speaker diarization is not part of this server; disabled" in caplog.text
