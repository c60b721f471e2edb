"""GPU tests of the HIP M2M100 translation engine (wlx_mt_*): encoder output and teacher-forced logits against the torch
restatement (tests/mt_oracle.py, fp16-rounded matrices as the engine uses them), generate() tokens against the transformers
recording (tests/golden/mt_golden.json, made by make_mt_golden.py) at the fixture config and against the restatement at small100's
full dimensions, batching, a max_src source, an ASR slot running beside a translation slot, and the server side channel.
No real small100 checkpoint exists offline: parity rests on seeded weights."""
from __future__ import annotations

import dataclasses
import json
import os
import threading

import numpy as np
import pytest

from whisperlive_amd.mt_weights import SMALL100, MTGenOptions, MTSpec, random_mt_weights

from .mt_oracle import M2M100Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "mt_golden.json")))
ARR = np.load(os.path.join(HERE, "golden", "mt_golden.npz"))
FIX = MTSpec(**GOLD["spec"])
# full small100 dimensions; decoder start <> EOS for the seeded weights (see random_mt_weights)
FULL = dataclasses.replace(SMALL100, decoder_start_id=0)


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))


def opts_of(c):
    return MTGenOptions(num_beams=c["num_beams"], max_length=c["max_length"], early_stopping=c["early_stopping"],
                        length_penalty=c["length_penalty"], no_repeat_ngram_size=c.get("no_repeat_ngram_size", 0),
                        forced_eos_token_id=c.get("forced_eos_token_id"))


def strip(seq, spec):
    s = seq[1:]
    if spec.eos_id in s:
        s = s[:s.index(spec.eos_id)]
    return s


@pytest.fixture(scope="module")
def fix():
    from whisperlive_amd.translation import HipMTEngine
    w = random_mt_weights(FIX, seed=GOLD["seed"], peaked=GOLD["peaked"])
    eng = HipMTEngine(FIX, w, device=0, max_batch=8, max_rows=5, max_src=128)
    yield eng, w
    eng.close()


@pytest.fixture(scope="module")
def full():
    from whisperlive_amd.translation import HipMTEngine
    w = random_mt_weights(FULL, seed=3, peaked=True)
    eng = HipMTEngine(FULL, w, device=0, max_batch=2, max_rows=5, max_src=1024)
    yield eng, M2M100Oracle(FULL, w, fp16_matrices=True)
    eng.close()


def test_encoder_output_fixture(fix):
    eng, w = fix
    orc = M2M100Oracle(FIX, w, fp16_matrices=True)
    srcs = [GOLD["sources"][0], GOLD["sources"][4]]
    got = eng.encoder_output(srcs)
    n0 = len(srcs[0])
    ref = np.concatenate([orc.encode(s).numpy() for s in srcs])
    assert rel_rms(got, ref) <= 2e-3
    # and against transformers' own encoder (fp32 weights): the fp16 rounding of the engine's matrices is all that differs
    assert rel_rms(got[:n0], ARR["enc_0"][:n0]) <= 1e-2
    assert rel_rms(got[n0:n0 + 8], ARR["enc_4"]) <= 1e-2


def test_teacher_forced_logits_fixture(fix):
    eng, w = fix
    orc = M2M100Oracle(FIX, w, fp16_matrices=True)
    src, dec = GOLD["sources"][GOLD["tf_source"]], GOLD["tf_decoder"]
    got = eng.decoder_logits(src, dec)
    ref = orc.decode_logits(orc.encode(src), dec).numpy()
    assert rel_rms(got, ref) <= 2e-3
    assert rel_rms(got[GOLD["tf_rows"]], ARR["tf_logits"]) <= 1e-2


def test_full_dims_encoder_and_logits(full):
    eng, orc = full
    rng = np.random.default_rng(7)
    src = [128000] + [int(x) for x in rng.integers(4, 128000, size=29)] + [2]
    got = eng.encoder_output([src])
    enc = orc.encode(src)
    assert rel_rms(got, enc.numpy()) <= 2e-3
    dec = [0, 17, 99, 12345]
    lg = eng.decoder_logits(src, dec)
    assert rel_rms(lg, orc.decode_logits(enc, dec).numpy()) <= 2e-3


@pytest.mark.parametrize("case", [c["name"] for c in GOLD["cases"]])
def test_translate_matches_transformers_golden(fix, case):
    eng, _ = fix
    c = next(x for x in GOLD["cases"] if x["name"] == case)
    toks, scores = eng.translate_ids(GOLD["sources"], opts_of(c))
    for i, r in enumerate(c["results"]):
        assert toks[i] == strip(r["sequence"], FIX), (case, i)
        if r["score"] is not None:
            assert abs(scores[i] - r["score"]) <= 2e-3 * max(1.0, abs(r["score"])), (case, i, scores[i], r["score"])


def test_batch_equals_single_calls(fix):
    eng, _ = fix
    o = MTGenOptions(num_beams=5, max_length=40, early_stopping=True, length_penalty=1.0)
    srcs = GOLD["sources"]
    assert len(srcs) == 8 and len({len(s) for s in srcs}) == 8
    batched, bs = eng.translate_ids(srcs, o)
    for i, s in enumerate(srcs):
        t, sc = eng.translate_ids([s], o)
        assert t[0] == batched[i]
        assert abs(sc[0] - bs[i]) <= 1e-4


def test_source_of_max_src_tokens(fix):
    eng, w = fix
    orc = M2M100Oracle(FIX, w, fp16_matrices=True)
    rng = np.random.default_rng(9)
    src = [2000] + [int(x) for x in rng.integers(4, 1900, size=eng.max_src - 2)] + [FIX.eos_id]
    assert len(src) == eng.max_src
    got = eng.encoder_output([src])
    assert rel_rms(got, orc.encode(src).numpy()) <= 2e-3
    o = MTGenOptions(num_beams=1, max_length=30)
    toks, _ = eng.translate_ids([src], o)
    ref, _ = orc.generate([src], o)
    assert toks[0] == ref[0]
    from whisperlive_amd._lib import WlxError
    with pytest.raises(WlxError):
        eng.translate_ids([src + [5]], o)


def _forced_score(orc, src, seq, o, eos=True):
    """HF's beam score of `seq` (generated tokens, without the decoder start; with the final EOS unless the hypothesis ran to
    max_length) under the restatement's own forced decoding"""
    full = [orc.spec.decoder_start_id] + list(seq) + ([orc.spec.eos_id] if eos else [])
    lp = orc.decode_logits(orc.encode(src), full[:-1]).log_softmax(-1)
    s = float(sum(lp[i, full[i + 1]] for i in range(len(full) - 1)))
    return s / (len(full) - 1) ** o.length_penalty


def _near_tie(orc, src, a, b, o, eos=True):
    """the two hypotheses score within 2e-3 under the restatement's own forced decoding"""
    return abs(_forced_score(orc, src, a, o, eos) - _forced_score(orc, src, b, o, eos)) <= 2e-3


def test_full_dims_translate_against_oracle(full):
    eng, orc = full
    rng = np.random.default_rng(11)
    srcs = [[128010] + [int(x) for x in rng.integers(4, 128000, size=L)] + [2] for L in (6, 21)]
    for o in (MTGenOptions(num_beams=1, max_length=24), MTGenOptions(num_beams=5, max_length=24, early_stopping=True)):
        toks, _ = eng.translate_ids(srcs, o)
        ref, _ = orc.generate(srcs, o)
        for i in range(len(srcs)):
            assert toks[i] == ref[i] or (o.num_beams > 1 and _near_tie(orc, srcs[i], toks[i], ref[i], o)), (o, i, toks[i], ref[i])


def test_asr_tokens_unchanged_by_concurrent_translation(fix):
    from oracle import logmel as olm
    from whisperlive_amd.engine import HipWhisperEngine, TokenIds
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.weights import random_weights
    eng_mt, _ = fix
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
        o = MTGenOptions(num_beams=5, max_length=40, early_stopping=True)
        mt_solo = eng_mt.translate_ids(GOLD["sources"], o)
        stop = threading.Event()
        errs, mt_together = [], []

        def translate_loop():
            try:
                while not stop.is_set():
                    mt_together.append(eng_mt.translate_ids(GOLD["sources"], o))
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = threading.Thread(target=translate_loop)
        th.start()
        try:
            together = [run() for _ in range(3)]
        finally:
            stop.set()
            th.join(timeout=120)
        assert not errs, errs
        assert all(t == solo for t in together)
        # and the translations made under contention are those of a solo call (tokens and scores)
        assert mt_together and all(r == mt_solo for r in mt_together)
    finally:
        slot.close()
        asr.close()


def test_server_client_receives_translated_segments(tmp_path, fix):
    """a translating client through TranscriptionServer.initialize_client: the seeded fixture model saved as a checkpoint
    directory, a completed segment on the transcription client's queue -> a translated_segments message from the HIP engine"""
    import shutil

    from safetensors.numpy import save_file

    from whisperlive_amd import server as srv
    from whisperlive_amd import translation as tr
    _, w = fix
    d = tmp_path / "small100-seeded"
    d.mkdir()
    json.dump(FIX.hf_config(), open(d / "config.json", "w"))
    json.dump({"num_beams": 5, "max_length": 40, "early_stopping": True}, open(d / "generation_config.json", "w"))
    save_file({k: np.ascontiguousarray(v) for k, v in w.items()}, str(d / "model.safetensors"))
    for f in ("vocab.json", "sentencepiece.bpe.model", "tokenizer_config.json"):     # (the full code list: no transformers)
        shutil.copy(os.path.join(HERE, "golden", "mt_tok", f), d / f)

    class FakeWS:
        def __init__(self):
            self.sent = []

        def send(self, m):
            self.sent.append(json.loads(m))

        def close(self):
            pass

    class FakeTranscriber:
        pass

    server = srv.TranscriptionServer()
    server.client_manager = srv.ClientManager()
    server.translation_model = str(d)
    server.model_factory = lambda model, device: FakeTranscriber()
    ws = FakeWS()
    opts = {"uid": "c1", "language": "en", "task": "transcribe", "model": "mt-server-test", "enable_translation": True,
            "target_language": "de", "use_vad": False}
    server.initialize_client(ws, opts, None, None, False)
    client = server.client_manager.get_client(ws)
    assert client and client.translation_queue is not None
    try:
        client.translation_queue.put({"start": "0.000", "end": "1.000", "text": "Hello world.", "completed": True})
        client.translation_queue.put({"start": "1.000", "end": "2.000", "text": "unfinished", "completed": False})
        client.translation_queue.join()
        msgs = [m for m in ws.sent if "translated_segments" in m]
        assert len(msgs) == 1 and msgs[0]["uid"] == "c1"
        seg = msgs[0]["translated_segments"][0]
        assert seg["target_language"] == "de" and seg["completed"] and (seg["start"], seg["end"]) == ("0.000", "1.000")
        ref = tr.shared_translator(str(d), client.translation_client.device)
        assert isinstance(ref.engine, tr.HipMTEngine)
        assert seg["text"] == ref.translate(["Hello world."], "de")[0]
    finally:
        server.cleanup(ws)
        srv.ServeClientHIP.MODELS.pop((0, "mt-server-test"), None)
    assert not client.translation_thread.is_alive()


# ------------------------------------------------------------------ the regime small100 runs in: long beam decodes, 16 beams,
# 448-token KV caches, 1024-token sources
@pytest.fixture(scope="module")
def long_fix():
    """the fixture's dimensions with the EOS row of the tied embedding at zero, on a 16-row slot: the EOS logit is 0 at every
    step, far below the top 2 x num_beams of 2112 logits of unit spread, so no beam finishes before max_length. (A large
    negative eos_margin of random_mt_weights(peaked=True) does not do it: the direction it adds meets the decoder's hidden state
    with either sign, and at the first steps it lifts EOS above everything.)"""
    from whisperlive_amd.translation import HipMTEngine
    w = random_mt_weights(FIX, seed=GOLD["seed"])
    w["model.shared.weight"][FIX.eos_id] = 0.0
    eng = HipMTEngine(FIX, w, device=0, max_batch=1, max_rows=16, max_src=128)
    yield eng, M2M100Oracle(FIX, w, fp16_matrices=True)
    eng.close()


def _beam_against_oracle(eng, orc, srcs, o, n_expect=None):
    toks, scores = eng.translate_ids(srcs, o)
    ref, ref_scores = orc.generate(srcs, o)
    for i, src in enumerate(srcs):
        if n_expect is not None:
            assert len(toks[i]) == n_expect and len(ref[i]) == n_expect, (i, len(toks[i]), len(ref[i]))
        ended = n_expect is None
        # tie-independent: the engine's score is that of its own hypothesis (a wrong ancestry gather scores another history)
        fs = _forced_score(orc, src, toks[i], o, eos=ended)
        assert abs(scores[i] - fs) <= 2e-3 * max(1.0, abs(fs)), (i, scores[i], fs)
        if toks[i] != ref[i]:
            assert _near_tie(orc, src, toks[i], ref[i], o, eos=ended), (i, toks[i], ref[i])
        else:
            assert abs(scores[i] - ref_scores[i]) <= 2e-3 * max(1.0, abs(ref_scores[i])), (i, scores[i], ref_scores[i])


def test_beam_decode_to_max_length_200(long_fix):
    """5 beams to max_length 200 (small100's generation config): the decoder self-attention crosses four key tiles through
    the ancestry table; every hypothesis runs to max_length (199 tokens, EOS pushed down)"""
    eng, orc = long_fix
    srcs = [GOLD["sources"][1]]
    _beam_against_oracle(eng, orc, srcs, MTGenOptions(num_beams=5, max_length=200, early_stopping=True), n_expect=199)


def test_sixteen_beams(long_fix):
    """num_beams 16: 32 candidates per row (top-k at its limit) and 16-row cross-attention groups (the four-wave kernel)"""
    eng, orc = long_fix
    srcs = [GOLD["sources"][3]]
    _beam_against_oracle(eng, orc, srcs, MTGenOptions(num_beams=16, max_length=40, early_stopping=True), n_expect=39)


def test_teacher_forced_logits_448_tokens(fix):
    """the whole KV cache: 448 decoder tokens (WLX_T_TEXT), seven key tiles of the self-attention"""
    eng, w = fix
    orc = M2M100Oracle(FIX, w, fp16_matrices=True)
    rng = np.random.default_rng(13)
    src = GOLD["sources"][2]
    dec = [FIX.decoder_start_id] + [int(x) for x in rng.integers(3, FIX.vocab, size=447)]
    got = eng.decoder_logits(src, dec)
    ref = orc.decode_logits(orc.encode(src), dec).numpy()
    assert got.shape == ref.shape == (448, FIX.vocab)
    assert rel_rms(got, ref) <= 2e-3
    assert rel_rms(got[384:], ref[384:]) <= 2e-3          # the last tile on its own


def test_full_dims_source_of_1024_tokens(full):
    """a 1024-token source (WLX_MT_MAX_SRC) at small100 dimensions: 16 key tiles in the encoder and the cross-attention"""
    eng, orc = full
    rng = np.random.default_rng(17)
    src = [128000] + [int(x) for x in rng.integers(4, 128000, size=1022)] + [2]
    assert len(src) == 1024
    got = eng.encoder_output([src])
    assert rel_rms(got, orc.encode(src).numpy()) <= 2e-3
    o = MTGenOptions(num_beams=1, max_length=8)
    toks, _ = eng.translate_ids([src], o)
    ref, _ = orc.generate([src], o)
    assert toks[0] == ref[0]
