"""GPU: BatchedInferencePipeline.transcribe_many on a real tiny.en engine (peaked weights, max_batch 8, batch_size 4): three files of
different lengths and routes — A, 16 s as a 16-bit WAV (put_frames); B, 16 s as FLAC (decoded on the device); C, the first 8.2 s of A as
a waveform (pcm_put) — decoded in groups that mix files, each file equal to `transcribe` of that file alone.

The weights are those of tests/test_gpu_multichannel_pipeline.py: the first seed of batched_common.SEEDS on which every one of the
twelve explicit chunks of A and B decodes well conditioned (the CPU oracle alone) — seed 5, searched on the CPU before this file was
committed; C's three chunks are A's first three. The fixture asserts that the search succeeds, it never skips, and no chunk is left
out of a comparison."""
import numpy as np
import pytest

from oracle import logmel as olm
from tests import batched_common as BC
from tests import helpers as H

from . import flac_writer as W
from . import wav_writer as WW

pytestmark = pytest.mark.gpu

KW = dict(language="en", temperature=0.0, max_new_tokens=BC.MAX_NEW, beam_size=5)
N_C = int(8.2 * BC.SR)
BATCH = 4                       # chunks per decode; the files sit in items 4, 5, 6 (, 7)
LANG_RTOL, LANG_ATOL = 2e-3, 2e-5          # tests/test_gpu_lean_family.py: batched detect_language against per-item calls


def _quantized(x):
    """what a 16-bit file holds of the waveform, as float32 (so the WAV, the FLAC and the waveform hear the same samples)"""
    q = np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    return q, (q / 32768.0).astype(np.float32)


def _flac(q):
    return W.encode_stream(q[:, None], BC.SR, 16, W.split_blocks(q.shape[0], 4096), subframe={"type": "fixed", "order": 2, "k": 12})


def _wav16(q):
    return WW.container(1, 1, BC.SR, 16, 2, q.astype("<i2").tobytes())


def _files():
    qa, a = _quantized(BC.audio16())
    qb, b = _quantized(olm.speech_like_pcm(16.0, seed=4321).astype(np.float32))
    return dict(a=a, b=b, A=_wav16(qa), B=_flac(qb), C=a[:N_C].copy())


@pytest.fixture(scope="module")
def setup(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    f = _files()
    tk, sot, _sup = BC.pipeline_prompt_and_suppress(spec)
    prompt = sot + [tk.no_timestamps]
    seed, w, _oracle, refs = BC.find_conditioned([BC.explicit_chunks(f["a"]), BC.explicit_chunks(f["b"])], [prompt, prompt])
    print("peaked seed used:", seed)
    hip = WhisperModelHIP("peaked", weights=w, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=8)
    yield dict(f, hip=hip, files=[f["A"], f["B"], f["C"]], refs=[refs[0], refs[1], refs[0][:3]])
    hip.close()
    hip.engine.close()


CLIPS = [[dict(c) for c in BC.CLIPS], [dict(c) for c in BC.CLIPS], [dict(c) for c in BC.CLIPS[:3]]]


def _pipe(hip):
    from whisperlive_amd.batched import BatchedInferencePipeline
    return BatchedInferencePipeline(hip)


def _single(hip, audio, **kw):
    segs, info = _pipe(hip).transcribe(audio, **{**KW, **kw})
    return list(segs), info


def _explicit_single(hip, i, audio, batch_size=BATCH, **kw):
    return _single(hip, audio, clip_timestamps=[dict(c) for c in CLIPS[i]], chunk_length=BC.CHUNK_LENGTH, vad_filter=False,
                   batch_size=batch_size, **kw)


def _explicit_many(hip, audios, batch_size=BATCH, clips=None, **kw):
    return _pipe(hip).transcribe_many(audios, clip_timestamps=[[dict(c) for c in cl] for cl in (clips or CLIPS)],
                                      chunk_length=BC.CHUNK_LENGTH, vad_filter=False, batch_size=batch_size, **{**KW, **kw})


@pytest.fixture(scope="module")
def alone(setup):
    return [_explicit_single(setup["hip"], i, audio) for i, audio in enumerate(setup["files"])]


def _same(got, want):
    assert len(got) == len(want) and want
    for g, w in zip(got, want):
        assert (g.tokens, g.seek, g.start, g.end, g.id, g.text) == (w.tokens, w.seek, w.start, w.end, w.id, w.text)
        print(f"avg_logprob {g.avg_logprob:.6f} alone {w.avg_logprob:.6f}")
        assert abs(g.avg_logprob - w.avg_logprob) <= 2e-3 * abs(w.avg_logprob) + 1e-3        # the decode suites' score bound


def test_each_file_equals_transcribe_of_that_file(setup, alone):
    out = _explicit_many(setup["hip"], setup["files"])
    assert len(out) == 3
    for i, ((segs, info), (want, winfo)) in enumerate(zip(out, alone)):
        assert len(segs) == (6, 6, 3)[i] and [s.id for s in segs] == list(range(1, len(segs) + 1))
        _same(segs, want)
        for s, ref in zip(segs, setup["refs"][i]):
            assert s.tokens == ref.sequences_ids[0]                                           # ... and the CPU oracle's tokens
        assert info.duration == winfo.duration == (16.0, 16.0, 8.2)[i] and info.language == winfo.language == "en"
        assert abs(info.duration_after_vad - winfo.duration_after_vad) < 1e-9 and info.language_probability == winfo.language_probability
        assert info.transcription_options == winfo.transcription_options and info.vad_options == winfo.vad_options


@pytest.mark.parametrize("batch_size", [1, 4])
def test_batch_size_does_not_change_the_tokens(setup, alone, batch_size):
    out = _explicit_many(setup["hip"], setup["files"], batch_size=batch_size)
    for (segs, _), (want, _w) in zip(out, alone):
        assert [s.tokens for s in segs] == [s.tokens for s in want]


def test_one_put_per_file_and_groups_that_mix_files(setup, monkeypatch):
    from whisperlive_amd import engine as E
    calls = []
    # (put_flac hands its frames to put_frames still compressed: the one way file frames reach a slot)
    for name in ("pcm_put", "put_frames", "put_frames_split", "put_wav", "logmel", "logmel_chunks", "encode"):
        real = getattr(E.Slot, name)
        monkeypatch.setattr(E.Slot, name, (lambda nm, rl: lambda self, *a, **k: (calls.append((nm, a, k)), rl(self, *a, **k))[1])(name, real))
    out = _explicit_many(setup["hip"], setup["files"])
    assert [len(segs) for segs, _ in out] == [6, 6, 3]
    assert [c[0] for c in calls] == ["put_frames", "put_frames", "pcm_put"] + ["logmel_chunks", "encode"] * 4    # ceil(15 / 4) groups
    # each file into its own item (put_flac names the item by position, the other routes by keyword)
    assert [c[2]["item"] if "item" in c[2] else c[1][-1] for c in calls[:3]] == [4, 5, 6]
    assert isinstance(calls[1][1][0], E.FlacFrames) and not isinstance(calls[0][1][0], E.FlacFrames)
    lm = [c for c in calls if c[0] == "logmel_chunks"]
    assert [list(c[2]["src_item"]) for c in lm] == [[4, 4, 4, 4], [4, 4, 5, 5], [5, 5, 5, 5], [6, 6, 6]]       # (file, start) order
    want = [[(c["start"], c["end"])] for c in BC.CLIPS]
    assert [r for c in lm for r in c[1][0]] == want + want + want[:3]


@pytest.fixture(scope="module")
def gate(gpu):
    from whisperlive_amd import vad
    from whisperlive_amd.synthetic import energy_following_vad_weights
    m = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    yield m
    m.close()


def test_one_gate_pass_for_the_wave_and_a_silent_file_changes_nothing(setup, gate, monkeypatch):
    from whisperlive_amd import vad
    hip = setup["hip"]
    monkeypatch.setattr(hip, "vad_model", gate)
    kw = dict(vad_filter=True, chunk_length=4, batch_size=BATCH)
    want = [_single(hip, audio, **kw) for audio in setup["files"]]
    seen = []
    real = vad.SileroHIPModel.probs_pcm_many
    monkeypatch.setattr(vad.SileroHIPModel, "probs_pcm_many",
                        lambda self, slot, counts, first_item=0: (seen.append((list(counts), first_item)), real(self, slot, counts, first_item))[1])
    three = _pipe(hip).transcribe_many(setup["files"], **{**KW, **kw})
    assert seen == [([16 * BC.SR, 16 * BC.SR, N_C], BATCH)]                                        # one pass, the files' own counts
    del seen[:]
    silent = np.zeros(5 * BC.SR, np.float32)
    four = _pipe(hip).transcribe_many(setup["files"] + [silent], **{**KW, **kw})
    assert seen == [([16 * BC.SR, 16 * BC.SR, N_C, 5 * BC.SR], BATCH)]
    assert four[3][0] == [] and four[3][1].duration_after_vad == 0 and four[3][1].duration == 5.0
    for out in (three, four[:3]):
        for (segs, info), (ws, wi) in zip(out, want):
            assert ws and info.transcription_options.clip_timestamps == wi.transcription_options.clip_timestamps       # the gate's clips
            assert [(s.tokens, s.seek, s.start, s.end, s.id) for s in segs] == [(s.tokens, s.seek, s.start, s.end, s.id) for s in ws]
            assert info.duration == wi.duration and abs(info.duration_after_vad - wi.duration_after_vad) < 1e-9
            assert 0 < info.duration_after_vad < info.duration


def test_a_prompt_per_file(setup):
    hip = setup["hip"]
    prompts = ["hello there", None, "a b c d e"]
    out = _explicit_many(hip, setup["files"], initial_prompt=prompts)
    for i, (segs, _info) in enumerate(out):
        want, _ = _explicit_single(hip, i, setup["files"][i], initial_prompt=prompts[i])
        _same(segs, want)


def test_word_timestamps_equal_the_single_runs(setup):
    """whole-second chunks (tests/test_gpu_batched_pipeline.py test_word_timestamps_on_two_chunks says why): clips of 2 s and 3 s in every
    file, six chunks in two groups, the first of which mixes files A and B"""
    hip = setup["hip"]
    clips = [{"start": 0, "end": 2 * BC.SR}, {"start": 3 * BC.SR, "end": 6 * BC.SR}]
    kw = dict(chunk_length=3, vad_filter=False, batch_size=BATCH, word_timestamps=True)
    out = _pipe(hip).transcribe_many(setup["files"], clip_timestamps=[clips] * 3, **{**KW, **kw})
    for (segs, _info), audio in zip(out, setup["files"]):
        want, _ = _single(hip, audio, clip_timestamps=[dict(c) for c in clips], **kw)
        assert len(segs) == len(want) == 2
        for g, w in zip(segs, want):
            assert g.words and (g.tokens, g.start, g.end) == (w.tokens, w.start, w.end)
            assert [(x.word, x.start, x.end) for x in g.words] == [(x.word, x.start, x.end) for x in w.words]      # exact boundaries
            assert max(abs(x.probability - y.probability) for x, y in zip(g.words, w.words)) <= 1e-3


def _damaged_flac():
    """a FLAC stream whose second frame's residual is a run of zero bits — a unary count that does not end inside the frame — with
    the frame's CRC-16 recomputed, so that the host index accepts the stream and the DEVICE decoder meets the bad frame
    (tests/test_gpu_multichannel_frontend.py builds its damaged frame the same way)"""
    rng = np.random.RandomState(5)
    pcm = rng.randint(-2000, 2000, size=(3 * 576, 1)).astype(np.int64)
    frames = W.encode_frames(pcm, BC.SR, 16, [576, 576, 576], subframe={"type": "fixed", "order": 1, "k": 11})
    body = bytearray(frames[1][:-2])
    for k in range(8, len(body) - 1):
        body[k] = 0x00
    f1 = bytes(body) + W.crc16(bytes(body)).to_bytes(2, "big")
    return W.metadata(W.streaminfo(pcm, BC.SR, 16, 576, 576)) + frames[0] + f1 + frames[2]


def test_a_damaged_file_costs_only_itself_and_leaves_nothing_stale(setup, alone):
    from whisperlive_amd.audio_io import flac_probe
    hip = setup["hip"]
    bad = _damaged_flac()
    assert flac_probe(bad).served                                                                 # the host probe passes
    clips = [CLIPS[0], [{"start": 0, "end": 1000}], CLIPS[2]]
    got = list(_pipe(hip).iter_many([setup["A"], bad, setup["C"]], clip_timestamps=clips, chunk_length=BC.CHUNK_LENGTH,
                                    vad_filter=False, batch_size=BATCH, **KW))
    assert [g[0] for g in got] == [0, 1, 2]
    assert isinstance(got[1][1], ValueError) and got[1][2] is None
    _same(got[0][1], alone[0][0])
    _same(got[2][1], alone[2][0])
    with pytest.raises(ValueError, match="damaged FLAC"):
        list(_pipe(hip).iter_many([setup["A"], bad, setup["C"]], clip_timestamps=clips, chunk_length=BC.CHUNK_LENGTH, vad_filter=False,
                                  batch_size=BATCH, on_error="raise", **KW))
    segs, _ = _explicit_single(hip, 1, setup["B"])                                                # a plain transcribe afterwards
    _same(segs, alone[1][0])


def test_a_language_per_file(gpu):
    """a multilingual tiny model: given languages are taken as given, the third file's is detected on its own leading chunks — in the
    batch of the wave — to the probability of the single-file run"""
    from whisperlive_amd.specs import SPECS
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = SPECS["tiny"]
    f = _files()
    hip = WhisperModelHIP("peaked", weights=H.peaked_weights(spec, 5), spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=8,
                          multilingual=True)
    try:
        files, languages = [f["A"], f["B"], f["C"]], ["en", "de", None]
        kw = dict(temperature=0.0, max_new_tokens=4, beam_size=5, chunk_length=BC.CHUNK_LENGTH, vad_filter=False, batch_size=BATCH)
        out = _pipe(hip).transcribe_many(files, language=languages, clip_timestamps=CLIPS, **kw)
        # ... and two files to detect in one wave: one encode, one detect_language for both
        both = _pipe(hip).transcribe_many([f["C"], f["B"]], language=None, clip_timestamps=[CLIPS[2], CLIPS[1]], **kw)
        for i, (segs, info) in enumerate(out):
            ws, wi = _pipe(hip).transcribe(files[i], language=languages[i], clip_timestamps=[dict(c) for c in CLIPS[i]], **kw)
            ws = list(ws)
            assert info.language == wi.language and len(segs) == len(ws)
            print("file", i, info.language, info.language_probability, wi.language_probability)
            if languages[i] is not None:
                assert info.language == languages[i] and info.language_probability == wi.language_probability == 1
            else:
                assert abs(info.language_probability - wi.language_probability) <= LANG_RTOL * wi.language_probability + LANG_ATOL
                got, want = dict(info.all_language_probs), dict(wi.all_language_probs)
                assert set(got) == set(want)
                assert all(abs(got[k] - want[k]) <= LANG_RTOL * want[k] + LANG_ATOL for k in want)
                assert both[0][1].language == wi.language
                assert abs(both[0][1].language_probability - wi.language_probability) <= LANG_RTOL * wi.language_probability + LANG_ATOL
        wb = _pipe(hip).transcribe(f["B"], language=None, clip_timestamps=[dict(c) for c in CLIPS[1]], **kw)[1]
        assert both[1][1].language == wb.language
        assert abs(both[1][1].language_probability - wb.language_probability) <= LANG_RTOL * wb.language_probability + LANG_ATOL
    finally:
        hip.close()
        hip.engine.close()


def test_the_slots_tracked_row_length_is_the_one_the_chunk_gather_is_refused_by(gpu):
    """What sizes the waves (many_files.next_wave: multichannel.source_rows_addressable on Slot.pcm_longest) against what the library
    refuses (wlx_logmel_chunks_multi: source rows past 2^31 - 1 samples apart, at the slot's REAL row stride), at the boundary: after
    one hour-long put the rows of a 40-item slot are 57.6e6 samples long and stay so, 37 neighbouring rows are addressable and 38 are
    not — for chunks of half a second out of short audio put afterwards."""
    from whisperlive_amd import _lib
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.multichannel import source_rows_addressable
    from whisperlive_amd.weights import random_weights
    spec = H.TINY_EN
    eng = HipWhisperEngine(spec, random_weights(spec, seed=7), device=0)
    slot = eng.create_slot(40, 5)
    try:
        assert slot.pcm_longest == 480000
        hour = 3600 * BC.SR
        slot.pcm_put(np.zeros(hour, np.float32), item=39)
        assert slot.pcm_longest == hour
        short = BC.audio16()[:BC.SR]
        for item in (1, 2, 3, 39):
            slot.pcm_put(short, item=item)                                   # the long audio is gone; the rows stay as long
        assert slot.pcm_longest == hour
        chunk = [(0, BC.SR // 2)]
        assert source_rows_addressable(37, slot.pcm_longest) and not source_rows_addressable(38, slot.pcm_longest)
        frames = slot.logmel_chunks([chunk, chunk], src_item=[3, 39], first_item=0)           # 37 rows from the lowest to the highest
        assert frames == [51, 51]
        with pytest.raises(_lib.WlxError) as ei:
            slot.logmel_chunks([chunk, chunk], src_item=[2, 39], first_item=0)                # 38 rows: refused, nothing launched
        assert ei.value.code == _lib.ERR_ARG
    finally:
        slot.close()
        eng.close()
