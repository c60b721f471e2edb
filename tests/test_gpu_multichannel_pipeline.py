"""GPU: BatchedInferencePipeline.transcribe(multichannel=True) on a real tiny.en engine (peaked weights, max_batch 8): every channel
of a file decodes to what the mono pipeline decodes from that channel alone, while the chunks of all channels share the decode groups.

The weights are the first seed of batched_common.SEEDS on which EVERY one of the twelve chunks — the six explicit chunks of waveform A
and of waveform B — decodes well conditioned (H.decode_is_well_conditioned at noise amplitude 0.02, the CPU oracle alone): seed 5
(searched on the CPU before this file was committed; the fixture asserts that the search succeeds, it never skips, and no chunk is
left out of a comparison)."""
import numpy as np
import pytest

from oracle import logmel as olm
from tests import batched_common as BC
from tests import helpers as H

from . import flac_writer as W

pytestmark = pytest.mark.gpu

KW = dict(language="en", temperature=0.0, max_new_tokens=BC.MAX_NEW, beam_size=5)


def audio_b() -> np.ndarray:
    return olm.speech_like_pcm(16.0, seed=4321).astype(np.float32)


def _quantized(x):
    """what a 16-bit file holds of the waveform, as float32 (so the WAV, the FLAC and the mono runs hear the same samples)"""
    q = np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    return q, (q / 32768.0).astype(np.float32)


@pytest.fixture(scope="module")
def setup(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    qa, a = _quantized(BC.audio16())
    qb, b = _quantized(audio_b())
    tk, sot, _sup = BC.pipeline_prompt_and_suppress(spec)
    prompt = sot + [tk.no_timestamps]
    seed, w, _oracle, refs = BC.find_conditioned([BC.explicit_chunks(a), BC.explicit_chunks(b)], [prompt, prompt])
    print("peaked seed used:", seed)
    hip = WhisperModelHIP("peaked", weights=w, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=8)
    stereo = np.stack([a, b], axis=1)
    q = np.stack([qa, qb], axis=1)
    flac = W.encode_stream(q, BC.SR, 16, W.split_blocks(q.shape[0], 4096), subframe={"type": "fixed", "order": 2, "k": 12},
                           assignment=W.MID_SIDE)
    yield dict(hip=hip, a=a, b=b, stereo=stereo, wav=BC.wav_bytes(stereo, BC.SR), flac=flac, refs=refs)
    hip.close()
    hip.engine.close()


def _run(hip, audio, **kw):
    from whisperlive_amd.batched import BatchedInferencePipeline
    segs, info = BatchedInferencePipeline(hip).transcribe(audio, **{**KW, **kw})
    return list(segs), info


def _explicit(hip, audio, batch_size, **kw):
    return _run(hip, audio, clip_timestamps=[dict(c) for c in BC.CLIPS], chunk_length=BC.CHUNK_LENGTH, vad_filter=False,
                batch_size=batch_size, **kw)


@pytest.fixture(scope="module")
def mono(setup):
    return [_explicit(setup["hip"], setup[k], 4)[0] for k in ("a", "b")]


def _same(got, want):
    assert len(got) == len(want) == 6
    for g, w in zip(got, want):
        assert (g.tokens, g.seek, g.start, g.end) == (w.tokens, w.seek, w.start, w.end)
        print(f"avg_logprob {g.avg_logprob:.6f} mono {w.avg_logprob:.6f}")
        assert abs(g.avg_logprob - w.avg_logprob) <= 2e-3 * abs(w.avg_logprob) + 1e-3        # the decode suites' score bound


@pytest.mark.parametrize("kind", ["wav", "flac", "waveform"])
def test_each_channel_equals_the_mono_pipeline_on_that_channel(setup, mono, kind):
    audio = setup["stereo"] if kind == "waveform" else setup[kind]
    segs, info = _explicit(setup["hip"], audio, 4, multichannel=True)
    assert [s.id for s in segs] == list(range(1, 13))
    assert [(s.start, s.channel) for s in segs] == sorted((s.start, s.channel) for s in segs)
    for c in (0, 1):
        _same([s for s in segs if s.channel == c], mono[c])
        for s, ref in zip([s for s in segs if s.channel == c], setup["refs"][c]):
            assert s.tokens == ref.sequences_ids[0]                                           # ... and the CPU oracle's tokens
    per = sum(c["end"] - c["start"] for c in BC.CLIPS) / BC.SR
    assert info.duration == 16.0 and abs(info.duration_after_vad - 2 * per) < 1e-9 and info.language == "en"


@pytest.mark.parametrize("batch_size", [1, 6])
def test_batch_size_does_not_change_the_tokens(setup, mono, batch_size):
    segs, _ = _explicit(setup["hip"], setup["wav"], batch_size, multichannel=True)
    for c in (0, 1):
        assert [s.tokens for s in segs if s.channel == c] == [s.tokens for s in mono[c]]


def test_one_upload_and_groups_that_mix_channels(setup, monkeypatch):
    from whisperlive_amd import engine as E
    calls = []
    for name in ("pcm_put", "put_frames", "put_frames_split", "logmel", "logmel_chunks", "encode"):
        real = getattr(E.Slot, name)
        monkeypatch.setattr(E.Slot, name, (lambda nm, rl: lambda self, *a, **k: (calls.append((nm, a, k)), rl(self, *a, **k))[1])(name, real))
    segs, _ = _explicit(setup["hip"], setup["wav"], 4, multichannel=True)
    assert len(segs) == 12
    assert [c[0] for c in calls] == ["put_frames_split"] + ["logmel_chunks", "encode"] * 3       # one upload, nothing put afterwards
    lm = [c for c in calls if c[0] == "logmel_chunks"]
    assert [len(c[1][0]) for c in lm] == [4, 4, 4]
    src = [list(c[2]["src_item"]) for c in lm]
    assert src == [[6, 6, 6, 6], [6, 6, 7, 7], [7, 7, 7, 7]]                                      # 12 chunks in (channel, start) order
    want = [[(c["start"], c["end"])] for c in BC.CLIPS]
    assert lm[0][1][0] + lm[1][1][0] + lm[2][1][0] == want + want


def test_a_mono_file_gives_the_multichannel_false_segments_on_channel_0(setup, mono):
    wav = BC.wav_bytes(setup["a"][:, None], BC.SR)
    segs, _ = _explicit(setup["hip"], wav, 4, multichannel=True)
    _same(segs, mono[0])
    assert {s.channel for s in segs} == {0} and [s.id for s in segs] == [s.id for s in mono[0]]
    segs, _ = _explicit(setup["hip"], setup["a"], 4, multichannel=True)                          # a 1-D waveform: channel 0 only
    _same(segs, mono[0])


@pytest.fixture(scope="module")
def gate(gpu):
    from whisperlive_amd import vad
    from whisperlive_amd.synthetic import energy_following_vad_weights
    m = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)
    yield m
    m.close()


def test_a_silent_second_channel_yields_channel_0_only_and_the_gate_runs_once(setup, gate, monkeypatch):
    from whisperlive_amd import vad
    hip = setup["hip"]
    monkeypatch.setattr(hip, "vad_model", gate)
    seen = []
    real = vad.SileroHIPModel.probs_pcm_many
    monkeypatch.setattr(vad.SileroHIPModel, "probs_pcm_many",
                        lambda self, slot, counts, first_item=0: (seen.append((list(counts), first_item)), real(self, slot, counts, first_item))[1])
    stereo = np.stack([setup["a"], np.zeros_like(setup["a"])], axis=1)
    segs, info = _run(hip, stereo, vad_filter=True, chunk_length=4, batch_size=4, multichannel=True)
    assert seen == [([16 * BC.SR] * 2, 6)]                                                        # one pass, both items
    want, wi = _run(hip, setup["a"], vad_filter=True, chunk_length=4, batch_size=4)
    assert segs and {s.channel for s in segs} == {0}
    assert [(s.tokens, s.seek, s.start, s.end) for s in segs] == [(s.tokens, s.seek, s.start, s.end) for s in want]
    assert info.duration == wi.duration == 16.0 and abs(info.duration_after_vad - wi.duration_after_vad) < 1e-9


def test_word_timestamps_lie_inside_their_chunks_span_per_channel(setup):
    """whole-second chunks (tests/test_gpu_batched_pipeline.py test_word_timestamps_on_two_chunks says why): explicit clips of 2 s and
    3 s, the same for both channels; a channel's chunks lie back to back on its concatenated timeline, [0, 2] and [2, 5]"""
    clips = [{"start": 0, "end": 2 * BC.SR}, {"start": 3 * BC.SR, "end": 6 * BC.SR}]
    segs, _ = _run(setup["hip"], setup["stereo"], clip_timestamps=clips, chunk_length=3, vad_filter=False, batch_size=3,
                   word_timestamps=True, multichannel=True)
    assert len(segs) == 4 and sorted(s.channel for s in segs) == [0, 0, 1, 1]
    for c in (0, 1):
        for s, (lo, hi) in zip([s for s in segs if s.channel == c], [(0.0, 2.0), (2.0, 5.0)]):
            assert s.words
            flat = [x for w in s.words for x in (w.start, w.end)]
            print("channel", c, "chunk span", lo, hi, "words", flat)
            assert flat == sorted(flat) and lo - 0.011 <= flat[0] and flat[-1] <= hi + 0.011, (c, flat, lo, hi)
            assert (s.start, s.end) == (s.words[0].start, s.words[-1].end)


def test_argument_errors(setup):
    from whisperlive_amd.batched import BatchedInferencePipeline
    hip = setup["hip"]
    p = BatchedInferencePipeline(hip)
    with pytest.raises(ValueError, match=r"batch_size 7 .*max_batch 8 - 2 channels"):
        p.transcribe(setup["wav"], batch_size=7, multichannel=True, **KW)
    with pytest.raises(ValueError, match=r"44101 Hz.*no host route"):
        p.transcribe(BC.wav_bytes(setup["stereo"][:4000], 44101), batch_size=4, multichannel=True, **KW)
    with pytest.raises(ValueError, match="3-dimensional"):
        p.transcribe(np.zeros((100, 2, 2), np.float32), batch_size=4, multichannel=True, **KW)
