"""GPU: the fallback of a chunk with more ranges than the log-mel kernel's table (LM_MAXRANGES) on the device route of BOTH routes of
BatchedInferencePipeline.transcribe, through the one DeviceChunks.to_device: a tiny.en engine (peaked weights, max_batch 4), explicit
clips of LM_MAXRANGES + 1 ranges of 160 samples that collect_chunks keeps in one chunk, and normal chunks of the same length beside it.

The weights are the first seed of batched_common.SEEDS on which EVERY chunk compared here — the oversize chunk (its host
concatenation) and the normal chunks of waveform A and of waveform B — decodes well conditioned (H.decode_is_well_conditioned at noise
amplitude 0.02, the CPU oracle alone): seed 5 (searched on the CPU before this file was committed; the fixture asserts that the
search succeeds, it never skips, and no chunk is left out of a comparison)."""
import numpy as np
import pytest

from oracle import logmel as olm
from tests import batched_common as BC
from tests import helpers as H
from whisperlive_amd._lib import LM_MAXRANGES

pytestmark = pytest.mark.gpu

KW = dict(language="en", temperature=0.0, max_new_tokens=BC.MAX_NEW, beam_size=5, vad_filter=False)
N = (LM_MAXRANGES + 1) * 160                                        # samples of every chunk here: 2.57 s
MANY = [{"start": 180 * i, "end": 180 * i + 160} for i in range(LM_MAXRANGES + 1)]           # ends at 46240: inside 3 s
NORMAL = [{"start": 3 * BC.SR, "end": 3 * BC.SR + N}, {"start": 6 * BC.SR, "end": 6 * BC.SR + N}]
CHUNK_LENGTH = (N + 80) / BC.SR                                     # a chunk closes after N samples, whatever the rounding


def _chunks(audio, clips_per_chunk):
    return [np.concatenate([audio[c["start"]:c["end"]] for c in clips]) for clips in clips_per_chunk]


@pytest.fixture(scope="module")
def setup(gpu):
    from whisperlive_amd.tokenizer import synthetic_tokenizer
    from whisperlive_amd.transcriber import WhisperModelHIP
    spec = H.TINY_EN
    a = BC.audio16()[: 9 * BC.SR]
    b = olm.speech_like_pcm(9.0, seed=4321).astype(np.float32)
    tk, sot, _sup = BC.pipeline_prompt_and_suppress(spec)
    prompt = sot + [tk.no_timestamps]
    per_chunk = [MANY, [NORMAL[0]], [NORMAL[1]]]
    seed, w, _oracle, refs = BC.find_conditioned([_chunks(a, per_chunk), _chunks(b, per_chunk[:2])], [prompt, prompt])
    print("peaked seed used:", seed)
    hip = WhisperModelHIP("peaked", weights=w, spec=spec, hf_tokenizer=synthetic_tokenizer(spec.vocab), max_batch=4)
    yield dict(hip=hip, a=a, b=b, refs=refs)
    hip.close()
    hip.engine.close()


def _run(hip, audio, clips, **kw):
    from whisperlive_amd.batched import BatchedInferencePipeline
    segs, info = BatchedInferencePipeline(hip).transcribe(audio, clip_timestamps=[dict(c) for c in clips], chunk_length=CHUNK_LENGTH,
                                                          batch_size=2, **{**KW, **kw})
    return list(segs), info


@pytest.mark.parametrize("seconds, clips", [(3, MANY), (6, MANY + NORMAL[:1])], ids=["oversize_chunks_only", "a_normal_chunk_beside_each"])
def test_multichannel_fallback_on_the_device_route_equals_the_mono_pipeline_per_channel(setup, seconds, clips, monkeypatch):
    from whisperlive_amd import engine as E
    hip = setup["hip"]
    waves = [setup[k][: seconds * BC.SR] for k in ("a", "b")]
    mono = [_run(hip, w, clips)[0] for w in waves]
    calls = []
    for name in ("logmel", "logmel_chunks"):
        real = getattr(E.Slot, name)
        monkeypatch.setattr(E.Slot, name, (lambda nm, rl: lambda self, *a, **k: (calls.append((nm, a, k)), rl(self, *a, **k))[1])(name, real))
    segs, info = _run(hip, np.stack(waves, axis=1), clips, multichannel=True)
    per = len(clips) - LM_MAXRANGES                                # chunks per channel: the oversize one, and the normal one
    # the oversize chunk of each channel went through the host concatenation, into its own destination item, in front of the sources
    assert [(c[0], c[2].get("item")) for c in calls if c[0] == "logmel"] == ([("logmel", 0), ("logmel", 1)] if per == 1 else [("logmel", 0)] * 2)
    assert [(list(c[2]["src_item"]), c[2]["first_item"]) for c in calls if c[0] == "logmel_chunks"] == ([] if per == 1 else [([2], 1), ([3], 1)])
    assert len(segs) == 2 * per and [s.id for s in segs] == list(range(1, 2 * per + 1))
    for c in (0, 1):
        got = [s for s in segs if s.channel == c]
        assert len(got) == len(mono[c]) == per
        for g, w, ref in zip(got, mono[c], setup["refs"][c]):
            assert (g.tokens, g.seek, g.start, g.end) == (w.tokens, w.seek, w.start, w.end)
            assert g.tokens == ref.sequences_ids[0]                                     # ... and the CPU oracle's, on the host concatenation
            print(f"channel {c}: avg_logprob {g.avg_logprob:.6f} mono {w.avg_logprob:.6f}")
            assert abs(g.avg_logprob - w.avg_logprob) <= 2e-3 * abs(w.avg_logprob) + 1e-3   # the decode suites' score bound
    assert info.duration == float(seconds) and abs(info.duration_after_vad - 2 * per * N / BC.SR) < 1e-9


def test_mono_fallback_evicts_the_waveform_and_it_goes_up_again_exactly_once(setup, monkeypatch):
    """groups [oversize, normal] and [normal]: the oversize chunk's host concatenation lands in item 0, over the resident waveform,
    after the group's normal chunk has been cut from it; the second group needs the waveform again"""
    from whisperlive_amd import engine as E
    calls = []
    for name in ("pcm_put", "logmel", "logmel_chunks"):
        real = getattr(E.Slot, name)
        monkeypatch.setattr(E.Slot, name, (lambda nm, rl: lambda self, *a, **k: (calls.append((nm, a, k)), rl(self, *a, **k))[1])(name, real))
    segs, _ = _run(setup["hip"], setup["a"], MANY + NORMAL)
    assert [c[0] for c in calls] == ["pcm_put", "logmel_chunks", "logmel", "pcm_put", "logmel_chunks"]      # one upload, one more after the eviction
    assert calls[3][1][0].shape == setup["a"].shape and np.array_equal(calls[3][1][0], setup["a"])
    assert len(segs) == 3 and [s.tokens for s in segs] == [r.sequences_ids[0] for r in setup["refs"][0]]
    assert [(s.id, s.start, s.end) for s in segs] == [(i + 1, round(i * N / BC.SR, 3), round((i + 1) * N / BC.SR, 3)) for i in range(3)]
