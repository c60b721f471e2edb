"""Host logic of the one file plan behind BatchedInferencePipeline.transcribe (batched._plan) on the scripted front end
(tests/fakes.py FrontEndSlot): the refusals both routes share are the same refusal, DeviceChunks.to_device with one source item per
chunk, and the one unpacking of an alignment result."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests.fakes import FrontEndEngine
from whisperlive_amd import word_timing as WT
from whisperlive_amd._lib import LM_MAXRANGES
from whisperlive_amd.batched import BatchedInferencePipeline, DeviceChunks
from whisperlive_amd.specs import WhisperSpec
from whisperlive_amd.tokenizer import synthetic_tokenizer
from whisperlive_amd.transcriber import WhisperModelHIP

SR = 16000


def _pipeline(max_batch):
    eng = FrontEndEngine(WhisperSpec(80, 128, 2, 1, 1, 512, 2310))
    eng.default_tokens = [300, 301, 302]
    hip = WhisperModelHIP("fake", engine=eng, hf_tokenizer=synthetic_tokenizer(eng.spec.vocab), max_batch=max_batch)
    return BatchedInferencePipeline(hip), eng


# (what is asked, the refusal) — every refusal the two routes share
REFUSALS = {
    "batch_size_below_1": (dict(audio=np.zeros(SR, np.float32), batch_size=0), ValueError, r"batch_size 0: at least one chunk"),
    "more_than_320_decoder_rows": (dict(audio=np.zeros(SR, np.float32), batch_size=64, beam_size=6), ValueError,
                                   r"batch_size 64 x beam_size 6 = 384 decoder rows: one decode step holds at most 320"),
    "no_clips_no_gate_long_file": (dict(audio=np.zeros(31 * SR, np.float32), vad_filter=False, batch_size=2), RuntimeError,
                                   r"No clip timestamps found. Set 'vad_filter' to True or provide 'clip_timestamps'\."),
    "not_audio": (dict(audio=12345, batch_size=2), TypeError, r"audio must be a float32 numpy waveform at 16 kHz, or a WAV / FLAC"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_a_shared_refusal_is_the_same_on_both_routes(case):
    kw, kind, text = REFUSALS[case]
    raised = []
    for multichannel in (False, True):
        pipe, _eng = _pipeline(max_batch=64)                # (the most a slot holds: batch_size 64 passes the mono max_batch check)
        with pytest.raises(kind, match=text) as ei:
            pipe.transcribe(**kw, multichannel=multichannel)
        raised.append(ei.value)
    assert type(raised[0]) is type(raised[1]) is kind and str(raised[0]) == str(raised[1])


def _few(base):
    return [(base + 1000 * i, base + 1000 * i + 600) for i in range(10)]


MANY = [(100000 + 40 * i, 100000 + 40 * i + 20) for i in range(LM_MAXRANGES + 1)]


def _concat(audio, ranges):
    return np.concatenate([audio[s:e] for s, e in ranges])


def test_per_chunk_sources_runs_on_either_side_and_the_oversize_chunk_reads_its_own_source():
    _pipe, eng = _pipeline(max_batch=6)
    slot = eng.create_slot(6, 5)
    waves = {4: np.arange(16 * SR, dtype=np.float32), 5: -np.arange(16 * SR, dtype=np.float32)}
    for item, w in waves.items():
        slot.pcm_put(w, item)
    slot.calls.clear()
    group = DeviceChunks(slot, [_few(0), MANY, _few(200000), _few(50000)], slot.pcm, [4, 5, 5, 4], 16 * SR)
    frames = group.to_device()
    assert slot.calls == [("logmel_chunks", [10], [4], 0), ("logmel_chunks", [10, 10], [5, 4], 2), ("pcm", 5),
                          ("logmel", 1, 20 * (LM_MAXRANGES + 1))]
    np.testing.assert_array_equal(slot.logmel_audio[1], _concat(waves[5], MANY))           # its own source's audio, not item 4's
    assert frames == [(6000 + 160) // 160, (20 * (LM_MAXRANGES + 1) + 160) // 160] + [(6000 + 160) // 160] * 2
    assert group.shared["resident"] is True                                               # item 1 is no source: nothing was evicted
    group[1:3].to_device()                                                                # (a slice shares the state and the host copy)
    assert [c for c in slot.calls[4:] if c[0] in ("pcm", "pcm_put")] == []
    with pytest.raises(ValueError, match=r"a group of 4 chunks would overwrite source item 3"):
        DeviceChunks(slot, [_few(0)] * 4, slot.pcm, [4, 3, 4, 4], 16 * SR).to_device()


def test_a_mono_fallback_into_item_0_evicts_the_source_and_the_next_group_puts_it_back():
    _pipe, eng = _pipeline(max_batch=3)
    slot = eng.create_slot(3, 5)
    wave = np.arange(16 * SR, dtype=np.float32)
    chunks = DeviceChunks(slot, [MANY, _few(0), _few(200000)], wave, 0, 16 * SR)
    assert chunks[1:3].to_device() and chunks.shared["resident"] is True                  # no fallback: nothing evicted
    slot.calls.clear()
    chunks[0:2].to_device()
    assert slot.calls == [("logmel_chunks", [10], 0, 1), ("logmel", 0, 20 * (LM_MAXRANGES + 1))]      # an int source: wlx_logmel_chunks
    np.testing.assert_array_equal(slot.logmel_audio[0], _concat(wave, MANY))
    assert chunks.shared["resident"] is False                                             # the chunk landed in the source item
    chunks[2:3].to_device()
    assert slot.calls[2:] == [("pcm_put", 0, 16 * SR), ("logmel_chunks", [10], 0, 0)] and chunks.shared["resident"] is True
    np.testing.assert_array_equal(slot.resident[0], wave)
    # a fallback that lands elsewhere leaves the source alone
    other = DeviceChunks(slot, [_few(0), MANY], wave, 0, 16 * SR)
    other.to_device()
    assert other.shared["resident"] is True and slot.calls[-1] == ("logmel", 1, 20 * (LM_MAXRANGES + 1))


@pytest.mark.parametrize("alignments, probs", [([], []), ([(0, 0)], [0.5]),
                                               ([(0, 0), (0, 1), (1, 2)], list(np.asarray([0.25, 0.1], np.float32)))],
                         ids=["empty", "single_pair", "float32_probabilities"])
def test_unpack_alignment_gives_int64_indices_and_float64_probabilities(alignments, probs):
    ti, fi, p = WT.unpack_alignment(SimpleNamespace(alignments=alignments, text_token_probs=probs))
    assert ti.dtype == fi.dtype == np.int64 and p.dtype == np.float64
    assert ti.shape == fi.shape == (len(alignments),) and p.shape == (len(probs),)
    assert ti.tolist() == [a for a, _ in alignments] and fi.tolist() == [b for _, b in alignments]
    assert p.tolist() == [float(x) for x in probs]                                        # the fp32 values, widened, not rounded again
