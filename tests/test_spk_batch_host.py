"""Host-side tests of batched speaker labelling (no GPU): the grouping of segments into wlx_spk_embed_batch calls
(diarization.plan_embed_groups), SpeakerDiarizer.identify_speakers against identify_speaker called once per segment, and
rest.speaker_labels_for_segments through its batch path and its one-by-one fallback."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

from whisperlive_amd.diarization import SpeakerDiarizer, plan_embed_groups
from whisperlive_amd.rest import speaker_labels_for_segments


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("seed", range(6))
def test_planner_keeps_order_and_caps(seed):
    rng = np.random.default_rng(seed)
    cap, max_items = 720000, (3, 64, 5, 64, 1, 64)[seed]
    lengths = [int(v) for v in rng.integers(0, 200000, 150)]
    for at in rng.integers(0, 150, 4):
        lengths[at] = cap + int(rng.integers(1, 50000))          # oversize items
    lengths[7] = cap                                               # one item that fills a group exactly
    groups = plan_embed_groups(lengths, cap, max_items)
    assert [i for g in groups for i in g] == list(range(len(lengths)))         # every index once, in order
    for g in groups:
        assert 1 <= len(g) <= max_items
        total = sum(lengths[i] for i in g)
        if any(lengths[i] > cap for i in g):
            assert len(g) == 1                                     # an oversize item is alone
        else:
            assert total <= cap
    # greedy: a group is closed only when the next item would not fit
    for g, nxt in zip(groups, groups[1:]):
        assert len(g) == max_items or sum(lengths[i] for i in g) + lengths[nxt[0]] > cap


def test_planner_small_cases():
    assert plan_embed_groups([], 100) == []
    assert plan_embed_groups([5], 100) == [[0]]
    assert plan_embed_groups([50, 50, 1], 100) == [[0, 1], [2]]
    assert plan_embed_groups([101, 1, 101], 100) == [[0], [1], [2]]
    assert plan_embed_groups([0, 0, 0], 100, max_items=2) == [[0, 1], [2]]
    assert plan_embed_groups([10] * 130, 10 ** 9) == [list(range(64)), list(range(64, 128)), [128, 129]]      # the engine's 64
    with pytest.raises(ValueError):
        plan_embed_groups([1], 0)


# ------------------------------------------------------------------------------------------------ identify_speakers
DIM = 24


def _cases(seed, n=40, voices=4):
    """n 'segments' of a few voices: audio whose first sample is the segment's number (what the fake embedders look up), every
    seventh one under 0.3 s; unit embeddings = the voice's direction plus noise"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((voices, DIM))
    embs, audios = [], []
    for i in range(n):
        e = base[rng.integers(voices)] + 0.35 * rng.standard_normal(DIM)
        embs.append((e / np.linalg.norm(e)).astype(np.float32))
        a = np.zeros(4799 if i % 7 == 3 else 4800 + int(rng.integers(0, 3000)), dtype=np.float32)
        a[0] = i
        audios.append(a)
    return audios, embs


class _Plain:
    """a plain callable embedder: (pcm, sample_rate) -> embedding; segment 5 gives None (an engine that finds it too short)"""

    def __init__(self, embs):
        self.embs, self.calls = embs, []

    def __call__(self, pcm, sample_rate):
        assert len(pcm) >= 4800                      # the diarizer never asks for less than 0.3 s
        self.calls.append(int(pcm[0]))
        return None if int(pcm[0]) == 5 else self.embs[int(pcm[0])]


class _Many(_Plain):
    def __init__(self, embs):
        super().__init__(embs)
        self.many_calls = 0

    def embed_many(self, pcms, sample_rate=16000):
        self.many_calls += 1
        return [self(p, sample_rate) for p in pcms]


@pytest.mark.parametrize("seed,threshold,max_speakers,names", [(0, 0.55, 10, None), (1, 0.4, 3, ["ann", "bob"]), (2, 0.8, 10, None)])
@pytest.mark.parametrize("kind", [_Plain, _Many])
def test_identify_speakers_equals_the_sequential_loop(kind, seed, threshold, max_speakers, names):
    audios, embs = _cases(seed)
    one = SpeakerDiarizer(similarity_threshold=threshold, max_speakers=max_speakers, speaker_names=names, embedder=_Plain(embs))
    want = [one.identify_speaker(a) for a in audios]
    assert want[3] is None and want[5] is None and len({w for w in want if w}) >= 2
    fake = kind(embs)
    many = SpeakerDiarizer(similarity_threshold=threshold, max_speakers=max_speakers, speaker_names=names, embedder=fake)
    assert many.identify_speakers(audios) == want
    assert fake.calls == [i for i in range(len(audios)) if i % 7 != 3]            # every long-enough segment once, in order
    if kind is _Many:
        assert fake.many_calls == 1
    assert list(many.speakers) == list(one.speakers)
    for k in one.speakers:
        assert (many.speakers[k] == one.speakers[k]).all()                       # the centroids went through the same updates
    # the state carries on: a further single call agrees too
    assert many.identify_speaker(audios[0]) == one.identify_speaker(audios[0])
    assert many.identify_speakers([]) == []


# ------------------------------------------------------------------------------------------------ the REST helper
class _OnlyOneByOne:
    """what the fakes of the other tests look like: identify_speaker and nothing else"""

    def __init__(self, diarizer):
        self._d = diarizer

    def identify_speaker(self, audio, sample_rate=16000):
        return self._d.identify_speaker(audio, sample_rate)


def test_speaker_labels_for_segments_batch_and_fallback_agree():
    rng = np.random.default_rng(3)
    audio = np.arange(20 * 16000, dtype=np.float32)              # a sample's value is its position: the embedder's key
    spans = [(0.0, 2.0), (2.0, 2.0), (2.5, 2.2), (2.0, 2.2), (2.2, 5.0), (5.0, 9.5), (25.0, 26.0), (9.5, 11.0), (11.0, 11.29),
             (11.3, 14.0), (19.0, 30.0), (-1.0, 0.5)]
    segments = [SimpleNamespace(start=a, end=b) for a, b in spans]
    base = rng.standard_normal((3, DIM))
    table = {}
    for k, (a, b) in enumerate(spans):
        e = base[k % 3] + 0.2 * rng.standard_normal(DIM)
        table[max(0, int(a * 16000))] = (e / np.linalg.norm(e)).astype(np.float32)

    class Embedder:
        many_calls = 0

        def __call__(self, pcm, sample_rate):
            return table[int(pcm[0])]

        def embed_many(self, pcms, sample_rate=16000):
            Embedder.many_calls += 1
            return [self(p, sample_rate) for p in pcms]

    batch = speaker_labels_for_segments(segments, audio, SpeakerDiarizer(embedder=Embedder()))
    assert Embedder.many_calls == 1
    loop = speaker_labels_for_segments(segments, audio, _OnlyOneByOne(SpeakerDiarizer(embedder=Embedder())))
    assert Embedder.many_calls == 1
    assert batch == loop
    # empty and inverted ranges (1, 2), the one past the audio (6) are skipped; 0.2 s and 0.29 s (3, 8) get no label
    assert sorted(batch) == [0, 4, 5, 7, 9, 10, 11]
    assert len(set(batch.values())) >= 2
    assert speaker_labels_for_segments(segments, None, SpeakerDiarizer(embedder=Embedder())) == {}
    assert speaker_labels_for_segments([], audio, SpeakerDiarizer(embedder=Embedder())) == {}
