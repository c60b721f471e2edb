"""GPU (-m gpu): a regular expression per item end to end, on the seeded MICRO model and the synthetic tokenizer of
tests/test_gpu_pattern.py. A batch of three prompts under set_patterns + select_patterns([A, -1, B]) yields, item by item, the tokens and
the scores of the same batch decoded in the single-pattern mode under A, under no pattern and under B: the network pass is the same
launch list on the same rows, and neither kernel does arithmetic, so the scores agree bit for bit. Then the selection permuted and the
set grown, in the same process: captured step graphs replay across selections and sets. And one transcribe_many job with
grammar_patterns=[A, None, B, "("]: each good file is what the same file yields alone, the malformed expression costs only its file."""
import struct

import pytest

from tests.test_gpu_pattern import NO_TS, clips, model  # noqa: F401  (the module's fixtures)
from whisperlive_amd import pattern as P

pytestmark = pytest.mark.gpu
A, B, GROWN = r"( w[34][0-9]*)+", r"( w5[0-9]*)+", r"( w6[0-9]*)+"      # (every reachable state accepts, as REGEX there)


def test_a_batch_under_three_selections_equals_three_single_pattern_decodes(model, clips):
    from whisperlive_amd.transcriber import get_suppressed_tokens
    ids, tk = model.token_ids, model._base_tokenizer
    vocab = (ids.eot, *P.token_bytes(tk, ids.eot))
    pats = {x: P.compile_pattern(x) for x in (A, B, GROWN)}
    slot = model._slot(rows=5)
    slot.encode(1, seek=[0], seg=[slot.logmel(clips[0]) - 1])
    kw = dict(beam_size=5, max_length=2 + 12, suppress_tokens=get_suppressed_tokens(tk, NO_TS["suppress_tokens"]), enc_items=[0, 0, 0])
    gen = lambda: [(r.sequences_ids[0], struct.pack("f", r.scores[0])) for r in slot.generate([[ids.sot, ids.no_timestamps]] * 3, ids, **kw)]
    single = {}
    for x in (A, None, B, GROWN):
        P.install(slot, pats.get(x), vocab)
        single[x] = gen()
    assert len({tuple(single[x][0][0]) for x in single}) == 4           # four different transcripts: a wrong selection shows
    pset = P.PatternSet()
    for asked in ([A, None, B], [B, A, None], [None, B, A], [GROWN, B, A]):       # permuted twice on the set as it is, then the set grown
        before = pset.version
        slot.select_patterns(P.install_items(slot, [pats.get(x) for x in asked], pset, vocab))
        assert (pset.version != before) == (asked[0] in (A, GROWN)) and slot._pattern is pset
        assert gen() == [single[x][i] for i, x in enumerate(asked)], asked
    P.install(slot, None)
    assert gen() == single[None]


def test_four_files_four_patterns_in_one_job(model, clips):
    from whisperlive_amd.batched import BatchedInferencePipeline
    pipe = BatchedInferencePipeline(model)
    kw = dict(batch_size=2, language="en", beam_size=5, temperature=0.0, vad_filter=False, **NO_TS)
    asked = [A, None, B, "("]
    many = pipe.transcribe_many(clips + clips[:1], **kw, grammar_patterns=asked)
    assert isinstance(many[3][0], ValueError) and P.current_items() is None
    for clip, x, (segs, _info) in zip(clips, asked, many):
        assert not isinstance(segs, Exception), segs
        one, _i = pipe.transcribe(clip, **kw, **({"grammar_pattern": x} if x else {}))
        assert segs and [s.tokens for s in segs] == [s.tokens for s in one], x
