"""GPU (-m gpu): a grammar per file end to end, on the TRAINED checkpoint of tests/test_gpu_grammar.py (a word of its language is one
token). One transcribe_many job over three files with grammars=[A, None, B] and a batch_size that puts all three chunks into ONE decode
group: every file's transcript is what the same file yields decoded alone — under A, under no grammar, under B. And one upload with
grammar fields to the file endpoint, with and without a FileBatcher: the same response, byte for byte."""
import json
import os

import pytest

from tests.golden.make_trained_tiny import utterance
from tests.test_gpu_grammar import DIR, DISTRACTORS
from tests.test_gpu_keyword_bias import WordTokenizer, _tokens, _wav
from tests.test_rest import Served
from whisperlive_amd import grammar as G

pytestmark = pytest.mark.gpu


def test_three_files_three_selections_in_one_decode_group(gpu):
    import tokenizers
    from whisperlive_amd import vad
    from whisperlive_amd.batched import BatchedInferencePipeline
    from whisperlive_amd.synthetic import energy_following_vad_weights
    from whisperlive_amd.transcriber import WhisperModelHIP
    tok = WordTokenizer(tokenizers.Tokenizer.from_file(os.path.join(DIR, "tokenizer.json")))
    gate = vad.SileroHIPModel(energy_following_vad_weights(3), device=0)      # (the pooled route gates every upload: seeded stand-in weights)
    m = WhisperModelHIP(DIR, device="cuda", device_index=0, hf_tokenizer=tok, max_batch=8, vad_model=gate)
    try:
        with open(os.path.join(DIR, "expected.json")) as f:
            exp = json.load(f)
        pcm, _ws = utterance(exp["cases"][0]["seed"])
        truth = [t for t in exp["cases"][0]["truth_tokens"] if t < exp["timestamp_begin"]]
        clip = pcm[:int(16000 * (0.5 + 0.5 * len(truth) + 0.5))]
        pipe = BatchedInferencePipeline(m)
        kw = dict(language="en", beam_size=5, temperature=0.0, vad_filter=False, without_timestamps=False, batch_size=3)
        lists = [DISTRACTORS, None, [f"w{t}" for t in sorted(set(truth))][:2]]

        def single(phrases):
            with (m.grammar(phrases=phrases) if phrases is not None else G.scope(None)):
                return _tokens(m, list(pipe.transcribe(clip, **kw)[0]))       # (the segments arrive lazily: drawn inside the scope)

        want = [single(p) for p in lists]
        assert want[1] == truth[:len(want[1])] and len(want[1]) >= 2 and len({tuple(w) for w in want}) == 3       # three different transcripts
        many = pipe.transcribe_many([clip, clip, clip], grammars=lists, **kw)         # one chunk a file: ONE decode group, three selections
        for (segs, _info), w, phrases in zip(many, want, lists):
            assert not isinstance(segs, Exception), segs
            assert _tokens(m, segs) == w and (phrases is None or G.accepts(m.compile_grammar(phrases), w))
        # the slot goes on: a job without grammars decodes unconstrained again
        assert _tokens(m, pipe.transcribe_many([clip], **kw)[0][0]) == want[1] and G.current_items() is None
        # the file endpoint: an upload with grammar fields answers the same bytes pooled (a FileBatcher runs) and in the request's thread
        fields = [("file", ("u.wav", _wav(clip))), ("response_format", "verbose_json")] + [("grammar", w) for w in lists[2]]
        answers = []
        for window_ms in (0, 20):                                       # (both through the batched pipeline; 0: no batcher)
            with Served(m, model_factory=lambda model, device_index, **k: m, file_batch_size=3, file_batch_window_ms=window_ms) as s:
                answers.append(s.post(fields))
                assert (s.server.batcher.jobs if window_ms else s.server.batcher) == (1 if window_ms else None)
        assert answers[0][0] == 200 and answers[0][2] == answers[1][2]
        assert json.loads(answers[1][2])["segments"]                    # (the gate's chunks were decoded, under the upload's grammar)
    finally:
        m.close()
        m.engine.close()
        gate.close()
