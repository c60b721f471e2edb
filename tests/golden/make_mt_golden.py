"""Generate the translation-engine fixtures (run once on a machine with `transformers` and `sentencepiece`; the tests read the
outputs only):

  tests/golden/mt_golden.json   — seeded M2M100 (random_mt_weights at a d_model 384 / 6 heads / 2 + 2 layers / FFN 1536 fixture
                                  config) run through transformers' M2M100ForConditionalGeneration: generate() tokens and
                                  sequences_scores for num_beams 1 and 5, early_stopping True / False / "never", length_penalty != 1,
                                  no_repeat_ngram_size, forced_eos_token_id and a case that runs to max_length.
  tests/golden/mt_golden.npz    — encoder-output rows and teacher-forced logits rows of the same model.
  tests/golden/mt_tok/          — a tiny sentencepiece model trained here, its vocab.json, a tokenizer_config.json with the 100
                                  language codes in fairseq order, and what transformers' M2M100Tokenizer
                                  yields for ~20 sentences with src_lang = the target code (small100's source layout:
                                  [tgt_lang_code] + pieces + [eos]) and for batch_decode(skip_special_tokens=True).

    python tests/golden/make_mt_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from whisperlive_amd.mt_weights import MTSpec, random_mt_weights  # noqa: E402

SPEC = MTSpec(d_model=384, n_heads=6, enc_layers=2, dec_layers=2, ffn=1536, vocab=2112, max_positions=1024,
              decoder_start_id=0)   # (a decoder start other than EOS: see random_mt_weights' note on tied embeddings)
SEED = 11
SENTENCES = [
    "Hello world.", "How are you today?", "The weather is nice and sunny.", "I would like a cup of coffee, please.",
    "Where is the train station?", "This is a small test of the translation engine.", "Numbers like 42 and 1999 matter.",
    "She sells sea shells by the sea shore.", "Please close the door when you leave.", "We are streaming audio in real time.",
    "Good morning, everyone!", "The quick brown fox jumps over the lazy dog.", "Can you hear me now?",
    "Thank you very much for your help.", "It is raining again.", "Let's meet at noon tomorrow.",
    "The meeting has been moved to Friday.", "Music makes people happy.", "Don't forget your umbrella.",
    "Translation should be fast and accurate.",
]
LANGS = ["fr", "de", "es", "zh", "ja", "ru", "en"]


def write_tokenizer_config(out_dir):
    """the code order as a checkpoint's tokenizer_config.json carries it (all 100 `__xx__` tokens, fairseq m2m100 order)"""
    from transformers.models.m2m_100.tokenization_m2m_100 import FAIRSEQ_LANGUAGE_CODES
    with open(os.path.join(out_dir, "tokenizer_config.json"), "w") as f:
        json.dump({"tokenizer_class": "M2M100Tokenizer",
                   "additional_special_tokens": [f"__{c}__" for c in FAIRSEQ_LANGUAGE_CODES["m2m100"]]}, f, indent=0)


def make_tokenizer_fixture(out_dir):
    import sentencepiece as spm
    from transformers.models.m2m_100.tokenization_m2m_100 import M2M100Tokenizer
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        corpus = os.path.join(td, "corpus.txt")
        with open(corpus, "w") as f:
            for _ in range(20):
                for s in SENTENCES:
                    f.write(s + "\n")
        spm.SentencePieceTrainer.train(input=corpus, model_prefix=os.path.join(out_dir, "sentencepiece.bpe"), vocab_size=200,
                                       model_type="bpe", character_coverage=1.0, bos_id=-1, eos_id=-1, unk_id=0, pad_id=-1,
                                       minloglevel=2, normalization_rule_name="identity")
    sp = spm.SentencePieceProcessor(model_file=os.path.join(out_dir, "sentencepiece.bpe.model"))
    vocab = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
    for i in range(sp.get_piece_size()):
        p = sp.id_to_piece(i)
        if p not in vocab:
            vocab[p] = len(vocab)
    with open(os.path.join(out_dir, "vocab.json"), "w") as f:
        json.dump(vocab, f, ensure_ascii=False, indent=0)
    write_tokenizer_config(out_dir)
    tok = M2M100Tokenizer(os.path.join(out_dir, "vocab.json"), os.path.join(out_dir, "sentencepiece.bpe.model"))
    cases = []
    for i, s in enumerate(SENTENCES + ["Ünïcödé wörds ñ", "  spaced   out  ", ""]):
        lang = LANGS[i % len(LANGS)]
        tok.src_lang = lang
        ids = tok(s)["input_ids"]
        cases.append({"text": s, "tgt_lang": lang, "ids": ids})
    rng = np.random.default_rng(3)
    decodes = []
    for _ in range(12):
        ids = [int(x) for x in rng.integers(0, len(tok), size=int(rng.integers(1, 14)))]
        decodes.append({"ids": ids, "text": tok.batch_decode([ids], skip_special_tokens=True)[0]})
    for c in cases[:6]:
        decodes.append({"ids": c["ids"], "text": tok.batch_decode([c["ids"]], skip_special_tokens=True)[0]})
    with open(os.path.join(out_dir, "tok_golden.json"), "w") as f:
        json.dump({"len": len(tok), "encode": cases, "decode": decodes}, f, ensure_ascii=False, indent=0)
    return len(tok)


def main():
    from transformers import GenerationConfig, M2M100Config, M2M100ForConditionalGeneration
    n_tok = make_tokenizer_fixture(os.path.join(HERE, "mt_tok"))
    assert n_tok <= SPEC.vocab, (n_tok, SPEC.vocab)
    w = random_mt_weights(SPEC, seed=SEED, peaked=True)
    model = M2M100ForConditionalGeneration(M2M100Config(**SPEC.hf_config())).eval()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("embed_tokens" in k or "lm_head" in k or "embed_positions" in k for k in missing), missing
    assert torch.equal(model.lm_head.weight, sd["model.shared.weight"])
    rng = np.random.default_rng(5)
    lang_ids = list(range(n_tok - 108, n_tok - 8))      # (the first source token only stands in for a language code)
    srcs = []
    for L in (3, 5, 9, 14, 22, 31, 47, 64):
        pieces = [int(x) for x in rng.integers(4, n_tok - 108, size=L - 2)]
        srcs.append([int(rng.choice(lang_ids))] + pieces + [SPEC.eos_id])
    arrays = {}
    with torch.no_grad():
        enc_rows = []
        for i in (0, 4):
            e = model.model.encoder(input_ids=torch.tensor([srcs[i]])).last_hidden_state[0].numpy()
            arrays[f"enc_{i}"] = e[:8].astype(np.float32)          # the first rows (all of source 0)
        dec = [SPEC.decoder_start_id] + [int(x) for x in rng.integers(4, n_tok, size=5)]
        lg = model(input_ids=torch.tensor([srcs[3]]), decoder_input_ids=torch.tensor([dec])).logits[0].numpy()
        arrays["tf_logits"] = lg[[0, 5]].astype(np.float32)
    cases = [
        dict(name="greedy", num_beams=1, max_length=40, early_stopping=False, length_penalty=1.0),
        dict(name="beam5_es_true", num_beams=5, max_length=40, early_stopping=True, length_penalty=1.0),
        dict(name="beam5_es_false", num_beams=5, max_length=40, early_stopping=False, length_penalty=1.0),
        dict(name="beam5_never_lp", num_beams=5, max_length=40, early_stopping="never", length_penalty=1.3),
        dict(name="beam5_lp06", num_beams=5, max_length=40, early_stopping=True, length_penalty=0.6),
        dict(name="beam5_ngram_forced", num_beams=5, max_length=24, early_stopping=True, length_penalty=1.0,
             no_repeat_ngram_size=3, forced_eos_token_id=SPEC.eos_id),
        dict(name="beam4_maxlen", num_beams=4, max_length=6, early_stopping=True, length_penalty=1.0),
        dict(name="greedy_maxlen", num_beams=1, max_length=6, early_stopping=False, length_penalty=1.0),
    ]
    out_cases = []
    for c in cases:
        gc = GenerationConfig(num_beams=c["num_beams"], max_length=c["max_length"], early_stopping=c["early_stopping"],
                              length_penalty=c["length_penalty"], no_repeat_ngram_size=c.get("no_repeat_ngram_size", 0),
                              forced_eos_token_id=c.get("forced_eos_token_id"), decoder_start_token_id=SPEC.decoder_start_id,
                              eos_token_id=SPEC.eos_id, pad_token_id=SPEC.pad_id, bos_token_id=0, do_sample=False)
        res = []
        for s in srcs:
            with torch.no_grad():
                o = model.generate(input_ids=torch.tensor([s]), generation_config=gc, return_dict_in_generate=True,
                                   output_scores=True)
            seq = o.sequences[0].tolist()
            res.append({"sequence": seq,
                        "score": None if o.get("sequences_scores") is None else float(o.sequences_scores[0])})
        out_cases.append({**c, "results": res})
        print(c["name"], [len(r["sequence"]) for r in res])
    js = {"spec": SPEC.__dict__, "seed": SEED, "peaked": True, "sources": srcs, "tf_decoder": dec, "tf_rows": [0, 5],
          "tf_source": 3, "cases": out_cases}
    with open(os.path.join(HERE, "mt_golden.json"), "w") as f:
        json.dump(js, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "mt_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
