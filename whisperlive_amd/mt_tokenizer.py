"""M2M100 / small100 tokenizer on ``sentencepiece`` plus the checkpoint's ``vocab.json`` (no ``transformers`` at run time).

Ids: the sentencepiece pieces are mapped through ``vocab.json`` (unknown pieces -> ``<unk>``); language-code tokens ``__xx__`` take
the ids ``len(vocab) + index`` in the fairseq m2m100 code order, followed by 8 made-up words — the layout of transformers'
``M2M100Tokenizer``. small100 puts the TARGET language on the source side: ``[__tgt__] + pieces + [</s>]``.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

NUM_MADEUP_WORDS = 8


N_LANGUAGE_CODES = 100          # the m2m100 code set (small100 uses the same 100 codes)


def fairseq_language_codes(model_dir: Optional[str] = None) -> List[str]:
    """The language-code order that fixes the code ids. Taken from the checkpoint's tokenizer files only when they carry the WHOLE
    set: a ``language_codes`` list or the ``__xx__`` entries of ``additional_special_tokens`` (tokenizer_config.json /
    special_tokens_map.json) with exactly 100 distinct codes. A partial list would shift every id after a gap, so it is ignored and
    the fairseq m2m100 order of transformers' M2M100Tokenizer is used instead."""
    if model_dir:
        for fn in ("tokenizer_config.json", "special_tokens_map.json"):
            p = os.path.join(model_dir, fn)
            if not os.path.isfile(p):
                continue
            cfg = json.load(open(p, encoding="utf-8"))
            codes = cfg.get("language_codes")
            if not isinstance(codes, list):
                toks = cfg.get("additional_special_tokens") or []
                toks = [t.get("content") if isinstance(t, dict) else t for t in toks]
                codes = [t[2:-2] for t in toks if isinstance(t, str) and t.startswith("__") and t.endswith("__") and len(t) > 4]
            codes = [str(c) for c in codes]
            if len(codes) == N_LANGUAGE_CODES and len(set(codes)) == N_LANGUAGE_CODES:
                return codes
    from transformers.models.m2m_100.tokenization_m2m_100 import FAIRSEQ_LANGUAGE_CODES
    return list(FAIRSEQ_LANGUAGE_CODES["m2m100"])


class M2M100SPTokenizer:
    def __init__(self, model_dir: str, spm_file: Optional[str] = None, language_codes: Optional[Sequence[str]] = None):
        import sentencepiece as spm
        if spm_file is None:
            for cand in ("sentencepiece.bpe.model", "spm.model", "sentencepiece.model"):
                if os.path.isfile(os.path.join(model_dir, cand)):
                    spm_file = os.path.join(model_dir, cand)
                    break
        if spm_file is None:
            raise FileNotFoundError(f"{model_dir}: no sentencepiece model")
        self.sp = spm.SentencePieceProcessor(model_file=spm_file)
        self.encoder = json.load(open(os.path.join(model_dir, "vocab.json"), encoding="utf-8"))
        self.decoder = {v: k for k, v in self.encoder.items()}
        codes = list(language_codes) if language_codes is not None else fairseq_language_codes(model_dir)
        n = len(self.encoder)
        self.lang_code_to_id = {c: n + i for i, c in enumerate(codes)}
        self.id_to_lang = {v: k for k, v in self.lang_code_to_id.items()}
        self.unk_id = self.encoder.get("<unk>", 3)
        self.pad_id = self.encoder.get("<pad>", 1)
        self.eos_id = self.encoder.get("</s>", 2)
        self.bos_id = self.encoder.get("<s>", 0)
        self.special_ids = {self.unk_id, self.pad_id, self.eos_id, self.bos_id} | set(self.id_to_lang)
        self.size = n + len(codes) + NUM_MADEUP_WORDS

    def __len__(self):
        return self.size

    def lang_id(self, code: str) -> int:
        if code not in self.lang_code_to_id:
            raise KeyError(f"unknown language code {code!r}")
        return self.lang_code_to_id[code]

    def encode_source(self, text: str, tgt_lang: str) -> List[int]:
        pieces = self.sp.encode(text, out_type=str)
        return [self.lang_id(tgt_lang)] + [self.encoder.get(p, self.unk_id) for p in pieces] + [self.eos_id]

    def decode(self, ids: Sequence[int]) -> str:
        """batch_decode(..., skip_special_tokens=True) of one sequence: <s> / <pad> / </s> / <unk> are dropped; language-code tokens
        are not among transformers' skipped tokens and come out as `__xx__`, separated from the text around them by a space"""
        skip = {self.unk_id, self.pad_id, self.eos_id, self.bos_id}
        parts, run = [], []

        def flush():
            if run:
                t = self.sp.decode(run)
                if t:
                    parts.append(t)
                run.clear()
        n_enc, n_lang = len(self.encoder), len(self.lang_code_to_id)
        for i in ids:
            i = int(i)
            if i in skip:
                continue
            if i in self.id_to_lang:
                flush()
                parts.append(f"__{self.id_to_lang[i]}__")
            elif i in self.decoder:
                run.append(self.decoder[i])
            elif i >= n_enc + n_lang:
                flush()
                parts.append(f"madeupword{i - n_enc - n_lang}")
        flush()
        return " ".join(parts).strip()
