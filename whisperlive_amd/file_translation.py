"""Translated transcripts for the file routes: the segments of one file go to the translation engine as ONE job
(HipTranslator.translate_many -> wlx_mt_translate_many: grouped by length, beam search on the device), after the transcription.

* ``translate_segments(segments, translator, target_language)`` — the segments with a ``translation`` attribute added; times,
  words, ``speaker`` and ``channel`` are untouched (the word times of a translated transcript stay those of the source).
* ``check_target_language(translator, code)``                   — ValueError for a code the translator's tokenizer does not know.
* ``per_file_languages`` / ``translated_job``                   — the option for BatchedInferencePipeline.transcribe_many / iter_many,
  one target language for all files or one entry per file (``None``: that file stays untranslated).

`translator`: an object with ``translate_many(texts, lang)`` (HipTranslator), with ``translate(texts, lang)``, or a callable
``(texts, lang) -> texts``. Empty and whitespace-only texts are not sent: their translation is the text itself.
"""
from __future__ import annotations

import copy
from typing import Callable, List, Optional, Sequence


def _call_of(translator) -> Callable:
    if translator is None:
        raise ValueError("target_language needs a translator (a HipTranslator, or a callable (texts, language) -> texts)")
    for name in ("translate_many", "translate"):
        fn = getattr(translator, name, None)
        if fn is not None:
            return fn
    if callable(translator):
        return translator
    raise TypeError("translator: an object with translate_many / translate, or a callable (texts, language) -> texts")


def check_target_language(translator, target_language: str) -> None:
    """ValueError when the translator can tell that it does not know the language code (its tokenizer's code table)"""
    if not isinstance(target_language, str) or not target_language.strip():
        raise ValueError("target_language must be a language code such as 'de'")
    tokenizer = getattr(translator, "tokenizer", None)
    lang_id = getattr(tokenizer, "lang_id", None)
    if lang_id is not None:
        try:
            lang_id(target_language)
        except KeyError:
            raise ValueError(f"target_language {target_language!r} is not a language the translation model knows") from None


def translate_texts(texts: Sequence[str], translator, target_language: str) -> List[str]:
    """one translator call for the non-empty texts (stripped, as the responses render them); the others come back as they are"""
    out = list(texts)
    todo = [i for i, t in enumerate(texts) if t and t.strip()]
    if todo:
        got = _call_of(translator)([texts[i].strip() for i in todo], target_language)
        if len(got) != len(todo):
            raise RuntimeError(f"the translator returned {len(got)} texts for {len(todo)}")
        for i, t in zip(todo, got):
            out[i] = t
    return out


def translate_segments(segments, translator, target_language: Optional[str]) -> list:
    """-> the segments (shallow copies, in order) with `.translation`; target_language None: the segments as a list, unchanged.
    One translator call per file."""
    segments = list(segments or [])
    if target_language is None:
        return segments
    texts = translate_texts([getattr(s, "text", "") or "" for s in segments], translator, target_language)
    out = []
    for seg, text in zip(segments, texts):
        seg = copy.copy(seg)
        seg.translation = text
        out.append(seg)
    return out


def per_file_languages(target_language, n_files: int) -> List[Optional[str]]:
    """`target_language` of a many-files job: one code for every file, or a list with one entry (a code or None) per file"""
    if isinstance(target_language, (list, tuple)):
        if len(target_language) != n_files:
            raise ValueError(f"target_language: a list of {len(target_language)} entries for {n_files} files "
                             "(one entry per file, or one value for all)")
        return list(target_language)
    return [target_language] * n_files


def translated_job(job, languages: Sequence[Optional[str]], translator):
    """iter_many's (index, segments, info) stream with the files' segments translated, each file in one call; a file that failed
    (segments is an exception) and a file without a target language pass through"""
    for index, segments, info in job:
        lang = languages[index]
        if lang is not None and not isinstance(segments, BaseException):
            segments = translate_segments(segments, translator, lang)
        yield index, segments, info
