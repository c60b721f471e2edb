"""Translation of completed transcript segments on the HIP M2M100 engine — the `enable_translation` side channel of the
WhisperLive protocol (reference: whisper_live/backend/translation_backend.py, wired in whisper_live/server.py:203-229).

* ``HipMTEngine``             — ctypes binding of the wlx_mt_* entry points (engine + one slot).
* ``HipTranslator``           — tokenizer + engine + generation options of one checkpoint directory; ``translate(texts, tgt_lang)``
                                batches texts of different lengths into ONE engine call. ``shared_translator`` keeps one per
                                (directory, device), loaded on the first translating client.
* ``ServeClientTranslation``  — the reference's per-client queue loop and ``translated_segments`` message.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import queue
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .mt_weights import MTGenOptions, MTSpec, generation_options, load_mt_dir


class HipMTEngine:
    """one wlx_mt engine and one slot of max_batch items x num_beams rows x max_src source tokens"""

    def __init__(self, spec: MTSpec, weights: Dict[str, "np.ndarray"], device: int = 0, max_batch: int = 8, max_rows: int = 5,
                 max_src: int = 256):
        self.lib = _lib.load()
        self.spec = spec
        self.max_batch, self.max_rows, self.max_src = max_batch, max_rows, max_src
        cs = _lib.wlx_mt_spec(spec.d_model, spec.n_heads, spec.enc_layers, spec.dec_layers, spec.ffn, spec.vocab, spec.max_positions,
                              spec.pad_id, spec.eos_id, spec.decoder_start_id, int(spec.scale_embedding))
        arr, keep = _lib.tensor_array(weights)      # (keep: alive until the create call returns)
        h = C.c_void_p()
        _lib.check(self.lib.wlx_mt_create(C.byref(cs), arr, len(weights), device, C.byref(h)))
        self.h = h
        slot = C.c_int32()
        rc = self.lib.wlx_mt_slot_create(h, max_batch, max_rows, max_src, C.byref(slot))
        if rc != 0:
            msg = self.lib.wlx_last_error()
            self.lib.wlx_mt_destroy(h)
            self.h = None
            raise _lib.WlxError(f"libwlx error {rc}: {msg.decode() if msg else '?'}")
        self.slot = slot.value

    @staticmethod
    def _opts(o: MTGenOptions) -> "_lib.wlx_mt_gen_opts":
        return _lib.wlx_mt_gen_opts(o.num_beams, o.max_length, o.early_stopping_code(), float(o.length_penalty),
                                    o.no_repeat_ngram_size, -1 if o.forced_eos_token_id is None else int(o.forced_eos_token_id))

    @staticmethod
    def _pack(srcs: Sequence[Sequence[int]]):
        stride = max(len(s) for s in srcs)
        ids = np.zeros((len(srcs), stride), dtype=np.int32)
        for i, s in enumerate(srcs):
            ids[i, :len(s)] = s
        return ids, np.array([len(s) for s in srcs], dtype=np.int32), stride

    def translate_ids(self, srcs: Sequence[Sequence[int]], opts: MTGenOptions) -> Tuple[List[List[int]], List[float]]:
        ids, lens, stride = self._pack(srcs)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        cap = opts.max_length
        toks = np.zeros((len(srcs), cap), dtype=np.int32)
        n = np.zeros(len(srcs), dtype=np.int32)
        sc = np.zeros(len(srcs), dtype=np.float32)
        o = self._opts(opts)
        _lib.check(self.lib.wlx_mt_translate(self.h, self.slot, len(srcs), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), stride,
                                             C.byref(o), toks.ctypes.data_as(i32p), cap, n.ctypes.data_as(i32p), sc.ctypes.data_as(f32p)))
        return [toks[i, :n[i]].tolist() for i in range(len(srcs))], sc.tolist()

    def translate_ids_many(self, srcs: Sequence[Sequence[int]], opts: MTGenOptions) -> Tuple[List[List[int]], List[float]]:
        """Any number of sources (up to _lib.MT_MANY_MAX, more than max_batch included) as ONE wlx_mt_translate_many job: grouped by
        length inside the library, searched on the device, results in input order."""
        ids, lens, stride = self._pack(srcs)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        cap = opts.max_length
        toks = np.zeros((len(srcs), cap), dtype=np.int32)
        n = np.zeros(len(srcs), dtype=np.int32)
        sc = np.zeros(len(srcs), dtype=np.float32)
        o = self._opts(opts)
        _lib.check(self.lib.wlx_mt_translate_many(self.h, self.slot, len(srcs), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), stride,
                                                  C.byref(o), toks.ctypes.data_as(i32p), cap, n.ctypes.data_as(i32p), sc.ctypes.data_as(f32p)))
        return [toks[i, :n[i]].tolist() for i in range(len(srcs))], sc.tolist()

    def encoder_output(self, srcs: Sequence[Sequence[int]]) -> np.ndarray:
        ids, lens, stride = self._pack(srcs)
        out = np.zeros((int(lens.sum()), self.spec.d_model), dtype=np.float32)
        i32p = C.POINTER(C.c_int32)
        _lib.check(self.lib.wlx_mt_debug_encode(self.h, self.slot, len(srcs), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                                stride, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def decoder_logits(self, src: Sequence[int], dec: Sequence[int]) -> np.ndarray:
        s = np.asarray(src, dtype=np.int32)
        d = np.asarray(dec, dtype=np.int32)
        out = np.zeros((len(d), self.spec.vocab), dtype=np.float32)
        i32p = C.POINTER(C.c_int32)
        _lib.check(self.lib.wlx_mt_debug_decode_logits(self.h, self.slot, s.ctypes.data_as(i32p), len(s), d.ctypes.data_as(i32p), len(d),
                                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def timings(self) -> Tuple[float, float, int]:
        a, b, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self.lib.wlx_mt_debug_timings(self.h, self.slot, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.wlx_mt_slot_destroy(self.h, self.slot)
            self.lib.wlx_mt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class HipTranslator:
    """A checkpoint directory (config.json, generation_config.json, weights, vocab.json, sentencepiece model) on one device.
    Calls are serialised (one slot); texts longer than the slot's source capacity are cut to it."""

    def __init__(self, model_dir: str, device: int = 0, max_batch: int = 8, max_src: int = 256, engine: Optional[HipMTEngine] = None,
                 tokenizer=None, options: Optional[MTGenOptions] = None):
        from .mt_tokenizer import M2M100SPTokenizer
        self.model_dir = model_dir
        self.options = options or generation_options(model_dir)
        if engine is None:
            spec, w = load_mt_dir(model_dir)
            engine = HipMTEngine(spec, w, device=device, max_batch=max_batch, max_rows=max(1, self.options.num_beams), max_src=max_src)
        self.engine = engine
        self.tokenizer = tokenizer or M2M100SPTokenizer(model_dir)
        self._mu = threading.Lock()

    def translate(self, texts: Sequence[str], tgt_lang: str) -> List[str]:
        out: List[str] = [""] * len(texts)
        todo = [(i, t) for i, t in enumerate(texts) if t and t.strip()]
        for i, t in enumerate(texts):
            if not (t and t.strip()):
                out[i] = t
        eng = self.engine
        with self._mu:
            for k in range(0, len(todo), eng.max_batch):
                chunk = todo[k:k + eng.max_batch]
                srcs = []
                for _, t in chunk:
                    ids = self.tokenizer.encode_source(t, tgt_lang)
                    if len(ids) > eng.max_src:
                        ids = ids[:eng.max_src - 1] + [ids[-1]]
                    srcs.append(ids)
                toks, _ = eng.translate_ids(srcs, self.options)
                for (i, _), tk in zip(chunk, toks):
                    out[i] = self.tokenizer.decode(tk)
        return out

    def _source_ids(self, text: str, tgt_lang: str) -> List[int]:
        ids = self.tokenizer.encode_source(text, tgt_lang)
        if len(ids) > self.engine.max_src:
            ids = ids[:self.engine.max_src - 1] + [ids[-1]]
        return ids

    def translate_many(self, texts: Sequence[str], tgt_lang: str) -> List[str]:
        """`translate` for a whole transcript: every non-empty text goes to the engine in ONE translate_ids_many call (jobs of more
        than _lib.MT_MANY_MAX texts: one call per MT_MANY_MAX). Empty and whitespace-only texts come back unchanged and are not sent."""
        out: List[str] = list(texts)
        todo = [(i, t) for i, t in enumerate(texts) if t and t.strip()]
        with self._mu:
            for k in range(0, len(todo), _lib.MT_MANY_MAX):
                chunk = todo[k:k + _lib.MT_MANY_MAX]
                toks, _ = self.engine.translate_ids_many([self._source_ids(t, tgt_lang) for _, t in chunk], self.options)
                for (i, _), tk in zip(chunk, toks):
                    out[i] = self.tokenizer.decode(tk)
        return out

    def close(self):
        self.engine.close()


def mt_debug_search(logits: np.ndarray, batch: int, opts: MTGenOptions, pad_id: int, eos_id: int, start_id: int, ban_ld: int = 448,
                    step_block: int = 0, use_device: bool = True, device: int = 0):
    """wlx_mt_debug_search: the translation engine's search alone on injected logits [steps][batch * num_beams][vocab] — the host
    bookkeeping of wlx_mt_translate (use_device=False) or the device search of wlx_mt_translate_many.
    -> (token lists, scores float32 array, decode steps run)"""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    steps, rows, vocab = lg.shape
    if rows != batch * opts.num_beams:
        raise ValueError(f"logits rows {rows} != batch {batch} x num_beams {opts.num_beams}")
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cap = opts.max_length
    toks = np.zeros((batch, cap), dtype=np.int32)
    n = np.zeros(batch, dtype=np.int32)
    sc = np.zeros(batch, dtype=np.float32)
    ran = C.c_int32(-1)
    o = HipMTEngine._opts(opts)
    _lib.check(lib.wlx_mt_debug_search(device, lg.ctypes.data_as(f32p), steps, batch, C.byref(o), vocab, pad_id, eos_id, start_id, ban_ld,
                                       step_block, 1 if use_device else 0, toks.ctypes.data_as(i32p), cap, n.ctypes.data_as(i32p),
                                       sc.ctypes.data_as(f32p), C.byref(ran)))
    return [toks[i, :n[i]].tolist() for i in range(batch)], sc, ran.value


_shared: Dict[Tuple[str, int], HipTranslator] = {}
_shared_mu = threading.Lock()


def shared_translator(model_dir: str, device: int = 0) -> HipTranslator:
    """one translator per (model directory, device), created by the first client that asks for translation"""
    with _shared_mu:
        key = (model_dir, device)
        if key not in _shared:
            _shared[key] = HipTranslator(model_dir, device)
        return _shared[key]


class ServeClientTranslation:
    """Per-client translation loop (translation_backend.py:19-239 of the reference): reads the segments the transcription client
    puts on `translation_queue`, translates the completed ones and sends the last `send_last_n_segments` translated segments as
    {"uid", "translated_segments": [{start, end, text, completed, target_language}]}. `translator` is a callable
    (texts, tgt_lang) -> texts or an object with .translate; None = look it up lazily (shared per device)."""

    def __init__(self, client_uid, websocket, translation_queue, target_language="fr", send_last_n_segments=10,
                 model_name="alirezamsh/small100", translator=None, device: int = 0):
        self.client_uid = client_uid
        self.websocket = websocket
        self.translation_queue = translation_queue
        self.target_language = target_language
        self.send_last_n_segments = send_last_n_segments
        self.model_name = model_name
        self.device = device
        self.translated_segments: List[dict] = []
        self.translator = translator
        self.exit = False
        self.model_loaded = translator is not None

    def load_translation_model(self):
        if self.translator is None:
            try:
                self.translator = shared_translator(self.model_name, self.device)
                self.model_loaded = True
            except Exception as e:  # noqa: BLE001 — the reference logs and sends untranslated text
                logging.error(f"Failed to load translation model: {e}")
                self.model_loaded = False
        return self.model_loaded

    def translate_text(self, text: str) -> str:
        if not text.strip():
            return text
        if not self.model_loaded and not self.load_translation_model():
            return text
        try:
            fn = self.translator.translate if hasattr(self.translator, "translate") else self.translator
            out = fn([text], self.target_language)
            return out[0] if out else text
        except Exception as e:  # noqa: BLE001
            logging.error(f"Translation failed for text '{text}': {e}")
            return text

    def process_translation_queue(self):
        logging.info(f"Starting translation processing for client {self.client_uid}")
        while not self.exit:
            try:
                segment = self.translation_queue.get(timeout=1.0)
            except queue.Empty:
                continue
            try:
                if segment is None:
                    break
                if not segment.get("completed", False):
                    continue
                translated = {"start": segment["start"], "end": segment["end"], "text": self.translate_text(segment.get("text", "")),
                              "completed": segment.get("completed", False), "target_language": self.target_language}
                self.translated_segments.append(translated)
                self.send_translation_to_client(self.prepare_translated_segments())
            except Exception as e:  # noqa: BLE001
                logging.error(f"Error processing translation queue: {e}")
            finally:
                try:
                    self.translation_queue.task_done()
                except ValueError:
                    pass
        logging.info(f"Translation processing ended for client {self.client_uid}")

    def prepare_translated_segments(self):
        if len(self.translated_segments) >= self.send_last_n_segments:
            return self.translated_segments[-self.send_last_n_segments:]
        return self.translated_segments[:]

    def send_translation_to_client(self, translated_segments):
        try:
            self.websocket.send(json.dumps({"uid": self.client_uid, "translated_segments": translated_segments}))
        except Exception as e:  # noqa: BLE001
            logging.error(f"[ERROR]: Sending translation data to client: {e}")

    def speech_to_text(self):
        self.process_translation_queue()

    def set_target_language(self, language: str):
        self.target_language = language

    def cleanup(self):
        self.exit = True
        try:
            self.translation_queue.put_nowait(None)
        except queue.Full:
            pass
