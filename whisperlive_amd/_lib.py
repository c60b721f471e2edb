"""ctypes binding of libwlx.so (include/wlx.h). There is NO CPU fallback: if the HIP library is missing or
fails to load, importing the engine raises and tells the user how to build it."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
# WLX_LIB selects another build of the same sources (scripts/trace_step.py: libwlx_trace.so, compiled with -DWLX_TRACE)
DEFAULT_LIB = PKG_DIR / "libwlx.so"
LIB_PATH = Path(os.environ["WLX_LIB"]).resolve() if os.environ.get("WLX_LIB") else DEFAULT_LIB
SOURCES = ["pack.hip", "logmel.hip", "gemm.hip", "attention.hip", "decoder.hip", "align.hip", "dec_gemv.hip", "dec_vocab.hip", "search.hip", "dec_bias.hip", "dec_grammar.hip", "host.hip", "engine.hip", "ring.hip", "engine_decode.hip", "engine_debug.hip", "resample.hip", "flac.hip", "adpcm.hip", "put_many.hip", "vad.hip", "mt.hip", "mt_search.hip", "mt_engine.hip", "spk.hip", "spk_cluster.hip", "spk_engine.hip",
           "kernel_hooks.hip"]
EXPORTS = [
    "wlx_abi_version", "wlx_last_error", "wlx_engine_create", "wlx_engine_destroy", "wlx_engine_spec",
    "wlx_slot_create", "wlx_slot_destroy", "wlx_logmel", "wlx_pcm_put", "wlx_pcm_put_frames", "wlx_pcm_put_frames_split", "wlx_flac_probe", "wlx_pcm_put_flac", "wlx_pcm_put_flac_split", "wlx_wav_probe", "wlx_pcm_put_wav", "wlx_pcm_put_wav_split", "wlx_pcm_put_many", "wlx_pcm_get", "wlx_logmel_resident", "wlx_features_get", "wlx_features_set", "wlx_encode",
    "wlx_encoder_output_get", "wlx_generate", "wlx_generate_ex", "wlx_detect_language", "wlx_bias_set", "wlx_bias_clear", "wlx_align", "wlx_align_batch", "wlx_timings_get", "wlx_sync",
    "wlx_vad_create", "wlx_vad_destroy", "wlx_vad_probs",
    "wlx_ring_create", "wlx_ring_destroy", "wlx_ring_append", "wlx_ring_state", "wlx_ring_set_format", "wlx_ring_append_frames", "wlx_resample_stream_count",
    "wlx_ring_group_create", "wlx_ring_group_destroy", "wlx_ring_group_lane", "wlx_ring_group_append_frames", "wlx_vad_probs_resident", "wlx_vad_segments", "wlx_logmel_ring",
    "wlx_logmel_chunks", "wlx_logmel_chunks_multi", "wlx_vad_probs_pcm", "wlx_vad_probs_batch", "wlx_vad_probs_pcm_batch",
    "wlx_mt_create", "wlx_mt_destroy", "wlx_mt_slot_create", "wlx_mt_slot_destroy", "wlx_mt_translate", "wlx_mt_translate_many",
    "wlx_spk_create", "wlx_spk_destroy", "wlx_spk_embed", "wlx_spk_embed_batch", "wlx_spk_embed_pcm_batch", "wlx_spk_embed_ring_batch",
    "wlx_spk_cluster", "wlx_spk_diarize_pcm", "wlx_spk_diarize_many",
    "wlx_debug_logits_get", "wlx_debug_decode_logits", "wlx_debug_search", "wlx_debug_search_batch", "wlx_debug_time_decode_step", "wlx_debug_profile_step", "wlx_debug_trace_step",
    "wlx_mt_debug_encode", "wlx_mt_debug_decode_logits", "wlx_mt_debug_timings", "wlx_mt_debug_attn", "wlx_mt_debug_topk",
    "wlx_mt_debug_embed", "wlx_mt_debug_search", "wlx_mt_debug_kv_append", "wlx_mt_debug_relu",
    "wlx_spk_debug_timings", "wlx_spk_debug_fbank", "wlx_spk_debug_conv", "wlx_spk_debug_pool",
    "wlx_spk_debug_conv_batch", "wlx_spk_debug_pool_batch", "wlx_spk_debug_fbank_batch", "wlx_spk_debug_head",
    "wlx_spk_debug_affinity", "wlx_spk_debug_ahc", "wlx_spk_debug_affinity_many", "wlx_spk_debug_ahc_many",
    "wlx_spk_debug_cluster_timings",
    "wlx_debug_layernorm", "wlx_debug_attn_encoder", "wlx_debug_dec_cross_attn", "wlx_debug_dec_self_attn", "wlx_debug_gemm",
    "wlx_debug_dec_gemv", "wlx_debug_dec_cq_cross_attn",
    "wlx_debug_resample", "wlx_debug_resample_split", "wlx_debug_resample_timed", "wlx_debug_resample_stream", "wlx_debug_flac_decode", "wlx_debug_flac_timings", "wlx_debug_adpcm_decode",
    "wlx_debug_resample_many", "wlx_debug_flac_decode_many", "wlx_debug_put_many_budget",
    "wlx_debug_dtw", "wlx_debug_align_post", "wlx_debug_align_timings", "wlx_debug_bias_apply",
    "wlx_debug_token_prob", "wlx_debug_token_prob_rows", "wlx_debug_lang_probs", "wlx_debug_dec_embed", "wlx_debug_prep_windows",
    "wlx_debug_f32_to_f16",
    "wlx_vad_debug_frontend", "wlx_vad_debug_lstm", "wlx_vad_debug_out",
]
# the per-item part of keyword boosting, declared in include/wlx_bias_items.h (which wlx.h includes): EXPORTS is wlx.h's own list
EXPORTS_BIAS_ITEMS = ["wlx_bias_set_items", "wlx_bias_select", "wlx_debug_bias_apply_items"]
# grammar-constrained decoding, declared in include/wlx_grammar.h (which wlx.h includes)
EXPORTS_GRAMMAR = ["wlx_grammar_set", "wlx_grammar_clear", "wlx_debug_grammar_apply"]


# MFMA accumulators in VGPRs (gfx950 has ONE register file; hipcc's default puts C/D in its AGPR half): every VALU touch of
# an accumulator — the softmax rescale of the attention kernel, the GEMM epilogues — otherwise costs a v_accvgpr_read and
# a v_accvgpr_write per register: a third of all VALU instructions of the encoder attention kernel (576 of 1738 per six key
# tiles), which is VALU-issue bound (rocprofv3: SQ_ACTIVE_INST_VALU 56 % of its wave cycles). No kernel spills with it.
HIPCC_EXTRA = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
# Kernel-argument preload (csrc/dec_gemv_internal.h, WLX_KERNARG_HEAD): the command processor places the leading kernel-argument dwords into user SGPRs
# at dispatch. The translation units of the decode step's kernels only (the vocabulary projection's not yet: it takes one struct) — their launches last 2 us each, an argument fetch is a tenth of that; the encoder, VAD, MT
# and speaker kernels run 15-30 us launches and keep their flags. A build with -DWLX_KERNARG_HEAD=0 (the previous argument layout) leaves it out.
KERNARG_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=14"]
KERNARG_PRELOAD_SOURCES = ("dec_gemv.hip", "decoder.hip", "search.hip")   # (decoder.hip, search.hip: flat argument lists as they stand)


class WlxError(RuntimeError):
    code = None             # the wlx_status the library returned (set by `check`)


class wlx_spec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_mels", "d_model", "n_heads", "enc_layers", "dec_layers", "ffn", "vocab", "n_audio_ctx", "n_text_ctx")]


class wlx_tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4),
                ("on_device", C.c_int32)]


class wlx_token_ids(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sot", "eot", "no_timestamps", "timestamp_begin", "no_speech", "blank")]


class wlx_gen_opts(C.Structure):
    _fields_ = [
        ("beam_size", C.c_int32), ("patience", C.c_float), ("num_hypotheses", C.c_int32),
        ("length_penalty", C.c_float), ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32),
        ("max_length", C.c_int32), ("suppress_blank", C.c_int32), ("suppress_tokens", C.POINTER(C.c_int32)),
        ("n_suppress_tokens", C.c_int32), ("max_initial_timestamp_index", C.c_int32), ("sampling_topk", C.c_int32),
        ("sampling_temperature", C.c_float), ("seed", C.c_uint64), ("ids", wlx_token_ids),
    ]


class wlx_timings(C.Structure):
    _fields_ = [("logmel_ms", C.c_float), ("encode_ms", C.c_float), ("generate_ms", C.c_float), ("decode_steps", C.c_int32)]


class wlx_kernel_stat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches_per_step", C.c_float), ("avg_us", C.c_float),
                ("total_us_per_step", C.c_float), ("bytes_per_launch", C.c_double)]


class wlx_vad_weights(C.Structure):
    _fields_ = [("stft_basis", C.POINTER(C.c_float)), ("enc_w", C.POINTER(C.c_float) * 4), ("enc_b", C.POINTER(C.c_float) * 4),
                ("lstm_w_ih", C.POINTER(C.c_float)), ("lstm_w_hh", C.POINTER(C.c_float)), ("lstm_b_ih", C.POINTER(C.c_float)),
                ("lstm_b_hh", C.POINTER(C.c_float)), ("out_w", C.POINTER(C.c_float)), ("out_b", C.POINTER(C.c_float))]


class wlx_flac_info(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32), ("total_samples", C.c_int64),
                ("n_frames", C.c_int32), ("max_blocksize", C.c_int32), ("served", C.c_int32)]


class wlx_wav_info(C.Structure):
    _fields_ = [("format_tag", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_int32), ("bits_per_sample", C.c_int32),
                ("block_align", C.c_int32), ("samples_per_block", C.c_int32), ("data_offset", C.c_int64), ("data_bytes", C.c_int64),
                ("n_frames", C.c_int64), ("served", C.c_int32)]


class wlx_put_entry(C.Structure):
    _fields_ = [("kind", C.c_int32), ("data", C.c_void_p), ("n", C.c_int64), ("channels", C.c_int32), ("sample_format", C.c_int32),
                ("sample_rate", C.c_int32)]


class wlx_put_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_out", C.c_int64)]


class wlx_mt_spec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "n_heads", "enc_layers", "dec_layers", "ffn", "vocab", "max_positions",
                                         "pad_id", "eos_id", "decoder_start_id", "scale_embedding")]


class wlx_spk_cluster_opts(C.Structure):
    _fields_ = [("threshold", C.c_float), ("max_clusters", C.c_int32)]


class wlx_spk_spec(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("planes", C.c_int32), ("blocks", C.c_int32 * 4), ("embed_dim", C.c_int32),
                ("max_seconds", C.c_int32), ("pool_eps", C.c_float)]


ERR_TOO_SHORT = 6       # wlx_status WLX_ERR_TOO_SHORT
ERR_DATA = 7            # wlx_status WLX_ERR_DATA: damaged input (the FLAC and telephony WAV front ends)
SPK_MAX_BATCH = 64      # wlx.h WLX_SPK_MAX_BATCH: segments of one wlx_spk_embed_batch call
SPK_CLUSTER_MAX = 2048  # wlx.h WLX_SPK_CLUSTER_MAX: rows of one wlx_spk_cluster / windows of one wlx_spk_diarize_pcm call
SPK_MIN_SAMPLES = 4800  # csrc/spk.h WLX_SPK_MIN_SAMPLES: a shorter window or segment takes no part (WLX_ERR_TOO_SHORT)
SPK_MANY_MAX_FILES = 64                                   # wlx.h WLX_SPK_MANY_MAX_FILES: files of one wlx_spk_diarize_many call,
SPK_MANY_MAX_ROWS = 8192                                   # WLX_SPK_MANY_MAX_ROWS: their windows together,
SPK_MANY_MAX_CELLS = 4 * SPK_CLUSTER_MAX * SPK_CLUSTER_MAX  # WLX_SPK_MANY_MAX_CELLS: floats of their distance matrices together
VAD_MAX_BATCH = 64      # wlx.h WLX_VAD_MAX_BATCH: sequences of one wlx_vad_probs_batch / wlx_vad_probs_pcm_batch call
ALIGN_MAX_BATCH = 64    # wlx.h WLX_ALIGN_MAX_BATCH: entries of one wlx_align_batch call
ALIGN_MAX_MEDIAN = 15   # wlx.h WLX_ALIGN_MAX_MEDIAN: the widest median filter the device post-processing serves
BIAS_MAX_NODES, BIAS_MAX_EDGES, BIAS_MAX_TOKENS = 4096, 16384, 1024   # wlx.h WLX_BIAS_MAX_*: the caps of a bias table (wlx_bias_set)
# wlx_bias_items.h WLX_BIAS_SET_MAX_*: tables of one set (wlx_bias_set_items) and the caps of its pool; WLX_BIAS_EDGE_SHARED: the flag bit in edge_next
BIAS_SET_MAX_TABLES, BIAS_SET_MAX_NODES, BIAS_SET_MAX_EDGES, BIAS_SET_MAX_TOKENS = 64, 16384, 65536, 4096
BIAS_EDGE_SHARED = 0x40000000
GRAMMAR_MAX_STATES, GRAMMAR_MAX_EDGES = 4096, 16384      # wlx_grammar.h WLX_GRAMMAR_MAX_*: the caps of a grammar table (wlx_grammar_set)
DEBUG_GUARD = 64        # wlx.h WLX_DEBUG_GUARD: words a debug hook's output carries past what the kernel owns
MT_MANY_MAX = 4096      # wlx.h WLX_MT_MANY_MAX: sources of one wlx_mt_translate_many call
ERR_ARG = 1             # wlx_status WLX_ERR_ARG
PUT_PCM, PUT_FRAMES, PUT_FLAC, PUT_WAV = 0, 1, 2, 3   # wlx.h WLX_PUT_*: the kinds of a wlx_put_entry
PUT_MANY_MAX = 64       # wlx.h WLX_PUT_MANY_MAX: entries of one wlx_pcm_put_many call
ERR_STATE = 4           # wlx_status WLX_ERR_STATE
LM_MAXRANGES = 256      # wlx.h WLX_LM_MAXRANGES: ranges per chunk of wlx_logmel_chunks / wlx_logmel_ring
PCM_F32, PCM_S16 = 0, 1           # wlx.h WLX_PCM_F32 / WLX_PCM_S16
PCM_U8, PCM_MULAW, PCM_ALAW = 3, 4, 5   # wlx.h WLX_PCM_U8 / _MULAW / _ALAW: the live path's 8-bit wire formats (wlx_ring_set_format); 2 is unassigned
PCM_MAX_CHANNELS = 8
# what the device resampler serves (csrc/resample.hip resample_ratio; engine.resample_supported restates its rule)
RESAMPLE_MAX_RATIO = 640          # max(up, down) of 16000 / rate (RS_MAX_RATIO)
RESAMPLE_MIN_TILE = 64            # the smallest tile of outputs a workgroup takes (RS_MIN_TILE) ...
RESAMPLE_MAX_LDS = 64 * 1024      # ... whose input span, with the tap table, has to fit this many bytes (RS_MAX_LDS)


class wlx_debug_gemm_args(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("zbatch", "M", "N", "K", "KT", "conv3_cin", "mode", "force_form", "d", "rows_per_item")] +
                [("qscale", C.c_float), ("reserved", C.c_int32)] +
                [(n, C.c_int64) for n in ("lda", "strideA", "a_len", "ldc", "strideC", "c_len", "ldx", "strideX", "x_len",
                                          "ldk", "kv_item_stride_k", "kv_layer_stride_k", "k_len",
                                          "ldvt", "kv_item_stride_v", "kv_layer_stride_v", "v_len")])


class wlx_debug_dec_gemv_args(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("in_mode", "out_mode", "xsrc", "M", "K", "KT", "N", "busy_device", "KTS", "H", "R", "d")] +
                [("qscale", C.c_float), ("reserved", C.c_int32)] +
                [(n, C.c_int64) for n in ("ldx", "ldxh", "ldyh", "ldy", "ldxres", "cache_row_stride", "slab_stride",
                                          "x_len", "xh_len", "part_o_len", "part_ml_len", "slab_len", "tok_emb_len", "pos_emb_len",
                                          "yh_len", "y_len", "xres_len", "kc_len", "vc_len", "intok_len")])


class wlx_mt_gen_opts(C.Structure):
    _fields_ = [("num_beams", C.c_int32), ("max_length", C.c_int32), ("early_stopping", C.c_int32),
                ("length_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32), ("forced_eos_token_id", C.c_int32)]


_extra_ok = None
_preload_ok = None


def _hipcc() -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise WlxError("hipcc not found: cannot build libwlx.so (ROCm toolchain required)")
    return hipcc


def _compile(out: Path, defines=(), verbose: bool = False, force: bool = False) -> Path:
    """hipcc --offload-arch=gfx950 of every source into `out`: one object per source (compiled in parallel, cached under
    csrc/.obj/<variant>/ and rebuilt when the source or any header is newer), linked into a temporary file and renamed
    (concurrent builders never see a half-written library). HIPCC_EXTRA is a hidden LLVM option: a hipcc that does not know
    it fails with 'Unknown command line argument' — retry once without it (the AGPR-form build: correct, the encoder
    attention ~8 % slower) and remember the answer for the other builds of this process. KERNARG_PRELOAD is decided on its own:
    a hipcc that rejects only that option keeps HIPCC_EXTRA, says so, and builds the argument head without the preload (correct:
    the kernels fetch the head themselves; the decode step loses log K1's gain)."""
    global _extra_ok, _preload_ok
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    defines = list(defines)
    hdrs = list(CSRC.glob("*.h")) + list((PKG_DIR.parent / "include").glob("*.h"))
    hdr_time = max(h.stat().st_mtime for h in hdrs)
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + [f"-D{d}" for d in defines]

    want_pre = "WLX_KERNARG_HEAD=0" not in defines

    def objects(extra, preload):
        tag = "_".join(["base" if extra else "agpr"] + (["nopre"] if want_pre and not preload else []) + [d.replace("=", "-") for d in defines])
        odir = CSRC / ".obj" / tag
        odir.mkdir(parents=True, exist_ok=True)

        def one(src):
            pre = KERNARG_PRELOAD if (preload and src in KERNARG_PRELOAD_SOURCES) else []
            obj = odir / (src + (".pre.o" if pre else ".o"))       # (the option is part of the cached object's name: the list of sources that get it may change)
            sp = CSRC / src
            if not force and obj.exists() and obj.stat().st_mtime >= max(sp.stat().st_mtime, hdr_time):
                return obj, None           # (force=True: a new hipcc / ROCm or changed flags must not link stale objects)
            tmp = obj.with_name(obj.name + f".tmp{os.getpid()}")
            proc = subprocess.run(base + extra + pre + ["-c", str(sp), "-o", str(tmp)], capture_output=True, text=True)
            if verbose and (proc.stdout or proc.stderr):
                print(proc.stdout, proc.stderr)
            if proc.returncode != 0:
                if tmp.exists():
                    tmp.unlink()
                return None, proc
            os.replace(tmp, obj)
            return obj, None
        with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4)) as ex:
            return list(ex.map(one, SOURCES))

    for _attempt in range(3):
        extra = HIPCC_EXTRA if _extra_ok is not False else []
        preload = want_pre and _preload_ok is not False
        res = objects(extra, preload)
        bad = [p for o, p in res if o is None]
        if not bad:
            if extra:
                _extra_ok = True
            if preload:
                _preload_ok = True
            tmp = out.with_name(out.name + f".tmp{os.getpid()}")
            proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(tmp)] + [str(o) for o, _ in res],
                                  capture_output=True, text=True)
            if proc.returncode != 0:
                if tmp.exists():
                    tmp.unlink()
                raise WlxError(f"hipcc link failed ({proc.returncode}):\n{proc.stderr[-4000:]}")
            os.replace(tmp, out)
            return out
        err = bad[0].stderr
        if (extra or preload) and ("Unknown command line argument" in err or "unknown argument" in err.lower()):
            # the error names the option it does not know; where it names neither, both go
            no_pre = preload and (KERNARG_PRELOAD[1].split("=")[0] in err or HIPCC_EXTRA[1].split("=")[0] not in err)
            no_extra = bool(extra) and (HIPCC_EXTRA[1].split("=")[0] in err or KERNARG_PRELOAD[1].split("=")[0] not in err)
            if no_pre:
                _preload_ok = False
                print(f"[wlx build] this hipcc rejects {' '.join(KERNARG_PRELOAD)}: the decode projections fetch their argument head themselves")
            if no_extra:
                _extra_ok = False
                print(f"[wlx build] this hipcc rejects {' '.join(HIPCC_EXTRA)}: building with MFMA accumulators in AGPR form")
            continue
        raise WlxError(f"hipcc failed ({bad[0].returncode}):\n{err[-4000:]}")
    raise WlxError("hipcc failed")


def _fresh(out: Path) -> bool:
    deps = [CSRC / s for s in SOURCES] + list(CSRC.glob("*.h")) + list((PKG_DIR.parent / "include").glob("*.h"))
    return out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps)


def build_trace() -> Path:
    """libwlx_trace.so: the same sources with -DWLX_TRACE (in-kernel timeline marks, profiling only)."""
    out = PKG_DIR / "libwlx_trace.so"
    return out if _fresh(out) else _compile(out, ["WLX_TRACE"])


def build_ab() -> Path:
    """libwlx_ab.so: the same sources with -DWLX_AB — the A/B switches that survive in the source (csrc/common.h wlx_ab: WLX_GEMM3,
    WLX_GEMM2_SHAPE, WLX_DECODE_V1) read the environment in THIS library only; the production libwlx.so compiles them out.
    Select with WLX_LIB=<path>."""
    out = PKG_DIR / "libwlx_ab.so"
    return out if _fresh(out) else _compile(out, ["WLX_AB"])


def build_variant(name: str, defines) -> Path:
    """Builds of the same sources with extra -D flags (e.g. libwlx_ks4.so: -DWLX_FC2_KS=4, the MLP output projection cut into
    four K slices; -DWLX_RESID_BATCHED=0, the encoder's tile-by-tile residual update); selected at run time with WLX_LIB=<path>."""
    out = PKG_DIR / name
    return out if _fresh(out) else _compile(out, list(defines))


def build_nohead() -> Path:
    """libwlx_nohead.so: -DWLX_KERNARG_HEAD=0 — the decode projections with their arguments in one by-value struct and no kernel-argument
    preload (the layout before the argument head): the A/B partner of libwlx.so for that change. Select with WLX_LIB=<path>."""
    return build_variant("libwlx_nohead.so", ["WLX_KERNARG_HEAD=0"])


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile every HIP source for gfx950 into whisperlive_amd/libwlx.so (hipcc cross-compiles without a GPU)."""
    if not force and _fresh(DEFAULT_LIB):
        return DEFAULT_LIB
    return _compile(DEFAULT_LIB, (), verbose, force=force)


_lib = None


def load() -> C.CDLL:
    """Load libwlx.so and declare prototypes. Raises WlxError (never falls back) if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise WlxError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). whisperlive_amd has no CPU fallback.")
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:  # e.g. libamdhip64 missing
        raise WlxError(f"cannot load {LIB_PATH}: {e}") from e
    missing = [s for s in EXPORTS + EXPORTS_GRAMMAR if not hasattr(lib, s)]
    if missing:
        raise WlxError(f"libwlx.so lacks symbols {missing}")
    i32, i64, f32p, i32p, vp = C.c_int32, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    lib.wlx_abi_version.restype = i32
    lib.wlx_last_error.restype = C.c_char_p
    lib.wlx_engine_create.argtypes = [C.POINTER(wlx_spec), C.POINTER(wlx_tensor), i32, i32, C.POINTER(vp)]
    lib.wlx_engine_destroy.argtypes = [vp]
    lib.wlx_engine_destroy.restype = None
    lib.wlx_engine_spec.argtypes = [vp, C.POINTER(wlx_spec)]
    lib.wlx_slot_create.argtypes = [vp, i32, i32, i32p]
    lib.wlx_slot_destroy.argtypes = [vp, i32]
    lib.wlx_logmel.argtypes = [vp, i32, i32, f32p, i64, i32p]
    lib.wlx_pcm_put.argtypes = [vp, i32, i32, f32p, i64]
    lib.wlx_pcm_put_frames.argtypes = [vp, i32, i32, vp, i64, i32, i32, i32, C.POINTER(C.c_int64)]
    lib.wlx_pcm_put_frames_split.argtypes = [vp, i32, i32, vp, i64, i32, i32, i32, C.POINTER(C.c_int64)]
    lib.wlx_flac_probe.argtypes = [vp, i64, C.POINTER(wlx_flac_info)]
    lib.wlx_pcm_put_flac.argtypes = [vp, i32, i32, vp, i64, C.POINTER(wlx_flac_info), C.POINTER(C.c_int64)]
    lib.wlx_pcm_put_flac_split.argtypes = [vp, i32, i32, vp, i64, C.POINTER(wlx_flac_info), C.POINTER(C.c_int64)]
    lib.wlx_wav_probe.argtypes = [vp, i64, C.POINTER(wlx_wav_info)]
    lib.wlx_pcm_put_wav.argtypes = [vp, i32, i32, vp, i64, C.POINTER(wlx_wav_info), C.POINTER(C.c_int64)]
    lib.wlx_pcm_put_wav_split.argtypes = [vp, i32, i32, vp, i64, C.POINTER(wlx_wav_info), C.POINTER(C.c_int64)]
    lib.wlx_pcm_put_many.argtypes = [vp, i32, i32, i32, C.POINTER(wlx_put_entry), C.POINTER(wlx_put_result)]
    lib.wlx_pcm_get.argtypes = [vp, i32, i32, f32p, i64, C.POINTER(C.c_int64)]
    lib.wlx_logmel_resident.argtypes = [vp, i32, i32, i32p]
    lib.wlx_features_get.argtypes = [vp, i32, i32, f32p, i64, i32p]
    lib.wlx_features_set.argtypes = [vp, i32, i32, f32p, i32, i32]
    lib.wlx_encode.argtypes = [vp, i32, i32, i32p, i32p]
    lib.wlx_encoder_output_get.argtypes = [vp, i32, i32, f32p, i64]
    lib.wlx_generate.argtypes = [vp, i32, i32, i32p, i32p, i32, C.POINTER(wlx_gen_opts), i32p, i32, i32p, f32p, f32p]
    lib.wlx_generate_ex.argtypes = [vp, i32, i32, i32p, i32p, i32p, i32, C.POINTER(wlx_gen_opts), i32p, i32, i32p, f32p, f32p]
    lib.wlx_detect_language.argtypes = [vp, i32, i32, i32, i32p, i32, f32p]
    lib.wlx_align.argtypes = [vp, i32, i32, i32p, i32, i32, i32, i32, i32p, i32, i32, i32p, i32p, i32, i32p, f32p]
    lib.wlx_align_batch.argtypes = [vp, i32, i32, i32p, i32p, i32p, i32, i32, i32p, i32, i32p, i32, i32, i32p, i32p, i32, i32p, f32p, i32]
    lib.wlx_timings_get.argtypes = [vp, i32, C.POINTER(wlx_timings)]
    lib.wlx_sync.argtypes = [vp, i32]
    lib.wlx_vad_create.argtypes = [C.POINTER(wlx_vad_weights), i32, C.POINTER(vp)]
    lib.wlx_vad_destroy.argtypes = [vp]
    lib.wlx_vad_destroy.restype = None
    lib.wlx_vad_probs.argtypes = [vp, f32p, i64, f32p, i32, i32p, f32p]
    i64p = C.POINTER(C.c_int64)
    lib.wlx_ring_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.wlx_ring_destroy.argtypes = [vp]
    lib.wlx_ring_destroy.restype = None
    lib.wlx_ring_append.argtypes = [vp, f32p, i64, i64, i64, i64p, i64p, i64p]
    lib.wlx_ring_state.argtypes = [vp, i64p, i64p]
    lib.wlx_ring_set_format.argtypes = [vp, i32, i32, i32]
    lib.wlx_ring_append_frames.argtypes = [vp, vp, i64, i32, i64, i64, f32p, i64, i64p, i64p, i64p, i64p]
    lib.wlx_resample_stream_count.argtypes = [i32, i64, i32, i64p]
    lib.wlx_ring_group_create.argtypes = [vp, i64, i32, i32, i32, C.POINTER(vp)]
    lib.wlx_ring_group_destroy.argtypes = [vp]
    lib.wlx_ring_group_destroy.restype = None
    lib.wlx_ring_group_lane.argtypes = [vp, i32, C.POINTER(vp)]
    lib.wlx_ring_group_append_frames.argtypes = [vp, vp, i64, i32, i64, i64, f32p, i64, i64p, i64p, i64p, i64p]
    lib.wlx_vad_probs_resident.argtypes = [vp, vp, i64, i64, i32, f32p, i32, i32p, f32p]
    lib.wlx_vad_segments.argtypes = [f32p, i32, i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, i64p, i32, i32p]
    lib.wlx_logmel_ring.argtypes = [vp, i32, i32, vp, i64p, i32, i32p]
    lib.wlx_logmel_chunks.argtypes = [vp, i32, i32, i64p, i32p, i32, i32, i32p]
    lib.wlx_logmel_chunks_multi.argtypes = [vp, i32, i32p, i64p, i32p, i32, i32, i32p]
    lib.wlx_vad_probs_pcm.argtypes = [vp, vp, i32, i32, i64, i64, i32, f32p, i32, i32p, f32p]
    lib.wlx_vad_probs_batch.argtypes = [vp, f32p, i64p, i32p, i32, f32p, i64, i32p, f32p]
    lib.wlx_vad_probs_pcm_batch.argtypes = [vp, vp, i32, i32, i64p, i32p, i32, f32p, i64, i32p, f32p]
    lib.wlx_debug_logits_get.argtypes = [vp, i32, f32p, i32, i64]
    lib.wlx_debug_decode_logits.argtypes = [vp, i32, i32p, i32, f32p]
    lib.wlx_debug_search.argtypes = [vp, i32, f32p, i32, i32p, i32, C.POINTER(wlx_gen_opts), i32p, i32, i32p, f32p]
    lib.wlx_debug_search_batch.argtypes = [vp, i32, f32p, i32, i32, i32p, i32p, i32, C.POINTER(wlx_gen_opts), i32p, i32, i32p, f32p]
    lib.wlx_debug_time_decode_step.argtypes = [vp, i32, i32, i32, i32, f32p]
    lib.wlx_debug_profile_step.argtypes = [vp, i32, i32, i32, i32, C.POINTER(wlx_kernel_stat), i32, i32p]
    lib.wlx_debug_trace_step.argtypes = [vp, i32, i32, i32, i32, C.POINTER(C.c_uint64), i64, C.c_char_p, i32p]
    lib.wlx_mt_create.argtypes = [C.POINTER(wlx_mt_spec), C.POINTER(wlx_tensor), i32, i32, C.POINTER(vp)]
    lib.wlx_mt_destroy.argtypes = [vp]
    lib.wlx_mt_destroy.restype = None
    lib.wlx_mt_slot_create.argtypes = [vp, i32, i32, i32, i32p]
    lib.wlx_mt_slot_destroy.argtypes = [vp, i32]
    lib.wlx_mt_translate.argtypes = [vp, i32, i32, i32p, i32p, i32, C.POINTER(wlx_mt_gen_opts), i32p, i32, i32p, f32p]
    lib.wlx_mt_translate_many.argtypes = [vp, i32, i32, i32p, i32p, i32, C.POINTER(wlx_mt_gen_opts), i32p, i32, i32p, f32p]
    lib.wlx_mt_debug_search.argtypes = [i32, f32p, i32, i32, C.POINTER(wlx_mt_gen_opts), i32, i32, i32, i32, i32, i32, i32, i32p, i32, i32p, f32p, i32p]
    lib.wlx_mt_debug_encode.argtypes = [vp, i32, i32, i32p, i32p, i32, f32p, i64]
    lib.wlx_mt_debug_decode_logits.argtypes = [vp, i32, i32p, i32, i32p, i32, f32p]
    lib.wlx_mt_debug_timings.argtypes = [vp, i32, f32p, f32p, i32p]
    u16p = C.POINTER(C.c_uint16)
    lib.wlx_mt_debug_attn.argtypes = [i32, u16p, i64, i64, u16p, i64, u16p, i64, i64, i32p, i32, i32, i32, i32p, i32, i32, u16p, i64, i64]
    lib.wlx_mt_debug_topk.argtypes = [i32, f32p, i32, i32, i32p, i32p, i32, i32, f32p, i32p]
    lib.wlx_mt_debug_embed.argtypes = [i32, f32p, i32, i32, i32p, i32p, i32, C.c_float, f32p, i32, f32p]
    lib.wlx_spk_create.argtypes = [C.POINTER(wlx_spk_spec), C.POINTER(wlx_tensor), i32, i32, C.POINTER(vp)]
    lib.wlx_spk_destroy.argtypes = [vp]
    lib.wlx_spk_destroy.restype = None
    lib.wlx_spk_embed.argtypes = [vp, f32p, i64, f32p]
    lib.wlx_spk_embed_batch.argtypes = [vp, f32p, i64p, i32, f32p, i32p]
    lib.wlx_spk_embed_pcm_batch.argtypes = [vp, vp, i32, i32, i64p, i64p, i32, f32p, i32p]
    lib.wlx_spk_embed_ring_batch.argtypes = [vp, vp, i64p, i64p, i32, f32p, i32p]
    copts = C.POINTER(wlx_spk_cluster_opts)
    lib.wlx_spk_cluster.argtypes = [vp, f32p, i32, i32, copts, i32p, f32p, i32p]
    lib.wlx_spk_diarize_pcm.argtypes = [vp, vp, i32, i32, i64p, i64p, i32, copts, i32p, i32p, f32p, f32p, f32p, i32p]
    lib.wlx_spk_diarize_many.argtypes = [vp, vp, i32, i32, i32p, i32p, i64p, i64p, copts, i32p, i32p, i32p, i32p, f32p, f32p]
    lib.wlx_spk_debug_affinity_many.argtypes = [i32, f32p, i32, i32p, i32, f32p]
    lib.wlx_spk_debug_ahc_many.argtypes = [i32, f32p, i32, i32p, copts, i32p, i32p, f32p, i32p, i32p]
    lib.wlx_spk_debug_affinity.argtypes = [i32, f32p, i32, i32, f32p]
    lib.wlx_spk_debug_ahc.argtypes = [i32, f32p, i32, copts, i32p, i32p, f32p, i32p, i32p]
    lib.wlx_spk_debug_cluster_timings.argtypes = [vp, f32p, f32p]
    lib.wlx_spk_debug_timings.argtypes = [vp, f32p, f32p]
    lib.wlx_spk_debug_fbank.argtypes = [i32, f32p, i64, i32, f32p, u16p, i32, i32p]
    lib.wlx_spk_debug_conv.argtypes = [i32, u16p, i32, i32, i32, f32p, f32p, u16p, i32, i32, i32, i32, u16p]
    lib.wlx_spk_debug_pool.argtypes = [i32, u16p, i32, i32, i32, C.c_float, f32p]
    lib.wlx_spk_debug_conv_batch.argtypes = [i32, u16p, i32, i32, i32p, i32, f32p, f32p, u16p, i32, i32, i32, i32, u16p]
    lib.wlx_spk_debug_pool_batch.argtypes = [i32, u16p, i32, i32, i32p, i32, C.c_float, f32p]
    lib.wlx_spk_debug_fbank_batch.argtypes = [i32, f32p, i64, i32, i64p, i32p, i32, f32p, u16p]
    lib.wlx_spk_debug_head.argtypes = [i32, f32p, f32p, f32p, i32, i32, i32, i32, f32p]
    lib.wlx_mt_debug_kv_append.argtypes = [i32, u16p, i64, i32, i32, u16p, u16p, i32, i32, i32]
    lib.wlx_mt_debug_relu.argtypes = [i32, u16p, i64, i32, i32]
    lib.wlx_debug_layernorm.argtypes = [i32, f32p, i64, f32p, f32p, i32, i32, u16p, f32p, i64]
    lib.wlx_debug_attn_encoder.argtypes = [i32, u16p, i64, i64, u16p, i64, i64, u16p, i64, i64, u16p, i64, i64, i32, i32, i32]
    lib.wlx_debug_dec_cross_attn.argtypes = [i32, u16p, i64, u16p, u16p, i64, i32, i32, i32, i32, i32, i32p, u16p, f32p, u16p, i64,
                                             i32, i32, f32p]
    lib.wlx_debug_dec_self_attn.argtypes = [i32, u16p, i64, u16p, u16p, i64, i32, i32, i32, i32, i32p, i32p, C.POINTER(C.c_int16), i32,
                                            u16p, i64]
    lib.wlx_debug_gemm.argtypes = [i32, C.POINTER(wlx_debug_gemm_args), u16p, f32p, f32p, f32p, u16p, f32p, u16p, u16p, i32p]
    lib.wlx_debug_dec_gemv.argtypes = [i32, C.POINTER(wlx_debug_dec_gemv_args), f32p, f32p, f32p, f32p, f32p, u16p, u16p, f32p, f32p, u16p, f32p,
                                       i32p, i32p, i32p, u16p, f32p, f32p, u16p, u16p, i32p, C.c_char_p, i32]
    lib.wlx_debug_dec_cq_cross_attn.argtypes = [i32, f32p, i64, f32p, f32p, f32p, f32p, C.c_float, i32, u16p, u16p, i64, i32, i32, i32, i32, i32,
                                                i32p, u16p, f32p]
    lib.wlx_debug_resample.argtypes = [i32, vp, i64, i32, i32, i32, i64, f32p, i64, i64p]
    lib.wlx_debug_resample_split.argtypes = [i32, vp, i64, i32, i32, i32, i64, f32p, i64, i64p]
    lib.wlx_debug_resample_timed.argtypes = [i32, vp, i64, i32, i32, i32, i64, f32p, i64, i64p, f32p]
    lib.wlx_debug_resample_stream.argtypes = [i32, vp, i64, i32, i32, i32, i64p, i32, i32, f32p, i64, i64p, i64p]
    lib.wlx_debug_flac_decode.argtypes = [i32, vp, i64, i32p, i64, C.POINTER(C.c_int64), i32p]
    lib.wlx_debug_flac_timings.argtypes = [vp, i32, f32p]
    lib.wlx_debug_adpcm_decode.argtypes = [i32, vp, i64, C.POINTER(C.c_int16), i64, C.POINTER(C.c_int64), i32p]
    lib.wlx_debug_resample_many.argtypes = [i32, i32, C.POINTER(vp), i64p, i32p, i32p, i32p, f32p, i64p, i64, i64p]
    lib.wlx_debug_flac_decode_many.argtypes = [i32, i32, C.POINTER(vp), i64p, i32p, i64p, i64, i64p, i32p, i32p]
    lib.wlx_debug_put_many_budget.argtypes = [i64, i64p, i32p]
    lib.wlx_debug_dtw.argtypes = [i32, f32p, i32, i32p, i32p, i32p, i32p, i32, i32p]
    lib.wlx_debug_align_post.argtypes = [i32, f32p, i32, i32, i32p, i32, i32p, i32, f32p, i32p, i32p, i32, i32p]
    lib.wlx_debug_align_timings.argtypes = [vp, i32, f32p, f32p]
    i16p = C.POINTER(C.c_int16)
    lib.wlx_bias_set.argtypes = [vp, i32, i32, i32p, i32p, i32p, C.c_float, i32, i32p, f32p]
    lib.wlx_bias_clear.argtypes = [vp, i32]
    lib.wlx_bias_set_items.argtypes = [vp, i32, i32, i32p, i32p, i32p, i32p, f32p, i32p, i32p, f32p]
    lib.wlx_bias_select.argtypes = [vp, i32, i32, i32p]
    lib.wlx_debug_bias_apply_items.argtypes = [i32, i32, i32, i32, i32p, i32p, i32p, i32p, f32p, i32p, i32p, f32p, f32p, i32, i32, i32p, i64, i32p, i32p,
                                               i32p, i32p, i32p, i16p, i16p]
    lib.wlx_debug_bias_apply.argtypes = [i32, i32, i32, i32, i32p, i32p, i32p, C.c_float, i32, i32p, f32p, f32p, i32, i64, i32p, i32p, i32p, i32, i32p,
                                         i16p, i16p]
    lib.wlx_grammar_set.argtypes = [vp, i32, i32, i32, i32p, i32p, i32p, i32p]
    lib.wlx_grammar_clear.argtypes = [vp, i32]
    lib.wlx_debug_grammar_apply.argtypes = [i32, i32, i32, i32, i32p, i32p, i32p, i32p, f32p, i32, i64, i32p, i32p, i32p, i32, i32p, i16p, i16p]
    lib.wlx_debug_token_prob.argtypes = [i32, f32p, i64, i32, i32, i32, f32p]
    lib.wlx_debug_token_prob_rows.argtypes = [i32, f32p, i64, i32, i32, i32p, f32p]
    lib.wlx_debug_lang_probs.argtypes = [i32, f32p, i64, i32, i32p, i32, f32p]
    lib.wlx_debug_dec_embed.argtypes = [i32, u16p, i32, f32p, i32, i32, i32p, i32p, i32, f32p, i32p]
    lib.wlx_debug_prep_windows.argtypes = [i32, f32p, i64, i64, i32, i64, i32, i32p, i32p, u16p, i64]
    lib.wlx_debug_f32_to_f16.argtypes = [i32, f32p, i64, u16p, i64]
    lib.wlx_vad_debug_frontend.argtypes = [vp, f32p, i64p, i32p, i32, f32p, i64]
    lib.wlx_vad_debug_lstm.argtypes = [vp, f32p, i32p, i32, f32p, i64]
    lib.wlx_vad_debug_out.argtypes = [vp, f32p, i32, f32p, i64]
    for name in EXPORTS + EXPORTS_BIAS_ITEMS + EXPORTS_GRAMMAR:
        fn = getattr(lib, name)
        if name not in ("wlx_last_error", "wlx_engine_destroy", "wlx_vad_destroy", "wlx_ring_destroy", "wlx_ring_group_destroy", "wlx_mt_destroy", "wlx_spk_destroy"):
            fn.restype = i32
    if lib.wlx_abi_version() != 1:
        raise WlxError("libwlx.so ABI version mismatch")
    _lib = lib
    return lib


def tensor_array(weights):
    """dict of name -> numpy array / torch tensor -> (wlx_tensor[], keep): fp32, contiguous; a torch tensor on the GPU goes
    over as a device pointer (on_device = 1). `keep` holds the converted arrays: keep it alive while the C side reads them."""
    keep = []
    arr = (wlx_tensor * len(weights))()
    for i, (name, t) in enumerate(weights.items()):
        on_dev = 0
        if hasattr(t, "data_ptr"):            # torch tensor (PyTorch-ROCm holds the weights)
            import torch
            t = t.detach().to(torch.float32).contiguous()
            on_dev = 1 if t.is_cuda else 0
            ptr, shape = t.data_ptr(), tuple(t.shape)
        else:
            t = np.ascontiguousarray(t, dtype=np.float32)
            ptr, shape = t.ctypes.data, t.shape
        keep.append(t)
        arr[i].name = name.encode()
        arr[i].data = ptr
        arr[i].ndim = len(shape)
        for j, s in enumerate(shape):
            arr[i].shape[j] = s
        arr[i].on_device = on_dev
    return arr, keep


def check(rc: int):
    if rc != 0:
        msg = load().wlx_last_error()
        err = WlxError(f"libwlx error {rc}: {msg.decode() if msg else '?'}")
        err.code = rc
        raise err
