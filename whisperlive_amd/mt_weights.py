"""Weights, architecture and generation options of the M2M100 / small100 translation model (fp32 numpy arrays keyed by
Hugging Face M2M100 state-dict names), for the HIP translation engine (csrc/mt_engine.hip).

* ``MTSpec.from_config``   — the architecture from ``config.json`` (small100's dimensions are not hard-coded anywhere).
* ``load_mt_dir``          — ``model.safetensors`` (single or sharded) or ``pytorch_model.bin`` (``torch.load(weights_only=True)``);
                             the tied embeddings are resolved to ``model.shared.weight``.
* ``random_mt_weights``    — seeded synthetic weights (numpy RNG; the tests regenerate identical tensors without ``transformers``).
* ``generation_options``   — num_beams / max_length / early_stopping / length_penalty / no_repeat_ngram_size / forced_eos_token_id
                             resolved as ``transformers`` does for a bare ``generate(**encoded_input)``.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from typing import Dict, Optional

import numpy as np

MAX_DECODE_LENGTH = 448          # the engine's KV cache (WLX_T_TEXT): max_length counts the decoder start token


@dataclasses.dataclass(frozen=True)
class MTSpec:
    d_model: int
    n_heads: int
    enc_layers: int
    dec_layers: int
    ffn: int
    vocab: int
    max_positions: int = 1024
    pad_id: int = 1
    eos_id: int = 2
    decoder_start_id: int = 2
    scale_embedding: bool = True

    @classmethod
    def from_config(cls, cfg: dict, state_shapes: Optional[Dict[str, tuple]] = None) -> "MTSpec":
        act = cfg.get("activation_function", "relu")
        if act != "relu":
            raise ValueError(f"M2M100 engine: activation_function {act!r} is not supported (relu only)")
        heads = int(cfg.get("encoder_attention_heads", 16))
        if int(cfg.get("decoder_attention_heads", heads)) != heads:
            raise ValueError("M2M100 engine: encoder and decoder head counts differ")
        ffn = int(cfg.get("encoder_ffn_dim", 4096))
        if int(cfg.get("decoder_ffn_dim", ffn)) != ffn:
            raise ValueError("M2M100 engine: encoder and decoder FFN widths differ")
        vocab = int(cfg.get("vocab_size", 128112))
        if state_shapes:
            for k in ("model.shared.weight", "model.encoder.embed_tokens.weight", "lm_head.weight"):
                if k in state_shapes:
                    vocab = int(state_shapes[k][0])
                    break
        eos = int(cfg.get("eos_token_id", 2))
        dst = cfg.get("decoder_start_token_id")
        return cls(d_model=int(cfg.get("d_model", 1024)), n_heads=heads, enc_layers=int(cfg.get("encoder_layers", 12)),
                   dec_layers=int(cfg.get("decoder_layers", 12)), ffn=ffn, vocab=vocab,
                   max_positions=int(cfg.get("max_position_embeddings", 1024)), pad_id=int(cfg.get("pad_token_id", 1)),
                   eos_id=eos, decoder_start_id=int(dst) if dst is not None else eos,
                   scale_embedding=bool(cfg.get("scale_embedding", True)))

    def hf_config(self) -> dict:
        """the config.json of this spec (the fixture generator and save_pretrained round trips)"""
        return dict(model_type="m2m_100", architectures=["M2M100ForConditionalGeneration"], vocab_size=self.vocab,
                    d_model=self.d_model, encoder_layers=self.enc_layers, decoder_layers=self.dec_layers,
                    encoder_attention_heads=self.n_heads, decoder_attention_heads=self.n_heads, encoder_ffn_dim=self.ffn,
                    decoder_ffn_dim=self.ffn, max_position_embeddings=self.max_positions, pad_token_id=self.pad_id,
                    bos_token_id=0, eos_token_id=self.eos_id, decoder_start_token_id=self.decoder_start_id,
                    scale_embedding=self.scale_embedding, activation_function="relu", dropout=0.0, attention_dropout=0.0,
                    activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0, tie_word_embeddings=True)


# small100 (alirezamsh/small100): M2M100 with a 12-layer encoder and a 3-layer decoder at Whisper-medium's width
SMALL100 = MTSpec(d_model=1024, n_heads=16, enc_layers=12, dec_layers=3, ffn=4096, vocab=128112)


def layer_names(spec: MTSpec):
    """every tensor the engine reads, in a stable order"""
    out = ["model.shared.weight"]
    attn = ("q_proj", "k_proj", "v_proj", "out_proj")
    for side, n, blocks in (("encoder", spec.enc_layers, ("self_attn",)), ("decoder", spec.dec_layers, ("self_attn", "encoder_attn"))):
        for l in range(n):
            p = f"model.{side}.layers.{l}."
            lns = ["self_attn_layer_norm", "final_layer_norm"] + (["encoder_attn_layer_norm"] if side == "decoder" else [])
            for ln in lns:
                out += [p + ln + ".weight", p + ln + ".bias"]
            for b in blocks:
                for a in attn:
                    out += [p + f"{b}.{a}.weight", p + f"{b}.{a}.bias"]
            out += [p + "fc1.weight", p + "fc1.bias", p + "fc2.weight", p + "fc2.bias"]
        out += [f"model.{side}.layer_norm.weight", f"model.{side}.layer_norm.bias"]
    return out


def random_mt_weights(spec: MTSpec, seed: int = 0, peaked: bool = False, eos_margin: float = 2.0) -> Dict[str, np.ndarray]:
    """Seeded weights whose activations stay O(1) through both stacks. ``peaked``: the decoder's final LayerNorm bias gets a
    large component along one direction u and the EOS row of the shared embedding a component along u, so that the EOS logit
    is lifted by ~eos_margin standard deviations of the other logits — beams then finish after a few to a few tens of steps
    instead of running to max_length (the output projection is tied and has no bias of its own)."""
    rng = np.random.default_rng(seed)
    d, F, V = spec.d_model, spec.ffn, spec.vocab
    w: Dict[str, np.ndarray] = {}
    # small embeddings: with tied input / output embeddings a large input share of the residual stream makes every step predict
    # the token it was fed; the decoder's final LayerNorm gain restores logits of unit spread (see `sigma` below)
    emb_std = (0.1 / math.sqrt(d)) if spec.scale_embedding else 1.0
    out_gain = 10.0 if spec.scale_embedding else 1.0
    w["model.shared.weight"] = (rng.standard_normal((V, d), dtype=np.float32) * emb_std).astype(np.float32)
    w["model.shared.weight"][spec.pad_id] = 0.0

    def lin(name, n, k, gain=0.7):
        w[name + ".weight"] = (rng.standard_normal((n, k), dtype=np.float32) * (gain / math.sqrt(k))).astype(np.float32)
        w[name + ".bias"] = (rng.standard_normal(n, dtype=np.float32) * 0.05).astype(np.float32)

    def ln(name):
        w[name + ".weight"] = (1.0 + 0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
        w[name + ".bias"] = (0.05 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)

    for side, n, blocks in (("encoder", spec.enc_layers, ("self_attn",)), ("decoder", spec.dec_layers, ("self_attn", "encoder_attn"))):
        for l in range(n):
            p = f"model.{side}.layers.{l}."
            ln(p + "self_attn_layer_norm")
            if side == "decoder":
                ln(p + "encoder_attn_layer_norm")
            ln(p + "final_layer_norm")
            for b in blocks:
                for a in ("q_proj", "k_proj", "v_proj"):
                    lin(p + f"{b}.{a}", d, d, gain=1.0)
                lin(p + f"{b}.out_proj", d, d, gain=0.5)
            lin(p + "fc1", F, d)
            lin(p + "fc2", d, F, gain=0.5)
        ln(f"model.{side}.layer_norm")
    w["model.decoder.layer_norm.weight"] = (w["model.decoder.layer_norm.weight"] * out_gain).astype(np.float32)
    if peaked:
        u = rng.standard_normal(d).astype(np.float32)
        u /= np.linalg.norm(u)
        w["model.decoder.layer_norm.bias"] = (w["model.decoder.layer_norm.bias"] + 3.0 * u).astype(np.float32)
        # other logits: h . e_j with |h| ~ out_gain sqrt(d), e_j ~ N(0, emb_std^2) per element -> spread sigma = out_gain sqrt(d) emb_std
        sigma = out_gain * math.sqrt(d) * emb_std
        w["model.shared.weight"][spec.eos_id] = (w["model.shared.weight"][spec.eos_id] + (eos_margin * sigma / 3.0) * u).astype(np.float32)
    return w


def _normalise_keys(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    out = {}
    for k, v in sd.items():
        if not k.startswith("model.") and not k.startswith("lm_head."):
            k = "model." + k
        out[k] = v
    if "model.shared.weight" not in out:
        for alt in ("model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight", "lm_head.weight"):
            if alt in out:
                out["model.shared.weight"] = out[alt]
                break
    return out


def read_state_dict(path: str) -> Dict[str, np.ndarray]:
    """fp32 numpy state dict of a Hugging Face M2M100 directory (safetensors single / sharded, or pytorch_model.bin)"""
    def f32(a):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float32))

    sd: Dict[str, np.ndarray] = {}
    st_single = os.path.join(path, "model.safetensors")
    st_index = os.path.join(path, "model.safetensors.index.json")
    pt = os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(st_single) or os.path.isfile(st_index):
        from safetensors.torch import load_file
        files = [st_single] if os.path.isfile(st_single) else sorted(
            {os.path.join(path, f) for f in json.load(open(st_index))["weight_map"].values()})
        for f in files:
            for k, v in load_file(f).items():
                sd[k] = f32(v.float().numpy())
    elif os.path.isfile(pt):
        import torch
        for k, v in torch.load(pt, map_location="cpu", weights_only=True).items():
            if hasattr(v, "float"):
                sd[k] = f32(v.float().numpy())
    else:
        raise FileNotFoundError(f"{path}: neither model.safetensors(.index.json) nor pytorch_model.bin")
    return _normalise_keys(sd)


def load_mt_dir(path: str):
    """(MTSpec, weights) of a Hugging Face M2M100 directory"""
    cfg = json.load(open(os.path.join(path, "config.json")))
    sd = read_state_dict(path)
    spec = MTSpec.from_config(cfg, {k: v.shape for k, v in sd.items()})
    missing = [k for k in layer_names(spec) if k not in sd]
    if missing:
        raise KeyError(f"{path}: missing tensors {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    return spec, {k: sd[k] for k in layer_names(spec)}


@dataclasses.dataclass(frozen=True)
class MTGenOptions:
    num_beams: int = 1
    max_length: int = 20
    early_stopping: object = False         # False | True | "never"
    length_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    forced_eos_token_id: Optional[int] = None

    def early_stopping_code(self) -> int:
        return 2 if self.early_stopping == "never" else (1 if self.early_stopping is True else 0)


# transformers' GenerationConfig defaults of the six options (a bare generate() with neither file setting them)
GEN_DEFAULTS = MTGenOptions()
_GEN_KEYS = ("num_beams", "max_length", "early_stopping", "length_penalty", "no_repeat_ngram_size", "forced_eos_token_id")


def generation_options(model_dir: Optional[str] = None, config: Optional[dict] = None, generation_config: Optional[dict] = None) -> MTGenOptions:
    """The options of a bare ``model.generate(**encoded_input)``: transformers reads ``generation_config.json`` when the checkpoint
    has one (its values over GenerationConfig's defaults) and otherwise takes the generation keys of ``config.json``
    (GenerationConfig.from_model_config). Defaults: num_beams 1, max_length 20, early_stopping False, length_penalty 1.0,
    no_repeat_ngram_size 0, forced_eos_token_id None. A max_length above 448 is refused (the engine's decode cache)."""
    if model_dir is not None:
        gp = os.path.join(model_dir, "generation_config.json")
        cp = os.path.join(model_dir, "config.json")
        if generation_config is None and os.path.isfile(gp):
            generation_config = json.load(open(gp))
        if config is None and os.path.isfile(cp):
            config = json.load(open(cp))
    src = generation_config if generation_config is not None else (config or {})
    vals = {k: src[k] for k in _GEN_KEYS if k in src and src[k] is not None}
    es = vals.get("early_stopping", GEN_DEFAULTS.early_stopping)
    if es not in (True, False, "never"):
        raise ValueError(f"early_stopping {es!r}: expected True, False or 'never'")
    opts = dataclasses.replace(GEN_DEFAULTS, **vals)
    if opts.max_length > MAX_DECODE_LENGTH:
        raise ValueError(f"max_length {opts.max_length} exceeds the translation engine's decode limit of {MAX_DECODE_LENGTH} tokens")
    if opts.num_beams < 1 or opts.num_beams > 16:
        raise ValueError(f"num_beams {opts.num_beams} outside 1..16")
    return opts
