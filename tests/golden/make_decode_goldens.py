#!/usr/bin/env python
"""Goldens that pin the HOST ORCHESTRATION of the Whisper decode (csrc/engine_decode.hip) to what the commit before a host-side
change did on the same MI355X — the library's own earlier answer, so equality is exact and no tolerance is involved:

  decode_step_launches.json   per family model (tests/test_gpu_lean_family.py FAMILY) and row count, the launch table of one decode
                              step as wlx_debug_profile_step lists it: {kernel name: [launches per step, algorithmic bytes per launch]}.
                              The row counts (STEP_ROWS, on a 12 x 5 slot) are the smallest that reach each branch of decoder_pass:
                              1; 5 (folded embedding, K-split MLP, fused query + cross attention where the shape is eligible); 16 (the last
                              single-tile shape); 20 (the first batched shape: combine launch, no K-split, separate embedding); 50 (the
                              first allowed count above 48: fused cross attention off); 60 (the slot's largest).
  generate_routes.json        tokens, float32 score bits and no_speech_prob bits of one `generate` call per prompt-prefill route
                              (route_calls). Models: tests/golden/trained_tiny, as a whole transcribing checkpoint — its d_model of 128 is
                              outside the lean kernels, so its long and batched prompts all take the chunked per-item prefill — and the
                              seeded `base-like` family member (d_model 512), on which the same calls select the one-pass and the joint prefill.

Run on the GPU with the library built from the commit the change starts from:
    python tests/golden/make_decode_goldens.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_SLOT = (12, 5)                      # items x rows per item of the slot the step tables are taken on
STEP_ROWS = (1, 5, 16, 20, 50, 60)
TRAINED_DIR = os.path.join(HERE, "trained_tiny")
ROUTE_MODELS = ("trained_tiny", "base-like")
BASE_LIKE = (80, 512, 8, 1, 2, 2048, 20000)     # (n_mels, d_model, heads, enc_layers, dec_layers, ffn, vocab): tests/test_gpu_lean_family.py FAMILY["base-like"]


def step_launch_table(slot, rows: int) -> dict:
    """{kernel name: [launches per step, bytes per launch]} of one decode step of `rows` rows at position 4"""
    return {k["name"]: [k["launches"], k["bytes_per_launch"]] for k in slot.debug_profile_step(rows, 4, 1)}


def step_launch_tables(eng, pcm) -> dict:
    """the tables of every STEP_ROWS row count, on a slot of its own on `eng` (closed again)"""
    slot = eng.create_slot(*STEP_SLOT)
    try:
        T = slot.logmel(pcm)
        slot.encode(1, seek=[0], seg=[T - 1])
        return {str(r): step_launch_table(slot, r) for r in STEP_ROWS}
    finally:
        slot.close()


def route_engine(model: str):
    """(engine, spec, three clips) of a ROUTE_MODELS member"""
    from whisperlive_amd.engine import HipWhisperEngine
    if model == "trained_tiny":
        from tests.golden.make_trained_tiny import utterance
        from whisperlive_amd.specs import spec_from_state_dict
        from whisperlive_amd.weights import load_model_dir
        sd = load_model_dir(TRAINED_DIR)
        spec = spec_from_state_dict(sd)
        with open(os.path.join(TRAINED_DIR, "expected.json")) as f:
            seeds = [c["seed"] for c in json.load(f)["cases"][:3]]
        return HipWhisperEngine(spec, sd), spec, [utterance(s)[0][: 16000 * 8] for s in seeds]
    from oracle import logmel as olm
    from whisperlive_amd.specs import WhisperSpec
    from whisperlive_amd.weights import random_weights
    n_mels, d, h, le, ld, f, v = BASE_LIKE
    spec = WhisperSpec(n_mels=n_mels, d_model=d, n_heads=h, enc_layers=le, dec_layers=ld, ffn=f, vocab=v)
    return HipWhisperEngine(spec, random_weights(spec, seed=11)), spec, [olm.speech_like_pcm(3.0 + 0.5 * i, seed=700 + i) for i in range(3)]


def route_calls(ids, vocab: int):
    """[(route, prompts, environment, generate keywords)]: the smallest prompts that select each prefill route of wlx_generate.
    A prompt's LAST token is the first decode step's input, so the prefill sees len(prompt) - 1 rows: the long prompt has 50 tokens =
    49 prefill rows, the first count past the 48-row chunk (one-pass prefill; with WLX_PREFILL_ONE_PASS=0 two chunks of 48 + 1)."""
    rng = np.random.default_rng(9)
    text = [int(t) for t in rng.integers(300, min(vocab, ids.eot) - 200, size=46)]
    lang, task = ids.sot + 1, ids.timestamp_begin - 5
    long_prompt = [ids.timestamp_begin - 3] + text + [ids.sot, lang, task]          # <|startofprev|> text <|sot|> lang task: sot not last
    short = [[ids.sot, lang, task], [ids.sot, lang + 2, task], [ids.sot, lang + 1, task]]
    assert len(long_prompt) == 50
    beam = dict(beam_size=5, patience=1.0)
    return [
        ("no prefill", [[ids.sot]], {}, beam),
        ("one-pass prefill", [long_prompt], {}, beam),
        ("chunked prefill", [long_prompt], {"WLX_PREFILL_ONE_PASS": "0"}, beam),
        ("joint prefill", short, {}, beam),
        ("per-item prefill in a batch", [long_prompt, short[0]], {}, beam),
        ("sampling", [[ids.sot]], {}, dict(beam_size=1)),
    ]


def run_routes(model: str) -> list:
    """one record per route_calls entry: tokens, float32 score bit patterns and no_speech_prob bit patterns of every item"""
    from tests import helpers as H
    eng, spec, clips = route_engine(model)
    slot = eng.create_slot(3, 5)
    try:
        ids = H.token_ids_for(spec.vocab)
        Ts = [slot.logmel(c, item=i) for i, c in enumerate(clips)]
        slot.encode(3, seek=[0] * 3, seg=[t - 1 for t in Ts])
        bits = lambda x: int(np.float32(x).view(np.uint32))
        out = []
        for route, prompts, env, kw in route_calls(ids, spec.vocab):
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                res = slot.generate(prompts, H.engine_ids(ids), max_length=max(len(p) for p in prompts) + 12,
                                    suppress_tokens=H.default_suppress(ids), **kw)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k)
                    else:
                        os.environ[k] = v
            out.append(dict(route=route, tokens=[r.sequences_ids[0] for r in res], score_bits=[bits(r.scores[0]) for r in res],
                            no_speech_bits=[bits(r.no_speech_prob) for r in res]))
        return out
    finally:
        slot.close()
        eng.close()


def main():
    from oracle import logmel as olm
    from tests.test_gpu_lean_family import FAMILY        # (only when run as a script: the test modules import this one, not the reverse)
    assert FAMILY["base-like"] == BASE_LIKE
    from whisperlive_amd.engine import HipWhisperEngine
    from whisperlive_amd.specs import WhisperSpec
    from whisperlive_amd.weights import random_weights
    steps = {}
    for name, (n_mels, d, h, le, ld, f, v) in FAMILY.items():
        spec = WhisperSpec(n_mels=n_mels, d_model=d, n_heads=h, enc_layers=le, dec_layers=ld, ffn=f, vocab=v)
        eng = HipWhisperEngine(spec, random_weights(spec, seed=11))
        try:
            steps[name] = step_launch_tables(eng, olm.speech_like_pcm(5.0, seed=21))
        finally:
            eng.close()
        print(name, {r: len(t) for r, t in steps[name].items()})
    routes = {m: run_routes(m) for m in ROUTE_MODELS}
    for m, recs in routes.items():
        for r in recs:
            print(m, r["route"], [len(t) for t in r["tokens"]], r["score_bits"], r["no_speech_bits"])
    for fn, obj in (("decode_step_launches.json", steps), ("generate_routes.json", routes)):
        with open(os.path.join(HERE, fn), "w") as f:
            json.dump(obj, f, indent=0, separators=(",", ":"), sort_keys=True)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
