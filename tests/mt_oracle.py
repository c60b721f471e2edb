"""A torch fp32 CPU restatement of M2M100ForConditionalGeneration's forward pass and of transformers' generate() (greedy and
beam search, transformers 5.x generation/utils.py), used to check the HIP translation engine without ``transformers``.
Inputs are the numpy weights of whisperlive_amd.mt_weights (Hugging Face key names)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as Fn

from whisperlive_amd.mt_weights import MTGenOptions, MTSpec


def sinusoidal_table(n: int, d: int, pad: int) -> torch.Tensor:
    half = d // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half, dtype=torch.int64).float() * -emb)
    emb = torch.arange(n, dtype=torch.int64).float().unsqueeze(1) * emb.unsqueeze(0)
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1).view(n, -1)
    emb[pad, :] = 0
    return emb


def positions(ids: Sequence[int], pad: int, past: int = 0) -> List[int]:
    c, out = 0, []
    for t in ids:
        if t != pad:
            c += 1
            out.append(c + past + pad)
        else:
            out.append(pad)
    return out


class M2M100Oracle:
    def __init__(self, spec: MTSpec, w: Dict[str, np.ndarray], fp16_matrices: bool = False):
        self.spec = spec
        cvt = (lambda a: torch.from_numpy(a.astype(np.float16).astype(np.float32))) if fp16_matrices else torch.from_numpy
        self.w = {k: (cvt(v) if v.ndim == 2 else torch.from_numpy(v)) for k, v in w.items()}
        self.pos = sinusoidal_table(spec.max_positions + 2, spec.d_model, spec.pad_id)
        self.scale = math.sqrt(spec.d_model) if spec.scale_embedding else 1.0

    def _ln(self, x, name):
        return Fn.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], 1e-5)

    def _lin(self, x, name):
        return x @ self.w[name + ".weight"].T + self.w[name + ".bias"]

    def _attn(self, xq, xkv, name, causal=False):
        H, hd = self.spec.n_heads, 64
        q = self._lin(xq, name + ".q_proj") * (hd ** -0.5)
        k = self._lin(xkv, name + ".k_proj")
        v = self._lin(xkv, name + ".v_proj")
        T, S = q.shape[0], k.shape[0]
        q = q.view(T, H, hd).transpose(0, 1)
        k = k.view(S, H, hd).transpose(0, 1)
        v = v.view(S, H, hd).transpose(0, 1)
        s = q @ k.transpose(1, 2)
        if causal:
            s = s + torch.triu(torch.full((T, S), float("-inf")), diagonal=1 + S - T)
        o = torch.softmax(s, dim=-1) @ v
        return self._lin(o.transpose(0, 1).reshape(T, H * hd), name + ".out_proj")

    def embed(self, ids: Sequence[int], past: int = 0) -> torch.Tensor:
        e = self.w["model.shared.weight"][torch.tensor(list(ids))] * self.scale
        return e + self.pos[torch.tensor(positions(ids, self.spec.pad_id, past))]

    @torch.no_grad()
    def encode(self, src: Sequence[int]) -> torch.Tensor:
        x = self.embed(src)
        for l in range(self.spec.enc_layers):
            p = f"model.encoder.layers.{l}."
            x = x + self._attn(self._ln(x, p + "self_attn_layer_norm"), self._ln(x, p + "self_attn_layer_norm"), p + "self_attn")
            h = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(torch.relu(self._lin(h, p + "fc1")), p + "fc2")
        return self._ln(x, "model.encoder.layer_norm")

    @torch.no_grad()
    def decode_logits(self, enc: torch.Tensor, dec: Sequence[int]) -> torch.Tensor:
        """teacher-forced logits [len(dec), vocab] (causal self-attention over the whole prefix)"""
        x = self.embed(dec)
        for l in range(self.spec.dec_layers):
            p = f"model.decoder.layers.{l}."
            h = self._ln(x, p + "self_attn_layer_norm")
            x = x + self._attn(h, h, p + "self_attn", causal=True)
            x = x + self._attn(self._ln(x, p + "encoder_attn_layer_norm"), enc, p + "encoder_attn")
            h = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(torch.relu(self._lin(h, p + "fc1")), p + "fc2")
        x = self._ln(x, "model.decoder.layer_norm")
        return x @ self.w["model.shared.weight"].T

    def last_logits(self, enc, dec):
        return self.decode_logits(enc, dec)[-1]

    # ------------------------------------------------------------------ generation
    def _banned(self, seq: List[int], n: int) -> List[int]:
        cur = len(seq)
        if n <= 0 or cur + 1 < n:
            return []
        key = tuple(seq[cur + 1 - n:cur])
        return [seq[a + n - 1] for a in range(cur - n + 1) if tuple(seq[a:a + n - 1]) == key]

    def _process(self, seqs: List[List[int]], scores: torch.Tensor, o: MTGenOptions) -> torch.Tensor:
        scores = scores.clone()
        cur = len(seqs[0])
        for r, s in enumerate(seqs):
            for b in self._banned(s, o.no_repeat_ngram_size):
                scores[r, b] = float("-inf")
        if o.forced_eos_token_id is not None and cur == o.max_length - 1:
            scores[:, :] = float("-inf")
            scores[:, o.forced_eos_token_id] = 0
        return scores

    @torch.no_grad()
    def generate(self, srcs: List[List[int]], o: MTGenOptions, logits_fn=None):
        """-> (list of token lists: generated tokens without the decoder start and the final EOS, list of scores)"""
        encs = [self.encode(s) for s in srcs]
        step = logits_fn or (lambda i, seq: self.last_logits(encs[i], seq))
        if o.num_beams == 1:
            return self._greedy(srcs, o, step)
        return self._beam(srcs, o, step)

    def _greedy(self, srcs, o, step):
        B, eos, pad = len(srcs), self.spec.eos_id, self.spec.pad_id
        seqs = [[self.spec.decoder_start_id] for _ in range(B)]
        done = [False] * B
        score = [0.0] * B
        while True:
            logits = torch.stack([step(i, seqs[i]) for i in range(B)])
            proc = self._process(seqs, logits, o)
            lp = self._process(seqs, torch.log_softmax(logits, -1), o)
            nxt = torch.argmax(proc, dim=-1).tolist()
            for i in range(B):
                if done[i]:
                    seqs[i].append(pad)
                    continue
                score[i] += float(lp[i, nxt[i]])
                seqs[i].append(nxt[i])
                done[i] = nxt[i] == eos
            if all(done) or len(seqs[0]) >= o.max_length:
                break
        out = []
        for i in range(B):
            s = seqs[i][1:]
            if eos in s:
                s = s[:s.index(eos)]
            out.append(s)
        return out, score

    def _beam(self, srcs, o, step):
        B, R, V, ML = len(srcs), o.num_beams, self.spec.vocab, o.max_length
        eos, lp_pen, es = self.spec.eos_id, o.length_penalty, o.early_stopping
        K = 2 * R
        cur_len = 1
        running = torch.full((B, R, ML), self.spec.pad_id, dtype=torch.long)
        running[:, :, 0] = self.spec.decoder_start_id
        sequences = running.clone()
        run_scores = torch.zeros((B, R))
        run_scores[:, 1:] = -1e9
        beam_scores = torch.full((B, R), -1e9)
        fin = torch.zeros((B, R), dtype=torch.bool)
        unsat = torch.ones((B, 1), dtype=torch.bool)
        top_mask = torch.cat([torch.ones(R, dtype=torch.bool), torch.zeros(K - R, dtype=torch.bool)])
        while True:
            flat = [running[b, r, :cur_len].tolist() for b in range(B) for r in range(R)]
            logits = torch.stack([step(i // R, flat[i]) for i in range(B * R)])
            lp = self._process(flat, torch.log_softmax(logits, -1), o).view(B, R, V)
            lp = (lp + run_scores[:, :, None]).reshape(B, R * V)
            tv, ti = torch.topk(lp, K)
            beam = ti // V
            tok = ti % V
            tseq = torch.take_along_dim(running, beam[:, :, None], dim=1).clone()
            tseq[:, :, cur_len] = tok
            hits = (tok == eos) | (cur_len + 1 >= ML)
            rv = tv + hits.float() * -1e9
            nidx = torch.topk(rv, R)[1]
            running = torch.take_along_dim(tseq, nidx[:, :, None], dim=1)
            run_scores = torch.take_along_dim(rv, nidx, dim=1)
            just = hits & top_mask[None, :]
            fv = tv / ((cur_len + 1 - 1) ** lp_pen)
            full = torch.all(fin, dim=-1, keepdim=True) & (es is True)
            fv = fv + full.float() * -1e9
            fv = fv + (~unsat).float() * -1e9
            fv = fv + (~just).float() * -1e9
            ms = torch.cat([beam_scores, fv], 1)
            mseq = torch.cat([sequences, tseq], 1)
            mfin = torch.cat([fin, just], 1)
            mi = torch.topk(ms, R)[1]
            sequences = torch.take_along_dim(mseq, mi[:, :, None], dim=1)
            beam_scores = torch.take_along_dim(ms, mi, dim=1)
            fin = torch.take_along_dim(mfin, mi, dim=1)
            cur_len += 1
            best_len = (ML - 1) if (es == "never" and lp_pen > 0.0) else (cur_len - 1)
            best = run_scores[:, :1] / (best_len ** lp_pen)
            worst = torch.where(fin, torch.min(beam_scores, dim=1, keepdim=True)[0], -1.0e9)
            unsat = unsat & torch.any(best > worst, dim=-1, keepdim=True)
            go = bool(torch.any(unsat)) and not (bool(torch.all(fin)) and es is True) and not bool(torch.all(hits))
            if not go or cur_len >= ML:
                break
        out, scores = [], []
        for b in range(B):
            s = sequences[b, 0, 1:].tolist()
            if eos in s:
                s = s[:s.index(eos)]
            else:
                s = [t for t in s]
                while s and s[-1] == self.spec.pad_id:
                    s.pop()
            out.append(s)
            scores.append(float(beam_scores[b, 0]))
        return out, scores
