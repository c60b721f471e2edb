"""CPU restatements for the speaker-embedding engine (whisperlive_amd/csrc/spk.hip). BOTH ARE UNPINNED: neither torchaudio nor
pyannote.audio nor a WeSpeaker checkpoint is available to compare against, so they are written from the published definitions
and pin the engine to those, not to a reference run.

* ``fbank`` / ``features`` — float64 restatement of Kaldi's `fbank` as pyannote's WeSpeaker wrapper calls it
  (torchaudio.compliance.kaldi.fbank: num_mel_bins 80, frame_length 25, frame_shift 10, dither 0, hamming window, snip_edges,
  remove_dc_offset, preemphasis 0.97, power spectrum of a 512-point FFT, triangular bins over 20 Hz .. Nyquist on the
  1127 ln(1 + f / 700) scale without the Nyquist bin, log with a float32-epsilon floor, no energy; waveform scaled by 2^15), and
  the wrapper's subtraction of the per-bin mean over the frames.
* ``UnfoldedResNet`` — torch restatement of WeSpeaker's ResNet (3 x 3 stem + BatchNorm + ReLU, four stages of BasicBlocks with
  1 x 1 stride-s shortcuts, TSTP statistics pooling, one Linear), BatchNorm UNFOLDED, for checking the fold.
* ``folded_forward`` — the same network on the FOLDED tensors that cross the C-ABI (spk_weights.fold), fp32, optionally with every
  activation rounded to fp16 where the engine stores one: the fp16 pipeline emulated on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

FRAME, SHIFT, NFFT = 400, 160, 512
EPS32 = float(np.finfo(np.float32).eps)


def n_frames(n: int) -> int:
    return 0 if n < FRAME else 1 + (n - FRAME) // SHIFT


def mel_banks(n_mels: int = 80, lo_hz: float = 20.0, hi_hz: float = 8000.0, sr: int = 16000) -> np.ndarray:
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    lo, hi = mel(lo_hz), mel(hi_hz)
    delta = (hi - lo) / (n_mels + 1)
    left = lo + delta * np.arange(n_mels)[:, None]
    centre, right = left + delta, left + 2 * delta
    m = mel(sr / NFFT * np.arange(NFFT // 2))[None, :]
    return np.maximum(0.0, np.minimum((m - left) / (centre - left), (right - m) / (right - centre)))      # [n_mels][256]


def windowed_frames(pcm: np.ndarray) -> np.ndarray:
    """[T][400] float64: scaled, DC removed, pre-emphasised, Hamming-windowed"""
    x = np.asarray(pcm, dtype=np.float64) * 32768.0
    T = n_frames(len(x))
    fr = x[np.arange(T)[:, None] * SHIFT + np.arange(FRAME)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr - 0.97 * prev
    return fr * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(FRAME) / (FRAME - 1)))[None, :]


def fbank(pcm: np.ndarray, n_mels: int = 80, dtype=np.float64) -> np.ndarray:
    """log-mel [T][n_mels] before the mean subtraction. dtype float32 runs the DFT and mel stages in float32 (a restatement of an
    fp32 implementation, for measuring what fp32 costs against float64)."""
    fr = windowed_frames(pcm).astype(dtype)
    if dtype == np.float64:
        spec = np.fft.rfft(fr, n=NFFT, axis=1)[:, :NFFT // 2]
        power = spec.real ** 2 + spec.imag ** 2
    else:
        k = np.arange(NFFT // 2)[:, None] * np.arange(FRAME)[None, :] % NFFT
        ang = 2.0 * np.pi * k / NFFT
        re = fr @ np.cos(ang).astype(dtype).T
        im = fr @ np.sin(ang).astype(dtype).T
        power = re * re + im * im
    e = power @ mel_banks(n_mels).astype(dtype).T
    return np.log(np.maximum(e, dtype(EPS32)))


def features(pcm: np.ndarray, n_mels: int = 80) -> np.ndarray:
    f = fbank(pcm, n_mels)
    return f - f.mean(axis=0, keepdims=True)


# ------------------------------------------------------------------------------------------------ network
class _Block(torch.nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(planes)
        self.conv2 = torch.nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(planes)
        self.shortcut = torch.nn.Sequential()
        if stride != 1 or cin != planes:
            self.shortcut = torch.nn.Sequential(torch.nn.Conv2d(cin, planes, 1, stride, bias=False), torch.nn.BatchNorm2d(planes))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + self.shortcut(x))


class UnfoldedResNet(torch.nn.Module):
    """state-dict names as WeSpeaker's (without the `resnet.` prefix of pyannote's wrapper)"""

    def __init__(self, spec):
        super().__init__()
        m = spec.planes
        self.spec = spec
        self.conv1 = torch.nn.Conv2d(1, m, 3, 1, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(m)
        cin = m
        for L in range(4):
            blocks = []
            for b in range(spec.blocks[L]):
                blocks.append(_Block(cin, m << L, 2 if (b == 0 and L > 0) else 1))
                cin = m << L
            setattr(self, f"layer{L + 1}", torch.nn.Sequential(*blocks))
        self.seg_1 = torch.nn.Linear(spec.pool_dim, spec.embed_dim)

    def forward(self, feats):          # feats [T][n_mels]
        x = feats.t()[None, None]      # (1, 1, F, T)
        x = F.relu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = x.reshape(1, -1, x.shape[-1])
        stats = torch.cat([x.mean(-1), torch.sqrt(x.var(-1, unbiased=True) + self.spec.pool_eps)], dim=-1)
        return self.seg_1(stats)[0]


def unfolded(spec, sd) -> UnfoldedResNet:
    net = UnfoldedResNet(spec)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return net.eval()


def folded_forward(spec, w, feats: np.ndarray, fp16_activations: bool = False) -> np.ndarray:
    """unnormalised embedding [embed_dim] of feats [T][n_mels] on the folded tensors `w` (float32 torch). With
    fp16_activations the input image and the output of every convolution (after bias, residual and ReLU) are rounded to fp16,
    which is where the engine stores fp16; pooling and the head stay fp32 as in the engine."""
    r = (lambda t: t.half().float()) if fp16_activations else (lambda t: t)
    W = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()}
    with torch.no_grad():
        x = r(torch.from_numpy(np.asarray(feats, dtype=np.float32)).t()[None, None].contiguous())
        x = r(F.relu(F.conv2d(x, W["conv1.weight"], W["conv1.bias"], 1, 1)))
        cin = spec.planes
        for L in range(4):
            planes = spec.planes << L
            for b in range(spec.blocks[L]):
                s = 2 if (b == 0 and L > 0) else 1
                p = f"layer{L + 1}.{b}."
                t = r(F.relu(F.conv2d(x, W[p + "conv1.weight"], W[p + "conv1.bias"], s, 1)))
                sc = x
                if s != 1 or cin != planes:
                    sc = r(F.conv2d(x, W[p + "shortcut.weight"], W[p + "shortcut.bias"], s, 0))
                x = r(F.relu(F.conv2d(t, W[p + "conv2.weight"], W[p + "conv2.bias"], 1, 1) + sc))
                cin = planes
        x = x.reshape(1, -1, x.shape[-1])
        stats = torch.cat([x.mean(-1), torch.sqrt(x.var(-1, unbiased=True) + spec.pool_eps)], dim=-1)
        return F.linear(stats, W["seg_1.weight"], W["seg_1.bias"])[0].numpy()


def embed(spec, w, pcm: np.ndarray, fp16_activations: bool = False) -> np.ndarray:
    """L2-normalised oracle embedding of 16 kHz PCM"""
    e = folded_forward(spec, w, features(pcm, spec.n_mels), fp16_activations).astype(np.float64)
    return (e / np.linalg.norm(e)).astype(np.float32)


def rel_rms(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))
