"""Weights of the speaker-embedding network (WeSpeaker ResNet34, `pyannote/wespeaker-voxceleb-resnet34-LM`).

* ``SpkSpec``          — depth / width / front-end fields of the network (include/wlx.h wlx_spk_spec).
* ``read_state_dict``  — a ``.safetensors`` file, or a torch file holding a plain state dict or one nested under ``state_dict`` (a
                         Lightning checkpoint, which is what pyannote publishes as ``pytorch_model.bin``), as float32 numpy under
                         WeSpeaker names without the ``resnet.`` prefix. Torch files are read with ``weights_only=True``; where that
                         refuses a checkpoint for the foreign objects it carries, a restricted unpickler reads the tensors and turns
                         every other global into an inert placeholder. No pickled code is ever executed.
* ``fold``             — BatchNorm (eval mode) folded into each convolution in float32 numpy, weights then rounded to fp16 (kept in
                         float32 arrays). These tensors are what crosses the C-ABI, and what a test oracle runs on.
* ``random_weights``   — a seeded, unfolded state dict for tests: no checkpoint of this network ships with the repository.
"""
from __future__ import annotations

import os
import pickle
import zipfile
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

BN_EPS = 1e-5          # torch.nn.BatchNorm2d default, which WeSpeaker's ResNet keeps


@dataclass(frozen=True)
class SpkSpec:
    n_mels: int = 80
    planes: int = 32
    blocks: Tuple[int, int, int, int] = (3, 4, 6, 3)
    embed_dim: int = 256
    max_seconds: int = 45
    pool_eps: float = 1e-7      # WeSpeaker's TSTP: sqrt(var + 1e-7). UNPINNED: pyannote's own StatsPool has no epsilon

    @property
    def pool_dim(self) -> int:
        return 2 * (self.planes * 8) * (self.n_mels // 8)

    def convs(self):
        """(name, cout, cin, ksize, stride, bn name) of every convolution, in execution order"""
        out = [("conv1", self.planes, 1, 3, 1, "bn1")]
        cin = self.planes
        for L in range(4):
            planes = self.planes << L
            for b in range(self.blocks[L]):
                stride = 2 if (b == 0 and L > 0) else 1
                p = f"layer{L + 1}.{b}."
                out.append((p + "conv1", planes, cin, 3, stride, p + "bn1"))
                out.append((p + "conv2", planes, planes, 3, 1, p + "bn2"))
                if stride != 1 or cin != planes:
                    out.append((p + "shortcut.0", planes, cin, 1, stride, p + "shortcut.1"))
                cin = planes
        return out


RESNET34 = SpkSpec()


def state_shapes(spec: SpkSpec) -> Dict[str, tuple]:
    """every tensor an unfolded state dict must hold, with its shape"""
    out: Dict[str, tuple] = {}
    for name, cout, cin, ks, _, bn in spec.convs():
        out[name + ".weight"] = (cout, cin, ks, ks)
        for f in ("weight", "bias", "running_mean", "running_var"):
            out[f"{bn}.{f}"] = (cout,)
    out["seg_1.weight"] = (spec.embed_dim, spec.pool_dim)
    out["seg_1.bias"] = (spec.embed_dim,)
    return out


def spec_from_state(sd: Dict[str, np.ndarray], **kw) -> SpkSpec:
    """depth and width read off the tensors (blocks per stage, stem channels, embedding size)"""
    if "conv1.weight" not in sd:
        raise KeyError("speaker weights: missing tensor 'conv1.weight'")
    if "seg_1.weight" not in sd:
        raise KeyError("speaker weights: missing tensor 'seg_1.weight'")
    planes = int(sd["conv1.weight"].shape[0])
    blocks = []
    for L in range(1, 5):
        n = 0
        while f"layer{L}.{n}.conv1.weight" in sd:
            n += 1
        if n == 0:
            raise KeyError(f"speaker weights: missing tensor 'layer{L}.0.conv1.weight'")
        blocks.append(n)
    embed, pool_dim = (int(v) for v in sd["seg_1.weight"].shape)
    n_mels = pool_dim // (2 * planes)
    return SpkSpec(n_mels=n_mels, planes=planes, blocks=tuple(blocks), embed_dim=embed, **kw)


def _strip(sd) -> Dict[str, np.ndarray]:
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.startswith("model."):
            k = k[len("model."):]
        if k.startswith("resnet."):
            k = k[len("resnet."):]
        if hasattr(v, "detach"):
            v = v.detach().to("cpu").float().numpy()
        if isinstance(v, np.ndarray):
            out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


class _Inert:
    """stands in for any global a checkpoint names that is not part of torch's tensor rebuilding: constructible, settable, inert"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self

    def __setstate__(self, state):
        pass


def _restricted_load(path: str):
    """torch's zip checkpoint format read with an unpickler that knows tensors, storages and plain containers only"""
    import torch

    dtypes = {"FloatStorage": torch.float32, "HalfStorage": torch.float16, "BFloat16Storage": torch.bfloat16,
              "DoubleStorage": torch.float64, "LongStorage": torch.int64, "IntStorage": torch.int32, "BoolStorage": torch.bool,
              "ByteStorage": torch.uint8, "ShortStorage": torch.int16, "CharStorage": torch.int8}
    with zipfile.ZipFile(path) as zf:
        names = zf.namelist()
        pkl = next(n for n in names if n.endswith("/data.pkl") or n == "data.pkl")
        root = pkl[:-len("data.pkl")]

        def rebuild(storage, offset, size, stride, *_):
            return torch.as_strided(storage, tuple(size), tuple(stride), offset).clone()

        class U(pickle.Unpickler):
            def find_class(self, module, name):
                if module == "torch._utils" and name in ("_rebuild_tensor_v2", "_rebuild_tensor"):
                    return rebuild
                if module == "torch._utils" and name == "_rebuild_parameter":
                    return lambda data, *_: data             # a Parameter is kept as its tensor
                if module == "torch" and name in dtypes:
                    return dtypes[name]
                if module == "collections" and name == "OrderedDict":
                    import collections
                    return collections.OrderedDict
                return _Inert

            def persistent_load(self, pid):
                _, dtype, key, _, numel = pid[:5]
                if not isinstance(dtype, torch.dtype):
                    return torch.zeros(0)
                raw = zf.read(f"{root}data/{key}")
                return torch.frombuffer(bytearray(raw), dtype=dtype)[:numel]

        return U(zf.open(pkl)).load()


def read_state_dict(path: str) -> Dict[str, np.ndarray]:
    path = os.path.expanduser(path)
    if os.path.isdir(path):
        for f in ("model.safetensors", "pytorch_model.bin", "avg_model.pt", "model.pt"):
            if os.path.isfile(os.path.join(path, f)):
                path = os.path.join(path, f)
                break
        else:
            raise FileNotFoundError(f"{path}: no model.safetensors / pytorch_model.bin / avg_model.pt")
    if path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return _strip(load_file(path))
    import torch
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        obj = _restricted_load(path)
    if isinstance(obj, dict) and isinstance(obj.get("state_dict"), dict):
        obj = obj["state_dict"]
    if not isinstance(obj, dict):
        raise ValueError(f"{path}: not a state dict")
    return _strip(obj)


def check_state(sd: Dict[str, np.ndarray], spec: SpkSpec) -> None:
    for name, shape in state_shapes(spec).items():
        if name not in sd:
            raise KeyError(f"speaker weights: missing tensor '{name}'")
        if tuple(sd[name].shape) != shape:
            raise ValueError(f"speaker weights: tensor '{name}' has shape {tuple(sd[name].shape)}, expected {shape}")


def fold(sd: Dict[str, np.ndarray], spec: SpkSpec, round_fp16: bool = True) -> Dict[str, np.ndarray]:
    """conv + BatchNorm(eval) -> conv with bias: w' = w * g / sqrt(var + eps), b' = beta - mean * g / sqrt(var + eps), float32.
    The shortcut's two members become "<block>.shortcut.weight" / ".bias". Weights (not biases) are then rounded to fp16."""
    check_state(sd, spec)
    r16 = (lambda a: a.astype(np.float16).astype(np.float32)) if round_fp16 else (lambda a: a)
    out: Dict[str, np.ndarray] = {}
    for name, _, _, _, _, bn in spec.convs():
        w = sd[name + ".weight"].astype(np.float32)
        scale = sd[bn + ".weight"].astype(np.float32) / np.sqrt(sd[bn + ".running_var"].astype(np.float32) + np.float32(BN_EPS))
        dst = name[:-2] if name.endswith("shortcut.0") else name
        out[dst + ".weight"] = r16(np.ascontiguousarray(w * scale[:, None, None, None], dtype=np.float32))
        out[dst + ".bias"] = (sd[bn + ".bias"].astype(np.float32) - sd[bn + ".running_mean"].astype(np.float32) * scale).astype(np.float32)
    out["seg_1.weight"] = r16(sd["seg_1.weight"].astype(np.float32))
    out["seg_1.bias"] = sd["seg_1.bias"].astype(np.float32)
    return out


def load(path: str, **kw) -> Tuple[SpkSpec, Dict[str, np.ndarray]]:
    """(spec, folded tensors) of a checkpoint file or directory"""
    sd = read_state_dict(path)
    spec = spec_from_state(sd, **kw)
    return spec, fold(sd, spec)


def random_weights(spec: SpkSpec = RESNET34, seed: int = 0) -> Dict[str, np.ndarray]:
    """a seeded UNFOLDED state dict (He-scaled convolutions, BatchNorm statistics away from the identity) that keeps activations of
    order one through the depth, so an fp16 pipeline is exercised in its normal range"""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for name, cout, cin, ks, _, bn in spec.convs():
        fan = cin * ks * ks
        gain = 1.0 if name.endswith(("conv2", "shortcut.0")) else np.sqrt(2.0)
        sd[name + ".weight"] = (rng.standard_normal((cout, cin, ks, ks)) * gain / np.sqrt(fan)).astype(np.float32)
        sd[bn + ".weight"] = rng.uniform(0.6, 1.0, cout).astype(np.float32)
        sd[bn + ".bias"] = (0.2 * rng.standard_normal(cout)).astype(np.float32)
        sd[bn + ".running_mean"] = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        sd[bn + ".running_var"] = rng.uniform(0.8, 1.3, cout).astype(np.float32)
    sd["seg_1.weight"] = (rng.standard_normal((spec.embed_dim, spec.pool_dim)) / np.sqrt(spec.pool_dim)).astype(np.float32)
    sd["seg_1.bias"] = (0.05 * rng.standard_normal(spec.embed_dim)).astype(np.float32)
    return sd
