"""Oracle-side helpers for linear biases and traditional RoPE (not a test; the oracle package itself is left as it is).

Numerics of a biased linear (from MLX's published behaviour):
  * dense ``nn.Linear``:      ``mx.addmm(bias, x, W.T)`` -- the bias joins the float32 accumulator, ONE rounding: T(acc + b);
  * ``nn.QuantizedLinear``:   ``quantized_matmul(...)`` then ``x + bias`` -- TWO roundings: T(T(acc) + b);
  * float32 activations (PagedKVCache mode after layer 0): T = float32, b is added in float32;
  * ``LoRALinear`` wraps the biased linear: y = T(acc + b) first, then y = T(y + T(z)).
``rope_traditional=True`` rotates the pairs (2i, 2i+1) of a head by pos * scale * theta^(-2i/D): the per-head permutation
``head_perm`` turns it into the half-split rotation of ``oracle.ref_model.rope``; q.k is unchanged when q and k are permuted
alike, so the oracle on the permuted checkpoint IS the traditional model's oracle.
"""
from __future__ import annotations

import glob
import json
import shutil
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Optional

import numpy as np

from oracle import numerics, ref_generate
from oracle.numerics import matmul_nt, round_to
from oracle.ref_model import Linear, RefModel, promote


@dataclass
class BiasedLinear(Linear):
    """nn.Linear(bias=True) / nn.QuantizedLinear(bias=True) (llama.py:59-67,155-162)."""
    bias: Optional[np.ndarray] = None          # (N,) float32 values of the checkpoint's `.bias`

    @classmethod
    def wrap(cls, lin: Linear, bias: np.ndarray) -> "BiasedLinear":
        return cls(**{f.name: getattr(lin, f.name) for f in fields(Linear)}, bias=np.asarray(bias, dtype=np.float32))

    @property
    def quantised(self) -> bool:
        return self.weight is None and self.w16 is None

    def __call__(self, x: np.ndarray, xdt: str):
        odt = promote(xdt, self.dtype)
        if numerics.X_SPLIT2 and xdt == "float32" and self.dtype != "float32" and x.size // x.shape[-1] > 16:
            x = numerics.split2(x, self.dtype)
        acc = self._matmul(x)                                     # float32: the exactly summed product, rounded once
        y = biased(acc, self.bias, odt, self.quantised)
        if self.lora_a is not None:                               # LoRALinear around the biased linear (App. A.6)
            zdt = promote(xdt, self.lora_dtype)
            z = round_to(matmul_nt(x, self.lora_a.T), zdt)
            z = round_to(matmul_nt(z, self.lora_b.T), zdt)
            z = round_to(np.float32(self.lora_scale) * z, zdt)
            z = round_to(z, xdt)
            odt2 = promote(odt, xdt)
            y = round_to(y + z, odt2)
            odt = odt2
        return y, odt


def biased(acc: np.ndarray, bias: Optional[np.ndarray], odt: str, quantised: bool) -> np.ndarray:
    """float32 accumulator + bias -> array of dtype ``odt``: one rounding (dense) or two (quantised)."""
    acc = np.asarray(acc, dtype=np.float32)
    if bias is None:
        return round_to(acc, odt)
    b = np.asarray(bias, dtype=np.float32)
    if quantised:
        return round_to(round_to(acc, odt) + b, odt)
    return round_to(acc + b, odt)                                 # (a float32 add: numpy keeps float32 + float32 in float32)


def load(model_dir: str, adapter_path: Optional[str] = None, max_pos: int = 4096) -> RefModel:
    """``ref_generate.load`` + the `.bias` tensors its loader ignores, swapped in as BiasedLinear."""
    model = ref_generate.load(model_dir, adapter_path=adapter_path, max_pos=max_pos)
    for f in sorted(glob.glob(str(Path(model_dir) / "model*.safetensors"))):
        for name, (arr, _dt) in ref_generate._load_safetensors(f).items():
            if name.endswith(".bias") and arr.ndim == 1:
                base = name[: -len(".bias")]
                model.w[base] = BiasedLinear.wrap(model.w[base], arr)
    return model


def head_perm(D: int) -> np.ndarray:
    """pi with new[j] = old[pi[j]]: new[j] = old[2j], new[D/2 + j] = old[2j + 1] for j < D/2."""
    return np.concatenate([np.arange(0, D, 2), np.arange(1, D, 2)])


def rows_perm(n_heads: int, D: int) -> np.ndarray:
    return (np.arange(n_heads)[:, None] * D + head_perm(D)[None, :]).reshape(-1)


def permuted_checkpoint(src: str, dst: str, adapter_src: Optional[str] = None, adapter_dst: Optional[str] = None) -> dict:
    """The pi-permuted copy of a checkpoint directory, with ``rope_traditional`` cleared: rows of the q / k weights
    (dense, or codes + scales + quantisation biases), their linear biases, and the columns of a LoRA B on q_proj / k_proj."""
    import torch
    from safetensors.torch import load_file, save_file

    src_p, dst_p = Path(src), Path(dst)
    dst_p.mkdir(parents=True, exist_ok=True)
    cfg = json.loads((src_p / "config.json").read_text())
    nh = cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D = cfg.get("head_dim") or cfg["hidden_size"] // nh
    idx = {"q_proj": torch.from_numpy(rows_perm(nh, D)), "k_proj": torch.from_numpy(rows_perm(nkv, D))}

    def take(t, rows):                         # (torch cannot index uint32 tensors: go through their int32 view)
        if t.dtype == torch.uint32:
            return t.view(torch.int32)[rows].contiguous().view(torch.uint32)
        return t[rows].contiguous()

    def which(name: str):
        for proj in idx:
            if f".self_attn.{proj}." in name:
                return proj
        return None

    for f in sorted(glob.glob(str(src_p / "model*.safetensors"))):
        w = {}
        for name, t in load_file(f).items():
            proj = which(name)
            w[name] = take(t, idx[proj]) if proj is not None else t.contiguous()
        save_file(w, str(dst_p / Path(f).name), metadata={"format": "mlx"})
    for f in src_p.iterdir():
        if f.is_file() and not f.name.endswith(".safetensors") and f.name != "config.json":
            shutil.copy(f, dst_p / f.name)
    out = dict(cfg)
    out["rope_traditional"] = False
    (dst_p / "config.json").write_text(json.dumps(out, indent=4, sort_keys=True))
    if adapter_src is not None:
        a_src, a_dst = Path(adapter_src), Path(adapter_dst)
        a_dst.mkdir(parents=True, exist_ok=True)
        w = {}
        for name, t in load_file(str(a_src / "adapters.safetensors")).items():
            proj = which(name)
            w[name] = t[:, idx[proj]].contiguous() if (proj is not None and name.endswith(".lora_b")) else t.contiguous()
        save_file(w, str(a_dst / "adapters.safetensors"))
        shutil.copy(a_src / "adapter_config.json", a_dst / "adapter_config.json")
    return out
