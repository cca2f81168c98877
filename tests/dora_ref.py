"""Oracle-side twin of a DoRA-adapted linear (not a test; the oracle package itself is left as it is).

``DoraLinear`` is ``oracle.ref_model.Linear`` with mlx-lm's ``DoRALinear`` on top, restated from its published formula (mlx-lm
is not among the reference's sources, so nothing here was run against it).  W (N, K) in the model dtype, A (K, r), B (r, N),
m (N,) float32, s the scale, T the dtype of x in the call:

    y   = T(x W^T)                                  the base linear
    out = T(y + T(s (x A) B))                       the LoRA term: Linear.__call__, unchanged
    g   = float32(m / ||float32(W) + (s B^T) A^T||_2 per row)      float64 norms, ONE rounding to float32
    out = T(T(g) * out)

``apply_adapters_dora`` reads an adapter directory with either config spelling (``"fine_tune_type": "dora"`` or the older
``"use_dora": true``) and leaves a plain LoRA directory to ``ref_generate.apply_adapters``.  ``load`` follows ``moe_ref.load``
and serves ``rope_traditional`` by regrouping rows, B's columns and m.  ``near_boundary`` tells a test whether a gain sits
so close to a rounding boundary of a dtype that an error of ``rel`` in it could change T(g).
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np

from biased_ref import rows_perm
from oracle import ref_generate
from oracle.numerics import round_to
from oracle.ref_model import Linear, RefConfig, RefModel

_plain_load = ref_generate.load


def exact_gain(weight: np.ndarray, a: np.ndarray, b: np.ndarray, m: np.ndarray, scale: float) -> np.ndarray:
    """m / ||W + s B^T A^T|| per row, in float64 (the float32 product s * B is NOT taken first: this is the formula)."""
    adapted = weight.astype(np.float64) + float(scale) * (b.astype(np.float64).T @ a.astype(np.float64).T)
    return m.astype(np.float64) / np.sqrt((adapted * adapted).sum(axis=1))


def condition(weight: np.ndarray, a: np.ndarray, b: np.ndarray, scale: float) -> float:
    """|| |W| + |s B^T| |A^T| || / || W + s B^T A^T ||, the largest over the rows: how much cancellation between W and the
    low-rank term amplifies a rounding error of the rank-r sum (1 when there is none)."""
    w64 = weight.astype(np.float64)
    delta = float(scale) * (b.astype(np.float64).T @ a.astype(np.float64).T)
    mag = np.abs(w64) + abs(float(scale)) * (np.abs(b.astype(np.float64)).T @ np.abs(a.astype(np.float64)).T)
    return float(np.max(np.sqrt((mag * mag).sum(axis=1)) / np.sqrt(((w64 + delta) ** 2).sum(axis=1))))


@dataclass
class DoraLinear(Linear):
    dora_m: Optional[np.ndarray] = None        # (N,) float32
    gain: Optional[np.ndarray] = None          # (N,) float32, set by wrap()

    @staticmethod
    def wrap(lin: Linear, m: np.ndarray) -> "DoraLinear":
        assert lin.weight is not None and lin.lora_a is not None, "DoRA sits on a dense linear with LoRA factors"
        out = DoraLinear(dtype=lin.dtype, weight=lin.weight, lora_a=lin.lora_a, lora_b=lin.lora_b, lora_scale=lin.lora_scale,
                         lora_dtype=lin.lora_dtype, dora_m=np.asarray(m, np.float32))
        out.gain = exact_gain(lin.weight, lin.lora_a, lin.lora_b, out.dora_m, lin.lora_scale).astype(np.float32)
        return out

    def __call__(self, x: np.ndarray, xdt: str):
        y, odt = Linear.__call__(self, x, xdt)
        return round_to(round_to(self.gain, xdt) * y, odt), odt


def adapter_kind(cfg: dict) -> str:
    return cfg.get("fine_tune_type") or ("dora" if cfg.get("use_dora") else "lora")


def apply_adapters_dora(weights, n_layers: int, adapter_dir: str) -> None:
    """``ref_generate.apply_adapters``, then every adapted linear of a DoRA directory wrapped with its ``<proj>.m``."""
    cfg = json.loads((Path(adapter_dir) / "adapter_config.json").read_text())
    ref_generate.apply_adapters(weights, n_layers, adapter_dir)
    if adapter_kind(cfg) != "dora":
        return
    raw = ref_generate._load_safetensors(str(Path(adapter_dir) / "adapters.safetensors"))
    keys = cfg["lora_parameters"].get("keys") or ["self_attn.q_proj", "self_attn.v_proj"]
    for i in range(n_layers - int(cfg["num_layers"]), n_layers):
        for key in keys:
            base = f"model.layers.{i}.{key}"
            if weights[base].lora_a is None:
                continue
            weights[base] = DoraLinear.wrap(weights[base], raw[base + ".m"][0])


def load(model_dir: str, adapter_path: Optional[str] = None, max_pos: int = 4096) -> RefModel:
    """``ref_generate.load`` with DoRA directories understood; ``rope_traditional`` by regrouped rows (tests/biased_ref.py)."""
    cfg_dict = json.loads((Path(model_dir) / "config.json").read_text())
    cfg = RefConfig.from_dict(cfg_dict)
    w = ref_generate.load_weights(model_dir, cfg_dict)
    if adapter_path is not None:
        apply_adapters_dora(w, cfg.num_hidden_layers, adapter_path)
    if cfg_dict.get("rope_traditional"):
        for i in range(cfg.num_hidden_layers):
            for proj, heads in (("q_proj", cfg.num_attention_heads), ("k_proj", cfg.num_key_value_heads)):
                name = f"model.layers.{i}.self_attn.{proj}"
                lin = w[name]
                perm = rows_perm(heads, cfg.head_dim)
                lin.weight = np.ascontiguousarray(lin.weight[perm])
                if lin.lora_b is not None:
                    lin.lora_b = np.ascontiguousarray(lin.lora_b[:, perm])
                if isinstance(lin, DoraLinear):
                    lin.dora_m, lin.gain = lin.dora_m[perm], lin.gain[perm]
    return RefModel(cfg, w, max_pos=max_pos)


_MANT = {"float32": 23, "bfloat16": 7, "float16": 10}


def near_boundary(g: np.ndarray, dtype: str, rel: float) -> bool:
    """Does any exact gain (float64) lie within relative ``rel`` of a rounding boundary of ``dtype`` -- a midpoint between two
    neighbouring values of its grid?  (Normal range only: gains are of order 1.)"""
    g = np.abs(np.asarray(g, np.float64))
    g = g[g > 0]
    if g.size == 0:
        return False
    ulp = np.exp2(np.floor(np.log2(g)) - _MANT[dtype])
    frac = g / ulp - np.floor(g / ulp)
    return bool(np.any(np.abs(frac - 0.5) * ulp <= rel * g))
