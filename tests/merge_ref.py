"""Oracle-side twin of merging a LoRA / DoRA adapter into the base weights (not a test; the oracle package is left as it is).

The steps are those of include/mi355_decode.h (``mi_lora_merge``), restated from mlx-lm's published ``LoRALinear.fuse``,
``DoRALinear.fuse`` and ``QuantizedLinear.from_linear`` (mlx-lm is not among the reference's sources: nothing here was run
against it).  Every SUM is exact (float64) and rounded once where the step rounds; the lone float32 products, the square root
and the divide are the correctly rounded float32 operations (float64 has the bits to give them exactly):

    1. Wd = W, or T(scale q + bias) of a quantised base               one rounding of the exact value
    2. b' = T(float32(s B^T)),  a' = T(A^T)
    3. delta = T(b' a')                                                 exact sum, one rounding
    4. Wm = T(Wd + delta)                                               exact sum, one rounding
    5. norm = float32(sqrt(sum_k Wm^2)), g = float32(m / norm), W' = T(float32(g Wm));  without m: W' = Wm
    6. re-quantised: oracle.ref_quant.quantize(W', 64, bits, T)

``load`` returns the RefModel of a checkpoint directory whose adapted linears hold the merged weights (llama / qwen3 with or
without linear biases and ``rope_traditional``, mixtral); a Phi-3 checkpoint is served through its split llama form, the fused
adapter cut by columns (``split_phi3_adapter``): the merge works row by row, so the cut commutes with it.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional

import numpy as np

from oracle import ref_generate, ref_quant
from oracle.numerics import round_f64, round_to
from oracle.ref_model import Linear, RefModel


def dequant_T(packed, scales, biases, bits: int, dtype: str, group: int = 64) -> np.ndarray:
    """step 1 of a quantised base: T(scale q + bias), the exact value rounded once"""
    q = ref_quant.unpack(packed, bits).astype(np.float64)
    n, k = q.shape
    v = q.reshape(n, k // group, group) * scales.astype(np.float64)[..., None] + biases.astype(np.float64)[..., None]
    return round_f64(v.reshape(n, k), dtype)


def factors(a, b, s: float, dtype: str):
    """step 2 -> (b' (N, r), a' (r, K)) as float32 values of T"""
    return round_to(np.float32(s) * np.asarray(b, np.float32).T, dtype), round_to(np.asarray(a, np.float32).T, dtype)


def lora_delta(a, b, s: float, dtype: str) -> np.ndarray:
    """steps 2-3 -> delta (float32 values of T)"""
    bp, ap = factors(a, b, s, dtype)
    return round_f64(bp.astype(np.float64) @ ap.astype(np.float64), dtype)


def merge_lora(wd, a, b, s: float, dtype: str) -> np.ndarray:
    """steps 2-4 -> Wm (float32 values of T)"""
    return round_f64(np.asarray(wd, np.float64) + lora_delta(a, b, s, dtype).astype(np.float64), dtype)


def exact_gain(wm, m) -> np.ndarray:
    """m / ||Wm|| per row in float64, no rounding (what the bound of the gain is measured against)"""
    return np.asarray(m, np.float64) / np.sqrt((np.asarray(wm, np.float64) ** 2).sum(axis=1))


def merge(wd, a, b, m, s: float, dtype: str):
    """steps 2-5 -> (W' as float32 values of T, g float32 or None)"""
    wm = merge_lora(wd, a, b, s, dtype)
    if m is None:
        return wm, None
    norm = np.sqrt((wm.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    g = (np.asarray(m, np.float64) / norm.astype(np.float64)).astype(np.float32)
    return round_to((g.astype(np.float64)[:, None] * wm.astype(np.float64)).astype(np.float32), dtype), g


def merge_linear(lin: Linear, a, b, m, s: float, de_quantize: bool = False) -> None:
    """``lin`` (dense or quantised, any Linear subclass) takes the merged weights in place"""
    quantised = lin.weight is None
    assert lin.w16 is None
    wd = dequant_T(lin.packed, lin.scales, lin.biases, lin.bits, lin.dtype, lin.group_size) if quantised else lin.weight
    assert not (quantised and m is not None), "DoRA on a quantised base is refused"
    w2, _g = merge(wd, a, b, m, s, lin.dtype)
    lin._dense_cache = lin._dense64 = None
    if quantised and not de_quantize:
        lin.packed, lin.scales, lin.biases = ref_quant.quantize(w2, lin.group_size, lin.bits, lin.dtype)
    else:
        lin.weight, lin.packed, lin.scales, lin.biases = w2, None, None, None


def read_adapter(n_layers: int, adapter_dir: str):
    """(name, a, b, m or None, scale) per adapted projection, the directory read as ``utils._read_adapter`` reads it"""
    cfg = json.loads((Path(adapter_dir) / "adapter_config.json").read_text())
    dora = (cfg.get("fine_tune_type") or ("dora" if cfg.get("use_dora") else "lora")) == "dora"
    lp = cfg["lora_parameters"]
    raw = ref_generate._load_safetensors(str(Path(adapter_dir) / "adapters.safetensors"))
    for i in range(n_layers - int(cfg["num_layers"]), n_layers):
        for key in lp.get("keys") or ["self_attn.q_proj", "self_attn.v_proj"]:
            base = f"model.layers.{i}.{key}"
            if base + ".lora_a" not in raw or base + ".lora_b" not in raw:
                continue
            yield base, raw[base + ".lora_a"][0], raw[base + ".lora_b"][0], (raw[base + ".m"][0] if dora else None), float(lp["scale"])


def load(model_dir: str, adapter_path: Optional[str] = None, max_pos: int = 4096, de_quantize: bool = False) -> RefModel:
    """The twin of ``utils.load(model_dir, adapter_path=..., merge_adapter=True)``."""
    import biased_ref
    import moe_ref
    from biased_ref import rows_perm

    cfg_dict = json.loads((Path(model_dir) / "config.json").read_text())
    trad = bool(cfg_dict.get("rope_traditional"))
    if cfg_dict["model_type"] == "mixtral":
        assert not trad
        model = moe_ref.load(model_dir, max_pos=max_pos)
    elif trad:                                               # loaded as the half-split model, regrouped AFTER the merge
        model = ref_generate.load(model_dir, max_pos=max_pos)
    else:
        model = biased_ref.load(model_dir, max_pos=max_pos)
    if adapter_path is not None:
        for name, a, b, m, s in read_adapter(model.cfg.num_hidden_layers, adapter_path):
            merge_linear(model.w[name], a, b, m, s, de_quantize=de_quantize)
    if trad:
        for i in range(model.cfg.num_hidden_layers):
            for proj, heads in (("q_proj", model.cfg.num_attention_heads), ("k_proj", model.cfg.num_key_value_heads)):
                lin = model.w[f"model.layers.{i}.self_attn.{proj}"]
                lin.weight = np.ascontiguousarray(lin.weight[rows_perm(heads, model.cfg.head_dim)])
    return model


def split_phi3_adapter(src: str, dst: str, cfg: dict) -> str:
    """A Phi-3 adapter directory (fused names) as the directory of the split llama form: A shared, B and m cut by columns."""
    import torch
    from safetensors.torch import load_file, save_file

    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv, inter = cfg.get("num_key_value_heads") or nh, cfg["intermediate_size"]
    D = H // nh
    cuts = {"self_attn.qkv_proj": (("self_attn.q_proj", nh * D), ("self_attn.k_proj", nkv * D), ("self_attn.v_proj", nkv * D)),
            "mlp.gate_up_proj": (("mlp.gate_proj", inter), ("mlp.up_proj", inter))}
    acfg = json.loads((Path(src) / "adapter_config.json").read_text())
    raw, out, keys = load_file(str(Path(src) / "adapters.safetensors")), {}, []
    for key in acfg["lora_parameters"]["keys"]:
        keys += [nm for nm, _ in cuts.get(key, ((key, 0),))]
    for name, t in raw.items():
        base, _, leaf = name.rpartition(".")
        prefix, _, key = base.partition(".self_attn.") if ".self_attn." in base else base.partition(".mlp.")
        key = ("self_attn." if ".self_attn." in base else "mlp.") + key
        if key not in cuts:
            out[name] = t
            continue
        c0 = 0
        for nm, n in cuts[key]:
            part = t if leaf == "lora_a" else (t[:, c0:c0 + n] if leaf == "lora_b" else t[c0:c0 + n])
            out[f"{prefix}.{nm}.{leaf}"] = part.contiguous().clone()
            c0 += n
    Path(dst).mkdir(parents=True, exist_ok=True)
    save_file(out, str(Path(dst) / "adapters.safetensors"))
    acfg["lora_parameters"]["keys"] = keys
    (Path(dst) / "adapter_config.json").write_text(json.dumps(acfg))
    return str(dst)
