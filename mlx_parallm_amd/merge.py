"""Merge a LoRA / DoRA adapter into the base weights of a checkpoint (the reference ships ``tools/merge_lora.py`` as a stub).

``merge_adapter_into_weights`` works on the flat ``name -> torch tensor`` dict of a checkpoint, before any engine exists: every
adapted projection's ``.weight`` (or packed ``.weight`` / ``.scales`` / ``.biases`` triple) is replaced by the merged one,
computed on the device by ``mi_lora_merge`` (csrc/lora_merge.hip; the rounding points stand in include/mi355_decode.h).  The
adapter directory is read by ``utils._read_adapter``, so ``num_layers``, ``keys``, ``fine_tune_type`` and ``use_dora`` mean what
they mean to ``load_adapters``.  A linear bias stays as it is (both of mlx-lm's ``fuse`` forms leave it alone).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

from . import _lib as L

_ATTN = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj")
_MLP = ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
# the projections ``Engine.set_lora`` accepts per family; phi3's fused matrices merge whole (A is shared, B spans all rows)
PROJECTIONS = {
    "llama": _ATTN + _MLP, "mistral": _ATTN + _MLP, "qwen3": _ATTN + _MLP, "mixtral": _ATTN,
    "phi3": ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj"),
}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def merge_adapter_into_weights(weights: Dict[str, "object"], config: dict, adapter_path: str, device: int = 0,
                               de_quantize: bool = False) -> List[str]:
    """Replace, in ``weights``, the tensors of every projection the adapter in ``adapter_path`` adapts by the merged ones.
    A quantised projection comes back re-quantised with its own bits and group, or, with ``de_quantize``, as a dense matrix in
    the dtype of its scales (its ``.scales`` / ``.biases`` leave the dict).  Returns the merged projections' names.

    NotImplementedError, naming the projection: a ``block_sparse_moe.*`` key (as ``set_lora`` on that family), any other name
    the family does not adapt, a float32 checkpoint, DoRA on a quantised projection, a group other than 64.  ValueError, naming
    it: factors whose shapes do not fit the matrix, a rank outside 1..64, a DoRA ``m`` that is not finite or a merged row of
    norm 0.  Factors stored in 16 bits are widened to float32 on the host."""
    import torch

    from .utils import _read_adapter

    model_type = config["model_type"]
    allowed = PROJECTIONS.get(model_type)
    if allowed is None:
        raise ValueError(f"Model type {model_type} not supported.")
    entries = list(_read_adapter(int(config["num_hidden_layers"]), adapter_path))    # (a bad directory raises first)
    quant = config.get("quantization") or {}
    for layer, key, *_ in entries:                                                    # (names are refused before any is merged)
        name = f"model.layers.{layer}.{key}"
        if key.startswith("block_sparse_moe."):
            raise NotImplementedError(f"{name}: adapters on the experts of a mixture-of-experts block are not supported")
        if key not in allowed or name + ".weight" not in weights:
            raise NotImplementedError(f"{name}: not a projection a {model_type} adapter can merge into")
    if not torch.cuda.is_available():
        raise RuntimeError("merge_adapter_into_weights: no HIP device available (the merge kernels have no CPU fallback)")
    dev = torch.device("cuda", int(device))
    dt_code = {torch.float32: L.MI_F32, torch.bfloat16: L.MI_BF16, torch.float16: L.MI_F16}
    merged: List[str] = []
    for layer, key, a, b, m, scale in entries:
        name = f"model.layers.{layer}.{key}"
        w = weights[name + ".weight"]
        sc, bi = weights.get(name + ".scales"), weights.get(name + ".biases")
        bits = int(quant.get("bits", 0)) if sc is not None else 0
        group = int(quant.get("group_size", 0)) if sc is not None else 0
        if sc is not None and bits not in (4, 8):
            raise ValueError(f"{name}: a packed weight without a usable config.json quantization entry")
        n_rows = int(w.shape[0])
        k_cols = int(w.shape[1]) * 32 // bits if bits else int(w.shape[1])
        model_dt = sc.dtype if sc is not None else w.dtype
        if model_dt not in dt_code:
            raise ValueError(f"{name}: dtype {model_dt} is not a model dtype")
        fa = torch.as_tensor(a).to(torch.float32).contiguous()
        fb = torch.as_tensor(b).to(torch.float32).contiguous()
        if fa.dim() != 2 or fb.dim() != 2 or fa.shape[1] != fb.shape[0] or fa.shape[0] != k_cols or fb.shape[1] != n_rows:
            raise ValueError(f"{name}: lora_a (K, r) / lora_b (r, N) expected for a ({n_rows}, {k_cols}) matrix, "
                             f"got {tuple(fa.shape)} / {tuple(fb.shape)}")
        fm = None
        if m is not None:
            fm = torch.as_tensor(m).to(torch.float32).contiguous()
            if fm.dim() != 1 or fm.shape[0] != n_rows:
                raise ValueError(f"{name}: m ({n_rows},) expected, got {tuple(fm.shape)}")
            fm = fm.to(dev)
        requant = bits != 0 and not de_quantize
        w_d, fa, fb = w.contiguous().to(dev), fa.to(dev), fb.to(dev)
        sc_d = sc.contiguous().to(dev) if sc is not None else None
        bi_d = bi.contiguous().to(dev) if bi is not None else None
        if requant:
            out_w, out_s, out_b = torch.empty_like(w_d), torch.empty_like(sc_d), torch.empty_like(bi_d)
        else:
            out_w, out_s, out_b = torch.empty((n_rows, k_cols), dtype=model_dt, device=dev), None, None
        torch.cuda.synchronize(dev)
        rc = L.lib().mi_lora_merge(int(device), n_rows, k_cols, int(fa.shape[1]), dt_code[model_dt], bits, group, _ptr(w_d),
                                   _ptr(sc_d), _ptr(bi_d), _ptr(fa), _ptr(fb), _ptr(fm), float(scale), int(requant),
                                   _ptr(out_w), _ptr(out_s), _ptr(out_b))
        if rc != 0:
            msg = L.lib().mi_last_error().decode("utf-8", "replace")
            raise L._ERRORS.get(rc, RuntimeError)(f"{name}: {msg}")
        weights[name + ".weight"] = out_w.to(w.device)
        if requant:
            weights[name + ".scales"], weights[name + ".biases"] = out_s.to(sc.device), out_b.to(bi.device)
        elif sc is not None:
            del weights[name + ".scales"], weights[name + ".biases"]
        merged.append(name)
    return merged
