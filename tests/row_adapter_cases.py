"""The adapters of the per-request adapter tests (test_gpu_row_adapters.py, test_gpu_server_adapters.py): the recipe of
test_gpu_lora_targets.py -- last two blocks, scale 10, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2), float32, one generator per
[seed, layer, key] -- at five (rank, seed, projections).  P is test_gpu_lora_targets.py's all-seven adapter."""
import json

import numpy as np
import torch
from safetensors.torch import save_file

SCALE, NLAYERS = 10.0, 2
ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
       "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
# name -> (rank, seed, projections)
ADAPTERS = {
    "P": (16, 5, ALL),
    "Q": (16, 6, ALL),
    "R1": (1, 7, ALL),
    "R5": (5, 8, ALL[:3]),          # q, k, v only; rank 5: the scalar path of the down kernel
    "R64": (64, 9, ALL[4:]),        # gate, up, down only
}


def dims(cfg):
    """key -> (K, n)"""
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D = cfg.get("head_dim") or H // nh
    I = cfg["intermediate_size"]
    return {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}


def factors(cfg, adapter):
    """{tensor name: float32 array} of one adapter of ADAPTERS"""
    rank, seed, keys = ADAPTERS[adapter]
    d, nl, w = dims(cfg), cfg["num_hidden_layers"], {}
    for i in range(nl - NLAYERS, nl):
        for ki, key in enumerate(ALL):
            if key not in keys:
                continue
            K, n = d[key]
            rng = np.random.default_rng([seed, i, ki])
            w[f"model.layers.{i}.{key}.lora_a"] = (rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32)
            w[f"model.layers.{i}.{key}.lora_b"] = (rng.standard_normal((rank, n)) * 0.05).astype(np.float32)
    return w


def write(dst, cfg, adapter):
    """The adapter as a directory that load_adapters / load_adapter_into / the oracle read -> its path"""
    rank, _, keys = ADAPTERS[adapter]
    dst.mkdir(parents=True, exist_ok=True)
    save_file({k: torch.from_numpy(v) for k, v in factors(cfg, adapter).items()}, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": NLAYERS,
        "lora_parameters": {"rank": rank, "scale": SCALE, "dropout": 0.0, "keys": list(keys)}}))
    return str(dst)
