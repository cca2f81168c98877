"""Host side of LoRA on every projection (no GPU): utils.load_adapters and weight_updater.apply_lora_update hand every key
that the adapter files hold -- k_proj, gate_proj and up_proj included -- to the engine, once per layer, in the files' order.
A recording stub stands in for the engine; what the engine does with the calls is tests/test_gpu_lora_targets.py."""
import json
import threading

import numpy as np
import torch
from safetensors.torch import save_file

from mlx_parallm_amd import utils
from mlx_parallm_amd.weight_updater import apply_lora_update

ALL = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
       "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
H, KD, I, RANK, LAYERS = 32, 16, 48, 4, 4
DIMS = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, KD), "self_attn.v_proj": (H, KD), "self_attn.o_proj": (H, H),
        "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}


class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_lora(self, layer, proj, a, b, scale):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        self.calls.append((int(layer), proj, tuple(a.shape), tuple(b.shape), float(scale), float(a.sum()), float(b.sum())))


class StubModel:
    def __init__(self):
        self.layers = [object()] * LAYERS
        self.engine = RecordingEngine()

    def eval(self):
        return self


def _tensors(layers, keys, seed=0):
    rng = np.random.default_rng(seed)
    w = {}
    for i in layers:
        for key in keys:
            K, n = DIMS[key]
            w[f"model.layers.{i}.{key}.lora_a"] = rng.standard_normal((K, RANK)).astype(np.float32)
            w[f"model.layers.{i}.{key}.lora_b"] = rng.standard_normal((RANK, n)).astype(np.float32)
    return w


def _adapter_dir(dst, layers, keys, cfg_keys, num_layers, scale=10.0, seed=0):
    dst.mkdir(parents=True, exist_ok=True)
    w = _tensors(layers, keys, seed)
    save_file({k: torch.from_numpy(v) for k, v in w.items()}, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": num_layers,
        "lora_parameters": {"rank": RANK, "scale": scale, "dropout": 0.0, "keys": cfg_keys}}))
    return w


def _expected(w, layers, keys, scale):
    return [(i, key, w[f"model.layers.{i}.{key}.lora_a"].shape, w[f"model.layers.{i}.{key}.lora_b"].shape, scale,
             float(torch.from_numpy(w[f"model.layers.{i}.{key}.lora_a"]).sum()),
             float(torch.from_numpy(w[f"model.layers.{i}.{key}.lora_b"]).sum())) for i in layers for key in keys]


def test_load_adapters_hands_all_seven_keys_to_the_engine(tmp_path):
    w = _adapter_dir(tmp_path / "ad", [2, 3], ALL, ALL, num_layers=2, scale=7.5)
    model = StubModel()
    utils.load_adapters(model, str(tmp_path / "ad"))
    assert model.engine.calls == _expected(w, [2, 3], ALL, 7.5)              # once per (layer, key), the config's key order


def test_load_adapters_skips_keys_the_file_does_not_hold(tmp_path):
    """the config may name more than the file holds (and blocks the file leaves out): only what is there reaches the engine"""
    held = ["self_attn.k_proj", "mlp.gate_proj", "mlp.up_proj"]
    w = _adapter_dir(tmp_path / "ad", [3], held, ALL, num_layers=2)
    model = StubModel()
    utils.load_adapters(model, str(tmp_path / "ad"))
    assert model.engine.calls == _expected(w, [3], held, 10.0)


def test_apply_lora_update_with_config_covers_every_key(tmp_path):
    w = _adapter_dir(tmp_path / "ad", [1, 2, 3], ALL, ALL, num_layers=3, scale=4.0, seed=1)
    model = StubModel()
    assert apply_lora_update(model, str(tmp_path / "ad"), lock=threading.RLock()) == 3 * len(ALL)
    assert model.engine.calls == _expected(w, [1, 2, 3], ALL, 4.0)
    assert model._lora_scale == 4.0


def test_apply_lora_update_from_npz_forwards_every_key_in_file_order(tmp_path):
    """no config: every `layers.<i>.<proj>.lora_a` of the archive, in the archive's order, with the scale in force"""
    keys = ["mlp.up_proj", "self_attn.k_proj", "mlp.gate_proj", "self_attn.q_proj", "self_attn.v_proj"]      # (not sorted)
    w = _tensors([3, 0], keys, seed=2)
    (tmp_path / "ad").mkdir()
    np.savez(tmp_path / "ad" / "adapter.npz", **w)
    model = StubModel()
    model._lora_scale = 2.5
    assert apply_lora_update(model, str(tmp_path / "ad")) == 2 * len(keys)
    assert model.engine.calls == _expected(w, [3, 0], keys, 2.5)
