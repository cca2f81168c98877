"""DoRA without a GPU: what ``utils._read_adapter`` accepts, how ``load_adapters`` / ``load_adapter_into`` and the weight
updater route LoRA and DoRA entries, and the oracle-side twin (tests/dora_ref.py) against a brute-force float64 formula."""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, str(Path(__file__).resolve().parent))

import dora_ref  # noqa: E402
from mlx_parallm_amd import utils, weight_updater  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from oracle.ref_model import Linear  # noqa: E402

KEYS = ["self_attn.q_proj", "mlp.down_proj"]


def write_adapter(path: Path, cfg_extra: dict, with_m: bool, n_layers=2, drop_m=None, seed=0):
    path.mkdir(parents=True, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    t = {}
    for i in range(n_layers):
        for key in KEYS:
            base = f"model.layers.{i}.{key}"
            t[base + ".lora_a"] = torch.randn(8, 2, generator=g)
            t[base + ".lora_b"] = torch.randn(2, 6, generator=g)
            if with_m and base != drop_m:
                t[base + ".m"] = torch.rand(6, generator=g) + 0.5
    save_file(t, str(path / "adapters.safetensors"))
    cfg = {"num_layers": n_layers, "lora_parameters": {"rank": 2, "scale": 3.0, "dropout": 0.0, "keys": KEYS}}
    cfg.update(cfg_extra)
    (path / "adapter_config.json").write_text(json.dumps(cfg))
    return t


class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_lora(self, layer, proj, a, b, scale):
        self.calls.append(("set_lora", layer, proj, tuple(np.asarray(a).shape), float(scale)))

    def set_dora(self, layer, proj, a, b, m, scale):
        self.calls.append(("set_dora", layer, proj, tuple(np.asarray(m).shape), float(scale)))

    def set_adapter_lora(self, slot, layer, proj, a, b, scale):
        self.calls.append(("set_adapter_lora", slot, layer, proj))

    def set_adapter_dora(self, slot, layer, proj, a, b, m, scale):
        self.calls.append(("set_adapter_dora", slot, layer, proj, tuple(m.shape)))

    def clear_adapter(self, slot):
        self.calls.append(("clear_adapter", slot))


def fake_model(n_layers=2):
    return SimpleNamespace(layers=[None] * n_layers, engine=RecordingEngine())


@pytest.mark.parametrize("cfg_extra", [{"fine_tune_type": "dora"}, {"use_dora": True}])
def test_read_adapter_takes_both_dora_spellings(tmp_path, cfg_extra):
    t = write_adapter(tmp_path / "a", cfg_extra, with_m=True)
    entries = list(utils._read_adapter(2, str(tmp_path / "a")))
    assert [(i, k) for i, k, *_ in entries] == [(i, k) for i in range(2) for k in KEYS]
    for i, key, a, b, m, scale in entries:
        assert torch.equal(m, t[f"model.layers.{i}.{key}.m"]) and scale == 3.0
        assert torch.equal(a, t[f"model.layers.{i}.{key}.lora_a"]) and torch.equal(b, t[f"model.layers.{i}.{key}.lora_b"])


def test_read_adapter_lora_has_no_m_and_full_is_refused(tmp_path):
    write_adapter(tmp_path / "l", {"fine_tune_type": "lora"}, with_m=False)
    assert all(m is None for *_, m, _s in utils._read_adapter(2, str(tmp_path / "l")))
    write_adapter(tmp_path / "plain", {}, with_m=False)                        # no fine_tune_type at all: LoRA
    assert all(m is None for *_, m, _s in utils._read_adapter(2, str(tmp_path / "plain")))
    write_adapter(tmp_path / "f", {"fine_tune_type": "full"}, with_m=False)
    with pytest.raises(NotImplementedError, match="full"):
        list(utils._read_adapter(2, str(tmp_path / "f")))


def test_read_adapter_names_the_missing_m(tmp_path):
    write_adapter(tmp_path / "d", {"fine_tune_type": "dora"}, with_m=True, drop_m="model.layers.1.mlp.down_proj")
    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.down_proj\.m"):
        list(utils._read_adapter(2, str(tmp_path / "d")))
    model = fake_model()
    with pytest.raises(ValueError):
        utils.load_adapter_into(model, 3, str(tmp_path / "d"))
    assert model.engine.calls == []                                            # refused before the slot was touched


def test_routing_of_mixed_slots(tmp_path):
    write_adapter(tmp_path / "d", {"fine_tune_type": "dora"}, with_m=True)
    write_adapter(tmp_path / "l", {"fine_tune_type": "lora"}, with_m=False)
    model = fake_model()
    utils.load_adapter_into(model, 0, str(tmp_path / "d"))
    utils.load_adapter_into(model, 1, str(tmp_path / "l"))
    calls = model.engine.calls
    assert calls[0] == ("clear_adapter", 0) and calls[5] == ("clear_adapter", 1)
    assert calls[1:5] == [("set_adapter_dora", 0, i, k, (6,)) for i in range(2) for k in KEYS]
    assert calls[6:] == [("set_adapter_lora", 1, i, k) for i in range(2) for k in KEYS]
    wide = fake_model()
    utils.load_adapters(wide, str(tmp_path / "d"))
    assert [c[0] for c in wide.engine.calls] == ["set_dora"] * 4
    wide = fake_model()
    utils.load_adapters(wide, str(tmp_path / "l"))
    assert [c[0] for c in wide.engine.calls] == ["set_lora"] * 4


def test_weight_updater_without_a_config_takes_a_sibling_m_as_dora(tmp_path):
    t = write_adapter(tmp_path / "u", {}, with_m=True, drop_m="model.layers.0.self_attn.q_proj")
    (tmp_path / "u" / "adapter_config.json").unlink()
    model = fake_model()
    model._lora_scale = 2.5
    assert weight_updater.apply_lora_update(model, str(tmp_path / "u")) == 4
    kinds = {(c[1], c[2]): c[0] for c in model.engine.calls}
    assert kinds == {(0, "self_attn.q_proj"): "set_lora", (0, "mlp.down_proj"): "set_dora",
                     (1, "self_attn.q_proj"): "set_dora", (1, "mlp.down_proj"): "set_dora"}
    assert all(c[4] == 2.5 for c in model.engine.calls) and len(t) == 11


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_twin_against_brute_force(dtype):
    rng = np.random.default_rng(5)
    N, K, r, s = 32, 64, 5, 1.75
    w = round_to(rng.standard_normal((N, K)).astype(np.float32) * 0.1, dtype)
    a = (rng.standard_normal((K, r)) * 0.05).astype(np.float32)
    b = (rng.standard_normal((r, N)) * 0.2).astype(np.float32)
    m = (rng.random(N) + 0.5).astype(np.float32)
    lin = dora_ref.DoraLinear.wrap(Linear(dtype=dtype, weight=w, lora_a=a, lora_b=b, lora_scale=s), m)
    gain = np.empty(N)
    for n in range(N):                                                          # the formula, element by element
        tot = 0.0
        for k in range(K):
            d = float(w[n, k]) + s * sum(float(b[j, n]) * float(a[k, j]) for j in range(r))
            tot += d * d
        gain[n] = float(m[n]) / tot ** 0.5
    assert np.allclose(dora_ref.exact_gain(w, a, b, m, s), gain, rtol=1e-13, atol=0)
    assert np.array_equal(lin.gain, gain.astype(np.float32))
    x = round_to(rng.standard_normal((3, K)).astype(np.float32), dtype)
    y, odt = lin(x, dtype)
    base, _ = Linear(dtype=dtype, weight=w, lora_a=a, lora_b=b, lora_scale=s)(x, dtype)
    assert odt == dtype and np.array_equal(y, round_to(round_to(gain.astype(np.float32), dtype) * base, dtype))
    y32, odt32 = lin(x.astype(np.float32), "float32")                          # float32 rows: g itself multiplies
    base32, _ = Linear(dtype=dtype, weight=w, lora_a=a, lora_b=b, lora_scale=s)(x, "float32")
    assert odt32 == "float32" and np.array_equal(y32, gain.astype(np.float32) * base32)
    assert dora_ref.condition(w, a, b, 0.0) == 1.0 and dora_ref.condition(w, a, b, s) >= 1.0


def test_near_boundary():
    assert dora_ref.near_boundary(np.array([1.0 + 2.0 ** -8]), "bfloat16", 1e-6)          # the midpoint of [1, 1 + 2^-7]
    assert not dora_ref.near_boundary(np.array([1.0 + 2.0 ** -7]), "bfloat16", 1e-3)      # a grid point
    assert dora_ref.near_boundary(np.array([0.75, 3.0 + 2.0 ** -10]), "float16", 1e-6)    # half an ulp (2^-9) above 3
    assert not dora_ref.near_boundary(np.array([0.75, 1.3]), "float16", 1e-6)
    assert dora_ref.near_boundary(np.array([np.float64(np.float32(1.3)) + 2.0 ** -24]), "float32", 1e-9)
