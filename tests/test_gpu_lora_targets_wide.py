"""LoRA on all seven projections at PRODUCTION width (-m gpu): two-layer checkpoints of tests/wide_models.py --
Mistral-7B bf16 at B = 8 and Qwen3-14B int4 at B = 64 (BASELINE config 5's regime: the decode step's gate|up runs gemm_q4.hip,
whose SwiGLU form an adapted gate|up must bypass) -- with an adapter on every linear of both blocks, a 16-token prompt and 2
decode steps, in both KV modes.  The oracle is far too slow here; the property is that of tests/test_gpu_fullsize.py: the
default routing and the exact routing (generic VALU GEMV, unfused VALU attention, no tile GEMM) are two implementations of
the same model.

Two bounds on the logits of every call:
  * test_gpu_fullsize.py's _noise_equal (measured at 32 layers: loose at 2);
  * self-calibrating: max |default - exact| <= 1/5 of the SMALLEST max-abs effect, on the exact route, of dropping k_proj,
    gate_proj or up_proj from the adapter -- so a route that lost one of the new terms cannot pass.  A projection is
    dropped by hot-swapping a zero B (its term is then exactly 0).  The adapter is the recipe of
    test_gpu_lora_targets.py (rank 16, scale 10, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2)): its terms are about as large as
    the projections' own outputs (std 10 * sqrt(16/3) * 0.05 = 1.15 against 0.02 * sqrt(K) = 1.28 at K = 4096), far above
    the rounding noise of two blocks; the test asserts that the choice holds (smallest effect >= 5 x the measured noise
    is the bound itself)."""
import gc
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import wide_models

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from test_gpu_fullsize import _noise_equal  # noqa: E402

ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
       "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
NEW = ("self_attn.k_proj", "mlp.gate_proj", "mlp.up_proj")
RANK, SCALE = 16, 10.0
EXACT = dict(force_generic_gemv=1, fused_decode_attention=0, prefill_gemm=0, decode_attention_mfma=0)
DEFAULT = dict(force_generic_gemv=0, fused_decode_attention=1, prefill_gemm=1, decode_attention_mfma=1)
CASES = [("mistral-7b", "bf16", 41, 8), ("qwen3-14b", "int4", 42, 64)]


def _factors(cfg, seed):
    H, nh, nkv, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["intermediate_size"]
    D = cfg.get("head_dim") or H // nh
    dims = {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}
    w = {}
    for i in range(cfg["num_hidden_layers"]):
        for ki, key in enumerate(ALL):
            K, n = dims[key]
            rng = np.random.default_rng([seed, i, ki])
            w[f"model.layers.{i}.{key}.lora_a"] = (rng.uniform(-1, 1, (K, RANK)) / np.sqrt(K)).astype(np.float32)
            w[f"model.layers.{i}.{key}.lora_b"] = (rng.standard_normal((RANK, n)) * 0.05).astype(np.float32)
    return w


@pytest.fixture(scope="module", params=CASES, ids=[f"{c[0]}-{c[1]}-B{c[3]}" for c in CASES])
def wide(request, tmp_path_factory):
    family, precision, seed, B = request.param
    d = tmp_path_factory.mktemp("wide_lora") / f"{family}-{precision}"
    cfg = wide_models.build_checkpoint(d, family, precision, seed)
    fac = _factors(cfg, seed)
    ad = d / "adapter"
    ad.mkdir()
    save_file({k: torch.from_numpy(v) for k, v in fac.items()}, str(ad / "adapters.safetensors"))
    (ad / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": cfg["num_hidden_layers"],
        "lora_parameters": {"rank": RANK, "scale": SCALE, "dropout": 0.0, "keys": list(ALL)}}))
    model = utils.load_model(str(d), max_positions=wide_models.MAX_POS)
    utils.load_adapters(model, str(ad))
    for f in d.rglob("*.safetensors"):
        f.unlink()                                            # (gigabytes: the engine holds the weights now)
    yield model, cfg, fac, B
    model.engine.close()
    gc.collect()


def _run(eng, prompts, kvd, opts):
    """prefill + 2 greedy decode steps under `opts` -> the logits of the three calls [3][B][V]"""
    for k, v in opts.items():
        eng.set_option(k, v)
    kv = eng.new_kv(prompts.shape[0], capacity=prompts.shape[1] + 4, kv_dtype=kvd)
    out = [eng.forward(prompts, kv)]
    for _ in range(2):
        out.append(eng.forward(np.argmax(out[-1], axis=-1).astype(np.int32)[:, None], kv))
    kv.close()
    for k, v in DEFAULT.items():
        eng.set_option(k, v)
    return np.stack(out)


@pytest.mark.parametrize("kvd", ["model", "float32"])
def test_default_routing_equals_exact_routing_with_all_seven_adapted(wide, kvd):
    model, cfg, fac, B = wide
    eng = model.engine
    prompts = np.random.default_rng(7).integers(3, cfg["vocab_size"], size=(B, 16)).astype(np.int32)
    exact = _run(eng, prompts, kvd, EXACT)
    assert np.isfinite(exact).all() and exact.std() > 0.05
    # teacher forcing by the exact route's tokens keeps the three calls comparable: feed the same ids on every route
    ids = [np.argmax(exact[i], axis=-1).astype(np.int32)[:, None] for i in range(2)]

    def forced(opts):
        for k, v in opts.items():
            eng.set_option(k, v)
        kv = eng.new_kv(B, capacity=20, kv_dtype=kvd)
        out = [eng.forward(prompts, kv), eng.forward(ids[0], kv), eng.forward(ids[1], kv)]
        kv.close()
        for k, v in DEFAULT.items():
            eng.set_option(k, v)
        return np.stack(out)

    effects = {}
    for key in NEW:                                           # the adapter without `key`, on the exact route
        for i in range(cfg["num_hidden_layers"]):
            a, b = fac[f"model.layers.{i}.{key}.lora_a"], fac[f"model.layers.{i}.{key}.lora_b"]
            eng.set_lora(i, key, a, np.zeros_like(b), SCALE)
        effects[key] = float(np.abs(forced(EXACT) - exact).max())
        for i in range(cfg["num_hidden_layers"]):
            eng.set_lora(i, key, fac[f"model.layers.{i}.{key}.lora_a"], fac[f"model.layers.{i}.{key}.lora_b"], SCALE)
    again = forced(EXACT)
    assert np.array_equal(again, exact)                       # the factors are back: the same bits as before
    default = forced(DEFAULT)
    noise = float(np.abs(default - exact).max())
    print(f"{kvd} B={B}: max |default - exact| = {noise:.4f}; effect of dropping " +
          ", ".join(f"{k.split('.')[-1]} {v:.3f}" for k, v in effects.items()))
    for i in range(3):
        _noise_equal(default[i], exact[i])
    assert noise <= min(effects.values()) / 5, (noise, effects)
