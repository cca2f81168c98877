"""Mixtral without a device: the model class and its arguments, the tiny builder's two name forms, the refusals of the new arch
(every one is decided before the device is looked for), conversion, the weight broadcast's bucket plan for 3-D tensors, and
the oracle twin (tests/moe_ref.py) against the committed goldens (tests/golden/moe) with their router-margin condition."""
import ctypes as C
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

MOE = Path(__file__).resolve().parent / "golden" / "moe"
sys.path.insert(0, str(MOE))

import make_golden_moe as gen  # noqa: E402
import moe_ref  # noqa: E402
import test_golden as cpu_golden  # noqa: E402
from mlx_parallm_amd import _lib, tiny_model, utils  # noqa: E402
from mlx_parallm_amd import distributed as D  # noqa: E402
from mlx_parallm_amd.engine import Engine  # noqa: E402
from mlx_parallm_amd.models import mixtral  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from oracle import ref_generate  # noqa: E402

GOLDEN = sorted(MOE.glob("*.npz"))

# every key of Mixtral-8x7B-v0.1's config.json
MIXTRAL_CONFIG = {
    "architectures": ["MixtralForCausalLM"], "attention_dropout": 0.0, "bos_token_id": 1, "eos_token_id": 2, "hidden_act": "silu",
    "hidden_size": 4096, "initializer_range": 0.02, "intermediate_size": 14336, "max_position_embeddings": 32768,
    "model_type": "mixtral", "num_attention_heads": 32, "num_experts_per_tok": 2, "num_hidden_layers": 32,
    "num_key_value_heads": 8, "num_local_experts": 8, "output_router_logits": False, "rms_norm_eps": 1e-05, "rope_theta": 1000000.0,
    "router_aux_loss_coef": 0.02, "sliding_window": None, "tie_word_embeddings": False, "torch_dtype": "bfloat16",
    "transformers_version": "4.36.0.dev0", "use_cache": True, "vocab_size": 32000,
}


def test_class_lookup_and_model_args_defaults():
    model_cls, args_cls = utils._get_classes({"model_type": "mixtral"})
    assert args_cls is mixtral.ModelArgs and model_cls._ARCH == "mixtral"
    a = args_cls.from_dict({"model_type": "mixtral"})                          # mixtral.py:12-31
    assert (a.vocab_size, a.hidden_size, a.intermediate_size, a.num_hidden_layers, a.num_attention_heads) == (32000, 4096, 14336, 32, 32)
    assert (a.num_experts_per_tok, a.num_key_value_heads, a.num_local_experts) == (2, 8, 8)
    assert (a.rms_norm_eps, a.rope_theta, a.rope_traditional, a.rope_scaling) == (1e-5, 1e6, False, None)
    full = args_cls.from_dict(MIXTRAL_CONFIG)
    assert (full.num_local_experts, full.num_experts_per_tok, full.hidden_size // full.num_attention_heads) == (8, 2, 128)
    assert args_cls.from_dict(dict(MIXTRAL_CONFIG, num_key_value_heads=None)).num_key_value_heads == 32


def test_tiny_builder_writes_both_name_forms_with_the_same_numbers(tmp_path):
    from safetensors.torch import load_file

    kw = dict(gen.MODELS["moe_e4k2_bf16"][0], seed=5)
    cfg = build_tiny_model(tmp_path / "stacked", **kw)
    cfg2 = build_tiny_model(tmp_path / "per", expert_names="per_expert", **kw)
    assert cfg == cfg2 == json.loads((tmp_path / "per" / "config.json").read_text())
    assert (cfg["model_type"], cfg["num_local_experts"], cfg["num_experts_per_tok"], cfg["tie_word_embeddings"]) == ("mixtral", 4, 2, False)
    st, per = load_file(str(tmp_path / "stacked" / "model.safetensors")), load_file(str(tmp_path / "per" / "model.safetensors"))
    assert st["model.layers.0.block_sparse_moe.switch_mlp.gate_proj.weight"].shape == (4, 192, 128)
    assert st["model.layers.1.block_sparse_moe.switch_mlp.down_proj.weight"].shape == (4, 128, 192)
    assert st["model.layers.0.block_sparse_moe.gate.weight"].shape == (4, 128)
    assert per["model.layers.0.block_sparse_moe.experts.3.w2.weight"].shape == (128, 192)
    assert not any(".mlp." in k for k in st) and not any("switch_mlp" in k for k in per)
    assert torch.equal(per["model.layers.1.block_sparse_moe.experts.2.w3.weight"],
                       st["model.layers.1.block_sparse_moe.switch_mlp.up_proj.weight"][2])       # w3 is up (mixtral.py:203)
    back = tiny_model.stack_experts(per)
    assert set(back) == set(st) and all(torch.equal(back[k], st[k]) for k in st)
    # router_gain scales the router alone
    build_tiny_model(tmp_path / "g1", **dict(kw, router_gain=1.0))
    g1 = load_file(str(tmp_path / "g1" / "model.safetensors"))
    r4, r1 = st["model.layers.0.block_sparse_moe.gate.weight"].float(), g1["model.layers.0.block_sparse_moe.gate.weight"].float()
    assert torch.allclose(r4, 4.0 * r1, rtol=2 ** -7) and torch.equal(g1["model.layers.0.self_attn.q_proj.weight"], st["model.layers.0.self_attn.q_proj.weight"])
    for bad in (dict(quantize_model=True), dict(dtype="float32"), dict(tie_word_embeddings=True), dict(expert_names="rows")):
        with pytest.raises(ValueError):
            build_tiny_model(tmp_path / "bad", **dict(kw, **bad))


def _desc(**over):
    d = _lib.ModelDesc()
    d.struct_size = C.sizeof(_lib.ModelDesc)
    vals = dict(arch=_lib.MI_ARCH_MIXTRAL, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=32,
                intermediate_size=192, vocab_size=1024, rms_norm_eps=1e-5, rope_theta=1e6, rope_scale=1.0, act_dtype=_lib.MI_BF16,
                max_positions=64, num_local_experts=4, num_experts_per_tok=2)
    vals.update(over)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _create(d):
    h = C.c_void_p()
    rc = _lib.lib().mi_engine_create(C.byref(d), 0, C.byref(h))
    msg = _lib.lib().mi_last_error().decode()
    if rc == 0:
        _lib.lib().mi_engine_destroy(h)
    return rc, msg


@pytest.mark.parametrize("over, code, word", [
    (dict(act_dtype=_lib.MI_F32), -3, "act_dtype"),
    (dict(quant_bits=4, quant_group_size=64), -3, "quant_bits"),
    (dict(quant_bits=8, quant_group_size=64), -3, "quant_bits"),
    (dict(tie_word_embeddings=1), -1, "tie_word_embeddings"),
    (dict(attention_bias=1), -1, "attention_bias"),
    (dict(mlp_bias=1), -1, "mlp_bias"),
    (dict(num_local_experts=0), -3, "num_local_experts"),
    (dict(num_local_experts=17), -3, "num_local_experts"),
    (dict(num_experts_per_tok=0), -3, "num_experts_per_tok"),
    (dict(num_experts_per_tok=3), -3, "num_experts_per_tok"),
    (dict(num_local_experts=1, num_experts_per_tok=2), -3, "num_experts_per_tok"),
    (dict(hidden_size=96, num_heads=3, num_kv_heads=3), -3, "hidden_size"),
    (dict(intermediate_size=160), -3, "intermediate_size"),
])
def test_creation_refusals_name_the_field(over, code, word):
    rc, msg = _create(_desc(**over))
    assert rc == code and word in msg and "mixtral" in msg, (rc, msg)


def test_a_good_desc_passes_every_check_up_to_the_device():
    for over in (dict(), dict(num_local_experts=16), dict(num_local_experts=1, num_experts_per_tok=1), dict(act_dtype=_lib.MI_F16),
                 dict(rope_traditional=1)):
        rc, msg = _create(_desc(**over))
        assert rc == 0 or (rc == -4 and "no HIP device" in msg), (over, rc, msg)
    # the two counts are ignored by every other arch
    rc, msg = _create(_desc(arch=_lib.MI_ARCH_LLAMA, num_local_experts=99, num_experts_per_tok=7))
    assert rc == 0 or (rc == -4 and "no HIP device" in msg), (rc, msg)


def test_engine_refuses_a_quantization_entry_and_ignores_rope_scaling():
    cfg = dict(MIXTRAL_CONFIG, num_hidden_layers=2, hidden_size=128, intermediate_size=192, num_attention_heads=4,
               num_key_value_heads=2, vocab_size=1024)
    with pytest.raises(NotImplementedError, match="quantization"):
        Engine(dict(cfg, quantization={"group_size": 64, "bits": 4}), max_positions=64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):               # past every check of the description
            Engine(dict(cfg, rope_scaling={"type": "yarn", "factor": 8.0}, head_dim=64), max_positions=64)


def test_convert_casts_a_mixtral_checkpoint_and_refuses_to_quantise_it(tmp_path):
    from safetensors.torch import load_file

    from mlx_parallm_amd import convert as cv

    kw = dict(gen.MODELS["moe_e4k2_bf16"][0], seed=9)
    build_tiny_model(tmp_path / "src", **kw)
    with pytest.raises(NotImplementedError, match="Mixtral"):
        cv.convert(str(tmp_path / "src"), str(tmp_path / "q4"), quantize=True)
    assert not (tmp_path / "q4").exists()
    cv.convert(str(tmp_path / "src"), str(tmp_path / "f16"), dtype="float16")
    src = load_file(str(tmp_path / "src" / "model.safetensors"))
    out = load_file(str(tmp_path / "f16" / "model.safetensors"))
    name = "model.layers.1.block_sparse_moe.switch_mlp.down_proj.weight"
    assert set(out) == set(src) and out[name].dtype == torch.float16 and out[name].shape == (4, 128, 192)
    assert torch.equal(out[name], src[name].to(torch.float16))
    assert json.loads((tmp_path / "f16" / "config.json").read_text())["num_local_experts"] == 4


def test_weight_broadcast_plan_carries_3d_tensors():
    specs = [("model.layers.0.block_sparse_moe.gate.weight", (4, 128)),
             ("model.layers.0.block_sparse_moe.switch_mlp.gate_proj.weight", (4, 192, 128)),
             ("model.layers.0.block_sparse_moe.switch_mlp.down_proj.weight", (4, 128, 192))]
    buckets = D.plan_buckets(specs, elem_size=2, bucket_bytes=1 << 20)
    flat = [b for bucket in buckets for b in bucket]
    assert [(n, s) for n, s, _o, _c in flat] == specs and flat[1][3] == 4 * 192 * 128 and all(o % 128 == 0 for _n, _s, o, _c in flat)
    src = {n: torch.randn(s).to(torch.bfloat16) for n, s in specs}
    for bucket in buckets:                                                     # the round trip of replicate_checkpoint, in one process
        buf = torch.zeros(D.bucket_numel(bucket), dtype=torch.bfloat16)
        for n, s, off, cnt in bucket:
            buf[off:off + cnt].copy_(src[n].reshape(-1))
        for n, s, off, cnt in bucket:
            assert torch.equal(buf[off:off + cnt].view(s), src[n])


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle twin and the goldens

def test_moe_golden_files_present():
    assert {p.stem for p in GOLDEN} == set(gen.CASES), "run tests/golden/moe/make_golden_moe.py"
    biggest = max(p.stat().st_size for p in (MOE.parent / "d96").glob("*.npz"))
    for p in GOLDEN:
        spec = json.loads(str(np.load(p)["spec"]))
        m = spec["model"]
        assert p.stat().st_size <= biggest
        assert (m["hidden_size"], m["layers"], m["heads"], m["kv_heads"], m["intermediate_size"]) == (128, 2, 4, 2, 192)
        assert (spec["B"], spec["L0"], spec["steps"]) == (2, 6, 6) and spec["seeds_tried"] <= gen.MAX_SEEDS
    models = [json.loads(str(np.load(p)["spec"]))["model"] for p in GOLDEN]
    shapes = {(m["num_local_experts"], m["num_experts_per_tok"], m["dtype"]) for m in models}
    assert {(4, 2, "bfloat16"), (8, 2, "bfloat16"), (4, 2, "float16"), (8, 2, "float16"), (4, 1, "bfloat16")} <= shapes
    assert any(json.loads(str(np.load(p)["spec"]))["model"].get("rope_traditional") for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_oracle_twin_reproduces_moe_golden(path, monkeypatch):
    monkeypatch.setattr(ref_generate, "load", moe_ref.load)
    cpu_golden.test_oracle_reproduces_golden(path)


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_moe_golden_meets_the_router_margin_condition(path):
    """Every (token, layer) pair of the oracle's run -- none is exempt -- keeps the k-th and the (k + 1)-th gate logit apart by
    1e-3 (float32-KV) or by 4 ulps of the model dtype at the larger of the two (model-KV)."""
    g = np.load(path)
    spec = json.loads(str(g["spec"]))
    _arrays, ref = gen.run_model(spec["model"], spec, g["prompts"])
    pairs = sum(len(m) for _l, m, _a in ref.margins)
    assert pairs == spec["router_pairs"] >= spec["model"]["layers"] * spec["B"] * (spec["L0"] + spec["steps"] - 1)
    assert moe_ref.margin_shortfall(ref, spec["model"]["dtype"], spec["paged"]) <= 0
    assert abs(min(float(np.min(m)) for _l, m, _a in ref.margins) - spec["router_margin_min"]) <= 1e-6
    if spec["model"]["num_local_experts"] > spec["model"]["num_experts_per_tok"]:
        assert all(np.all(np.isfinite(m)) for _l, m, _a in ref.margins)


def test_twin_routing_rule_and_the_e1_block_is_the_dense_mlp():
    g = np.array([[1.0, 3.0, 3.0, -1.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 4.0]], np.float32)
    sel, soft, margin, _at = moe_ref.route(g, 2)
    assert sel.tolist() == [[1, 2], [0, 1], [2, 3]] and margin.tolist() == [2.0, 0.0, 4.0]           # a tie goes to the lower index
    assert np.allclose(soft[0], [0.5, 0.5]) and np.allclose(soft[2], np.exp([0.0, -1.0]) / (1 + np.exp(-1.0)), atol=1e-7)
    sel1, soft1, margin1, _ = moe_ref.route(g[:, :1], 1)
    assert sel1.tolist() == [[0]] * 3 and soft1.tolist() == [[1.0]] * 3 and np.all(np.isinf(margin1))
    # E = 1, k = 1: the block is the dense SwiGLU MLP holding the one expert's matrices
    with tempfile.TemporaryDirectory() as d:
        kw = dict(gen.MODELS["moe_e4k1_bf16"][0], seed=3, num_local_experts=1)
        build_tiny_model(d, **kw)
        ref = moe_ref.load(d, max_pos=64)
    x = np.asarray(np.random.default_rng(0).standard_normal((2, 3, 128)), np.float32)
    x = moe_ref.round_to(x, "bfloat16")
    got, gdt = ref._mlp(0, x, "bfloat16")
    p = "model.layers.0.block_sparse_moe.experts.0."
    want, wdt = moe_ref.swiglu_mlp(ref.w[p + "gate_proj"], ref.w[p + "up_proj"], ref.w[p + "down_proj"], x, "bfloat16")
    assert gdt == wdt == "bfloat16" and np.array_equal(got, want)
