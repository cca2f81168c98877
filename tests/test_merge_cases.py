"""The adapter-merge cases on the CPU: the exact constructions are exact on the twin alone, the float32 envelope is counted
against the twin (the counts the GPU test's rule rests on: tests/merge_cases.py), a deliberately wrong variant changes the
bits, and the merge tool / the flags refuse what they must -- all without a device."""
import json

import numpy as np
import pytest

import merge_cases as mc
import merge_ref
from oracle import ref_quant
from oracle.numerics import round_to


def _wd(inp, dtype, bits):
    return merge_ref.dequant_T(inp["packed"], inp["scales"], inp["biases"], bits, dtype) if bits else inp["w"]


@pytest.mark.parametrize("bits", mc.BASES)
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_exact_constructions_are_exact_on_the_twin(dtype, bits):
    for N, K, r in mc.SHAPES:
        for dora in ((False, True) if bits == 0 else (False,)):
            inp = mc.exact_inputs(N, K, r, dtype, bits, dora)
            assert mc.exact_is_exact(inp, dtype, bits), (N, K, r, dora)
            twin = merge_ref.merge_lora(_wd(inp, dtype, bits), inp["a"], inp["b"], inp["s"], dtype)
            for variant in (dict(), dict(descending=True), dict(sum_before_rounding=True)):     # any order, the same bits
                assert np.array_equal(mc.restate_f32(inp, dtype, bits, **variant).view(np.uint32), twin.view(np.uint32)), (N, K, r, variant)
            if dora:                                                                          # the norm is a float32 number
                ss = (twin.astype(np.float64) ** 2).sum(axis=1)
                assert np.array_equal(ss, ss.astype(np.float32).astype(np.float64)) and (ss > 0).all()


def envelope_count(dtype, bits):
    diff = total = 0
    for N, K, r in mc.SHAPES:
        inp = mc.random_inputs(N, K, r, dtype, bits)
        twin = merge_ref.merge_lora(_wd(inp, dtype, bits), inp["a"], inp["b"], inp["s"], dtype)
        got = mc.restate_f32(inp, dtype, bits)
        assert np.isfinite(got).all()
        delta = merge_ref.lora_delta(inp["a"], inp["b"], inp["s"], dtype)
        assert (np.abs(got.astype(np.float64) - twin) <= mc.one_ulp(dtype, got, twin, delta)).all(), "the envelope is off by more than one ulp"
        diff += int((got != twin).sum())
        total += got.size
    return diff, total


@pytest.mark.parametrize("bits", mc.BASES)
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_envelope_counts_are_the_recorded_ones(dtype, bits):
    diff, total = envelope_count(dtype, bits)
    print(f"ENVELOPE {dtype} bits {bits}: restate_f32 differs from the exact twin on {diff} of {total} elements")
    assert total == 127872
    assert diff == mc.ENVELOPE[dtype, bits]


def test_a_wrong_variant_changes_the_bits():
    """The factors multiplied before they are rounded to T, and the rank terms in descending j: both move elements of a
    random case, so the comparison against the twin does tell the variants apart."""
    N, K, r = 40, 320, 64
    for dtype in mc.DTYPES:
        inp = mc.random_inputs(N, K, r, dtype, 0)
        twin = merge_ref.merge_lora(inp["w"], inp["a"], inp["b"], inp["s"], dtype)
        right = mc.restate_f32(inp, dtype, 0)
        wrong = mc.restate_f32(inp, dtype, 0, sum_before_rounding=True)
        n_right, n_wrong = int((right != twin).sum()), int((wrong != twin).sum())
        print(f"{dtype}: right order differs on {n_right}, unrounded factors on {n_wrong} of {twin.size}")
        assert n_wrong > 100 * max(1, mc.RULE_CAP * n_right)
    # descending j: the float32 chain itself moves (before the rounding to T hides most of it)
    inp = mc.random_inputs(N, K, r, "float16", 0)
    bp, ap = merge_ref.factors(inp["a"], inp["b"], inp["s"], "float16")
    up = np.zeros((N, K), np.float32)
    down = np.zeros((N, K), np.float32)
    for j in range(r):
        up = (bp[:, j:j + 1] * ap[j:j + 1] + up).astype(np.float32)
        down = (bp[:, r - 1 - j:r - j] * ap[r - 1 - j:r - j] + down).astype(np.float32)
    assert (up != down).sum() > N * K // 4


def test_twin_quantised_base_round_trip():
    """step 6 on the twin: the re-quantised triple is ref_quant.quantize of the merged matrix, and a zero adapter on an exact
    base gives the base's own dequantised values back."""
    inp = mc.exact_inputs(17, 192, 7, "bfloat16", 4, False)
    from oracle.ref_model import Linear

    lin = Linear(dtype="bfloat16", packed=inp["packed"], scales=inp["scales"], biases=inp["biases"], bits=4)
    wd = merge_ref.dequant_T(inp["packed"], inp["scales"], inp["biases"], 4, "bfloat16")
    merge_ref.merge_linear(lin, inp["a"], np.zeros_like(inp["b"]), None, inp["s"], de_quantize=True)
    assert np.array_equal(lin.weight, wd) and lin.packed is None
    lin = Linear(dtype="bfloat16", packed=inp["packed"], scales=inp["scales"], biases=inp["biases"], bits=4)
    merge_ref.merge_linear(lin, inp["a"], inp["b"], None, inp["s"])
    want = ref_quant.quantize(merge_ref.merge_lora(wd, inp["a"], inp["b"], inp["s"], "bfloat16"), 64, 4, "bfloat16")
    assert all(np.array_equal(g, w) for g, w in zip((lin.packed, lin.scales, lin.biases), want)) and lin.weight is None


# ------------------------------------------------------------------------------------------------ the tool and the flags
def _adapter_dir(dst, keys, n_layers=1, extra=None):
    import torch
    from safetensors.torch import save_file

    dst.mkdir(parents=True, exist_ok=True)
    t = {}
    for key in keys:
        t[f"model.layers.1.{key}.lora_a"] = torch.zeros(64, 2)
        t[f"model.layers.1.{key}.lora_b"] = torch.zeros(2, 64)
    save_file(t, str(dst / "adapters.safetensors"))
    cfg = {"fine_tune_type": "lora", "num_layers": n_layers, "lora_parameters": {"rank": 2, "scale": 2.0, "dropout": 0.0, "keys": list(keys)}}
    cfg.update(extra or {})
    (dst / "adapter_config.json").write_text(json.dumps(cfg))
    return str(dst)


def test_tool_arguments_and_refusals(tmp_path):
    from mlx_parallm_amd.tools import merge_lora as tool
    from mlx_parallm_amd.utils import ModelNotFoundError

    p = tool.build_parser()
    ns = p.parse_args(["--base-model", "b", "--lora-path", "l", "--output-path", "o"])
    assert (ns.base_model, ns.lora_path, ns.output_path, ns.de_quantize, ns.device) == ("b", "l", "o", False, 0)
    assert p.parse_args(["--base-model", "b", "--lora-path", "l", "--output-path", "o", "--de-quantize"]).de_quantize is True
    for missing in (["--lora-path", "l", "--output-path", "o"], ["--base-model", "b", "--output-path", "o"], ["--base-model", "b", "--lora-path", "l"]):
        with pytest.raises(SystemExit):
            p.parse_args(missing)
    with pytest.raises(ModelNotFoundError):
        tool.merge(str(tmp_path / "nowhere"), "l", str(tmp_path / "o"))
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps({"model_type": "llama", "num_hidden_layers": 2}))
    with pytest.raises(ValueError, match="nothing is merged in place"):
        tool.merge(str(base), "l", str(base))
    full = tmp_path / "full"
    full.mkdir()
    (full / "x").write_text("x")
    with pytest.raises(ValueError, match="not an empty directory"):
        tool.merge(str(base), "l", str(full))
    with pytest.raises(ValueError, match="not quantised"):
        tool.merge(str(base), "l", str(tmp_path / "o"), de_quantize=True)
    with pytest.raises(SystemExit):                                                # main() turns a refusal into a usage error
        tool.main(["--base-model", str(base), "--lora-path", "l", "--output-path", str(base)])
    assert not (tmp_path / "o").exists()


def test_merge_refuses_names_before_any_device_work(tmp_path):
    """An expert key is NotImplementedError as Engine.set_lora's on that family, any other unknown projection too, a missing
    adapter directory FileNotFoundError: all name the projection / path and need no device."""
    import torch

    from mlx_parallm_amd.merge import merge_adapter_into_weights

    weights = {f"model.layers.1.{k}.weight": torch.zeros(64, 64, dtype=torch.bfloat16)
               for k in ("self_attn.q_proj", "block_sparse_moe.switch_mlp.gate_proj", "mlp.gate_proj")}
    cfg = {"model_type": "mixtral", "num_hidden_layers": 2}
    with pytest.raises(NotImplementedError, match=r"layers\.1\.block_sparse_moe\.switch_mlp\.gate_proj"):
        merge_adapter_into_weights(weights, cfg, _adapter_dir(tmp_path / "moe", ["self_attn.q_proj", "block_sparse_moe.switch_mlp.gate_proj"]))
    with pytest.raises(NotImplementedError, match=r"layers\.1\.mlp\.gate_proj"):      # the dense MLP names do not exist on that family
        merge_adapter_into_weights(weights, cfg, _adapter_dir(tmp_path / "mlp", ["mlp.gate_proj"]))
    with pytest.raises(NotImplementedError, match=r"layers\.1\.self_attn\.qkv_proj"):
        merge_adapter_into_weights(weights, dict(cfg, model_type="llama"), _adapter_dir(tmp_path / "qkv", ["self_attn.qkv_proj"]))
    with pytest.raises(FileNotFoundError):
        merge_adapter_into_weights(weights, cfg, str(tmp_path / "missing"))
    with pytest.raises(NotImplementedError, match="fine_tune_type"):
        merge_adapter_into_weights(weights, cfg, _adapter_dir(tmp_path / "full", ["self_attn.q_proj"], extra={"fine_tune_type": "full"}))
    assert all(float(t.abs().sum()) == 0 for t in weights.values())


def test_flags_refuse_at_start_up(tmp_path):
    from mlx_parallm_amd import cli, utils
    from mlx_parallm_amd.server.main import ServerConfig, create_app

    cfg = cli.parse_args(["--model-path", "m", "--lora-path", "a", "--merge-lora"])
    assert cfg.merge_lora is True and cfg.lora_path == "a"
    assert cli.parse_args(["--model-path", "m", "--lora-path", "a"]).merge_lora is False
    for bad in (["--model-path", "m", "--merge-lora"], ["--model-path", "m", "--merge-lora", "--lora-modules", "x=y"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    with pytest.raises(ValueError, match="merge_lora"):
        create_app(ServerConfig(model_path="m", merge_lora=True))
    with pytest.raises(ValueError, match="merge_lora"):
        create_app(ServerConfig(model_path="m", merge_lora=True, lora_modules={"x": "y"}))
    with pytest.raises(ValueError, match="adapter_path"):
        utils.load_model(tmp_path, merge_adapter=True)
    with pytest.raises(ValueError, match="merge_adapter=True"):
        utils.load_model(tmp_path, adapter_path="a")


def test_a_merged_model_refuses_further_adapters(tmp_path):
    from mlx_parallm_amd import utils, weight_updater

    class Merged:
        merged_adapter = "some/adapter"
        layers = [None, None]

    for call in (lambda: utils.load_adapters(Merged(), str(tmp_path)), lambda: utils.load_adapter_into(Merged(), 0, str(tmp_path)),
                 lambda: weight_updater.apply_lora_update(Merged(), str(tmp_path))):
        with pytest.raises(ValueError, match="merged into this model's weights"):
            call()
