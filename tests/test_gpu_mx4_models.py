"""Tiny llama (tied embedding, GQA), qwen3 and phi3 checkpoints in MLX's mxfp4 mode through the engine (-m gpu).  Checkpoint A
holds quant.quantize_mxfp4 of every linear and of the embedding with "mode": "mxfp4"; checkpoint B is dense bf16 and holds
dequantize_mxfp4 of A, the identical weights, and the oracle loads B unchanged (phi3: B's Llama-form twin -- the oracle has no
phi3 -- and A the same quantised rows fused).  3 left-padded prompts of 140 tokens (420 rows: the prefill GEMM over the one-term
copy), then 16 teacher-forced greedy steps (gemm_mx4.hip in the 16-bit mode, the generic kernel in the float32-KV mode); a mixed
step.  Bounds: tests/test_gpu_q36_models.py::_check, which tests/test_gpu_qgroup_models.py uses."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import quant, tiny_model, utils  # noqa: E402
from mlx_parallm_amd.engine import Engine, SampleArgs  # noqa: E402
from oracle import ref_generate  # noqa: E402
from test_gpu_gqa_models import _assert_sequences  # noqa: E402
from test_gpu_q36_models import _adapter, _check  # noqa: E402

SHAPE = dict(vocab_size=512, hidden_size=128, layers=2, heads=4, kv_heads=2, intermediate_size=256, dtype="bfloat16",
             quantize_model=False, with_tokenizer=False)
QCFG = {"group_size": 32, "bits": 4, "mode": "mxfp4"}


def _pair(tmp, model_type):
    """-> (mxfp4 checkpoint A, its dense bf16 twin B, A's config)"""
    phi3 = model_type == "phi3"
    cfg = tiny_model.build_tiny_model(tmp / "b", seed=7, model_type="llama" if phi3 else model_type,
                                      tie_word_embeddings=model_type == "llama", **SHAPE)
    dense = load_file(str(tmp / "b" / "model.safetensors"))
    a = dict(dense)
    for k in [k for k, t in dense.items() if k.endswith(".weight") and t.ndim == 2]:
        a[k], a[k[:-7] + ".scales"] = quant.quantize_mxfp4(dense[k])
        dense[k] = quant.dequantize_mxfp4(a[k], a[k[:-7] + ".scales"]).to(torch.bfloat16)
    if phi3:
        a, cfg = tiny_model.fuse_phi3(a), tiny_model.phi3_config(cfg)
    cfg = dict(cfg, quantization=QCFG, quantization_config=QCFG)
    (tmp / "a").mkdir()
    save_file(a, str(tmp / "a" / "model.safetensors"), metadata={"format": "mlx"})
    save_file(dense, str(tmp / "b" / "model.safetensors"), metadata={"format": "mlx"})
    (tmp / "a" / "config.json").write_text(json.dumps(cfg))
    return tmp / "a", tmp / "b", cfg


@pytest.mark.parametrize("mode", ["model", "float32"])
@pytest.mark.parametrize("model_type,lora", [("llama", False), ("llama", True), ("qwen3", False), ("phi3", False)])
def test_tiny_models(tmp_path, model_type, lora, mode):
    a, b, cfg = _pair(tmp_path, model_type)
    ad = _adapter(tmp_path / "adapter", cfg) if lora else None
    model = utils.load_model(Path(a), max_positions=512)
    assert model.engine.desc.quant_mode == 1
    if lora:
        utils.load_adapters(model, ad)
    _check(model, ref_generate.load(str(b), adapter_path=ad, max_pos=512), cfg, mode)
    model.engine.close()


def test_mixed_step_16bit_kv(tmp_path):
    """mi_step_enqueue_mixed in the 16-bit mode: a 40-token prompt enters row 0 in chunks of 16 / 16 / 8 tokens while rows 1 and 2
    decode in the same steps (18 / 18 / 10-row linears with L != 1 on gemm_mx4.hip).  The rule of
    tests/test_gpu_gqa_models.py::test_chunked_prefill_next_to_two_decode_rows: every sequence produces what it produces alone
    (a differing token only at an oracle margin <= 0.13, the bound of _check), inner chunks return nothing."""
    a, b, cfg = _pair(tmp_path, "llama")
    eng, ref = utils.load_model(Path(a), max_positions=512).engine, ref_generate.load(str(b), max_pos=512)
    rng = np.random.default_rng(23)
    P = {nm: rng.integers(3, cfg["vocab_size"], size=n) for nm, n in (("A", 9), ("B", 6), ("C", 40))}
    kv, got = eng.new_kv(3, capacity=64, kv_dtype="model"), {k: [] for k in P}

    def mixed(rows, names, toks, want):
        res = eng.step_wait(eng.step_enqueue_mixed(kv, rows, toks, want, SampleArgs(temp=0.0)), sum(want))
        for nm, t in zip([n for n, w in zip(names, want) if w], res["tokens"]):
            got[nm].append(int(t))

    mixed([1, 2], ["A", "B"], [P["A"], P["B"]], [1, 1])
    for lo, hi in ((0, 16), (16, 32), (32, 40)):
        mixed([1, 2, 0], ["A", "B", "C"], [[got["A"][-1]], [got["B"][-1]], P["C"][lo:hi]], [1, 1, int(hi == 40)])
        assert kv.offsets == [hi, 9 + len(got["A"]) - 1, 6 + len(got["B"]) - 1] and len(got["C"]) == int(hi == 40)
    for _ in range(3):
        mixed([0, 1, 2], ["C", "A", "B"], [[got["C"][-1]], [got["A"][-1]], [got["B"][-1]]], [1, 1, 1])
    _assert_sequences(ref, P, got, False)
    kv.close(); eng.close()


@pytest.mark.parametrize("case", ["biases", "nvfp4", "f16", "mixtral", "group64"])
def test_refusals(tmp_path, case):
    a, _, cfg = _pair(tmp_path, "llama")
    if case == "biases":                                 # a `.biases` tensor for an mxfp4 linear: MI_ERR_INVALID
        eng = Engine(cfg, device=0, max_positions=64, act_dtype="bfloat16")
        with pytest.raises(ValueError, match="no biases"):
            eng.set_tensor("model.layers.0.mlp.down_proj.biases", torch.zeros((128, 8), dtype=torch.bfloat16))
        eng.close()
        return
    bad = {"nvfp4": dict(cfg, quantization=dict(QCFG, mode="nvfp4")), "f16": cfg,
           "mixtral": dict(cfg, model_type="mixtral", tie_word_embeddings=False),
           "group64": dict(cfg, quantization=dict(QCFG, group_size=64))}[case]
    match = {"nvfp4": "nvfp4", "f16": "act_dtype", "mixtral": "ixtral", "group64": "quant_group_size 32"}[case]
    with pytest.raises(NotImplementedError, match=match):
        Engine(bad, device=0, max_positions=64, act_dtype="float16" if case == "f16" else "bfloat16")
