"""Tiny llama (tied embedding), qwen3 and phi3 checkpoints in MLX's mxfp8 mode through the engine (-m gpu), the pattern of
tests/test_gpu_mx4_models.py: A = quantize_mxfp8 of every linear and the embedding, B = its dense bf16 dequantisation, which the
oracle loads unchanged.  Bounds: tests/test_gpu_q36_models.py::_check."""
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
from test_gpu_mx4_models import SHAPE  # noqa: E402
from test_gpu_q36_models import _adapter, _check  # noqa: E402

QCFG = {"group_size": 32, "bits": 8, "mode": "mxfp8"}


def _pair(tmp, model_type):
    phi3 = model_type == "phi3"
    cfg = tiny_model.build_tiny_model(tmp / "b", seed=7, model_type="llama" if phi3 else model_type,
                                      tie_word_embeddings=model_type == "llama", **SHAPE)
    dense = load_file(str(tmp / "b" / "model.safetensors"))
    a = dict(dense)
    for k in [k for k, t in dense.items() if k.endswith(".weight") and t.ndim == 2]:
        a[k], a[k[:-7] + ".scales"] = quant.quantize_mxfp8(dense[k])
        dense[k] = quant.dequantize_mxfp8(a[k], a[k[:-7] + ".scales"]).to(torch.bfloat16)
    if phi3:
        a, cfg = tiny_model.fuse_phi3(a), tiny_model.phi3_config(cfg)
    cfg = dict(cfg, quantization=QCFG, quantization_config=QCFG)
    (tmp / "a").mkdir()
    for d, w in (("a", a), ("b", dense)):
        save_file(w, str(tmp / d / "model.safetensors"), metadata={"format": "mlx"})
    (tmp / "a" / "config.json").write_text(json.dumps(cfg))
    return tmp / "a", tmp / "b", cfg


@pytest.mark.parametrize("mode", ["model", "float32"])
@pytest.mark.parametrize("model_type,lora", [("llama", False), ("llama", True), ("qwen3", False), ("phi3", False)])
def test_tiny_models(tmp_path, model_type, lora, mode):
    a, b, cfg = _pair(tmp_path, model_type)
    ad = _adapter(tmp_path / "adapter", cfg) if lora else None
    model = utils.load_model(Path(a), max_positions=512)
    assert model.engine.desc.quant_mode == 2
    if lora:
        utils.load_adapters(model, ad)
    _check(model, ref_generate.load(str(b), adapter_path=ad, max_pos=512), cfg, mode)
    model.engine.close()


def test_mixed_step_16bit_kv(tmp_path):
    """a 40-token prompt enters row 0 in chunks while rows 1 and 2 decode in the same steps (18 / 18 / 10-row linears on gemm_mx8.hip)"""
    a, b, cfg = _pair(tmp_path, "llama")
    eng, ref = utils.load_model(Path(a), max_positions=512).engine, ref_generate.load(str(b), max_pos=512)
    assert eng.desc.quant_mode == 2
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


@pytest.mark.parametrize("case", ["f16", "group64", "bits4", "mixtral"])
def test_refusals(tmp_path, case):
    cfg = _pair(tmp_path, "llama")[2]
    bad = {"f16": cfg, "group64": dict(cfg, quantization=dict(QCFG, group_size=64)),
           "bits4": dict(cfg, quantization=dict(QCFG, bits=4)),
           "mixtral": dict(cfg, model_type="mixtral", tie_word_embeddings=False)}[case]
    match = {"f16": "act_dtype", "group64": "quant_group_size 32", "bits4": "mxfp8.*bits 8", "mixtral": "ixtral"}[case]
    with pytest.raises(NotImplementedError, match=match):
        Engine(bad, device=0, max_positions=64, act_dtype="float16" if case == "f16" else "bfloat16")
