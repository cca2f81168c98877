"""Tiny llama checkpoints at 3 and 6 bits through the engine (-m gpu): a batch of 3 left-padded prompts of 140 tokens (420
rows: the prefill goes through the [hi | lo] copy of the bit planes), then 16 teacher-forced greedy steps (gemm_q36.hip in the
16-bit mode, the generic kernel's bit-plane unpack in the float32-KV mode), tied embedding (the gather's unpack).

The oracle cannot unpack 3 / 6 bits: it gets the SAME codes re-packed at 4 / 8 bits with the same scales and biases -- W_hat
is identical (tests/test_quant36_host.py), so the function is.  Bounds: float32-KV ids equal and logprobs within 1e-3; 16-bit
mode those of tests/test_gpu_engine.py::test_greedy_model_dtype_kv_16bit_models (lines 250-262)."""
import json
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import merge, quant, utils  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from oracle import ref_generate  # noqa: E402
from test_gpu_engine import MODEL_KV_LOGPROB_TOL, _teacher_forced_greedy  # noqa: E402

WIDE = {3: 4, 6: 8}
SHAPE = dict(vocab_size=512, hidden_size=128, layers=2, heads=4, kv_heads=2, intermediate_size=256, tie_word_embeddings=True)


def _dirs(tmp, bits, dtype):
    """-> (the 3- / 6-bit checkpoint, the same codes at 4 / 8 bits for the oracle, config)"""
    cfg = build_tiny_model(tmp / "q", seed=bits, dtype=dtype, quantize_model=True, q_bits=bits, **SHAPE)
    shutil.copytree(tmp / "q", tmp / "wide")
    w = load_file(str(tmp / "wide" / "model.safetensors"))
    for k in [k for k in w if k.endswith(".scales")]:
        name = k[:-7] + ".weight"
        w[name] = quant.pack_codes(quant.unpack_codes(w[name], bits), WIDE[bits])
    save_file(w, str(tmp / "wide" / "model.safetensors"), metadata={"format": "mlx"})
    wide_cfg = dict(cfg, quantization={"group_size": 64, "bits": WIDE[bits]})
    (tmp / "wide" / "config.json").write_text(json.dumps(wide_cfg, indent=4, sort_keys=True))
    return str(tmp / "q"), str(tmp / "wide"), cfg


def _adapter(dst, cfg):
    """rank 8 on q|k|v and down of every block (the recipe of test_gpu_engine.py::test_lora_adapter_applied, scale 10)"""
    H, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["hidden_size"] // cfg["num_attention_heads"]
    dims = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, cfg["num_key_value_heads"] * D),
            "self_attn.v_proj": (H, cfg["num_key_value_heads"] * D), "mlp.down_proj": (I, H)}
    rng, w = np.random.default_rng(5), {}
    for i in range(cfg["num_hidden_layers"]):
        for key, (K, n) in dims.items():
            w[f"model.layers.{i}.{key}.lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (K, 8)) / np.sqrt(K)).astype(np.float32))
            w[f"model.layers.{i}.{key}.lora_b"] = torch.from_numpy((rng.standard_normal((8, n)) * 0.05).astype(np.float32))
    dst.mkdir()
    save_file(w, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": cfg["num_hidden_layers"],
        "lora_parameters": {"rank": 8, "scale": 10.0, "dropout": 0.0, "keys": list(dims)}}))
    return str(dst)


def _check(model, ref, cfg, mode):
    if mode == "float32":
        near, total, lp = _teacher_forced_greedy(model, ref, cfg, "float32", True, B=3, L0=140, steps=16, margin_eps=0.0)
        assert near == 0 and lp <= 1e-3, (near, total, lp)
    else:
        near, total, lp = _teacher_forced_greedy(model, ref, cfg, "model", False, B=3, L0=140, steps=16, margin_eps=0.13)
        assert near <= max(2, total // 10) and lp <= MODEL_KV_LOGPROB_TOL, (near, total, lp)


@pytest.mark.parametrize("mode", ["model", "float32"])
@pytest.mark.parametrize("bits,dtype,lora", [(3, "bfloat16", False), (6, "bfloat16", False), (6, "float16", False), (6, "bfloat16", True)])
def test_tiny_llama(tmp_path, bits, dtype, lora, mode):
    q, wide, cfg = _dirs(tmp_path, bits, dtype)
    ad = _adapter(tmp_path / "adapter", cfg) if lora else None
    model = utils.load_model(Path(q), max_positions=512)
    if lora:
        utils.load_adapters(model, ad)
    ref = ref_generate.load(wide, adapter_path=ad, max_pos=512)
    _check(model, ref, cfg, mode)
    model.engine.close()


def test_refusals(tmp_path):
    """Mixtral experts and mi_lora_merge stay at 4 / 8 bits: MI_ERR_UNSUPPORTED from the library, NotImplementedError above it"""
    import ctypes as C

    from mlx_parallm_amd import _lib as L
    from mlx_parallm_amd.engine import Engine
    lib = L.lib()
    q, _, cfg = _dirs(tmp_path, 6, "bfloat16")
    eng = Engine(cfg, device=0, max_positions=64, act_dtype="bfloat16")
    d = type(eng.desc).from_buffer_copy(eng.desc)               # a valid 6-bit description, turned into a Mixtral's
    eng.close()
    d.arch, d.tie_word_embeddings, d.num_local_experts, d.num_experts_per_tok = L.MI_ARCH_MIXTRAL, 0, 4, 2
    h = C.c_void_p()
    assert lib.mi_engine_create(C.byref(d), 0, C.byref(h)) == -3 and b"grouped expert kernels" in lib.mi_last_error()
    with pytest.raises(NotImplementedError, match="4 or 8 bits"):
        Engine(dict(cfg, model_type="mixtral", tie_word_embeddings=False), device=0, max_positions=64, act_dtype="bfloat16")
    N, K, r = 16, 64, 4
    t = {"w": torch.zeros((N, K * 6 // 32), dtype=torch.int32), "s": torch.ones((N, 1), dtype=torch.bfloat16),
         "b": torch.zeros((N, 1), dtype=torch.bfloat16), "A": torch.zeros((K, r)), "B": torch.zeros((r, N)),
         "o": torch.zeros((N, K), dtype=torch.bfloat16)}
    t = {k: v.cuda() for k, v in t.items()}
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    torch.cuda.synchronize()
    rc = lib.mi_lora_merge(0, N, K, r, L.MI_BF16, 6, 64, p["w"], p["s"], p["b"], p["A"], p["B"], None, 1.0, 0, p["o"], None, None)
    assert rc == -3 and b"6-bit base" in lib.mi_last_error(), (rc, lib.mi_last_error())
    with pytest.raises(NotImplementedError, match="6-bit base"):
        merge.merge_adapter_into_weights(load_file(q + "/model.safetensors"), cfg, _adapter(tmp_path / "adapter", cfg))
