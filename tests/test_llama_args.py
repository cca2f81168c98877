"""The three ModelArgs switches of llama.py that change the arithmetic of the forward pass -- attention_bias, mlp_bias,
rope_traditional (llama.py:29-32,59-67,77-82,155-162) -- on the CPU side: the model arguments accept them, the tiny-model
builder and the converter carry the `.bias` tensors, and the per-head permutation that lets the engine serve
rope_traditional with its half-split RoPE kernels is pinned in NumPy (no engine involved)."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from biased_ref import head_perm
from oracle.ref_model import rope, rope_tables

BIASED = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
          "mlp.down_proj")
BASE = {"model_type": "llama", "hidden_size": 64, "num_hidden_layers": 2, "intermediate_size": 128, "num_attention_heads": 4,
        "rms_norm_eps": 1e-6, "vocab_size": 128}


@pytest.mark.parametrize("flag", ["attention_bias", "mlp_bias", "rope_traditional"])
def test_model_args_accept_the_flag(flag):
    from mlx_parallm_amd.models.llama import ModelArgs

    args = ModelArgs.from_dict({**BASE, flag: True})
    assert getattr(args, flag) is True
    others = {"attention_bias", "mlp_bias", "rope_traditional"} - {flag}
    assert all(getattr(args, o) is False for o in others)


def test_model_args_accept_all_three_flags_together():
    from mlx_parallm_amd.models.llama import ModelArgs

    args = ModelArgs.from_dict({**BASE, "attention_bias": True, "mlp_bias": True, "rope_traditional": True})
    assert args.attention_bias and args.mlp_bias and args.rope_traditional


def _tiny(dst, **kw):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    return build_tiny_model(dst, seed=11, vocab_size=256, hidden_size=64, layers=2, heads=4, kv_heads=2, intermediate_size=128,
                            with_tokenizer=False, tie_word_embeddings=False, **kw)


@pytest.mark.parametrize("quantize_model", [False, True])
def test_tiny_model_writes_the_bias_tensors_and_the_config_flags(tmp_path, quantize_model):
    cfg = _tiny(tmp_path / "m", dtype="bfloat16", quantize_model=quantize_model, attention_bias=True, mlp_bias=True,
                rope_traditional=True)
    on_disk = json.loads((tmp_path / "m" / "config.json").read_text())
    for c in (cfg, on_disk):
        assert c["attention_bias"] is True and c["mlp_bias"] is True and c["rope_traditional"] is True
    w = load_file(str(tmp_path / "m" / "model.safetensors"))
    for i in range(2):
        names = [k for k in w if k.startswith(f"model.layers.{i}.") and k.endswith(".bias")]
        assert sorted(names) == sorted(f"model.layers.{i}.{p}.bias" for p in BIASED)
        for p in BIASED:
            b, wt = w[f"model.layers.{i}.{p}.bias"], w[f"model.layers.{i}.{p}.weight"]
            assert b.ndim == 1 and b.shape[0] == wt.shape[0] and b.dtype == torch.bfloat16
            # drawn so that they matter: about the RMS of the layer's outputs for unit-RMS inputs (U(-1/sqrt K, 1/sqrt K)
            # weights: sqrt(K) * 1/sqrt(3 K) = 0.58), not nn.Linear's vanishing U(-1/sqrt K, 1/sqrt K)
            assert 0.3 <= float(b.float().pow(2).mean().sqrt()) <= 1.0
    assert not any(k.endswith(".bias.scales") or k.endswith(".bias.biases") for k in w)
    # one flag alone gives its own four / three tensors per layer
    _tiny(tmp_path / "a", quantize_model=False, attention_bias=True)
    wa = load_file(str(tmp_path / "a" / "model.safetensors"))
    assert sorted(k for k in wa if k.endswith(".bias")) == sorted(f"model.layers.{i}.{p}.bias" for i in range(2) for p in BIASED[:4])
    # and none at all leaves the checkpoint of that seed as it was
    _tiny(tmp_path / "n", quantize_model=False)
    wn = load_file(str(tmp_path / "n" / "model.safetensors"))
    assert not any(k.endswith(".bias") for k in wn)
    assert all(torch.equal(wn[k], wa[k]) for k in wn)


@pytest.mark.parametrize("src_dtype", ["bfloat16", "float32"])
def test_convert_with_quantisation_leaves_the_bias_tensors_bit_identical(tmp_path, src_dtype):
    from mlx_parallm_amd.convert import convert

    _tiny(tmp_path / "src", dtype=src_dtype, quantize_model=False, attention_bias=True, mlp_bias=True)
    convert(str(tmp_path / "src"), str(tmp_path / "q4"), quantize=True, q_group_size=64, q_bits=4)
    a = load_file(str(tmp_path / "src" / "model.safetensors"))
    b = load_file(str(tmp_path / "q4" / "model.safetensors"))
    names = [k for k in a if k.endswith(".bias")]
    assert len(names) == 14
    for k in names:
        assert k in b and b[k].dtype == a[k].dtype and b[k].shape == a[k].shape
        assert b[k].view(torch.uint8).numpy().tobytes() == a[k].view(torch.uint8).numpy().tobytes(), k
        base = k[: -len(".bias")]
        assert b[base + ".weight"].dtype in (torch.uint32, torch.int32) and base + ".scales" in b and base + ".biases" in b
        assert k + ".scales" not in b
    assert json.loads((tmp_path / "q4" / "config.json").read_text())["attention_bias"] is True
    # ... and back: de-quantising does not touch them either, and a plain dtype conversion keeps their dtype
    convert(str(tmp_path / "q4"), str(tmp_path / "dq"), dequantize=True, dtype="float16")
    c = load_file(str(tmp_path / "dq" / "model.safetensors"))
    for k in names:
        assert c[k].dtype == a[k].dtype and torch.equal(c[k], a[k])


@pytest.mark.parametrize("D", [16, 64, 128])
def test_head_permutation_turns_the_interleaved_rotation_into_the_half_split_one(D):
    """rope_traditional rotates the pairs (2i, 2i+1) by pos * theta^(-2i/D).  With new[j] = old[pi[j]] (new[j] = old[2j],
    new[D/2 + j] = old[2j+1]) the oracle's half-split rope on (q[pi], k[pi]) gives the same rotated numbers in permuted
    places, hence the same q.k -- which pins the DIRECTION of pi (its inverse fails both assertions)."""
    rng = np.random.default_rng(D)
    B, H, L = 2, 3, 5
    q = rng.standard_normal((B, H, L, D))                       # float64
    k = rng.standard_normal((B, H, L, D))
    pos = rng.integers(0, 200, size=(B, L))
    cos, sin = rope_tables(D, 10000.0, 1.0, 256)
    pi = head_perm(D)
    assert sorted(pi.tolist()) == list(range(D)) and pi[0] == 0 and pi[1] == 2 and pi[D // 2] == 1

    def rope_interleaved(x):
        c, s = cos[pos][:, None, :, :], sin[pos][:, None, :, :]
        x1, x2 = x[..., 0::2], x[..., 1::2]
        out = np.empty_like(x)
        out[..., 0::2] = x1 * c - x2 * s
        out[..., 1::2] = x1 * s + x2 * c
        return out.astype(np.float32)                            # (the oracle's rope returns float32 arrays)

    qt, kt = rope_interleaved(q), rope_interleaved(k)
    qh, kh = rope(q[..., pi], "float32", pos, cos, sin), rope(k[..., pi], "float32", pos, cos, sin)
    assert np.array_equal(qt[..., pi], qh) and np.array_equal(kt[..., pi], kh)          # permutations of each other
    dots_t = np.einsum("bhld,bhmd->bhlm", qt.astype(np.float64), kt.astype(np.float64))
    dots_h = np.einsum("bhld,bhmd->bhlm", qh.astype(np.float64), kh.astype(np.float64))
    assert np.abs(dots_t - dots_h).max() <= 1e-12
    if D > 2:                                                     # the inverse permutation is another model
        inv = np.argsort(pi)
        assert not np.array_equal(qt[..., inv], rope(q[..., inv], "float32", pos, cos, sin))
