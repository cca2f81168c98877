"""Build a small local checkpoint for smoke tests -- the job of the reference's
``scripts/build_tiny_model.py`` (defaults :108-118: hidden 64, 8 layers, 4 heads, 4 kv heads,
intermediate 128, rope_theta 1e4, tied embeddings, int4 group 64; vocab fallback 151936 :125;
rms_norm_eps 1e-6 :89) without MLX:

  * weights are drawn with a seeded NumPy generator using MLX's layer initialisers
    (nn.Linear: U(-1/sqrt(K), 1/sqrt(K)); nn.Embedding: N(0, 1/sqrt(H)); RMSNorm: ones) --
    ``mx.random.seed`` streams cannot be reproduced, so the VALUES differ from a reference-built
    tiny model while the architecture, dtypes and file format are the same;
  * ``model.safetensors`` carries ``metadata={"format": "mlx"}`` (utils.py:870) and, when
    quantised, the ``.weight``(uint32)/``.scales``/``.biases`` triples of ``nn.quantize``;
    ``config.json`` carries ``quantization`` + ``quantization_config`` (build_tiny_model.py:98-100);
  * the reference copies tokenizer files from ``models/hermes-qwen3-14b-4bit`` (git-ignored and
    absent); here a byte-level tokenizer is generated instead (``build_byte_tokenizer``).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

from .quant import quantize

_TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}

CHATML_TEMPLATE = (
    "{% for message in messages %}{{ '<|im_start|>' + message['role'] + '\n' + message['content'] + '<|im_end|>' + '\n' }}"
    "{% endfor %}{% if add_generation_prompt %}{{ '<|im_start|>assistant\n' }}{% endif %}"
)


def build_config(*, model_type: str, vocab_size: int, hidden_size: int, num_hidden_layers: int,
                 intermediate_size: int, num_attention_heads: int, num_key_value_heads: Optional[int],
                 rope_theta: float, tie_word_embeddings: bool, quantization: Optional[Dict[str, Any]],
                 head_dim: Optional[int] = None, rms_norm_eps: float = 1e-6,
                 max_position_embeddings: int = 4096, attention_bias: bool = False, mlp_bias: bool = False,
                 rope_traditional: bool = False, num_local_experts: Optional[int] = None,
                 num_experts_per_tok: Optional[int] = None) -> Dict[str, Any]:
    """build_tiny_model.py:70-101 (+ head_dim / max_position_embeddings for qwen3, the three ModelArgs switches
    of llama.py:29-32, and the two expert counts of mixtral.py:20,22 for model_type "mixtral")."""
    cfg: Dict[str, Any] = {
        "model_type": model_type,
        "hidden_size": int(hidden_size),
        "num_hidden_layers": int(num_hidden_layers),
        "intermediate_size": int(intermediate_size),
        "num_attention_heads": int(num_attention_heads),
        "num_key_value_heads": int(num_key_value_heads) if num_key_value_heads else int(num_attention_heads),
        "rms_norm_eps": float(rms_norm_eps),
        "vocab_size": int(vocab_size),
        "rope_theta": float(rope_theta),
        "rope_traditional": bool(rope_traditional),
        "rope_scaling": None,
        "attention_bias": bool(attention_bias),
        "mlp_bias": bool(mlp_bias),
        "tie_word_embeddings": bool(tie_word_embeddings),
        "max_position_embeddings": int(max_position_embeddings),
    }
    if model_type == "qwen3" or head_dim is not None:
        cfg["head_dim"] = int(head_dim or hidden_size // num_attention_heads)
    if model_type == "mixtral":
        cfg["num_local_experts"] = int(num_local_experts)
        cfg["num_experts_per_tok"] = int(num_experts_per_tok)
    if quantization is not None:
        cfg["quantization"] = dict(quantization)
        cfg["quantization_config"] = dict(quantization)
    return cfg


def init_weights(cfg: Dict[str, Any], seed: int = 0, dtype: str = "float32", norm_jitter: float = 0.0,
                 weight_std: Optional[float] = None, router_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Random weights keyed like an MLX / HF checkpoint.  ``weight_std``: N(0, std) instead of
    the MLX initialisers (SURVEY §8d synthetic weights).  With ``attention_bias`` / ``mlp_bias`` in ``cfg`` the
    projections get a 1-D ``.bias`` each, drawn at about the RMS of the layer's outputs for inputs of unit RMS
    (|W x| ~ sqrt(K) x the RMS of W's entries) -- nn.Linear's own U(-1/sqrt(K), 1/sqrt(K)) would vanish against it."""
    rng = np.random.default_rng(seed)
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    D = cfg.get("head_dim") or H // nh
    tdt = _TORCH_DT[dtype]

    def lin(n, k):
        if weight_std is not None:
            a = rng.standard_normal((n, k), dtype=np.float32) * np.float32(weight_std)
        else:
            s = 1.0 / np.sqrt(k)
            a = rng.uniform(-s, s, size=(n, k)).astype(np.float32)
        return torch.from_numpy(a).to(tdt)

    def bias(weight):
        n, k = weight.shape
        s = float(weight.to(torch.float32).pow(2).mean().sqrt()) * np.sqrt(k)
        return torch.from_numpy((rng.standard_normal(n, dtype=np.float32) * np.float32(s))).to(tdt)

    def norm(n):
        a = np.ones(n, dtype=np.float32)
        if norm_jitter:
            a = a + norm_jitter * rng.standard_normal(n).astype(np.float32)
        return torch.from_numpy(a).to(tdt)

    w: Dict[str, torch.Tensor] = {}
    std = weight_std if weight_std is not None else 1.0 / np.sqrt(H)
    w["model.embed_tokens.weight"] = torch.from_numpy(
        (rng.standard_normal((V, H), dtype=np.float32) * np.float32(std))).to(tdt)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        w[p + "self_attn.q_proj.weight"] = lin(nh * D, H)
        w[p + "self_attn.k_proj.weight"] = lin(nkv * D, H)
        w[p + "self_attn.v_proj.weight"] = lin(nkv * D, H)
        w[p + "self_attn.o_proj.weight"] = lin(H, nh * D)
        if cfg["model_type"] == "qwen3":
            w[p + "self_attn.q_norm.weight"] = norm(D)
            w[p + "self_attn.k_norm.weight"] = norm(D)
        if cfg["model_type"] == "mixtral":
            # the stacked form of mixtral.py:198-215: the router (scaled by router_gain, which spreads the gate logits) and
            # SwitchGLU's three tensors, every expert drawn like the dense MLP's matrices
            E = cfg["num_local_experts"]
            m = p + "block_sparse_moe."
            w[m + "gate.weight"] = (lin(E, H).to(torch.float32) * float(router_gain)).to(tdt)
            w[m + "switch_mlp.gate_proj.weight"] = torch.stack([lin(I, H) for _ in range(E)])
            w[m + "switch_mlp.down_proj.weight"] = torch.stack([lin(H, I) for _ in range(E)])
            w[m + "switch_mlp.up_proj.weight"] = torch.stack([lin(I, H) for _ in range(E)])
        else:
            w[p + "mlp.gate_proj.weight"] = lin(I, H)
            w[p + "mlp.down_proj.weight"] = lin(H, I)
            w[p + "mlp.up_proj.weight"] = lin(I, H)
        w[p + "input_layernorm.weight"] = norm(H)
        w[p + "post_attention_layernorm.weight"] = norm(H)
    w["model.norm.weight"] = norm(H)
    if not cfg["tie_word_embeddings"]:
        w["lm_head.weight"] = lin(V, H)
    # (drawn after every weight, so that the weights of a seed do not depend on the bias flags)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        projs = (["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj"] if cfg.get("attention_bias") else []) + \
                (["mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"] if cfg.get("mlp_bias") else [])
        for name in projs:
            w[p + name + ".bias"] = bias(w[p + name + ".weight"])
    return w


def quantize_weights(w: Dict[str, torch.Tensor], group_size: int, bits: int) -> Dict[str, torch.Tensor]:
    """``nn.quantize``: every Linear and Embedding (2-D ``.weight``) becomes a packed triple."""
    out: Dict[str, torch.Tensor] = {}
    for k, t in w.items():
        if k.endswith(".weight") and t.ndim == 2 and t.shape[1] % group_size == 0:
            base = k[: -len(".weight")]
            packed, scales, biases = quantize(t, group_size, bits)
            out[base + ".weight"] = packed
            out[base + ".scales"] = scales
            out[base + ".biases"] = biases
        else:
            out[k] = t
    return out


_PHI3_FUSED = (("self_attn.qkv_proj", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")),
               ("mlp.gate_up_proj", ("mlp.gate_proj", "mlp.up_proj")))


def fuse_phi3(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A Llama-form checkpoint (dense or quantised) in Phi-3 form: ``qkv_proj`` = q, then k, then v along the rows,
    ``gate_up_proj`` = gate, then up (phi3.py:56-57,93-95,120,125).  Quantisation groups run along K, so stacking rows
    of codes, scales and biases is quantising the stacked matrix."""
    out = dict(w)
    layers = sorted({int(k.split(".")[2]) for k in w if k.startswith("model.layers.")})
    for i in layers:
        p = f"model.layers.{i}."
        for fused, parts in _PHI3_FUSED:
            for suf in (".weight", ".scales", ".biases"):
                if p + parts[0] + suf in w:
                    out[p + fused + suf] = torch.cat([out.pop(p + name + suf) for name in parts], dim=0)
    return out


def split_phi3(w: Dict[str, torch.Tensor], cfg: Dict[str, Any]) -> Dict[str, torch.Tensor]:
    """The inverse of ``fuse_phi3`` for the geometry in ``cfg``: the Llama-form twin of a Phi-3 checkpoint."""
    nh = int(cfg["num_attention_heads"])
    nkv = int(cfg.get("num_key_value_heads") or nh)
    D = int(cfg["hidden_size"]) // nh
    rows = {"self_attn.qkv_proj": [nh * D, nkv * D, nkv * D], "mlp.gate_up_proj": [int(cfg["intermediate_size"])] * 2}
    out = dict(w)
    for k in list(w):
        for fused, parts in _PHI3_FUSED:
            for suf in (".weight", ".scales", ".biases"):
                if k.endswith(fused + suf):
                    for name, t in zip(parts, torch.split(out.pop(k), rows[fused], dim=0)):
                        out[k[: -len(fused + suf)] + name + suf] = t.contiguous()
    return out


def phi3_config(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The key set of a Phi-3 ``config.json`` (phi3.py:11-25): no ``head_dim``, no ``tie_word_embeddings``, no bias flags."""
    keys = ("hidden_size", "num_hidden_layers", "intermediate_size", "num_attention_heads", "num_key_value_heads",
            "rms_norm_eps", "vocab_size", "rope_theta", "rope_traditional", "rope_scaling", "max_position_embeddings",
            "quantization", "quantization_config")
    out = {k: cfg[k] for k in keys if k in cfg}
    out["model_type"] = "phi3"
    out["original_max_position_embeddings"] = int(cfg["max_position_embeddings"])
    return out


_MIXTRAL_EXPERT_NAMES = (("gate_proj", "w1"), ("down_proj", "w2"), ("up_proj", "w3"))      # mixtral.py:203


def unstack_experts(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A Mixtral checkpoint in the stacked form (``block_sparse_moe.switch_mlp.*``, 3-D) in the per-expert form of the
    original checkpoints (``block_sparse_moe.experts.<e>.{w1,w2,w3}``, 2-D): the inverse of mixtral.py:198-215."""
    out: Dict[str, torch.Tensor] = {}
    for k, t in w.items():
        for stacked, single in _MIXTRAL_EXPERT_NAMES:
            tag = f".block_sparse_moe.switch_mlp.{stacked}.weight"
            if k.endswith(tag):
                for e in range(t.shape[0]):
                    out[f"{k[: -len(tag)]}.block_sparse_moe.experts.{e}.{single}.weight"] = t[e].contiguous()
                break
        else:
            out[k] = t
    return out


def stack_experts(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of ``unstack_experts`` (what the reference's ``sanitize`` does)."""
    out = {k: t for k, t in w.items() if ".block_sparse_moe.experts." not in k}
    groups: Dict[str, Dict[int, torch.Tensor]] = {}
    for k, t in w.items():
        if ".block_sparse_moe.experts." in k:
            head, rest = k.split(".block_sparse_moe.experts.")
            e, single, _ = rest.split(".")
            stacked = {s: n for n, s in _MIXTRAL_EXPERT_NAMES}[single]
            groups.setdefault(f"{head}.block_sparse_moe.switch_mlp.{stacked}.weight", {})[int(e)] = t
    for k, parts in groups.items():
        out[k] = torch.stack([parts[e] for e in range(len(parts))])
    return out


def build_byte_tokenizer(dst: Path) -> int:
    """Writes a byte-level HF fast tokenizer (256 byte tokens + <|endoftext|>, <|im_start|>,
    <|im_end|>) with a ChatML template.  Returns its vocabulary size."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    alphabet = sorted(pre_tokenizers.ByteLevel.alphabet())
    vocab = {ch: i for i, ch in enumerate(alphabet)}
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    tok.decoder = decoders.ByteLevel()
    fast = PreTrainedTokenizerFast(
        tokenizer_object=tok, eos_token="<|endoftext|>",
        additional_special_tokens=["<|im_start|>", "<|im_end|>"],
    )
    fast.chat_template = CHATML_TEMPLATE
    dst.mkdir(parents=True, exist_ok=True)
    fast.save_pretrained(str(dst))
    return len(fast)


def build_tiny_model(dst, *, seed: int = 0, model_type: str = "llama", hidden_size: int = 64, layers: int = 8,
                     heads: int = 4, kv_heads: int = 4, intermediate_size: int = 128, rope_theta: float = 10000.0,
                     tie_word_embeddings: bool = True, quantize_model: bool = True, q_bits: int = 4,
                     q_group_size: int = 64, vocab_size: Optional[int] = None, dtype: str = "float32",
                     head_dim: Optional[int] = None, with_tokenizer: bool = True, norm_jitter: float = 0.0,
                     weight_std: Optional[float] = None, rms_norm_eps: float = 1e-6,
                     max_position_embeddings: int = 4096, attention_bias: bool = False, mlp_bias: bool = False,
                     rope_traditional: bool = False, num_local_experts: int = 4, num_experts_per_tok: int = 2,
                     expert_names: str = "stacked", router_gain: float = 1.0) -> Dict[str, Any]:
    """scripts/build_tiny_model.py:104-160.  Returns the config dict it wrote.

    ``model_type="mixtral"``: ``num_local_experts`` experts of ``intermediate_size`` each, ``num_experts_per_tok`` of them per
    token; ``expert_names`` = "stacked" (``switch_mlp.*``, 3-D) or "per_expert" (``experts.<e>.{w1,w2,w3}``, the same numbers);
    ``router_gain`` scales the router's weights.  Dense 16-bit only: pass ``quantize_model=False`` and a 16-bit ``dtype``."""
    from safetensors.torch import save_file

    dst = Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    phi3 = model_type == "phi3"
    if phi3:
        # models/phi3.py: no linear biases, an lm_head of its own, head_dim = hidden_size // heads.  The tensors are those
        # that model_type="llama" draws with the same arguments; q|k|v and gate|up are written as one matrix each.
        if tie_word_embeddings or attention_bias or mlp_bias:
            raise ValueError("phi3 has neither a tied lm_head nor linear biases: pass tie_word_embeddings=False")
        if head_dim is not None and head_dim != hidden_size // heads:
            raise ValueError("phi3: head_dim is hidden_size // heads")
        model_type, head_dim = "llama", None
    mixtral = model_type == "mixtral"
    if mixtral:
        if quantize_model or dtype == "float32":
            raise ValueError("mixtral: dense bfloat16 / float16 checkpoints only (quantize_model=False, a 16-bit dtype)")
        if tie_word_embeddings or attention_bias or mlp_bias:
            raise ValueError("mixtral has neither a tied lm_head nor linear biases: pass tie_word_embeddings=False")
        if expert_names not in ("stacked", "per_expert"):
            raise ValueError("expert_names is 'stacked' or 'per_expert'")
        if head_dim is not None and head_dim != hidden_size // heads:
            raise ValueError("mixtral: head_dim is hidden_size // heads")
        head_dim = None
    tok_vocab = build_byte_tokenizer(dst) if with_tokenizer else 0
    if vocab_size is None:
        vocab_size = 151936                                  # build_tiny_model.py:125 fallback
    if vocab_size < tok_vocab:
        raise ValueError(f"vocab_size {vocab_size} smaller than the tokenizer's {tok_vocab}")
    quant = {"group_size": int(q_group_size), "bits": int(q_bits)} if quantize_model else None
    cfg = build_config(model_type=model_type, vocab_size=vocab_size, hidden_size=hidden_size,
                       num_hidden_layers=layers, intermediate_size=intermediate_size,
                       num_attention_heads=heads, num_key_value_heads=kv_heads, rope_theta=rope_theta,
                       tie_word_embeddings=tie_word_embeddings, quantization=quant, head_dim=head_dim,
                       rms_norm_eps=rms_norm_eps, max_position_embeddings=max_position_embeddings,
                       attention_bias=attention_bias, mlp_bias=mlp_bias, rope_traditional=rope_traditional,
                       num_local_experts=num_local_experts, num_experts_per_tok=num_experts_per_tok)
    w = init_weights(cfg, seed=seed, dtype=dtype, norm_jitter=norm_jitter, weight_std=weight_std, router_gain=router_gain)
    if mixtral and expert_names == "per_expert":
        w = unstack_experts(w)
    if quantize_model:
        w = quantize_weights(w, q_group_size, q_bits)
    if phi3:
        w = fuse_phi3(w)
        cfg = phi3_config(cfg)
    save_file({k: v.contiguous() for k, v in w.items()}, str(dst / "model.safetensors"), metadata={"format": "mlx"})
    (dst / "config.json").write_text(json.dumps(cfg, indent=4, sort_keys=True))   # utils.save_config sorts keys
    return cfg
