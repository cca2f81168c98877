"""Mixtral model handle (mirror of ``mlx_parallm/models/mixtral.py``).

The attention half of a block is Mistral's (RMSNorm, RoPE, SDPA, no linear biases, an untied ``lm_head``); the MLP half is
the sparse mixture of experts of mixtral.py:95-119: a router picks ``num_experts_per_tok`` of ``num_local_experts`` SwiGLU
experts per token and sums their outputs under the softmax of the picked router logits.  The engine runs it on the device
(``MI_ARCH_MIXTRAL``, csrc/moe.hip); a tie between router logits goes to the lower expert index (``mx.argpartition`` leaves the
order open).

Checkpoints: dense bfloat16 / float16 only, in either name form -- the stacked ``block_sparse_moe.switch_mlp.*`` tensors that
the reference's ``sanitize`` produces, or the per-expert ``block_sparse_moe.experts.<e>.{w1,w3,w2}`` tensors of the original
checkpoints, which the engine copies into their slots one by one (nothing is stacked on the host).  ``rope_scaling`` is
ignored, as mixtral.py:57-61 ignores it; ``head_dim`` is ``hidden_size // num_attention_heads`` (mixtral.py:38).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Union

from .base import BaseModelArgs
from .llama import Model as _LlamaModel


@dataclass
class ModelArgs(BaseModelArgs):                                                # mixtral.py:12-31
    model_type: str
    vocab_size: int = 32000
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_experts_per_tok: int = 2
    num_key_value_heads: int = 8
    num_local_experts: int = 8
    rms_norm_eps: float = 1e-5
    rope_theta: float = 1e6
    rope_traditional: bool = False
    rope_scaling: Optional[Dict[str, Union[float, str]]] = None

    def __post_init__(self):
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads


class Model(_LlamaModel):
    _ARCH = "mixtral"

    def __init__(self, args: ModelArgs, *, config: Optional[dict] = None, **kw):
        # the engine reads the dataclass's values (the reference's defaults where config.json has no key) and never a
        # `head_dim` or a `rope_scaling`: the reference's model uses neither
        cfg = dict(config) if config is not None else {}
        cfg.update({k: getattr(args, k) for k in args.__dataclass_fields__})
        cfg["rope_scaling"] = None
        cfg.pop("head_dim", None)
        cfg.setdefault("tie_word_embeddings", False)                           # mixtral.py:187: an lm_head of its own
        super().__init__(args, config=cfg, **kw)

    def sanitize(self, weights):
        """mixtral.py:198-215 stacks the per-expert tensors into ``switch_mlp``; here both forms pass through and the
        engine places every expert's tensor in its slot (``mi_engine_set_tensor``)."""
        return weights

    @property
    def head_dim(self):                                                        # mixtral.py:221-223
        return self.args.hidden_size // self.args.num_attention_heads
