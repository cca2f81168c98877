"""Phi-3 model handle (mirror of ``mlx_parallm/models/phi3.py``).

The block is arithmetically Llama's (RMSNorm, half-split RoPE, SDPA, SwiGLU, no linear biases, an untied
``lm_head``); the checkpoint stores ``self_attn.qkv_proj`` (q, then k, then v along the rows, phi3.py:56-57,93-95)
and ``mlp.gate_up_proj`` (gate, then up, phi3.py:120,125) as one matrix each, which the engine takes as they are
(``MI_ARCH_PHI3``).  ``head_dim`` is ``hidden_size // num_attention_heads`` (phi3.py:53): 96 for Phi-3-mini.

``rope_scaling``: ``linear`` is served (``rope_scale = 1 / factor``, phi3.py:73-75).  ``su`` (SuScaledRotaryEmbedding,
the 128k checkpoints) is refused: su_rope.py:59-70 picks the short or the long factors per call from the scalar
``cache.offset + L``, which a batch of rows of different lengths does not have.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Union

from .base import BaseModelArgs
from .llama import Model as _LlamaModel


@dataclass
class ModelArgs(BaseModelArgs):
    model_type: str
    hidden_size: int
    num_hidden_layers: int
    intermediate_size: int
    num_attention_heads: int
    rms_norm_eps: float
    vocab_size: int
    num_key_value_heads: Optional[int] = None
    rope_theta: float = 10000
    rope_traditional: bool = False
    rope_scaling: Optional[Dict[str, Union[float, List[float]]]] = None
    max_position_embeddings: int = 131072
    original_max_position_embeddings: int = 4096

    def __post_init__(self):
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads

        if self.rope_scaling:                                                  # phi3.py:31-40
            required_keys = {"long_factor", "type"}
            if not all(key in self.rope_scaling for key in required_keys):
                raise ValueError(f"rope_scaling must contain keys {required_keys}")

            if self.rope_scaling["type"] not in ["su", "linear"]:
                print(
                    "[WARNING] rope_scaling 'type' currently only supports 'linear' and 'su'; setting rope scaling to false."
                )
                self.rope_scaling = None
            elif self.rope_scaling["type"] == "su":
                raise NotImplementedError(
                    "rope_scaling type su is not supported by the MI355X engine (its short / long factors are chosen "
                    "from one scalar sequence length per call, which a batch of rows of different lengths does not have)")


class Model(_LlamaModel):
    _ARCH = "phi3"

    def __init__(self, args: ModelArgs, *, config: Optional[dict] = None, **kw):
        # the engine reads the VALIDATED rope_scaling (an unknown type was dropped above), and never a `head_dim` key:
        # the reference ignores one (BaseModelArgs.from_dict filters it, phi3.py:53 divides)
        cfg = dict(config) if config is not None else {k: getattr(args, k) for k in args.__dataclass_fields__}
        cfg["rope_scaling"] = args.rope_scaling
        cfg["num_key_value_heads"] = args.num_key_value_heads
        cfg.pop("head_dim", None)
        super().__init__(args, config=cfg, **kw)

    def sanitize(self, weights):                                               # (phi3.py has no sanitize: every tensor is taken)
        return weights

    @property
    def head_dim(self):                                                        # phi3.py:209-211
        return self.args.hidden_size // self.args.num_attention_heads
