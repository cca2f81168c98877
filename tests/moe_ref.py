"""Oracle-side twin of the Mixtral block (not a test; the oracle package itself is left as it is).

``MoeRefModel`` is ``oracle.ref_model.RefModel`` with the MLP half of a block replaced by MixtralSparseMoeBlock
(mixtral.py:95-119, switch_layers.py:73-140), every MLX op rounded where it produces an array, T = the dtype of the normed input:

    g   = T(xn Wg^T)                                    nn.Linear, float32 accumulation, one rounding
    sel = the k largest g, a tie going to the LOWER expert index   (mx.argpartition leaves the order open: the rule is ours,
                                                                    and csrc/moe.hip's)
    s   = T(softmax_float32(g[sel]))                    mx.softmax(..., precise=True): exp(g - max) / sum in float32
    y_e = down_e(T(T(silu(gate_e xn)) * up_e xn))       the dense SwiGLU MLP of RefModel._mlp, per selected expert
    r   = T(T(y_a s_a) + T(y_b s_b))                    (y * scores[..., None]).sum(axis=-2)

The model records, per call of the block, the router margin g_(k) - g_(k+1) of every token (``margins``: a list of
(layer, margins (tokens,), larger |logit| of the two (tokens,))): how far the oracle alone is from picking another expert.
``load`` reads both name forms of a checkpoint (``switch_mlp.*`` stacked, ``experts.<e>.{w1,w2,w3}`` per expert) and serves
``rope_traditional`` by regrouping the q / k rows (tests/biased_ref.py).
"""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Optional

import numpy as np

from biased_ref import rows_perm
from oracle import ref_generate
from oracle.numerics import round_to
from oracle.ref_model import Linear, RefConfig, RefModel, promote

_SINGLE = {"w1": "gate_proj", "w2": "down_proj", "w3": "up_proj"}          # mixtral.py:203
_plain_load = ref_generate.load                                            # (tests put `load` below in its place)


def swiglu_mlp(gate: Linear, up: Linear, down: Linear, x: np.ndarray, xdt: str):
    """RefModel._mlp on explicit linears: down(T(T(silu(gate x)) * up x))."""
    g, gdt = gate(x, xdt)
    u, udt = up(x, xdt)
    sig = round_to(1.0 / (1.0 + np.exp(-g.astype(np.float64))), gdt)
    s = round_to(g * sig, gdt)
    hdt = promote(gdt, udt)
    return down(round_to(s * u, hdt), hdt)


def route(g: np.ndarray, k: int):
    """g (tokens, E) float32 -> (sel (tokens, k) by descending logit with ties to the lower index, float32 softmax over the
    selected (tokens, k), margin g_(k) - g_(k+1) (tokens,; inf when k == E), larger |logit| of that pair (tokens,))."""
    order = np.argsort(-g, axis=-1, kind="stable")
    sel = order[:, :k]
    gs = np.take_along_axis(g, sel, axis=-1).astype(np.float32)
    # float32 throughout, with the exp correctly rounded to float32 (taken in float64): np.exp on float32 input is a SIMD
    # approximation whose error depends on the CPU (2 ulps at exp(-10) with numpy 2.2 on x86-64), and a reference must not
    e = np.exp((gs - gs.max(axis=-1, keepdims=True)).astype(np.float64)).astype(np.float32)
    soft = (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    if g.shape[1] > k:
        nxt = np.take_along_axis(g, order[:, k:k + 1], axis=-1)[:, 0]
        margin = gs[:, k - 1] - nxt
        at = np.maximum(np.abs(gs[:, k - 1]), np.abs(nxt))
    else:
        margin = np.full(g.shape[0], np.inf, np.float32)
        at = np.abs(gs[:, k - 1])
    return sel, soft, margin, at


class MoeRefModel(RefModel):
    def __init__(self, cfg: RefConfig, weights, max_pos: int, n_experts: int, top_k: int):
        super().__init__(cfg, weights, max_pos=max_pos)
        self.n_experts, self.top_k = int(n_experts), int(top_k)
        self.margins = []

    def _mlp(self, i, x, xdt):                                            # mixtral.py:108-119
        p = f"model.layers.{i}.block_sparse_moe."
        B, L, H = x.shape
        xf = x.reshape(B * L, H)
        g, gdt = self.w[p + "gate"](xf, xdt)
        sel, soft, margin, at = route(g, self.top_k)
        self.margins.append((i, margin, at))
        scores = round_to(soft, gdt)
        out, odt = None, None
        terms = []
        for j in range(self.top_k):
            y = None
            for e in range(self.n_experts):
                rows = np.nonzero(sel[:, j] == e)[0]
                if rows.size == 0:
                    continue
                ye, ydt = swiglu_mlp(self.w[f"{p}experts.{e}.gate_proj"], self.w[f"{p}experts.{e}.up_proj"],
                                     self.w[f"{p}experts.{e}.down_proj"], xf[rows], xdt)
                if y is None:
                    y = np.zeros((B * L, ye.shape[-1]), np.float32)
                y[rows] = ye
                odt = ydt
            tdt = promote(odt, gdt)
            terms.append(round_to(y * scores[:, j:j + 1], tdt))
            odt = tdt
        out = terms[0] if self.top_k == 1 else round_to(terms[0] + terms[1], odt)
        return out.reshape(B, L, -1), odt


def load(model_dir: str, adapter_path: Optional[str] = None, max_pos: int = 4096) -> MoeRefModel:
    """``ref_generate.load`` for a Mixtral checkpoint directory, either name form."""
    cfg_dict = json.loads((Path(model_dir) / "config.json").read_text())
    if cfg_dict["model_type"] != "mixtral":
        return _plain_load(model_dir, adapter_path=adapter_path, max_pos=max_pos)
    cfg_dict = dict(cfg_dict, rope_scaling=None)                          # mixtral.py:57-61 ignores it
    cfg_dict.pop("head_dim", None)                                        # mixtral.py:38
    cfg_dict.setdefault("tie_word_embeddings", False)
    cfg = RefConfig.from_dict(cfg_dict)
    raw = ref_generate.load_weights(model_dir, cfg_dict)
    E, k = int(cfg_dict.get("num_local_experts", 8)), int(cfg_dict.get("num_experts_per_tok", 2))
    w = {}
    for name, val in raw.items():
        m = re.match(r"(model\.layers\.\d+\.block_sparse_moe\.)(switch_mlp\.(\w+)|experts\.(\d+)\.(w[123]))$", name)
        if m is None:
            w[name] = val
        elif m.group(3):                                                   # stacked: one Linear per expert
            assert val.weight.ndim == 3 and val.weight.shape[0] == E, name
            for e in range(E):
                w[f"{m.group(1)}experts.{e}.{m.group(3)}"] = Linear(dtype=val.dtype, weight=np.ascontiguousarray(val.weight[e]))
        else:
            w[f"{m.group(1)}experts.{m.group(4)}.{_SINGLE[m.group(5)]}"] = val
    if adapter_path is not None:
        ref_generate.apply_adapters(w, cfg.num_hidden_layers, adapter_path)
    if cfg_dict.get("rope_traditional"):                                   # the regrouped model IS the traditional one's oracle
        for i in range(cfg.num_hidden_layers):
            for proj, heads in (("q_proj", cfg.num_attention_heads), ("k_proj", cfg.num_key_value_heads)):
                lin = w[f"model.layers.{i}.self_attn.{proj}"]
                perm = rows_perm(heads, cfg.head_dim)
                lin.weight = np.ascontiguousarray(lin.weight[perm])
                if lin.lora_b is not None:
                    lin.lora_b = np.ascontiguousarray(lin.lora_b[:, perm])
    return MoeRefModel(cfg, w, max_pos, E, k)


def ulp(x: np.ndarray, dtype: str) -> np.ndarray:
    """The spacing of ``dtype`` (bfloat16 / float16) at |x|."""
    bits, emin = (7, -126) if dtype == "bfloat16" else (10, -14)
    ex = np.floor(np.log2(np.maximum(np.abs(x).astype(np.float64), 2.0 ** emin)))
    return np.exp2(ex - bits)


def margin_shortfall(model: MoeRefModel, dtype: str, paged: bool) -> float:
    """The largest amount by which a recorded router margin misses its bound: at least 1e-3 in the float32-KV mode (the
    project's logprob bound on these widths), at least 4 ulps of the model dtype at the larger of the two logits in the
    model-KV mode.  <= 0: every (token, layer) pair meets it."""
    worst = -np.inf
    for _layer, margin, at in model.margins:
        need = np.full(margin.shape, 1e-3) if paged else 4.0 * ulp(at, dtype)
        worst = max(worst, float(np.max(need - margin)))
    return worst
