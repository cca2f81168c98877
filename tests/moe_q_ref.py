"""Oracle-side loading of a quantised Mixtral checkpoint (not a test): moe_ref.load with one quantised Linear per expert."""
import json
import re
from pathlib import Path

import numpy as np

import moe_ref
from oracle import ref_generate
from oracle.ref_model import Linear, RefConfig


def expert_linears(packed, scales, biases, dtype, bits):
    """[E][N][..] stacks -> one quantised Linear per expert."""
    return [Linear(dtype=dtype, packed=np.ascontiguousarray(packed[e]), scales=np.ascontiguousarray(scales[e]),
                   biases=np.ascontiguousarray(biases[e]), group_size=64, bits=bits) for e in range(packed.shape[0])]


def load(model_dir: str, max_pos: int = 4096) -> moe_ref.MoeRefModel:
    cfg_dict = dict(json.loads((Path(model_dir) / "config.json").read_text()), rope_scaling=None)      # (mixtral.py:57-61 ignores it)
    raw = ref_generate.load_weights(model_dir, cfg_dict)
    E, k = int(cfg_dict["num_local_experts"]), int(cfg_dict["num_experts_per_tok"])
    w = {}
    for name, val in raw.items():
        m = re.match(r"(model\.layers\.\d+\.block_sparse_moe\.)(switch_mlp\.(\w+)|experts\.(\d+)\.(w[123]))$", name)
        if m is None:
            w[name] = val
        elif m.group(3):
            for e, lin in enumerate(expert_linears(val.packed, val.scales, val.biases, val.dtype, val.bits)):
                w[f"{m.group(1)}experts.{e}.{m.group(3)}"] = lin
        else:
            w[f"{m.group(1)}experts.{m.group(4)}.{moe_ref._SINGLE[m.group(5)]}"] = val
    return moe_ref.MoeRefModel(RefConfig.from_dict(cfg_dict), w, max_pos, E, k)
