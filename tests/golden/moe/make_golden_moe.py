#!/usr/bin/env python3
"""Generates tests/golden/moe/*.npz -- outputs of the oracle twin of the Mixtral block (tests/moe_ref.py), in the format of
tests/golden/make_golden.py ("parity unpinned", like every golden here: the build's own oracle, not the reference's MLX run).

Models: 128 wide, 2 layers, 4 / 2 heads of 32, intermediate 192, vocabulary 1024, router_gain 4 (gate logits of order 1):
E = 4 and E = 8 with k = 2 in bfloat16 and float16, E = 4 with k = 1, and E = 4, k = 2 with rope_traditional.  Each in both KV
modes: 2 rows, 6 prompt tokens, 6 greedy steps.

A device sum that differs from the oracle's by rounding noise may pick another expert at a near-tie, and the rest of that row is
then another computation.  So every case takes the first model seed (of at most 200, starting at the case's base) for which
the ORACLE ALONE never comes near a tie: every recorded router margin g_(k) - g_(k+1) is at least 1e-3 in the float32-KV mode
and at least 4 ulps of the model dtype at the larger of the two logits in the model-KV mode (moe_ref.margin_shortfall).  The
seed taken is in the file's spec; the smallest margin and the number of seeds tried are stored beside it.

Run:  python tests/golden/moe/make_golden_moe.py [case ...]
"""
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import moe_ref  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from oracle import ref_generate  # noqa: E402

OUT = HERE
MAX_SEEDS = 200


def _tiny(dtype, experts, per_tok, **extra):
    return dict(model_type="mixtral", vocab_size=1024, dtype=dtype, quantize_model=False, hidden_size=128, layers=2, heads=4,
                kv_heads=2, intermediate_size=192, tie_word_embeddings=False, norm_jitter=0.1, with_tokenizer=False,
                num_local_experts=experts, num_experts_per_tok=per_tok, router_gain=4.0, **extra)


# name -> (build_tiny_model kwargs without the seed, first seed tried)
MODELS = {
    "moe_e4k2_bf16": (_tiny("bfloat16", 4, 2), 1000),
    "moe_e8k2_bf16": (_tiny("bfloat16", 8, 2), 2000),
    "moe_e4k2_f16": (_tiny("float16", 4, 2), 3000),
    "moe_e8k2_f16": (_tiny("float16", 8, 2), 4000),
    "moe_e4k1_bf16": (_tiny("bfloat16", 4, 1), 5000),
    "moe_e4k2_trad_bf16": (_tiny("bfloat16", 4, 2, rope_traditional=True), 6000),
}
CASES = {f"{m}_{'paged' if paged else 'modelkv'}": dict(model=m, B=2, L0=6, steps=6, paged=paged, temp=0.0, top_p=1.0)
         for m in MODELS for paged in (True, False)}


def run_model(model_kw, case, prompts):
    """The oracle twin on one checkpoint: -> (arrays of the golden format, the twin with its recorded margins)."""
    with tempfile.TemporaryDirectory() as d:
        build_tiny_model(d, **model_kw)
        ref = moe_ref.load(d, max_pos=256)
    toks, lps, top_ids, top_vals, margins = [], [], [], [], []
    gen = ref_generate.generate_step(prompts, ref, temp=0.0, top_p=1.0, paged=case["paged"], return_logits=True)
    for (t, _p, logits, lp), _ in zip(gen, range(case["steps"])):
        toks.append(t[:, 0])
        lps.append(lp)
        order = np.argsort(-logits, axis=-1, kind="stable")[:, :8]
        top_ids.append(order)
        tv = np.take_along_axis(logits, order, axis=-1)
        top_vals.append(tv)
        margins.append(tv[:, 0] - tv[:, 1])
    arrays = dict(tokens=np.stack(toks).astype(np.int32), logprobs=np.stack(lps).astype(np.float32),
                  top_ids=np.stack(top_ids).astype(np.int32), top_vals=np.stack(top_vals).astype(np.float32),
                  margins=np.stack(margins).astype(np.float32))
    return arrays, ref


def prompts_of(name, case):
    rng = np.random.default_rng(sum(ord(c) for c in name))
    return rng.integers(3, 1024, size=(case["B"], case["L0"]))


def run_case(name, case):
    base_kw, seed0 = MODELS[case["model"]]
    prompts = prompts_of(name, case)
    for tried in range(MAX_SEEDS):
        kw = dict(base_kw, seed=seed0 + tried)
        arrays, ref = run_model(kw, case, prompts)
        short = moe_ref.margin_shortfall(ref, kw["dtype"], case["paged"])
        if short <= 0:
            break
    else:
        raise SystemExit(f"{name}: no seed in {seed0}..{seed0 + MAX_SEEDS - 1} meets the router-margin condition")
    pairs = sum(len(m) for _l, m, _a in ref.margins)
    smallest = min(float(np.min(m)) for _l, m, _a in ref.margins)
    spec = dict(model=kw, B=case["B"], L0=case["L0"], steps=case["steps"], paged=case["paged"], temp=0.0, top_p=1.0,
                seeds_tried=tried + 1, router_pairs=pairs, router_margin_min=smallest)
    uniforms = np.zeros((case["steps"] + 2, case["B"]), np.float32)        # (greedy: the format's field, unused)
    np.savez_compressed(OUT / f"{name}.npz", spec=json.dumps(spec), prompts=prompts.astype(np.int32), uniforms=uniforms, **arrays)
    print(f"{name}: seed {kw['seed']} (tried {tried + 1}), {pairs} (token, layer) pairs, smallest router margin {smallest:.4g}, "
          f"min top1-top2 margin {arrays['margins'].min():.4f}")


if __name__ == "__main__":
    only = sys.argv[1:]
    for n, c in CASES.items():
        if not only or n in only:
            run_case(n, c)
