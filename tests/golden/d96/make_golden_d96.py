#!/usr/bin/env python3
"""Generates tests/golden/d96/*.npz -- oracle outputs at head_dim 96 (Phi-3's width).

Two sets, both outputs of the build's own oracle ("parity unpinned", like every golden here).  The oracle has no Phi-3
loader and needs none: a Phi-3 checkpoint with qkv_proj and gate_up_proj split is a Llama checkpoint, so every spec
holds build_tiny_model kwargs in LLAMA form and the oracle runs that form; the device tests build the phi3_* ones with
model_type="phi3" (the same tensors, written fused) and the d96_* ones as they are.

* SMALL (format of tests/golden/make_golden.py): vocabulary 1024, 2 layers, intermediate 2 x hidden, untied, 4 left-padded
  prompts of 10, 12 greedy steps, each in both KV modes.  phi3_h384_{bf16,int4,f16}: 4 / 4 heads of 96; phi3_h768_{bf16,int4}:
  8 / 8 heads of 96; d96_h384_g2_bf16 (4 / 2 heads) and d96_h384_g4_int4 (4 / 1 heads): Llama checkpoints with head_dim 96 in
  the config.
* WIDE (format of tests/golden/make_golden_wide.py): the Phi-3-mini layer shapes (hidden 3072, 32 / 32 heads of 96,
  intermediate 8192, vocabulary 32064, rms_norm_eps 1e-5, rope_theta 10000, untied) truncated to 2 decoder blocks, int4 g64
  in both KV modes and bf16 in float32-KV, batch 8 with 1024-token prompts decoded over 77 steps (make_golden_wide.MAIN), each
  with its float32-accumulation envelope under envelope/ (minutes per case on 8 cores).

Run:  python tests/golden/d96/make_golden_d96.py [--small | --wide | --envelope] [case ...]
"""
import sys
import tempfile
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "tests" / "golden"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import make_golden  # noqa: E402
import make_golden_wide  # noqa: E402
import wide_models  # noqa: E402
from oracle import ref_generate, ref_model  # noqa: E402

OUT = HERE

# ---------------------------------------------------------------------------------------------------------------------------
# small checkpoints


def _tiny(seed, hidden, heads, kv_heads, dtype, q4):
    return dict(seed=seed, vocab_size=1024, dtype=dtype, quantize_model=q4, hidden_size=hidden, layers=2, heads=heads,
                kv_heads=kv_heads, intermediate_size=2 * hidden, head_dim=96, tie_word_embeddings=False, norm_jitter=0.1,
                with_tokenizer=False)


SMALL_MODELS = {
    "phi3_h384_bf16": _tiny(71, 384, 4, 4, "bfloat16", False),
    "phi3_h384_int4": _tiny(72, 384, 4, 4, "bfloat16", True),
    "phi3_h384_f16": _tiny(73, 384, 4, 4, "float16", False),
    "phi3_h768_bf16": _tiny(74, 768, 8, 8, "bfloat16", False),
    "phi3_h768_int4": _tiny(75, 768, 8, 8, "bfloat16", True),
    "d96_h384_g2_bf16": _tiny(76, 384, 4, 2, "bfloat16", False),
    "d96_h384_g4_int4": _tiny(77, 384, 4, 1, "bfloat16", True),
}
SMALL = {f"{m}_{'paged' if paged else 'modelkv'}": dict(model=kw, B=4, L0=10, steps=12, paged=paged, temp=0.0, top_p=1.0, pad=True)
         for m, kw in SMALL_MODELS.items() for paged in (True, False)}


def phi3_kwargs(kw):
    """The build_tiny_model kwargs of the Phi-3 form of a Llama-form spec whose head_dim is hidden_size // heads."""
    assert kw["hidden_size"] // kw["heads"] == kw.get("head_dim", kw["hidden_size"] // kw["heads"]) and not kw["tie_word_embeddings"]
    out = {k: v for k, v in kw.items() if k != "head_dim"}
    out["model_type"] = "phi3"
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the Phi-3-mini width

# layer shapes of Phi-3-mini-4k-instruct (config.json of the checkpoint): 32 query / 32 KV heads of 96, an lm_head of its own
PHI3_MINI = dict(model_type="llama", hidden_size=3072, heads=32, kv_heads=32, head_dim=96, intermediate_size=8192,
                 vocab_size=32064, rms_norm_eps=1e-5, rope_theta=10000.0)
FAMILY = "phi-3-mini"

MAIN = make_golden_wide.MAIN
CHECKPOINTS = {
    (FAMILY, "int4", 81): [
        dict(name="wide_phi3_mini_int4_modelkv", paged=False, **MAIN, prompt_seed=181),
        dict(name="wide_phi3_mini_int4_paged", paged=True, **MAIN, prompt_seed=182),
    ],
    (FAMILY, "bf16", 82): [
        dict(name="wide_phi3_mini_bf16_paged", paged=True, **MAIN, prompt_seed=183),
    ],
}


def model_kwargs(precision, seed, layers=wide_models.LAYERS):
    """wide_models.model_kwargs for the family above, in Llama form: the same seeding, weight distribution and quantisation."""
    kw = dict(PHI3_MINI)
    kw.update(seed=seed, layers=layers, dtype="bfloat16", tie_word_embeddings=False, weight_std=0.02,
              quantize_model=(precision == "int4"), q_bits=4, q_group_size=64, with_tokenizer=False,
              max_position_embeddings=wide_models.MAX_POS)
    return kw


def build_checkpoint(dst, family, precision, seed, phi3=False, layers=wide_models.LAYERS):
    """Llama form (what the oracle loads) or, with ``phi3``, the same tensors as a Phi-3 checkpoint (what the device loads)."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    assert family == FAMILY, family
    kw = model_kwargs(precision, seed, layers)
    return build_tiny_model(dst, **(phi3_kwargs(kw) if phi3 else kw))


def main():
    args = sys.argv[1:]
    small, wide, envelope = "--small" in args, "--wide" in args, "--envelope" in args
    only = set(a for a in args if not a.startswith("--"))
    make_golden.OUT = OUT
    make_golden_wide.OUT = OUT
    if small or not (wide or envelope):
        for name, spec in SMALL.items():
            if not only or name in only:
                make_golden.run_case(name, spec)
    if small and not (wide or envelope):
        return
    for ck, cases in CHECKPOINTS.items():
        cases = [c for c in cases if not only or c["name"] in only]
        if not cases:
            continue
        with tempfile.TemporaryDirectory() as d:
            t0 = time.time()
            cfg = build_checkpoint(d, *ck)
            ref = ref_generate.load(d, max_pos=wide_models.MAX_POS)
            print(f"checkpoint {ck}: built + loaded in {time.time() - t0:.0f} s", flush=True)
            for case in cases:
                if wide or not envelope:
                    ref_model.CACHE_F64 = True
                    try:
                        make_golden_wide.run_case(ref, cfg, ck, case)
                    finally:
                        ref_model.CACHE_F64 = False
                if envelope or not wide:
                    make_golden_wide.run_envelope(ref, cfg, ck, case)


if __name__ == "__main__":
    main()
