#!/usr/bin/env python3
"""Generates tests/golden/gqa/*.npz -- oracle outputs for GQA groups of 3 and 6 query heads per KV head.

Two sets, both outputs of the build's own oracle ("parity unpinned", like every golden here):

* SMALL (format of tests/golden/make_golden.py, spec["model"] = the build_tiny_model kwargs): tiny llama checkpoints
  with 6 / 2 heads of 32, 6 / 2 heads of 64 and 12 / 2 heads of 64 (G = 3, 3, 6), bf16 and int4 g64 with tied embeddings
  (the 384-wide one also f16), 4 left-padded prompts, 12 greedy steps, each in both KV modes.
* WIDE (format of tests/golden/make_golden_wide.py): the Llama-3.2-3B layer shapes (hidden 3072, 24 q / 8 kv heads x 128,
  intermediate 8192, vocabulary 128256, rms_norm_eps 1e-5, rope_theta 500000, tied embeddings) truncated to 2 decoder
  blocks, int4 g64 in both KV modes and bf16 in float32-KV, batch 8 with 1024-token prompts decoded over 77 steps
  (make_golden_wide.MAIN), each with its float32-accumulation envelope under envelope/ (about 5 minutes per case on 8 cores).

Run:  python tests/golden/gqa/make_golden_gqa.py [--small | --wide | --envelope] [case ...]
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


def _tiny(seed, hidden, heads, head_dim, dtype, q4):
    return dict(seed=seed, vocab_size=1024, dtype=dtype, quantize_model=q4, hidden_size=hidden, layers=2, heads=heads, kv_heads=2,
                intermediate_size=2 * hidden, head_dim=head_dim, tie_word_embeddings=True, norm_jitter=0.1, with_tokenizer=False)


SMALL_MODELS = {
    "h192_bf16": _tiny(41, 192, 6, 32, "bfloat16", False),
    "h192_int4": _tiny(42, 192, 6, 32, "bfloat16", True),
    "h384_bf16": _tiny(43, 384, 6, 64, "bfloat16", False),
    "h384_int4": _tiny(44, 384, 6, 64, "bfloat16", True),
    "h384_f16": _tiny(45, 384, 6, 64, "float16", False),
    "h768_bf16": _tiny(46, 768, 12, 64, "bfloat16", False),
    "h768_int4": _tiny(47, 768, 12, 64, "bfloat16", True),
}
SMALL = {f"gqa_{m}_{'paged' if paged else 'modelkv'}": dict(model=kw, B=4, L0=10, steps=12, paged=paged, temp=0.0, top_p=1.0, pad=True)
         for m, kw in SMALL_MODELS.items() for paged in (True, False)}

# ---------------------------------------------------------------------------------------------------------------------------
# the Llama-3.2-3B width

# layer shapes of Llama-3.2-3B-Instruct (config.json of the checkpoint): 3 query heads per kv head, tied embeddings
LLAMA32_3B = dict(model_type="llama", hidden_size=3072, heads=24, kv_heads=8, head_dim=128, intermediate_size=8192,
                  vocab_size=128256, rms_norm_eps=1e-5, rope_theta=500000.0)
FAMILY = "llama-3.2-3b"

MAIN = make_golden_wide.MAIN
CHECKPOINTS = {
    (FAMILY, "int4", 51): [
        dict(name="wide_llama32_3b_int4_modelkv", paged=False, **MAIN, prompt_seed=151),
        dict(name="wide_llama32_3b_int4_paged", paged=True, **MAIN, prompt_seed=152),
    ],
    (FAMILY, "bf16", 52): [
        dict(name="wide_llama32_3b_bf16_paged", paged=True, **MAIN, prompt_seed=153),
    ],
}


def model_kwargs(precision, seed):
    """wide_models.model_kwargs for the family above: the same seeding, weight distribution and quantisation, tied embeddings."""
    kw = dict(LLAMA32_3B)
    kw.update(seed=seed, layers=wide_models.LAYERS, dtype="bfloat16", tie_word_embeddings=True, weight_std=0.02,
              quantize_model=(precision == "int4"), q_bits=4, q_group_size=64, with_tokenizer=False,
              max_position_embeddings=wide_models.MAX_POS)
    return kw


def build_checkpoint(dst, family, precision, seed):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    assert family == FAMILY, family
    return build_tiny_model(dst, **model_kwargs(precision, seed))


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
