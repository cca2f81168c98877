"""The geometries of the head_dim 96 tests (Phi-3's width; 1, 2 and 4 query heads per KV head): shared by
tests/test_gpu_attn_d96.py (device) and tests/test_attn_d96_cases.py (what needs none).  Inputs, expectations and the rule are
those of tests/attn16_cases.py, which is generic in (Hq, Hkv, D); L, offsets and capacity are those of tests/attn_gqa_cases.py."""
from attn_gqa_cases import F32_PREFILL_CAP, F32_PREFILL_L, F32_PREFILL_OFFS  # noqa: F401

GS = [1, 2, 4]
DS = [96]

# (Hq, Hkv, D, q/k norm) of the random-data tests under attn16_cases.assert_rule
RANDOM_GEOMS = [(2, 2, 96, False), (4, 2, 96, True), (4, 1, 96, False), (8, 8, 96, True)]

# one-hot unfused decode (attn_kernel + attn_combine_kernel)
UNFUSED_GEOMS = [(2, 2, 96), (4, 1, 96)]

# float32 caches: (Hq, Hkv, D) per variant of mi_op_attention_decode (0: matrix-core kernel, 1: vector-ALU kernel)
F32_DECODE_GEOMS = {0: [(2, 2, 96), (4, 2, 96), (4, 1, 96)], 1: [(2, 2, 96), (4, 1, 96)]}
F32_PREFILL_GEOMS = [(2, 2, 96), (4, 1, 96)]
F32_UNFUSED_GEOM = (4, 2, 96)

# refused before anything is launched: (Hq, Hkv, D)
REFUSED_GEOMS = [(3, 1, 96), (5, 1, 96), (6, 1, 96), (8, 1, 96), (2, 2, 48), (2, 2, 80)]
