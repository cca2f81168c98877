"""The geometries of the GQA-group tests (3 and 6 query heads per KV head): shared by tests/test_gpu_attn_gqa.py (device) and
tests/test_attn_gqa_cases.py (what needs none).  Inputs, expectations and the rule are those of tests/attn16_cases.py, which
is generic in (Hq, Hkv, D)."""

GS = [3, 6]
DS = [32, 64, 128]

# (Hq, Hkv, D, q/k norm) of the random-data tests under attn16_cases.assert_rule
RANDOM_GEOMS = [(6, 2, 128, False), (3, 1, 64, True), (12, 2, 128, True), (6, 1, 64, False), (6, 2, 32, False)]

# one-hot unfused decode (attn_kernel + attn_combine_kernel)
UNFUSED_GEOMS = [(6, 2, 128), (6, 1, 64)]

# float32 caches: (Hq, Hkv, D) per variant of mi_op_attention_decode (0: matrix-core kernel, 1: vector-ALU kernel)
F32_DECODE_GEOMS = {0: [(12, 2, 128), (6, 1, 64)], 1: [(6, 2, 128), (3, 1, 32), (12, 2, 64)]}
F32_PREFILL_GEOMS = [(6, 2, 128), (12, 2, 64)]
F32_PREFILL_L = [2, 17, 50]
F32_PREFILL_OFFS = [0, 31, 207]
F32_PREFILL_CAP = 264
F32_UNFUSED_GEOM = (6, 2, 64)
