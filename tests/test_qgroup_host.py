"""Quantisation groups of 32 and 128 on the host: the random cases of tests/test_gpu_qgroup_kernels.py and the proof that
skinny_cases.RULE_CAP holds for them (the oracle's float32 envelopes on exactly these inputs)."""
import numpy as np
import pytest
import torch

from mlx_parallm_amd import quant
from oracle import numerics

from attn16_cases import rule_stats
from skinny_cases import RULE_CAP

TDT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
RANDOM_SHAPES = [(1, 1024), (8, 1024), (17, 1024), (33, 1024), (128, 1024), (129, 384), (256, 384)]      # (rows, K), N = 32


def random_case(bits, group, act, rows, K, N=32):
    """N(0,1) x in the dtype, 0.05 N(0,1) weights through quant.quantize -> (codes, scales, biases, x), float64 / int64"""
    rng = np.random.default_rng([bits, group, rows, K, act == "float16"])
    pk, sc, bi = quant.quantize(torch.from_numpy(rng.standard_normal((N, K)) * 0.05).to(TDT[act]), group, bits)
    x = numerics.round_to(rng.standard_normal((rows, K)), act).astype(np.float64)
    return quant.unpack_codes(pk, bits).numpy(), sc.double().numpy(), bi.double().numpy(), x


def w_hat(q, s, b):
    group = q.shape[1] // s.shape[1]
    return np.repeat(s, group, axis=1) * q + np.repeat(b, group, axis=1)


@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("group", [32, 128])
@pytest.mark.parametrize("bits", [4, 8])
def test_float32_envelopes_of_the_random_cases_stay_under_the_rule_cap(bits, group, act):
    for rows, K in RANDOM_SHAPES:
        q, s, b, x = random_case(bits, group, act, rows, K)
        w = w_hat(q, s, b)
        want = numerics.round_to(x @ w.T, act)
        for mode in ("f32_seq32", "f32_pairwise"):
            env = numerics.round_to(numerics.matmul_nt_f32(x, w.astype(np.float32), mode), act)
            worst, frac = rule_stats(env, want, act)
            print(f"ENVELOPE q{bits} g{group} {act} m{rows} K{K} {mode}: worst {worst:.3f} unit, {frac * rows * 32:.0f} of {rows * 32} beyond half a unit")
            assert worst <= 1.0 and frac <= RULE_CAP, (rows, K, mode, worst, frac)
