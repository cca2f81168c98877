"""3- and 6-bit MLX-affine packing on the host: the bit stream of quant.py against a plain per-bit loop, the 6-bit / 8-bit
dequantisation identity that tests/test_gpu_q36_models.py leans on, and convert(..., q_bits=6)."""
import json

import numpy as np
import pytest
import torch

from mlx_parallm_amd import convert as cv, quant
from mlx_parallm_amd.tiny_model import build_tiny_model
from oracle import numerics

from attn16_cases import rule_stats
from skinny_cases import RULE_CAP

TDT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
RANDOM_SHAPES = [(1, 1024), (8, 1024), (17, 1024), (33, 1024), (128, 1024), (129, 384), (256, 384)]      # (rows, K), N = 32


def random_case(bits, act, rows, K, N=32):
    """The random construction of tests/test_gpu_q36_kernels.py: N(0,1) x in the dtype, 0.05 N(0,1) weights through
    quant.quantize -> (codes, scales, biases, x) as float64 / int64 arrays."""
    rng = np.random.default_rng([bits, rows, K, act == "float16"])
    pk, sc, bi = quant.quantize(torch.from_numpy(rng.standard_normal((N, K)) * 0.05).to(TDT[act]), 64, bits)
    x = numerics.round_to(rng.standard_normal((rows, K)), act).astype(np.float64)
    return quant.unpack_codes(pk, bits).numpy(), sc.double().numpy(), bi.double().numpy(), x


def w_hat(q, s, b):
    return np.repeat(s, 64, axis=1) * q + np.repeat(b, 64, axis=1)


@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits", [3, 6])
def test_float32_envelopes_of_the_random_cases_stay_under_the_rule_cap(bits, act):
    """The GPU test judges its random cases by skinny_cases.RULE_CAP; that cap holds for THESE inputs only if the oracle's own
    float32-accumulating envelopes (neither is the kernel's order) stay under it against the exact reference."""
    for rows, K in RANDOM_SHAPES:
        q, s, b, x = random_case(bits, act, rows, K)
        w = w_hat(q, s, b)
        want = numerics.round_to(x @ w.T, act)
        for mode in ("f32_seq32", "f32_pairwise"):
            env = numerics.round_to(numerics.matmul_nt_f32(x, w.astype(np.float32), mode), act)
            worst, frac = rule_stats(env, want, act)
            print(f"ENVELOPE q{bits} {act} m{rows} K{K} {mode}: worst {worst:.3f} unit, {frac * rows * 32:.0f} of {rows * 32} beyond half a unit")
            assert worst <= 1.0 and frac <= RULE_CAP, (rows, K, mode, worst, frac)


def _codes_by_bit(packed, bits, K):
    """code j of a row = bits [bits j, bits (j + 1)) of the row's little-endian byte stream, one bit at a time"""
    out = np.zeros((packed.shape[0], K), np.int64)
    for r, row in enumerate(packed.numpy().view(np.uint8).reshape(packed.shape[0], -1)):
        for j in range(K):
            for i in range(bits):
                p = bits * j + i
                out[r, j] |= ((int(row[p >> 3]) >> (p & 7)) & 1) << i
    return out


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("bits", [3, 6])
def test_quantize_round_trips_through_the_bit_stream(bits, K):
    torch.manual_seed(bits * K)
    w = torch.randn(3, K) * 0.05
    packed, s, b = quant.quantize(w, 64, bits)
    assert packed.shape == (3, K * bits // 32) and packed.dtype == torch.int32
    q = _codes_by_bit(packed, bits, K)
    assert q.min() >= 0 and q.max() == (1 << bits) - 1
    assert np.array_equal(quant.unpack_codes(packed, bits).numpy(), q)
    assert torch.equal(quant.pack_codes(torch.from_numpy(q), bits), packed)
    want = torch.from_numpy(q).float().reshape(3, -1, 64) * s.float()[..., None] + b.float()[..., None]
    assert torch.equal(quant.dequantize(packed, s, b, 64, bits), want.reshape(3, K))


def test_six_bit_codes_repacked_as_eight_bit_dequantise_alike():
    torch.manual_seed(1)
    packed, s, b = quant.quantize(torch.randn(3, 192) * 0.05, 64, 6)
    as8 = quant.pack_codes(quant.unpack_codes(packed, 6), 8)
    assert torch.equal(quant.dequantize(as8, s, b, 64, 8), quant.dequantize(packed, s, b, 64, 6))


def test_convert_writes_six_bit_quantization(tmp_path):
    build_tiny_model(tmp_path / "src", seed=0, vocab_size=512, dtype="float16", quantize_model=False, layers=1)
    cv.convert(str(tmp_path / "src"), str(tmp_path / "q6"), quantize=True, q_bits=6)
    assert json.loads((tmp_path / "q6" / "config.json").read_text())["quantization"] == {"group_size": 64, "bits": 6}
    w = cv.load_weights_dir(tmp_path / "q6")
    assert w["model.layers.0.mlp.down_proj.weight"].shape[1] == 128 * 6 // 32
