"""quant.quantize_mxfp8 / dequantize_mxfp8 against torch's float8_e4m3fn view and the quantisation rule restated in float64"""
import math

import numpy as np
import pytest
import torch

from mlx_parallm_amd import quant

CODES = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.int64)      # the 254 finite codes


def _all_codes(s):
    """9 groups: the code of 448 and 31 others each, so that the rule finds the scale again (a largest value of mantissa 1.875 saturates)"""
    q = torch.cat([CODES, torch.zeros(25, dtype=torch.int64)]).reshape(9, 31)
    q = torch.cat([torch.full((9, 1), 0x7e, dtype=torch.int64), q], dim=1)
    return quant.pack_codes(q, 8), torch.full((9, 1), s, dtype=torch.uint8), q


def test_every_code_under_every_pinned_scale():
    for s in range(10, 247):
        packed, scales, q = _all_codes(s)
        w = quant.dequantize_mxfp8(packed, scales)
        want = q.to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float64) * 2.0 ** (s - 127)
        assert torch.equal(w.to(torch.float64), want), s
        assert torch.equal(w.to(torch.bfloat16).to(torch.float64), want), s             # exact in bf16
        p2, s2 = quant.quantize_mxfp8(w)                                                # (the round trip)
        assert torch.equal(quant.dequantize_mxfp8(p2, s2), w), s


def _rule(g):
    amax = max(abs(v) for v in g)
    e = max(-127, min(127, math.frexp(amax)[1] - 1 - 8)) if amax > 0 else -127
    out = []
    for v in g:
        a = min(abs(v) / 2.0 ** e, 448.0)
        ex = max(math.frexp(a)[1] - 1, -6) if a > 0 else -6
        a = min(float(np.round(a * 2.0 ** (3 - ex))) * 2.0 ** (ex - 3), 448.0)           # (np.round: ties to even)
        out.append(math.copysign(a, v) if a > 0 else 0.0)
    return out, e


def test_quantize_follows_the_rule():
    rng = np.random.default_rng(8)
    w = rng.standard_normal((16, 64)) * np.exp2(rng.integers(-20, 20, size=(16, 1)))
    w[0, :32] = 0.0                                                       # an all-zero group: scale byte 0, codes 0
    w[1:4, :32] = 0.3
    w[1, :7] = [465.0, -465.0, 448.0, 17.0, 19.0, -21.0, 2.0 ** -3 * 1.0625]      # scale 2^0: 465 saturates to 448; ties
    w[2, :4] = [256.0, 2.5 * 2.0 ** -9, 3.5 * 2.0 ** -9, -2.0 ** -10]     # ties among the subnormals (steps of 2^-9), and below
    w[3, 0] = 1000.0                                                      # scale 2^1: 500 saturates to the code of 448
    packed, scales = quant.quantize_mxfp8(torch.from_numpy(w))
    got = quant.dequantize_mxfp8(packed, scales).to(torch.float64).numpy()
    codes = quant.unpack_codes(packed, 8).numpy()
    assert not ((codes & 0x7f) == 0x7f).any() and not (codes == 0x80).any()              # no NaN code, no negative zero
    for n in range(16):
        for j in range(2):
            vals, e = _rule(list(w[n, 32 * j:32 * j + 32]))
            assert int(scales[n, j]) == e + 127
            assert np.array_equal(got[n, 32 * j:32 * j + 32], np.array(vals) * 2.0 ** e), (n, j)
    assert list(got[1, :7]) == [448.0, -448.0, 448.0, 16.0, 20.0, -20.0, 2.0 ** -3]
    assert list(got[2, :4]) == [256.0, 2.0 ** -8, 2.0 ** -7, 0.0] and int(scales[0, 0]) == 0
    assert got[3, 0] == 896.0 and codes[3, 0] == 0x7e and int(scales[3, 0]) == 128


@pytest.mark.parametrize("mode", ["mxfp4", "mxfp8"])
def test_convert_refuses_the_mode_by_name(mode):
    from mlx_parallm_amd.convert import dequantize_model
    with pytest.raises(NotImplementedError, match=mode):
        dequantize_model({}, {"quantization": {"group_size": 32, "bits": 8, "mode": mode}})
