"""quant.quantize_mxfp4 / dequantize_mxfp4 on the host: every representable value round-trips exactly, and both agree with a
float64 restatement of the format (OCP MX v1.0: E2M1 codes, E8M0 scale 2^(s - 127) per 32, round to nearest even, saturate)."""
import numpy as np
import torch

from mlx_parallm_amd import quant

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _restate(w):
    """(N, K) float64 -> (codes, scale bytes, W_hat), group by group"""
    g = w.reshape(w.shape[0], -1, 32)
    amax = np.abs(g).max(axis=-1, keepdims=True)
    e = np.clip(np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2, -127), -127, 127)
    v = np.minimum(np.abs(g) / 2.0 ** e, 6.0)
    d = np.abs(v[..., None] - GRID)
    idx = np.array([[min(np.flatnonzero(r == r.min()), key=lambda i: (i % 2, i)) for r in row] for row in d.reshape(-1, 32, 8)]).reshape(v.shape)
    q = idx | (((g < 0) & (idx > 0)).astype(np.int64) << 3)
    return q.reshape(w.shape), (e + 127).astype(np.uint8)[..., 0], (GRID[idx] * np.where(g < 0, -1.0, 1.0) * 2.0 ** e).reshape(w.shape)


def test_every_representable_value_round_trips():
    codes = torch.arange(16).repeat(2)                                    # a group holds all 16 codes (so its maximum is 6)
    q = codes.repeat(253, 1)                                              # one group per scale byte 0..252 (above: 6 x 2^(s - 127) leaves float32)
    s = torch.arange(253, dtype=torch.uint8).reshape(253, 1)
    w = quant.dequantize_mxfp4(quant.pack_codes(q, 4), s)
    assert w.dtype == torch.float32 and torch.isfinite(w).all()
    want = (GRID[q.numpy() & 7] * np.where(q.numpy() & 8, -1.0, 1.0)) * 2.0 ** (np.arange(253.0) - 127)[:, None]
    assert np.array_equal(w.double().numpy(), want)
    p2, s2 = quant.quantize_mxfp4(w.double())
    assert torch.equal(s2, s) and np.array_equal(quant.dequantize_mxfp4(p2, s2).double().numpy(), want)   # (-0 comes back as +0)
    assert torch.equal(w[1:].to(torch.bfloat16).float(), w[1:])           # exact in bf16 above scale byte 0


def test_agrees_with_the_restated_format():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((16, 128)) * np.exp2(rng.integers(-20, 20, size=(16, 1)))
    w[0, :32] = 0.0                                                       # an empty group
    w[1, :32] = 0.0
    w[1, :9] = [2.5, -2.5, 5.0, 0.25, 0.75, 1.25, 1.75, 3.5, 6.0]       # ties (the group's maximum, 6, makes the scale 1)
    q, s, w_hat = _restate(w)
    packed, scales = quant.quantize_mxfp4(torch.from_numpy(w))
    assert np.array_equal(quant.unpack_codes(packed, 4).numpy(), q) and np.array_equal(scales.numpy(), s)
    assert np.array_equal(quant.dequantize_mxfp4(packed, scales).double().numpy(), w_hat.astype(np.float32).astype(np.float64))
