"""MLX affine quantisation on torch tensors (CPU or GPU) -- the ``nn.quantize(model, group_size,
bits)`` step of ``scripts/build_tiny_model.py:150-151`` / ``utils.quantize_model`` (utils.py:888-908),
producing the on-disk triple ``<p>.weight`` (uint32) / ``<p>.scales`` / ``<p>.biases``.

Format (mlx 0.25.2 ``mx.quantize``): per group of ``group_size`` consecutive
input features, ``w ~ scale * q + bias`` with ``q`` an unsigned ``bits``-bit code; code j of a row
occupies bits [bits*j, bits*(j+1)) of the row's little-endian byte stream, viewed as uint32 words.
For 2, 4 and 8 bits that is 32/bits whole codes per word; for 3 and 6 bits every 3 bytes hold 8 or
4 codes and a code may straddle a byte or word boundary (unpinned like the rest of the format:
DESIGN §2).
"""
from __future__ import annotations

from typing import Tuple

import torch


def quantize(w: torch.Tensor, group_size: int = 64, bits: int = 4) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """w (N, K) float -> (packed int32-viewed-as-uint32 (N, K*bits/32), scales (N, K/g), biases (N, K/g)).
    scales/biases come back in ``w.dtype``."""
    if w.ndim != 2 or w.shape[1] % group_size != 0:
        raise ValueError("quantize expects (N, K) with K divisible by group_size")
    if bits not in (2, 3, 4, 6, 8):
        raise ValueError("bits must be 2, 3, 4, 6 or 8")
    dt = w.dtype
    n, k = w.shape
    g = w.to(torch.float32).reshape(n, k // group_size, group_size)
    n_bins = float((1 << bits) - 1)
    w_max = g.amax(dim=-1, keepdim=True)
    w_min = g.amin(dim=-1, keepdim=True)
    mask = w_min.abs() > w_max.abs()
    scales = torch.clamp((w_max - w_min) / n_bins, min=1e-7)
    scales = torch.where(mask, scales, -scales)
    edge = torch.where(mask, w_min, w_max)
    q0 = torch.round(edge / scales)
    scales = torch.where(q0 != 0, edge / q0, scales)
    biases = torch.where(q0 == 0, torch.zeros_like(edge), edge)
    q = torch.clamp(torch.round((g - biases) / scales), 0, n_bins).to(torch.int64)
    return pack_codes(q.reshape(n, k), bits), scales.reshape(n, -1).to(dt), biases.reshape(n, -1).to(dt)


def pack_codes(q: torch.Tensor, bits: int) -> torch.Tensor:
    """codes (N, K) integer in [0, 2^bits) -> the packed bit stream as int32 words (N, K*bits/32)."""
    n, k = q.shape
    if (k * bits) % 32 != 0:
        raise ValueError("a packed row must be whole 32-bit words")
    q = q.to(torch.int64)
    if 32 % bits == 0:
        per = 32 // bits
        shifts = torch.arange(per, device=q.device, dtype=torch.int64) * bits
        packed = (q.reshape(n, k // per, per) << shifts).sum(dim=-1)                       # < 2^32
    else:                                                    # 3 / 6 bits: through the stream's single bits
        bit = (q[..., None] >> torch.arange(bits, device=q.device, dtype=torch.int64)) & 1  # (N, K, bits), LSB first
        shifts = torch.arange(32, device=q.device, dtype=torch.int64)
        packed = (bit.reshape(n, k * bits // 32, 32) << shifts).sum(dim=-1)
    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)


def unpack_codes(packed: torch.Tensor, bits: int) -> torch.Tensor:
    """the inverse of pack_codes: int32 words (N, K*bits/32) -> codes (N, K) int64."""
    p = packed.to(torch.int64) & 0xFFFFFFFF
    n = packed.shape[0]
    if 32 % bits == 0:
        shifts = torch.arange(32 // bits, device=packed.device, dtype=torch.int64) * bits
        return ((p[..., None] >> shifts) & ((1 << bits) - 1)).reshape(n, -1)
    bit = ((p[..., None] >> torch.arange(32, device=packed.device, dtype=torch.int64)) & 1).reshape(n, -1, bits)
    return (bit << torch.arange(bits, device=packed.device, dtype=torch.int64)).sum(dim=-1)


# ---- mode "mxfp4": the OCP Microscaling FP4 format (MX v1.0) in MLX's packing -- E2M1 codes, code j of a row at bits
# [4j, 4j+4) like affine int4, one E8M0 scale byte (2^(s-127)) per 32 weights, no bias.  Restated from the published
# definitions, not pinned against MLX.
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)     # bits 0..2 of a code; bit 3 is the sign


def quantize_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w (N, K) float, K % 32 == 0 -> (packed int32 (N, K/8), scales uint8 (N, K/32)).  Scale = 2^(floor(log2 max|w|) - 2)
    per group (E2M1's largest exponent is 2), clamped to E8M0's bytes 0..254; codes round to nearest, ties to the even
    mantissa, onto the E2M1 grid and saturate at +-6."""
    if w.ndim != 2 or w.shape[1] % 32 != 0:
        raise ValueError("quantize_mxfp4 expects (N, K) with K divisible by 32")
    n, k = w.shape
    g = w.to(torch.float64).reshape(n, k // 32, 32)
    amax = g.abs().amax(dim=-1, keepdim=True)
    e = torch.where(amax > 0, torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))) - 2, torch.full_like(amax, -127.0))
    e = e.clamp(-127, 127)
    v = (g / torch.exp2(e)).abs().clamp(max=6.0)
    grid = torch.tensor(MXFP4_VALUES, dtype=torch.float64, device=w.device)
    d = (v[..., None] - grid).abs()                           # (N, K/32, 32, 8); a tie sits between two neighbours:
    lo = d.argmin(dim=-1)                                     # argmin takes the lower one, the even code wins it
    tie = (lo < 7) & (d.gather(-1, lo[..., None]).squeeze(-1) == d.gather(-1, (lo + 1).clamp(max=7)[..., None]).squeeze(-1))
    mag = torch.where(tie & (lo % 2 == 1), lo + 1, lo)
    q = mag | ((g < 0) & (mag > 0)).to(torch.int64) << 3      # (no negative zero is written)
    return pack_codes(q.reshape(n, k), 4), (e + 127).reshape(n, -1).to(torch.uint8)


def dequantize_mxfp4(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """-> (N, K) float32, code value x 2^(s - 127): exact in float32 and in bfloat16 (subnormals at scale byte 0)."""
    q = unpack_codes(packed, 4)
    n, k = q.shape
    grid = torch.tensor(MXFP4_VALUES, dtype=torch.float64, device=packed.device)
    v = grid[q & 7] * torch.where((q & 8) != 0, -1.0, 1.0)
    s = torch.exp2(scales.to(torch.float64) - 127.0)
    return (v.reshape(n, k // 32, 32) * s[..., None]).reshape(n, k).to(torch.float32)


# ---- mode "mxfp8": OCP Microscaling FP8 -- one E4M3 ("fn") code byte per weight (sign, four exponent bits with bias 7, three
# mantissa bits, subnormals m x 2^-9, largest value 448, 0x7f / 0xff NaN), code j of a row at byte j like affine int8, the same
# E8M0 scale bytes, no bias.
def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e in float64 for integer e in float64's normal range, exactly (torch.exp2 is not exact everywhere)"""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def quantize_mxfp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w (N, K) float, K % 32 == 0 -> (packed int32 (N, K/4), scales uint8 (N, K/32)).  Scale = 2^(floor(log2 max|w|) - 8) per
    group (E4M3's largest exponent is 8), clamped to E8M0's bytes 0..254; codes round to nearest, ties to the even mantissa,
    onto the E4M3 grid and saturate at +-448 (clamped in float64, before any code is formed: no NaN code and no negative zero
    is written).  The scale rule restates the MX specification; it could not be checked against MLX."""
    if w.ndim != 2 or w.shape[1] % 32 != 0:
        raise ValueError("quantize_mxfp8 expects (N, K) with K divisible by 32")
    n, k = w.shape
    g = w.to(torch.float64).reshape(n, k // 32, 32)
    amax = g.abs().amax(dim=-1, keepdim=True)
    e = torch.where(amax > 0, torch.frexp(amax)[1].to(torch.int64) - 1 - 8, torch.full_like(amax, -127, dtype=torch.int64)).clamp(-127, 127)
    v = (g * _pow2(-e)).abs().clamp(max=448.0)
    ex = (torch.frexp(v)[1].to(torch.int64) - 1).clamp(min=-6)         # floor(log2 v); below 2^-6 the grid is the subnormals' 2^-9
    a = (torch.round(v * _pow2(3 - ex)) * _pow2(ex - 3)).clamp(max=448.0)      # (torch.round: ties to even)
    ea = torch.frexp(a)[1].to(torch.int64) - 1                # (a may have carried into the next binade)
    q = torch.where(a < 2.0 ** -6, (a * 512.0).to(torch.int64), ((ea + 7) << 3) | ((a * _pow2(-ea) - 1.0) * 8.0).to(torch.int64))
    q = q | ((g < 0) & (q > 0)).to(torch.int64) << 7
    return pack_codes(q.reshape(n, k), 8), (e + 127).reshape(n, -1).to(torch.uint8)


def dequantize_mxfp8(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """-> (N, K) float32, code value x 2^(s - 127): exact in float32 and in bfloat16 (four significant bits)."""
    q = unpack_codes(packed, 8)
    n, k = q.shape
    ef, m = ((q >> 3) & 15).to(torch.float64), (q & 7).to(torch.float64)
    v = torch.where(ef == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * _pow2(ef - 7)) * torch.where((q & 128) != 0, -1.0, 1.0)
    s = _pow2(scales.to(torch.int64) - 127)
    return (v.reshape(n, k // 32, 32) * s[..., None]).reshape(n, k).to(torch.float32)


def dequantize(packed: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor, group_size: int = 64,
               bits: int = 4) -> torch.Tensor:
    q = unpack_codes(packed, bits).to(torch.float32)
    n, k = q.shape
    q = q.reshape(n, k // group_size, group_size)
    w = q * scales.to(torch.float32)[..., None] + biases.to(torch.float32)[..., None]
    return w.reshape(n, k)
