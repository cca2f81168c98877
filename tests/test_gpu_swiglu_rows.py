"""swiglu_rows_kernel (csrc/lora_rows.hip) through mi_op_swiglu_rows (-m gpu): the SwiGLU of an ADAPTED gate|up linear, whose
LoRA term has to be added before the activation -- the linear stores gate|up, this kernel writes silu(gate) * up.

Yardstick: a NumPy restatement of the three rounding points of nn.silu(gate) * up in the activation dtype T (llama.py:165;
gemv_v1.hip's EPI_SWIGLU):  sig = T(1 / (1 + exp(-g))),  s = T(g * sig),  out = T(s * u)  with the exp taken in float64.
The products of two 16-bit values are exact in float32, so for the 16-bit types the yardstick is the correctly rounded value
at every point and a kernel can differ only where its own exp moves sig across a rounding boundary of T.

Requirements (set before any run):
  16-bit T (bf16, f16, and float32 storage with the logical bf16 rounding): every element within ONE ulp of T (distance of
      the bit patterns), at least 99.9 % bit-equal.  A float32 expf (a few 1e-7 relative) moves a result across a boundary of
      a 2^-8 / 2^-11 grid with probability ~2^-14 per rounding, three roundings: the 0.1 % cap is a condition, not a
      measurement.
  float32: relative error <= 4e-6 (expf's error, then three float32 roundings of 6e-8 each, with a wide margin).
The yardstick rounds the float64 sigmoid to T ONCE.  Rounded through float32 first (as this file did at first, and as a
float32 expf does) the few g whose sigmoid lies within a float32 ulp of a midpoint of T's grid (g = 11 x 2^-10 in f16) land ON
the midpoint and the tie goes the other way; g * sig can carry that one ulp to two ulps of the product.  Measured on the
device against the twice-rounding yardstick, f16 at 129 x 14336: float32 expf 99.9999 % equal with one element two ulps
off; float64 exp rounded once 99.9995 % equal, nine elements off, one by two ulps -- all of them at such g, the kernel's
value the correctly rounded one.  The kernel therefore takes the exp in float64 and rounds once, as the yardstick does.
Shapes: M in {1, 3, 129} x I in {8, 264, 14336} (one vector per row; rows that are no multiple of a block; more than one
block per row and a grid of thousands of blocks), contiguous rows, and once with odd row strides on both sides."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.numerics import round_f64, round_to

pytestmark = pytest.mark.gpu

from gpu_helpers import MIDT, TDT, ptr  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402

# name -> (storage dtype, MI_RND_*, the logical dtype T)
TYPES = {"bf16": ("bfloat16", L.RND_NONE, "bfloat16"), "f16": ("float16", L.RND_NONE, "float16"),
         "f32": ("float32", L.RND_NONE, "float32"), "f32_rnd_bf16": ("float32", L.RND_BF16, "bfloat16")}
_INPUTS = {}


def _inputs(M, I, ldx, logical):
    """g | u rows of T values (float32 array [M][ldx]; the padding columns hold a NaN the kernel must not read into a result)"""
    key = (M, I, ldx, logical)
    if key not in _INPUTS:
        rng = np.random.default_rng([M, I, ldx])
        x = np.full((M, ldx), np.nan, dtype=np.float32)
        x[:, :2 * I] = round_to((rng.standard_normal((M, 2 * I)) * 2.5).astype(np.float32), logical)
        _INPUTS[key] = x
    return _INPUTS[key]


def _yardstick(x, I, logical):
    g, u = x[:, :I].astype(np.float64), x[:, I:2 * I].astype(np.float64)
    sig = round_f64(1.0 / (1.0 + np.exp(-g)), logical).astype(np.float64)
    s = round_to(g * sig, logical).astype(np.float64)
    return round_to(s * u, logical)


def _ordered16(a, logical):
    """bit patterns of 16-bit values as integers in value order (+0 and -0 alike): |difference| = distance in ulps"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TDT[logical])
    bits = t.view(torch.int16).numpy().astype(np.int32) & 0xFFFF
    return np.where(bits >= 0x8000, -(bits - 0x8000), bits)


def _call(x_dev, ldx, out_dev, ldo, M, I, act, rnd):
    torch.cuda.synchronize()
    return L.lib().mi_op_swiglu_rows(ptr(x_dev), int(ldx), ptr(out_dev), int(ldo), int(M), int(I), int(act), int(rnd))


def _run_and_check(M, I, ldx, ldo, tname):
    storage, rnd, logical = TYPES[tname]
    x = _inputs(M, I, ldx, logical)
    want = _yardstick(x, I, logical)
    xd = torch.from_numpy(x).to(TDT[storage]).cuda().contiguous()
    outs = []
    for _ in range(2):
        od = torch.full((M, ldo), -7.0, dtype=TDT[storage], device="cuda")
        L.check(_call(xd, ldx, od, ldo, M, I, MIDT[storage], rnd))
        outs.append(od.cpu())
    assert torch.equal(outs[0].view(torch.int16 if storage != "float32" else torch.int32),
                       outs[1].view(torch.int16 if storage != "float32" else torch.int32))          # the same call twice
    got = outs[0].to(torch.float32).numpy()
    assert np.all(got[:, I:] == -7.0)                               # nothing written behind a row
    got = got[:, :I]
    assert np.isfinite(got).all()
    if logical == "float32":
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
        print(f"{tname} M={M} I={I}: max relative error {rel.max():.2e}")
        assert rel.max() <= 4e-6, rel.max()
        return
    assert np.array_equal(got, round_to(got, logical))              # float32 storage holds T values
    dist = np.abs(_ordered16(got, logical) - _ordered16(want, logical))
    equal = float((dist == 0).mean())
    print(f"{tname} M={M} I={I}: max distance {dist.max()} ulp, bit-equal {100 * equal:.4f} %")
    for m, n in list(zip(*np.nonzero(dist)))[:12]:                  # the elements that differ, before anything is asserted
        print(f"    [{m}][{n}]: g = {x[m, n]!r}, u = {x[m, I + n]!r}, kernel {got[m, n]!r}, yardstick {want[m, n]!r}, {dist[m, n]} ulp")
    assert dist.max() <= 1, dist.max()
    assert equal >= 0.999, equal


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("I", [8, 264, 14336])
@pytest.mark.parametrize("M", [1, 3, 129])
def test_swiglu_rows_against_the_rounding_points(M, I, tname):
    _run_and_check(M, I, 2 * I, I, tname)


@pytest.mark.parametrize("tname", list(TYPES))
def test_swiglu_rows_row_strides(tname):
    """ldx > 2 I and ldo > I, both odd: rows that start at no multiple of 16 bytes"""
    _run_and_check(3, 264, 2 * 264 + 3, 264 + 5, tname)


def test_swiglu_rows_refuses_bad_arguments():
    M, I = 3, 264
    x = torch.zeros((M, 2 * I), dtype=torch.bfloat16, device="cuda")
    out = torch.full((M, I), -7.0, dtype=torch.bfloat16, device="cuda")
    bf = L.MI_BF16
    INVALID, UNSUPPORTED = -1, -3
    cases = [
        (UNSUPPORTED, (x, 2 * I, out, I, M, 12, bf, 0)),            # I no multiple of 8
        (UNSUPPORTED, (x, 2 * I, out, I, M, 260, bf, 0)),
        (INVALID, (x, 2 * I, out, I, 0, I, bf, 0)),                 # no rows
        (INVALID, (x, 2 * I, out, I, M, 0, bf, 0)),
        (INVALID, (x, 2 * I - 8, out, I, M, I, bf, 0)),             # a stride shorter than its row
        (INVALID, (x, 2 * I, out, I - 8, M, I, bf, 0)),
        (INVALID, (x, 2 * I, out, I, M, I, 7, 0)),                  # not a dtype
        (INVALID, (x, 2 * I, out, I, M, I, L.MI_U32, 0)),
        (INVALID, (x, 2 * I, out, I, M, I, bf, 5)),                 # not a rounding mode
        (INVALID, (None, 2 * I, out, I, M, I, bf, 0)),
        (INVALID, (x, 2 * I, None, I, M, I, bf, 0)),
    ]
    for want, args in cases:
        assert _call(*args) == want, (want, args[1:])
        assert L.lib().mi_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                # the sentinel-filled output was never touched
    # a misaligned float32 buffer (not a float32 address)
    raw = torch.zeros(4 * M * 2 * I + 8, dtype=torch.uint8, device="cuda")
    o32 = torch.full((M, I), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = L.lib().mi_op_swiglu_rows(C.c_void_p(raw.data_ptr() + 2), 2 * I, ptr(o32), I, M, I, L.MI_F32, 0)
    assert rc == INVALID
    torch.cuda.synchronize()
    assert bool((o32 == -7.0).all())
