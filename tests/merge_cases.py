"""Inputs and the float32 envelope of the adapter-merge tests (not a test): shared by tests/test_merge_cases.py (CPU) and
tests/test_gpu_lora_merge.py.

Shapes: N in {1, 16, 17, 40} x K in {64, 192, 320} (tails of the kernel's 256-thread stride, more than one 64-group) x rank in
{1, 7, 64}, every combination, in bfloat16 and float16, on a dense, an int4 and an int8 base.

* ``exact_inputs``: W = integers -4..4 times 2^-3 (a quantised base: codes times 2^-3 plus such a bias), A and B integers
  -3..3, s = 1/8, m a power of two.  Every float32 sum of steps 1-5 is then exact in any order (``exact_is_exact`` proves it per
  case from the magnitudes), so every rounding is determined and the kernel must equal the twin (tests/merge_ref.py) bit for bit.
* ``random_inputs``: W = T(0.05 N(0,1)), A = U(-1,1) / sqrt(K), B = 0.3 N(0,1), s = 4; a quantised base is
  ``ref_quant.quantize`` of that W.  ``restate_f32`` is steps 1-4 as a float32 program would run them (the multiply-add of
  step 1 and the ascending-j chain of step 3 rounded to float32 at every operation, the add of step 4 in float32 before the
  rounding to T): the envelope.  It differs from the exact twin only where a float32 rounding lands on the other side of a
  rounding boundary of T in step 3 or step 4: by one ulp of T at delta or at Wm (``one_ulp``).  Where Wd and delta cancel, one
  ulp at delta is more than one at Wm: measured below, the envelope itself is 2 ulps of Wm off on 3 float16 elements per base
  (shapes (16, 320, 64) and (40, 320, 64)), so "one ulp of T" is taken at the larger of |delta| and |Wm|.

MEASURED on the CPU (tests/test_merge_cases.py asserts these counts; they are the envelope's, not a kernel's), elements of the
36 shapes (127 872 per dtype and base) on which ``restate_f32`` differs from the exact twin:

    base     bfloat16   float16
    dense        0          9
    int4         0         11
    int8         0         10

(the figures stand in ``ENVELOPE`` below).  The GPU test allows the kernel ``RULE_CAP`` = 4 times these counts per dtype and
base -- the factor covers that the envelope's order need not be the kernel's, as ``skinny_cases.RULE_CAP`` does -- and one ulp
of T at most per element; where the envelope shows no difference the kernel may show none.
"""
from __future__ import annotations

import itertools

import numpy as np

from oracle import ref_quant
from oracle.numerics import round_to

SEED = 20250917
NS, KS, RANKS = (1, 16, 17, 40), (64, 192, 320), (1, 7, 64)
SHAPES = list(itertools.product(NS, KS, RANKS))
DTYPES = ("bfloat16", "float16")
BASES = (0, 4, 8)                                   # quant_bits of the base
RULE_CAP = 4
# (dtype, bits) -> elements on which restate_f32 differs from the exact twin, summed over SHAPES (random_inputs)
ENVELOPE = {("bfloat16", 0): 0, ("bfloat16", 4): 0, ("bfloat16", 8): 0,
            ("float16", 0): 9, ("float16", 4): 11, ("float16", 8): 10}


def one_ulp(dtype: str, *values: np.ndarray) -> np.ndarray:
    """The spacing of ``dtype`` at the largest of the |values| (two neighbours across a power of two are one ulp apart)."""
    from moe_ref import ulp

    return ulp(np.maximum.reduce([np.abs(np.asarray(v, np.float64)) for v in values]), dtype)


def _pack(q: np.ndarray, bits: int) -> np.ndarray:
    per = 32 // bits
    n, k = q.shape
    shifts = (np.arange(per, dtype=np.uint32) * bits).astype(np.uint32)
    return np.bitwise_or.reduce(q.astype(np.uint32).reshape(n, k // per, per) << shifts, axis=-1).astype(np.uint32)


def exact_inputs(N: int, K: int, r: int, dtype: str, bits: int, dora: bool):
    """-> dict(w | packed, scales, biases; a, b, s, m)"""
    rng = np.random.default_rng([SEED, 1, N, K, r, bits, int(dora)])
    out = dict(a=rng.integers(-3, 4, (K, r)).astype(np.float32), b=rng.integers(-3, 4, (r, N)).astype(np.float32), s=0.125,
               m=np.exp2(rng.integers(-2, 3, N)).astype(np.float32) if dora else None)
    if bits == 0:
        out["w"] = (rng.integers(-4, 5, (N, K)) / 8.0).astype(np.float32)
    else:
        out["packed"] = _pack(rng.integers(0, 1 << bits, (N, K)), bits)
        out["scales"] = np.full((N, K // 64), 0.125, np.float32)
        out["biases"] = (rng.integers(-4, 5, (N, K // 64)) / 8.0).astype(np.float32)
    return out


def random_inputs(N: int, K: int, r: int, dtype: str, bits: int, dora: bool = False, seed: int = 0):
    rng = np.random.default_rng([SEED, 2, N, K, r, seed])
    w = round_to((0.05 * rng.standard_normal((N, K))).astype(np.float32), dtype)
    out = dict(a=(rng.uniform(-1, 1, (K, r)) / np.sqrt(K)).astype(np.float32), b=(0.3 * rng.standard_normal((r, N))).astype(np.float32),
               s=4.0, m=(0.5 + rng.random(N)).astype(np.float32) if dora else None)
    if bits == 0:
        out["w"] = w
    else:
        out["packed"], out["scales"], out["biases"] = ref_quant.quantize(w, 64, bits, dtype)
    return out


def base_f32(inp, dtype: str, bits: int) -> np.ndarray:
    """step 1 as the float32 program runs it: the multiply-add rounded to float32, then to T"""
    if bits == 0:
        return inp["w"]
    q = ref_quant.unpack(inp["packed"], bits).astype(np.float64)
    n, k = q.shape
    v = q.reshape(n, k // 64, 64) * inp["scales"].astype(np.float64)[..., None] + inp["biases"].astype(np.float64)[..., None]
    return round_to(v.reshape(n, k).astype(np.float32), dtype)                  # (the float64 value is exact: one fmaf)


def restate_f32(inp, dtype: str, bits: int, descending: bool = False, sum_before_rounding: bool = False) -> np.ndarray:
    """steps 1-4 in float32 -> Wm.  The two flags are the deliberately wrong variants: the rank terms in descending j, and
    the factors multiplied BEFORE they are rounded to T."""
    wd = base_f32(inp, dtype, bits)
    bp = np.float32(inp["s"]) * inp["b"].T.astype(np.float32)
    ap = inp["a"].T.astype(np.float32)
    if not sum_before_rounding:
        bp, ap = round_to(bp, dtype), round_to(ap, dtype)
    d = np.zeros(wd.shape, np.float32)
    r = bp.shape[1]
    for j in (range(r - 1, -1, -1) if descending else range(r)):
        d = (bp[:, j:j + 1] * ap[j:j + 1, :] + d).astype(np.float32)            # (the product of two T values is exact in float32)
    return round_to(wd + round_to(d, dtype), dtype)


def exact_is_exact(inp, dtype: str, bits: int) -> bool:
    """Are all float32 sums of steps 1-5 on these inputs exact in any order?  Every term is a multiple of one quantum and the
    sum of the terms' magnitudes stays below 2^24 quanta."""
    import merge_ref

    wd = merge_ref.dequant_T(inp["packed"], inp["scales"], inp["biases"], bits, "float32") if bits else inp["w"].astype(np.float64)
    quantum = 0.125                                                             # W and s a b in eighths
    rank_terms = np.abs(inp["s"] * inp["b"].T.astype(np.float64)) @ np.abs(inp["a"].T.astype(np.float64))
    ok = bool(((rank_terms + np.abs(wd)) / quantum < 2 ** 24).all())
    ok &= bool(np.all(np.mod(np.asarray(wd, np.float64) / quantum, 1.0) == 0))
    if inp["m"] is not None:                                                    # Wm: eighths still (a rounding to T drops low bits only)
        wm = merge_ref.merge_lora(wd, inp["a"], inp["b"], inp["s"], dtype).astype(np.float64)
        ok &= bool(np.all(np.mod(wm / quantum, 1.0) == 0)) and bool(((wm * wm).sum(axis=1) / quantum ** 2 < 2 ** 24).all())
    return ok
