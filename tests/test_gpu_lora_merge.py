"""mi_lora_merge and mi_quantize_mlx (csrc/lora_merge.hip) through the C ABI alone, no engine (-m gpu), against the twin
tests/merge_ref.py on the cases of tests/merge_cases.py (its docstring has the shapes, the inputs and the measured envelope).

* exact cases: every float32 sum is exact, every rounding determined -- the dense output, the DoRA output and the re-quantised
  triple equal the twin bit for bit.
* random cases, dense output (from a dense, an int4 and an int8 base): every element finite and within one ulp of T of the twin
  (``merge_cases.one_ulp``: at the larger of |delta| and |Wm|, the two roundings to T); the elements that differ at all number at
  most RULE_CAP = 4 times the CPU-measured envelope per dtype and base (``merge_cases.ENVELOPE``; 0 in bfloat16).
* DoRA random cases: the gain is not an output, so its bound is held through the products.  With Wm the kernel's own LoRA-only
  output (held to the twin by the case above), g = m / ||Wm|| in float64 and p = g Wm, the kernel's element is T(float32(g' Wm))
  with |g' - g| <= bound |g|, bound = (ceil(K / 256) + 9 + 2) 2^-24: DESIGN.md §5 "DoRA" without the rank terms (Wm is given
  exactly) -- a thread's k, the wave sum, the four waves, the root and the divide.  So wherever p is farther than
  (bound + 2^-24) |p| from a rounding boundary of T (``dora_ref.near_boundary``'s test, per element) the bits must equal T(p);
  every element is within one ulp; the skipped share stays under 1 %.
* the quantiser equals ``ref_quant.quantize`` bit for bit on random T-valued rows and on the special groups; the re-quantised
  output equals ``ref_quant.quantize`` of the kernel's own dense output; two runs give the same bits; the refusals return their
  codes and leave the outputs untouched.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dora_ref  # noqa: E402
import merge_cases as mc  # noqa: E402
import merge_ref  # noqa: E402
from gpu_helpers import MIDT, TDT, dev, dev_u32, host, ptr  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from oracle import ref_quant  # noqa: E402
from oracle.numerics import round_to  # noqa: E402

U = 2.0 ** -24
INVALID, UNSUPPORTED = -1, -3
SENTINEL = 0x5A


def _u32(t):
    return t.cpu().view(torch.int32).numpy().view(np.uint32)


def _bits16(t):
    return t.cpu().contiguous().view(torch.int16).numpy()


class Out:
    """the output buffers of one call, pre-filled with a sentinel byte"""

    def __init__(self, N, K, dtype, bits, requant):
        def fill(shape, tdt):
            t = torch.empty(shape, dtype=tdt, device="cuda")
            t.view(torch.uint8).fill_(SENTINEL)
            return t

        self.requant = requant
        if requant:
            self.w = fill((N, K * bits // 32), torch.int32)
            self.scales, self.biases = fill((N, K // 64), TDT[dtype]), fill((N, K // 64), TDT[dtype])
        else:
            self.w, self.scales, self.biases = fill((N, K), TDT[dtype]), None, None

    def untouched(self):
        return all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in (self.w, self.scales, self.biases) if t is not None)

    def dense(self):
        return host(self.w)

    def triple(self):
        return _u32(self.w), host(self.scales), host(self.biases)


def upload(inp, dtype, bits):
    d = dict(a=dev(inp["a"]), b=dev(inp["b"]), m=dev(inp["m"]) if inp.get("m") is not None else None)
    if bits:
        d.update(w=dev_u32(inp["packed"]), scales=dev(inp["scales"], dtype), biases=dev(inp["biases"], dtype))
    else:
        d.update(w=dev(inp["w"], dtype), scales=None, biases=None)
    return d


def lora_merge(d, N, K, r, dtype, bits, s, out, *, group=None, dt=None, use_m=True, check=True):
    torch.cuda.synchronize()
    rc = L.lib().mi_lora_merge(0, N, K, r, MIDT[dtype] if dt is None else dt, bits, (64 if bits else 0) if group is None else group,
                               ptr(d["w"]), ptr(d["scales"]), ptr(d["biases"]), ptr(d["a"]), ptr(d["b"]),
                               ptr(d["m"] if use_m else None), float(s), int(out.requant), ptr(out.w), ptr(out.scales), ptr(out.biases))
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


def quantize_mlx(w_d, N, K, dtype, bits, out, *, group=64, dt=None, check=True):
    torch.cuda.synchronize()
    rc = L.lib().mi_quantize_mlx(0, N, K, MIDT[dtype] if dt is None else dt, bits, group, ptr(w_d), ptr(out.w), ptr(out.scales), ptr(out.biases))
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


def same_bits(got: np.ndarray, want: np.ndarray, dtype: str) -> bool:
    return np.array_equal(_bits16(dev(got, dtype)), _bits16(dev(want, dtype)))


def twin_base(inp, dtype, bits):
    return merge_ref.dequant_T(inp["packed"], inp["scales"], inp["biases"], bits, dtype) if bits else inp["w"]


# ------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("bits", mc.BASES)
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_exact_cases_equal_the_twin_bit_for_bit(dtype, bits):
    for N, K, r in mc.SHAPES:
        for dora in ((False, True) if bits == 0 else (False,)):
            inp = mc.exact_inputs(N, K, r, dtype, bits, dora)
            want, _g = merge_ref.merge(twin_base(inp, dtype, bits), inp["a"], inp["b"], inp["m"], inp["s"], dtype)
            d = upload(inp, dtype, bits)
            out = Out(N, K, dtype, bits, False)
            lora_merge(d, N, K, r, dtype, bits, inp["s"], out)
            assert same_bits(out.dense(), want, dtype), (N, K, r, dora, "dense output")
            if bits:
                out = Out(N, K, dtype, bits, True)
                lora_merge(d, N, K, r, dtype, bits, inp["s"], out)
                for g, w, what in zip(out.triple(), ref_quant.quantize(want, 64, bits, dtype), ("codes", "scales", "biases")):
                    assert np.array_equal(g, w), (N, K, r, what)


# ------------------------------------------------------------------------------------------------------------ random cases
@pytest.mark.parametrize("bits", mc.BASES)
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_random_cases_within_one_ulp_and_the_envelope_rule(dtype, bits):
    differ = total = 0
    for N, K, r in mc.SHAPES:
        inp = mc.random_inputs(N, K, r, dtype, bits)
        want = merge_ref.merge_lora(twin_base(inp, dtype, bits), inp["a"], inp["b"], inp["s"], dtype)
        delta = merge_ref.lora_delta(inp["a"], inp["b"], inp["s"], dtype)
        d = upload(inp, dtype, bits)
        outs = []
        for _ in range(2):
            out = Out(N, K, dtype, bits, False)
            lora_merge(d, N, K, r, dtype, bits, inp["s"], out)
            outs.append(out)
        assert np.array_equal(_bits16(outs[0].w), _bits16(outs[1].w)), "two runs differ"
        got = outs[0].dense()
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= mc.one_ulp(dtype, got, want, delta)).all(), (N, K, r, float(err.max()))
        differ += int((got != want).sum())
        total += got.size
    cap = mc.RULE_CAP * mc.ENVELOPE[dtype, bits]
    print(f"RULE {dtype} bits {bits}: the kernel differs from the exact twin on {differ} of {total} elements (cap {cap})")
    assert differ <= cap


# ------------------------------------------------------------------------------------------------------------ DoRA, random
def merged_gain_bound(K: int) -> float:
    return (math.ceil(K / 256) + 9 + 2) * U


def near_boundary_each(p: np.ndarray, dtype: str, rel: float) -> np.ndarray:
    """dora_ref.near_boundary, element by element"""
    a = np.abs(np.asarray(p, np.float64))
    safe = np.where(a > 0, a, 1.0)
    ulp = np.exp2(np.floor(np.log2(safe)) - dora_ref._MANT[dtype])
    frac = safe / ulp - np.floor(safe / ulp)
    return (a > 0) & (np.abs(frac - 0.5) * ulp <= rel * safe)


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_dora_random_cases(dtype):
    skipped = total = 0
    for N, K, r in mc.SHAPES:
        inp = mc.random_inputs(N, K, r, dtype, 0, dora=True)
        d = upload(inp, dtype, 0)
        plain, out = Out(N, K, dtype, 0, False), Out(N, K, dtype, 0, False)
        lora_merge(d, N, K, r, dtype, 0, inp["s"], plain, use_m=False)
        lora_merge(d, N, K, r, dtype, 0, inp["s"], out)
        wm, got = plain.dense(), out.dense()
        g = merge_ref.exact_gain(wm, inp["m"])
        p = g[:, None] * wm.astype(np.float64)
        rel = merged_gain_bound(K) + U
        skip = near_boundary_each(p, dtype, rel)
        assert bool(skip.any()) == dora_ref.near_boundary(p, dtype, rel)
        want = round_to(p.astype(np.float32), dtype)                       # (off the boundaries the double rounding cannot matter)
        assert np.isfinite(got).all()
        assert (np.abs(got.astype(np.float64) - p) <= mc.one_ulp(dtype, got, p)).all(), (N, K, r)
        assert np.array_equal(got[~skip], want[~skip]), (N, K, r, "an element off a rounding boundary moved: the gain is outside its bound")
        assert not np.array_equal(got, wm)
        skipped += int(skip.sum())
        total += skip.size
    print(f"DoRA {dtype}: {skipped} of {total} elements sit on a rounding boundary ({100.0 * skipped / total:.3f} %)")
    assert skipped <= 0.01 * total


def test_dora_bad_norm_or_m_is_refused_and_writes_nothing():
    N, K, r, dtype = 17, 192, 7, "bfloat16"
    inp = mc.exact_inputs(N, K, r, dtype, 0, True)
    lib = L.lib()
    for what in ("zero_row", "inf_m", "nan_m"):
        bad = dict(inp)
        if what == "zero_row":
            bad["w"], bad["b"] = inp["w"].copy(), inp["b"].copy()
            bad["w"][5] = 0.0
            bad["b"][:, 5] = 0.0
        else:
            bad["m"] = inp["m"].copy()
            bad["m"][11] = np.inf if what == "inf_m" else np.nan
        out = Out(N, K, dtype, 0, False)
        assert lora_merge(upload(bad, dtype, 0), N, K, r, dtype, 0, inp["s"], out, check=False) == INVALID, what
        assert (b"row 5" if what == "zero_row" else b"row 11") in lib.mi_last_error()
        assert out.untouched(), what


# ------------------------------------------------------------------------------------------------------------ the quantiser
def special_rows(dtype: str) -> np.ndarray:
    """rows of 128: a random group beside one special group each"""
    rng = np.random.default_rng([mc.SEED, 9])
    rows = []

    def row(special):
        rows.append(np.concatenate([round_to(rng.standard_normal(64).astype(np.float32) * 0.05, dtype), special.astype(np.float32)]))

    row(np.full(64, 0.37))                                           # a constant group
    row(np.full(64, -1.5))
    row(np.zeros(64))                                                # an all-zero group
    row(np.concatenate([[-3.0], rng.random(63) * 0.5]))              # the minimum dominates
    row(-np.abs(rng.standard_normal(64)) - 0.1)                      # all negative
    tiny = 4e-8 if dtype == "bfloat16" else 2.0 ** -24               # |edge / 1e-7| = 0.4: the edge rounds to code 0 (bfloat16);
    row(np.where(np.arange(64) % 2 == 0, tiny, 0.0))                 # float16 has no such value: its smallest gives 0.6, code 1
    row(np.where(np.arange(64) % 2 == 0, -tiny, 0.0))
    row(np.linspace(-1.0, 1.0, 64))                                  # |min| == |max|
    return round_to(np.stack(rows), dtype)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_quantiser_equals_ref_quant_bit_for_bit(dtype, bits):
    rng = np.random.default_rng([mc.SEED, 8, bits])
    cases = {"random": round_to(rng.standard_normal((17, 320)).astype(np.float32) * 0.05, dtype),
             "one_row": round_to(rng.standard_normal((1, 64)).astype(np.float32), dtype), "special": special_rows(dtype)}
    if dtype == "bfloat16":
        q0 = np.rint(np.float32(4e-8) / np.float32(-1e-7))
        assert q0 == 0                                               # the construction does reach the q0 == 0 branch
    for name, w in cases.items():
        N, K = w.shape
        want = ref_quant.quantize(w, 64, bits, dtype)
        outs = []
        for _ in range(2):
            out = Out(N, K, dtype, bits, True)
            quantize_mlx(dev(w, dtype), N, K, dtype, bits, out)
            outs.append(out.triple())
        for g, g2, wv, what in zip(outs[0], outs[1], want, ("codes", "scales", "biases")):
            assert np.array_equal(g, wv), (name, what)
            assert np.array_equal(g, g2), (name, what, "two runs differ")


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_requantised_output_is_the_quantiser_on_the_dense_output(dtype, bits):
    for N, K, r in ((17, 320, 7), (40, 192, 64), (1, 64, 1)):
        inp = mc.random_inputs(N, K, r, dtype, bits)
        d = upload(inp, dtype, bits)
        dense, packed, again = Out(N, K, dtype, bits, False), Out(N, K, dtype, bits, True), Out(N, K, dtype, bits, True)
        lora_merge(d, N, K, r, dtype, bits, inp["s"], dense)
        lora_merge(d, N, K, r, dtype, bits, inp["s"], packed)
        lora_merge(d, N, K, r, dtype, bits, inp["s"], again)
        for g, g2, w in zip(packed.triple(), again.triple(), ref_quant.quantize(dense.dense(), 64, bits, dtype)):
            assert np.array_equal(g, w) and np.array_equal(g, g2)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_codes_and_write_nothing():
    N, K, r, dtype = 17, 192, 7, "bfloat16"
    lib = L.lib()
    dense_in = mc.exact_inputs(N, K, r, dtype, 0, True)
    q_in = dict(mc.exact_inputs(N, K, r, dtype, 4, False), m=dense_in["m"])
    dd, qd = upload(dense_in, dtype, 0), upload(q_in, dtype, 4)

    def refused(code, needle, d, bits, requant, **kw):
        out = Out(N, kw.pop("K", K), dtype, bits or 4, requant)
        rc = lora_merge(d, N, kw.pop("K_arg", K), kw.pop("r", r), dtype, bits, 0.5, out, check=False, **kw)
        assert rc == code, (needle, rc)
        assert needle in lib.mi_last_error(), (needle, lib.mi_last_error())
        assert out.untouched(), needle

    refused(UNSUPPORTED, b"float32", dd, 0, False, dt=L.MI_F32)
    refused(UNSUPPORTED, b"DoRA on a quantised base", qd, 4, True)
    refused(UNSUPPORTED, b"DoRA on a quantised base", qd, 4, False)
    refused(UNSUPPORTED, b"groups of 64", qd, 4, True, group=32, use_m=False)
    refused(UNSUPPORTED, b"groups of 64", qd, 4, True, group=128, use_m=False)
    refused(UNSUPPORTED, b"multiple of 64", qd, 4, False, K_arg=160, use_m=False)
    refused(INVALID, b"rank", dd, 0, False, r=0)
    refused(INVALID, b"rank", dd, 0, False, r=65)
    refused(INVALID, b"quantised input", dd, 0, True)
    refused(INVALID, b"quant_bits", qd, 3, False, use_m=False)
    out = Out(N, K, dtype, 0, False)
    assert lib.mi_lora_merge(0, N, K, r, L.MI_BF16, 0, 0, ptr(dd["w"]), None, None, None, ptr(dd["b"]), None, 0.5, 0, ptr(out.w), None, None) == INVALID
    assert lib.mi_lora_merge(0, N, K, r, L.MI_BF16, 0, 0, ptr(dd["w"]), None, None, ptr(dd["a"]), ptr(dd["b"]), None, float("nan"), 0,
                             ptr(out.w), None, None) == INVALID
    assert lib.mi_lora_merge(99, N, K, r, L.MI_BF16, 0, 0, ptr(dd["w"]), None, None, ptr(dd["a"]), ptr(dd["b"]), None, 0.5, 0,
                             ptr(out.w), None, None) == INVALID and b"device" in lib.mi_last_error()
    assert out.untouched()
    # the quantiser alone
    w_d = dev(dense_in["w"], dtype)
    for code, needle, kw in ((UNSUPPORTED, b"float32", dict(dt=L.MI_F32)), (UNSUPPORTED, b"groups of 64", dict(group=32)),
                             (UNSUPPORTED, b"groups of 64", dict(group=128)), (INVALID, b"quant_bits", dict(bits=2))):
        out = Out(N, K, dtype, 4, True)
        assert quantize_mlx(w_d, N, K, dtype, kw.pop("bits", 4), out, check=False, **kw) == code and needle in lib.mi_last_error()
        assert out.untouched(), needle
    out = Out(N, 192, dtype, 4, True)
    assert quantize_mlx(w_d, N, 160, dtype, 4, out, check=False) == UNSUPPORTED and out.untouched()
    # and the accepted calls do write
    out = Out(N, K, dtype, 0, False)
    lora_merge(dd, N, K, r, dtype, 0, 0.5, out)
    assert not out.untouched()
