"""3- and 6-bit weights at kernel level (-m gpu): mi_op_gemm_skinny (gemm_q36.hip, 1..128 rows, explicit ksplit) and
mi_op_gemm_prefill (the [hi | lo] copy of the bit planes) against float64 NumPy x . (s q + b)^T.
exact: x integers, scales 2^-3..2^-1, biases = scale x integer -- every summation order and offset form is exact: bit for bit
(SwiGLU goes through expf: the rule, as tests/skinny_cases.py holds its own).  one-hot: an output row IS a column of W_hat;
probes on both sides of 3-byte units, dwords, groups, blocks, slice bounds, and K - 1: bit for bit.  random: quant.quantize
weights under attn16_cases.rule_stats with skinny_cases.RULE_CAP.  The cap holds on these inputs: the oracle's float32 envelopes
(tests/test_quant36_host.py, same random_case) show at most 2 of 4128 elements = 0.048 % beyond half a unit (q3 float16, 129 rows,
f32_pairwise; worst element 0.755 unit) against the cap's 0.235 %, and 0 on every decode shape."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L, quant  # noqa: E402
from gpu_helpers import TDT, dev, dev_i32, gemm_prefill, gemm_skinny, gemv, op_linear, ptr, to_tiled  # noqa: E402
from attn16_cases import rule_stats  # noqa: E402
from skinny_cases import RULE_CAP  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_quant36_host import random_case, w_hat as _w_hat  # noqa: E402

KS = {128: (1,), 384: (1, 2, 3), 1024: (2, 3)}       # K -> forced K slices (384: an odd block count; uneven slices at 2 / 3)


def _exact_w(rng, bits, N, K):
    q = rng.integers(0, 1 << bits, size=(N, K))
    s = 2.0 ** -rng.integers(1, 4, size=(N, K // 64)).astype(np.float64)
    b = s * rng.integers(-(1 << bits) + 1, 1, size=(N, K // 64))
    return q, s, b


def _linear(bits, act, q, s, b, bias=None):
    N, K = q.shape
    keep = [quant.pack_codes(torch.from_numpy(q), bits).cuda(), dev(s, act), dev(b, act)]
    ol = op_linear(f"q{bits}_{'bf16' if act == 'bfloat16' else 'f16'}", N, K, *keep)
    nbytes = int(L.lib().mi_op_tiled_bytes(C.byref(ol)))
    assert 0 < nbytes <= N * K * bits // 8 + N * (K // 64) * 4          # the resident copy stays packed, no padding
    assert to_tiled(ol, keep)
    if bias is not None:
        keep.append(torch.from_numpy(bias.astype(np.float32)).cuda())
        ol.bias = keep[-1].data_ptr()
    return ol, keep


def _run(ol, x, act, epi, N, *, ksplit=1, h=None, pair=0, prefill=False):
    M = x.shape[0]
    f32 = epi == L.EPI_STORE_F32
    out = dev(h, act) if h is not None else torch.zeros((M, N), dtype=torch.float32 if f32 else TDT[act], device="cuda")
    kw = dict(epi=epi, ldo=N, pair_offset=pair)
    kw["resid" if epi == L.EPI_RESID else "out"] = out
    if prefill:
        gemm_prefill(ol, dev(x, act), M, act, **kw)
    else:
        assert gemm_skinny(ol, dev(x, act), M, act, ksplit=ksplit, **kw)[0] == ksplit
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


def _rule(got, want, act, what):
    worst, frac = rule_stats(got, want, act)
    print(f"RULE {what}: worst {worst:.3f} unit, {100 * frac:.4f} % beyond half a unit")
    assert np.isfinite(got).all() and worst <= 1.0 and frac <= RULE_CAP, (what, worst, frac)


def _probes(bits, K, ksplit):
    unit = 8 if bits == 3 else 4                                        # codes per 3 bytes
    edges = {unit, 2 * unit, 64, 128, K} | {32 * j // bits + 1 for j in range(1, 7)} | {(32 * j + bits - 1) // bits for j in range(1, 7)}
    edges |= {128 * ((s * (K // 128)) // ksplit) for s in range(1, ksplit)} | set(range(192, K, 192))
    return sorted({p for e in edges for p in (e - 1, e) if 0 <= p < K})


@pytest.mark.parametrize("rows", [1, 8, 17, 33, 128])
@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits", [3, 6])
def test_decode(bits, act, rows):
    rng = np.random.default_rng(bits * 1000 + rows)
    N = 32
    for K, splits in KS.items():
        q, s, b = _exact_w(rng, bits, N, K)
        ol, keep = _linear(bits, act, q, s, b)
        w = _w_hat(q, s, b)
        x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
        h = rng.integers(-8, 9, size=(rows, N)).astype(np.float64)
        want = round_to(x @ w.T, act)
        for ks in splits:
            assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, ksplit=ks), want), ("store", K, ks)
            pr = _probes(bits, K, ks)
            for i in range(0, len(pr), rows):                           # one-hot: as many launches as the probes need
                cols = [pr[(i + j) % len(pr)] for j in range(rows)]
                hot = np.zeros((rows, K)); hot[np.arange(rows), cols] = 1.0
                got = _run(ol, hot, act, L.EPI_STORE, N, ksplit=ks)
                assert np.array_equal(got, round_to(w[:, cols].T, act)), ("one-hot", K, ks, cols)
        ks = splits[-1]
        assert np.array_equal(_run(ol, x, act, L.EPI_STORE_F32, N, ksplit=ks), want), ("store_f32", K)
        assert np.array_equal(_run(ol, x, act, L.EPI_RESID, N, ksplit=ks, h=h), round_to(h + want, act)), ("resid", K)
    # a linear bias on 3 tiles (the second unit holds one tile): T(T(acc) + b)
    K, N = 384, 48
    q, s, b = _exact_w(rng, bits, N, K)
    lb = rng.integers(-8, 9, size=N).astype(np.float64)
    ol, keep = _linear(bits, act, q, s, b, bias=lb)
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    want = round_to(round_to(x @ _w_hat(q, s, b).T, act) + lb, act)
    assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, ksplit=2), want), "bias"
    # SwiGLU on gate|up (2 x 32 rows) of exact sums of moderate size (x in sixteenths): g and u are exact, the sigmoid is not
    K, I = 384, 32
    q, s, b = _exact_w(rng, bits, 2 * I, K)
    ol, keep = _linear(bits, act, q, s, b)
    x = rng.integers(-3, 4, size=(rows, K)) / 16.0
    y = round_to(x @ _w_hat(q, s, b).T, act).astype(np.float64)
    g, u = y[:, :I], y[:, I:]
    with np.errstate(over="ignore"):
        sw = round_to(round_to(g * round_to(1.0 / (1.0 + np.exp(-g)), act), act) * u, act)
    _rule(_run(ol, x, act, L.EPI_SWIGLU, I, ksplit=2, pair=I), sw, act, f"swiglu q{bits} {act} m{rows}")
    q, s, b, xr = random_case(bits, act, rows, 1024)
    ol, keep = _linear(bits, act, q, s, b)
    _rule(_run(ol, xr, act, L.EPI_STORE, 32, ksplit=3), round_to(xr @ _w_hat(q, s, b).T, act), act, f"rand q{bits} {act} m{rows}")


@pytest.mark.parametrize("rows", [129, 256])
@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits", [3, 6])
def test_prefill_through_the_hilo_copy(bits, act, rows):
    """more than 128 rows: the tile GEMM on the [hi | lo] copy that dequant_q36_hilo_kernel makes from the bit planes"""
    rng = np.random.default_rng(bits * 1000 + rows)
    N, K = 32, 384
    q, s, b = _exact_w(rng, bits, N, K)
    ol, keep = _linear(bits, act, q, s, b)
    w = _w_hat(q, s, b)                                                 # |q + b / s| < 2^bits: exact in the dtype, lo = 0
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, prefill=True), round_to(x @ w.T, act))
    pr = _probes(bits, K, 1)
    cols = (pr * (rows // len(pr) + 1))[:rows]
    hot = np.zeros((rows, K)); hot[np.arange(rows), cols] = 1.0
    assert np.array_equal(_run(ol, hot, act, L.EPI_STORE, N, prefill=True), round_to(w[:, cols].T, act))
    q, s, b, xr = random_case(bits, act, rows, K)
    ol, keep = _linear(bits, act, q, s, b)
    _rule(_run(ol, xr, act, L.EPI_STORE, N, prefill=True), round_to(xr @ _w_hat(q, s, b).T, act), act, f"prefill q{bits} {act} m{rows}")


@pytest.mark.parametrize("act", ["bfloat16", "float32"])
@pytest.mark.parametrize("bits", [3, 6])
def test_row_major_bit_stream_on_the_generic_kernel_and_the_gather(bits, act):
    """layout 0, K = 192 (no tile-major copy: K % 128 != 0): gemv_v1 and the embedding gather unpack the checkpoint's
    straddling bit stream themselves; float32 activations carry float32 scales (the *_F32 kinds).  Exact data: bit for bit."""
    rng = np.random.default_rng(bits)
    N, K, M = 16, 192, 3
    q, s, b = _exact_w(rng, bits, N, K)
    keep = [quant.pack_codes(torch.from_numpy(q), bits).cuda(), dev(s, act), dev(b, act)]
    ol = op_linear(f"q{bits}_{'bf16' if act == 'bfloat16' else 'f32'}", N, K, *keep)
    assert int(L.lib().mi_op_tiled_bytes(C.byref(ol))) == 0
    w = _w_hat(q, s, b)
    x = rng.integers(-3, 4, size=(M, K)).astype(np.float64)
    out = torch.zeros((M, N), dtype=TDT[act], device="cuda")
    gemv(ol, dev(x, act), M, act, out=out, ldo=N)
    torch.cuda.synchronize()
    assert np.array_equal(out.float().cpu().numpy(), round_to(x @ w.T, act))
    toks = dev_i32([0, 7, 15])
    rows = torch.zeros((3, K), dtype=TDT[act], device="cuda")
    L.check(L.lib().mi_op_embed(C.byref(ol), ptr(toks), 3, L.MI_BF16 if act == "bfloat16" else L.MI_F32, 0, ptr(rows)))
    torch.cuda.synchronize()
    assert np.array_equal(rows.float().cpu().numpy(), round_to(w[[0, 7, 15]], act))
