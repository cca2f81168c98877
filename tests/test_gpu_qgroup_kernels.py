"""int4 / int8 weights in quantisation groups of 32 and 128 at kernel level (-m gpu): mi_op_gemm_skinny (gemm_qg.hip, 1..128
rows, explicit ksplit), mi_op_gemm_prefill(_f32) (the [hi | lo] copy of the new blocks) and mi_op_gemv (the generic kernel on the
same blocks) against float64 NumPy x . (s q + b)^T.
exact: x integers, scales 2^-3..2^-1, biases = scale x integer -- every partial sum is an exact float32 in any order: bit for bit
(SwiGLU goes through expf: the rule).  one-hot: an output row IS a column of W_hat; probes on both sides of every group edge,
block edge, K-slice bound, and K - 1: bit for bit.  random: quant.quantize weights under attn16_cases.rule_stats with
skinny_cases.RULE_CAP.  The cap holds on these inputs: the oracle's float32 envelopes (tests/test_qgroup_host.py, same
random_case) show at most 1 of 4096 elements = 0.024 % beyond half a unit (worst element 0.792 unit: q4 g128 float16, 256 rows, f32_seq32)
against the cap's 0.235 %."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L, quant  # noqa: E402
from gpu_helpers import TDT, dev, dev_i32, gemm_prefill, gemm_prefill_f32, gemm_skinny, gemv, op_linear, ptr, to_tiled  # noqa: E402
from attn16_cases import rule_stats  # noqa: E402
from skinny_cases import RULE_CAP  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402
from test_qgroup_host import random_case, w_hat as _w_hat  # noqa: E402

KS = {128: (1,), 384: (1, 2, 3), 1024: (2, 3)}       # K -> forced K slices (384: an odd block count; uneven slices at 2 / 3)
CASES = [(b, g) for b in (4, 8) for g in (32, 128)]


def _exact_w(rng, bits, group, N, K):
    q = rng.integers(0, 1 << bits, size=(N, K))
    s = 2.0 ** -rng.integers(1, 4, size=(N, K // group)).astype(np.float64)
    b = s * rng.integers(-(1 << bits) + 1, 1, size=(N, K // group))
    return q, s, b


def _linear(bits, group, act, q, s, b, bias=None, tiled=True):
    N, K = q.shape
    keep = [quant.pack_codes(torch.from_numpy(q), bits).cuda(), dev(s, act), dev(b, act)]
    ol = op_linear(f"q{bits}_{'bf16' if act == 'bfloat16' else 'f16'}", N, K, *keep, group=group)
    if tiled:
        nbytes = int(L.lib().mi_op_tiled_bytes(C.byref(ol)))
        assert 0 < nbytes <= N * K * bits // 8 + N * (K // group) * 4       # the resident copy stays packed, no padding
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


def _probes(K, ksplit):
    edges = set(range(32, K + 1, 32)) | {128 * ((s * (K // 128)) // ksplit) for s in range(1, ksplit)}
    return sorted({p for e in edges for p in (e - 1, e) if 0 <= p < K} | {0})


def _one_hot(ol, w, act, rows, N, K, pr, **kw):
    for i in range(0, len(pr), rows):                                   # as many launches as the probes need
        cols = [pr[(i + j) % len(pr)] for j in range(rows)]
        hot = np.zeros((rows, K)); hot[np.arange(rows), cols] = 1.0
        assert np.array_equal(_run(ol, hot, act, L.EPI_STORE, N, **kw), round_to(w[:, cols].T, act)), ("one-hot", K, kw, cols)


@pytest.mark.parametrize("rows", [1, 8, 17, 33, 128])
@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits,group", CASES)
def test_decode(bits, group, act, rows):
    rng = np.random.default_rng(bits * 1000 + group + rows)
    N = 32
    for K, splits in KS.items():
        q, s, b = _exact_w(rng, bits, group, N, K)
        ol, keep = _linear(bits, group, act, q, s, b)
        w = _w_hat(q, s, b)
        x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
        h = rng.integers(-8, 9, size=(rows, N)).astype(np.float64)
        want = round_to(x @ w.T, act)
        for ks in splits:
            assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, ksplit=ks), want), ("store", K, ks)
            _one_hot(ol, w, act, rows, N, K, _probes(K, ks), ksplit=ks)
        ks = splits[-1]
        assert np.array_equal(_run(ol, x, act, L.EPI_STORE_F32, N, ksplit=ks), want), ("store_f32", K)
        assert np.array_equal(_run(ol, x, act, L.EPI_RESID, N, ksplit=ks, h=h), round_to(h + want, act)), ("resid", K)
    # a linear bias on 3 tiles (the second unit holds one tile): T(T(acc) + b)
    K, N = 384, 48
    q, s, b = _exact_w(rng, bits, group, N, K)
    lb = rng.integers(-8, 9, size=N).astype(np.float64)
    ol, keep = _linear(bits, group, act, q, s, b, bias=lb)
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    want = round_to(round_to(x @ _w_hat(q, s, b).T, act) + lb, act)
    assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, ksplit=2), want), "bias"
    # SwiGLU on gate|up (2 x 32 rows) of exact sums of moderate size: g and u are exact, the sigmoid is not.  x in sixteenths at
    # 4 bits; at 8 bits W_hat is 16 times larger and g u would leave float16's range: x in 256ths (sums of < 2^20 units: exact)
    K, I = 384, 32
    q, s, b = _exact_w(rng, bits, group, 2 * I, K)
    ol, keep = _linear(bits, group, act, q, s, b)
    x = rng.integers(-3, 4, size=(rows, K)) / (16.0 if bits == 4 else 256.0)
    y = round_to(x @ _w_hat(q, s, b).T, act).astype(np.float64)
    g, u = y[:, :I], y[:, I:]
    with np.errstate(over="ignore"):
        sw = round_to(round_to(g * round_to(1.0 / (1.0 + np.exp(-g)), act), act) * u, act)
    _rule(_run(ol, x, act, L.EPI_SWIGLU, I, ksplit=2, pair=I), sw, act, f"swiglu q{bits} g{group} {act} m{rows}")
    q, s, b, xr = random_case(bits, group, act, rows, 1024)
    ol, keep = _linear(bits, group, act, q, s, b)
    _rule(_run(ol, xr, act, L.EPI_STORE, 32, ksplit=3), round_to(xr @ _w_hat(q, s, b).T, act), act, f"rand q{bits} g{group} {act} m{rows}")


@pytest.mark.parametrize("rows", [129, 256])
@pytest.mark.parametrize("act", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits,group", CASES)
def test_prefill_through_the_hilo_copy(bits, group, act, rows):
    """more than 128 rows: the tile GEMM on the [hi | lo] copy that dequant_qg_hilo_kernel makes from the blocks"""
    rng = np.random.default_rng(bits * 1000 + group + rows)
    N, K = 32, 384
    q, s, b = _exact_w(rng, bits, group, N, K)
    ol, keep = _linear(bits, group, act, q, s, b)
    w = _w_hat(q, s, b)                                                 # |q + b / s| < 2^bits: exact in the dtype, lo = 0
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    assert np.array_equal(_run(ol, x, act, L.EPI_STORE, N, prefill=True), round_to(x @ w.T, act))
    _one_hot(ol, w, act, rows, N, K, _probes(K, 1), prefill=True)
    q, s, b, xr = random_case(bits, group, act, rows, K)
    ol, keep = _linear(bits, group, act, q, s, b)
    _rule(_run(ol, xr, act, L.EPI_STORE, N, prefill=True), round_to(xr @ _w_hat(q, s, b).T, act), act, f"prefill q{bits} g{group} {act} m{rows}")


@pytest.mark.parametrize("group", [32, 128])
def test_float32_prefill_of_a_bf16_int4_model(group):
    """float32 activations in three bf16 terms against the [hi | lo] copy (the float32-KV prefill): exact data, the float32
    comparison of tests/test_gpu_gemm_prefill_f32.py"""
    rng = np.random.default_rng(group)
    M, N, K = 150, 32, 384
    q, s, b = _exact_w(rng, 4, group, N, K)
    ol, keep = _linear(4, group, "bfloat16", q, s, b)
    x = rng.integers(-3, 4, size=(M, K)).astype(np.float32)
    out = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    gemm_prefill_f32(ol, torch.from_numpy(x).cuda(), M, x_terms=3, out=out, ldo=N)
    torch.cuda.synchronize()
    _assert_close(out.cpu().numpy(), (x.astype(np.float64) @ _w_hat(q, s, b).T).astype(np.float32), "float32")


@pytest.mark.parametrize("bits,group,K", [(b, g, K) for b, g in CASES for K in (192, 384) if K % g == 0])
def test_gemv_and_the_gather_give_the_same_answer_on_either_layout(bits, group, K):
    """mi_op_gemv and mi_op_embed run these groups on the generic kernels: the tile-major blocks (K = 384) and the checkpoint's
    rows (K = 192 has no tile-major form: K % 128 != 0; no rows of 192 exist in groups of 128) give the reference bit for bit on
    exact data"""
    rng = np.random.default_rng(bits + group + K)
    N, M, act = 32, 5, "bfloat16"
    q, s, b = _exact_w(rng, bits, group, N, K)
    w = _w_hat(q, s, b)
    x = rng.integers(-3, 4, size=(M, K)).astype(np.float64)
    toks = dev_i32([0, 17, 31])
    for tiled in (False, K % 128 == 0):
        ol, keep = _linear(bits, group, act, q, s, b, tiled=tiled)
        assert tiled or K % 128 == 0 or int(L.lib().mi_op_tiled_bytes(C.byref(ol))) == 0
        out = torch.zeros((M, N), dtype=TDT[act], device="cuda")
        gemv(ol, dev(x, act), M, act, out=out, ldo=N)
        rows = torch.zeros((3, K), dtype=TDT[act], device="cuda")
        L.check(L.lib().mi_op_embed(C.byref(ol), ptr(toks), 3, L.MI_BF16, 0, ptr(rows)))
        torch.cuda.synchronize()
        assert np.array_equal(out.float().cpu().numpy(), round_to(x @ w.T, act)), ("gemv", tiled, K)
        assert np.array_equal(rows.float().cpu().numpy(), round_to(w[[0, 17, 31]], act)), ("gather", tiled, K)
