"""mxfp4 weights at kernel level (-m gpu): mi_op_gemm_skinny (gemm_mx4.hip, 1..128 rows, explicit ksplit), mi_op_gemm_prefill
(the one-term bf16 copy), mi_op_gemv (the generic kernel, both layouts) and mi_op_embed against float64 NumPy x . W_hat^T.
exact: all 16 codes, scale bytes 124..126, x small integers -- every partial sum is an exact float32 in any order: bit for bit
(SwiGLU goes through expf: the rule of tests/test_gpu_qgroup_kernels.py).  one-hot: an output row IS a column of W_hat; probes
on both sides of every group edge, block edge, K-slice bound, and K - 1."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L, quant  # noqa: E402
from gpu_helpers import TDT, dev, dev_i32, gemv, op_linear, ptr, to_tiled  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_gpu_qgroup_kernels import KS, _one_hot, _probes, _rule, _run  # noqa: E402  (launch, one-hot probes, the SwiGLU rule)

ACT = "bfloat16"
GRID = np.array(quant.MXFP4_VALUES)


def _weights(rng, N, K, kind="mx4_bf16", bias=None, tiled=True, sbytes=(124, 127)):
    q = rng.integers(0, 16, size=(N, K))
    s = rng.integers(*sbytes, size=(N, K // 32))
    w = GRID[q & 7] * np.where(q & 8, -1.0, 1.0) * np.repeat(2.0 ** (s - 127.0), 32, axis=1)
    keep = [quant.pack_codes(torch.from_numpy(q), 4).cuda(), torch.from_numpy(s.astype(np.uint8)).cuda()]
    ol = op_linear(kind, N, K, *keep, group=32)
    if tiled:
        assert int(L.lib().mi_op_tiled_bytes(C.byref(ol))) == N * K // 2 + N * K // 32
        assert to_tiled(ol, keep)
    if bias is not None:
        keep.append(torch.from_numpy(bias.astype(np.float32)).cuda())
        ol.bias = keep[-1].data_ptr()
    return ol, keep, w


@pytest.mark.parametrize("rows", [1, 8, 17, 33, 128])
def test_decode(rows):
    rng = np.random.default_rng(4000 + rows)
    N = 32
    for K, splits in KS.items():
        ol, keep, w = _weights(rng, N, K)
        x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
        h = rng.integers(-8, 9, size=(rows, N)).astype(np.float64)
        want = round_to(x @ w.T, ACT)
        for ks in splits:
            assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE, N, ksplit=ks), want), ("store", K, ks)
            _one_hot(ol, w, ACT, rows, N, K, _probes(K, ks), ksplit=ks)
        ks = splits[-1]
        assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE_F32, N, ksplit=ks), want), ("store_f32", K)
        assert np.array_equal(_run(ol, x, ACT, L.EPI_RESID, N, ksplit=ks, h=h), round_to(h + want, ACT)), ("resid", K)
    # a linear bias on 3 tiles (the last unit holds one tile): T(T(acc) + b)
    K, N = 384, 48
    lb = rng.integers(-8, 9, size=N).astype(np.float64)
    ol, keep, w = _weights(rng, N, K, bias=lb)
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE, N, ksplit=2), round_to(round_to(x @ w.T, ACT) + lb, ACT)), "bias"
    # SwiGLU on gate|up (2 x 32 rows): x in sixteenths, g and u are exact sums of moderate size, the sigmoid is not
    K, I = 384, 32
    ol, keep, w = _weights(rng, 2 * I, K)
    x = rng.integers(-3, 4, size=(rows, K)) / 16.0
    y = round_to(x @ w.T, ACT).astype(np.float64)
    g, u = y[:, :I], y[:, I:]
    with np.errstate(over="ignore"):
        sw = round_to(round_to(g * round_to(1.0 / (1.0 + np.exp(-g)), ACT), ACT) * u, ACT)
    _rule(_run(ol, x, ACT, L.EPI_SWIGLU, I, ksplit=2, pair=I), sw, ACT, f"swiglu mx4 m{rows}")


def test_prefill_through_the_one_term_copy():
    """more than 128 rows: the tile GEMM over K (not 2 K) on the exact bf16 copy that dequant_mx4_kernel makes"""
    rng = np.random.default_rng(160)
    rows, N, K = 160, 32, 384
    ol, keep, w = _weights(rng, N, K)
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE, N, prefill=True), round_to(x @ w.T, ACT))
    _one_hot(ol, w, ACT, rows, N, K, _probes(K, 1), prefill=True)


@pytest.mark.parametrize("kind,act,K,tiled,sbytes", [
    ("mx4_f32", "float32", 384, True, (124, 127)), ("mx4_bf16", "float32", 384, True, (124, 127)),
    ("mx4_bf16", "bfloat16", 96, False, (124, 127)), ("mx4_bf16", "bfloat16", 384, True, (124, 127)),
    ("mx4_f32", "float32", 128, True, (0, 1)), ("mx4_f32", "float32", 96, False, (0, 2))])
def test_gemv_and_the_gather_on_either_layout(kind, act, K, tiled, sbytes):
    """the generic kernel (float32 activations; K = 96 has no tile-major form) and mi_op_embed read both layouts.  The last two
    cases hold scale byte 0 (2^-127) alone / beside byte 1: weights and sums are float32 subnormals, multiples of 2^-128 below
    2^-115, so still exact in any order -- a device that flushed them, or a scale read as s << 23, gives zeros"""
    rng = np.random.default_rng(K + tiled + sbytes[0])
    N, M = 32, 5
    ol, keep, w = _weights(rng, N, K, kind=kind, tiled=tiled, sbytes=sbytes)
    assert sbytes[0] or (0 < np.abs(w).max() < 2.0 ** -123)
    assert tiled or int(L.lib().mi_op_tiled_bytes(C.byref(ol))) == 0
    x = rng.integers(-3, 4, size=(M, K)).astype(np.float64)
    out = torch.zeros((M, N), dtype=TDT[act], device="cuda")
    assert not gemv(ol, dev(x, act), M, act, out=out, ldo=N)
    toks = dev_i32([0, 17, 31])
    rows = torch.zeros((3, K), dtype=TDT[act], device="cuda")
    L.check(L.lib().mi_op_embed(C.byref(ol), ptr(toks), 3, L.MI_F32 if act == "float32" else L.MI_BF16, 0, ptr(rows)))
    torch.cuda.synchronize()
    assert np.array_equal(out.float().cpu().numpy(), round_to(x @ w.T, act)), ("gemv", kind, K)
    assert np.array_equal(rows.float().cpu().numpy(), round_to(w[[0, 17, 31]], act)), ("gather", kind, K)
