"""The prefill tile GEMM on packed mxfp4 weights at kernel level (-m gpu): mi_op_gemm_prefill_q with kind mx4_bf16
(qtile_mx4_kernel of gemm_qtile.hip).

Weights as tests/test_gpu_mx4_kernels.py builds them (all 16 codes, scale bytes 124..126), x small integers: every partial sum is
an exact float32 in any order, so the output equals float64 NumPy round_to(x . W_hat^T) BIT FOR BIT -- no tolerance (SwiGLU goes
through expf: the rule of tests/test_gpu_qgroup_kernels.py).  one-hot: an output row IS a column of W_hat; probes on both sides
of every group edge, block edge, K-slice bound, and K - 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import TDT, dev, host  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_gpu_gemm_qtile import _run  # noqa: E402  (one launch of mi_op_gemm_prefill_q -> the return code)
from test_gpu_mx4_kernels import ACT, _weights  # noqa: E402
from test_gpu_qgroup_kernels import _probes, _rule  # noqa: E402


@pytest.mark.parametrize("M,N,K,epi", [(129, 208, 128, "store"), (129, 208, 384, "f32"), (300, 384, 2048, "resid"),
                                       (129, 208, 384, "bias"), (300, 416, 384, "swiglu")])
def test_exact(M, N, K, epi):
    """ragged row tile and N block on one block of K; an odd block count; several row tiles with a K split -- 3 x 3 blocks of
    128 x 128 make the launcher's rule min(8, 512 // 9, (2048 / 64) / 8) = 4 slices of four blocks; a linear bias; SwiGLU with
    pair_offset 208 (a ragged block of 64 gate columns)"""
    rng = np.random.default_rng(M + N + K + len(epi))
    bias = rng.integers(-8, 9, size=N).astype(np.float64) if epi == "bias" else None
    ol, keep, w = _weights(rng, N, K, bias=bias)
    x = rng.integers(-3, 4, size=(M, K)) / (16.0 if epi == "swiglu" else 1.0)
    y = round_to(x @ w.T, ACT).astype(np.float64)
    if epi == "swiglu":
        I = N // 2
        out = torch.full((M + 16, I), 7.0, dtype=TDT[ACT], device="cuda")
        L.check(_run(ol, x, M, ACT, L.EPI_SWIGLU, out, pair=I))
        g, u = y[:, :I], y[:, I:]
        with np.errstate(over="ignore"):
            want = round_to(round_to(g * round_to(1.0 / (1.0 + np.exp(-g)), ACT), ACT) * u, ACT)
        _rule(host(out)[:M], want, ACT, "swiglu mx4 tile")
    elif epi == "resid":
        h0 = rng.integers(-8, 9, size=(M + 16, N)).astype(np.float64)
        out = dev(h0, ACT)
        L.check(_run(ol, x, M, ACT, L.EPI_RESID, out))
        assert np.array_equal(host(out)[:M], round_to(h0[:M] + y, ACT))
        assert np.array_equal(host(out)[M:], h0[M:])
        return
    else:
        out = torch.full((M + 16, N), 7.0, dtype=torch.float32 if epi == "f32" else TDT[ACT], device="cuda")
        L.check(_run(ol, x, M, ACT, L.EPI_STORE_F32 if epi == "f32" else L.EPI_STORE, out))
        assert np.array_equal(host(out)[:M], y if bias is None else round_to(y + bias, ACT))
    assert np.all(host(out)[M:] == 7.0)                    # the rows past M are not written


def test_one_hot_probes():
    rng = np.random.default_rng(11)
    M, N, K = 300, 384, 2048                               # 4 K slices (test_exact)
    ol, keep, w = _weights(rng, N, K)
    pr = _probes(K, 4)
    assert {511, 512, 1535, 1536, 31, 32, 127, 128, K - 1} <= set(pr)
    cols = [pr[i % len(pr)] for i in range(M)]             # every probe is some row's hot column (len(pr) < M)
    assert len(pr) <= M
    hot = np.zeros((M, K)); hot[np.arange(M), cols] = 1.0
    out = torch.zeros((M, N), dtype=TDT[ACT], device="cuda")
    L.check(_run(ol, hot, M, ACT, L.EPI_STORE, out))
    assert np.array_equal(host(out), round_to(w[:, cols].T, ACT))


def test_deterministic_rows_independent_and_refusals():
    rng = np.random.default_rng(7)
    M, N, K, kept = 300, 384, 2048, [0, 127, 128, 299]
    ol, keep, _ = _weights(rng, N, K)
    x = round_to(rng.standard_normal((M, K)), ACT)
    outs = []
    for xi in (x, x, np.where(np.isin(np.arange(M), kept)[:, None], x, round_to(rng.standard_normal((M, K)) * 3, ACT))):
        outs.append(torch.zeros((M, N), dtype=TDT[ACT], device="cuda"))
        L.check(_run(ol, xi, M, ACT, L.EPI_STORE, outs[-1]))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][kept], outs[2][kept]) and not torch.equal(outs[0], outs[2])
    for kind, act, tiled in (("mx4_f32", "float32", True), ("mx4_bf16", "float32", True), ("mx4_bf16", ACT, False)):
        ol, keep, _ = _weights(rng, 32, 128, kind=kind, tiled=tiled)
        out = torch.full((129, 32), 7.0, dtype=TDT[act], device="cuda")
        assert _run(ol, rng.standard_normal((129, 128)), 129, act, L.EPI_STORE, out) == -3, (kind, act, tiled)      # MI_ERR_UNSUPPORTED
        assert bool((out == 7.0).all())
