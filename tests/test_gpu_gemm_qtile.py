"""The prefill tile GEMM on packed int4 / int8 group-64 weights at kernel level (-m gpu): mi_op_gemm_prefill_q (gemm_qtile.hip).

Against float64 NumPy round_to(x . (s q + b)^T) under test_gpu_kernels._assert_close (2 units at worst, 90 % within half a unit)
for every epilogue, at shapes that reach a ragged row tile (129), several row tiles and the K split (300 x 384 x 1024), a ragged
N tile (208), one block of int4 (K 128) and an odd block count (384).  exact: codes drawn directly, scales 2^-1..2^-3, biases =
scale x integer, x small integers -- every partial sum is an exact float32 in any order, so the output equals the reference bit for
bit (a wrong lane map or a wrong group's scale cannot pass).  Then: two runs give equal bits, rows do not see each other, and what
the kernel does not take is refused with the output untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import TDT, dev, dev_u32, gemv_args, host, op_linear, to_tiled  # noqa: E402
from oracle import ref_quant  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402

BITS_ACT = [(b, a) for b in (4, 8) for a in ("bfloat16", "float16")]


def _linear(kind_bits, act, packed, s, b, *, group=64, bias=None, tiled=True):
    """-> (op_linear on the device, keepalive).  packed: uint32 codes as the checkpoint holds them; s, b: [N][K / group]"""
    N, K = s.shape[0], s.shape[1] * group
    keep = [dev_u32(packed), dev(s, act), dev(b, act)]
    ol = op_linear(f"q{kind_bits}_{'bf16' if act == 'bfloat16' else 'f16'}", N, K, *keep, group=group)
    if tiled:
        assert to_tiled(ol, keep)
    if bias is not None:
        keep.append(dev(bias))
        ol.bias = keep[-1].data_ptr()
    return ol, keep


def _random(rng, bits, act, N, K, group=64):
    packed, s, b = ref_quant.quantize(rng.standard_normal((N, K)).astype(np.float32) * 0.05, group, bits, dtype=act)
    return packed, s, b, ref_quant.dequantize(packed, s, b, group, bits).astype(np.float64)


def _run(ol, x, M, act, epi, out, pair=0):
    """one launch on x[:M] -> the return code; out is the output (the residual stream for EPI_RESID)"""
    xd = x if torch.is_tensor(x) else dev(x, act)
    a = gemv_args(xd, M, act, epi=epi, ldo=out.shape[1], pair_offset=pair, **{"resid" if epi == L.EPI_RESID else "out": out})
    torch.cuda.synchronize()
    rc = L.lib().mi_op_gemm_prefill_q(C.byref(ol), C.byref(a), 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("M,N,K,epi", [(129, 208, 128, "store"), (300, 384, 1024, "resid"), (129, 384, 384, "f32"),
                                       (300, 416, 384, "swiglu"), (129, 208, 1024, "bias")])
@pytest.mark.parametrize("bits,act", BITS_ACT)
def test_against_float64(bits, act, M, N, K, epi):
    rng = np.random.default_rng(bits * 100 + M + N + K)
    packed, s, b, w = _random(rng, bits, act, N, K)
    bias = rng.standard_normal(N).astype(np.float32) if epi == "bias" else None
    ol, keep = _linear(bits, act, packed, s, b, bias=bias)
    x = round_to(rng.standard_normal((M, K)), act)
    y = x.astype(np.float64) @ w.T
    if epi == "swiglu":
        I = N // 2
        out = torch.full((M + 16, I), 7.0, dtype=TDT[act], device="cuda")
        L.check(_run(ol, x, M, act, L.EPI_SWIGLU, out, pair=I))
        gt, up = round_to(y[:, :I], act), round_to(y[:, I:], act)
        sig = round_to(1.0 / (1.0 + np.exp(-gt.astype(np.float64))), act)
        want, scale = round_to(round_to(gt * sig, act) * up, act), float(np.abs(y).max())
    elif epi == "resid":
        h0 = round_to(rng.standard_normal((M + 16, N)), act)
        out = dev(h0, act)
        L.check(_run(ol, x, M, act, L.EPI_RESID, out))
        want, scale = round_to(h0[:M] + round_to(y, act), act), None
        assert np.array_equal(host(out)[M:], h0[M:])
    else:
        out = torch.full((M + 16, N), 7.0, dtype=torch.float32 if epi == "f32" else TDT[act], device="cuda")
        L.check(_run(ol, x, M, act, L.EPI_STORE_F32 if epi == "f32" else L.EPI_STORE, out))
        want, scale = round_to(y, act), None
        if bias is not None:
            want = round_to(want + bias, act)
    got = host(out)
    if epi != "resid":
        assert np.all(got[M:] == 7.0)                  # the rows past M are not written
    _assert_close(got[:M], want, act, scale=scale)


@pytest.mark.parametrize("M,N,K", [(129, 208, 384), (300, 384, 1024)])
@pytest.mark.parametrize("bits,act", BITS_ACT)
def test_exact(bits, act, M, N, K):
    rng = np.random.default_rng(bits + M)
    q = rng.integers(0, 1 << bits, size=(N, K))
    s = 2.0 ** -rng.integers(1, 4, size=(N, K // 64)).astype(np.float64)
    b = s * rng.integers(-(1 << bits) + 1, 1, size=(N, K // 64))
    per = 32 // bits
    packed = (q.reshape(N, -1, per).astype(np.uint32) << (np.arange(per, dtype=np.uint32) * bits)).sum(-1).astype(np.uint32)
    assert np.array_equal(ref_quant.unpack(packed, bits), q)
    ol, keep = _linear(bits, act, packed, s, b)
    x = rng.integers(-4, 5, size=(M, K)).astype(np.float64)
    w = np.repeat(s, 64, axis=1) * q + np.repeat(b, 64, axis=1)
    out = torch.zeros((M, N), dtype=TDT[act], device="cuda")
    L.check(_run(ol, x, M, act, L.EPI_STORE, out))
    assert np.array_equal(host(out), round_to(x @ w.T, act))


def test_deterministic_and_rows_independent():
    rng = np.random.default_rng(7)
    M, N, K, act, kept = 300, 384, 1024, "bfloat16", [0, 127, 128, 299]
    packed, s, b, _ = _random(rng, 4, act, N, K)
    ol, keep = _linear(4, act, packed, s, b)
    x = round_to(rng.standard_normal((M, K)), act)
    outs = []
    for xi in (x, x, np.where(np.isin(np.arange(M), kept)[:, None], x, round_to(rng.standard_normal((M, K)) * 3, act))):
        outs.append(torch.zeros((M, N), dtype=TDT[act], device="cuda"))
        L.check(_run(ol, xi, M, act, L.EPI_STORE, outs[-1]))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][kept], outs[2][kept]) and not torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("what", ["float32 activations", "row-major", "group 32", "3 bits"])
def test_refusals(what):
    rng = np.random.default_rng(3)
    M, N, K, act = 129, 32, 128, "bfloat16"
    group, bits = (32 if what == "group 32" else 64), (3 if what == "3 bits" else 4)
    packed, s, b, _ = _random(rng, 4, act, N, K, group)
    if bits == 3:
        packed = np.zeros((N, K * 3 // 32), dtype=np.uint32)
    ol, keep = _linear(bits, act, packed, s, b, group=group, tiled=what != "row-major")
    xact = "float32" if what == "float32 activations" else act
    out = torch.full((M, N), 7.0, dtype=TDT[xact], device="cuda")
    assert _run(ol, rng.standard_normal((M, K)), M, xact, L.EPI_STORE, out) == -3          # MI_ERR_UNSUPPORTED
    assert bool((out == 7.0).all())
