"""mxfp8 weights at kernel level (-m gpu) against float64 NumPy x . W_hat^T, bit for bit.  every code: x is the identity, so the
output IS W_hat^T -- all 254 finite E4M3 codes under scale bytes 10 / 120 / 127 / 246.  accumulation: the 50 codes with exponent
fields 7..9 and +-0 (multiples of 2^-3 up to 7.5), scale bytes 124..126, x integers in -3..3: every partial sum is a multiple of
2^-6 below 1024 x 3 x 3.75 < 2^14, an exact float32 in any order (SwiGLU: the rule of tests/test_gpu_qgroup_kernels.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L, quant  # noqa: E402
from gpu_helpers import TDT, dev, dev_i32, gemm_skinny, gemv, op_linear, ptr, to_tiled  # noqa: E402
from oracle.numerics import round_to  # noqa: E402
from test_gpu_qgroup_kernels import KS, _one_hot, _probes, _rule, _run  # noqa: E402  (launch, one-hot probes, the SwiGLU rule)

ACT = "bfloat16"
EXACT = np.array([0x00, 0x80] + [s | e << 3 | m for s in (0, 0x80) for e in (7, 8, 9) for m in range(8)])


def _linear(q, s, kind="mx8_bf16", bias=None, tiled=True):
    N, K = q.shape
    w = torch.from_numpy(q.astype(np.uint8)).view(torch.float8_e4m3fn).double().numpy() * np.repeat(2.0 ** (s - 127.0), 32, axis=1)
    keep = [quant.pack_codes(torch.from_numpy(q), 8).cuda(), torch.from_numpy(s.astype(np.uint8)).cuda()]
    ol = op_linear(kind, N, K, *keep, group=32)
    if tiled:
        assert int(L.lib().mi_op_tiled_bytes(C.byref(ol))) == N * K + N * K // 32
        assert to_tiled(ol, keep)
    if bias is not None:
        keep.append(torch.from_numpy(bias.astype(np.float32)).cuda())
        ol.bias = keep[-1].data_ptr()
    return ol, keep, w


def _weights(rng, N, K, **kw):
    return _linear(EXACT[rng.integers(0, len(EXACT), size=(N, K))], rng.integers(124, 127, size=(N, K // 32)), **kw)


@pytest.mark.parametrize("route", ["skinny", "prefill", "gemv_tiled", "gemv_rows", "embed"])
def test_every_code(route):
    q = (128 * np.arange(16)[:, None] + np.arange(128)[None, :]) % 256
    q[(q & 0x7f) == 0x7f] = 0
    ol, keep, w = _linear(q, np.tile(np.array([10, 120, 127, 246]), (16, 1)), tiled=route != "gemv_rows")
    eye = np.eye(128)
    if route == "skinny":
        got = _run(ol, eye, ACT, L.EPI_STORE, 16)
    elif route == "prefill":
        got = _run(ol, np.concatenate([eye, np.zeros((32, 128))]), ACT, L.EPI_STORE, 16, prefill=True)
        assert not got[128:].any()
        got = got[:128]
    elif route == "embed":
        toks, rows = dev_i32(np.arange(16)), torch.zeros((16, 128), dtype=TDT[ACT], device="cuda")
        L.check(L.lib().mi_op_embed(C.byref(ol), ptr(toks), 16, L.MI_BF16, 0, ptr(rows)))
        torch.cuda.synchronize()
        got = rows.float().cpu().numpy().T
    else:
        out = torch.zeros((128, 16), dtype=TDT[ACT], device="cuda")
        for r in range(0, 128, 8):                                       # (the generic kernel takes 8 rows a call)
            assert not gemv(ol, dev(eye[r:r + 8], ACT), 8, ACT, out=out[r:r + 8], ldo=16)
        torch.cuda.synchronize()
        got = out.float().cpu().numpy()
    assert np.array_equal(got, w.T), route


@pytest.mark.parametrize("rows", [1, 8, 17, 33, 128])
def test_decode(rows):
    rng = np.random.default_rng(8000 + rows)
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
        assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE, N, ksplit=ks), want), ("a second launch", K)
    K, N = 384, 48                             # a linear bias on 3 tiles (the last unit holds one tile): T(T(acc) + b)
    lb = rng.integers(-8, 9, size=N).astype(np.float64)
    ol, keep, w = _weights(rng, N, K, bias=lb)
    x = rng.integers(-3, 4, size=(rows, K)).astype(np.float64)
    assert np.array_equal(_run(ol, x, ACT, L.EPI_STORE, N, ksplit=2), round_to(round_to(x @ w.T, ACT) + lb, ACT)), "bias"
    K, I = 384, 32                             # SwiGLU on gate|up: x in sixteenths, g and u are exact sums, the sigmoid is not
    ol, keep, w = _weights(rng, 2 * I, K)
    x = rng.integers(-3, 4, size=(rows, K)) / 16.0
    y = round_to(x @ w.T, ACT).astype(np.float64)
    g, u = y[:, :I], y[:, I:]
    with np.errstate(over="ignore"):
        sw = round_to(round_to(g * round_to(1.0 / (1.0 + np.exp(-g)), ACT), ACT) * u, ACT)
    _rule(_run(ol, x, ACT, L.EPI_SWIGLU, I, ksplit=2, pair=I), sw, ACT, f"swiglu mx8 m{rows}")


@pytest.mark.parametrize("case", ["f16", "group64", "row_major", "rows129"])
def test_refusals(case):
    rng = np.random.default_rng(129)
    act, rows = ("float16" if case == "f16" else ACT), (129 if case == "rows129" else 8)
    ol, keep, _ = _weights(rng, 32, 128, tiled=case != "row_major")
    if case == "group64":
        ol.group = 64
    out = torch.full((rows, 32), 7.0, dtype=TDT[act], device="cuda")
    x = dev(rng.integers(-3, 4, size=(rows, 128)), act)
    assert gemm_skinny(ol, x, rows, act, out=out, ldo=32, check=False) == -3      # MI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 7.0).all()
