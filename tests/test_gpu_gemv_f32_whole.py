"""Kernel-level parity (-m gpu) of the whole-K form of gemv_f32.hip -- one 16-row tile per workgroup over all of K <= 4096,
every load of the launch issued up front (the o_proj launch of a float32-KV decode step) -- through mi_op_gemv_f32_whole
(include/mi355_ops.h).

The form promises more than closeness: it splits x, multiplies and sums exactly as gemv_f32_kernel does, so every output
must be BIT-IDENTICAL to mi_op_gemv_f32 on the same call (np.array_equal over the whole guarded buffer), besides passing
the project's float32 criterion against the oracle's float64 product (test_gpu_kernels._assert_close; scale 4.0 for the
residual form).

Shapes are the smallest at which this kernel can go wrong.  Tiles in {1, 5, CU count}: one workgroup, a few, the full grid.
K decides how many of a wave's 16 load slots are real (wave v owns k-blocks v, v + 8, ...): 32 = one block, wave 0 only;
64; 256 = one block per wave; 288 = wave 0 has two; 1056 = 33 blocks, ragged; 4096 = all 16 slots of every wave.  Rows in
{1, 3, 8}: fewer than 8 rows leave image rows unwritten that no fragment read may touch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, gemv_args, host  # noqa: E402
from test_gpu_gemv_f32 import _check_guard, _cus, _guarded, _oracle_nt, _wide_x, gemv_f32  # noqa: E402
from test_gpu_gemv_f32 import _weight as _f32_weight  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402

RNG = np.random.default_rng(40961)      # h and the residual form's x; weights and the wide x come from test_gpu_gemv_f32's helpers
CU = -1            # "as many tiles as the device has compute units"
_weight = functools.lru_cache(maxsize=None)(_f32_weight)      # tile-major bf16 weights: made once per (N, K), never written


def _n(tiles: int) -> int:
    return 16 * (_cus() if tiles == CU else tiles)


def whole(ol, x, M, *, epi=0, out=None, ldo=0, resid=None, iters=0):
    a = gemv_args(x, M, "float32", epi=epi, out=out, ldo=ldo, resid=resid)
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    L.check(L.lib().mi_op_gemv_f32_whole(C.byref(ol), C.byref(a), int(iters), C.byref(ms)))
    return ms.value if iters >= 1 else None


def _both_stores(ol, w, M, N, K):
    """EPI_STORE (twice) and EPI_STORE_F32 on guarded buffers, against mi_op_gemv_f32 bit for bit and against the oracle"""
    x = _wide_x(M, K)
    xd = dev(x, "float32")
    want = _oracle_nt(x, w)
    ref = _guarded(M, N)
    gemv_f32(ol, xd, M, epi=L.EPI_STORE, out=ref, ldo=N + 16)
    ref = host(ref)
    outs = []
    for epi in (L.EPI_STORE, L.EPI_STORE, L.EPI_STORE_F32):
        out = _guarded(M, N)
        whole(ol, xd, M, epi=epi, out=out, ldo=N + 16)
        outs.append(host(out))
        _check_guard(outs[-1], M, N)
    assert np.array_equal(outs[0], outs[1]), "two runs differ"
    assert np.array_equal(outs[0], ref), "not bit-identical to gemv_f32_kernel (EPI_STORE)"
    ref32 = _guarded(M, N)
    gemv_f32(ol, xd, M, epi=L.EPI_STORE_F32, out=ref32, ldo=N + 16)
    assert np.array_equal(outs[2], host(ref32)), "not bit-identical to gemv_f32_kernel (EPI_STORE_F32)"
    _assert_close(outs[0][:M, :N], want, "float32")
    _assert_close(outs[2][:M, :N], want, "float32")


def _residual(ol, w, M, N, K):
    """EPI_RESID (twice, same h) on a guarded h, against mi_op_gemv_f32 bit for bit and against the oracle"""
    x1 = RNG.standard_normal((M, K)).astype(np.float32)
    h = RNG.standard_normal((M, N)).astype(np.float32)
    x1d, hd = dev(x1, "float32"), dev(h, "float32")
    got = []
    for run in (whole, whole, gemv_f32):
        hbuf = _guarded(M, N)
        hbuf[:M, :N] = hd
        run(ol, x1d, M, epi=L.EPI_RESID, resid=hbuf, ldo=N + 16)
        got.append(host(hbuf))
        _check_guard(got[-1], M, N)
    assert np.array_equal(got[0], got[1]), "two runs differ"
    assert np.array_equal(got[0], got[2]), "not bit-identical to gemv_f32_kernel (EPI_RESID)"
    _assert_close(got[0][:M, :N], h + _oracle_nt(x1, w), "float32", scale=4.0)


# (M, tiles, K): every K with 8 rows and with fewer, every tile count four times
SHAPES = [
    (8, 1, 32), (1, 5, 32),
    (8, 5, 64), (3, CU, 64),
    (8, CU, 256), (1, 1, 256),
    (8, 1, 288), (3, 5, 288),
    (8, 5, 1056), (1, CU, 1056),
    (8, CU, 4096), (3, 1, 4096),
]


@pytest.mark.parametrize("M,tiles,K", SHAPES)
def test_bit_identical_to_gemv_f32_and_close_to_oracle(M, tiles, K):
    N = _n(tiles)
    ol, w, keep = _weight(N, K)
    _both_stores(ol, w, M, N, K)
    _residual(ol, w, M, N, K)


@pytest.mark.parametrize("tiles,K", [(5, 64), (1, 288), (5, 4096)])
def test_lo_term_is_pinned(tiles, K):
    """test_gpu_gemv_f32.test_lo_term_is_pinned on this kernel: one non-zero column per row of x (a different k-block and
    lane group for each row), a float32 with all 24 significant bits in use, so hi, mid and lo are all non-zero.  Every output
    is then hi w + mid w + lo w: three exact products and at most three float32 additions of half an ulp each.  Bound: 4 ulps =
    2^-22 relative to the exact product -- a lost or misplaced `lo` term costs 2^-17, a lost `mid` 2^-9."""
    M, N = 8, _n(tiles)
    ol, w, keep = _weight(N, K)
    x = np.zeros((M, K), np.float32)
    cols = [((5 * m * (K // 64)) % (K // 8)) * 8 + (3 * m) % 8 for m in range(M)]     # distinct 8-wide pieces
    for m, k in enumerate(cols):
        x[m, k] = np.float32((1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23) * 2.0 ** (m - 3)) * (-1.0 if m & 1 else 1.0)
    assert len(set(k // 8 for k in cols)) == M
    want = np.stack([x[m, k].astype(np.float64) * w[:, k].astype(np.float64) for m, k in enumerate(cols)])
    out = _guarded(M, N)
    whole(ol, dev(x, "float32"), M, epi=L.EPI_STORE, out=out, ldo=N + 16)
    got = host(out)
    _check_guard(got, M, N)
    err = np.abs(got[:M, :N].astype(np.float64) - want)
    bound = 2.0 ** -22 * np.abs(want)
    print("max err / |want| in ulps of 2^-24:", float(np.max(err[want != 0] / np.abs(want[want != 0])) * 2.0 ** 24))
    assert np.all(err <= bound), float(np.max(err / np.maximum(np.abs(want), 1e-300)))


def test_production_o_proj():
    """8 x 4096 -> 4096 added to h: the o_proj launch of the Mistral-7B step"""
    M, K, N = 8, 4096, 4096
    ol, w, keep = _weight(N, K)
    _residual(ol, w, M, N, K)


def test_calls_outside_the_kernel_are_refused():
    """No quiet fall-back: each of these is a non-zero return of this entry point, next to a call it accepts."""
    lib, ms = L.lib(), C.c_float(0.0)

    def rc(ol, a):
        torch.cuda.synchronize()
        return lib.mi_op_gemv_f32_whole(C.byref(ol), C.byref(a), 0, C.byref(ms))

    N, K = 64, 64
    ol, w, keep = _weight(N, K)
    xd = dev(RNG.standard_normal((9, K)).astype(np.float32), "float32")
    out = torch.zeros((9, N), dtype=torch.float32, device="cuda")
    assert rc(ol, gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=N)) == 0
    # K above 16 k-blocks per wave
    olk, _, _ = _weight(16, 4128)
    xk = dev(RNG.standard_normal((8, 4128)).astype(np.float32), "float32")
    assert rc(olk, gemv_args(xk, 8, "float32", epi=L.EPI_STORE, out=out, ldo=N)) != 0
    # one tile more than the device has compute units
    Nw = 16 * (_cus() + 1)
    olw, _, _ = _weight(Nw, 32)
    xw = dev(RNG.standard_normal((8, 32)).astype(np.float32), "float32")
    outw = torch.zeros((8, Nw), dtype=torch.float32, device="cuda")
    assert rc(olw, gemv_args(xw, 8, "float32", epi=L.EPI_STORE, out=outw, ldo=Nw)) != 0
    # 9 rows
    assert rc(ol, gemv_args(xd, 9, "float32", epi=L.EPI_STORE, out=out, ldo=N)) != 0
    # logical rounding
    a = gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=N)
    a.rnd = 1
    assert rc(ol, a) != 0
    # 16-bit activations
    xb = dev(RNG.standard_normal((8, K)).astype(np.float32), "bfloat16")
    assert rc(ol, gemv_args(xb, 8, "bfloat16", epi=L.EPI_STORE, out=out, ldo=N)) != 0
    # a norm prologue
    nw = dev(np.ones(K, np.float32), "float32")
    assert rc(ol, gemv_args(xd, 8, "float32", pro=1, norm_w=nw, eps=1e-5, epi=L.EPI_STORE, out=out, ldo=N)) != 0
    # a biased linear (a copy of the descriptor: the cached one stays as it is)
    olb = L.OpLinear.from_buffer_copy(ol)
    bd = dev(RNG.standard_normal(N).astype(np.float32), "float32")
    olb.bias = bd.data_ptr()
    assert rc(olb, gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=N)) != 0
