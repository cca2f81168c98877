"""Kernel-level parity (-m gpu) of the resident form of gemv_f32.hip -- the one-pass weight stream of gemv_f32_kernel with x
and the norm weights staged once per workgroup and kept in LDS (the gate|up and lm_head launches of a float32-KV decode
step at K <= 4096) -- through mi_op_gemv_f32_resident (include/mi355_ops.h).

The form splits x, multiplies and sums exactly as gemv_f32_kernel does, so every output must be BIT-IDENTICAL to
mi_op_gemv_f32 on the same call (np.array_equal over the whole guarded buffer, no tolerance), besides passing the project's
float32 criterion against the oracle's float64 product (test_gpu_kernels._assert_close; scale 4.0 for the residual form).
Each shape runs the plain, float32, residual and SwiGLU epilogues, each with and without the RMSNorm prologue.

Shapes are (M, whole tiles per CU, extra tiles, K), the smallest at which this form can go wrong; what each is for stands
next to it.  x always lives in an allocation of 8 rows whose rows beyond M - 1 are NaN: with fewer than 8 rows the image rows
of the missing rows may hold anything, and nothing of them may reach an output."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ref_model

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, gemv_args, host, op_linear  # noqa: E402
from test_gpu_gemv_f32 import EPS, _check_guard, _cus, _guarded, _oracle_nt, _swiglu, _wide_x, gemv_f32  # noqa: E402
from test_gpu_gemv_f32 import _weight as _f32_weight  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402

RNG = np.random.default_rng(40962)      # h, the residual form's x and the norm weights; weights and the wide x come from test_gpu_gemv_f32's helpers
MI_ERR_UNSUPPORTED = -3
_weight = functools.lru_cache(maxsize=None)(_f32_weight)      # tile-major bf16 weights: made once per (N, K), never written


def resident(ol, x, M, *, epi=0, out=None, ldo=0, resid=None, pair_offset=0, norm_w=None, eps=0.0, iters=0):
    a = gemv_args(x, M, "float32", pro=1 if norm_w is not None else 0, norm_w=norm_w, eps=eps, epi=epi, out=out, ldo=ldo,
                  resid=resid, pair_offset=pair_offset)
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    L.check(L.lib().mi_op_gemv_f32_resident(C.byref(ol), C.byref(a), int(iters), C.byref(ms)))
    return ms.value if iters >= 1 else None


def _x_dev(x):
    """x in an allocation of 8 rows, NaN beyond its own"""
    full = np.full((8, x.shape[1]), np.nan, np.float32)
    full[:x.shape[0]] = x
    return dev(full, "float32")


def _three(ol, xd, M, cols, want, *, scale=None, h=None, **kw):
    """The call twice on the resident form and once on gemv_f32_kernel, each on a fresh guarded buffer (holding h for the
    residual form): guard intact, run-to-run equal, bit-identical between the kernels, finite, close to `want`."""
    got = []
    for run in (resident, resident, gemv_f32):
        buf = _guarded(M, cols)
        if h is not None:
            buf[:M, :cols] = h
            run(ol, xd, M, resid=buf, ldo=cols + 16, **kw)
        else:
            run(ol, xd, M, out=buf, ldo=cols + 16, **kw)
        got.append(host(buf))
        _check_guard(got[-1], M, cols)
    assert np.array_equal(got[0], got[1]), "two runs differ"
    assert np.array_equal(got[0], got[2]), "not bit-identical to gemv_f32_kernel"
    assert np.all(np.isfinite(got[0])), "a non-finite output"
    _assert_close(got[0][:M, :cols], want, "float32", scale=scale)
    return got[0]


def _all_epilogues(ol, w, M, N, x, x1, h, norm_w):
    """EPI_STORE, EPI_STORE_F32, EPI_RESID (on x1 and h) and EPI_SWIGLU, with the prologue that `norm_w` selects"""
    kw = {}
    xo, x1o = x, x1
    if norm_w is not None:
        kw = dict(norm_w=dev(norm_w, "float32"), eps=EPS)
        xo = ref_model.rms_norm(x, "float32", norm_w, "float32", EPS)[0]
        x1o = ref_model.rms_norm(x1, "float32", norm_w, "float32", EPS)[0]
    xd, x1d = _x_dev(x), _x_dev(x1)
    want = _oracle_nt(xo, w)
    _three(ol, xd, M, N, want, epi=L.EPI_STORE, **kw)
    _three(ol, xd, M, N, want, epi=L.EPI_STORE_F32, **kw)
    _three(ol, x1d, M, N, h + _oracle_nt(x1o, w), scale=4.0, h=dev(h, "float32"), epi=L.EPI_RESID, **kw)
    if N % 32 == 0:
        I = N // 2
        _three(ol, xd, M, I, _swiglu(want[:, :I], want[:, I:]), epi=L.EPI_SWIGLU, pair_offset=I, **kw)


# (M, whole tiles per CU, extra tiles, K)
SHAPES = [
    (1, 0, 5, 64),          # five workgroups of one tile, six waves idle
    (3, 3, 0, 1024),        # one chunk
    (8, 8, 0, 1536),        # a ragged second chunk
    (8, 16, 5, 256),        # two full passes with the roll, then a pass of one tile: x must survive the passes unstaged
    (8, 9, 0, 1056),        # a full pass, then a pass of one tile; the last chunk holds one k-block
    (8, 16, 0, 2048),       # two full passes over two chunks
    (8, 7, 0, 4096),        # Mistral's pass: every image block of every wave in use, LDS at its limit
    (3, 1, 0, 4096),        # LDS at its limit with fewer than 8 rows
    (1, 7, 0, 1056), (8, 4, 0, 1056), (3, 5, 0, 1056), (8, 6, 0, 1056), (3, 2, 0, 1056),      # the remaining pass sizes
]


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("M,per_cu,extra,K", SHAPES)
def test_bit_identical_to_gemv_f32_and_close_to_oracle(M, per_cu, extra, K, norm):
    N = 16 * (per_cu * _cus() + extra)
    ol, w, keep = _weight(N, K)
    x = _wide_x(M, K)
    x1 = RNG.standard_normal((M, K)).astype(np.float32)
    h = RNG.standard_normal((M, N)).astype(np.float32)
    nw = (1.0 + 0.3 * RNG.standard_normal(K)).astype(np.float32) if norm else None
    _all_epilogues(ol, w, M, N, x, x1, h, nw)


def test_row_scale_counts_the_last_block():
    """PRO_NORM, K = 1536 (a ragged second chunk): row 2 of x is ~1e-3 everywhere but for one element of 1000 in the last
    k-block of the last chunk (block 47: wave 7's second block of chunk 1), which is then all of the row's sum of squares.
    A block that is missing from the sums, or counted twice, moves rs -- and every output of the row -- by far more than
    the float32 criterion allows: without the block rs is ~1e6 times too large, twice counted it is 0.71 of its value."""
    M, K = 8, 1536
    N = 16 * 8 * _cus()
    ol, w, keep = _weight(N, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    x[2] *= np.float32(1e-3)
    x[2, K - 3] = np.float32(1000.0)
    nw = (1.0 + 0.3 * RNG.standard_normal(K)).astype(np.float32)
    xn = ref_model.rms_norm(x, "float32", nw, "float32", EPS)[0]
    _three(ol, _x_dev(x), M, N, _oracle_nt(xn, w), epi=L.EPI_STORE, norm_w=dev(nw, "float32"), eps=EPS)


def test_calls_outside_the_kernel_are_refused():
    """No quiet fall-back: each of these returns MI_ERR_UNSUPPORTED and leaves the output as it was, next to a call that
    this entry point accepts."""
    lib, ms = L.lib(), C.c_float(0.0)
    out = torch.full((9, 64), 7.0, dtype=torch.float32, device="cuda")

    def rc(ol, a):
        torch.cuda.synchronize()
        r = lib.mi_op_gemv_f32_resident(C.byref(ol), C.byref(a), 0, C.byref(ms))
        torch.cuda.synchronize()
        return r

    def refused(ol, a):
        assert rc(ol, a) == MI_ERR_UNSUPPORTED
        assert bool(torch.all(out == 7.0)), "a refused call wrote its output"

    N, K = 64, 64
    ol, w, keep = _weight(N, K)
    xd = dev(RNG.standard_normal((9, K)).astype(np.float32), "float32")
    # K = 5120 (Qwen3-14B: the images do not fit) and K = 4128 (17 k-blocks for wave 0)
    for Kb in (5120, 4128):
        olk, _, _ = _weight(16, Kb)
        xk = dev(RNG.standard_normal((8, Kb)).astype(np.float32), "float32")
        refused(olk, gemv_args(xk, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64))
    # 9 rows
    refused(ol, gemv_args(xd, 9, "float32", epi=L.EPI_STORE, out=out, ldo=64))
    # a biased linear (a copy of the descriptor: the cached one stays as it is)
    olb = L.OpLinear.from_buffer_copy(ol)
    bd = dev(RNG.standard_normal(N).astype(np.float32), "float32")
    olb.bias = bd.data_ptr()
    refused(olb, gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64))
    # row-major weights
    wd = dev(w, "bfloat16")
    refused(op_linear("bf16", N, K, wd), gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64))
    # quantised weights (the descriptor alone decides: nothing is launched, so nothing is read)
    olq = L.OpLinear.from_buffer_copy(ol)
    olq.wk = L.WK["q4_bf16"]
    refused(olq, gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64))
    # ... and the call itself is taken
    assert rc(ol, gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64)) == 0
    assert not bool(torch.any(out[:8] == 7.0))
