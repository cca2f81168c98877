"""Kernel-level parity (-m gpu) of gemv_f32.hip -- the one-pass weight-streaming GEMV for float32 activations, <= 8 rows,
on tile-major bf16 weights (the wide linears of a float32-KV decode step) -- through mi_op_gemv_f32 (include/mi355_ops.h),
against the oracle's matmul in float64 and against skinny_kernel<.., X32> (gemm_skinny.hip) on the same call.

Criterion: the project's float32 one (test_gpu_kernels._assert_close: rtol 2e-5, atol 2e-5 x rms; scale 4.0 for the
residual form).  Shapes are stated in tiles per compute unit, since a workgroup (one per CU) walks its tiles in passes of
at most 8: fewer than 8, exactly 8, several passes (rolling from one full pass into the next), a last pass of one tile,
every pass size 1..8 (each has its own prefetch depth), K shorter than a chunk, one chunk, and not a multiple of 1024."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_model
from oracle.numerics import matmul_nt, round_to

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, gemm_skinny, gemv_args, host, op_linear, to_tiled  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402

RNG = np.random.default_rng(9051)
EPS = 1e-5
SENTINEL = 7.0


def _cus() -> int:
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _weight(N, K):
    w = round_to(RNG.standard_normal((N, K)).astype(np.float32) * 0.05, "bfloat16")
    wd = dev(w, "bfloat16")
    ol, keep = op_linear("bf16", N, K, wd), [wd]
    assert to_tiled(ol, keep)
    return ol, w, keep


def _oracle_nt(x, w, block=8192):
    """matmul_nt over row blocks of w (the float64 copy of a production-size matrix would not fit comfortably)."""
    return np.concatenate([matmul_nt(x, w[i:i + block]) for i in range(0, w.shape[0], block)], axis=-1)


def _wide_x(M, K):
    """entries spanning 2^-20 .. 2^10: the `mid` and `lo` terms of the three-way split carry weight"""
    return (RNG.standard_normal((M, K)) * np.exp2(RNG.uniform(-20.0, 10.0, (M, K)))).astype(np.float32)


def gemv_f32(ol, x, M, *, epi=0, out=None, ldo=0, resid=None, pair_offset=0, norm_w=None, eps=0.0, iters=0):
    a = gemv_args(x, M, "float32", pro=1 if norm_w is not None else 0, norm_w=norm_w, eps=eps, epi=epi, out=out, ldo=ldo,
                  resid=resid, pair_offset=pair_offset)
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    L.check(L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), int(iters), C.byref(ms)))
    return ms.value if iters >= 1 else None


def _guarded(M, N):
    """an output buffer with one spare row and 16 spare columns, all SENTINEL"""
    return torch.full((M + 1, N + 16), SENTINEL, dtype=torch.float32, device="cuda")


def _check_guard(got, M, N):
    assert np.all(got[M:] == SENTINEL), "rows beyond M were written"
    assert np.all(got[:, N:] == SENTINEL), "columns beyond N were written"


def _swiglu(g, u):
    with np.errstate(over="ignore"):           # (exp of a large -g overflows to inf: silu -> -0, as it should)
        return (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u


# (M, whole tiles per CU, extra tiles, K)
SHAPES = [
    (1, 0, 5, 64),          # 5 workgroups of one tile, K shorter than a chunk (two k-blocks: six waves idle)
    (3, 3, 0, 1024),        # one pass with fewer tiles than the maximum, K of one chunk
    (8, 8, 0, 1536),        # exactly the maximum, K not a multiple of 1024
    (8, 16, 5, 256),        # 17 / 16 tiles: two full passes (the first rolls into the second), a last pass of one tile
    (3, 2, 3, 5120),        # Qwen3's K: five chunks; passes of 3 and 2 tiles
    (8, 9, 0, 1056),        # a full pass, then a pass of one tile; the last chunk holds one k-block
    (8, 16, 0, 2048),       # two full passes over two chunks: the roll into the next pass happens in a later chunk than the first
    (1, 1, 0, 2048), (3, 2, 0, 1056), (8, 4, 0, 1056), (3, 5, 0, 1056), (8, 6, 0, 1056), (1, 7, 0, 1056),   # every pass size
]


@pytest.mark.parametrize("M,per_cu,extra,K", SHAPES)
def test_epilogues_match_oracle_and_skinny(M, per_cu, extra, K):
    N = 16 * (per_cu * _cus() + extra)
    ol, w, keep = _weight(N, K)
    x = _wide_x(M, K)
    xd = dev(x, "float32")
    want = _oracle_nt(x, w)
    # plain store, twice: guarded buffer untouched outside [M, N], run-to-run bit-identical
    outs = []
    for _ in range(2):
        out = _guarded(M, N)
        gemv_f32(ol, xd, M, epi=L.EPI_STORE, out=out, ldo=N + 16)
        outs.append(host(out))
    assert np.array_equal(outs[0], outs[1])
    _check_guard(outs[0], M, N)
    _assert_close(outs[0][:M, :N], want, "float32")
    # the same call on skinny_kernel<.., X32>: the same float32 criterion between the two kernels
    ref = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    gemm_skinny(ol, xd, M, "float32", epi=L.EPI_STORE, out=ref, ldo=N)
    _assert_close(outs[0][:M, :N], host(ref), "float32")
    # float32 logits
    out = _guarded(M, N)
    gemv_f32(ol, xd, M, epi=L.EPI_STORE_F32, out=out, ldo=N + 16)
    got = host(out)
    _check_guard(got, M, N)
    assert np.array_equal(got, outs[0])                        # the two stores coincide in float32
    # residual add (inputs and scale as in test_float32_activations_on_bf16_weights)
    x1 = RNG.standard_normal((M, K)).astype(np.float32)
    h = RNG.standard_normal((M, N)).astype(np.float32)
    hbuf = _guarded(M, N)
    hbuf[:M, :N] = dev(h, "float32")
    gemv_f32(ol, dev(x1, "float32"), M, epi=L.EPI_RESID, resid=hbuf, ldo=N + 16)
    got = host(hbuf)
    _check_guard(got, M, N)
    _assert_close(got[:M, :N], h + _oracle_nt(x1, w), "float32", scale=4.0)
    # SwiGLU over the fused gate|up matrix (on its row-interleaved copy)
    if N % 32 == 0:
        I = N // 2
        out = _guarded(M, I)
        gemv_f32(ol, xd, M, epi=L.EPI_SWIGLU, out=out, ldo=I + 16, pair_offset=I)
        got = host(out)
        _check_guard(got, M, I)
        _assert_close(got[:M, :I], _swiglu(want[:, :I], want[:, I:]), "float32")


@pytest.mark.parametrize("M,per_cu,extra,K", [(1, 0, 5, 64), (3, 3, 0, 1024), (8, 16, 5, 256), (3, 2, 3, 5120), (8, 7, 0, 1536)])
def test_deferred_rmsnorm(M, per_cu, extra, K):
    """PRO_NORM against the oracle's rms_norm in float32 with a non-trivial norm weight.  In the several-pass case the
    squares of x must be counted once although x is walked once per pass."""
    N = 16 * (per_cu * _cus() + extra)
    ol, w, keep = _weight(N, K)
    x = _wide_x(M, K)
    nw = (1.0 + 0.3 * RNG.standard_normal(K)).astype(np.float32)
    xn = ref_model.rms_norm(x, "float32", nw, "float32", EPS)[0]
    want = _oracle_nt(xn, w)
    xd, nwd = dev(x, "float32"), dev(nw, "float32")
    outs = []
    for _ in range(2):
        out = _guarded(M, N)
        gemv_f32(ol, xd, M, epi=L.EPI_STORE, out=out, ldo=N + 16, norm_w=nwd, eps=EPS)
        outs.append(host(out))
    assert np.array_equal(outs[0], outs[1])
    _check_guard(outs[0], M, N)
    _assert_close(outs[0][:M, :N], want, "float32")
    if N % 32 == 0:
        I = N // 2
        out = _guarded(M, I)
        gemv_f32(ol, xd, M, epi=L.EPI_SWIGLU, out=out, ldo=I + 16, pair_offset=I, norm_w=nwd, eps=EPS)
        got = host(out)
        _check_guard(got, M, I)
        _assert_close(got[:M, :I], _swiglu(want[:, :I], want[:, I:]), "float32")


@pytest.mark.parametrize("M,per_cu,extra,K", [(8, 0, 5, 64), (8, 3, 0, 2048), (3, 8, 0, 1056)])
def test_lo_term_is_pinned(M, per_cu, extra, K):
    """One non-zero column per row of x (a different k-block and lane group for each row), its value a float32 with all 24
    significant bits in use (1 + 2^-8 + 2^-16 + 2^-23 scaled), so hi, mid and lo are all non-zero.  Every output is then
    hi w + mid w + lo w: three exact products and at most three float32 additions of half an ulp each.  Bound: 4 ulps =
    2^-22 relative to the exact product -- a lost or misplaced `lo` term costs 2^-17, a lost `mid` 2^-9."""
    N = 16 * (per_cu * _cus() + extra)
    ol, w, keep = _weight(N, K)
    x = np.zeros((M, K), np.float32)
    cols = [((5 * m * (K // 64)) % (K // 8)) * 8 + (3 * m) % 8 for m in range(M)]     # distinct 8-wide pieces
    for m, k in enumerate(cols):
        x[m, k] = np.float32((1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23) * 2.0 ** (m - 3)) * (-1.0 if m & 1 else 1.0)
    assert len(set(k // 8 for k in cols)) == M
    want = np.stack([x[m, k].astype(np.float64) * w[:, k].astype(np.float64) for m, k in enumerate(cols)])
    out = _guarded(M, N)
    gemv_f32(ol, dev(x, "float32"), M, epi=L.EPI_STORE, out=out, ldo=N + 16)
    got = host(out)
    _check_guard(got, M, N)
    err = np.abs(got[:M, :N].astype(np.float64) - want)
    bound = 2.0 ** -22 * np.abs(want)
    print("max err / |want| in ulps of 2^-24:", float(np.max(err[want != 0] / np.abs(want[want != 0])) * 2.0 ** 24))
    assert np.all(err <= bound), float(np.max(err / np.maximum(np.abs(want), 1e-300)))


def test_production_gate_up():
    """8 x 4096 -> 2 x 14336, RMSNorm in front, SwiGLU on the interleaved copy: the gate|up launch of the Mistral-7B step."""
    M, K, I = 8, 4096, 14336
    ol, w, keep = _weight(2 * I, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    nw = (1.0 + 0.1 * RNG.standard_normal(K)).astype(np.float32)
    xn = ref_model.rms_norm(x, "float32", nw, "float32", EPS)[0]
    want = _swiglu(_oracle_nt(xn, w[:I]), _oracle_nt(xn, w[I:]))
    xd, nwd = dev(x, "float32"), dev(nw, "float32")
    outs = []
    for _ in range(2):
        out = _guarded(M, I)
        gemv_f32(ol, xd, M, epi=L.EPI_SWIGLU, out=out, ldo=I + 16, pair_offset=I, norm_w=nwd, eps=EPS)
        outs.append(host(out))
    assert np.array_equal(outs[0], outs[1])
    _check_guard(outs[0], M, I)
    _assert_close(outs[0][:M, :I], want, "float32")


def test_production_lm_head():
    """8 x 4096 -> 32000 float32 logits, the final RMSNorm in front: the lm_head launch of the Mistral-7B step."""
    M, K, N = 8, 4096, 32000
    ol, w, keep = _weight(N, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    nw = (1.0 + 0.1 * RNG.standard_normal(K)).astype(np.float32)
    xn = ref_model.rms_norm(x, "float32", nw, "float32", EPS)[0]
    want = _oracle_nt(xn, w)
    xd, nwd = dev(x, "float32"), dev(nw, "float32")
    outs = []
    for _ in range(2):
        out = _guarded(M, N)
        gemv_f32(ol, xd, M, epi=L.EPI_STORE_F32, out=out, ldo=N + 16, norm_w=nwd, eps=EPS)
        outs.append(host(out))
    assert np.array_equal(outs[0], outs[1])
    _check_guard(outs[0], M, N)
    _assert_close(outs[0][:M, :N], want, "float32")
    ref = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    gemm_skinny(ol, xd, M, "float32", epi=L.EPI_STORE_F32, out=ref, ldo=N, norm_w=nwd, eps=EPS)
    _assert_close(outs[0][:M, :N], host(ref), "float32")


def test_calls_outside_the_kernel_are_refused():
    """No quiet fall-back: 9 rows, logical rounding and 16-bit activations are errors of this entry point."""
    ol, w, keep = _weight(64, 64)
    xd = dev(RNG.standard_normal((9, 64)).astype(np.float32), "float32")
    out = torch.zeros((9, 64), dtype=torch.float32, device="cuda")
    ms = C.c_float(0.0)
    a = gemv_args(xd, 9, "float32", epi=L.EPI_STORE, out=out, ldo=64)
    assert L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), 0, C.byref(ms)) != 0
    a = gemv_args(xd, 8, "float32", epi=L.EPI_STORE, out=out, ldo=64)
    a.rnd = 1
    assert L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), 0, C.byref(ms)) != 0
    xb = dev(RNG.standard_normal((8, 64)).astype(np.float32), "bfloat16")
    a = gemv_args(xb, 8, "bfloat16", epi=L.EPI_STORE, out=out, ldo=64)
    assert L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), 0, C.byref(ms)) != 0
