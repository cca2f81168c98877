"""Kernel-level parity (-m gpu) of the linear bias (mi_op_linear.bias -> LinearW::bias) in the four kernel families that apply
it -- gemv_mfma.hip, gemv_v1.hip, gemm_skinny.hip, gemm_prefill.hip -- against tests/biased_ref.py, through mi_op_gemv,
mi_op_gemm_skinny, mi_op_gemm_prefill and mi_op_gemm_prefill_f32, at the smallest shapes that reach each code path.

Semantics: dense weights y = T(acc + b), quantised weights y = T(T(acc) + b), float32 activations y = acc + b
(after the deferred RMSNorm's row scale), SwiGLU with a bias of its own for gate and up, the bias added once where K slices are
combined.  The bias is drawn at the RMS of the product, rounded to the activation dtype like a checkpoint's tensor.

Bounds as in tests/test_gpu_kernels.py (_assert_close).  That bound alone cannot tell one rounding from two: at this bias size
the two semantics differ in 29 % of the elements but by more than half a unit in only 9 % (CPU measurement), inside the 10 % the
bound allows.  So the dense bf16 and the int4 STORE cases also count the elements that are BIT-EQUAL to the oracle: the share
with the bias must not be lower than the same launch's share without one, minus 0.05 (the wrong semantics loses ~0.29)."""
import numpy as np
import pytest
import torch

from oracle import numerics, ref_model, ref_quant
from oracle.numerics import matmul_nt, round_to

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from biased_ref import biased  # noqa: E402
from gpu_helpers import (dev, dev_u32, gemm_prefill, gemm_prefill_f32, gemm_skinny, gemv, host, op_linear,  # noqa: E402
                         to_tiled)
from test_gpu_kernels import _assert_close  # noqa: E402

RNG = np.random.default_rng(20240607)
DT = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}


def _weight(kind, N, K, tiled=True):
    """-> (op_linear, the dense float32 matrix the oracle multiplies with, quantised?, keepalive)"""
    if kind in DT:
        w = round_to(RNG.standard_normal((N, K)).astype(np.float32) * 0.05, DT[kind])
        wd = dev(w, DT[kind])
        ol, keep = op_linear(kind, N, K, wd), [wd]
        if tiled:
            to_tiled(ol, keep)
        return ol, w, False, keep
    bits = 4 if kind.startswith("q4") else 8
    sdt = DT[kind.split("_")[1]]
    w = RNG.standard_normal((N, K)).astype(np.float32) * 0.05
    packed, scales, biases = ref_quant.quantize(round_to(w, sdt), 64, bits, sdt)
    pd, sd, bd = dev_u32(packed), dev(scales, sdt), dev(biases, sdt)
    ol, keep = op_linear(kind, N, K, pd, sd, bd), [pd, sd, bd]
    if tiled:
        to_tiled(ol, keep)
    return ol, ref_quant.dequantize(packed, scales, biases, 64, bits), True, keep


def _bias(ol, N, acc, act, keep):
    """a bias at the RMS of the product, a checkpoint's values (rounded to the model dtype), attached to the op_linear"""
    rms = float(np.sqrt(np.mean(np.square(acc)))) + 1e-12
    b = round_to(RNG.standard_normal(N).astype(np.float32) * np.float32(rms), "bfloat16" if act == "float32" else act)
    bd = torch.from_numpy(b).cuda().contiguous()
    keep.append(bd)
    ol.bias = bd.data_ptr()
    return b


def _share_check(tag, got_b, want_b, got_nb, want_nb):
    sb, snb = float(np.mean(got_b == want_b)), float(np.mean(got_nb == want_nb))
    print(f"bit-equal share {tag}: with bias {sb:.4f}, without {snb:.4f}")
    assert sb >= snb - 0.05, (tag, sb, snb)


def _swiglu(g, u, act):
    sig = round_to(1.0 / (1.0 + np.exp(-g.astype(np.float64))), act)
    return round_to(round_to(g * sig, act) * u, act)


# ------------------------------------------------------------------------------------------------ mi_op_gemv
GEMV_KINDS = [("bf16", "bfloat16"), ("f16", "float16"), ("q4_bf16", "bfloat16"), ("q8_f16", "float16"), ("f32", "float32"),
              ("bf16", "float32")]
MFMA = {("bf16", "bfloat16"), ("f16", "float16"), ("q4_bf16", "bfloat16")}      # gemv_mfma.hip takes them (up to 16 rows)
# the generic kernel (and every kind without a matrix-core GEMV) serves at most 8 rows per launch: 16 rows exist on the
# matrix-core path alone
GEMV_CASES = [(k, a, M, fg) for (k, a) in GEMV_KINDS for M in (1, 8, 16) for fg in (0, 1)
              if M <= 8 or ((k, a) in MFMA and fg == 0)]


@pytest.mark.parametrize("kind,act,M,force_generic", GEMV_CASES)
def test_gemv_store(kind, act, M, force_generic):
    N, K = 80, 256
    ol, w, quant, keep = _weight(kind, N, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    xd = dev(x, act)
    out_nb = torch.zeros((M, N), dtype=xd.dtype, device="cuda")
    used = gemv(ol, xd, M, act, epi=L.EPI_STORE, out=out_nb, ldo=N, force_generic=force_generic)
    assert used == ((kind, act) in MFMA and not force_generic)
    b = _bias(ol, N, acc, act, keep)
    out = torch.zeros((M, N), dtype=xd.dtype, device="cuda")
    gemv(ol, xd, M, act, epi=L.EPI_STORE, out=out, ldo=N, force_generic=force_generic)
    want = biased(acc, b, act, quant)
    _assert_close(host(out), want, act)
    assert np.abs(want - round_to(acc, act)).max() > 0.25 * np.abs(acc).max()       # the bias matters
    if (kind, act) in (("bf16", "bfloat16"), ("q4_bf16", "bfloat16")) and M >= 8:
        _share_check(f"gemv {kind} M={M} generic={force_generic}", host(out), want, host(out_nb), round_to(acc, act))
    # float32 logits store (no model has a biased lm_head; the epilogue shares the value with the plain store)
    out32 = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    gemv(ol, xd, M, act, epi=L.EPI_STORE_F32, out=out32, ldo=N, force_generic=force_generic)
    _assert_close(host(out32), want, act)


@pytest.mark.parametrize("kind,act,M,force_generic", [c for c in GEMV_CASES if c[2] != 1])
def test_gemv_resid_and_swiglu(kind, act, M, force_generic):
    # residual: h = T(h + y), y biased; K = 4608 spans several activation chunks
    N, K = 64, 4608
    ol, w, quant, keep = _weight(kind, N, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32) * 0.5, act)
    h = round_to(RNG.standard_normal((M, N)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    b = _bias(ol, N, acc, act, keep)
    want = round_to(h + biased(acc, b, act, quant), act)
    xd, hd = dev(x, act), dev(h, act)
    gemv(ol, xd, M, act, epi=L.EPI_RESID, resid=hd, ldo=N, force_generic=force_generic)
    _assert_close(host(hd), want, act, scale=4.0)
    # SwiGLU: gate and up each get their own bias in front of silu(g) * u
    I, K = 48, 256
    ol, w, quant, keep = _weight(kind, 2 * I, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    b = _bias(ol, 2 * I, acc, act, keep)
    assert not np.array_equal(b[:I], b[I:])
    want = _swiglu(biased(acc[:, :I], b[:I], act, quant), biased(acc[:, I:], b[I:], act, quant), act)
    xd = dev(x, act)
    out = torch.zeros((M, I), dtype=xd.dtype, device="cuda")
    gemv(ol, xd, M, act, epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I, force_generic=force_generic)
    _assert_close(host(out), want, act)


# ------------------------------------------------------------------------------------------------ mi_op_gemm_skinny
@pytest.mark.parametrize("kind", ["bf16", "q4_bf16", "q8_bf16"])
@pytest.mark.parametrize("M,N,K,ksplit", [(9, 80, 128, 1), (13, 144, 384, 3), (27, 256, 1024, 2)])
def test_skinny_store_and_resid(kind, M, N, K, ksplit):
    """the unsplit path (ksplit 1) and the last arriver's combine (ksplit >= 2: the bias lands once, deterministically)"""
    act = "bfloat16"
    ol, w, quant, keep = _weight(kind, N, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    xd = dev(x, act)
    out_nb = torch.zeros((M, N), dtype=xd.dtype, device="cuda")
    gemm_skinny(ol, xd, M, act, epi=L.EPI_STORE, out=out_nb, ldo=N, ksplit=ksplit)
    b = _bias(ol, N, acc, act, keep)
    want = biased(acc, b, act, quant)
    outs = []
    for _ in range(2):
        out = torch.full((M + 2, N), 7.0, dtype=xd.dtype, device="cuda")
        gemm_skinny(ol, xd, M, act, epi=L.EPI_STORE, out=out, ldo=N, ksplit=ksplit)
        outs.append(host(out))
    assert np.array_equal(outs[0], outs[1])
    assert np.all(outs[0][M:] == 7.0)
    _assert_close(outs[0][:M], want, act)
    if kind in ("bf16", "q4_bf16"):
        _share_check(f"skinny {kind} {M}x{N}x{K}/{ksplit}", outs[0][:M], want, host(out_nb), round_to(acc, act))
    h = round_to(RNG.standard_normal((M, N)).astype(np.float32), act)
    hd = dev(h, act)
    gemm_skinny(ol, xd, M, act, epi=L.EPI_RESID, resid=hd, ldo=N, ksplit=ksplit)
    _assert_close(host(hd), round_to(h + want, act), act, scale=4.0)
    out32 = torch.zeros((M, N), dtype=torch.float32, device="cuda")      # the float32 store shares the value with the plain one
    gemm_skinny(ol, xd, M, act, epi=L.EPI_STORE_F32, out=out32, ldo=N, ksplit=ksplit)
    assert np.array_equal(host(out32), outs[0][:M])


@pytest.mark.parametrize("kind", ["bf16", "q4_bf16", "q8_bf16"])
def test_skinny_swiglu_72_rows(kind):
    act, M, I, K = "bfloat16", 72, 176, 768
    ol, w, quant, keep = _weight(kind, 2 * I, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    b = _bias(ol, 2 * I, acc, act, keep)
    want = _swiglu(biased(acc[:, :I], b[:I], act, quant), biased(acc[:, I:], b[I:], act, quant), act)
    xd = dev(x, act)
    for ks in (1, 3):
        out = torch.zeros((M, I), dtype=xd.dtype, device="cuda")
        gemm_skinny(ol, xd, M, act, epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I, ksplit=ks)
        _assert_close(host(out), want, act)


@pytest.mark.parametrize("M,N,K,ksplit,norm", [(1, 80, 128, 1, False), (8, 256, 4608, 0, True)])
def test_skinny_float32_activations(M, N, K, ksplit, norm):
    """PagedKVCache mode after layer 0 on bf16 weights: b is added in float32; with the RMSNorm deferred to the epilogue the
    row scale multiplies the accumulator first, y = rs * acc + b.  The K-split case twice: bit-identical."""
    ol, w, quant, keep = _weight("bf16", N, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    nw = (1.0 + 0.1 * RNG.standard_normal(K)).astype(np.float32)
    xn = ref_model.rms_norm(x, "float32", nw, "float32", 1e-5)[0] if norm else x
    acc = matmul_nt(xn, w)
    b = _bias(ol, N, acc, "float32", keep)
    want = biased(acc, b, "float32", quant)
    xd = torch.from_numpy(x).cuda()
    nwd = torch.from_numpy(nw).cuda() if norm else None
    h = RNG.standard_normal((M, N)).astype(np.float32)
    for ks in [ksplit] + ([4] if K > 256 else []):       # (the cost model's split, and four K slices whatever it chose)
        outs, h_outs = [], []
        for _ in range(2):
            out = torch.zeros((M, N), dtype=torch.float32, device="cuda")
            gemm_skinny(ol, xd, M, "float32", epi=L.EPI_STORE, out=out, ldo=N, ksplit=ks, norm_w=nwd, eps=1e-5)
            outs.append(host(out))
            hd = torch.from_numpy(h).cuda()
            gemm_skinny(ol, xd, M, "float32", epi=L.EPI_RESID, resid=hd, ldo=N, ksplit=ks, norm_w=nwd, eps=1e-5)
            h_outs.append(host(hd))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(h_outs[0], h_outs[1])
        _assert_close(outs[0], want, "float32")
        _assert_close(h_outs[0], h + want, "float32")
    assert np.abs(want - acc).max() > 0.25 * np.abs(acc).max()


def test_skinny_float32_activations_swiglu_and_quantised():
    M, I, K = 8, 48, 512
    for kind in ("bf16", "q4_bf16"):
        ol, w, quant, keep = _weight(kind, 2 * I, K)
        x = RNG.standard_normal((M, K)).astype(np.float32)
        acc = matmul_nt(x, w)
        b = _bias(ol, 2 * I, acc, "float32", keep)
        want = _swiglu(biased(acc[:, :I], b[:I], "float32", quant), biased(acc[:, I:], b[I:], "float32", quant), "float32")
        out = torch.zeros((M, I), dtype=torch.float32, device="cuda")
        gemm_skinny(ol, torch.from_numpy(x).cuda(), M, "float32", epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I, ksplit=2)
        _assert_close(host(out), want, "float32")


# ------------------------------------------------------------------------------------------------ mi_op_gemm_prefill
PREFILL = [
    ("bf16", 33, 208, 64),          # the 128 x 128 tile
    ("f16", 33, 208, 64),
    ("bf16", 200, 208, 1024),       # its K split + splitk_epilogue_kernel
    ("bf16", 2085, 5648, 64),       # the register-staged 256 x 256 tile (one K tile: no LDS-DMA)
    ("bf16", 2048, 6400, 128),      # the LDS-DMA 256 x 256 tile
    ("bf16", 300, 2048, 2048),      # its K split + the reduce
    ("q4_bf16", 150, 208, 512),     # through the [hi | lo] copy: two roundings
]


@pytest.mark.parametrize("kind,M,N,K", PREFILL)
def test_prefill_store_and_resid(kind, M, N, K):
    act = DT[kind.split("_")[-1]]
    ol, w, quant, keep = _weight(kind, N, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    xd = dev(x, act)
    out_nb = torch.zeros((M, N), dtype=xd.dtype, device="cuda")
    gemm_prefill(ol, xd, M, act, epi=L.EPI_STORE, out=out_nb, ldo=N)
    b = _bias(ol, N, acc, act, keep)
    want = biased(acc, b, act, quant)
    out = torch.full((M + 2, N), 7.0, dtype=xd.dtype, device="cuda")
    gemm_prefill(ol, xd, M, act, epi=L.EPI_STORE, out=out, ldo=N)
    got = host(out)
    assert np.all(got[M:] == 7.0)
    _assert_close(got[:M], want, act)
    if kind in ("bf16", "q4_bf16"):
        _share_check(f"prefill {kind} {M}x{N}x{K}", got[:M], want, host(out_nb), round_to(acc, act))
    h = round_to(RNG.standard_normal((M, N)).astype(np.float32), act)
    hd = dev(h, act)
    gemm_prefill(ol, xd, M, act, epi=L.EPI_RESID, resid=hd, ldo=N)
    _assert_close(host(hd), round_to(h + want, act), act, scale=4.0)


@pytest.mark.parametrize("M,I,K", [(2048, 3200, 256), (40, 48, 128)])      # the 256-row SwiGLU tile; the 128-row one
def test_prefill_swiglu(M, I, K):
    act = "bfloat16"
    ol, w, quant, keep = _weight("bf16", 2 * I, K)
    x = round_to(RNG.standard_normal((M, K)).astype(np.float32), act)
    acc = matmul_nt(x, w)
    b = _bias(ol, 2 * I, acc, act, keep)
    want = _swiglu(biased(acc[:, :I], b[:I], act, quant), biased(acc[:, I:], b[I:], act, quant), act)
    xd = dev(x, act)
    out = torch.zeros((M, I), dtype=xd.dtype, device="cuda")
    gemm_prefill(ol, xd, M, act, epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I)
    _assert_close(host(out), want, act)


# ------------------------------------------------------------------------------------------------ mi_op_gemm_prefill_f32
@pytest.mark.parametrize("kind,M,N,K,terms", [("bf16", 40, 208, 256, 2), ("bf16", 40, 208, 256, 3), ("bf16", 300, 464, 512, 2),
                                              ("bf16", 300, 464, 512, 3), ("q4_bf16", 150, 208, 512, 3)])
def test_prefill_float32_activations(kind, M, N, K, terms):
    """the float32-activation route over the split image: float32 outputs, b added in float32 (one or two roundings coincide)"""
    ol, w, quant, keep = _weight(kind, N, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    xk = numerics.split2(x, "bfloat16") if terms == 2 else x          # two terms: the kernel multiplies hi + mid of x
    acc = matmul_nt(xk, w)
    b = _bias(ol, N, acc, "float32", keep)
    want = biased(acc, b, "float32", quant)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((M + 2, N), 7.0, dtype=torch.float32, device="cuda")
    gemm_prefill_f32(ol, xd, M, x_terms=terms, epi=L.EPI_STORE, out=out, ldo=N)
    got = host(out)
    assert np.all(got[M:] == 7.0)
    _assert_close(got[:M], want, "float32")
    assert np.abs(want - acc).max() > 0.25 * np.abs(acc).max()
    h = RNG.standard_normal((M, N)).astype(np.float32)
    hd = torch.from_numpy(h).cuda()
    gemm_prefill_f32(ol, xd, M, x_terms=terms, epi=L.EPI_RESID, out=hd, resid=hd, ldo=N)
    _assert_close(host(hd), h + want, "float32")


def test_prefill_float32_activations_swiglu():
    M, I, K = 40, 112, 256
    ol, w, quant, keep = _weight("bf16", 2 * I, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    acc = matmul_nt(x, w)
    b = _bias(ol, 2 * I, acc, "float32", keep)
    want = _swiglu(biased(acc[:, :I], b[:I], "float32", quant), biased(acc[:, I:], b[I:], "float32", quant), "float32")
    out = torch.zeros((M, I), dtype=torch.float32, device="cuda")
    gemm_prefill_f32(ol, torch.from_numpy(x).cuda(), M, x_terms=3, epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I)
    _assert_close(host(out), want, "float32")


# ------------------------------------------------------------------------------------------------ the routes that decline
def test_routes_without_a_biased_form_refuse_the_matrix():
    """gemv_f32.hip and a forced gemm_q4.hip plan have no biased epilogue: MI_ERR_UNSUPPORTED, never a launch that drops b"""
    import ctypes as C

    from gpu_helpers import gemv_args, q4_force

    M, N, K = 4, 64, 256
    ol, w, quant, keep = _weight("bf16", N, K)
    x = RNG.standard_normal((M, K)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    a = gemv_args(xd, M, "float32", epi=L.EPI_STORE, out=out, ldo=N)
    torch.cuda.synchronize()
    assert L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), 0, None) == 0
    _bias(ol, N, matmul_nt(x, w), "float32", keep)
    assert L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), 0, None) == -3
    M, N, K = 40, 96, 512
    ol, w, quant, keep = _weight("q4_bf16", N, K)
    x16 = round_to(RNG.standard_normal((M, K)).astype(np.float32), "bfloat16")
    xd = dev(x16, "bfloat16")
    out = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    gemm_skinny(ol, xd, M, "bfloat16", epi=L.EPI_STORE, out=out, ldo=N, ksplit=q4_force(2, 2, 4, 1, 4))
    acc = matmul_nt(x16, w)
    b = _bias(ol, N, acc, "bfloat16", keep)
    with pytest.raises(NotImplementedError):
        gemm_skinny(ol, xd, M, "bfloat16", epi=L.EPI_STORE, out=out, ldo=N, ksplit=q4_force(2, 2, 4, 1, 4))
    # unforced, the call falls through to skinny_kernel's int4 instantiation, which applies the bias
    gemm_skinny(ol, xd, M, "bfloat16", epi=L.EPI_STORE, out=out, ldo=N, ksplit=0)
    _assert_close(host(out), biased(acc, b, "bfloat16", True), "bfloat16")
