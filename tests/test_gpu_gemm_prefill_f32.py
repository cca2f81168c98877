"""Kernel-level parity (-m gpu) of gemm_prefill.hip on FLOAT32 activations -- the prefill of the PagedKVCache mode (base.py:
111-112 promotes every activation behind layer 0 to float32; the linears are llama.py:64-67,93,143,160-165) -- through
mi_op_split_rows and mi_op_gemm_prefill_f32 (include/mi355_ops.h).

The split is compared bit for bit with NumPy.  The GEMM is compared with a float64 product, on the CPU, of the operands the
kernel is documented to multiply, under two bounds:
  gross  _assert_close(.., "float32") (rtol 2e-5, atol 2e-5 x rms): a lost `mid` term of x or `lo` half of W, a wrong pairing
         in the six-pass walk, wrong rows or columns -- all 1e-3 of the rms or more;
  fine   (true K <= 512, no norm, dense bf16 in three terms and f16) E <= D / 3, where E = rms(got - want) over the sampled
         elements and D = rms((hi + mid) . w - x . w), the distance of a kernel that lost x's `lo` term (2.4e-6 of the rms),
         computed here in float64 from the same inputs.  Basis (CPU model, x = normal x exp(normal), w = 0.05 normal in
         bf16): the split is exact, and a float32 accumulator fed the exact products eight at a time -- coarser than the
         MFMA's 32 -- gives E / D = 0.14 at K = 512 (0.21 at 1536, 0.33 at 4096: hence K <= 512).  The residual epilogue adds
         the rounding of h + y in float32 (half an ulp of |h| ~ 3: 1e-7, 1.5 % of D); the SwiGLU epilogue is held to the
         same fraction with D taken through silu(g) * u in float64 -- its float32 evaluation (expf, one division, two
         products: about an ulp of each element) is a few per cent of D.  E / D is printed per case; measured values:
         DESIGN.md section 8d and profiles/gemm_prefill_f32_parity.md.
Which kernel a shape lands on is annotated next to it, read from launch_gemm_prefill's choice (256 CUs).

Not tested: the (lo, lo) pair of the 3 : 2 walk over [hi | lo] weights contributes about 2^-26 of the result and cannot be
told from accumulation noise."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_quant
from oracle.numerics import bf16_bits_to_f32, f32_to_bf16_bits, round_to, split2

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_u32, gemm_prefill, gemm_prefill_f32, op_linear, split_rows, to_tiled  # noqa: E402
from test_gpu_kernels import _assert_close  # noqa: E402

RNG = np.random.default_rng(4242)
SENT = 7.0
PAD = 8          # sentinel columns past N (ldo = N + PAD) and sentinel rows past M


def _x(M, K):
    """float32 normals times exp(normal), both signs, with a few exact zeros, a few values whose low 16 mantissa bits are zero
    (mid = lo = 0) and a few whose low 8 are (lo = 0)"""
    x = (RNG.standard_normal((M, K)) * np.exp(RNG.standard_normal((M, K)))).astype(np.float32)
    flat = x.reshape(-1)
    n = max(4, flat.size // 97)
    idx = RNG.choice(flat.size, 3 * n, replace=False)
    flat[idx[:n]] = 0.0
    flat[idx[n:2 * n]] = (flat[idx[n:2 * n]].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    flat[idx[2 * n:]] = (flat[idx[2 * n:]].view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)
    return x


def _split_np(x):
    """hi = T(x), mid = T(x - hi), lo = T(x - hi - mid) in float32 arithmetic (every difference is exact)"""
    hi = round_to(x, "bfloat16")
    r1 = (x - hi).astype(np.float32)
    mid = round_to(r1, "bfloat16")
    lo = round_to((r1 - mid).astype(np.float32), "bfloat16")
    return hi, mid, lo


def _xdev(x, pad=4):
    """x on the device with a row stride of K + pad floats (NaN in the padding: nothing may read it)"""
    M, K = x.shape
    buf = np.full((M, K + pad), np.nan, np.float32)
    buf[:, :K] = x
    return torch.from_numpy(buf).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ the split kernel
@pytest.mark.parametrize("terms", [2, 3])
@pytest.mark.parametrize("K", [64, 2112, 68])      # one trip; two 2048-element trips; the K % 8 != 0 branch (4 per thread)
def test_split_rows_is_numpys_split_bit_for_bit(K, terms):
    rows = 5
    x = _x(rows, K)
    xd = _xdev(x)
    tail = 64
    out = torch.full((rows * terms * K + tail,), 0x7B7B, dtype=torch.int16, device="cuda")
    split_rows(xd, rows, K, terms, out, ldx=K + 4)
    o = out.cpu().numpy().view(np.uint16)
    assert np.all(o[rows * terms * K:] == 0x7B7B), "the split wrote behind its last row"
    img = o[:rows * terms * K].reshape(rows, terms, K)          # row stride terms x K: [hi | mid (| lo)]
    hi, mid, lo = _split_np(x)
    assert np.array_equal(img[:, 0], f32_to_bf16_bits(hi)), "hi"
    assert np.array_equal(img[:, 1], f32_to_bf16_bits(mid)), "mid"
    if terms == 3:
        assert np.array_equal(img[:, 2], f32_to_bf16_bits(lo)), "lo"
        total = sum(bf16_bits_to_f32(img[:, t]).astype(np.float64) for t in range(3))
        assert np.array_equal(total, x.astype(np.float64)), "hi + mid + lo != x"
    else:
        total = bf16_bits_to_f32(img[:, 0]).astype(np.float64) + bf16_bits_to_f32(img[:, 1]).astype(np.float64)
        assert np.array_equal(total, split2(x, "bfloat16").astype(np.float64))


def test_split_rows_with_the_rmsnorm_in_front():
    rows, K, eps = 5, 2112, 1e-5
    x = _x(rows, K)
    nw = (1.0 + 0.1 * RNG.standard_normal(K)).astype(np.float32)
    out = torch.full((rows * 3 * K + 64,), 0x7B7B, dtype=torch.int16, device="cuda")
    split_rows(_xdev(x), rows, K, 3, out, norm_w=torch.from_numpy(nw).cuda(), eps=eps, ldx=K + 4)
    o = out.cpu().numpy().view(np.uint16)
    assert np.all(o[rows * 3 * K:] == 0x7B7B)
    img = o[:rows * 3 * K].reshape(rows, 3, K)
    total = sum(bf16_bits_to_f32(img[:, t]).astype(np.float64) for t in range(3))
    got = total.astype(np.float32)
    assert np.array_equal(got.astype(np.float64), total), "the three terms do not sum to a float32"
    x64 = x.astype(np.float64)
    want = x64 / np.sqrt(np.mean(x64 * x64, axis=1, keepdims=True) + eps) * nw.astype(np.float64)
    _assert_close(got, want.astype(np.float32), "float32")


# ------------------------------------------------------------------------------------------------ the GEMM
def _rows(M, bm):
    """the first rows, the ragged last row block (of bm rows) whole, and a few from the middle"""
    pick = set(range(min(M, 16))) | set(range(max(0, (M - 1) // bm * bm), M)) | set(RNG.integers(0, M, 12).tolist())
    return np.array(sorted(pick))


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def _weight(kind, N, K):
    """-> (tile-major op_linear, [float64 terms the kernel multiplies: W, or (hi, lo) of an int4 matrix], keepalive)"""
    if kind == "q4_bf16":
        w = round_to(RNG.standard_normal((N, K)).astype(np.float32) * 0.05, "bfloat16")
        packed, scales, biases = ref_quant.quantize(w, 64, 4, "bfloat16")
        w32 = ref_quant.dequantize(packed, scales, biases, 64, 4)       # float32, two roundings (mul_add_unfused)
        hi = round_to(w32, "bfloat16")
        lo = round_to((w32 - hi).astype(np.float32), "bfloat16")
        pd, sd, bd = dev_u32(packed), dev(scales, "bfloat16"), dev(biases, "bfloat16")
        ol, keep = op_linear(kind, N, K, pd, sd, bd), [pd, sd, bd]
        assert to_tiled(ol, keep)
        return ol, (hi.astype(np.float64), lo.astype(np.float64)), keep
    dt = {"bf16": "bfloat16", "f16": "float16"}[kind]
    w = RNG.standard_normal((N, K)).astype(np.float32) * 0.05
    if kind == "f16":                                   # a few f16 subnormals (multiples of 2^-24 below 2^-14)
        flat = w.reshape(-1)
        idx = RNG.choice(flat.size, 64, replace=False)
        flat[idx] = RNG.integers(-1023, 1024, 64).astype(np.float32) * np.float32(2.0 ** -24)
    w = round_to(w, dt)
    wd = dev(w, dt)
    ol, keep = op_linear(kind, N, K, wd), [wd]
    assert to_tiled(ol, keep)
    return ol, (w.astype(np.float64),), keep


def _env(name, value):
    class _Set:
        def __enter__(self):
            self.old = os.environ.get(name)
            os.environ[name] = str(value)

        def __exit__(self, *exc):
            if self.old is None:
                del os.environ[name]
            else:
                os.environ[name] = self.old
    return _Set()


def _norm64(x, nw, eps):
    x64 = x.astype(np.float64)
    return x64 / np.sqrt(np.mean(x64 * x64, axis=1, keepdims=True) + eps) * nw.astype(np.float64)


def _run_plain(ol, xd, M, N, terms, epi, h0, dma, norm_w=None, eps=0.0):
    """one launch into a sentinel-framed float32 buffer -> the M x N result (the frame is checked here)"""
    buf = torch.full((M + PAD, N + PAD), SENT, dtype=torch.float32, device="cuda")
    if epi == L.EPI_RESID:
        buf[:M, :N] = torch.from_numpy(h0).cuda()
    with _env("MI_GEMM_DMA", int(dma)):
        gemm_prefill_f32(ol, xd, M, x_terms=terms, epi=epi, out=buf, resid=buf if epi == L.EPI_RESID else None, ldo=N + PAD,
                         norm_w=norm_w, eps=eps, ldx=xd.shape[1])
        torch.cuda.synchronize()
    o = buf.cpu().numpy()
    assert np.all(o[M:] == SENT), "rows past M were written"
    assert np.all(o[:, N:] == SENT), "columns past N were written"
    return o[:M, :N]


def _report(tag, E, D):
    print(f"E/D {tag}: E = {E:.3e}  D = {D:.3e}  E/D = {E / D:.3f}")


# (kind, M, N, true K, rows per block, MI_GEMM_DMA=0 must equal the default bit for bit)
PLAIN = [
    # grid 1 x 2 of the 128 x 128 tile: one ragged row block, N ragged against 128 (208 = 128 + 80); 3 terms = 12 K tiles, 2 terms =
    # 8: below the 16 a K split needs
    ("bf16", 40, 208, 256, 128, False),
    # 128 x 128 tile, 2 x 2 blocks, ragged second row block; 3 terms = 33 K tiles in 4 slices of 8 / 8 / 8 / 9 cutting terms of 11
    # tiles; 2 terms = 22 tiles in 2 slices of 11.  True K > 512: E / D is printed, not asserted
    ("bf16", 150, 208, 704, 128, False),
    # 2 x 2 blocks of the LDS-DMA 256 tile, the second of each ragged (44 rows, 208 columns); 3 terms = 24 K tiles in 3 slices, 2
    # terms = 16 in 2; float32 reduce (N % 4 == 0).  MI_GEMM_DMA=0: no 256-row split, the 128 x 128 tile (3 x 4 blocks) with the
    # same 3 / 2 slices [z nk / ks, (z + 1) nk / ks) -- every accumulator runs the same MFMA chain in K order and the reduce
    # adds the slices in order, so the two are bit-equal as well
    ("bf16", 300, 464, 512, 256, True),
    # 9 x 23 = 207 blocks (>= 192) of the 256 tile, unsplit (6 / 4 K tiles: below 8 per slice); last column block 16 wide, last
    # row block 37 rows; 2 terms = 4 K tiles; LDS-DMA tile by default, register-staged with MI_GEMM_DMA=0
    ("bf16", 2085, 5648, 128, 256, True),
    # pair walk, int4: ka = 3 K, kw = 2 K, 48 K tiles; 128 x 128 tile in 6 slices of 8
    ("q4_bf16", 150, 208, 512, 128, False),
    # ... and the LDS-DMA 256 tile in 6 slices of 8 (MI_GEMM_DMA=0: 128 x 128 tile, the same 6 slices: bit-equal)
    ("q4_bf16", 300, 464, 512, 256, True),
    # pair walk over the [hi | lo] bf16 copy of an f16 matrix (with f16 subnormals): as the first int4 shape
    ("f16", 150, 208, 512, 128, False),
]
NORM = {("bf16", 40), ("bf16", 300), ("bf16", 2085)}       # shapes that run once more with MI_PRO_NORM (3 terms, plain store)


def _plain_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}"


_CACHE = {}


def _plain_case(i):
    """operands and float64 references of one shape, computed once and shared by its tests (never modified)"""
    if ("plain", i) in _CACHE:
        return _CACHE["plain", i]
    kind, M, N, K, bm, both256 = PLAIN[i]
    ol, wt, keep = _weight(kind, N, K)
    x = _x(M, K)
    h0 = RNG.standard_normal((M, N)).astype(np.float32)
    rows = _rows(M, bm)
    xs = x[rows].astype(np.float64)
    hi, mid, lo = _split_np(x[rows])
    x2 = hi.astype(np.float64) + mid.astype(np.float64)
    w = sum(wt)                                                # what the kernel multiplies: W, or hi + lo of the int4 matrix
    ref = {"y3": xs @ w.T, "y2": x2 @ w.T}
    if kind == "q4_bf16":
        ref["y_hi"] = xs @ wt[0].T
    c = dict(kind=kind, M=M, N=N, K=K, both256=both256, ol=ol, keep=keep, x=x, xd=_xdev(x), h0=h0, rows=rows, ref=ref, w64=w,
             D=_rms(ref["y2"] - ref["y3"]), id=_plain_id(PLAIN[i]))
    _CACHE["plain", i] = c
    return c


# every plain route with both epilogues; dense bf16 with two and with three terms
PLAIN_RUNS = [(i, terms, epi) for i, c in enumerate(PLAIN) for terms in ((3, 2) if c[0] == "bf16" else (3,))
              for epi in (L.EPI_STORE, L.EPI_RESID)]


@pytest.mark.parametrize("i,terms,epi", PLAIN_RUNS,
                         ids=[f"{_plain_id(PLAIN[i])}-{t}terms-{'resid' if e == L.EPI_RESID else 'store'}" for i, t, e in PLAIN_RUNS])
def test_plain_and_residual_epilogues(i, terms, epi):
    c = _plain_case(i)
    M, N, rows, ref, D = c["M"], c["N"], c["rows"], c["ref"], c["D"]
    base = c["h0"][rows].astype(np.float64) if epi == L.EPI_RESID else 0.0
    want = base + ref["y3" if terms == 3 else "y2"]
    got = {dma: _run_plain(c["ol"], c["xd"], M, N, terms, epi, c["h0"], dma) for dma in (1, 0)}
    tag = f"{c['id']} terms={terms} {'resid' if epi == L.EPI_RESID else 'store'}"
    for dma in (1, 0):
        g = got[dma][rows].astype(np.float64)
        E = _rms(g - want)
        _report(f"{tag} MI_GEMM_DMA={dma}", E, D)
        _assert_close(got[dma][rows], want.astype(np.float32), "float32")
        if c["kind"] == "q4_bf16":
            assert E < _rms(g - (base + ref["y_hi"])) / 100, "the lo half of W was not multiplied"
        elif terms == 2:
            assert E <= D / 3, (E, D)
            assert E < _rms(g - (base + ref["y3"])), "two terms: no closer to the two-term product than to x . w"
        elif c["K"] <= 512:
            assert E <= D / 3, (E, D)
    if c["both256"]:
        assert np.array_equal(got[1], got[0]), "MI_GEMM_DMA=0 differs from the LDS-DMA tile"


# one shape per tile family once more with MI_PRO_NORM (three terms, plain store): 128 x 128 unsplit, LDS-DMA 256 with K split
# (MI_GEMM_DMA=0: the 128 x 128 tile with K split), 256 x 256 unsplit on both tiles
@pytest.mark.parametrize("i", [0, 2, 3], ids=[_plain_id(PLAIN[i]) for i in (0, 2, 3)])
def test_rmsnorm_in_front(i):
    """The reference normalises in float64; the kernel's float32 norm is within an ulp or two per element of it
    (test_split_rows_with_the_rmsnorm_in_front), far inside the gross bound -- the fine bound does not apply."""
    c = _plain_case(i)
    M, N, K, rows, eps = c["M"], c["N"], c["K"], c["rows"], 1e-5
    nw = (1.0 + 0.1 * np.random.default_rng(K + M).standard_normal(K)).astype(np.float32)
    nwd = torch.from_numpy(nw).cuda()
    want = _norm64(c["x"][rows], nw, eps) @ c["w64"].T
    got = {dma: _run_plain(c["ol"], c["xd"], M, N, 3, L.EPI_STORE, None, dma, norm_w=nwd, eps=eps) for dma in (1, 0)}
    for dma in (1, 0):
        _assert_close(got[dma][rows], want.astype(np.float32), "float32")
    if c["both256"]:
        assert np.array_equal(got[1], got[0])


def _swiglu64(y, I):
    g, u = y[:, :I], y[:, I:]
    return g / (1.0 + np.exp(-g)) * u


SWIGLU = [
    # 128 x 128 tile, 1 x 2 blocks of 64 gate columns + their up columns, I ragged against 64 (80 = 64 + 16): epi32_swiglu
    (40, 80, 256, 128, False),
    # 256 tile, 9 x 23 = 207 blocks of 128 gate columns, the last 16 wide; last row block 37 rows; 6 / 4 K tiles; LDS-DMA tile
    # by default, register-staged with MI_GEMM_DMA=0
    (2085, 2832, 128, 256, True),
]
SWIGLU_RUNS = [(i, terms) for i in range(len(SWIGLU)) for terms in (3, 2)]


def _swiglu_case(i):
    if ("swiglu", i) in _CACHE:
        return _CACHE["swiglu", i]
    M, I, K, bm, both256 = SWIGLU[i]
    ol, (w,), keep = _weight("bf16", 2 * I, K)
    x = _x(M, K)
    rows = _rows(M, bm)
    hi, mid, lo = _split_np(x[rows])
    y3 = _swiglu64(x[rows].astype(np.float64) @ w.T, I)
    y2 = _swiglu64((hi.astype(np.float64) + mid.astype(np.float64)) @ w.T, I)
    c = dict(M=M, I=I, K=K, both256=both256, ol=ol, keep=keep, xd=_xdev(x), rows=rows, y3=y3, y2=y2, D=_rms(y2 - y3))
    _CACHE["swiglu", i] = c
    return c


@pytest.mark.parametrize("i,terms", SWIGLU_RUNS, ids=[f"{SWIGLU[i][0]}x{SWIGLU[i][1]}x{SWIGLU[i][2]}-{t}terms" for i, t in SWIGLU_RUNS])
def test_swiglu_epilogue(i, terms):
    c = _swiglu_case(i)
    M, I, rows, D = c["M"], c["I"], c["rows"], c["D"]
    want = c["y3"] if terms == 3 else c["y2"]
    got = {}
    for dma in (1, 0):
        buf = torch.full((M + PAD, I + PAD), SENT, dtype=torch.float32, device="cuda")
        with _env("MI_GEMM_DMA", dma):
            gemm_prefill_f32(c["ol"], c["xd"], M, x_terms=terms, epi=L.EPI_SWIGLU, out=buf, ldo=I + PAD, pair_offset=I,
                             ldx=c["xd"].shape[1])
            torch.cuda.synchronize()
        o = buf.cpu().numpy()
        assert np.all(o[M:] == SENT), "rows past M were written"
        assert np.all(o[:, I:] == SENT), "columns past I were written"
        got[dma] = o[:M, :I]
        g = got[dma][rows].astype(np.float64)
        E = _rms(g - want)
        _report(f"swiglu {M}x{I}x{c['K']} terms={terms} MI_GEMM_DMA={dma}", E, D)
        _assert_close(got[dma][rows], want.astype(np.float32), "float32")
        assert E <= D / 3, (E, D)
        if terms == 2:
            assert E < _rms(g - c["y3"]), "two terms: no closer to the two-term product than to x . w"
    if c["both256"]:
        assert np.array_equal(got[1], got[0]), "MI_GEMM_DMA=0 differs from the LDS-DMA tile"


# ------------------------------------------------------------------------------------------------ what the entries refuse
def test_calls_the_tile_gemm_does_not_take_are_refused():
    """MI_ERR_UNSUPPORTED (-3), never another kernel: the output keeps its sentinel."""
    M, N, K = 40, 208, 256
    x = _x(M, K)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((M, N), SENT, dtype=torch.float32, device="cuda")
    ol, _, keep = _weight("bf16", N, K)
    assert gemm_prefill_f32(ol, xd, 31, out=out, ldo=N, check=False) == -3, "fewer than 32 rows"
    assert gemm_prefill_f32(ol, xd, M, x_terms=4, out=out, ldo=N, check=False) == -3
    wd = dev(np.zeros((N, K), np.float32), "bfloat16")
    assert gemm_prefill_f32(op_linear("bf16", N, K, wd), xd, M, out=out, ldo=N, check=False) == -3, "row-major weights"
    q4, _, keepq = _weight("q4_bf16", N, K)
    assert gemm_prefill_f32(q4, xd, M, x_terms=2, out=out, ldo=N, check=False) == -3, "two terms against a [hi | lo] pair"
    # an f16 matrix whose K is no multiple of the K tile: the x terms of the [hi | lo] walk would wrap inside a tile
    f16, _, keeph = _weight("f16", N, 96)
    assert gemm_prefill_f32(f16, xd, M, out=out, ldo=N, ldx=K, check=False) == -3, "f16, K = 96"
    # the 16-bit entry points at this one for float32 rows
    with pytest.raises(NotImplementedError, match="mi_op_gemm_prefill_f32"):
        gemm_prefill(ol, xd, M, "float32", out=out, ldo=N)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENT)
