"""dora_gain_kernel and the gain-aware lora_up_add_by_row_kernel (csrc/lora_rows.hip) on their own, through mi_op_dora_gain and
mi_op_dora_rows only (-m gpu).

* mi_op_dora_gain against the float64 twin (tests/dora_ref.py) within the bound DERIVED from the kernel's summation order
  (DESIGN.md §5 "DoRA"), in units of u = 2^-24:
      (ceil(K / 256) + 9)   the longest chain of additions behind one sum of squares: a thread's k, the wave sum, the four waves
    + kappa (r + 1)         the rank terms of d = W + sum_j A (s B), one rounding each and one for s B, amplified by the
                            cancellation between W and the low-rank term (dora_ref.condition: an input property, 1 when s = 0);
                            the inputs are chosen so that kappa <= 1.25 (asserted), i.e. the bound is chain + r + 2 and at
                            most a quarter of r more: 13 .. 93 u at the test shapes
    + 2                     the square root and the divide
  (at K = 17408, r = 64, kappa = 1: 144 u).  Run to run, and row-major against tile-major, the bits are equal.
* mi_op_dora_rows' up stage, from the test's own t, equals the NumPy restatement of the rounding chain bit for bit, no element
  excluded.  t and B hold small dyadic values, so z = t B is exact in float32 in any order; the gains come from
  mi_op_dora_gain, with m chosen on the CPU (seed fixed below) so that every exact gain sits within 2^-24 of a bfloat16 grid
  point: near_boundary is false for both 16-bit types at rel = the bound, hence T(g) of the device's gain is T(g) of the twin's.
  With T = float32 without a logical rounding there is no rounding of g to restate, so that leg checks the multiply and its
  place in the chain ONLY: the restatement multiplies by the device's own gain, whose value is held to the float64 twin by the
  bound asserted beside it and by the gain tests above, not by the exact comparison.  Rows without a gain equal mi_op_lora_rows on the same buffers bit for bit.
* the refusals of both entries launch nothing.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dora_ref  # noqa: E402
from gpu_helpers import MIDT, TDT, dev, dev_i32, lora_rows, op_linear, to_tiled  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from oracle.numerics import round_to  # noqa: E402

U = 2.0 ** -24
SEED = 20240611
INVALID, UNSUPPORTED = -1, -3
COLS = L.MI_MAX_ADAPTERS + 1


def gain_bound(K: int, r: int, kappa: float) -> float:
    return (math.ceil(K / 256) + 9 + kappa * (r + 1) + 2) * U


def dora_gain(ol, a, b, m, rank, scale, row0, n, gain, check=True):
    torch.cuda.synchronize()
    rc = L.lib().mi_op_dora_gain(C.byref(ol), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(m.data_ptr()), int(rank),
                                 float(scale), int(row0), int(n), C.c_void_p(gain if isinstance(gain, int) else gain.data_ptr()))
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


# ---------------------------------------------------------------------------------------------------- mi_op_dora_gain
# (name, K, rank, scale, N of the matrix, row0, n, what is special)
GAIN_CASES = [
    ("k64_r1", 64, 1, 2.0, 48, 0, 48, ""),
    ("k64_r7", 64, 7, 1.5, 48, 0, 48, ""),
    ("k160_r64", 160, 64, 0.75, 48, 0, 48, ""),
    ("k160_r7_scale0", 160, 7, 0.0, 48, 0, 48, "s0"),
    ("k64_r64_b0", 64, 64, 3.0, 48, 0, 48, "b0"),
    ("k160_r1_mixed_m", 160, 1, 1.0, 48, 0, 48, "mixed"),
    ("k64_r7_middle_part", 64, 7, 2.0, 96, 24, 40, ""),          # a part in the middle of a fused matrix, ragged last tile
    ("k544_r7_three_per_thread", 544, 7, 1.0, 48, 0, 48, ""),    # a thread adds more than two k
]


def gain_inputs(case, dtype):
    name, K, r, s, N, row0, n, special = case
    rng = np.random.default_rng([SEED, K, r, N, row0])
    w = round_to(rng.standard_normal((N, K)).astype(np.float32) * 0.05, dtype)
    a = (rng.standard_normal((K, r)) * 0.05).astype(np.float32)
    b = (rng.standard_normal((r, n)) * 0.1 / r).astype(np.float32)      # (|s B^T| |A^T| stays a few per cent of |W|: kappa near 1)
    if special == "b0":
        b[:] = 0.0
    m = (0.5 + rng.random(n)).astype(np.float32)
    if special == "mixed":
        m = (m * np.exp2(rng.integers(-20, 20, n))).astype(np.float32) * np.where(rng.random(n) < 0.3, -1, 1).astype(np.float32)
    return w, a, b, m


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("case", GAIN_CASES, ids=[c[0] for c in GAIN_CASES])
def test_gain_within_the_derived_bound_and_bit_stable(case, dtype):
    name, K, r, s, N, row0, n, special = case
    w, a, b, m = gain_inputs(case, dtype)
    want = dora_ref.exact_gain(w[row0:row0 + n], a, b, m, s)
    kappa = dora_ref.condition(w[row0:row0 + n], a, b, s)
    bound = gain_bound(K, r, kappa)
    assert kappa <= 1.25 and bound <= 100 * U          # the inputs do not widen the bound: chain + r + 2, a quarter on top of r at most
    if special in ("s0", "b0"):
        assert kappa == 1.0
        assert np.array_equal(want, m.astype(np.float64) / np.sqrt((w[row0:row0 + n].astype(np.float64) ** 2).sum(axis=1)))
    w_d, a_d, b_d, m_d = dev(w, dtype), dev(a), dev(b), dev(m)
    keep = []
    ol = op_linear("bf16" if dtype == "bfloat16" else "f16", N, K, w_d)
    tiled = op_linear("bf16" if dtype == "bfloat16" else "f16", N, K, w_d)
    assert to_tiled(tiled, keep)
    outs = []
    for lin in (ol, ol, tiled, tiled):
        g = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
        dora_gain(lin, a_d, b_d, m_d, r, s, row0, n, g)
        got = g.cpu().numpy()
        assert np.isnan(got[n:]).all(), "written behind the part"
        outs.append(got[:n].copy())
    for other in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint32), other.view(np.uint32)), "not bit-equal run to run / across layouts"
    rel = np.abs(outs[0].astype(np.float64) - want) / np.abs(want)
    print(f"FRACTION {name} {dtype}: largest relative error / bound = {rel.max() / bound:.4f} (bound {bound / U:.1f} u, kappa {kappa:.3f})")
    assert rel.max() <= bound


def test_gain_refusals_launch_nothing():
    case = GAIN_CASES[1]
    _, K, r, s, N, row0, n, _ = case
    w, a, b, m = gain_inputs(case, "bfloat16")
    w_d, a_d, b_d, m_d = dev(w, "bfloat16"), dev(a), dev(b), dev(m)
    ol = op_linear("bf16", N, K, w_d)
    g = torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda")
    lib = L.lib()
    assert dora_gain(ol, a_d, b_d, m_d, 0, s, row0, n, g, check=False) == INVALID and b"rank" in lib.mi_last_error()
    assert dora_gain(ol, a_d, b_d, m_d, 65, s, row0, n, g, check=False) == INVALID
    assert dora_gain(ol, a_d, b_d, m_d, r, s, row0, n, g.data_ptr() + 2, check=False) == INVALID and b"misaligned" in lib.mi_last_error()
    assert dora_gain(ol, a_d, b_d, m_d, r, s, row0, n, 0, check=False) == INVALID
    assert dora_gain(ol, a_d, b_d, m_d, r, s, 8, n, g, check=False) == INVALID          # rows 8 .. 56 of 48
    q = op_linear("q4_bf16", N, K, w_d)
    assert dora_gain(q, a_d, b_d, m_d, r, s, row0, n, g, check=False) == UNSUPPORTED
    bad = op_linear("bf16", N, K, w_d)
    bad.layout = 1
    bad.K = 72                                                                             # tile-major needs K % 32 == 0
    assert dora_gain(bad, a_d, b_d, m_d, r, s, row0, n, g, check=False) == INVALID
    assert np.isnan(g.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------- mi_op_dora_rows
PARTS3 = [(0, 1040), (1040, 48), (1088, 272)]
KW = 64                                             # K of the matrix behind the gains
ROWS = [0, 1, -1, L.MI_MAX_ADAPTERS]               # a DoRA slot, a LoRA slot, no adapter, the engine-wide column (DoRA)
TYPES = {"f32": ("float32", 0, "float32"), "f32_rbf16": ("float32", L.RND_BF16, "bfloat16"),
         "f32_rf16": ("float32", L.RND_F16, "float16"), "bf16": ("bfloat16", 0, "bfloat16"), "f16": ("float16", 0, "float16")}


def dyadic(rng, shape, den, top):
    return (rng.integers(-top, top + 1, shape) / den).astype(np.float32)


def rows_inputs(rank, parts, wdt):
    """-> y, h, t (float32 values), table {(part, col): dict(a, b, rank, scale, m or None)}, W (fused rows, KW), row0s"""
    rng = np.random.default_rng([SEED, rank, len(parts)])
    ldy = sum(n for _, n in parts) + 8
    y = rng.standard_normal((4, ldy)).astype(np.float32)
    h = rng.standard_normal((4, parts[0][1] + 8)).astype(np.float32)
    t = dyadic(rng, (4, 192), 8, 16)
    w = round_to(rng.standard_normal((ldy - 8, KW)).astype(np.float32) * 0.05, wdt)
    table = {}
    ranks = {0: rank, 1: max(1, rank // 2), L.MI_MAX_ADAPTERS: 65 - rank}
    for col, rk in ranks.items():
        for p, (row0, n) in enumerate(parts):
            a = (rng.standard_normal((KW, rk)) * 0.05).astype(np.float32)
            b = dyadic(rng, (rk, n), 16, 16)
            scale = [0.375, 2.0, 0.5][p]
            m = None
            if col != 1 and p != 1:                 # a gain on parts 0 and 2 of the two DoRA columns only
                # m such that the exact gain sits within 2^-24 (relative) of a bfloat16 grid point in [0.5, 2): as far from
                # every rounding boundary of bfloat16 and float16 as a value can be
                target = round_to(0.5 + 1.5 * rng.random(n).astype(np.float32), "bfloat16").astype(np.float64)
                denom = 1.0 / dora_ref.exact_gain(w[row0:row0 + n], a, b, np.ones(n, np.float32), scale)
                m = (target * denom).astype(np.float32)
            table[p, col] = dict(a=a, b=b, rank=rk, scale=scale, m=m)
    return y, h, t, table, w


def dora_rows(*, M, act, rnd, row_adapter, parts, table, t, y, ldy, resid=None, ldr=0, tab_gain="auto", check=True):
    """mi_op_dora_rows, up stage.  table: {(part, col): (A, B, rank, scale, gain address or None)}"""
    slots = 3 * COLS
    ta, tb, tg = (C.c_void_p * slots)(), (C.c_void_p * slots)(), (C.c_void_p * slots)()
    tr, ts = (C.c_int32 * slots)(), (C.c_float * slots)()
    for (p, col), (a, b, rank, scale, gain) in table.items():
        i = p * COLS + col
        ta[i], tb[i], tr[i], ts[i], tg[i] = a.data_ptr(), b.data_ptr(), rank, scale, gain
    row0 = (C.c_int32 * 3)(*([p[0] for p in parts] + [0] * (3 - len(parts))))
    n = (C.c_int32 * 3)(*([p[1] for p in parts] + [0] * (3 - len(parts))))
    torch.cuda.synchronize()
    rc = L.lib().mi_op_dora_rows(None, 0, int(M), 0, int(act), int(rnd), 0, None, 0.0, C.c_void_p(row_adapter.data_ptr()), len(parts),
                                 row0, n, ta, tb, tr, ts, tg if tab_gain == "auto" else tab_gain, C.c_void_p(t.data_ptr()),
                                 C.c_void_p(y.data_ptr()), int(ldy), C.c_void_p(resid.data_ptr()) if resid is not None else None,
                                 int(ldr), L.LORA_STAGE_UP)
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


def restate(y, h, t, table, parts, logical, gains):
    """the rounding chain in NumPy float32: T(y + T(s (t B))), then T(T(g) * .), then T(h + .)  -> (y', h')"""
    R = lambda v: round_to(np.asarray(v, np.float32), logical)  # noqa: E731
    y2, h2 = y.copy(), (None if h is None else h.copy())
    for mrow, ad in enumerate(ROWS):
        for p, (row0, n) in enumerate(parts):
            v = y[mrow, row0:row0 + n].copy()
            e = table.get((p, ad))
            if e is not None:
                z = (t[mrow, p * 64:p * 64 + e["rank"]].astype(np.float64) @ e["b"].astype(np.float64)).astype(np.float32)   # exact
                z = np.float32(e["scale"]) * z
                v = R(v + R(z))
                if (p, ad) in gains:
                    v = R(R(gains[p, ad]) * v)
            if h is not None:
                h2[mrow, :n] = R(h[mrow, :n] + v)
            elif e is not None:
                y2[mrow, row0:row0 + n] = v
    return y2, h2


def bits(tn):
    return tn.cpu().contiguous().view(torch.int32 if tn.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("rank", [1, 64])
def test_rows_equal_the_restated_chain_exactly(rank, tname, resid):
    storage, rnd, logical = TYPES[tname]
    wdt = "float16" if logical == "float16" else "bfloat16"
    parts = PARTS3[:1] if resid else PARTS3         # (a residual goes with one part at column 0)
    y, h, t, table, w = rows_inputs(rank, parts, wdt)
    y, h = round_to(y, logical), round_to(h, logical)
    ldy, ldr = y.shape[1], h.shape[1]
    w_d = dev(w, wdt)
    ol = op_linear("bf16" if wdt == "bfloat16" else "f16", w.shape[0], KW, w_d)
    dtab, ltab, gains, g_dev = {}, {}, {}, {}
    for (p, col), e in table.items():
        a_d, b_d = dev(e["a"]), dev(e["b"])
        gptr = None
        if e["m"] is not None:
            row0, n = parts[p]
            exact = dora_ref.exact_gain(w[row0:row0 + n], e["a"], e["b"], e["m"], e["scale"])
            bound = gain_bound(KW, e["rank"], dora_ref.condition(w[row0:row0 + n], e["a"], e["b"], e["scale"]))
            for dt in ("bfloat16", "float16"):
                assert not dora_ref.near_boundary(exact, dt, bound), "the CPU-side choice of m left a gain near a boundary"
            g = torch.zeros(n, dtype=torch.float32, device="cuda")
            dora_gain(ol, a_d, b_d, dev(e["m"]), e["rank"], e["scale"], row0, n, g)
            g_dev[p, col] = g
            got = g.cpu().numpy()
            twin = exact.astype(np.float32)
            assert np.abs(got.astype(np.float64) - exact).max() <= bound * np.abs(exact).max()
            if logical != "float32":
                assert np.array_equal(round_to(got, logical), round_to(twin, logical))
            gains[p, col] = got if logical == "float32" else twin
            gptr = g.data_ptr()
        dtab[p, col] = (a_d, b_d, e["rank"], e["scale"], gptr)
        ltab[p, col] = (a_d, b_d, e["rank"], e["scale"])
    want_y, want_h = restate(y, h if resid else None, t, table, parts, logical, gains)
    rows_d, t_d = dev_i32(np.asarray(ROWS)), dev(t)
    y_d, h_d = dev(y, storage), (dev(h, storage) if resid else None)
    dora_rows(M=4, act=MIDT[storage], rnd=rnd, row_adapter=rows_d, parts=parts, table=dtab, t=t_d, y=y_d, ldy=ldy, resid=h_d, ldr=ldr)
    assert np.array_equal(bits(y_d), bits(dev(want_y, storage))), "y differs from the restated chain"
    if resid:
        assert np.array_equal(bits(h_d), bits(dev(want_h, storage))), "h differs from the restated chain"
    # the chain really multiplied: the DoRA rows moved away from the plain-LoRA result, the others did not
    y_l, h_l = dev(y, storage), (dev(h, storage) if resid else None)
    lora_rows(stages=L.LORA_STAGE_UP, M=4, act=MIDT[storage], rnd=rnd, row_adapter=rows_d, parts=parts, table=ltab, t=t_d, y=y_l,
              ldy=ldy, resid=h_l, ldr=ldr)
    out_d, out_l = (bits(h_d), bits(h_l)) if resid else (bits(y_d), bits(y_l))
    assert np.array_equal(out_d[1:3], out_l[1:3]), "rows without a gain differ from mi_op_lora_rows"
    assert not np.array_equal(out_d[0], out_l[0]) and not np.array_equal(out_d[3], out_l[3])
    if not resid:                                  # part 1 carries no gain in any column: plain LoRA bits on every row
        c0, c1 = PARTS3[1][0], PARTS3[1][0] + PARTS3[1][1]
        assert np.array_equal(out_d[:, c0:c1], out_l[:, c0:c1])
    # a table none of whose entries has a gain: the plain instantiation, mi_op_lora_rows bit for bit
    y_n, h_n = dev(y, storage), (dev(h, storage) if resid else None)
    dora_rows(M=4, act=MIDT[storage], rnd=rnd, row_adapter=rows_d, parts=parts, table={k: v[:4] + (None,) for k, v in dtab.items()},
              t=t_d, y=y_n, ldy=ldy, resid=h_n, ldr=ldr)
    assert np.array_equal(bits(h_n) if resid else bits(y_n), out_l)


def test_rows_refusals_launch_nothing():
    parts = PARTS3
    y, h, t, table, w = rows_inputs(1, parts, "bfloat16")
    e = table[0, 0]
    a_d, b_d = dev(e["a"]), dev(e["b"])
    g = torch.ones(parts[0][1] + 1, dtype=torch.float32, device="cuda")
    rows_d, t_d = dev_i32(np.asarray(ROWS)), dev(t)
    y_d = dev(round_to(y, "bfloat16"), "bfloat16")
    before = bits(y_d).copy()
    lib = L.lib()
    kw = dict(M=4, act=L.MI_BF16, rnd=0, row_adapter=rows_d, parts=parts, t=t_d, y=y_d, ldy=y.shape[1], check=False)
    ok = {(0, 0): (a_d, b_d, 1, 0.375, g.data_ptr())}
    assert dora_rows(table=ok, tab_gain=None, **kw) == INVALID and b"null" in lib.mi_last_error()
    assert dora_rows(table={(0, 0): (a_d, b_d, 1, 0.375, g.data_ptr() + 2)}, **kw) == INVALID and b"aligned" in lib.mi_last_error()
    assert dora_rows(table={(0, 0): (a_d, b_d, 0, 0.375, g.data_ptr())}, **kw) == INVALID and b"rank" in lib.mi_last_error()
    slots = 3 * COLS
    tg = (C.c_void_p * slots)()
    tg[1] = g.data_ptr()                                                       # a gain on an entry without A / B
    assert dora_rows(table=ok, tab_gain=tg, **kw) == INVALID
    assert np.array_equal(bits(y_d), before)
    assert dora_rows(table=ok, **dict(kw, check=True)) == 0                    # and the accepted call does write
    assert not np.array_equal(bits(y_d), before)
