"""What tests/test_gpu_gemv16.py rests on and needs no device (tests/gemv16_cases.py):

* the launch plan restated from gemv_mfma.hip / gemv_phase.h, and that the case table reaches every class of it on devices
  of 64, 256 and 304 compute units;
* the exactness premise on the REFERENCE alone: for every exact case, float32 accumulation forward, reversed and in the
  kernel's shape (32-wide blocks dealt to 8 waves, the waves summed in order) equals the float64 sum, and every partial sum
  of absolute values stays below 2^24 units -- so ANY order is exact; for int4, the kernel's formula
  scale * sum((offs + q) x) + (bias - offs * scale) * sum(x), evaluated in float32 per 64-group, equals sum((scale q + bias) x);
* the one-hot probes cover both sides of every boundary of their case's plan, and the oracle returns W's columns;
* the rule's cap: the oracle's float32-accumulating envelopes, on the very inputs of the device tests, stay under it, and it is
  4 x the largest share they show (never above 10 %).
"""
import numpy as np
import pytest

from oracle import numerics, ref_quant

import gemv16_cases as cases

EXACT_INT = [c for c in cases.CASES if c.data == "int"]
ONEHOT = [c for c in cases.CASES if c.data in ("onehot", "pair")]
RULE = [c for c in cases.CASES if not c.exact]
CUS = 256


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plan and the table's coverage

def test_launch_plan_restates_the_host_code():
    P = cases.launch_plan
    p = P(8, 48, 4096, "dense", "store", 256)
    assert (p.MB, p.kc, p.nchunks, p.J, p.DB, p.tiles_first, p.tiles_last, p.batches) == (8, 4096, 1, 1, False, 1, 1, 1)
    assert (p.BK, p.UK, p.TB, p.KS) == (32, 16, 1, 4096)
    p = P(8, 48, 6144, "q4", "store", 256)
    assert (p.kc, p.nchunks, p.J, p.DB, p.batches) == (6144, 1, 2, False, 1) and (p.BK, p.UK, p.TB, p.KS) == (128, 4, 2, 4096)
    p = P(8, 16 * 257, 8320, "q4", "store", 256)
    assert (p.kc, p.nchunks, p.J, p.DB) == (4096, 3, 1, True) and (p.tiles_first, p.tiles_last, p.batches) == (2, 1, 1)
    p = P(9, 16 * 513, 4224, "q4", "store", 256)
    assert (p.MB, p.kc, p.nchunks, p.J, p.DB) == (16, 4096, 2, 1, False) and (p.tiles_first, p.tiles_last, p.batches) == (3, 2, 2)
    p = P(7, 48, 2080, "dense", "swiglu", 256)
    assert (p.UK, p.TB, p.KS) == (8, 1, 2048)
    p = P(16, 48, 4096, "q4", "swiglu", 304)
    assert (p.MB, p.UK, p.TB, p.KS, p.grid) == (16, 4, 1, 4096, 3)
    p = P(1, 16 * 64, 256, "dense", "store", 64)
    assert (p.grid, p.tiles_first, p.tiles_last) == (64, 1, 1)
    p = P(16, 48, 6144, "dense", "store", 256)                # 9..16 rows never hold more than 4096 columns
    assert (p.kc, p.nchunks, p.J, p.DB) == (4096, 2, 1, False)


@pytest.mark.parametrize("cus", cases.CUS_CHECKED)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_case_table_reaches_every_class(kind, cus):
    reached = set()
    for c in cases.CASES:
        if c.kind == kind:
            reached |= cases.classes_of(c, cus)
    missing = cases.REQUIRED[kind] - reached
    print(f"{kind}, {cus} CUs: reached {sorted(reached)}")
    assert not missing, missing


def test_case_table_is_not_a_cross_product():
    for kind in cases.KINDS:
        n = sum(c.kind == kind for c in cases.CASES)
        assert 30 <= n <= 60, (kind, n)
    # the largest matrix: (CUs + 1) x 16 rows of 8320 columns
    assert max(c.wrows(CUS) * c.K for c in cases.CASES) == 257 * 16 * 8320
    for c in cases.CASES:
        if c.epi == "gu8":
            assert c.kind == "dense" and all(c.width(cus) % 16 == 0 for cus in cases.CUS_CHECKED)
    pair = {c.width(CUS) // 16 for c in cases.CASES if c.data == "pair"}
    assert 1 in pair and any(i % 2 == 1 and i > 1 for i in pair)           # I = 16 and I = 16 x odd


# ---------------------------------------------------------------------------------------------------------------------------
# the exactness premise

def _sample_rows(rows, rng):
    if rows <= 64:
        return np.arange(rows)
    return np.unique(np.concatenate([np.arange(16), np.arange(rows - 16, rows), rng.integers(0, rows, 32)]))


def _f32_orders(x, w):
    """Sum over k of x[m, k] w[n, k] with float32 accumulators in three orders -> [(name, (M, n))]."""
    prod = (x[:, None, :] * w[None, :, :]).astype(np.float32)
    out = [("forward", np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1]),
           ("reversed", np.cumsum(prod[..., ::-1], axis=-1, dtype=np.float32)[..., -1])]
    blocks = np.cumsum(prod.reshape(*prod.shape[:2], -1, 32), axis=-1, dtype=np.float32)[..., -1]      # one MFMA step each
    total = np.zeros(prod.shape[:2], np.float32)
    for wave in range(8):
        mine = blocks[..., wave::8]
        part = np.cumsum(mine, axis=-1, dtype=np.float32)[..., -1] if mine.shape[-1] else np.zeros(prod.shape[:2], np.float32)
        total = (total + part).astype(np.float32)
    out.append(("waves", total))
    return out


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("c", EXACT_INT, ids=cases.case_id)
def test_exact_cases_are_exact_in_float32_in_any_order(c, act):
    d = cases.build(c, act, CUS)
    x, w = d["x"][0], d["w"]
    unit = 2.0 ** -(cases._wexp(c) + (3 if c.kind == "q4" else 0))
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 3
    assert np.array_equal(w / unit, np.rint(w / unit))
    # (values of the dtypes: what reaches the device is what the oracle multiplies)
    assert np.array_equal(numerics.round_to(x, act), x)
    if c.kind == "dense":
        assert np.array_equal(numerics.round_to(w, act), w)
    else:
        assert all(np.array_equal(numerics.round_to(a, act), a) for a in d["q"][1:])
    # any order: every partial sum of any subset is a multiple of `unit` of magnitude below 2^24 units
    bound = (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T).max() / unit
    if c.kind == "q4":                    # the kernel's terms: scale (16 + q) x and (bias - 16 scale) x, group by group
        s, b = d["q"][1].astype(np.float64), d["q"][2].astype(np.float64)
        qmax = np.repeat(31 * np.abs(s) + np.abs(b - 16 * s), 64, axis=1)
        bound = (np.abs(x).astype(np.float64) @ qmax.T).max() / unit
    assert bound < 2 ** 24, bound
    idx = _sample_rows(w.shape[0], np.random.default_rng(1))
    want = x.astype(np.float64) @ w[idx].astype(np.float64).T
    for name, got in _f32_orders(x, w[idx]):
        assert np.array_equal(got.astype(np.float64), want), name


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("K", [128, 4224, 8320])
def test_int4_kernel_formula_is_exact(act, K):
    """y = sum over 64-groups of fma(sc, sum((offs + q) x), fma(bias - offs sc, sum(x), y)) in float32, groups forward and
    reversed, equals sum((sc q + bias) x) in float64: offs = 16 on bfloat16 (the magic-number unpack), 0 on float16."""
    rng = np.random.default_rng(K)
    N, M = 48, 8
    packed, scales, biases = cases.exact_q4(rng, N, K)
    x = rng.integers(-3, 4, (M, K)).astype(np.float32)
    q = ref_quant.unpack(packed, 4).astype(np.float32)
    want = x.astype(np.float64) @ ref_quant.dequantize(packed, scales, biases, 64, 4).astype(np.float64).T
    offs = np.float32(16.0 if act == "bfloat16" else 0.0)
    for order in (range(K // 64), reversed(range(K // 64))):
        y32, y64 = np.zeros((M, N), np.float32), np.zeros((M, N), np.float64)
        for g in order:
            xs, qs = x[:, 64 * g:64 * g + 64], q[:, 64 * g:64 * g + 64]
            d = ((offs + qs)[None] * xs[:, None]).astype(np.float32)
            d = np.cumsum(d, axis=-1, dtype=np.float32)[..., -1]
            sx = np.cumsum(xs, axis=-1, dtype=np.float32)[:, -1:]
            sc, bb = scales[None, :, g], (biases[:, g] - offs * scales[:, g]).astype(np.float32)[None]
            # fused or not makes no difference when the products are exact: both are checked against float64
            t32 = ((bb * sx).astype(np.float32) + y32).astype(np.float32)
            t64 = bb.astype(np.float64) * sx + y64
            assert np.array_equal(t32, t64)
            y32 = ((sc * d).astype(np.float32) + t32).astype(np.float32)
            y64 = sc.astype(np.float64) * d + t64
            assert np.array_equal(y32, y64)
        assert np.array_equal(y32.astype(np.float64), want)


def test_int4_scales_and_biases_vary_by_row_and_group():
    """A scale or bias read from the neighbouring row or group changes the result."""
    c = next(c for c in EXACT_INT if c.kind == "q4" and c.K == 4096 and c.epi == "store")
    d = cases.build(c, "bfloat16", CUS)
    packed, scales, biases = d["q"]
    x = d["x"]
    for axis in (0, 1):
        for which in (1, 2):
            q = [packed, scales, biases]
            q[which] = np.roll(q[which], 1, axis=axis)
            got = numerics.round_to(numerics.matmul_nt(x, ref_quant.dequantize(*q, 64, 4)), "bfloat16")
            assert np.mean(got != d["want"]) > 0.5, (axis, which)


# ---------------------------------------------------------------------------------------------------------------------------
# column selection

@pytest.mark.parametrize("c", ONEHOT, ids=cases.case_id)
def test_probes_cover_both_sides_of_every_boundary(c):
    for cus in cases.CUS_CHECKED:
        p = c.plan(cus)
        d = cases.build(c, "bfloat16", cus)
        hot = set(d["x"].argmax(axis=-1).ravel().tolist())
        assert {0, c.K - 1} <= hot
        for e in (8, 32, p.BK, p.KS, p.kc, 2 * p.kc):
            if 0 < e < c.K:
                assert {e - 1, e} <= hot, e
        if p.J == 2:
            assert 8 * (c.K // 8 - 1) in hot and 8 * (c.K // 8 - 1) >= 8 * 512       # a second staging item's first column
        if c.K > 4096 and c.data == "onehot":
            assert {4095, 4096} <= hot
        assert d["x"].shape[1] == c.M and (d["x"].sum(axis=-1) == 1).all()


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("c", ONEHOT, ids=cases.case_id)
def test_one_hot_oracle_returns_columns_of_w(c, act):
    d = cases.build(c, act, CUS)
    assert np.array_equal(d["want"], cases.onehot_want(c, d))
    cols = d["w"].T[sorted(set(d["x"].argmax(axis=-1).ravel().tolist()))]
    if c.data == "onehot":                                    # no two probed columns look alike
        assert len({a.tobytes() for a in cols}) == len(cols)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule on the reference side

def test_rule_cap_is_measured_on_the_reference():
    shares = []
    try:
        for c in RULE:
            for act in cases.ACTS:
                d = cases.build(c, act, CUS)
                for mode in ("f32_seq32", "f32_pairwise"):
                    numerics.set_accum(mode)
                    got = cases.oracle(c, act, d)
                    numerics.set_accum("exact")
                    worst, frac = cases.rule_stats(got, d["want"], act)
                    print(f"{cases.case_id(c)} {act} {mode}: worst {worst:.3f} unit, {100 * frac:.4f} % of {got.size} beyond half")
                    assert np.isfinite(got).all() and worst <= 1.0, (cases.case_id(c), act, mode, worst)
                    shares.append((frac, cases.case_id(c), act, mode))
    finally:
        numerics.set_accum("exact")
    top = max(shares)
    print(f"largest share {100 * top[0]:.4f} % ({top[1:]}); cap {100 * cases.RULE_CAP:.4f} %")
    assert top[0] > 0                                                     # (a cap of zero would be no rule)
    assert all(s[0] <= cases.RULE_CAP for s in shares)                    # the reference alone stays under the cap
    assert cases.RULE_CAP <= 4 * top[0] * (1 + 1e-9) and cases.RULE_CAP <= 0.10
    # SwiGLU on exact sums: the envelopes ARE the oracle
    assert all(s[0] == 0 for s in shares if s[1].split("-")[1] == "int")


def test_rule_rejects_what_it_should():
    want = np.linspace(-2, 2, 64).astype(np.float32).reshape(4, 16)
    assert cases.assert_rule(want, want, "bfloat16") == (0.0, 0.0)
    got = want.copy()
    got[1, 3] = np.nan
    with pytest.raises(AssertionError):
        cases.assert_rule(got, want, "bfloat16")
    rms = np.sqrt(np.mean(np.square(want), axis=-1, keepdims=True))
    got = (want + 0.8 * 2.0 ** -7 * np.maximum(np.abs(want), rms)).astype(np.float32)      # all within a unit, beyond half of one
    assert cases.rule_stats(got, want, "bfloat16")[0] <= 1.0
    with pytest.raises(AssertionError):
        cases.assert_rule(got, want, "bfloat16")
