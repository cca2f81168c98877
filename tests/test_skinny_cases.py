"""What tests/test_gpu_skinny_exact.py rests on and needs no device (tests/skinny_cases.py):

* the launch plans restated from gemm_skinny.hip and gemm_q4.hip, and that the case table reaches every required class;
* the exactness premise on the REFERENCE alone: for every exact "int" case the sum over k of the absolute values of the
  kernel's own terms stays below 2^24 units of the smallest scale -- so ANY order is exact -- and float32 accumulation
  forward, reversed and in the kernel's shape (32-wide blocks, the K slices summed in slice order) equals the float64 sum;
  the quantised kernels' formula, evaluated in float32 group by group, equals sum((scale q + bias) x);
* the one-hot probes cover both sides of every boundary of their case's plan, no two probed columns of W look alike, and the
  oracle returns W's columns; the three-term split of a float32 activation is exact and a lost term is seen;
* sensitivity: scales or biases rolled by a row or a group, a unit dropped at a slice boundary, two probed columns swapped,
  `lo` zeroed -- each changes the expected bits;
* the rules' caps: the oracle's float32-accumulating envelopes, on the very inputs of the device tests, stay under them, and a
  cap is 4 x the largest figure they show (the 16-bit one never above 10 %).
"""
import numpy as np
import pytest

from oracle import numerics, ref_quant

import skinny_cases as cases

EXACT_INT = [c for c in cases.CASES if c.data == "int"]
ONEHOT = [c for c in cases.CASES if c.data in ("onehot", "pair", "hot3p", "hot3g")]
RULE16 = [c for c in cases.CASES if not c.exact and cases.odt_of(c, "bfloat16") != "float32"]
RULE32 = [c for c in cases.CASES if c.data == "rand" and c.x32 and not c.rnd]


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plans and the table's coverage

def test_skinny_plan_restates_the_host_code():
    assert [cases.skinny_mt(m) for m in (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 6, 6, 8, 8, 8, 8]
    P = cases.skinny_plan
    p = P(40, 9, 4608, "dense", ksplit=5)
    assert (p.mt, p.nslab, p.ntiles, p.ngroups, p.nchunks, p.ksplit, p.grid) == (3, 1, 9, 2, 18, 5, 10)
    assert [s[:2] for s in p.slices] == [(0, 3), (3, 7), (7, 10), (10, 14), (14, 18)] and p.bounds == (768, 1792, 2560, 3584)
    assert p.slices[1][2:] == (24, 56)
    p = P(33, 3, 384, "q4", ksplit=3)                           # slabs, the split clamped, the last chunk half full
    assert (p.mt, p.nslab, p.ngroups, p.nchunks, p.ksplit, p.grid) == (2, 2, 1, 2, 2, 16) and p.slices == ((0, 1, 0, 2), (1, 2, 2, 3))
    p = P(100, 9, 640, "q4", ksplit=2)
    assert (p.mt, p.nslab, p.ngroups, p.grid, p.rows_padded) == (2, 4, 2, 32, 128)
    assert P(96, 3, 512, "q4", swiglu=True, ksplit=2).nslab == 1 and P(96, 3, 512, "q4", swiglu=True, ksplit=2).mt == 6
    assert P(97, 3, 512, "q4", swiglu=True, ksplit=2).nslab == 4
    assert P(64, 3, 512, "q4", swiglu=True).nslab == 1 and P(64, 3, 512, "q4").nslab == 2
    assert P(32, 3, 512, "q4").nslab == 1 and P(32, 3, 512, "q4", x32=True).nslab == 1
    assert P(128, 3, 512, "q8").mt == 8 and P(128, 3, 512, "q8").nslab == 1
    p = P(17, 9, 288, "dense", ksplit=2)                        # K % 256 = 32: the second slice holds one unit
    assert p.slices == ((0, 1, 0, 8), (1, 2, 8, 9))
    p = P(17, 9, 320, "q8", ksplit=2)
    assert p.slices == ((0, 1, 0, 4), (1, 2, 4, 5))
    p = P(65, 3, 480, "dense", ksplit=3)                        # K % 256 = 224: seven of the last chunk's eight units
    assert p.ksplit == 2 and p.slices[1] == (1, 2, 8, 15)
    assert P(8, 3, 8192, "dense", x32=True, ksplit=32, defer_norm=True).ksplit == 16


def test_q4_plan_restates_the_host_code():
    Q = cases.q4_plan
    p = Q(61, 17, 1152, False, (2, 4, 2, 2, 2))
    assert (p.mt, p.nslab, p.ntu, p.ntiles, p.ngroups, p.nblk, p.grid) == (2, 2, 9, 17, 3, 9, 16) and p.slices == ((0, 4), (4, 9))
    p = Q(64, 9, 1024, True, (4, 4, 2, 1, 4))
    assert (p.mt, p.nslab, p.ntu, p.ngroups, p.grid) == (4, 1, 9, 3, 3)
    p = Q(100, 9, 896, True, (4, 10, 1, 1, 2))
    assert (p.nslab, p.ngroups, p.grid) == (2, 1, 16)
    assert Q(17, 5, 640, False, (1, 1, 8, 1, 4)) is None       # nblk / ks < KW
    assert Q(17, 5, 640, False, (3, 4, 2, 1, 4)) is None       # 3 / 4 row tiles: SwiGLU only
    assert Q(17, 5, 640, True, (3, 4, 2, 1, 4)) is None        # more row tiles than rows
    assert Q(64, 9, 1024, False, (2, 4, 2, 1, 1)) is None      # one staging wave cannot carry 17 pieces
    S = cases.q4_supported
    assert S("q4", False, 17, 640, 5, forced=True) and not S("q4", False, 17, 640, 5)
    assert S("q4", False, 33, 128, 1024) and not S("q4", False, 33, 128, 1024, bias=True)
    assert not S("q4", False, 16, 640, 2048) and not S("q8", False, 33, 640, 2048) and not S("q4", True, 17, 640, 2048)
    for c in cases.CASES:
        assert c.plan() is not None, cases.case_id(c)
        if c.q4plan is not None:
            assert c.routed_to_q4() and c.kind == "q4" and not c.x32, cases.case_id(c)
        else:
            assert not c.routed_to_q4(forced=False), cases.case_id(c)       # (no forced plan: the narrow matrices stay on skinny_kernel)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_case_table_reaches_every_class(kind):
    reached = set()
    for c in cases.CASES:
        if c.kind == kind:
            reached |= cases.classes_of(c)
    missing = cases.REQUIRED[kind] - reached
    print(f"{kind}: {sum(c.kind == kind for c in cases.CASES)} cases; reached {sorted(reached)}")
    assert not missing, missing


def test_case_table_is_not_a_cross_product():
    n = {kind: sum(c.kind == kind for c in cases.CASES) for kind in cases.KINDS}
    print("cases per kind:", n)
    assert all(40 <= v <= 110 for v in n.values()), n
    for c in cases.CASES:
        assert c.K <= 4608 and c.K % cases.UNIT[c.kind] == 0, cases.case_id(c)
        assert c.tiles in (1, 3, 5, 8, 9, 17) or (c.tiles == 34 and c.data == "rand") or (c.tiles == 1024 and c.bias), cases.case_id(c)
        if c.x32:
            assert c.M <= 32
        if c.pro:
            assert c.data == "rand" and (c.x32 or c.q4plan is not None)      # 16-bit: only gemm_q4's preparation pass takes a norm
    assert all(c.ksplit == 0 and c.data == "int" for c in cases.COST_MODEL)


# ---------------------------------------------------------------------------------------------------------------------------
# the exactness premise

def _offs(c, act):
    """what the kernel adds to a code: int4 on bfloat16 weights 16 (the magic-number unpack), else 0"""
    return 16.0 if (c.kind == "q4" and cases.wdt_of(c, act) == "bfloat16") else 0.0


def _unit(c):
    return 2.0 ** -(cases._wexp(c) + (0 if c.kind == "dense" else 3))


def _term_bound(c, act, d):
    """max over outputs of sum_k |terms|, in units of the smallest scale"""
    x = np.abs(d["x"][0]).astype(np.float64)
    if c.kind == "dense":
        t = np.abs(d["w"]).astype(np.float64)
    else:
        packed, s, b = d["q"]
        q = ref_quant.unpack(packed, 4 if c.kind == "q4" else 8).astype(np.float64)
        o = _offs(c, act)
        s, b = np.repeat(s.astype(np.float64), 64, axis=1), np.repeat(b.astype(np.float64), 64, axis=1)
        t = np.abs(s) * (o + q) + np.abs(b - o * s)
    bound = (x @ t.T).max()
    if d["h"] is not None:
        bound += 8
    if d["b"] is not None:
        bound += 8
    return bound / _unit(c)


def _f32_orders(x, w, p):
    """Sum over k of x[m, k] w[n, k] with float32 accumulators -> [(name, (M, n))]: forward, reversed, and 32-wide blocks
    (one MFMA step each) added in order inside each K slice of plan p, the slices added in slice order."""
    prod = (x[:, None, :] * w[None, :, :]).astype(np.float32)
    out = [("forward", np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1]),
           ("reversed", np.cumsum(prod[..., ::-1], axis=-1, dtype=np.float32)[..., -1])]
    blocks = np.cumsum(prod.reshape(*prod.shape[:2], -1, 32), axis=-1, dtype=np.float32)[..., -1]
    step = 256 if p.kernel == "skinny" else 128
    cuts = [0] + [b // 32 for b in p.bounds] + [blocks.shape[-1]]
    total = np.zeros(prod.shape[:2], np.float32)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if p.kernel == "q4":                                  # K lanes: lane kw owns every KW-th block of the slice; lanes in order
            part = np.zeros(prod.shape[:2], np.float32)
            for kw in range(p.KW):
                mine = np.concatenate([blocks[..., i:i + step // 32] for i in range(a + kw * 4, b, 4 * p.KW)], axis=-1)
                part = (part + np.cumsum(mine, axis=-1, dtype=np.float32)[..., -1]).astype(np.float32)
        else:
            part = np.cumsum(blocks[..., a:b], axis=-1, dtype=np.float32)[..., -1]
        total = (total + part).astype(np.float32)
    out.append(("slices", total))
    return out


def _sample(n, k, rng):
    if n <= k:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(k // 4), np.arange(n - k // 4, n), rng.integers(0, n, k // 2)]))


@pytest.mark.parametrize("c", EXACT_INT, ids=cases.case_id)
def test_exact_cases_are_exact_in_float32_in_any_order(c):
    for act in c.acts:
        d = cases.build(c, act)
        x, w = d["x"][0], d["w"]
        unit, xdt = _unit(c), ("float32" if c.x32 else act)
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= cases.xmax_of(c)
        assert np.array_equal(w / unit, np.rint(w / unit))
        # (values of the dtypes: what reaches the device is what the oracle multiplies)
        assert np.array_equal(numerics.round_to(x, xdt), x)
        if c.kind == "dense":
            assert np.array_equal(numerics.round_to(w, cases.wdt_of(c, act)), w)
        else:
            assert all(np.array_equal(numerics.round_to(a, cases.wdt_of(c, act)), a) for a in d["q"][1:])
            assert np.array_equal(ref_quant.dequantize(*d["q"], 64, 4 if c.kind == "q4" else 8), w)
        if c.x32:                                             # integers: mid and lo of the split are zero
            hi, mid, lo = cases.split3(x)
            assert np.array_equal(hi, x) and not mid.any() and not lo.any()
        # any order: every partial sum of any subset is a multiple of `unit` of magnitude below 2^24 units
        bound = _term_bound(c, act, d)
        assert bound < 2 ** 24, bound
        rng = np.random.default_rng(1)
        mi, ni = _sample(x.shape[0], 16, rng), _sample(w.shape[0], 48, rng)
        want = x[mi].astype(np.float64) @ w[ni].astype(np.float64).T
        for name, got in _f32_orders(x[mi], w[ni], c.plan()):
            assert np.array_equal(got.astype(np.float64), want), name


@pytest.mark.parametrize("kind,act,K", [("q4", "bfloat16", 4608), ("q4", "float16", 1152), ("q8", "bfloat16", 4608),
                                        ("q8", "float16", 320)])
def test_quantised_kernel_formula_is_exact(kind, act, K):
    """y = sum over 64-groups of fma(sc, sum((offs + q) x), fma(bias - offs sc, sum(x), y)) in float32 (quant_accumulate),
    groups forward and reversed, equals sum((sc q + bias) x) in float64: offs = 16 for int4 on bfloat16, else 0."""
    rng = np.random.default_rng(K)
    N, M, bits = 48, 8, (4 if kind == "q4" else 8)
    packed, scales, biases = (cases.exact_q4 if kind == "q4" else cases.exact_q8)(rng, N, K)
    xm = 1 if (kind == "q8" and K > 2048) else 3
    x = rng.integers(-xm, xm + 1, (M, K)).astype(np.float32)
    q = ref_quant.unpack(packed, bits).astype(np.float32)
    want = x.astype(np.float64) @ ref_quant.dequantize(packed, scales, biases, 64, bits).astype(np.float64).T
    offs = np.float32(16.0 if (kind == "q4" and act == "bfloat16") else 0.0)
    for order in (range(K // 64), reversed(range(K // 64))):
        y32, y64 = np.zeros((M, N), np.float32), np.zeros((M, N), np.float64)
        for g in order:
            xs, qs = x[:, 64 * g:64 * g + 64], q[:, 64 * g:64 * g + 64]
            d = ((offs + qs)[None] * xs[:, None]).astype(np.float32)
            d = np.cumsum(d, axis=-1, dtype=np.float32)[..., -1]
            sx = np.cumsum(xs, axis=-1, dtype=np.float32)[:, -1:]
            sc, bb = scales[None, :, g], (biases[:, g] - offs * scales[:, g]).astype(np.float32)[None]
            t32 = ((bb * sx).astype(np.float32) + y32).astype(np.float32)
            t64 = bb.astype(np.float64) * sx + y64
            assert np.array_equal(t32, t64)
            y32 = ((sc * d).astype(np.float32) + t32).astype(np.float32)
            y64 = sc.astype(np.float64) * d + t64
            assert np.array_equal(y32, y64)
        assert np.array_equal(y32.astype(np.float64), want)


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity: a subtly wrong kernel changes the expected bits

@pytest.mark.parametrize("kind", ["q4", "q8"])
def test_scales_and_biases_vary_by_row_and_group(kind):
    """A scale or bias read from the neighbouring row or group changes the result."""
    c = next(c for c in EXACT_INT if c.kind == kind and c.K == 4608 and c.epi == "store" and not c.x32)
    d = cases.build(c, "bfloat16")
    for axis in (0, 1):
        for which in (1, 2):
            q = list(d["q"])
            q[which] = np.roll(q[which], 1, axis=axis)
            got = cases.oracle(c, "bfloat16", d, w=ref_quant.dequantize(*q, 64, 4 if kind == "q4" else 8))
            assert np.mean(got != d["want"]) > 0.5, (axis, which)


@pytest.mark.parametrize("c", [c for c in EXACT_INT if c.exact and len(c.plan().bounds) >= 1], ids=cases.case_id)
def test_a_unit_dropped_or_read_twice_at_a_slice_boundary_is_seen(c):
    act = c.acts[0]
    d = cases.build(c, act)
    p = c.plan()
    u = cases.UNIT[c.kind]
    for b in (p.bounds[0], p.bounds[-1]):
        for lo in (b - u, b):                                 # the last unit of the slice in front, the first of the slice behind
            x = d["x"].copy()
            x[..., lo:lo + u] = 0                             # dropped
            assert np.mean(cases.oracle(c, act, d, x=x) != d["want"]) > 0.25, (b, lo)
            x = d["x"].copy()
            x[..., lo:lo + u] *= 2                            # read twice
            assert np.mean(cases.oracle(c, act, d, x=x) != d["want"]) > 0.25, (b, lo)


def test_a_padded_row_or_a_neighbouring_row_is_seen():
    """rows differ: an output row computed from the row above it changes (65 and 97 rows: 31 padded fragment rows)."""
    for c in (c for c in EXACT_INT if c.exact and c.M in (65, 97) and not c.x32):
        d = cases.build(c, "bfloat16")
        assert np.mean(cases.oracle(c, "bfloat16", d, x=np.roll(d["x"], 1, axis=1)) != d["want"]) > 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# column selection

@pytest.mark.parametrize("c", ONEHOT, ids=cases.case_id)
def test_probes_cover_both_sides_of_every_boundary(c):
    p = c.plan()
    d = cases.build(c, c.acts[0])
    x = d["x"]
    assert x.shape[1:] == (c.M, c.K) and ((x != 0).sum(axis=-1) == 1).all()
    cols = np.abs(x).argmax(axis=-1)                          # (launches, M)
    hot = set(cols.ravel().tolist())
    assert {0, c.K - 1} <= hot
    u = cases.UNIT[c.kind]
    named = {8, u, 256} | {s[0] * 256 for s in p.slices[1:]} if p.kernel == "skinny" else \
        {8, 128, 128 * p.KW, 256} | {b0 * 128 for b0, _ in p.slices[1:]}
    assert len(p.slices) == p.ksplit and set(p.bounds) <= named
    for e in named:
        if 0 < e < c.K:
            assert {e - 1, e} <= hot, e
    if p.kernel == "skinny" and c.K > 256:                    # the last chunk, ragged or not: its first column and K - 1
        assert {(c.K - 1) // 256 * 256 - 1, (c.K - 1) // 256 * 256} <= hot
    assert x.shape[0] >= 2
    if c.M > 16:                                              # the rows on both sides of a fragment-row boundary change probes
        for r in range(16, c.M, 16):
            assert len(set(cols[:, r - 1].tolist())) >= 2 and len(set(cols[:, r].tolist())) >= 2, r
            assert (cols[:, r - 1] != cols[:, r]).all()


@pytest.mark.parametrize("c", ONEHOT, ids=cases.case_id)
def test_one_hot_oracle_returns_columns_of_w(c):
    for act in c.acts:
        d = cases.build(c, act)
        if c.data != "hot3g":
            assert np.array_equal(d["want"], cases.onehot_want(c, act, d))
        hot = sorted(set(np.abs(d["x"]).argmax(axis=-1).ravel().tolist()))
        w = d["w"]
        cols = (w[:c.N] * w[c.N:]).T[hot] if c.data == "pair" else numerics.round_to(w.T[hot], cases.odt_of(c, act))
        assert len({a.tobytes() for a in cols}) == len(cols)           # no two probed columns look alike
        # ... so swapping two probed columns of W changes the expectation
        w2 = w.copy()
        w2[:, [hot[0], hot[-1]]] = w2[:, [hot[-1], hot[0]]]
        w2[:, [hot[1], hot[2]]] = w2[:, [hot[2], hot[1]]]
        got = cases.oracle(c, act, d, w=w2)
        assert (got != d["want"]).any(axis=-1).sum() >= 4
        if c.data == "pair":                                           # silu(g) = g: sigmoid is 1 in float32 and in float64
            g = w[:c.N]
            assert g.min() >= 32 and np.float32(1.0) / (np.float32(1.0) + np.exp(-g.min(), dtype=np.float32)) == 1.0
            assert (w[c.N:] % 2 == 1).all() and w[c.N:].max() < 128
            if c.kind == "q4":
                assert all(np.array_equal(numerics.round_to(a, "float16"), a) and np.array_equal(numerics.round_to(a, "bfloat16"), a)
                           for a in d["q"][1:])


@pytest.mark.parametrize("c", [c for c in cases.CASES if c.data.startswith("hot3")], ids=cases.case_id)
def test_hot3_pins_mid_and_lo(c):
    d = cases.build(c, "float32")
    x, w = d["x"], d["w"]
    hi, mid, lo = cases.split3(x)
    assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))       # the split is exact
    nz = x != 0
    assert (hi[nz] != 0).all() and (mid[nz] != 0).all() and (lo[nz] != 0).all()
    assert c.epi == "store" and c.x32 and not c.rnd
    want64 = x.astype(np.float64) @ w.astype(np.float64).T
    bound = 2.0 ** -22 * np.abs(want64)
    if c.data == "hot3p":                                     # +-2^j x is a float32: the oracle's value is exact
        assert np.array_equal(d["want"].astype(np.float64), want64)
    else:
        assert (np.abs(d["want"] - want64) <= bound).all()
    for name, xs in (("lo", hi.astype(np.float64) + mid), ("mid", hi.astype(np.float64) + lo)):
        got = (xs @ w.astype(np.float64).T).astype(np.float32)
        assert (got != d["want"]).all(), name                 # every element moves ...
        assert (np.abs(got - want64) > bound).all(), name     # ... by more than the bound allows (2^-17 and 2^-9 against 2^-22)


# ---------------------------------------------------------------------------------------------------------------------------
# the rules on the reference side

def _envelopes(c, act, d):
    try:
        for mode in ("f32_seq32", "f32_pairwise"):
            numerics.set_accum(mode)
            yield mode, cases.oracle(c, act, d)
    finally:
        numerics.set_accum("exact")


def test_rule_cap_is_measured_on_the_reference():
    shares = []
    for c in RULE16:
        for act in c.acts:
            d = cases.build(c, act)
            odt = cases.odt_of(c, act)
            for mode, got in _envelopes(c, act, d):
                worst, frac = cases.rule_stats(got, d["want"], odt)
                print(f"{cases.case_id(c)} {act} {mode}: worst {worst:.3f} unit, {100 * frac:.4f} % of {got.size} beyond half")
                assert np.isfinite(got).all() and worst <= 1.0, (cases.case_id(c), act, mode, worst)
                shares.append((frac, cases.case_id(c), act, mode))
    top = max(shares)
    print(f"largest share {100 * top[0]:.4f} % ({top[1:]}); cap {100 * cases.RULE_CAP:.4f} %")
    assert top[0] > 0                                                     # (a cap of zero would be no rule)
    assert all(s[0] <= cases.RULE_CAP for s in shares)                    # the reference alone stays under the cap
    assert cases.RULE_CAP <= 4 * top[0] * (1 + 1e-9) and cases.RULE_CAP <= 0.10
    # SwiGLU on exact sums: the envelopes ARE the oracle
    assert all(s[0] == 0 for s in shares if s[1].split("-")[1] == "int")


def test_float32_cap_is_measured_on_the_reference():
    worsts = []
    assert RULE32 and all(c.x32 and c.pro and not c.swiglu and c.epi == "store" for c in RULE32)
    for c in RULE32:
        d = cases.build(c, "float32")
        scale = cases.sum_abs_xw(c, "float32", d)
        for mode, got in _envelopes(c, "float32", d):
            worst = cases.f32_rule_stat(got, d["want"], scale)
            print(f"{cases.case_id(c)} {mode}: worst {worst:.4f} unit of 2^-24 sum |x w|")
            worsts.append((worst, cases.case_id(c), mode))
    top = max(worsts)
    print(f"largest {top[0]:.4f} ({top[1:]}); cap {cases.F32_CAP:.4f}")
    assert top[0] > 0 and all(w[0] <= cases.F32_CAP for w in worsts)
    assert cases.F32_CAP <= 4 * top[0] * (1 + 1e-3)


def test_rules_reject_what_they_should():
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
    scale = np.full(want.shape, 100.0)
    assert cases.assert_f32_rule(want, want, scale) == 0.0
    with pytest.raises(AssertionError):
        cases.assert_f32_rule(want + np.float32(2.0 ** -22 * 100.0), want, scale)          # four whole units
    with pytest.raises(AssertionError):
        cases.assert_f32_rule(got * np.float32("nan"), want, scale)
