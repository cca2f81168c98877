"""What tests/test_gpu_lora_rows.py rests on and needs no device (tests/lora_rows_cases.py):

* the case table reaches every branch tag of the two kernels, restated from the shapes alone, and is no cross product;
* the exactness premise on the REFERENCE alone, per exact case: all data are small integers (values of T), the sum of the
  absolute values of the terms of x A and of t B stays below 2^24 -- so ANY float32 order is exact -- and float32 sums in the
  kernel's order and reversed equal the float64 sum; the exact norm stages +-w; the yardstick's bits are the oracle's
  (ref_model.Linear's LoRA term); the 16-bit types sit on ties of T at every rounding point, counted here;
* the rule cases: the near share of each, printed and held under NEAR_CAP; the bound on t is a positive multiple of 2^-24
  and the reference's own float32 orders stay inside it;
* sensitivity: each of the wrong kernels the device test must catch changes the expected bits of some exact case.
"""
import numpy as np
import pytest

from oracle.numerics import round_f64, round_to

import lora_rows_cases as cases

EXACT = [c for c in cases.CASES if c.exact]
RULE = [c for c in cases.CASES if not c.exact]


# ---------------------------------------------------------------------------------------------------------------------------
# the table

def test_case_table_reaches_every_tag():
    reached = set()
    for c in cases.CASES:
        reached |= cases.tags(c)
    print(f"{len(cases.CASES)} cases ({len(EXACT)} exact, {len(RULE)} rule); reached {sorted(reached)}")
    missing = cases.REQUIRED - reached
    assert not missing, missing


def test_case_table_is_not_a_cross_product():
    assert 24 <= len(cases.CASES) <= 48, len(cases.CASES)
    for c in cases.CASES:
        cid = cases.case_id(c)
        assert c.M in (1, 3, 9) and 1 <= c.K <= cases.K_MAX and 1 <= len(c.parts) <= 3, cid
        ends = sorted((r0, r0 + n) for r0, n in c.parts)
        assert ends[0][0] >= 0 and ends[-1][1] < c.ldy and all(a[1] <= b[0] for a, b in zip(ends[:-1], ends[1:])), cid
        ranks = [p[0] for _, parts in c.adapters for p in parts if p is not None]
        assert all(1 <= r <= 64 for r in ranks) and all(len(parts) == len(c.parts) for _, parts in c.adapters), cid
        if c.K > 4096:                                  # the big K: M <= 3, rank <= 8 (A stays around a megabyte)
            assert c.M <= 3 and max(ranks) <= 8, cid
        for _, parts in c.adapters:
            for p in parts:
                if p is not None:
                    sc = abs(p[1])
                    if c.cancel:
                        assert sc == cases.THIRD and c.tname == "f32", cid
                    else:
                        assert (np.log2(sc) == np.rint(np.log2(sc))) if c.exact else sc in (10.0, 0.25), cid
    assert any(p[1] < 0 for c in EXACT for _, parts in c.adapters for p in parts if p is not None)


def test_branch_restatement():
    G = cases.down_groups
    assert G(1) == G(3) == G(4) == G(5) == G(8) == ["scalar"] and G(16) == ["vec"]
    assert G(17) == G(18) == ["scalar", "scalar"] and G(20) == ["vec", "scalar"] and G(32) == ["vec", "vec"]
    assert G(36) == ["vec", "vec", "scalar"] and G(60) == ["vec"] * 3 + ["scalar"] and G(63) == ["scalar"] * 4 and G(64) == ["vec"] * 4
    assert cases.c_K(8) == 10 and cases.c_K(256) == 10 and cases.c_K(320) == 11 and cases.c_K(36864) == 153
    by = {cases.case_id(c): c for c in cases.CASES}
    assert cases.up_blocks(by["exact-f16-k256-w2056-256"]) == (3, [3, 1])
    assert cases.up_blocks(by["exact-bf16-zoo-k320"]) == (2, [2, 1, 1])
    assert cases.up_blocks(by["exact-bf16-k8-w1024"]) == (1, [1])


# ---------------------------------------------------------------------------------------------------------------------------
# exact data

def _f32_orders(xs, a):
    """sum_k xs[k] a[k][j] with float32 accumulators: the kernel's shape (thread tid adds k = tid, tid + 256, ... ascending,
    then 16-lane rows, the four rows of a wave pairwise, the four waves in order) and plainly reversed"""
    K = len(xs)
    prod = (xs[:, None] * a).astype(np.float32)
    pad = np.zeros((-K % 256, a.shape[1]), np.float32)
    per_thread = np.cumsum(np.concatenate([prod, pad]).reshape(-1, 256, a.shape[1]), axis=0, dtype=np.float32)[-1]
    rows = np.cumsum(per_thread.reshape(16, 16, -1), axis=1, dtype=np.float32)[:, -1]          # (16 rows of 16 lanes)
    w = rows.reshape(4, 4, -1)
    waves = ((w[:, 0] + w[:, 1]).astype(np.float32) + (w[:, 2] + w[:, 3]).astype(np.float32)).astype(np.float32)
    kern = ((waves[0] + waves[1]).astype(np.float32) + waves[2]).astype(np.float32) + waves[3]
    return kern.astype(np.float32), np.cumsum(prod[::-1], axis=0, dtype=np.float32)[-1]


@pytest.mark.parametrize("c", EXACT, ids=cases.case_id)
def test_exact_cases_are_exact_in_float32_in_any_order(c):
    d = cases.build(c)
    T = c.logical
    for name in ("x", "y", "h", "nw"):
        v = d[name]
        if v is not None:
            v = v[np.isfinite(v)]
            assert np.array_equal(round_to(v, T), v), name                      # values of T
            if not (c.norm and name == "x") and not (c.cancel and name == "y"):
                assert np.array_equal(v, np.rint(v)), name                      # small integers
    for a in list(d["A"].values()) + list(d["B"].values()):
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 4
    if c.norm:                                                                  # +-2^e rows: the norm stages +-w exactly
        assert (np.abs(d["x"]) == np.abs(d["x"][:, :1])).all() and np.log2(np.abs(d["x"][:, 0])).tolist() == np.rint(np.log2(np.abs(d["x"][:, 0]))).tolist()
        assert cases.eps_of(c) == 0.0 and np.array_equal(d["xs"], np.sign(d["x"]) * d["nw"][None])
        ss = np.cumsum((d["x"] * d["x"]).astype(np.float32), axis=-1, dtype=np.float32)[:, -1]
        rs = np.float32(1.0) / np.sqrt(ss / np.float32(c.K), dtype=np.float32)
        assert np.array_equal(rs.astype(np.float64), 1.0 / np.abs(d["x"][:, 0]).astype(np.float64))
    s1, s2 = cases.exactness(c, d)
    print(f"{cases.case_id(c)}: sum |x A| <= {s1:.0f}, sum |t B| <= {s2:.0f} (limit {2 ** 24})")
    assert s1 < 2 ** 24 and s2 < 2 ** 24
    t64 = d["t64"]
    assert np.array_equal(np.nan_to_num(t64), np.nan_to_num(d["t_up"].astype(np.float64)))     # t is a float32, exactly
    m, r = next((m, r) for m in range(c.M) for r in range(len(c.parts)) if c.cover(m, r))
    rk = c.cover(m, r)[0]
    for got in _f32_orders(d["xs"][m], d["A"][c.rows[m], r]):
        assert np.array_equal(got.astype(np.float64), t64[m, r, :rk])
    e = cases.up_expect(c, d)
    src = d["h"] if c.resid else d["y"]
    assert np.isfinite(e["want"][e["wrote"]]).all() and np.array_equal(e["want"][~e["wrote"]], src[~e["wrote"]], equal_nan=True)
    assert np.array_equal(round_to(e["want"], T), e["want"], equal_nan=True)
    # the restated yardstick and the oracle's own LoRALinear give the same bits
    assert np.array_equal(e["want"], cases.oracle_rows(c, d), equal_nan=True)
    if c.resid:
        assert e["wrote"][:, :c.parts[0][1]].all() and not e["wrote"][:, c.parts[0][1]:].any()


def test_sixteen_bit_exact_cases_sit_on_ties():
    """per 16-bit type: elements exactly on a tie of T at T(scale z), at T(y + .) and at the residual's T(h + .)"""
    count = {}
    for c in EXACT:
        if c.logical == "float32":
            continue
        ties = cases.up_expect(c, cases.build(c))["ties"]
        print(f"{cases.case_id(c)}: ties at (term, y, h) = {ties}")
        if c.tname in ("bf16", "f16"):
            count[c.tname] = np.add(count.get(c.tname, (0, 0, 0)), ties)
            if c.resid:
                assert min(ties) >= 8, (cases.case_id(c), ties)            # one case carries all three points
    for T, n in count.items():
        assert min(n) >= 64, (T, n)
    assert set(count) == {"bf16", "f16"}
    # is_tie itself: 257 lies between the bfloat16 values 256 and 258, 2049 between the float16 values 2048 and 2050
    assert cases.is_tie(np.array([257.0, 258.0, 257.5]), "bfloat16").tolist() == [True, False, False]
    assert cases.is_tie(np.array([2049.0, -2049.0, 2050.0]), "float16").tolist() == [True, True, False]
    assert round_f64(np.array([257.0, 259.0]), "bfloat16").tolist() == [256.0, 260.0]             # ties to even


# ---------------------------------------------------------------------------------------------------------------------------
# rule data

@pytest.mark.parametrize("c", RULE, ids=cases.case_id)
def test_rule_case_near_share_and_bounds(c):
    d = cases.build(c)
    e = cases.up_expect(c, d)
    share = cases.near_share(c, d)
    print(f"NEAR {cases.case_id(c)}: {100 * share:.3f} % of {int(e['wrote'].sum())} elements (cap {100 * cases.NEAR_CAP:.0f} %)")
    assert share <= cases.NEAR_CAP
    if c.logical == "float32":
        assert share == 0 and (e["allowed"][e["wrote"]] > 0).all()
    else:
        assert (e["allowed"][~e["near"]] == 0).all() and (e["allowed"][e["near"]] > 0).all()
    # the bound on t: defined exactly where the kernel writes, positive, and the reference's own float32 orders fit in it
    b, t64 = cases.t_bound(c, d), d["t64"]
    assert np.array_equal(np.isnan(b), np.isnan(t64)) and (b[~np.isnan(b)] > 0).all()
    if not c.norm:
        m, r = next((m, r) for m in range(c.M) for r in range(len(c.parts)) if c.cover(m, r))
        rk = c.cover(m, r)[0]
        for got in _f32_orders(d["xs"][m], d["A"][c.rows[m], r]):
            err = np.abs(got.astype(np.float64) - t64[m, r, :rk])
            assert (err <= b[m, r, :rk]).all()
            assert err.max() > 0                       # (rule data do round: the bound is not vacuous)
    elif c.logical != "float32":
        flagged, xs_alt = cases.norm_alternatives(c, d)
        print(f"    norm: {int(flagged.sum())} of {flagged.size} elements within delta_K = {cases.delta_K(c.K) / cases.U:.1f} x 2^-24 of a boundary")
        assert flagged.mean() < 0.01 and (xs_alt[~flagged] == d["xs"][~flagged]).all()


def test_near_logic_on_known_values():
    r = round_f64(np.array([1.0 + 2.0 ** -8 + 1e-9, 1.25]), "bfloat16")
    gap = cases.boundary_gap(np.array([1.0 + 2.0 ** -8 + 1e-9, 1.25]), r, "bfloat16")
    assert abs(gap[0] - 1e-9) < 1e-12 and gap[1] == 2.0 ** -8
    assert cases.ulp_T(np.float32([1.0, 1.5, -3.0]), "bfloat16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert cases.ulp_T(np.float32([1.0, 2048.0]), "float16").tolist() == [2.0 ** -10, 2.0]


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity: the wrong kernels of the issue change the expected bits of an exact case

def _case(name):
    return next(c for c in EXACT if cases.case_id(c) == name)


def test_a_dropped_k_step_or_a_wave_read_twice_changes_t():
    c = _case("exact-bf16-zoo-k320")
    d = cases.build(c)
    xs, a, want = d["xs"][0], d["A"][0, 0], d["t64"][0, 0, :20]
    drop = xs.astype(np.float64).copy()
    drop[256:] = 0                                                     # the last k step of threads 0..63
    assert (drop @ a != want).mean() > 0.5
    wave = xs.astype(np.float64).copy()                                # red16[3] read in place of red16[2]
    k = np.arange(c.K) % 256
    wave[(k >= 128) & (k < 192)] = 0
    twice = wave @ a + (np.where(k >= 192, xs, 0).astype(np.float64) @ a)
    assert (twice != want).mean() > 0.5


def test_a_rank_read_too_far_changes_t():
    """the scalar loop's guard taken as j0 + j <= rk writes t[rank] -- a NaN sentinel the device test watches; and in the up-add a
    rank too many reads t[rank], which the test's own t leaves as NaN"""
    for c in EXACT:
        d = cases.build(c)
        for m in range(c.M):
            for r in range(len(c.parts)):
                p = c.cover(m, r)
                if p is not None and p[0] < 64:
                    assert np.isnan(d["t64"][m, r, p[0]]) and np.isnan(d["t_up"][m, r, p[0]])


def test_a_fused_lora_add_changes_y():
    """scale * z + y in one rounding differs from T(y + T(scale z)) on a 16-bit type -- and on plain float32 exact data cannot
    show it (everything is exact there), which is why the rule cases bound float32 and the 16-bit exact cases pin the rest"""
    c = _case("exact-bf16-zoo-k320")
    d = cases.build(c)
    e = cases.up_expect(c, d)
    fused = d["y"].copy()
    for m in range(c.M):
        for r, (r0, n) in enumerate(c.parts):
            p = c.cover(m, r)
            if p is not None:
                z = d["t64"][m, r, :p[0]] @ d["B"][c.rows[m], r].astype(np.float64)
                fused[m, r0:r0 + n] = round_f64(p[1] * z + d["y"][m, r0:r0 + n], c.logical)
    assert (fused[e["wrote"]] != e["want"][e["wrote"]]).mean() > 0.01
    # plain float32: the "cancel" case -- the fused form rounds scale z + y once, the kernel's rounds fl(scale z) first
    c = _case("exact-f32-cancel-k256")
    d = cases.build(c)
    e = cases.up_expect(c, d)
    fused = d["y"].copy()
    for m in range(c.M):
        rk, sc = c.cover(m, 0)
        z = d["t64"][m, 0, :rk] @ d["B"][c.rows[m], 0].astype(np.float64)
        p = sc * z                                                           # 14 + 24 bits: exact in float64
        assert (np.abs(z) < 2 ** 24).all() and (p.astype(np.float32).astype(np.float64) != p).mean() > 0.9
        assert (np.abs(p + d["y"][m, :200]) <= 1 / 16 + 1e-9).all()         # the sum cancels: exact in float32 (Sterbenz)
        fused[m, :200] = (p + d["y"][m, :200].astype(np.float64)).astype(np.float32)
    assert (fused[e["wrote"]] != e["want"][e["wrote"]]).mean() > 0.9


def test_the_residual_add_on_rows_without_adapter_and_grid_z_are_seen():
    c = _case("exact-bf16-resid-k256")
    d = cases.build(c)
    e = cases.up_expect(c, d)
    n = c.parts[0][1]
    bare = [m for m in range(c.M) if c.cover(m, 0) is None]
    assert len(bare) >= 4 and (e["want"][bare, :n] != d["h"][bare, :n]).mean() > 0.5        # skipping the add is seen
    c = _case("exact-bf16-zoo-k320")
    d = cases.build(c)
    e = cases.up_expect(c, d)
    r0 = c.parts[0][0]
    tail = slice(r0 + cases.UP_COLS, r0 + c.parts[0][1])                                    # what blockIdx.z = 1 writes
    rows = [m for m in range(c.M) if c.cover(m, 0) is not None]
    assert (e["want"][rows, tail] != d["y"][rows, tail]).mean() > 0.5
