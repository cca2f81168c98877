"""lora_down_by_row_kernel and lora_up_add_by_row_kernel (csrc/lora_rows.hip) on their own, through mi_op_lora_rows only
(-m gpu).  Inputs, expectations, bounds and the case table: tests/lora_rows_cases.py (what they rest on, and each rule case's
near share: tests/test_lora_rows_cases.py).

* down stage: t bit for bit on exact cases, within the derived bound on rule cases; the NaN pattern the buffer is filled with
  stays in rows without a usable adapter, in parts the row's adapter does not cover and at j >= rank; x has exactly M rows of
  ldx > K with NaN behind K;
* up-add stage, from the test's own t: y bit for bit (exact cases; rule cases: every element that is near no rounding boundary)
  or within the near allowance; columns outside every part, rows beyond M and rows without a usable adapter keep their bits;
* the residual form: h as expected on every row, y bit-identical to what went in, h behind column n untouched;
* both stages in one call give the bits of the two single-stage calls; the same call twice gives the same bits;
* every refusal returns its code, sets mi_last_error() and leaves sentinel-filled t, y and resid alone; K = 36864 runs (a
  case of the table), K = 36868 is refused;
* composed with the base linear (mi_op_gemv, MI_EPI_STORE, the same x and norm) the three launches give, row by row, the bits
  of oracle.ref_model.Linear carrying that row's lora_a / lora_b / lora_scale behind ref_model.rms_norm.

Each rule case prints its largest error as a fraction of its bound (lines "FRACTION ...") before anything is asserted.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_model  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import MIDT, TDT, dev, dev_i32, gemv, lora_rows, op_linear, to_tiled  # noqa: E402

import lora_rows_cases as cases  # noqa: E402

SENT16, SENT32 = 0x7fc1, 0x7fc0c0c1               # NaN patterns of bfloat16 / float16 and of float32
DOWN, UP = L.LORA_STAGE_DOWN, L.LORA_STAGE_UP
INVALID, UNSUPPORTED = -1, -3
PARAMS = [pytest.param(c, id=cases.case_id(c)) for c in cases.CASES]


def _bits(values, storage):
    """float32 array (NaN = the sentinel stays) -> the bit patterns of its storage type, as int64"""
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
    if storage == "float32":
        b = v.view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF
        return np.where(np.isnan(values), SENT32, b)
    b = v.to(TDT[storage]).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    return np.where(np.isnan(values), SENT16, b)


class _Buf:
    """A (rows + 2) x ld buffer of sentinels holding `values` (NaN = sentinel) in its first rows, in the storage type."""

    def __init__(self, values, storage):
        self.storage, self.rows = storage, values.shape[0]
        self.idt = torch.int32 if storage == "float32" else torch.int16
        want = np.full((self.rows + 2, values.shape[1]), SENT32 if storage == "float32" else SENT16, np.int64)
        want[:self.rows] = _bits(values, storage)
        self.before = want
        self.raw = torch.from_numpy(want.astype(np.uint32).view(np.int32) if storage == "float32"
                                    else want.astype(np.uint16).view(np.int16)).cuda().contiguous()

    def bits(self):
        return self.raw.cpu().numpy().astype(np.int64) & (0xFFFFFFFF if self.storage == "float32" else 0xFFFF)

    def values(self):
        return self.raw[:self.rows].contiguous().view(TDT[self.storage]).float().cpu().numpy().astype(np.float64)


class _Dev:
    """the inputs of a case on the device"""

    def __init__(self, c):
        self.c, self.d = c, cases.build(c)
        self.storage, self.rnd, _ = cases.TYPES[c.tname]
        d = self.d
        self.x = torch.full((c.M, c.ldx), float("nan"), dtype=TDT[self.storage], device="cuda")      # exactly M rows, NaN behind K
        self.x[:, :c.K] = dev(d["x"], self.storage)
        self.nw = dev(d["nw"], self.storage) if c.norm else None
        self.rows = dev_i32(np.asarray(c.rows))
        self.table = {}
        for (col, r), a in d["A"].items():
            rank, scale = dict(c.adapters)[col][r]
            self.table[r, col] = (dev(a), dev(d["B"][col, r]), rank, scale)

    def call(self, stages, t, y=None, h=None, check=True):
        c = self.c
        return lora_rows(stages=stages, M=c.M, act=MIDT[self.storage], rnd=self.rnd, row_adapter=self.rows, parts=c.parts,
                         table=self.table, t=t, x=self.x, ldx=c.ldx, K=c.K, pro=L.PRO_NORM if c.norm else L.PRO_NONE,
                         norm_w=self.nw, eps=cases.eps_of(c), y=None if y is None else y.raw, ldy=c.ldy,
                         resid=None if h is None else h.raw, ldr=c.ldr, check=check)

    def t_buffer(self, values=None):
        """[M + 2][192] float32: the sentinel everywhere, or `values` (NaN = sentinel) in the first M rows"""
        v = np.full((self.c.M, cases.T_LD), np.nan, np.float32) if values is None else values.reshape(self.c.M, cases.T_LD)
        return _Buf(v, "float32")

    def outputs(self):
        return _Buf(self.d["y"], self.storage), (_Buf(self.d["h"], self.storage) if self.c.resid else None)


def _differ(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} elements differ; first (m, column): {bad[:6].tolist()}"


def _check_t(c, d, buf):
    """the down stage's t against the expectation -> the largest error as a fraction of its bound (rule cases)"""
    got_bits = buf.bits()
    t64 = d["t64"].reshape(c.M, cases.T_LD)
    if c.exact:
        want = np.full(got_bits.shape, SENT32, np.int64)
        want[:c.M] = _bits(d["t_up"].reshape(c.M, cases.T_LD), "float32")
        assert np.array_equal(got_bits, want), _differ(got_bits, want)
        return 0.0
    written = np.zeros(got_bits.shape, bool)
    written[:c.M] = ~np.isnan(t64)
    assert (got_bits[~written] == SENT32).all(), "t was written where no adapter covers it"
    got = buf.values()
    bound = cases.t_bound(c, d).reshape(c.M, cases.T_LD)
    w = written[:c.M]
    assert np.isfinite(got[w]).all()
    frac = float((np.abs(got[w] - t64[w]) / bound[w]).max())
    print(f"FRACTION {cases.case_id(c)} down: largest |t - t64| / bound = {frac:.4f} (c_K = {cases.c_K(c.K)})")
    assert frac <= 1.0, frac
    return frac


def _check_out(c, d, out, e, storage, what):
    """the up-add's output buffer (y, or h with a residual) against up_expect's yardstick"""
    got_bits = out.bits()
    want_bits = out.before.copy()
    want_bits[:c.M] = _bits(e["want"], storage)
    wrote = np.zeros(got_bits.shape, bool)
    wrote[:c.M] = e["wrote"]
    assert np.array_equal(got_bits[~wrote], out.before[~wrote]), what + ": written outside the parts / rows: " + _differ(
        np.where(wrote, 0, got_bits), np.where(wrote, 0, out.before))
    if c.exact:
        assert np.array_equal(got_bits, want_bits), what + ": " + _differ(got_bits, want_bits)
        return
    got = out.values()
    w = e["wrote"]
    assert np.isfinite(got[w]).all()
    err = np.abs(got - e["want64"])
    if c.logical == "float32":
        frac = float((err[w] / e["allowed"][w]).max())
        print(f"FRACTION {cases.case_id(c)} {what}: largest error / bound = {frac:.4f}")
        assert frac <= 1.0, frac
        return
    far = w & ~e["near"]
    differ = got_bits[:c.M] != want_bits[:c.M]
    n_near = int(e["near"].sum())
    worst = float((err[e["near"]] / e["allowed"][e["near"]]).max()) if n_near else 0.0
    print(f"FRACTION {cases.case_id(c)} {what}: {int((differ & far).sum())} of {int(far.sum())} elements off the boundaries differ; "
          f"{int((differ & e['near']).sum())} of {n_near} near ones differ, largest near error / allowance = {worst:.4f}")
    assert not (differ & far).any(), what + ": " + _differ(np.where(far, got_bits[:c.M], 0), np.where(far, want_bits[:c.M], 0))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("c", PARAMS)
def test_down_stage(c):
    dv = _Dev(c)
    t = dv.t_buffer()
    dv.call(DOWN, t.raw)
    _check_t(c, dv.d, t)
    again = dv.t_buffer()
    dv.call(DOWN, again.raw)
    assert np.array_equal(t.bits(), again.bits())                  # the same call twice


@pytest.mark.parametrize("c", PARAMS)
def test_up_add_stage_from_the_tests_own_t(c):
    dv = _Dev(c)
    d = dv.d
    e = cases.up_expect(c, d)
    runs = []
    for _ in range(2):
        t = dv.t_buffer(d["t_up"])                                 # (NaN at j >= rank and wherever nothing covers)
        y, h = dv.outputs()
        dv.call(UP, t.raw, y, h)
        assert np.array_equal(t.bits(), t.before)                  # t is read only
        if c.resid:
            assert np.array_equal(y.bits(), y.before), "y changed under a residual: " + _differ(y.bits(), y.before)
            n = c.parts[0][1]
            assert np.array_equal(h.bits()[:, n:], h.before[:, n:])
        runs.append((h if c.resid else y).bits())
    _check_out(c, d, h if c.resid else y, e, dv.storage, "h" if c.resid else "y")
    assert np.array_equal(runs[0], runs[1])                        # the same call twice
    bare = [m for m in range(c.M) if all(c.cover(m, r) is None for r in range(len(c.parts)))]
    if not c.resid:
        assert np.array_equal(y.bits()[bare], y.before[bare])      # rows without a usable adapter keep their y bits


@pytest.mark.parametrize("c", PARAMS)
def test_both_stages_in_one_call(c):
    dv = _Dev(c)
    t1 = dv.t_buffer()
    dv.call(DOWN, t1.raw)
    y1, h1 = dv.outputs()
    dv.call(UP, t1.raw, y1, h1)
    t2 = dv.t_buffer()
    y2, h2 = dv.outputs()
    dv.call(DOWN | UP, t2.raw, y2, h2)
    assert np.array_equal(t1.bits(), t2.bits())
    assert np.array_equal(y1.bits(), y2.bits())
    if c.resid:
        assert np.array_equal(h1.bits(), h2.bits())
    if c.exact:                                                    # ... and on exact data they are the expectation's
        _check_out(c, dv.d, h2 if c.resid else y2, cases.up_expect(c, dv.d), dv.storage, "h" if c.resid else "y")


def test_refusals_touch_nothing():
    for name, resid in (("exact-bf16-small-k256", False), ("exact-bf16-resid-k256", True)):
        c = next(c for c in cases.CASES if cases.case_id(c) == name)
        dv = _Dev(c)
        t = dv.t_buffer()
        y, h = dv.outputs()
        base = dict(stages=DOWN | UP, M=c.M, act=MIDT["bfloat16"], rnd=0, row_adapter=dv.rows, parts=c.parts, table=dv.table, t=t.raw,
                    x=dv.x, ldx=c.ldx, K=c.K, pro=L.PRO_NONE, norm_w=None, eps=0.0, y=y.raw, ldy=c.ldy,
                    resid=h.raw if resid else None, ldr=c.ldr, check=False)
        (r0, col), (a, b, rank, scale) = next(iter(dv.table.items()))

        def entry(*v):
            return {**dv.table, (r0, col): v}

        n0 = c.parts[0][1]
        bad = [
            (INVALID, "null x", dict(x=None)), (INVALID, "null y", dict(y=None)), (INVALID, "null t", dict(t=None)),
            (INVALID, "null row_adapter", dict(row_adapter=None)),
            (INVALID, "M = 0", dict(M=0)), (INVALID, "no parts", dict(n_parts=0)), (INVALID, "four parts", dict(n_parts=4)),
            (INVALID, "stages 0", dict(stages=0)), (INVALID, "stages 4", dict(stages=4)),
            (INVALID, "act", dict(act=7)), (INVALID, "act u32", dict(act=L.MI_U32)), (INVALID, "rnd", dict(rnd=5)),
            (INVALID, "pro", dict(pro=2)), (INVALID, "norm without norm_w", dict(pro=L.PRO_NORM)),
            (INVALID, "ldx < K", dict(ldx=c.K - 1)), (UNSUPPORTED, "K above the limit", dict(K=36868, ldx=36868 + 8)),
            (INVALID, "part beyond ldy", dict(ldy=c.parts[-1][0] + c.parts[-1][1] - 1)),
            (INVALID, "part at a negative column", dict(parts=((-1, n0),) + tuple(c.parts[1:]))),
            (INVALID, "empty part", dict(parts=((0, 0),) + tuple(c.parts[1:]))),
            (INVALID, "only A", dict(table=entry(a, None, rank, scale))), (INVALID, "only B", dict(table=entry(None, b, rank, scale))),
            (INVALID, "rank 0", dict(table=entry(a, b, 0, scale))), (INVALID, "rank 65", dict(table=entry(a, b, 65, scale))),
            (INVALID, "A misaligned", dict(table=entry(a.data_ptr() + 4, b, rank, scale))),
            (INVALID, "B misaligned", dict(table=entry(a, b.data_ptr() + 8, rank, scale))),
            (INVALID, "x misaligned", dict(x=dv.x.data_ptr() + 1)), (INVALID, "y misaligned", dict(y=y.raw.data_ptr() + 1)),
        ]
        if resid:
            bad += [(INVALID, "residual with two parts", dict(parts=((0, 100), (100, 100)))),
                    (INVALID, "residual at row0 != 0", dict(parts=((1, n0),))), (INVALID, "ldr < n", dict(ldr=n0 - 1)),
                    (INVALID, "resid misaligned", dict(resid=h.raw.data_ptr() + 1))]
        for want, what, change in bad:
            rc = lora_rows(**{**base, **change})
            assert rc == want, (what, rc)
            assert L.lib().mi_last_error(), what
        # every refusal left the sentinel-filled buffers alone
        assert np.array_equal(t.bits(), t.before) and np.array_equal(y.bits(), y.before)
        assert not resid or np.array_equal(h.bits(), h.before)
        # a stage does not ask for what it does not read; a row_adapter outside the table is not refused (the zoo cases)
        assert lora_rows(**{**base, "stages": DOWN, "y": None, "resid": None}) == 0
        assert lora_rows(**{**base, "stages": UP, "x": None, "K": 0, "ldx": 0}) == 0


def test_k_limit():
    """K = 36864 runs (exact-bf16-k36864 and rule-bf16-norm-k36864 of the table); four more columns are refused, nothing touched"""
    assert any(c.K == cases.K_MAX for c in cases.CASES)
    K = cases.K_MAX + 4
    x = torch.zeros((1, K), dtype=torch.bfloat16, device="cuda")
    a, b = torch.zeros((K, 4), dtype=torch.float32, device="cuda"), torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    t = _Buf(np.full((1, cases.T_LD), np.nan, np.float32), "float32")
    y = _Buf(np.full((1, 8), np.nan, np.float32), "bfloat16")
    rc = lora_rows(stages=DOWN | UP, M=1, act=MIDT["bfloat16"], rnd=0, row_adapter=dev_i32(np.zeros(1)), parts=((0, 8),),
                   table={(0, 0): (a, b, 4, 1.0)}, t=t.raw, x=x, ldx=K, K=K, y=y.raw, ldy=8, check=False)
    assert rc == UNSUPPORTED and b"36864" in L.lib().mi_last_error()
    assert np.array_equal(t.bits(), t.before) and np.array_equal(y.bits(), y.before)


@pytest.mark.parametrize("tname", ["bf16", "f16", "f32"])
def test_composed_with_the_base_linear_against_the_oracle(tname):
    """down, mi_op_gemv (MI_EPI_STORE, the same x and norm), up-add: row by row the bits of ref_model.Linear with that row's
    lora_a / lora_b / lora_scale behind ref_model.rms_norm -- exact data, the exact norm, M = 3 rows on three adapters"""
    N, K = 64, 256
    c = cases.Case("composed", "exact", tname, K, ((0, N),), N, (0, 7, cases.ENGINE_COL),
                   ((0, ((20, 0.5),)), (7, ((7, -2.0),)), (cases.ENGINE_COL, ((64, 0.25),))), norm=True)
    dv = _Dev(c)
    d, T = dv.d, c.logical
    wdt = "bfloat16" if tname == "f32" else dv.storage
    w = np.random.default_rng(K).integers(-4, 5, (N, K)).astype(np.float32)
    wd = dev(w, wdt)
    keep = [wd]
    ol = op_linear("bf16" if wdt == "bfloat16" else "f16", N, K, wd)
    assert to_tiled(ol, keep)
    t = dv.t_buffer()
    y = _Buf(np.full((c.M, N), np.nan, np.float32), dv.storage)
    dv.call(DOWN, t.raw)
    gemv(ol, dv.x, c.M, dv.storage, pro=L.PRO_NORM, norm_w=dv.nw, eps=0.0, epi=L.EPI_STORE, out=y.raw, ldo=N, ldx=c.ldx)
    dv.call(UP, t.raw, y)
    xs, _ = ref_model.rms_norm(d["x"], T, d["nw"], T, 0.0)
    want = np.empty((c.M, N), np.float32)
    for m in range(c.M):
        rank, scale = c.cover(m, 0)
        lin = ref_model.Linear(wdt, weight=w, lora_a=d["A"][c.rows[m], 0], lora_b=d["B"][c.rows[m], 0], lora_scale=scale)
        want[m] = lin(xs[m][None], T)[0][0]
    got, want_bits = y.bits()[:c.M], _bits(want, dv.storage)
    assert np.array_equal(got, want_bits), _differ(got, want_bits)
    assert (y.bits()[c.M:] == (SENT32 if dv.storage == "float32" else SENT16)).all()
