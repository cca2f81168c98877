"""The 9..128-row decode GEMMs (gemm_skinny.hip's skinny_kernel, gemm_q4.hip behind its preparation pass) against the float64
oracle, launch form by launch form (-m gpu), through mi_op_gemm_skinny only.  Inputs, expectations, the rules and the case
table: tests/skinny_cases.py (what they rest on: tests/test_skinny_cases.py).

* every case with an explicit ksplit (> 0: skinny_kernel; a forced code: gemm_q4.hip); exact cases bit for bit, the others
  under their measured rule;
* outputs and residuals live in (16 MT nslab + 2) x ldo buffers filled with a NaN sentinel: rows >= M and columns >= N keep
  it.  x has exactly M rows of ldx (columns K.. hold NaN): nothing here provokes a read beyond them, the test only refrains
  from padding;
* two launches of every split case give identical bits (the last arriver adds the slices in slice order);
* on exact data every route returns the oracle's bits, hence the same bits: every ksplit in {1, 2, nchunks}; for int4 above 16
  rows the forced gemm_q4.hip plan and skinny_kernel; for dense / int4 at <= 16 rows mi_op_gemv (gemv_mfma.hip);
* the cost model's own split (ksplit = 0) equals the forced run with *ksplit_used;
* a biased int4 call above 16 rows stays on skinny_kernel: a forced gemm_q4.hip plan refuses it and leaves the output alone.

Out of scope (no way to them through mi_op_gemm_skinny; their engine-level tests keep them): the RMSNorm hand-over between
launches (sq_in / sq_out), the publish-only form and [hi | lo] matrices (kx).  The LoRA terms no longer ride in these
kernels: lora_rows.hip adds them around a plain-store launch, and tests/test_gpu_lora_rows.py checks it at its own level.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_u32, gemm_skinny, gemv, op_linear, q4_force, to_tiled  # noqa: E402

import skinny_cases as cases  # noqa: E402

SENT16, SENT32 = 0x7fc1, 0x7fc0c0c1               # NaN patterns of bfloat16 / float16 and of float32
EPI = {"store": L.EPI_STORE, "store_f32": L.EPI_STORE_F32, "resid": L.EPI_RESID, "swiglu": L.EPI_SWIGLU}
MI_ERR_UNSUPPORTED = -3
TDT = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
PARAMS = [pytest.param(c, act, id=f"{cases.case_id(c)}-{act}") for c in cases.CASES for act in c.acts]


def _weights(c, act, d):
    """-> (op_linear on the tile-major copy, keepalive); a linear bias as float32 [rows]"""
    wdt = cases.wdt_of(c, act)
    kind = cases.weight_kind(c.kind, wdt)
    if c.kind == "dense":
        wd = dev(d["w"], wdt)
        ol, keep = op_linear(kind, c.wrows, c.K, wd), [wd]
    else:
        packed, scales, biases = d["q"]
        pd, sd, bd = dev_u32(packed), dev(scales, wdt), dev(biases, wdt)
        ol, keep = op_linear(kind, c.wrows, c.K, pd, sd, bd), [pd, sd, bd]
    assert to_tiled(ol, keep)
    if c.bias:
        b = torch.from_numpy(np.ascontiguousarray(d["b"], dtype=np.float32)).cuda()
        keep.append(b)
        ol.bias = b.data_ptr()
    return ol, keep


def _x(c, act, xl):
    """One launch's activations: exactly M rows of ldx elements; the columns past K hold NaN."""
    xdt = "float32" if c.x32 else act
    ldx = c.K + 8 if c.strides else c.K
    x = torch.full((c.M, ldx), float("nan"), dtype=TDT[xdt], device="cuda")
    x[:, :c.K] = dev(xl, xdt)
    return x, ldx


class _Out:
    """A (rows_padded + 2) x ldo buffer of sentinels that holds the M x N result (for a residual epilogue: h going in)."""

    def __init__(self, c, act, rows_padded, h=None):
        self.f32 = c.epi == "store_f32" or c.x32
        self.M, self.N, self.ldo = c.M, c.N, (c.N + 3 if c.strides else c.N)
        self.dt = torch.float32 if self.f32 else TDT[act]
        self.raw = torch.full((rows_padded + 2, self.ldo), SENT32 if self.f32 else SENT16,
                              dtype=torch.int32 if self.f32 else torch.int16, device="cuda")
        if h is not None:
            hd = dev(h, "float32" if c.x32 else act)
            self.raw[:self.M, :self.N] = hd.view(torch.int32 if c.x32 else torch.int16)

    def result(self):
        return self.raw[:self.M, :self.N].contiguous().view(self.dt).float().cpu().numpy()

    def bits(self):
        return self.raw[:self.M, :self.N].cpu().numpy()

    def assert_padding_untouched(self):
        sent = SENT32 if self.f32 else SENT16
        assert bool((self.raw[self.M:] == sent).all()), "rows >= M were written"
        assert bool((self.raw[:, self.N:] == sent).all()), "columns N..ldo-1 were written"


def _launch(c, act, ol, d, xl, *, ksplit=None, check=True):
    """One call of case c on launch xl of its activations, with the case's own ksplit / forced plan or the given one
    -> (_Out, ksplit used); check False: -> (_Out, return code)."""
    forced = c.q4plan is not None and ksplit is None
    plan = c.plan(ksplit)
    x, ldx = _x(c, act, xl)
    out = _Out(c, act, plan.rows_padded, d["h"] if c.epi == "resid" else None)
    nw = dev(d["nw"], "float32" if c.x32 else act) if c.pro else None
    kw = dict(epi=EPI[c.epi], ldo=out.ldo, ldx=ldx, pair_offset=c.N if c.swiglu else 0, norm_w=nw, eps=cases.EPS,
              rnd=L.RND_BF16 if c.rnd else L.RND_NONE, ksplit=q4_force(*c.q4plan) if forced else (c.ksplit if ksplit is None else ksplit))
    kw["resid" if c.epi == "resid" else "out"] = out.raw
    res = gemm_skinny(ol, x, c.M, "float32" if c.x32 else act, check=check, **kw)
    torch.cuda.synchronize()
    if not check:
        return out, res
    out.assert_padding_untouched()
    return out, res[0]


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} elements differ; first (launch, m, n): {bad[:6].tolist()}"


def _run(c, act, ol, d, *, ksplit=None, twice=False):
    """every launch of the case's activations -> (launches, M, N) float32; twice: each launch a second time, same bits"""
    got, used = [], None
    for xl in d["x"]:
        out, used = _launch(c, act, ol, d, xl, ksplit=ksplit)
        if twice:
            again, _ = _launch(c, act, ol, d, xl, ksplit=ksplit)
            assert np.array_equal(out.bits(), again.bits()), "two launches of a split case differ"
        got.append(out.result())
    return np.stack(got), used


@pytest.mark.parametrize("c,act", PARAMS)
def test_skinny_case(c, act):
    d = cases.build(c, act)
    ol, keep = _weights(c, act, d)
    plan, want, odt = c.plan(), d["want"], cases.odt_of(c, act)
    got, used = _run(c, act, ol, d, twice=plan.ksplit > 1)
    # the route: *ksplit_used echoes a forced split; a forced gemm_q4.hip plan reports its own K slices over workgroups
    if c.q4plan is not None:
        assert plan.kernel == "q4" and used == plan.ksplit
    elif c.ksplit > 0:
        assert plan.kernel == "skinny" and used == c.ksplit
    else:                                           # the biased int4 call on a matrix gemm_q4.hip would take: skinny_kernel's one chunk
        assert c.bias and not c.routed_to_q4() and plan.nchunks == 1 and used == 1
    if c.exact:
        assert np.array_equal(got, want), _mismatch(got, want)
    elif c.data == "hot3g":
        err = np.abs(got.astype(np.float64) - d["x"].astype(np.float64) @ d["w"].astype(np.float64).T)
        bound = 2.0 ** -22 * np.abs(want.astype(np.float64))
        print("max err / |want| in ulps of 2^-24:", float(np.max(err[want != 0] / np.abs(want[want != 0])) * 2.0 ** 24))
        assert np.isfinite(got).all() and np.all(err <= bound), _mismatch(err <= bound, np.ones_like(err, bool))
    elif odt == "float32":
        cases.assert_f32_rule(got, want, cases.sum_abs_xw(c, act, d), cases.case_id(c))
    else:
        cases.assert_rule(got, want, odt, cases.case_id(c))
    if not c.exact or c.data != "int":
        return
    # ---- agreement across kernels on exact data: each returns the oracle's bits
    if c.q4plan is not None:                        # the same call on skinny_kernel
        other, _ = _run(c, act, ol, d, ksplit=2)
        assert np.array_equal(other, want), "skinny_kernel: " + _mismatch(other, want)
        return
    if c.ksplit > 0:
        for ks in sorted({1, 2, plan.nchunks} - {plan.ksplit}):
            if ks <= plan.nchunks:
                other, _ = _run(c, act, ol, d, ksplit=ks, twice=ks > 1)
                assert np.array_equal(other, want), f"ksplit {ks}: " + _mismatch(other, want)
    if c.M <= 16 and c.kind in ("dense", "q4") and not c.x32 and not c.bias:      # gemv_mfma.hip on the same rows
        x, ldx = _x(c, act, d["x"][0])
        out = _Out(c, act, 16, d["h"] if c.epi == "resid" else None)
        kw = dict(epi=EPI[c.epi], ldo=out.ldo, ldx=ldx, pair_offset=c.N if c.swiglu else 0)
        kw["resid" if c.epi == "resid" else "out"] = out.raw
        assert gemv(ol, x, c.M, act, **kw), "mi_op_gemv did not take gemv_mfma.hip"
        torch.cuda.synchronize()
        out.assert_padding_untouched()
        assert np.array_equal(out.result()[None], want), "gemv_mfma: " + _mismatch(out.result()[None], want)


@pytest.mark.parametrize("c", cases.COST_MODEL, ids=cases.case_id)
@pytest.mark.parametrize("act", cases.ACTS)
def test_cost_model_split_equals_the_forced_run(c, act):
    d = cases.build(c, act)
    ol, keep = _weights(c, act, d)
    got, used = _run(c, act, ol, d, ksplit=0)
    assert 1 <= used <= min(16, c.plan().nchunks)
    forced, echoed = _run(c, act, ol, d, ksplit=used, twice=used > 1)
    assert echoed == used
    assert np.array_equal(got, forced), _mismatch(got, forced)
    assert np.array_equal(got, d["want"]), _mismatch(got, d["want"])


@pytest.mark.parametrize("act", cases.ACTS)
def test_biased_int4_call_is_refused_by_a_forced_q4_plan(act):
    c = next(c for c in cases.CASES if c.kind == "q4" and c.bias and c.M > 16 and c.epi == "store" and c.ksplit > 0)
    d = cases.build(c, act)
    ol, keep = _weights(c, act, d)
    forced = cases.Case(c.data, c.kind, c.epi, c.M, c.tiles, c.K, q4plan=(2, 2, 2, 1, 2), bias=True)
    assert forced.plan() is not None and not forced.routed_to_q4()
    out, rc = _launch(forced, act, ol, d, d["x"][0], check=False)
    assert rc == MI_ERR_UNSUPPORTED, rc
    assert bool((out.raw == SENT16).all()), "a refused call wrote its output"
