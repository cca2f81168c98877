"""The decode GEMV on 16-bit activations (gemv_mfma.hip / gemv_phase.h) against the float64 oracle, launch form by launch form
(-m gpu).  Inputs, expectations, the rule and the case table: tests/gemv16_cases.py (what they rest on: test_gemv16_cases.py).

* every case through mi_op_gemv (the row-interleaved gate|up copy: mi_op_gemv_gu8), behind mi_op_gemv_uses_mfma == 1;
  exact cases bit for bit, the others under the rule;
* outputs and residuals live in 16-row x ldo buffers filled with a sentinel: rows M..15 and columns N..ldo-1 keep it.  x has
  exactly M rows of ldx (columns K.. hold NaN): nothing here provokes a read beyond them, the test only refrains from padding;
* mi_op_gemv_gu8 == mi_op_gemv with MI_EPI_SWIGLU, bit for bit (both forms give wave w the k-blocks = w mod 8 in ascending
  order and add the waves in the same order);
* the row-major gemv_v1 path returns the same bits on the exact cases (both are exact), one case per K class;
* the refusals of mi_op_gemv_gu8 leave the output untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_u32, gemv, gemv_args, gemv_gu8, op_linear, to_tiled  # noqa: E402

import gemv16_cases as cases  # noqa: E402

SENT16, SENT32 = 0x7fc1, 0x7fc0c0c1               # NaN patterns of bfloat16 / float16 and of float32
EPI = {"store": L.EPI_STORE, "store_f32": L.EPI_STORE_F32, "resid": L.EPI_RESID, "swiglu": L.EPI_SWIGLU, "gu8": L.EPI_SWIGLU}
MI_ERR_UNSUPPORTED = -3
TDT = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _weights(c, act, d, tiled=True):
    """-> (op_linear, keepalive).  tiled=False keeps the checkpoint's row-major layout (the gemv_v1 path)."""
    kind = cases.weight_kind(c.kind, act)
    if c.kind == "dense":
        wd = dev(d["w"], act)
        ol, keep = op_linear(kind, d["rows"], c.K, wd), [wd]
    else:
        packed, scales, biases = d["q"]
        pd, sd, bd = dev_u32(packed), dev(scales, act), dev(biases, act)
        ol, keep = op_linear(kind, d["rows"], c.K, pd, sd, bd), [pd, sd, bd]
    if tiled:
        assert to_tiled(ol, keep)
    return ol, keep


def _x(c, act, xl):
    """One launch's activations: exactly M rows of ldx elements; the columns past K hold NaN."""
    ldx = c.K + 8 if c.strides else c.K
    x = torch.full((c.M, ldx), float("nan"), dtype=TDT[act], device="cuda")
    x[:, :c.K] = dev(xl, act)
    return x, ldx


class _Out:
    """A 16 x ldo buffer of sentinels that holds the M x N result (for a residual epilogue: h going in)."""

    def __init__(self, c, act, N, h=None):
        self.f32 = c.epi == "store_f32"
        self.M, self.N, self.ldo = c.M, N, (N + 3 if c.strides else N)
        self.dt = torch.float32 if self.f32 else TDT[act]
        self.raw = torch.full((16, self.ldo), SENT32 if self.f32 else SENT16, dtype=torch.int32 if self.f32 else torch.int16,
                              device="cuda")
        if h is not None:
            self.raw[:self.M, :N] = dev(h, act).view(torch.int16)

    def result(self):
        return self.raw[:self.M, :self.N].contiguous().view(self.dt)

    def assert_padding_untouched(self):
        sent = SENT32 if self.f32 else SENT16
        assert bool((self.raw[self.M:] == sent).all()), "rows M..15 were written"
        assert bool((self.raw[:, self.N:] == sent).all()), "columns N..ldo-1 were written"


def _launch(c, act, ol, d, xl, *, gu8=None, force_generic=0):
    """One call of case c on launch xl of its activations -> _Out.  gu8: run mi_op_gemv_gu8 (default: the case says)."""
    N = d["N"]
    gu8 = (c.epi == "gu8") if gu8 is None else gu8
    x, ldx = _x(c, act, xl)
    out = _Out(c, act, N, d["h"] if c.epi == "resid" else None)
    nw = dev(d["nw"], act) if c.pro else None
    kw = dict(pro=L.PRO_NORM if c.pro else L.PRO_NONE, norm_w=nw, eps=cases.EPS, epi=EPI[c.epi], ldo=out.ldo, ldx=ldx,
              pair_offset=N if c.epi in ("swiglu", "gu8") else 0)
    kw["resid" if c.epi == "resid" else "out"] = out.raw
    if gu8:
        a = gemv_args(x, c.M, act, **kw)
        assert L.lib().mi_op_gemv_uses_mfma(C.byref(ol), C.byref(a)) == 1
        gemv_gu8(ol, a)
    else:
        used = gemv(ol, x, c.M, act, force_generic=force_generic, **kw)
        assert used == (not force_generic), "the call did not take the path under test"
    out.assert_padding_untouched()
    return out


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} elements differ; first (launch, m, n): {bad[:6].tolist()}"


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_gemv16_case(c, act):
    d = cases.build(c, act, _cus())
    ol, keep = _weights(c, act, d)
    got = np.stack([_launch(c, act, ol, d, xl).result().float().cpu().numpy() for xl in d["x"]])
    if c.exact:
        assert np.array_equal(got, d["want"]), _mismatch(got, d["want"])
    else:
        cases.assert_rule(got, d["want"], act, cases.case_id(c))


PAIRED = [c for c in cases.CASES + cases.PAIRED_EXTRA if c.kind == "dense" and c.epi == "swiglu"]


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("c", PAIRED, ids=cases.case_id)
def test_gu8_equals_paired_tile_swiglu(c, act):
    d = cases.build(c, act, _cus())
    ol, keep = _weights(c, act, d)
    paired = _launch(c, act, ol, d, d["x"][0]).result()
    gu8 = _launch(c, act, ol, d, d["x"][0], gu8=True).result()
    assert bool(torch.isfinite(paired.float()).all())
    assert torch.equal(paired.view(torch.int16), gu8.view(torch.int16)), \
        _mismatch(gu8.float().cpu().numpy(), paired.float().cpu().numpy())


def _k_class_representatives():
    """Exact cases of at most 8 rows, the narrowest one per (kind, K)."""
    best = {}
    for c in cases.CASES:
        if c.exact and c.data == "int" and c.M <= 8 and c.epi in ("store", "store_f32", "resid"):
            key = (c.kind, c.K)
            if key not in best or c.ntiles(256) < best[key].ntiles(256):
                best[key] = c
    return list(best.values())


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("c", _k_class_representatives(), ids=cases.case_id)
def test_row_major_gemv_v1_returns_the_same_bits(c, act):
    d = cases.build(c, act, _cus())
    ol_t, keep_t = _weights(c, act, d)
    ol_r, keep_r = _weights(c, act, d, tiled=False)
    tiled = _launch(c, act, ol_t, d, d["x"][0]).result().float().cpu().numpy()
    generic = _launch(c, act, ol_r, d, d["x"][0], force_generic=1).result().float().cpu().numpy()
    assert np.array_equal(generic, d["want"][0]), _mismatch(generic, d["want"][0])
    assert np.array_equal(tiled, generic)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals of mi_op_gemv_gu8

def _refusal_setup(act="bfloat16", I=48, K=256, M=4):
    rng = np.random.default_rng(3)
    w = rng.integers(-4, 5, (2 * I, K)).astype(np.float32)
    wd = dev(w, act)
    ol, keep = op_linear(cases.weight_kind("dense", act), 2 * I, K, wd), [wd]
    assert to_tiled(ol, keep)
    x = dev(rng.integers(-3, 4, (16, K + 8)).astype(np.float32), act)
    out = torch.full((16, I), SENT16, dtype=torch.int16, device="cuda")
    a = gemv_args(x, M, act, epi=L.EPI_SWIGLU, out=out, ldo=I, pair_offset=I, ldx=K + 8)
    return ol, a, out, keep + [x]


def _refused(ol, a, out):
    rc = gemv_gu8(ol, a, check=False)
    torch.cuda.synchronize()
    assert rc == MI_ERR_UNSUPPORTED, rc
    assert bool((out == SENT16).all()), "a refused call wrote its output"


def test_gu8_takes_the_call_the_refusals_start_from():
    ol, a, out, keep = _refusal_setup()
    assert gemv_gu8(ol, a, check=False) == 0
    assert not bool((out[:4] == SENT16).any()) and bool((out[4:] == SENT16).all())


@pytest.mark.parametrize("what", ["bias", "quantised", "row-major", "act", "rnd", "M=0", "M=17", "pair%16", "N!=2I", "ldx%8", "K%32",
                                  "epi"])
def test_gu8_refusals(what):
    ol, a, out, keep = _refusal_setup()
    if what == "bias":
        b = torch.zeros(ol.N, dtype=torch.float32, device="cuda")
        keep.append(b)
        ol.bias = b.data_ptr()
    elif what == "quantised":
        packed, scales, biases = cases.exact_q4(np.random.default_rng(4), ol.N, ol.K)
        pd, sd, bd = dev_u32(packed), dev(scales, "bfloat16"), dev(biases, "bfloat16")
        keep += [pd, sd, bd]
        ol = op_linear("q4_bf16", ol.N, ol.K, pd, sd, bd)
        assert to_tiled(ol, keep)
    elif what == "row-major":
        wd = torch.zeros((ol.N, ol.K), dtype=torch.bfloat16, device="cuda")
        keep.append(wd)
        ol = op_linear("bf16", ol.N, ol.K, wd)
    elif what == "act":
        a.act = L.MI_F16
    elif what == "rnd":
        a.rnd = L.RND_BF16
    elif what == "M=0":
        a.M = 0
    elif what == "M=17":
        a.M = 17
    elif what == "pair%16":                        # 2 x 24 rows: N == 2 x pair_offset holds, the tile condition does not
        ol.N, a.pair_offset = 48, 24
    elif what == "N!=2I":
        a.pair_offset = 32
    elif what == "ldx%8":
        a.ldx = ol.K + 4
    elif what == "K%32":                           # (refused in front of any access: the buffer is that of K = 256)
        ol.K = 48
    elif what == "epi":
        a.epi = L.EPI_STORE
    _refused(ol, a, out)
