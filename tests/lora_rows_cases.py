"""Inputs, expectations, bounds and the case table of the kernel-level tests of the by-row LoRA kernels (csrc/lora_rows.hip:
lora_down_by_row_kernel, lora_up_add_by_row_kernel): tests/test_gpu_lora_rows.py runs them on the device through
mi_op_lora_rows, tests/test_lora_rows_cases.py checks without one what needs none (every branch tag is reached, the exact
cases are exact on the reference alone and carry ties, the rule cases' near sets stay under their cap).  NumPy and the oracle
only, in the shape of tests/skinny_cases.py.

What the kernels compute (restated from the code).  Row m names table column ad = row_adapter[m]; a value outside
[0, MI_MAX_ADAPTERS] is "no adapter".  Part r of column ad is (A [K][rank], B [rank][n_r], rank, scale) or null.
  down    t[m][r][j] = sum_k xs[m][k] A[k][j], j < rank, for every covered (m, r); xs = x, or behind MI_PRO_NORM
          xs = T(T(x rs) w) with rs = 1 / sqrt(sum(x^2) / K + eps) in float32.  Nothing else of t is written.
  up-add  y[m][row0_r + c] = T(y + T(scale z)), z = sum_j t[m][r][j] B[j][c], for every covered (m, r); nothing else of y is
          written.  With a residual (one part): h[m][c] = T(h + y') for EVERY row (y' = y where the row is not covered) and
          y stays as it was.
T(.) is the rounding to the logical activation type: the storage type for bf16 / f16, the run-time rounding for float32.

Exact data ("exact").  x integers -3..3, A, B integers -4..4, y and h integers -8..8, scales powers of two of either sign.
For x A over K and t B over the rank the sum of the absolute values of the terms stays below 2^24 (asserted per case by the
CPU test), so every float32 partial sum in every order is an integer below 2^24: exact.  The expectation is then the
oracle's value bit for bit, with real roundings at T(scale z) and T(y + .) (the integers grow past T's 8 / 11 bits), ties
included -- the CPU test counts the elements that sit exactly on a tie at each point.  The norm is exact too where every
element of a row is +-2^e and eps = 0: sum / K = 2^2e, the root and the reciprocal are exact, T(x rs) = +-1 and xs = +-w.
On plain float32 all of that is exact and a fused scale * z + y would give the same bits; one case ("cancel") therefore takes
scale = +-float32(1 / 3) (24 bits) on its exact integer z and y = -(scale z) rounded to an eighth: fl(scale z) rounds for real,
the sum cancels exactly (Sterbenz), and the one rounding of a fused multiply-add lands elsewhere on nearly every element.

Rule data ("rule").  x ~ N(0,1) rounded to T, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2), scales 10 and 0.25, y and h ~ N(0,1)
rounded to T, norm weights 1 + 0.1 N(0,1) rounded to T, eps = 1e-5.  Bounds, with u = 2^-24:

  c_K = ceil(K / 256) + 9: the float32 roundings on the longest path of a column's sum in lora_down_by_row_kernel -- one fmaf
      per k step of a thread (ceil(K / 256) of them), four adds in row16_sum, two levels of adds over the four rows of a wave
      in wave_sum ((a + b) + (c + d)), three adds across the four waves (red16[0] + [1] + [2] + [3]).
      |t - t64| <= c_K u sum_k |xs_k| |A_kj|, t64 summed in float64 from xs, the oracle's staged row.
  delta_K = (c_K / 2 + 6) u: the relative distance between the kernel's float32 x rs and the oracle's float64 x rs64.  The sum
      of squares runs through the same tree as a column of t (c_K roundings, all terms positive: relative c_K u), / K and + eps
      round once each; the root halves that ((c_K + 2) / 2 u); sqrtf and the division are allowed one ulp (2 u) each; the
      product x rs rounds once more (u).  eps reaches both sides as the same float32.
      16-bit or logically rounded T: an element whose x rs64 lies within delta_K |x rs64| of a rounding boundary of T may be
      staged as the other neighbour; its alternative xs_alt = T(alt w) adds sum_k |A_kj| |xs_alt,k - xs_k| (1 + c_K u) to the
      bound of t.  Plain float32: (delta_K + 2 u) sum |xs| |A| is added instead.
  up-add, from a float32 t the test supplies: z64 = sum t_j B_jc in float64 (exact products); lora_dot adds rank fmaf in
      order: |z - z64| <= rank u sum_j |t_j| |B_jc| = e_z.  The yardstick rounds ONCE from float64 at each point:
      term* = T(scale z64), y* = T(y + term*), h* = T(h + y*).  The propagated float32 error there: e1 = |scale| e_z +
      u |scale z64| (the float32 product), e2 = |fl32(y + term*) - (y + term*)| and e3 likewise for h + y* (the float32 sum of
      two KNOWN T values loses exactly that, at most u |.|, and nothing where they add exactly -- an exact tie rounds one way
      only).  An element is NEAR at a point if its error there is not zero and a boundary of T (the midpoint of two
      neighbours) lies within it of the float64 value.  An element near at no point must be bit-equal; a near one may differ by ulp_T(term*) + ulp_T(y*) (+ ulp_T(h*)).  Plain float32 has no
      boundaries: |y - y*| <= e1 + u |y*| (+ u |h*| on the residual), the yardstick unrounded in float64.
  NEAR_CAP: the near set of a rule case is at most 10 % of its elements -- a condition on the case, computed here; a case that
      misses it gets a smaller rank, never a higher cap.  (e1 / |scale z| is about rank^1.5 u: against half a spacing of
      2^-9 (bf16) or 2^-12 (f16) that is 0.2 % / 1.6 % at rank 16 and 1.5 % / 12 % at rank 64 -- hence no rank above 16 on f16
      rule cases; the exact cases carry the large ranks' bit patterns.)
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from oracle import ref_model
from oracle.numerics import round_f64, round_to

MAX_ADAPTERS = 16                     # MI_MAX_ADAPTERS (include/mi355_decode.h)
ENGINE_COL = MAX_ADAPTERS             # LORA_ENGINE_COL (csrc/lora_rows.h)
TABLE_COLS = MAX_ADAPTERS + 1
T_LD = 3 * 64                         # LORA_ROWS_T_LD
NTHR, UP_COLS = 256, 1024
K_MAX = 36864
U = 2.0 ** -24
THIRD = float(np.float32(1.0 / 3.0))
NEAR_CAP = 0.10
# name -> (storage dtype, MI_RND_*, the logical dtype T)
TYPES = {"bf16": ("bfloat16", 0, "bfloat16"), "f16": ("float16", 0, "float16"), "f32": ("float32", 0, "float32"),
         "f32_rnd_bf16": ("float32", 1, "bfloat16"), "f32_rnd_f16": ("float32", 2, "float16")}


def c_K(K):
    return -(-K // NTHR) + 9


def delta_K(K):
    return (c_K(K) / 2 + 6) * U


# ---------------------------------------------------------------------------------------------------------------------------
# the case table

@dataclass(frozen=True)
class Case:
    name: str
    data: str                                  # "exact" | "rule"
    tname: str                                 # key of TYPES
    K: int
    parts: Tuple[Tuple[int, int], ...]         # (row0, n) of every part
    ldy: int
    rows: Tuple[int, ...]                      # row_adapter
    adapters: tuple                            # ((column, ((rank, scale) | None per part)), ...)
    norm: bool = False
    resid: bool = False
    ldr: int = 0
    cancel: bool = False                       # plain float32: scale = +-float32(1 / 3) and y = -(scale z) to an eighth

    @property
    def M(self):
        return len(self.rows)

    @property
    def ldx(self):
        return self.K + 8

    @property
    def exact(self):
        return self.data == "exact"

    @property
    def logical(self):
        return TYPES[self.tname][2]

    def cover(self, m, r):
        """(rank, scale) of part r under row m's adapter, or None"""
        ad = self.rows[m]
        if ad < 0 or ad >= TABLE_COLS:
            return None
        parts = dict(self.adapters).get(ad)
        return None if parts is None else parts[r]


def case_id(c):
    return f"{c.data}-{c.tname}-{c.name}"


def _cat(*widths, gap=5, start=0):
    """parts laid side by side from column `start` -> (parts, ldy) with `gap` spare columns behind the last"""
    parts, col = [], start
    for n in widths:
        parts.append((col, n))
        col += n
    return tuple(parts), col + gap


# the three-part layout of the issue: widths 1032, 8 and 264 at non-zero row0, a hole between parts 0 and 1, a gap at the end
ZOO_PARTS, ZOO_LDY = ((8, 1032), (1048, 8), (1064, 264)), 1336
ZOO_ROWS = (0, 7, 15, ENGINE_COL, -1, 17, -3, 5, 7)             # slot 5 is resident nowhere: all its entries are null
ZOO_ADAPTERS = (
    (0, ((20, 0.5), (17, -2.0), (64, 0.25))),
    (7, ((36, -0.5), None, (7, 2.0))),                           # covers parts 0 and 2 only
    (MAX_ADAPTERS - 1, ((60, 1.0), (18, -0.25), (9, 4.0))),
    (ENGINE_COL, ((63, -1.0), (5, 0.5), (32, 2.0))),
)
SMALL_ROWS = (0, ENGINE_COL, MAX_ADAPTERS - 1)
SMALL_ADAPTERS = ((0, ((1, 2.0), (16, -0.5))), (ENGINE_COL, ((3, 1.0), (4, -4.0))), (MAX_ADAPTERS - 1, ((8, 0.5), (1, -1.0))))
RESID_ROWS = (0, -1, 7, 3, ENGINE_COL, 17, 0, 7, -2)            # 7: resident, but not on this part; 3: resident nowhere


def _table():
    t = []

    def E(name, tname, K, parts_ldy, rows, adapters, **kw):
        t.append(Case(name, "exact", tname, K, parts_ldy[0], parts_ldy[1], tuple(rows), tuple(adapters), **kw))

    def R(name, tname, K, parts_ldy, rows, adapters, **kw):
        t.append(Case(name, "rule", tname, K, parts_ldy[0], parts_ldy[1], tuple(rows), tuple(adapters), **kw))

    # ---- every kind of row and the tail / vector / clamped ranks, three parts, K with a tail: once per type
    for tn in ("bf16", "f16", "f32", "f32_rnd_bf16"):
        E("zoo-k320", tn, 320, (ZOO_PARTS, ZOO_LDY), ZOO_ROWS, ZOO_ADAPTERS)
    # ---- the small ranks, widths 200 and 256, K = 256 (one step per thread)
    for tn in ("bf16", "f16", "f32_rnd_f16"):
        E("small-k256", tn, 256, _cat(200, 256), SMALL_ROWS, SMALL_ADAPTERS)
    # ---- K = 8: most threads idle; one full z-block
    E("k8-w1024", "bf16", 8, _cat(1024), (0,), ((0, ((8, 2.0),)),))
    E("k8-w8", "f16", 8, _cat(8), (7,), ((7, ((1, -0.5),)),))
    # ---- parts of unequal width, three z-blocks on the wide one
    E("k256-w2056-256", "f16", 256, _cat(2056, 256, gap=3), (0, -1, 7), ((0, ((9, 0.5), (16, -1.0))), (7, (None, (64, 0.125)))))
    # ---- the large K: M <= 3, rank <= 8 (A of about a megabyte); rank 64 at K = 4096 puts f16 on ties
    E("k4096-r64", "f16", 4096, _cat(200), (0, -1, 0), ((0, ((64, 0.25),)),))
    E("k4096", "bf16", 4096, _cat(8), (0, 7, ENGINE_COL), ((0, ((8, 0.5),)), (7, ((3, -1.0),)), (ENGINE_COL, ((4, 0.25),))))
    E("k12288", "f16", 12288, _cat(8), (0,), ((0, ((8, -0.125),)),))
    E("k12296", "bf16", 12296, _cat(8), (0, 7, 0), ((0, ((5, 0.5),)), (7, ((8, -0.25),))))
    E("k14336", "f32", 14336, _cat(8), (ENGINE_COL,), ((ENGINE_COL, ((8, 1.0),)),))
    E("k36864", "bf16", 36864, _cat(8), (0, -1, 7), ((0, ((8, 0.25),)), (7, ((4, -0.5),))))
    # ---- the exact norm: every type, and once behind the LDS opt-in
    norm_ad = ((0, ((20, 0.5),)), (7, ((4, -2.0),)), (ENGINE_COL, ((17, 1.0),)))
    for tn in ("bf16", "f16", "f32", "f32_rnd_bf16"):
        E("norm-k320", tn, 320, _cat(8), (0, 7, ENGINE_COL), norm_ad, norm=True)
    E("norm-k12296", "bf16", 12296, _cat(8), (0, 7, -1), ((0, ((8, 0.5),)), (7, ((1, 1.0),))), norm=True)
    # ---- the residual form
    resid_ad = ((0, ((64, 2.0),)), (7, (None,)), (ENGINE_COL, ((9, -0.5),)))
    for tn in ("bf16", "f16", "f32"):
        E("resid-k256", tn, 256, _cat(200, gap=3), RESID_ROWS, resid_ad, resid=True, ldr=205)
    # ---- plain float32, where nothing but `fp contract(off)` stands between scale * z and y + (.): a scale of 24 bits
    E("cancel-k256", "f32", 256, _cat(200), (0, 7, ENGINE_COL), ((0, ((64, THIRD),)), (7, ((9, -THIRD),)), (ENGINE_COL, ((16, THIRD),))),
      cancel=True)
    # ---- rule data
    rule_ad = ((0, ((16, 10.0),)), (7, ((7, 0.25),)), (ENGINE_COL, ((1, 10.0),)))
    R("k320", "bf16", 320, _cat(264), (0, 7, ENGINE_COL), rule_ad)
    R("k4096", "f16", 4096, _cat(264), (0, 7, -1), ((0, ((8, 10.0),)), (7, ((16, 0.25),))))
    R("k4096-r64", "f32", 4096, _cat(1032), (0, -1, 0), ((0, ((64, 10.0),)),))
    R("k256-r32", "f32_rnd_bf16", 256, _cat(200), (0, 7, ENGINE_COL), ((0, ((32, 10.0),)), (7, ((63, 0.25),)), (ENGINE_COL, ((9, 0.25),))))
    R("norm-k4096", "bf16", 4096, _cat(200), (0, 7, 17), ((0, ((16, 10.0),)), (7, ((20, 0.25),))), norm=True)
    R("norm-k320", "f16", 320, _cat(200), (0, 7, ENGINE_COL), ((0, ((9, 10.0),)), (7, ((16, 0.25),)), (ENGINE_COL, ((5, 0.25),))), norm=True)
    R("norm-k12296", "f32", 12296, _cat(8), (0, -1, 7), ((0, ((8, 10.0),)), (7, ((4, 0.25),))), norm=True)
    R("norm-k256", "f32_rnd_bf16", 256, _cat(200), (0, 7, -1), ((0, ((36, 10.0),)), (7, ((3, 0.25),))), norm=True)
    R("norm-k36864", "bf16", 36864, _cat(8), (0, -1, 7), ((0, ((8, 10.0),)), (7, ((5, 0.25),))), norm=True)
    rr = ((0, ((16, 10.0),)), (7, (None,)), (ENGINE_COL, ((9, 0.25),)))
    for tn in ("bf16", "f16", "f32"):
        R("resid-k256", tn, 256, _cat(200, gap=3), RESID_ROWS, rr, resid=True, ldr=205)
    return tuple(t)


CASES = _table()
assert len({case_id(c) for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# which branches of the two kernels a case runs, from its shapes alone

def down_groups(rk):
    """the 16-rank groups of one part in lora_down_by_row_kernel -> ["vec" | "scalar", ...]"""
    rk = min(rk, 64)
    return ["vec" if (rk % 4 == 0 and j0 + 16 <= rk) else "scalar" for j0 in range(0, rk, 16)]


def up_blocks(c):
    """grid.z of the up-add launch, and per part the z-blocks that do work"""
    widest = max(n for _, n in c.parts)
    gz = -(-widest // UP_COLS)
    return gz, [-(-n // UP_COLS) for _, n in c.parts]


def tags(c):
    T = c.tname
    out = {f"type:{T}", f"m:{c.M}", f"k:{c.K}", f"{c.data}:{T}"}
    if c.K < NTHR:
        out.add("down:idle-threads")
    if c.K > NTHR:
        out.add("down:k-loop-repeats")
    if c.K % NTHR:
        out.add("down:k-tail")
    out.add("down:lds-opt-in" if 4 * c.K > 48 * 1024 else "down:lds-default")
    if c.K == K_MAX:
        out.add("down:k-limit")
    if c.norm:
        out.add(f"norm-{c.data}:{T}")
    if c.cancel:
        assert T == "f32" and c.exact
        out.add("up:float32-two-roundings")
    if c.resid:
        out |= {f"resid-{c.data}:{T}", "resid"}
        assert len(c.parts) == 1 and c.parts[0][0] == 0 and c.ldr > c.parts[0][1]
    gz, per_part = up_blocks(c)
    if gz > 1:
        out.add("up:z-blocks")
    if any(b < gz for b in per_part):
        out.add("up:surplus-blocks-leave")
    for _, n in c.parts:
        out.add(f"w:{n}")
    if tuple(n for _, n in c.parts) == (1032, 8, 264) and all(r0 > 0 for r0, _ in c.parts):
        out.add("up:three-parts-at-row0")
    ends = sorted((r0, r0 + n) for r0, n in c.parts)
    if c.ldy > ends[-1][1]:
        out.add("up:gap-behind-last-part")
    if any(a[1] < b[0] for a, b in zip(ends[:-1], ends[1:])):
        out.add("up:hole-between-parts")
    table = dict(c.adapters)
    prev = None
    for m, ad in enumerate(c.rows):
        if ad == -1:
            out.add("row:-1")
        elif ad < 0:
            out.add("row:negative")
        elif ad >= TABLE_COLS:
            out.add(f"row:{ad}")
        elif ad not in table or all(p is None for p in table[ad]):
            out.add("row:null-slot")
        else:
            out.add({0: "row:slot-0", 7: "row:slot-7", MAX_ADAPTERS - 1: "row:slot-last", ENGINE_COL: "row:engine-column"}.get(ad, "row:slot"))
        cov = [c.cover(m, r) for r in range(len(c.parts))]
        if c.resid and cov[0] is None:
            out.add("resid:row-without-adapter" if not (0 <= ad < TABLE_COLS and ad in table) else "resid:row-adapter-not-on-part")
        ncov = sum(p is not None for p in cov)
        if 0 < ncov < len(cov):
            out.add("down:parts-some")
            if len(cov) == 3 and cov[0] and cov[2] and not cov[1]:
                out.add("down:parts-0-and-2")
        ngroups = 0
        for p in cov:
            if p is None:
                continue
            rk = p[0]
            g = down_groups(rk)
            ngroups += len(g)
            out |= {f"down:rank:{rk}", f"up:rank:{rk}"}
            if g == ["vec"]:
                out.add("down:one-vector-group")
            if len(g) == 2 and set(g) == {"scalar"}:
                out.add("down:two-scalar-groups")
            if "vec" in g and g[-1] == "scalar":
                out.add("down:vector-then-scalar-tail")
            if rk % 8:
                out.add("up:clamped-group")
        if ngroups > 1:
            out.add("down:red16-reused")
        cur = tuple(p for p in cov if p is not None)
        if prev and cur and {p[0] for p in prev} != {p[0] for p in cur} and {p[1] for p in prev} != {p[1] for p in cur}:
            out.add("rows:neighbours-differ-in-rank-and-scale")
        prev = cur
    return out


_PER_TYPE = {f"{k}:{T}" for T in ("bf16", "f16", "f32") for k in ("exact", "rule", "norm-exact", "norm-rule", "resid-exact", "resid-rule")}
REQUIRED = (_PER_TYPE
            | {f"type:{T}" for T in TYPES} | {"exact:f32_rnd_bf16", "rule:f32_rnd_bf16", "norm-exact:f32_rnd_bf16", "norm-rule:f32_rnd_bf16"}
            | {f"k:{K}" for K in (8, 256, 320, 4096, 12288, 12296, 14336, 36864)}
            | {"down:idle-threads", "down:k-loop-repeats", "down:k-tail", "down:lds-opt-in", "down:lds-default", "down:k-limit"}
            | {f"down:rank:{r}" for r in (1, 3, 4, 5, 16, 17, 18, 20, 36, 60, 32, 63, 64)}
            | {"down:one-vector-group", "down:two-scalar-groups", "down:vector-then-scalar-tail", "down:red16-reused",
               "down:parts-some", "down:parts-0-and-2"}
            | {f"up:rank:{r}" for r in (1, 7, 8, 9, 63, 64)} | {"up:clamped-group"}
            | {f"w:{n}" for n in (8, 200, 256, 1024, 1032, 2056, 264)}
            | {"up:z-blocks", "up:surplus-blocks-leave", "up:three-parts-at-row0", "up:gap-behind-last-part", "up:hole-between-parts"}
            | {"m:1", "m:3", "m:9"}
            | {"row:slot-0", "row:slot-7", "row:slot-last", "row:engine-column", "row:-1", "row:17", "row:negative", "row:null-slot",
               "rows:neighbours-differ-in-rank-and-scale"}
            | {"resid", "resid:row-without-adapter", "resid:row-adapter-not-on-part", "up:float32-two-roundings"})


# ---------------------------------------------------------------------------------------------------------------------------
# rounding boundaries of T

def t_next(r, logical, up):
    """the neighbour of the T value r (float32 array) towards +inf (up) or -inf, as float64"""
    r = np.asarray(r, dtype=np.float32)
    if logical == "float16":
        with np.errstate(over="ignore"):
            return np.nextafter(r.astype(np.float16), np.float16(np.inf if up else -np.inf)).astype(np.float64)
    assert logical == "bfloat16"
    i = r.view(np.int32).astype(np.int64)
    o = np.where(i < 0, -(i & 0x7FFFFFFF), i) + (0x10000 if up else -0x10000)
    back = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)
    return back.view(np.float32).astype(np.float64)


def ulp_T(r, logical):
    """the spacing of T at r (the wider side at a power of two)"""
    r64 = np.asarray(r, dtype=np.float64)
    return np.maximum(t_next(r, logical, True) - r64, r64 - t_next(r, logical, False))


def boundary_gap(v, r, logical):
    """distance of the float64 value v from the rounding boundary it is closest to; r = T(v)"""
    v = np.asarray(v, dtype=np.float64)
    nb = np.where(v >= r, t_next(r, logical, True), t_next(r, logical, False))
    return np.abs((np.asarray(r, np.float64) + nb) / 2 - v)


def is_tie(v, logical):
    """v (float64) sits exactly between two neighbouring T values"""
    r = round_f64(v, logical)
    return (r.astype(np.float64) != v) & (boundary_gap(v, r, logical) == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _rng(c, salt=""):
    return np.random.default_rng(zlib.crc32(f"{case_id(c)}/{salt}".encode()))


def eps_of(c):
    return 0.0 if (c.exact or not c.norm) else float(np.float32(1e-5))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def build(c):
    """-> dict: x (M, K); nw (K,) or None; A / B {(column, part): array}; y (M, ldy), NaN outside the parts; h (M, ldr) or
    None, NaN behind the part; xs (M, K) the staged row; t64 (M, 3, 64) float64, NaN where the kernel writes nothing; t_up
    (M, 3, 64) float32 = the t the up-add test supplies.  Nothing in it is writable."""
    rng = _rng(c)
    M, K, T = c.M, c.K, c.logical
    nw = None
    if c.exact:
        if c.norm:
            x = (rng.choice([-1.0, 1.0], (M, K)) * np.exp2(rng.integers(-3, 4, (M, 1)))).astype(np.float32)
            nw = rng.integers(-3, 4, K).astype(np.float32)
        else:
            x = rng.integers(-3, 4, (M, K)).astype(np.float32)
    else:
        x = round_to(rng.standard_normal((M, K)).astype(np.float32), T)
        if c.norm:
            nw = round_to((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32), T)
    A, B = {}, {}
    for col, parts in c.adapters:
        for r, p in enumerate(parts):
            if p is None:
                continue
            rk, n = p[0], c.parts[r][1]
            if c.exact:
                A[col, r] = rng.integers(-4, 5, (K, rk)).astype(np.float32)
                B[col, r] = rng.integers(-4, 5, (rk, n)).astype(np.float32)
            else:
                A[col, r] = (rng.uniform(-1.0, 1.0, (K, rk)) / np.sqrt(K)).astype(np.float32)
                B[col, r] = (0.05 * rng.standard_normal((rk, n))).astype(np.float32)

    def values(shape):
        return rng.integers(-8, 9, shape).astype(np.float32) if c.exact else round_to(rng.standard_normal(shape).astype(np.float32), T)

    y = np.full((M, c.ldy), np.nan, np.float32)
    for r0, n in c.parts:
        y[:, r0:r0 + n] = values((M, n))
    h = None
    if c.resid:
        h = np.full((M, c.ldr), np.nan, np.float32)
        h[:, :c.parts[0][1]] = values((M, c.parts[0][1]))
    xs = ref_model.rms_norm(x, T, nw, T, eps_of(c))[0] if c.norm else x
    t64 = np.full((M, 3, 64), np.nan, np.float64)
    for m in range(M):
        for r in range(len(c.parts)):
            p = c.cover(m, r)
            if p is not None:
                t64[m, r, :p[0]] = xs[m].astype(np.float64) @ A[c.rows[m], r].astype(np.float64)
    if c.cancel:
        for m in range(M):
            for r, (r0, n) in enumerate(c.parts):
                p = c.cover(m, r)
                if p is not None:
                    z = t64[m, r, :p[0]] @ B[c.rows[m], r].astype(np.float64)
                    y[m, r0:r0 + n] = -np.rint(p[1] * z * 8) / 8
    return _freeze(dict(x=x, nw=nw, A=A, B=B, y=y, h=h, xs=xs, t64=t64, t_up=t64.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------------------
# the down stage

def exactness(c, d):
    """-> (largest sum of |terms| of x A, of t B) over the case, in units of the smallest term's last bit (all data are
    integers: the unit is 1)"""
    s1 = s2 = 0.0
    for m in range(c.M):
        for r in range(len(c.parts)):
            p = c.cover(m, r)
            if p is None:
                continue
            a, b = d["A"][c.rows[m], r], d["B"][c.rows[m], r]
            s1 = max(s1, float((np.abs(d["xs"][m]).astype(np.float64) @ np.abs(a).astype(np.float64)).max()))
            s2 = max(s2, float((np.abs(d["t64"][m, r, :p[0]]) @ np.abs(b).astype(np.float64)).max()))
    return s1, s2


def norm_alternatives(c, d):
    """Behind the norm on a 16-bit or logically rounded T: -> (flagged (M, K) bool, xs_alt (M, K)): the elements whose
    x rs64 lies within delta_K of a rounding boundary of T, and what they are staged as if they fall on the other side."""
    T = c.logical
    x64 = d["x"].astype(np.float64)
    rs = 1.0 / np.sqrt(np.mean(x64 * x64, axis=-1, keepdims=True) + eps_of(c))
    p = x64 * rs
    xn = round_to(p.astype(np.float32), T)                          # the oracle's own xn
    gap = boundary_gap(p, xn, T)
    flagged = gap <= delta_K(c.K) * np.abs(p)
    alt = np.where(p >= xn, t_next(xn, T, True), t_next(xn, T, False)).astype(np.float32)
    xs_alt = round_to(alt * d["nw"], T)
    return flagged, np.where(flagged, xs_alt, d["xs"]).astype(np.float32)


def t_bound(c, d):
    """(M, 3, 64) float64: the bound on |t - t64| of a rule case (NaN where nothing is written)"""
    out = np.full((c.M, 3, 64), np.nan, np.float64)
    ck = c_K(c.K)
    if c.norm and c.logical != "float32":
        flagged, xs_alt = norm_alternatives(c, d)
        dxs = np.abs(xs_alt.astype(np.float64) - d["xs"])
    for m in range(c.M):
        for r in range(len(c.parts)):
            p = c.cover(m, r)
            if p is None:
                continue
            a = np.abs(d["A"][c.rows[m], r]).astype(np.float64)
            s = np.abs(d["xs"][m]).astype(np.float64) @ a
            b = ck * U * s
            if c.norm:
                b += (delta_K(c.K) + 2 * U) * s if c.logical == "float32" else (dxs[m] @ a) * (1 + ck * U)
            out[m, r, :p[0]] = b
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the up-add stage

def _f32_error(v):
    """what the float32 sum of two T values loses: |fl32(v) - v|, zero where they add exactly (at most u |v|)"""
    return np.abs(v.astype(np.float32).astype(np.float64) - v)


def _near(v, r, e, T):
    """a boundary of T within the float32 error e > 0 of v (r = T(v)); an exact v -- a tie included -- rounds one way only"""
    return (e > 0) & (boundary_gap(v, r, T) <= e)


def up_expect(c, d, t=None):
    """The yardstick of the up-add run from t (default: the case's t_up) -> dict over the OUTPUT buffer (y [M][ldy], or with
    a residual h [M][ldr]): want (float32; NaN where the sentinel stays), wrote (bool: elements the kernel writes),
    near (bool), allowed (float64: 0 where the element must be bit-equal), want64 (plain float32 only), ties (3 counts)."""
    t = d["t_up"] if t is None else t
    T = c.logical
    plain = T == "float32"
    src = d["h"] if c.resid else d["y"]
    want = src.copy()
    want64 = src.astype(np.float64)
    wrote = np.zeros(src.shape, bool)
    near = np.zeros(src.shape, bool)
    allowed = np.zeros(src.shape, np.float64)
    ties = [0, 0, 0]
    for m in range(c.M):
        for r, (r0, n) in enumerate(c.parts):
            p = c.cover(m, r)
            if p is None and not c.resid:
                continue
            yv = d["y"][m, r0:r0 + n].astype(np.float64)
            nr = np.zeros(n, bool)
            al = np.zeros(n, np.float64)
            if p is not None:
                rk, sc = p
                b = d["B"][c.rows[m], r].astype(np.float64)
                tt = t[m, r, :rk].astype(np.float64)
                z64 = tt @ b
                ez = rk * U * (np.abs(tt) @ np.abs(b))
                v1 = float(np.float32(sc)) * z64
                e1 = abs(sc) * ez + U * np.abs(v1)
                if plain and not c.exact:
                    v2 = yv + v1
                    al += e1 + U * np.abs(v2)
                    ys = v2
                elif plain:                                        # exact z: two float32 roundings, each of an exact value
                    ys = round_f64(yv + round_f64(v1, T), T)
                else:
                    term = round_f64(v1, T)
                    nr |= _near(v1, term, e1, T)
                    ties[0] += int(is_tie(v1, T).sum())
                    v2 = yv + term
                    ys = round_f64(v2, T)
                    nr |= _near(v2, ys, _f32_error(v2), T)
                    ties[1] += int(is_tie(v2, T).sum())
                    al += ulp_T(term, T) + ulp_T(ys, T)
            else:
                ys = yv
            if c.resid:
                v3 = d["h"][m, :n].astype(np.float64) + ys
                if plain:
                    al += U * np.abs(v3)
                    ys = v3 if not c.exact else round_f64(v3, T)
                else:
                    ys = round_f64(v3, T)
                    nr |= _near(v3, ys, _f32_error(v3), T)
                    ties[2] += int(is_tie(v3, T).sum())
                    al += ulp_T(ys, T)
            want64[m, r0:r0 + n] = ys
            want[m, r0:r0 + n] = np.asarray(ys, np.float64).astype(np.float32)
            wrote[m, r0:r0 + n] = True
            near[m, r0:r0 + n] = nr
            allowed[m, r0:r0 + n] = al if plain else np.where(nr, al, 0.0)
    return dict(want=want, want64=want64, wrote=wrote, near=near, allowed=allowed, ties=tuple(ties))


def near_share(c, d):
    e = up_expect(c, d)
    return float(e["near"].sum()) / max(int(e["wrote"].sum()), 1)


def oracle_rows(c, d):
    """Exact cases: the up-add in the oracle's own words -- ref_model.Linear with a zero weight carrying the row's A, B and
    scale, y + (scale * ((x A) B)).astype(x.dtype) -- on the staged row xs, added to y (and to h) -> the output buffer."""
    T = c.logical
    out = (d["h"] if c.resid else d["y"]).copy()
    for m in range(c.M):
        for r, (r0, n) in enumerate(c.parts):
            p = c.cover(m, r)
            yv = d["y"][m, r0:r0 + n]
            if p is not None:
                lin = ref_model.Linear(T, weight=np.zeros((n, c.K), np.float32), lora_a=d["A"][c.rows[m], r],
                                       lora_b=d["B"][c.rows[m], r], lora_scale=p[1])
                term, _ = lin(d["xs"][m][None], T)                 # T(0 + T(scale z)): the term alone
                yv = round_to(yv + term[0], T)
            elif not c.resid:
                continue
            out[m, r0:r0 + n] = round_to(d["h"][m, :n] + yv, T) if c.resid else yv
    return out
