"""Inputs, expectations, the acceptance rules and the case table of the exact tests of the 9..128-row decode GEMMs
(gemm_skinny.hip: skinny_kernel; gemm_q4.hip: q4_kernel behind its preparation pass): tests/test_gpu_skinny_exact.py runs
them on the device through mi_op_gemm_skinny, tests/test_skinny_cases.py checks without one what does not need it (the launch
plans' classes are all reached, the exact constructions are exact on the reference alone, the probes cover their boundaries,
the reference's own envelopes stay under the measured caps, a subtly wrong kernel would change the expected bits).  NumPy
and the oracle only, in the shape of tests/gemv16_cases.py.

Launch plans.  `skinny_plan` restates skinny_mt / skinny_plan / launch_gemm_skinny and the head of skinny_kernel: row tiles
per workgroup (5 -> 6, 7 -> 8), the row slabs of int4 weights (16-bit activations, more than 32 rows, and not SwiGLU or more
than 96 rows: two row tiles x ceil(rows / 32) slabs, the grid padded to 8 units x slabs), tiles, tile groups of 8, 256-wide
chunks, the slices' chunk bounds c0 = s nchunks / ksplit, c1 = (s + 1) nchunks / ksplit and the units a slice multiplies
(dense 8 x 32 k per chunk, int8 4 x 64 k, int4 2 x 128 k; u_end = min(c1 UPC, K / unit)).  `q4_plan` restates a FORCED plan of
gemm_q4.hip (mt, TW, KW, ksplit, NS), its tile units, the nblk / ks >= KW condition and gemm_q4_supported.  Every case passes
its ksplit (> 0: skinny_kernel; a forced code: gemm_q4.hip), so nothing depends on the device's compute units or on a cost
model; COST_MODEL holds the few ksplit = 0 cases, which only ask "the result equals the forced run with *ksplit_used".

Out of scope -- not reachable through mi_op_gemm_skinny without new ABI, and kept by their engine-level tests: the RMSNorm
hand-over between launches (sq_in / sq_out), the publish-only form, a [hi | lo] matrix (kx) and the LoRA terms.  On 16-bit
activations PRO_NORM therefore exists only behind gemm_q4.hip's preparation pass, on float32 ones as the deferred norm.

Exact cases ("int").  x holds integers -3..3 (-1..1 on int8 weights above 2048 columns, where 3 would pass the bound), dense
weights integers -4..4 (times 2^-e where a SwiGLU wants sums of moderate size), int4 weights come from gemv16_cases.exact_q4,
int8 weights from `exact_q8` (codes 0..255, per-(row, group) scales 2^-3 .. 2^-1, biases = scale x an integer in -128..0),
residuals and linear biases integers -8..8.  The sum over k of the absolute values of the kernel's own terms -- int4
s (offs + q) x and (b - offs s) x with offs 16 on bfloat16 and 0 on float16; int8 s q x and b x -- stays below 2^24 units of
the smallest scale: every summation order, slice order and wave order is exact and the kernel has to return the oracle's bits.

Column selection ("onehot").  Every row of x is 1 at one probed column, so an output row IS a column of W; the probes sit on
both sides of the 8-piece, the unit (32 / 64 / 128), the chunk (256), every slice bound, and end at K - 1; above 16 rows the
assignment of probes to rows moves from launch to launch, so that every 16-row fragment boundary carries different probes.

Pairing ("pair").  One-hot x, gate weights 2^5 .. 2^8 (sigmoid = 1 in float32 and float64: silu(g) = g) and odd up weights
below 128: out = g x u exactly -- SwiGLU bit for bit, one dense and one int4 case per fragment size.

Float32 activations ("hot3p", "hot3g"; bf16 weights).  One-hot x whose value has a full 24-bit mantissa, so hi, mid and lo
of the three-way split are all non-zero.  "hot3p": weights +-2^j, the output is +-2^j x bit for bit.  "hot3g": general bf16
weights, the bound of tests/test_gpu_gemv_f32.py::test_lo_term_is_pinned (three exact products, three float32 additions of
half an ulp each: 4 ulps = 2^-22 relative; a lost `lo` costs 2^-17, a lost `mid` 2^-9).

The rules ("rand", and every SwiGLU on exact sums that is not a "pair").
16-bit results (16-bit activations, or float32 ones with rnd = bf16): gemv16_cases' rule -- finite, every element within 1
unit of attn16_cases.rule_stats, at most RULE_CAP beyond half a unit.  RULE_CAP is measured: 4 x the largest share that
the oracle's own float32 envelopes (numerics.set_accum "f32_seq32" / "f32_pairwise") show against the exact oracle on these
very inputs; neither envelope is the kernel's order, hence the factor.  Measured by tests/test_skinny_cases.py over the rule
cases (N(0,1) activations, 0.05 N(0,1) weights, 34 tiles = 544 columns, 2048 columns of K):
  q4 rand-store-pro-m17 (plan 1,8,1,1,2)         bf16 0 / 0,  f16 0 / 0                (f32_seq32 / f32_pairwise)
  q4 rand-store-pro-m100 (plan 2,2,4,2,4)        bf16 0 / 0,  f16 0.0588 % / 0.0110 %  of 54400 elements
  q4 rand-store_f32-pro-ld-m64 (plan 2,4,2,1,4)  bf16 0 / 0,  f16 0.0230 % / 0.0057 %  of 34816
  float32 x, rnd = bf16, m32 (17408 elements): dense 0 / 0; q4 0 / 0; q8 0.0057 % / 0
  every SwiGLU on exact sums: 0 (the envelopes ARE the oracle there)
The largest is 32 of 54400 elements (q4 rand-store-pro-m100, float16, f32_seq32): RULE_CAP = 4 x 32 / 54400 = 0.2353 %,
below the 10 % of test_gpu_kernels._assert_close; the worst element of any envelope is 0.947 unit.
Float32 results without rounding (the deferred RMSNorm: "rand" + pro on float32 activations): error per element in units of
2^-24 x sum_k |x_k w_k| (x after the norm); the kernel is allowed F32_CAP = 4 x the envelopes' worst.  The envelopes also sum
the norm's squares in float32, so their row scale differs from the exact oracle's by an ulp and with it the rounding of
every normalised x -- as the kernel's does, which applies the row scale in the epilogue.  Measured (f32_seq32 / f32_pairwise):
dense m8 0.6249 / 0.2546, m32 0.7762 / 0.2568; q4 m8 0.7376 / 0.3606, m32 0.7463 / 0.3740; q8 m8 0.8945 / 0.3674, m32 0.7000 /
0.2611: F32_CAP = 4 x 0.8945 = 3.578 units.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from oracle import ref_model, ref_quant
from oracle.numerics import matmul_nt, round_to

from gemv16_cases import exact_q4, pack_q4
from attn16_cases import rule_stats

ACTS = ("bfloat16", "float16")
KINDS = ("dense", "q4", "q8")
EPS = 1e-5
UNIT = {"dense": 32, "q8": 64, "q4": 128}        # k of one weight load (a tile-major block)
UPC = {"dense": 8, "q8": 4, "q4": 2}             # loads per 256-wide chunk
RULE_CAP = 4 * (32 / 54400)                      # measured: see the module docstring and tests/test_skinny_cases.py
F32_CAP = 4 * 0.8945                             # ... in units of 2^-24 sum |x w|
Q4_MIN_TILES = 1024


def weight_kind(kind, wdt):
    """The library's weight kind name (gpu_helpers.wk_code) of a case's kind under a weight dtype."""
    t = "bf16" if wdt == "bfloat16" else "f16"
    return {"dense": t, "q4": "q4_" + t, "q8": "q8_" + t}[kind]


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plans

def skinny_mt(rows):
    mt = (rows + 15) // 16
    return 6 if mt == 5 else 8 if mt == 7 else mt


@dataclass(frozen=True)
class Plan:
    """skinny_kernel.  slices: per K slice (c0, c1, u_begin, u_end) -- chunks [c0, c1), units [u_begin, u_end)."""
    mt: int
    nslab: int
    ntiles: int
    ngroups: int
    nchunks: int
    ksplit: int
    grid: int
    unit: int
    upc: int
    slices: Tuple[Tuple[int, int, int, int], ...]
    kernel: str = "skinny"

    @property
    def rows_padded(self):
        return 16 * self.mt * self.nslab

    @property
    def bounds(self):
        """columns at which a K slice begins"""
        return tuple(s[0] * 256 for s in self.slices[1:])


def skinny_plan(M, ntiles, K, kind, swiglu=False, x32=False, ksplit=1, defer_norm=False):
    assert ksplit > 0 and 1 <= M <= (32 if x32 else 128)
    mt, nslab = skinny_mt(M), 1
    if kind == "q4" and not x32 and M > 32 and (not swiglu or M > 96):
        mt, nslab = 2, (M + 31) // 32
    ngroups, nchunks = (ntiles + 7) // 8, (K + 255) // 256
    ks = min(ksplit, nchunks)
    if defer_norm:
        ks = min(ks, 16)
    units = ngroups * ks
    grid = (units + 7) // 8 * 8 * nslab if nslab > 1 else units
    upc, nunits = UPC[kind], K // UNIT[kind]
    slices = []
    for s in range(ks):
        c0, c1 = s * nchunks // ks, (s + 1) * nchunks // ks
        slices.append((c0, c1, c0 * upc, min(c1 * upc, nunits)))
    return Plan(mt, nslab, ntiles, ngroups, nchunks, ks, grid, UNIT[kind], upc, tuple(slices))


@dataclass(frozen=True)
class Q4Plan:
    """q4_kernel under a forced plan.  slices: per K slice over workgroups (b0, b1), in 128-k blocks."""
    mt: int
    nslab: int
    TW: int
    KW: int
    NS: int
    ksplit: int
    ntu: int
    ntiles: int
    ngroups: int
    nblk: int
    grid: int
    slices: Tuple[Tuple[int, int], ...]
    kernel: str = "q4"

    @property
    def rows_padded(self):
        return 16 * self.mt * self.nslab

    @property
    def bounds(self):
        return tuple(s[0] * 128 for s in self.slices[1:])


def q4_plan(M, ntiles, K, swiglu, forced):
    """forced = (mt, TW, KW, ksplit, NS), every field > 0 -> the plan q4_plan() (gemm_q4.hip) makes of it, or None where its
    loops find none (the launch then fails with MI_ERR_INVALID)."""
    mt, TW, KW, ks, NS = forced
    assert min(forced) > 0
    mt_all, nblk = (M + 15) // 16, K // 128
    NP, npc = KW * 4 * mt + 1, (17 if mt >= 3 else 9)
    if (mt > (4 if swiglu else 2) or mt > mt_all or TW > 10 or KW * TW > 10 or NP > 33 or TW * KW + NS > 12 or NS * npc < NP
            or ks > 8 or nblk // ks < KW):
        return None
    nslab = (mt_all + mt - 1) // mt
    ntu = ntiles if swiglu else (ntiles + 1) // 2
    ngroups = (ntu + TW - 1) // TW
    units = ngroups * ks
    grid = (units + 7) // 8 * 8 * nslab if nslab > 1 else units
    return Q4Plan(mt, nslab, TW, KW, NS, ks, ntu, ntiles, ngroups, nblk, grid,
                  tuple((s * nblk // ks, (s + 1) * nblk // ks) for s in range(ks)))


def q4_supported(kind, x32, M, K, w_tiles, *, rnd=False, bias=False, forced=False):
    """gemm_q4_supported: w_tiles = W.N / 16 (both halves of a gate|up matrix)."""
    if rnd or bias or kind != "q4" or x32 or K % 128 or not 17 <= M <= 128:
        return False
    return forced or w_tiles >= Q4_MIN_TILES


# ---------------------------------------------------------------------------------------------------------------------------
# the case table

@dataclass(frozen=True)
class Case:
    data: str                 # "int" | "onehot" | "pair" | "hot3p" | "hot3g" | "rand"
    kind: str                 # "dense" | "q4" | "q8"
    epi: str                  # "store" | "store_f32" | "resid" | "swiglu"
    M: int
    tiles: int                # output columns / 16 (SwiGLU: per half)
    K: int
    ksplit: int = 1           # > 0: skinny_kernel with that split; 0: the cost model's (COST_MODEL only)
    q4plan: Optional[Tuple[int, int, int, int, int]] = None    # gemm_q4.hip under this forced plan
    pro: bool = False         # RMSNorm in front
    strides: bool = False     # ldx = K + 8, ldo = N + 3
    bias: bool = False        # a float32 linear bias (the bf16_bias / f16_bias instantiations)
    x32: bool = False         # float32 activations on bf16 / q4_bf16 / q8_bf16 weights
    rnd: bool = False         # ... with the outputs rounded to bfloat16 (RND_BF16)

    @property
    def name(self):
        f = "".join(t for t, on in (("-pro", self.pro), ("-ld", self.strides), ("-bias", self.bias), ("-x32", self.x32),
                                    ("-rnd", self.rnd)) if on)
        how = "p" + ".".join(map(str, self.q4plan)) if self.q4plan else f"s{self.ksplit}"
        return f"{self.data}-{self.epi}{f}-m{self.M}-t{self.tiles}-k{self.K}-{how}"

    @property
    def swiglu(self):
        return self.epi == "swiglu"

    @property
    def exact(self):
        """compared bit for bit"""
        if self.pro or self.data in ("rand", "hot3g"):
            return False
        return not self.swiglu or self.data == "pair"

    @property
    def N(self):
        return self.tiles * 16

    @property
    def wrows(self):
        return self.N * (2 if self.swiglu else 1)

    @property
    def acts(self):
        return ("float32",) if self.x32 else ACTS

    def plan(self, ksplit=None):
        if self.q4plan is not None and ksplit is None:
            return q4_plan(self.M, self.tiles, self.K, self.swiglu, self.q4plan)
        ks = self.ksplit if ksplit is None else ksplit
        return skinny_plan(self.M, self.tiles, self.K, self.kind, self.swiglu, self.x32, max(ks, 1),
                           defer_norm=self.pro and self.x32 and not self.rnd)

    def routed_to_q4(self, forced=None):
        forced = (self.q4plan is not None) if forced is None else forced
        return q4_supported(self.kind, self.x32, self.M, self.K, self.wrows // 16, rnd=self.rnd, bias=self.bias, forced=forced)


def wdt_of(c, act):
    """dtype of the weights (and of a quantised matrix's scales and biases)"""
    return "bfloat16" if c.x32 else act


def odt_of(c, act):
    """dtype whose values the outputs are (float32 activations store float32 either way)"""
    return ("bfloat16" if c.rnd else "float32") if c.x32 else act


def case_id(c):
    return f"{c.kind}-{c.name}"


def _k(kind, dense, q8, q4):
    return {"dense": dense, "q8": q8, "q4": q4}[kind]


def _table(kind):
    def S(data, epi, M, tiles, K, ks=1, **kw):
        return Case(data, kind, epi, M, tiles, K, ks, **kw)

    u = UNIT[kind]
    rag = 256 + _k(kind, 32, 64, 128)                  # K % 256 = one unit
    rag2 = _k(kind, 480, 320, 384)                     # K % 256 = 224 (dense), the last unit of a chunk missing / one unit
    t = [
        # ---- rows / fragment: first and last row count of every MT; the K and tile classes ride along
        S("int", "store", 9, 1, u),                    # one unit, one tile: seven spare waves
        S("int", "store", 16, 8, 256),                 # one chunk, one full group
        S("int", "store", 17, 9, rag, 2),              # ksplit = nchunks, the second slice is the ragged chunk; 8 + 1 tiles
        S("int", "store", 32, 17, 4608, 5),            # 18 chunks in 5 unequal slices
        S("int", "store", 33, 3, rag2, 3),             # ksplit > nchunks (clamped to 2); int4: the second slab holds 1 row
        S("int", "store", 48, 9, 1024, 4),             # ksplit = nchunks = 4
        S("int", "store", 49, 3, 4608, 16),            # 16 slices
        S("int", "store", 64, 8, 512, 2),
        S("int", "store", 65, 9, 768, 2),              # 31 padded rows; 3 chunks in 2 slices
        S("int", "store", 96, 3, 1024, 3),
        S("int", "store", 97, 1, 512, 2),              # 31 padded rows
        S("int", "store", 128, 17, 768, 1),
        # ---- epilogues
        S("int", "store_f32", 40, 9, 768, 3), S("int", "resid", 24, 17, 1024, 2), S("int", "resid", 80, 3, rag, 2),
        S("int", "swiglu", 9, 3, 512, 2), S("int", "swiglu", 32, 9, 768, 1), S("int", "swiglu", 64, 1, rag, 2),
        # ---- strides: x and out are slabs of wider buffers
        S("int", "store", 17, 3, rag, 2, strides=True), S("int", "store_f32", 33, 9, 512, 1, strides=True),
        S("int", "resid", 65, 1, 768, 3, strides=True), S("int", "swiglu", 48, 3, 512, 2, strides=True),
        # ---- column selection
        S("onehot", "store", 9, 3, u), S("onehot", "store", 16, 3, 256), S("onehot", "store", 17, 9, rag, 2),
        S("onehot", "store", 33, 3, 4608, 5), S("onehot", "store", 65, 3, rag2, 3), S("onehot", "store", 128, 3, 1024, 4),
        S("onehot", "resid", 40, 3, 768, 2, strides=True),
    ]
    if kind != "q8":
        # ---- SwiGLU bit for bit, per fragment size (int4 at 128 rows: slabs)
        t += [S("pair", "swiglu", M, 3, 512, 2) for M in (16, 32, 48, 64, 96, 128)]
        # ---- a float32 linear bias, added once where the slices meet
        t += [S("int", "store", 40, 9, 768, 3, bias=True), S("int", "resid", 16, 3, 512, 1, bias=True),
              S("int", "resid", 72, 9, rag, 2, bias=True, strides=True)]
    if kind == "dense":
        t += [S("int", "store", 8, 3, 4608, 5)]        # below 9 rows: the K % 4096 in 1..1024 hand-over from gemv_mfma
    if kind == "q8":
        t += [S("int", "store", 1, 3, 64), S("int", "store", 8, 9, 4608, 5), S("onehot", "store", 1, 3, 320, 2),
              S("int", "swiglu", 128, 3, 512, 2), S("int", "swiglu", 96, 1, 256)]
    if kind == "q4":
        t += [S("int", "store", 100, 9, 640, 2),       # 4 slabs of (32, 32, 32, 4) rows; 4 units in a grid of 8 x 4
              S("int", "swiglu", 96, 3, 512, 2),       # no slabs: MT = 6
              S("int", "swiglu", 97, 3, 512, 2), S("int", "swiglu", 128, 9, 768, 3),      # slabs
              S("onehot", "store", 100, 3, 640, 2),
              # a biased int4 call above 16 rows on a matrix gemm_q4.hip would take (1024 tiles): it stays on skinny_kernel
              S("int", "store", 33, 1024, 128, 0, bias=True)]
        # ---- gemm_q4.hip: the 13 forced plans of test_gpu_skinny.Q4_PLANS; shapes: ragged rows, an odd number of tiles, K
        # blocks that do not divide by the K lanes
        A, B, C_, D, E = (17, 5, 640), (61, 17, 1152), (64, 9, 1024), (100, 9, 896), (128, 8, 2560)
        plain = {(1, 1, 8, 1, 4): (B, E), (1, 8, 1, 1, 2): (A, D), (2, 2, 4, 1, 4): (A, C_), (2, 4, 2, 2, 2): (A, B),
                 (2, 8, 1, 1, 2): (D, E), (2, 1, 4, 1, 4): (C_, A), (2, 5, 2, 1, 2): (B, D), (2, 3, 2, 1, 2): (A, E)}
        sw = {(3, 4, 2, 1, 4): (B, D), (4, 4, 2, 1, 4): (C_, E), (4, 8, 1, 3, 2): (B, E), (4, 2, 2, 2, 4): (C_, E),
              (4, 10, 1, 1, 2): (D, C_)}
        for p, shapes in plain.items():
            t += [Case("int", kind, "store", *sh, q4plan=p) for sh in shapes]
        for p, shapes in sw.items():
            t += [Case("int", kind, "swiglu", *sh, q4plan=p) for sh in shapes]
            t += [Case("pair", kind, "swiglu", shapes[0][0], 3, 1152, q4plan=p)]
        t += [Case("int", kind, "resid", 61, 17, 1152, q4plan=(2, 4, 2, 2, 2), strides=True),
              Case("int", kind, "store_f32", 100, 9, 896, q4plan=(2, 5, 2, 1, 2), strides=True),
              Case("onehot", kind, "store", 61, 3, 1152, q4plan=(2, 4, 2, 2, 2)),
              Case("onehot", kind, "store", 17, 3, 640, q4plan=(1, 8, 1, 1, 2)),
              Case("onehot", kind, "store", 100, 3, 896, q4plan=(2, 2, 4, 1, 4)),
              # RMSNorm in the preparation pass (random data, the rule; 34 tiles)
              Case("rand", kind, "store", 17, 34, 2048, q4plan=(1, 8, 1, 1, 2), pro=True),
              Case("rand", kind, "store", 100, 34, 2048, q4plan=(2, 2, 4, 2, 4), pro=True),
              Case("rand", kind, "store_f32", 64, 34, 2048, q4plan=(2, 4, 2, 1, 4), pro=True, strides=True)]
    # ---- float32 activations (bf16 / q4_bf16 / q8_bf16 weights): 16- and 32-row instantiations
    X = functools.partial(S, x32=True)
    t += [X("int", "store", 1, 1, u), X("int", "store", 8, 9, 4608, 5), X("int", "resid", 16, 8, rag, 2),
          X("int", "store", 17, 3, 768, 3, rnd=True), X("int", "store_f32", 32, 17, 1024, 16, strides=True),
          X("int", "resid", 32, 3, 512, 2, rnd=True), X("int", "swiglu", 17, 3, 512, 2, rnd=True),
          X("int", "swiglu", 8, 9, 768, 1, rnd=True, strides=True),
          X("onehot", "store", 8, 3, rag, 2), X("onehot", "store", 32, 3, 768, 3),
          X("rand", "store", 32, 34, 2048, 2, rnd=True),
          # the deferred RMSNorm (the row scale in the epilogue; the slices' sums of squares meet with the partial tiles)
          X("rand", "store", 8, 34, 2048, 1, pro=True), X("rand", "store", 32, 34, 2048, 4, pro=True)]
    if kind != "q8":
        t += [X("pair", "swiglu", 16, 3, 512, 2), X("pair", "swiglu", 32, 3, 512, 1)]
    if kind == "dense":
        t += [X("hot3p", "store", 8, 3, 768, 3), X("hot3p", "store", 17, 9, 288, 2), X("hot3g", "store", 32, 3, 768, 2),
              X("hot3g", "store", 16, 3, 256, 1), X("int", "store", 8, 3, 512, 2, bias=True)]
    return t


CASES = tuple(c for kind in KINDS for c in _table(kind))
assert len({case_id(c) for c in CASES}) == len(CASES)

# the cost model's own split (ksplit = 0): the result must equal the forced run with *ksplit_used
COST_MODEL = (Case("int", "dense", "store", 40, 9, 4608, 0), Case("int", "q8", "store", 12, 17, 4608, 0))


def classes_of(c):
    """The classes of the issue's table that case c reaches."""
    p = c.plan()
    out = {f"e:{c.epi}"}
    if c.strides:
        out.add(f"s:{c.epi}")
    if c.data in ("onehot", "pair", "hot3p", "hot3g"):
        out.add(f"x:{c.data}")
    if c.bias:
        out.add(f"b:{c.epi}")
        if c.kind == "q4" and c.M > 16 and c.wrows // 16 >= Q4_MIN_TILES and not c.routed_to_q4():
            out.add("b:q4-stays-on-skinny")
    if c.x32:
        out |= {f"x32:m{c.M}", f"x32:{c.epi}", "x32:rnd" if c.rnd else "x32:plain"}
        if c.pro:
            out.add("x32:norm-ks1" if p.ksplit == 1 else "x32:norm-split")
        return out
    if p.kernel == "q4":
        out |= {"q4:plan:" + ".".join(map(str, c.q4plan)), f"q4:m{c.M}"}
        if p.ntiles % 2 and not c.swiglu:
            out.add("q4:odd-tiles")
        if any((b1 - b0) % p.KW for b0, b1 in p.slices):
            out.add("q4:blocks-not-divisible-by-kw")
        if p.ksplit > 1:
            out.add("q4:ksplit")
        if c.swiglu:
            out.add(f"q4:swiglu-mt{p.mt}")
        if c.pro:
            out.add("q4:norm")
        return out
    out |= {f"m:{c.M}", f"mt:{p.mt}"}
    if p.nslab > 1:
        out.add(f"slab:{'swiglu-' if c.swiglu else ''}m{c.M}")
        if (p.ngroups * p.ksplit) % 8:
            out.add("slab:padded-grid")
        if c.M % 32 == 1:
            out.add("slab:last-holds-one-row")
    if c.kind == "q4" and c.swiglu and c.M == 96 and p.nslab == 1 and p.mt == 6:
        out.add("slab:none-swiglu-m96")
    if p.ntiles in (1, 8, 9, 17):
        out.add(f"t:{p.ntiles}")
    if c.K == p.unit:
        out.add("k:one-unit")
    if c.K == 256:
        out.add("k:256")
    if c.K % 256:
        out.add(f"k:ragged-{c.K % 256}")
    if c.ksplit == 1:
        out.add("ks:1")
    if c.ksplit == p.nchunks > 1:
        out.add("ks:nchunks")
    if c.ksplit > p.nchunks:
        out.add("ks:clamped")
    if p.nchunks % p.ksplit:
        out.add("ks:unequal")
    if p.ksplit == 16:
        out.add("ks:16")
    if c.kind == "dense" and c.M < 9:
        assert c.K > 4096 and 1 <= c.K % 4096 <= 1024 and not c.pro
        out.add("m:dense-handover-below-9")
    return out


_ROWS = (9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128)
_COMMON = ({f"m:{m}" for m in _ROWS} | {f"t:{t}" for t in (1, 8, 9, 17)}
           | {"e:store", "e:store_f32", "e:resid", "e:swiglu", "s:store", "s:store_f32", "s:resid", "s:swiglu", "x:onehot",
              "k:one-unit", "k:256", "ks:1", "ks:nchunks", "ks:clamped", "ks:unequal", "ks:16"}
           | {f"x32:m{m}" for m in (1, 8, 16, 17, 32)}
           | {"x32:store", "x32:resid", "x32:swiglu", "x32:rnd", "x32:plain", "x32:norm-ks1", "x32:norm-split"})
REQUIRED = {
    "dense": _COMMON | {f"mt:{m}" for m in (1, 2, 3, 4, 6, 8)} | {"k:ragged-32", "k:ragged-224", "m:dense-handover-below-9",
                                                                   "b:store", "b:resid", "x:pair", "x:hot3p", "x:hot3g"},
    "q8": _COMMON | {f"mt:{m}" for m in (1, 2, 3, 4, 6, 8)} | {"k:ragged-64", "m:1", "m:8"},
    "q4": _COMMON | {"mt:1", "mt:2", "mt:3", "mt:4", "mt:6", "k:ragged-128", "b:store", "b:resid", "b:q4-stays-on-skinny", "x:pair",
                     "slab:m33", "slab:m64", "slab:m100", "slab:m128", "slab:swiglu-m97", "slab:swiglu-m128",
                     "slab:none-swiglu-m96", "slab:padded-grid", "slab:last-holds-one-row",
                     "q4:odd-tiles", "q4:blocks-not-divisible-by-kw", "q4:ksplit", "q4:swiglu-mt3", "q4:swiglu-mt4", "q4:norm"}
    | {f"q4:m{m}" for m in (17, 61, 64, 100, 128)}
    | {"q4:plan:" + ".".join(map(str, p)) for p in
       [(1, 1, 8, 1, 4), (1, 8, 1, 1, 2), (2, 2, 4, 1, 4), (2, 4, 2, 2, 2), (2, 8, 1, 1, 2), (3, 4, 2, 1, 4), (4, 4, 2, 1, 4),
        (4, 8, 1, 3, 2), (2, 1, 4, 1, 4), (2, 5, 2, 1, 2), (4, 2, 2, 2, 4), (2, 3, 2, 1, 2), (4, 10, 1, 1, 2)]},
}


# ---------------------------------------------------------------------------------------------------------------------------
# column selection: the probes

def edges(c, p):
    """Columns E with 0 < E < K at which something of the launch plan changes hands: a 16-byte piece, a weight load (unit),
    the activation chunk, a K slice; gemm_q4.hip: a 128-k block, a K lane's next block, a slice of blocks."""
    e = {8, UNIT[c.kind], 256} | set(p.bounds)
    if p.kernel == "q4":
        e |= {128, 128 * p.KW}
    else:
        e.add((c.K - 1) // 256 * 256)                  # the last chunk, ragged or not
    return sorted(x for x in e if 0 < x < c.K)


def probes(c, p):
    cols = [0, c.K - 1]
    for e in edges(c, p):
        cols += [e - 1, e]
    return sorted(set(cols))


def hot_rows(c, p):
    """-> (launches, M) probe index of every row: windows of M probes that overlap by one, so the probe a row carries moves
    from launch to launch (above 16 rows: every fragment-row boundary sees different probes); at least two launches."""
    n = len(probes(c, p))
    step = max(c.M - 1, 1)
    while n > 1 and step % n == 0:
        step -= 1
    launches = max(2, -(-n // step))
    return (np.arange(c.M)[None, :] + step * np.arange(launches)[:, None]) % n


def hot3_value(m):
    """a float32 whose 24-bit mantissa is in use from end to end -- hi = 1, mid = 2^-9 (1 + 2^-7), lo = -2^-17 (1 - 2^-6), all
    non-zero, `mid` at 2^-9 and `lo` at 2^-17 of the value -- its scale and sign by row"""
    return np.float32((1.0 + 2.0 ** -9 + 2.0 ** -17 + 2.0 ** -23) * 2.0 ** (m % 7 - 3)) * np.float32(-1.0 if m & 1 else 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and expectations

def _rng(c, act, salt=0):
    return np.random.default_rng(zlib.crc32(f"{case_id(c)}/{act}/{salt}".encode()))


def _wexp(c):
    """Exact SwiGLU cases: weights times 2^-e so that the (still exact) gate and up sums have a deviation of about 4."""
    if not c.swiglu or c.data != "int":
        return 0
    dev_w = {"dense": 2.58, "q4": 1.7, "q8": 37.0}[c.kind]          # deviation of one weight, roughly
    return int(round(np.log2(np.sqrt(c.K) * 2.0 * dev_w / 4)))


def xmax_of(c):
    return 1 if (c.kind == "q8" and c.K > 2048) else 3


def pack_q8(q):
    """Codes (N, K) in 0..255 -> MLX-packed uint32 (N, K / 4): element j of a word at bits [8 j, 8 j + 8)."""
    n, k = q.shape
    sh = (np.arange(4, dtype=np.uint32) * 8).astype(np.uint32)
    return np.bitwise_or.reduce(q.astype(np.uint32).reshape(n, k // 4, 4) << sh, axis=-1).astype(np.uint32)


def exact_q8(rng, N, K, e=0):
    """-> (packed, scales, biases) with scales 2^-e x {2^-3, 2^-2, 2^-1} and biases = scale x (-128..0), per (row, group)."""
    q = rng.integers(0, 256, (N, K), dtype=np.uint32)
    scales = np.exp2(rng.integers(-3, 0, (N, K // 64)) - e).astype(np.float32)
    biases = (scales * rng.integers(-128, 1, (N, K // 64))).astype(np.float32)
    return pack_q8(q), scales, biases


def pair_q4(N, K):
    """The "pair" weights as int4: gate rows 2^5 x a code in {1, 2, 4, 8}, up rows 2 x code + an odd bias below 98."""
    n, k = np.arange(2 * N)[:, None], np.arange(K)[None, :]
    gate = n < N
    q = np.where(gate, 1 << ((n + k) % 4), (7 * n + 3 * k) % 16).astype(np.uint32)
    g = np.arange(K // 64)[None, :]
    scales = np.where(gate, 32.0, 2.0).astype(np.float32) * np.ones((2 * N, K // 64), np.float32)
    biases = np.where(gate, 0.0, 2 * ((5 * n + 3 * g) % 49) + 1).astype(np.float32)
    return pack_q4(q), scales, biases


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for a in v:
                a.setflags(write=False)
    return d


def _bits(c):
    return 4 if c.kind == "q4" else 8


@functools.lru_cache(maxsize=4)
def build(c, act):
    """-> dict(x (launches, M, K), w (rows, K) float32 = what the oracle multiplies with, q = (packed, scales, biases) or
    None, h (M, N) or None, nw (K,) or None, b (rows,) or None, want (launches, M, N)).  Nothing in it is writable."""
    rng = _rng(c, act)
    N, rows, K, M = c.N, c.wrows, c.K, c.M
    wdt, xdt = wdt_of(c, act), ("float32" if c.x32 else act)
    p = c.plan()
    q = None
    if c.data == "rand":
        x = round_to(rng.standard_normal((1, M, K)).astype(np.float32), xdt)
        w = round_to(rng.standard_normal((rows, K)).astype(np.float32) * 0.05, wdt)
        if c.kind != "dense":
            q = ref_quant.quantize(w, 64, _bits(c), wdt)
            w = ref_quant.dequantize(*q, 64, _bits(c))
    else:
        e = _wexp(c)
        if c.data == "pair":
            n, k = np.arange(rows)[:, None], np.arange(K)[None, :]
            if c.kind == "q4":
                q = pair_q4(N, K)
                w = ref_quant.dequantize(*q, 64, 4)
            else:
                w = np.where(n < N, np.exp2(rng.integers(5, 9, (rows, K))), 2 * rng.integers(0, 64, (rows, K)) + 1).astype(np.float32)
        elif c.data == "hot3p":
            w = (np.exp2(rng.integers(-4, 5, (rows, K))) * rng.choice([-1.0, 1.0], (rows, K))).astype(np.float32)
        elif c.data == "hot3g":
            w = round_to(rng.standard_normal((rows, K)).astype(np.float32) * 0.05, wdt)
        elif c.kind == "q4":
            q = exact_q4(rng, rows, K, e)
            w = ref_quant.dequantize(*q, 64, 4)
        elif c.kind == "q8":
            q = exact_q8(rng, rows, K, e)
            w = ref_quant.dequantize(*q, 64, 8)
        else:
            w = (rng.integers(-4, 5, (rows, K)) * np.exp2(-e)).astype(np.float32)
        if c.data == "int":
            xm = xmax_of(c)
            x = rng.integers(-xm, xm + 1, (1, M, K)).astype(np.float32)
        else:
            cols = np.asarray(probes(c, p))[hot_rows(c, p)]
            x = np.zeros(cols.shape + (K,), np.float32)
            val = np.array([hot3_value(m) for m in range(M)], np.float32) if c.data.startswith("hot3") else np.ones(M, np.float32)
            for l in range(cols.shape[0]):
                x[l, np.arange(M), cols[l]] = val
    nw = None
    if c.pro:
        nw = round_to(1.0 + 0.1 * rng.standard_normal(K).astype(np.float32), xdt)
    h = None
    if c.epi == "resid":
        h = (round_to(rng.standard_normal((M, N)).astype(np.float32), odt_of(c, act)) if c.data in ("rand", "hot3g")
             else rng.integers(-8, 9, (M, N)).astype(np.float32))
    b = rng.integers(-8, 9, rows).astype(np.float32) if c.bias else None
    d = dict(x=x, w=w, q=q, h=h, nw=nw, b=b)
    d["want"] = oracle(c, act, d)
    return _freeze(d)


def _linear(acc, b, odt, quant):
    """float32 accumulator (+ bias) -> values of odt: one rounding (dense) or two (quantised), as tests/biased_ref.py."""
    if b is None:
        return round_to(acc, odt)
    if quant:
        return round_to(round_to(acc, odt) + b, odt)
    return round_to(acc + b, odt)


def oracle(c, act, d, x=None, w=None):
    """The float64 oracle with the reference's rounding points, under the oracle's CURRENT accumulation mode."""
    x = d["x"] if x is None else x
    w = d["w"] if w is None else w
    N, odt, quant = c.N, odt_of(c, act), c.kind != "dense"
    if c.pro:
        xdt = "float32" if c.x32 else act
        x, _ = ref_model.rms_norm(x, xdt, d["nw"], xdt, EPS)
    b = d["b"]
    if c.swiglu:
        g = _linear(matmul_nt(x, w[:N]), None if b is None else b[:N], odt, quant)
        u = _linear(matmul_nt(x, w[N:]), None if b is None else b[N:], odt, quant)
        sig = round_to((1.0 / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32), odt)
        return round_to(round_to(g * sig, odt) * u, odt)
    y = _linear(matmul_nt(x, w), b, odt, quant)
    if c.epi == "resid":
        return round_to(d["h"][None] + y, odt)
    return y


def onehot_want(c, act, d):
    """What column selection means, without a sum: output row m of launch l is column cols[l][m] of W (times the row's value)."""
    x, w, N = d["x"], d["w"], c.N
    cols = np.abs(x).argmax(axis=-1)
    val = np.take_along_axis(x, cols[..., None], axis=-1)
    assert ((x != 0).sum(axis=-1) == 1).all()
    odt = odt_of(c, act)
    if c.data == "pair":
        return round_to((w[:N].T[cols] * w[N:].T[cols]).astype(np.float32), odt)
    y = round_to((w.T[cols].astype(np.float64) * val).astype(np.float32), odt)
    return round_to(d["h"][None] + y, odt) if c.epi == "resid" else y


def split3(x):
    """x = hi + mid + lo, each a bfloat16 value (store_x of skinny_kernel's float32 instantiations)."""
    hi = round_to(x, "bfloat16")
    r1 = (x - hi).astype(np.float32)
    mid = round_to(r1, "bfloat16")
    lo = round_to((r1 - mid).astype(np.float32), "bfloat16")
    return hi, mid, lo


def sum_abs_xw(c, act, d):
    """sum_k |x_k w_k| per output element, x after the norm: the scale of the float32 rule."""
    x = d["x"]
    if c.pro:
        x, _ = ref_model.rms_norm(x, "float32", d["nw"], "float32", EPS)
    return np.abs(x).astype(np.float64) @ np.abs(d["w"]).astype(np.float64).T


def f32_rule_stat(got, want, scale):
    """worst |got - want| in units of 2^-24 x scale (a non-finite got is infinitely far)"""
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(got, np.float64) - want) / (2.0 ** -24 * scale)
    return float(np.where(np.isfinite(got), r, np.inf).max())


def assert_rule(got, want, odt, what=""):
    """gemv16_cases.assert_rule under this file's measured cap"""
    worst, frac = rule_stats(got, want, odt)
    print(f"RULE {what}: worst {worst:.3f} unit, {100 * frac:.4f} % beyond half a unit (cap {100 * RULE_CAP:.4f} %)")
    assert np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst)
    assert frac <= RULE_CAP, (what, frac)
    return worst, frac


def assert_f32_rule(got, want, scale, what=""):
    worst = f32_rule_stat(got, want, scale)
    print(f"F32 RULE {what}: worst {worst:.4f} unit of 2^-24 sum |x w| (cap {F32_CAP:.4f})")
    assert np.isfinite(got).all(), what
    assert worst <= F32_CAP, (what, worst)
    return worst
