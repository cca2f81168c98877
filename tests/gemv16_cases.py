"""Inputs, expectations, the acceptance rule and the case table of the decode-GEMV tests on 16-bit activations
(gemv_mfma.hip / gemv_phase.h): tests/test_gpu_gemv16.py runs them on the device, tests/test_gemv16_cases.py checks without
one what does not need it (the launch plan's classes are all reached, the exact constructions are exact on the reference
alone, the probes cover their boundaries, the reference's own envelopes stay under the rule's cap).  NumPy and the oracle only.

Launch plan.  `launch_plan` restates make_params / launch_one / phase_nbuf (gemv_mfma.hip) and the Phase constants BK / UK /
TB / KS (gemv_phase.h): which instantiation a call runs (MB rows per fragment, chunk kc, J staging items, DB double
buffering) and how many tiles workgroup 0 and the last workgroup own.  The case table names its widths in tiles of 16 output
columns, symbolically in the device's compute units ("cus+1"), and `classes_of` names the classes a case reaches.

Exact cases ("int").  x holds integers -3..3, dense weights integers -4..4 (times a power of two where a SwiGLU wants sums
of moderate size), int4 weights are built directly: random codes, per-(row, group) scales from {2^-3, 2^-2, 2^-1} and biases
= scale x an integer in -12..0.  Every product and every partial sum, in any order, is then a multiple of one power of two
below 2^24 of them: float32 accumulation is exact whatever the order, and the kernel has to return the oracle's bits.

Column selection ("onehot").  Every row of x is 1 at one probed column, so an output row IS a column of W; the probes sit on
both sides of every boundary the launch plan names.

Pairing ("pair", the row-interleaved gate|up copy).  One-hot x again, gate weights 2^5 .. 2^8 (sigmoid = 1 in float32 and
in float64, so silu(g) = g) and odd up weights < 128: out = g x u exactly, and the product names both factors.

The rule ("rand", and every SwiGLU case: the activation's own roundings).  Every output finite; every element within 1 unit
of attn16_cases.rule_stats (RMS per output row); at most RULE_CAP of the elements beyond half a unit.  The cap is measured:
4 x the largest share that the oracle's own float32-accumulating envelopes (numerics.set_accum, both orders) show against
the exact oracle on these very inputs -- the kernel's order (32-wide MFMA blocks dealt to 8 waves, chunks) is neither
envelope's.  Measured by tests/test_gemv16_cases.py over all rule cases (N(0,1) activations, 0.05 N(0,1) weights, RMSNorm in
front, 34 tiles = 544 columns): bfloat16 0 % but for one case at 0.0123 %; float16 between 0 % and 0.2363 % -- the largest,
9 of 3808 elements, on dense "rand-store-pro-m7-t34-k4224" under f32_seq32 (the same case under f32_pairwise: 0 %; int4 at
4224 columns and 15 rows: 0.2206 % / 0.0980 %; int4 at 8320 columns: 0.2068 % / 0 %); the worst element of any envelope is
0.997 unit.  The SwiGLU cases on exact sums show 0 %.  RULE_CAP = 4 x 9 / 3808 = 0.9454 %, below the 10 % of
test_gpu_kernels._assert_close.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

from oracle import ref_model, ref_quant
from oracle.numerics import matmul_nt, round_to

from attn16_cases import rule_stats

ACTS = ("bfloat16", "float16")
KINDS = ("dense", "q4")
CUS_CHECKED = (64, 256, 304)
EPS = 1e-5
RULE_CAP = 4 * (9 / 3808)             # measured: see the module docstring and tests/test_gemv16_cases.py


def weight_kind(kind, act):
    """The library's weight kind name (gpu_helpers.wk_code) of a case's kind under an activation type."""
    t = "bf16" if act == "bfloat16" else "f16"
    return t if kind == "dense" else "q4_" + t


# ---------------------------------------------------------------------------------------------------------------------------
# the launch plan

@dataclass(frozen=True)
class Plan:
    MB: int
    kc: int
    nchunks: int
    J: int
    DB: bool
    tiles_first: int          # tiles owned by workgroup 0
    tiles_last: int           # ... by the last workgroup of the grid
    batches: int              # tile batches of workgroup 0
    BK: int
    UK: int
    TB: int
    KS: int
    tiles: int
    grid: int


def launch_plan(M, N, K, kind, epi, cus):
    """N: the rows the launch deals in tiles -- the output width (plain stores, and the paired-tile SwiGLU: pair_offset), or
    for "gu8" the 2 x pair_offset rows of the row-interleaved copy."""
    q4 = kind == "q4"
    paired = epi == "swiglu"
    MB = 8 if M <= 8 else 16
    kc = K if K <= (6144 if M <= 8 else 4096) else 4096                 # make_params
    nchunks = -(-K // kc)
    DB = MB == 8 and K > kc                                             # phase_nbuf == 2
    J = 2 if (MB == 8 and not DB and kc > 4096) else 1                  # launch_one
    assert kc <= 4096 or J == 2
    NW, NA = 8, (2 if paired else 1)
    BK = 128 if q4 else 32
    UK = 32 // NW if q4 else (128 // NW) // NA
    TB = 2 if (q4 and not paired) else 1
    KS = NW * UK * BK
    tiles = N // 16
    grid = min(tiles, cus)
    first = -(-tiles // grid)
    last = -(-(tiles - (grid - 1)) // grid)
    return Plan(MB, kc, nchunks, J, DB, first, last, -(-first // TB), BK, UK, TB, KS, tiles, grid)


# ---------------------------------------------------------------------------------------------------------------------------
# the case table

TILES = {"1": (0, 1), "2": (0, 2), "3": (0, 3), "6": (0, 6), "34": (0, 34), "cus": (1, 0), "cus+1": (1, 1), "2cus+1": (2, 1),
         "cus+2": (1, 2), "2cus+2": (2, 2)}


@dataclass(frozen=True)
class Case:
    data: str                 # "int" | "onehot" | "pair" | "rand"
    kind: str                 # "dense" | "q4"
    epi: str                  # "store" | "store_f32" | "resid" | "swiglu" | "gu8"
    M: int
    tiles: str                # tiles of the launch (TILES), resolved against the device's compute units
    K: int
    pro: bool = False
    strides: bool = False     # ldx = K + 8, ldo = N + 3

    @property
    def name(self):
        return (f"{self.data}-{self.epi}{'-pro' if self.pro else ''}{'-ld' if self.strides else ''}"
                f"-m{self.M}-t{self.tiles}-k{self.K}")

    @property
    def exact(self):
        return self.data in ("int", "onehot", "pair") and not self.pro and (self.epi not in ("swiglu", "gu8") or self.data == "pair")

    def ntiles(self, cus):
        a, b = TILES[self.tiles]
        return a * cus + b

    def width(self, cus):
        """Output columns: 16 per tile, 8 per tile of the row-interleaved copy."""
        return self.ntiles(cus) * (8 if self.epi == "gu8" else 16)

    def wrows(self, cus):
        return self.width(cus) * (2 if self.epi in ("swiglu", "gu8") else 1)

    def plan(self, cus):
        return launch_plan(self.M, self.ntiles(cus) * 16, self.K, self.kind, self.epi, cus)


def _c(data, epi, M, tiles, K, **kw):
    return [Case(data, kind, epi, M, tiles, K, **kw) for kind in KINDS]


def _d(data, epi, M, tiles, K, **kw):
    return [Case(data, "dense", epi, M, tiles, K, **kw)]


def _q(data, epi, M, tiles, K, **kw):
    return [Case(data, "q4", epi, M, tiles, K, **kw)]


CASES = (
    # ---- K classes, exact
    _d("int", "store", 1, "1", 32) + _q("int", "store", 1, "1", 128)            # one k-block: seven waves idle
    + _c("int", "store", 8, "3", 4096)                                          # exactly one full batch
    + _c("int", "store", 2, "3", 4224)                                          # J = 2, 16 threads own a second item
    + _c("int", "store_f32", 8, "3", 6144)                                      # J = 2, full second item
    + _c("int", "store", 7, "3", 6272)                                          # DB, two chunks, ragged last
    + _c("int", "store", 8, "cus+1", 8320)                                      # DB, three chunks (parity flips per tile), >= 2 tiles
    + _c("int", "store", 9, "3", 4224)                                          # 9..16 rows: single-buffered re-staging
    + _c("int", "store", 15, "cus+1", 4224)                                     # ... handing back to chunk 0 of a next tile
    + _c("int", "store", 16, "3", 4096)                                         # 9..16 rows: largest single chunk
    # ---- tiles per workgroup, exact
    + _c("int", "store", 7, "1", 256) + _c("int", "store", 2, "cus", 256) + _c("int", "store_f32", 1, "cus+1", 256)
    + _c("int", "store", 8, "2cus+1", 256) + _c("int", "store", 16, "2cus+1", 384)
    # ---- epilogues, exact
    + _c("int", "resid", 7, "cus+1", 512) + _c("int", "resid", 15, "2cus+1", 128) + _c("int", "resid", 8, "cus+1", 6272)
    # ---- strides: x and out are slabs of wider buffers
    + _c("int", "store", 7, "3", 4224, strides=True) + _c("int", "resid", 9, "2cus+1", 256, strides=True)
    + _c("int", "store_f32", 8, "3", 6272, strides=True)
    # ---- column selection
    + _d("onehot", "store", 3, "3", 32) + _q("onehot", "store", 3, "3", 128)
    + _c("onehot", "store", 8, "3", 4096) + _c("onehot", "store", 8, "3", 4224) + _c("onehot", "store", 8, "3", 6144)
    + _c("onehot", "store", 8, "3", 6272) + _c("onehot", "store", 8, "3", 8320) + _c("onehot", "store", 16, "3", 4224)
    + _c("onehot", "store", 16, "3", 4096, strides=True)
    # ---- paired-tile SwiGLU (the sums exact, the activation under the rule); every dense one also runs as GU8
    + _d("int", "swiglu", 7, "3", 2080)                                         # second SwiGLU batch holds one block
    + _c("int", "swiglu", 8, "cus+1", 512) + _c("int", "swiglu", 2, "3", 4224) + _c("int", "swiglu", 8, "3", 6144)
    + _c("int", "swiglu", 7, "2", 8320) + _c("int", "swiglu", 9, "3", 4224) + _c("int", "swiglu", 1, "2cus+1", 128)
    + _c("int", "swiglu", 15, "3", 512, strides=True)
    + _q("int", "swiglu", 16, "3", 4096)                                        # largest LDS footprint
    + _d("int", "swiglu", 16, "3", 4096)
    # ---- the row-interleaved gate|up copy (dense only): tiles of 8 output columns
    + _d("int", "gu8", 8, "cus+2", 512) + _d("int", "gu8", 7, "2cus+2", 128) + _d("int", "gu8", 2, "6", 4224)
    + _d("int", "gu8", 8, "6", 6272) + _d("int", "gu8", 16, "6", 4096) + _d("int", "gu8", 9, "2", 4224, strides=True)
    + _d("pair", "gu8", 8, "2", 64) + _d("pair", "gu8", 16, "6", 64) + _d("pair", "gu8", 8, "34", 4224)
    # ---- RMSNorm in front (random data, the rule): single chunk, J = 2, double-buffered chunks, re-staged chunks
    # (34 tiles: enough elements for a share of a fraction of a per cent to mean something)
    + _c("rand", "store", 8, "34", 512, pro=True) + _c("rand", "store", 7, "34", 4224, pro=True)
    + _c("rand", "store", 8, "34", 6144, pro=True) + _c("rand", "store_f32", 8, "34", 8320, pro=True)
    + _c("rand", "store", 15, "34", 4224, pro=True) + _c("rand", "resid", 2, "34", 6272, pro=True, strides=True)
)
assert len({(c.name, c.kind) for c in CASES}) == len(CASES)

# RMSNorm + SwiGLU on random data, the gate|up call of a real decode step: the paired-tile form and the row-interleaved copy
# must agree bit for bit (test_gu8_equals_paired_tile_swiglu).  They are under no rule: a gate sum that straddles a rounding
# boundary moves through sigmoid, g * sigmoid and * u, and the oracle's own float32 envelopes leave one unit there (1.3 units
# at 4224 columns, float16) -- the rule covers the activation on exact sums only.
PAIRED_EXTRA = (_d("rand", "swiglu", 8, "3", 4224, pro=True) + _d("rand", "swiglu", 7, "6", 8320, pro=True)
                + _d("rand", "swiglu", 16, "3", 4096, pro=True) + _d("rand", "swiglu", 9, "3", 4224, pro=True))


def case_id(c):
    return f"{c.kind}-{c.name}"


def classes_of(c, cus):
    """The classes of the issue's table that case c reaches on a device of `cus` compute units."""
    p = c.plan(cus)
    paired = c.epi == "swiglu"
    out = {f"m:{c.M}", f"e:{c.epi}"}
    if p.nchunks == 1 and c.K == p.BK:
        out.add("k:one-block")
    if p.nchunks == 1 and c.K == 4096 and c.M <= 8:
        out.add("k:one-full-batch")
    if paired and c.kind == "dense" and p.nchunks == 1 and c.K - p.KS == p.BK:
        out.add("k:swiglu-second-batch-one-block")
    if p.J == 2 and c.K // 8 - 512 == 16:
        out.add("k:j2-16-threads")
    if p.J == 2 and c.K == 6144:
        out.add("k:j2-full")
    if p.DB and p.nchunks == 2 and c.K % p.kc:
        out.add("k:db-2-ragged")
    if p.DB and p.nchunks == 3 and c.K - 2 * p.kc == 128 and p.tiles_first >= 2:
        out.add("k:db-3-odd-multi-tile")
    if p.MB == 16 and p.nchunks > 1:
        out.add("k:m16-restaging")
        if p.tiles_first >= 2:
            out.add("k:m16-restaging-multi-tile")
    if p.MB == 16 and c.K == 4096:
        out.add("k:m16-largest-chunk")
    if p.tiles == 1:
        out.add("t:1-on-1")
    if p.tiles == 3 and p.grid == 3:
        out.add("t:3-on-3")
    if p.tiles == cus:
        out.add("t:cus")
    if p.tiles == cus + 1:
        out.add("t:cus+1")
        assert (p.tiles_first, p.tiles_last) == (2, 1)
    if p.tiles == 2 * cus + 1:
        out.add("t:2cus+1")
        assert (p.tiles_first, p.tiles_last) == (3, 2)
    if p.TB == 2 and (p.tiles_first, p.tiles_last) == (2, 1):
        out.add("t:q4-full-batch-beside-half-empty")
    if p.TB == 2 and p.tiles_first == 3 and p.batches == 2:
        out.add("t:q4-full-then-half-empty")
    if c.epi == "resid" and p.tiles_first >= 2:
        out.add("e:resid-multi-tile")
    if c.pro:
        if p.nchunks == 1:
            out.add(f"p:norm-j{p.J}")
        elif p.DB:
            out.add("p:norm-db")
        else:
            out.add("p:norm-m16-chunks")
    if c.strides:
        out.add("s:strides")
    if c.M == 16 and c.K == 4096 and c.kind == "q4" and paired:
        out.add("l:largest-lds")
    if c.data == "onehot":
        out.add("x:onehot")
    return out


_COMMON = ({f"m:{m}" for m in (1, 2, 7, 8, 9, 15, 16)}
           | {"e:store", "e:store_f32", "e:resid", "e:resid-multi-tile", "e:swiglu", "s:strides", "x:onehot",
              "k:one-block", "k:one-full-batch", "k:j2-16-threads", "k:j2-full", "k:db-2-ragged", "k:db-3-odd-multi-tile",
              "k:m16-restaging", "k:m16-restaging-multi-tile", "k:m16-largest-chunk",
              "t:1-on-1", "t:3-on-3", "t:cus", "t:cus+1", "t:2cus+1",
              "p:norm-j1", "p:norm-j2", "p:norm-db", "p:norm-m16-chunks"})
REQUIRED = {
    "dense": _COMMON | {"k:swiglu-second-batch-one-block", "e:gu8"},
    "q4": _COMMON | {"t:q4-full-batch-beside-half-empty", "t:q4-full-then-half-empty", "l:largest-lds"},
}


# ---------------------------------------------------------------------------------------------------------------------------
# column selection: the probes

def edges(c, p):
    """Columns E with 0 < E < K at which something of the launch plan changes hands: a 16-byte piece, a k-block, the int4
    block / a wave's next block (BK), the batch (KS), the activation chunk (kc, 2 kc)."""
    return sorted({e for e in (8, 32, p.BK, p.KS, p.kc, 2 * p.kc) if 0 < e < c.K})


def probes(c, p):
    cols = [0, c.K - 1]
    for e in edges(c, p):
        cols += [e - 1, e]
    if p.J == 2:
        cols.append(c.K - 8)              # first column of the thread that owns the last second item
    return sorted(set(cols))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and expectations

def _rng(c, act, salt=0):
    return np.random.default_rng(zlib.crc32(f"{case_id(c)}/{act}/{salt}".encode()))


def _wexp(c):
    """Exact SwiGLU cases: weights times 2^-e so that the (still exact) gate and up sums have a deviation of about 4."""
    if c.epi not in ("swiglu", "gu8") or c.data != "int":
        return 0
    return int(round(np.log2(np.sqrt(c.K) * 5.16 / 4)))


def pack_q4(q):
    """Codes (N, K) in 0..15 -> MLX-packed uint32 (N, K / 8): element j of a word at bits [4 j, 4 j + 4)."""
    n, k = q.shape
    sh = (np.arange(8, dtype=np.uint32) * 4).astype(np.uint32)
    return np.bitwise_or.reduce(q.astype(np.uint32).reshape(n, k // 8, 8) << sh, axis=-1).astype(np.uint32)


def exact_q4(rng, N, K, e=0):
    """-> (packed, scales, biases) with scales 2^-e x {2^-3, 2^-2, 2^-1} and biases = scale x (-12..0), per (row, group)."""
    q = rng.integers(0, 16, (N, K), dtype=np.uint32)
    scales = np.exp2(rng.integers(-3, 0, (N, K // 64)) - e).astype(np.float32)
    biases = (scales * rng.integers(-12, 1, (N, K // 64))).astype(np.float32)
    return pack_q4(q), scales, biases


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for a in v:
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=3)
def build(c, act, cus):
    """-> dict(x (launches, M, K), w (rows, K) float32 = what the oracle multiplies with, q = (packed, scales, biases) or
    None, h (M, N) or None, nw (K,) or None, want (launches, M, N), N, rows).  Nothing in it is writable."""
    rng = _rng(c, act)
    N, rows, K, M = c.width(cus), c.wrows(cus), c.K, c.M
    p = c.plan(cus)
    q = None
    if c.data == "rand":
        x = round_to(rng.standard_normal((1, M, K)).astype(np.float32), act)
        w = round_to(rng.standard_normal((rows, K)).astype(np.float32) * 0.05, act)
        if c.kind == "q4":
            q = ref_quant.quantize(w, 64, 4, act)
            w = ref_quant.dequantize(*q, 64, 4)
    elif c.data == "pair":
        n, k = np.arange(rows)[:, None], np.arange(K)[None, :]
        w = np.where(n < N, np.exp2(5 + (n + k) % 4), 2 * ((7 * n + 3 * k) % 64) + 1).astype(np.float32)
        cols = probes(c, p)
        x = np.zeros((-(-len(cols) // M), M, K), np.float32)
        for i in range(x.shape[0] * M):
            x[i // M, i % M, cols[i % len(cols)]] = 1.0
    else:
        e = _wexp(c)
        if c.kind == "q4":
            q = exact_q4(rng, rows, K, e)
            w = ref_quant.dequantize(*q, 64, 4)
        else:
            w = (rng.integers(-4, 5, (rows, K)) * np.exp2(-e)).astype(np.float32)
        if c.data == "int":
            x = rng.integers(-3, 4, (1, M, K)).astype(np.float32)
        else:
            cols = probes(c, p)
            x = np.zeros((-(-len(cols) // M), M, K), np.float32)
            for i in range(x.shape[0] * M):
                x[i // M, i % M, cols[i % len(cols)]] = 1.0
    nw = round_to(1.0 + 0.1 * rng.standard_normal(K).astype(np.float32), act) if c.pro else None
    h = None
    if c.epi == "resid":
        h = (rng.integers(-8, 9, (M, N)).astype(np.float32) if c.data != "rand"
             else round_to(rng.standard_normal((M, N)).astype(np.float32), act))
    d = dict(x=x, w=w, q=q, h=h, nw=nw, N=N, rows=rows)
    d["want"] = oracle(c, act, d)
    return _freeze(d)


def oracle(c, act, d):
    """The float64 oracle with the reference's rounding points, under the oracle's CURRENT accumulation mode."""
    x, w, N = d["x"], d["w"], d["N"]
    if c.pro:
        x, _ = ref_model.rms_norm(x, act, d["nw"], act, EPS)
    if c.epi in ("swiglu", "gu8"):
        g = round_to(matmul_nt(x, w[:N]), act)
        u = round_to(matmul_nt(x, w[N:]), act)
        sig = round_to(1.0 / (1.0 + np.exp(-g.astype(np.float64))), act)
        return round_to(round_to(g * sig, act) * u, act)
    y = round_to(matmul_nt(x, w), act)
    if c.epi == "resid":
        return round_to(d["h"][None] + y, act)
    return y


def onehot_want(c, d):
    """What column selection means, without a product: output row m of launch l is column cols[l][m] of W."""
    x, w = d["x"], d["w"]
    cols = x.argmax(axis=-1)
    assert (x.sum(axis=-1) == 1).all() and (x.max(axis=-1) == 1).all()
    if c.data == "pair":
        N = d["N"]
        return (w[:N].T[cols] * w[N:].T[cols]).astype(np.float32)
    return w.T[cols]


def assert_rule(got, want, act, what=""):
    worst, frac = rule_stats(got, want, act)
    print(f"RULE {what}: worst {worst:.3f} unit, {100 * frac:.4f} % beyond half a unit (cap {100 * RULE_CAP:.4f} %)")
    assert np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst)
    assert frac <= RULE_CAP, (what, frac)
    return worst, frac
