"""Inputs, expectations and the acceptance rule of the 16-bit attention tests: tests/test_gpu_attn_16bit.py runs them on the
device, tests/test_attn_16bit_cases.py checks without one what does not need it (the one-hot constructions against the
float64 oracle, the coverage of the probes, the reference's own envelopes under the rule).  NumPy and the oracle only.

One-hot constructions.  With a query of one non-zero element and keys of one non-zero element, a head's scores are 0 but for
the keys whose hot dimension is the query's; the gaps are so large (>= 260 in the exp2 domain) that exp2 of the difference is
0 in float32, so every softmax weight is 0 or 1 and an output row IS one V row, bit for bit.  All values (64, 128, 32 k) are
exact in bfloat16 and float16.
"""
from __future__ import annotations

import numpy as np

from oracle import ref_model
from oracle.numerics import round_to

UNIT = {"bfloat16": 2.0 ** -7, "float16": 2.0 ** -10}


# ---------------------------------------------------------------------------------------------------------------------------
# the rule of the random-data tests

def rule_stats(got, want, dtype):
    """-> (worst element, fraction of elements beyond half a unit), in units of 2^-7 (bfloat16) / 2^-10 (float16) times
    max(|want|, |got|, rms(want)) -- the unit of test_gpu_kernels._assert_close, with the RMS taken per output row (the last
    axis: one query's Hq x D outputs).  Rows of a case differ in their number of keys and with it in magnitude -- one key
    gives a V row, 1100 keys a mean of 1100 -- and an RMS over the whole case would be the short rows' and hide the long
    ones.  A non-finite `got` is infinitely far."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rms = np.sqrt(np.mean(np.square(want), axis=-1, keepdims=True)) + 1e-12
    with np.errstate(invalid="ignore"):
        unit = UNIT[dtype] * np.maximum(np.maximum(np.abs(want), np.abs(got)), rms)
        r = np.abs(got - want) / unit
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max()), float(np.mean(~(r <= 0.5)))


def assert_rule(got, want, dtype, what=""):
    """Every output finite; every element within 1 unit (got and want are both values of the dtype: a sum that straddles a
    rounding boundary moves the result one step, and one step is at most one unit); at most 2 % of the elements beyond half
    a unit (the oracle's float32-accumulating envelopes stay below 0.1 % on these inputs, a kernel that rounds P to one
    16-bit value is above 4 %: tests/test_attn_16bit_cases.py)."""
    worst, frac = rule_stats(got, want, dtype)
    print(f"RULE {what}: worst {worst:.3f} unit, {100 * frac:.3f} % beyond half a unit")
    assert np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst)
    assert frac <= 0.02, (what, frac)
    return worst, frac


# ---------------------------------------------------------------------------------------------------------------------------
# prefill: exact key selection and the causal edge

PREFILL_L = 50                       # three full 16-query tiles and a ragged one of two queries
PREFILL_OFFS = [0, 14, 31, 207]      # off + t0 = 0, 30, 31, 63 (mod 32): both sides of the diagonal-block condition
PREFILL_CAP = 288


def prefill_probes(D):
    """Distances of the probed key from the query's own position; "masked": the class of the first masked key."""
    return ["masked", 0, 1, 2, D // 2, 3, 5, 7, 15, 17, 31]


def prefill_one_hot(Hq, Hkv, D, act, seed=7):
    """K[b, kh, pos, (pos + 3 kh) % D] = 32 + 32 (pos // D) over the WHOLE cache (positions past off + L too), q = 64 e_r:
    among the keys of residue class r the latest visible one has the largest score, by >= 32 x 64 x scale x log2(e) >= 260.
    The probe of (b, t, h) picks r: the key `dist` positions back (its class has no later visible member since dist < D),
    or the class of the first masked key off + t + 1, whose winner is off + t + 1 - D -- a mask that lets one key through
    selects the masked key (larger magnitude) and returns the wrong V row.  A probe whose key does not exist (before the
    start of the row) is not chosen; distance 0 always exists."""
    B, L, G, cap = len(PREFILL_OFFS), PREFILL_L, Hq // Hkv, PREFILL_CAP
    probes = prefill_probes(D)
    assert all(p == "masked" or p < D for p in probes)
    rng = np.random.default_rng(seed + Hq + D)
    pos = np.arange(cap)
    k = np.zeros((B, Hkv, cap, D), np.float32)
    for kh in range(Hkv):
        k[:, kh, pos, (pos + 3 * kh) % D] = 32.0 + 32.0 * (pos // D)
    v = round_to(rng.standard_normal((B, Hkv, cap, D)).astype(np.float32), act)
    q = np.zeros((B, L, Hq, D), np.float32)
    want = np.zeros((B, L, Hq, D), np.float32)
    winner = np.zeros((B, L, Hq), np.int64)
    reached, dtiles, masked_last = set(), set(), set()
    uses = [[0] * len(probes) for _ in range(16)]
    for b, off in enumerate(PREFILL_OFFS):
        for t in range(L):
            for h in range(Hq):
                kh, g, qpos = h // G, h % G, off + t
                # among the probes whose key exists, the one this query slot has seen least (ties: rotating with h and t)
                valid = [i for i, p in enumerate(probes) if (qpos + 1 - D if p == "masked" else qpos - p) >= 0]
                i = min(valid, key=lambda i: (uses[t % 16][i], (i - h - t) % len(probes)))
                if t == L - 1 and g % 2 == 0 and 0 in valid:
                    i = 0                                  # the last query: the first masked key lies beyond off + L
                uses[t % 16][i] += 1
                probe = probes[i]
                target = qpos + 1 - D if probe == "masked" else qpos - probe
                r = (target + 3 * kh) % D
                q[b, t, h, r] = 64.0
                want[b, t, h] = v[b, kh, target]
                winner[b, t, h] = target
                reached.add((probe, t % 16))
                dtiles.add(r // 16)
                if probe == "masked" and t == L - 1:
                    masked_last.add(b)
    for a in (q, k, v, want, winner):
        a.setflags(write=False)
    return dict(q=q, k=k, v=v, want=want, winner=winner, reached=reached, dtiles=dtiles, masked_last=masked_last)


def assert_prefill_coverage(c, D):
    """Every probe ran in every query slot of a tile, every 16-wide d tile was hit, and the first-masked probe ran for the
    last query of every row whose class has a visible member (off + L >= D; the longest row always has one)."""
    assert c["reached"] >= {(p, c16) for p in prefill_probes(D) for c16 in range(16)}
    assert c["dtiles"] == set(range(D // 16))
    rows = {b for b, off in enumerate(PREFILL_OFFS) if off + PREFILL_L - D >= 0}
    assert rows and c["masked_last"] == rows, (rows, c["masked_last"])


def prefill_oracle(q, k, v, offs, L, D, act):
    """The float64 oracle over a cache that already holds the call's keys: -> (B, L, Hq, D)."""
    out = []
    for b, off in enumerate(offs):
        n = off + L
        mask = ref_model.create_additive_causal_mask_variable(L, [off], n)
        o, _ = ref_model.sdpa(q[b:b + 1].transpose(0, 2, 1, 3), k[b:b + 1, :, :n], v[b:b + 1, :, :n], D ** -0.5, mask, act, act)
        out.append(o[0].transpose(1, 0, 2))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------
# fused decode: exact key selection, the split cut, stale rows

DECODE_POS = [0, 1, 2, 5, 31, 32, 33, 255, 256, 257, 300, 1099]      # cached keys per row
DECODE_CAP = 1108


def decode_candidates(pos, nsplit):
    """Keys that exercise every place of both kernels' walk over a row of `pos` cached keys: both sides of every cut of the
    matrix-core kernel (chunk = ceil(pos / nsplit), not tile-aligned) and of the VALU kernel (ceil((pos + 1) / nsplit): it
    cuts the new key with the others); in the first and the last split a key in each of the eight waves' 32-key spans of a
    round and a key of the second round; the last cached key; the new key."""
    keys = []

    def add(k, lo, hi):
        if lo <= k < hi and k not in keys:
            keys.append(k)

    chunk = -(-pos // nsplit)
    for sp in range(nsplit):
        s0, send = sp * chunk, min(sp * chunk + chunk, pos)
        add(s0, s0, send)
        add(send - 1, s0, send)
        if sp in (0, nsplit - 1):
            for w in range(8):
                add(s0 + 32 * w + (7 * w + 3) % 32, s0, send)
            add(s0 + 256 + 32 + 9, s0, send)
    chunk = -(-(pos + 1) // nsplit)
    for sp in range(nsplit):
        s0, s1 = sp * chunk, min(sp * chunk + chunk, pos + 1)
        add(s0, 0, pos)
        add(s1 - 1, 0, pos)
    add(pos - 1, 0, pos)
    return keys + [pos]


def decode_launches(Hq, Hkv, D, nsplit):
    """-> (candidates per row, [(key[b][h], d[b][h]) per launch]): as many launches as it takes for every candidate key of
    every row to have had a head.  d: the hot dimension of (b, h), distinct within a GQA group (37 is odd: 37 g mod 32 / 64 /
    128 differ for g < 8) and moving with the launch."""
    G, B = Hq // Hkv, len(DECODE_POS)
    cand = [decode_candidates(pos, nsplit) for pos in DECODE_POS]
    launches = []
    for p in range(-(-max(len(c) for c in cand) // Hq)):
        key = np.array([[cand[b][(p * Hq + h) % len(cand[b])] for h in range(Hq)] for b in range(B)])
        d = np.array([[(5 * (b * Hkv + h // G) + 37 * (h % G) + 3 * p) % D for h in range(Hq)] for b in range(B)])
        launches.append((key, d))
    return cand, launches


def assert_decode_coverage(cand, launches, D):
    """The sweep reached every candidate key of every row, every 16-wide d tile and every place of a lane's 16 elements."""
    seen = {(b, int(k)) for key, _ in launches for b, row in enumerate(key) for k in row}
    assert seen == {(b, k) for b, c in enumerate(cand) for k in c}
    ds = {int(x) for _, d in launches for x in d.ravel()}
    assert {x // 16 for x in ds} == set(range(D // 16)) and {x % 16 for x in ds} == set(range(16))


def decode_values(Hkv, D, act, seed=99):
    """The V cache and the new value rows of the one-hot decode test (random, values of the dtype; shared by the launches)."""
    rng = np.random.default_rng(seed + D)
    B = len(DECODE_POS)
    vc = round_to(rng.standard_normal((B, Hkv, DECODE_CAP, D)).astype(np.float32), act)
    vnew = round_to(rng.standard_normal((B, Hkv * D)).astype(np.float32), act)
    vc.setflags(write=False)
    vnew.setflags(write=False)
    return vc, vnew


def decode_one_hot(Hq, Hkv, D, key, d, vc, vnew, after=True):
    """One launch: q[b, h] = 64 e_d, K[b, kh, key, d] = 64 (the new key: in the q|k|v row), everything else 0 -- but for the
    STALE rows: the cache rows at pos and pos + 1 hold the head's hot dimension at magnitude 128, as a reused cache row may.
    Row pos must be overwritten by the new K / V; a kernel that scores it instead of the new key in registers, or reads one
    key too far, picks the decoy.  -> (q|k|v rows, K cache, expected output rows[, expected K cache, expected V cache: the
    new rows at pos])."""
    G, B = Hq // Hkv, len(DECODE_POS)
    kc = np.zeros((B, Hkv, DECODE_CAP, D), np.float32)
    qkv = np.zeros((B, (Hq + 2 * Hkv) * D), np.float32)
    qkv[:, (Hq + Hkv) * D:] = vnew
    want = np.zeros((B, Hq, D), np.float32)
    for b, pos in enumerate(DECODE_POS):
        for h in range(Hq):
            kh, dd, kk = h // G, int(d[b, h]), int(key[b, h])
            qkv[b, h * D + dd] = 64.0
            kc[b, kh, pos, dd] = kc[b, kh, pos + 1, dd] = 128.0
            if kk == pos:
                qkv[b, (Hq + kh) * D + dd] = 64.0
                want[b, h] = vnew[b, kh * D:(kh + 1) * D]
            else:
                kc[b, kh, kk, dd] = 64.0
                want[b, h] = vc[b, kh, kk]
    if not after:
        return qkv, kc, want
    kc_after, vc_after = kc.copy(), vc.copy()
    for b, pos in enumerate(DECODE_POS):
        kc_after[b, :, pos] = qkv[b, Hq * D:(Hq + Hkv) * D].reshape(Hkv, D)
        vc_after[b, :, pos] = vnew[b].reshape(Hkv, D)
    return qkv, kc, want, kc_after, vc_after


# ---------------------------------------------------------------------------------------------------------------------------
# random data against the float64 oracle

# (Hq, Hkv, D, q/k norm): geometries without a kernel-level case in test_gpu_kernels.py
RANDOM_GEOMS = [(4, 2, 128, True), (2, 2, 128, False), (8, 1, 64, True), (10, 2, 64, False), (4, 2, 64, False),
                (2, 2, 32, False), (4, 2, 32, False), (8, 2, 32, False)]
RANDOM_DECODE_LENS = [0, 2, 37, 255, 256, 1100]
RANDOM_PREFILL_L = [2, 17, 50]
RANDOM_PREFILL_OFFS = [0, 31, 207]
RANDOM_PREFILL_CAP = 264
EPS = 1e-6


def rope_base(norm):
    return 1e6 if norm else 1e4


def random_inputs(Hq, Hkv, D, act, B, L, rows, cap, seed):
    """`rows` cache rows of random K / V, B x L q|k|v rows and the q / k norm weights, all values of the dtype."""
    rng = np.random.default_rng(seed + 1000 * Hq + 10 * D + L + (0 if act == "bfloat16" else 1))
    nqkv = (Hq + 2 * Hkv) * D
    inp = dict(kc=round_to(rng.standard_normal((rows, Hkv, cap, D)).astype(np.float32), act),
               vc=round_to(rng.standard_normal((rows, Hkv, cap, D)).astype(np.float32), act),
               qkv=round_to(rng.standard_normal((B, L, nqkv)).astype(np.float32), act),
               qn=round_to(1 + 0.1 * rng.standard_normal(D).astype(np.float32), act),
               kn=round_to(1 + 0.1 * rng.standard_normal(D).astype(np.float32), act))
    for a in inp.values():
        a.setflags(write=False)
    return inp


def attention_oracle(inp, Hq, Hkv, D, act, norm, offs, rows=None):
    """q / k norm + RoPE + append + attention under the oracle's CURRENT accumulation mode (oracle.numerics): batch entry b
    lives in cache row rows[b] (default b) and holds offs[b] keys.  -> (outputs (B, L, Hq D), K cache, V cache)."""
    qkv = inp["qkv"]
    B, L = qkv.shape[:2]
    rows = list(range(B)) if rows is None else rows
    max_pos = max(offs) + L + 8
    c_ref, s_ref = ref_model.rope_tables(D, rope_base(norm), 1.0, max_pos)
    q = qkv[..., :Hq * D].reshape(B, L, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, L, Hkv, D)
    v = qkv[..., (Hq + Hkv) * D:].reshape(B, L, Hkv, D).transpose(0, 2, 1, 3)
    if norm:
        q, _ = ref_model.rms_norm(q, act, inp["qn"], act, EPS)
        k, _ = ref_model.rms_norm(k, act, inp["kn"], act, EPS)
    pos = np.array([[o + t for t in range(L)] for o in offs])
    q = ref_model.rope(q.transpose(0, 2, 1, 3), act, pos, c_ref, s_ref)
    k = ref_model.rope(k.transpose(0, 2, 1, 3), act, pos, c_ref, s_ref)
    kc, vc = inp["kc"].copy(), inp["vc"].copy()
    want = np.zeros((B, L, Hq * D), np.float32)
    for b, (r, off) in enumerate(zip(rows, offs)):
        kc[r, :, off:off + L] = k[b]
        vc[r, :, off:off + L] = v[b]
        n = off + L
        mask = ref_model.create_additive_causal_mask_variable(L, [off], n) if L > 1 else None
        o, _ = ref_model.sdpa(q[b:b + 1], kc[r:r + 1, :, :n], vc[r:r + 1, :, :n], D ** -0.5, mask, act, act)
        want[b] = o[0].transpose(1, 0, 2).reshape(L, Hq * D)
    return want, kc, vc


# ---------------------------------------------------------------------------------------------------------------------------
# cache-row and length lookups (mi_op_attention_decode_host)

LOOKUP_GEOMS = [(8, 2, 128), (5, 1, 64)]
LOOKUP_LENS = [0, 2, 31, 32, 33, 255, 256, 300]         # cached keys of batch entry b
LOOKUP_ROWS = [7, 2, 11, 0, 5, 9, 3, 6]                 # ... which lives in this row of a 12-row cache
LOOKUP_NROWS = 12
LOOKUP_CAP = 308


def check_new_rows(gk, gv, kc_ref, vc_ref, rows, lens, act):
    """The V cache and every K row but the new ones: exactly the oracle's; the new K row (norm + RoPE in float32 against the
    oracle's float64): within 2 units of max(|want|, 2), the worst-element bound test_gpu_kernels.py holds for it."""
    assert np.array_equal(gv, vc_ref)
    for r, n in zip(rows, lens):
        err = np.abs(gk[r, :, n] - kc_ref[r, :, n])
        assert np.all(err <= 2 * UNIT[act] * np.maximum(np.abs(kc_ref[r, :, n]), 2.0)), (r, n, float(err.max()))
        gk[r, :, n] = kc_ref[r, :, n]
    assert np.array_equal(gk, kc_ref)
