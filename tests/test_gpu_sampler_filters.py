"""-m gpu: the sampler's top-k / min-p controls and per-row random streams at kernel level (``mi_op_sample_ex``), against the
CPU definition of tests/sampler_filters_ref.py (built from the oracle).  Semantics: DESIGN.md §2."""
import math

import numpy as np
import pytest
import torch

import sampler_filters_ref as sfr
from sampler_filters_ref import _nucleus_cut_slack, _sampler_edge_bound
from oracle import ref_sample
from oracle.numerics import round_to

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_i32, ptr  # noqa: E402

B = 8
U_LAST = 1.0 - 2.0 ** -24                  # the largest float32 below 1: the draw that must land on the last kept candidate
VS = [37, 5000, 32000, 151936]             # 37: the scalar path (V % 4 != 0); 32000: bf16-rounded, big tie groups; 151936: largest
# either side of the tie table's capacity (64 chunks of 1024 lanes): 65535 (scalar walk) and 262144 (vector walk) fill it exactly,
# 65537 and 262148 need a 65th chunk and take the rank loop
EDGE_VS = [65535, 65537, 262144, 262148]


def _dev_i64(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.int64)).cuda().contiguous()


def run_ex(lg, temp=1.0, top_p=1.0, top_k=0, min_p=0.0, u=None, row_params=None, row_top_k=None, row_min_p=None,
           streams=None, seed=0, step=0, k=0, plain=False):
    """One launch of mi_op_sample_ex (plain: of mi_op_sample, which has only temp / top_p / u / k) -> dict of host arrays."""
    lg = np.asarray(lg, np.float32)
    n, V = lg.shape
    t = dev(lg)
    ud = dev(np.asarray(u, np.float32)) if u is not None else None
    rt, rp = (dev(np.asarray(row_params[0], np.float32)), dev(np.asarray(row_params[1], np.float32))) if row_params else (None, None)
    rk = dev_i32(row_top_k) if row_top_k is not None else None
    rm = dev(np.asarray(row_min_p, np.float32)) if row_min_p is not None else None
    rs, rq = (_dev_i64(streams[0], np.uint64), _dev_i64(streams[1], np.int64)) if streams else (None, None)
    toks = torch.zeros(n, dtype=torch.int32, device="cuda")
    lp = torch.zeros(n, dtype=torch.float32, device="cuda")
    p0 = torch.zeros(n, dtype=torch.float32, device="cuda")
    ki = torch.zeros((n, max(k, 1)), dtype=torch.int32, device="cuda")
    kl = torch.zeros((n, max(k, 1)), dtype=torch.float32, device="cuda")
    st = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if plain:
        L.check(L.lib().mi_op_sample(ptr(t), n, V, temp, top_p, ptr(ud), k, ptr(toks), ptr(lp), ptr(p0), ptr(ki), ptr(kl), ptr(st)))
    else:
        L.check(L.lib().mi_op_sample_ex(ptr(t), n, V, temp, top_p, top_k, min_p, ptr(rt), ptr(rp), ptr(rk), ptr(rm), ptr(rs),
                                        ptr(rq), seed, step, ptr(ud), k, ptr(toks), ptr(lp), ptr(p0), ptr(ki), ptr(kl), ptr(st)))
    return {"tokens": toks.cpu().numpy(), "logprobs": lp.cpu().numpy(), "probs_row0": p0.cpu().numpy(),
            "top_ids": ki.cpu().numpy(), "top_logprobs": kl.cpu().numpy(), "row_stats": st.cpu().numpy()}


def make_rows(V, rng, n=B):
    lg = (rng.standard_normal((n, V)) * (1.3 if V == 32000 else 3.0)).astype(np.float32)
    return round_to(lg, "bfloat16") if V == 32000 else lg


def masked(row, top_k):
    """The row with everything outside the top-k prefix at -inf (what the nucleus is taken over)."""
    out = np.array(row, np.float32, copy=True)
    if 0 < top_k < len(out):
        out[sfr.oracle_order(out)[top_k:]] = -np.inf
    return out


def _min_p_ambiguous(row, temp, min_p):
    """The device tests a_i = (l_i - max) * (1/T) >= logf(min_p) in float32: the roundings of l - max, 1/T and the product
    (and T itself, a float32 there) are 5.5 half-ulps relative on a_i like the argument of the mass, and logf(min_p) is within
    half an ulp of a value below 8, i.e. 4 * 2^-24.  A candidate within (5.5 |a_i| + 4) 2^-24 nats of ln(min_p) may fall on
    either side."""
    if min_p <= 0.0:
        return False
    a = (row.astype(np.float64) - float(row.max())) / float(temp)
    return bool(np.any(np.abs(a - math.log(min_p)) <= (5.5 * np.abs(a) + 4.0) * 2.0 ** -24))


def unambiguous_rows(V, rng, temp, top_p, top_k, min_p, n=B):
    """n logits rows whose nucleus cut (over the top-k survivors) and min-p threshold are not within the device's rounding of
    a candidate; ambiguous rows are redrawn, at most 50 times in all."""
    rows, redraws = [], 0
    while len(rows) < n:
        row = make_rows(V, rng, 1)[0]
        ids, _ = sfr.kept_candidates(row, temp, top_p, top_k, 0.0)
        if _nucleus_cut_slack(masked(row, top_k), temp, top_p, len(ids)) != 0.0 or _min_p_ambiguous(row, temp, min_p):
            redraws += 1
            if redraws > 50:
                pytest.fail("more than 50 redraws for rows with an unambiguous cut")
            continue
        rows.append(row)
    return np.stack(rows)


def check_against_reference(lg, temp, top_p, top_k, min_p, rng):
    """u = 1 - 2^-24 draws the reference's last kept id; every draw lies in the reference's kept set; random u draws the
    reference's pick, or a neighbouring candidate with u within the derived bound of the edge (at most one such row).
    (The last kept id: where its share of the kept mass is at least 2^-23.  A candidate with a smaller share lies beyond what
    u * mass(kept) reaches with the largest float32 u -- the reference's own inverse-CDF pick does not reach it either -- and
    the draw at that u then follows the rule for any other u.)"""
    n = len(lg)
    cands = [sfr.kept_candidates(row, temp, top_p, top_k, min_p) for row in lg]
    got_last = run_ex(lg, temp, top_p, top_k, min_p, u=np.full(n, U_LAST))["tokens"]
    reach = [bool(pr[-1] >= 2.0 ** -23) for _, pr in cands]
    last = [int(ids[-1]) for ids, _ in cands]
    print("last kept:", got_last.tolist(), last, reach, "kept counts:", [len(ids) for ids, _ in cands])
    assert [g for g, r in zip(got_last.tolist(), reach) if r] == [w for w, r in zip(last, reach) if r]
    u = rng.random(n)
    got = run_ex(lg, temp, top_p, top_k, min_p, u=u)["tokens"]
    pairs = [(b, got[b], float(u[b])) for b in range(n)] + [(b, got_last[b], U_LAST) for b in range(n) if not reach[b]]
    mism = 0
    for b, tok, ub in pairs:
        ids, pr = cands[b]
        assert tok in set(ids.tolist()), (b, int(tok), len(ids))
        want = ref_sample.inverse_cdf_pick(ids, pr, ub)
        if tok != want:
            cum = np.cumsum(pr)
            rw, rg = int(np.where(ids == want)[0][0]), int(np.where(ids == tok)[0][0])
            j = min(rw, rg)
            with np.errstate(divide="ignore", invalid="ignore"):
                bound = _sampler_edge_bound(masked(lg[b], top_k), temp, top_p, ids, pr, j, ub)
            print("edge row", b, rw, rg, ub, float(cum[j]), bound)
            assert abs(rw - rg) == 1 and abs(ub - cum[j]) <= bound, (b, rw, rg, ub, cum[j], bound)
            mism += 1
    assert mism <= 1, (got.tolist(), mism)


# ---- 1. ruler rows: all logits equal, every mass exactly 2^40, ties by ascending id -- no tolerance
@pytest.mark.parametrize("k", [1, 2, 3, 64, 1000, 4095])
def test_top_k_on_a_ruler_row_is_exact(k):
    rng = np.random.default_rng(100 + k)
    u = np.concatenate([[0.0, 0.5, U_LAST], rng.random(B - 3)]).astype(np.float32)
    got = run_ex(np.zeros((B, 4096), np.float32), 1.0, 1.0, top_k=k, u=u)["tokens"]
    want = [int(math.floor(float(x) * k)) for x in u]            # float32(u) * k is exact in float64
    assert got.tolist() == want


# ---- 2. top-k on real rows
TOP_KS = [1, 2, 7, 64, 257, 1000]


@pytest.mark.parametrize("V", VS)
def test_top_k_matches_the_reference(V):
    rng = np.random.default_rng(1)
    lg = make_rows(V, rng)
    srt = -np.sort(-lg, axis=1)
    cuts = [k for k in TOP_KS if k < V and np.any(srt[:, k - 1] == srt[:, k])]     # k that cut inside a tie group, in some row
    print("V", V, "top_k values that cut a tie group:", cuts)
    if V == 32000:
        assert cuts, "the bf16-rounded rows must make at least one top_k cut a tie group"
    for k in TOP_KS:
        check_against_reference(lg, 1.0, 1.0, k, 0.0, rng)


# ---- 3. top-k, then the nucleus over the survivors (cut against top_p * Z_k)
@pytest.mark.parametrize("V", VS + EDGE_VS)
@pytest.mark.parametrize("k,top_p,temp", [(50, 0.9, 0.7), (5, 0.3, 1.0)])
def test_top_k_then_top_p(V, k, top_p, temp):
    rng = np.random.default_rng(300 + V + k)
    lg = unambiguous_rows(V, rng, temp, top_p, k, 0.0)
    check_against_reference(lg, temp, top_p, k, 0.0, rng)


# ---- 4. min-p
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("temp,min_p", [(1.0, 0.05), (0.7, 0.2), (1.3, 0.01)])
def test_min_p_matches_the_reference(V, temp, min_p):
    rng = np.random.default_rng(400 + V + int(100 * temp))
    lg = unambiguous_rows(V, rng, temp, 1.0, 0, min_p)
    check_against_reference(lg, temp, 1.0, 0, min_p, rng)


@pytest.mark.parametrize("binder,top_k,top_p,min_p", [("top_k", 5, 0.99, 1e-4), ("top_p", 1000, 0.3, 1e-4), ("min_p", 1000, 0.99, 0.3)])
def test_all_three_controls_each_binding_once(binder, top_k, top_p, min_p):
    """One row, the three controls on together.  Taken alone, the named control keeps strictly fewer candidates than either of
    the others (with top-k on, the nucleus is one of its survivors, so it is never longer than top_k); the kept set is the
    shortest of the nucleus of the top-k survivors and the min-p prefix."""
    V, temp = 5000, 1.0
    lg = unambiguous_rows(V, np.random.default_rng(44), temp, top_p, top_k, min_p, n=1)
    row = lg[0]
    alone = {"top_k": top_k, "top_p": len(sfr.kept_candidates(row, temp, top_p, 0, 0.0)[0]),
             "min_p": len(sfr.kept_candidates(row, temp, 1.0, 0, min_p)[0])}
    n_pk = len(sfr.kept_candidates(row, temp, top_p, top_k, 0.0)[0])             # nucleus of the top-k survivors
    n_all = len(sfr.kept_candidates(row, temp, top_p, top_k, min_p)[0])
    print(binder, alone, n_pk, n_all)
    assert min(alone, key=alone.get) == binder and sorted(alone.values())[0] < sorted(alone.values())[1]
    assert n_all == min(n_pk, alone["min_p"]) <= alone[binder]
    check_against_reference(np.repeat(lg, B, axis=0), temp, top_p, top_k, min_p, np.random.default_rng(45))


# ---- 5. per-row arrays
def test_per_row_controls_equal_single_row_launches():
    rng = np.random.default_rng(5)
    row = round_to((rng.standard_normal((1, 32000)) * 1.3).astype(np.float32), "bfloat16")
    params = [(1.0, 1.0, 0, 0.0), (0.7, 0.9, 0, 0.0), (1.0, 1.0, 7, 0.0), (1.3, 1.0, 0, 0.05), (0.7, 0.9, 50, 0.0),
              (1.0, 0.3, 5, 0.2), (0.0, 1.0, 3, 0.5), (1.5, 0.95, 1000, 0.01)]          # (T, top_p, top_k, min_p); one greedy row
    u = rng.random(B).astype(np.float32)
    together = run_ex(np.repeat(row, B, axis=0), u=u, row_params=([p[0] for p in params], [p[1] for p in params]),
                      row_top_k=[p[2] for p in params], row_min_p=[p[3] for p in params])
    alone = [run_ex(row, p[0], p[1], p[2], p[3], u=u[i:i + 1]) for i, p in enumerate(params)]
    assert together["tokens"].tolist() == [int(a["tokens"][0]) for a in alone]
    assert np.array_equal(together["logprobs"], np.concatenate([a["logprobs"] for a in alone]))
    assert together["tokens"][6] == int(np.argmax(row[0]))
    assert len(set(together["tokens"].tolist())) > 2              # the settings do make a difference on this row


# ---- 6. streams: on a ruler row of 4096 equal logits the token is floor(u * 4096), i.e. the top 12 bits of the uniform
RULER = np.zeros((1, 4096), np.float32)


def test_row_streams_do_not_depend_on_the_slot():
    s, p = 0x1234567890ABCDEF, 41
    base = int(run_ex(RULER, seed=s, step=p)["tokens"][0])                       # call-wide (s, p), row 0 of B = 1
    seeds = [11, 12, 13, 14, 15, s, 17, 18]
    pos = [0, 5, 41, 7, 41, p, 2, 41]
    at5 = run_ex(np.repeat(RULER, 8, axis=0), seed=999, step=3, streams=(seeds, pos))["tokens"]
    at0 = run_ex(np.repeat(RULER, 3, axis=0), seed=555, step=9, streams=([s, 21, 22], [p, 41, 0]))["tokens"]
    assert int(at5[5]) == base and int(at0[0]) == base
    assert len(set(at5.tolist())) > 4                             # other seeds / positions draw other values
    # a row with position -1 keeps the call-wide stream (seed, step, b)
    callwide = run_ex(np.repeat(RULER, 8, axis=0), seed=999, step=3)["tokens"]
    mixed = run_ex(np.repeat(RULER, 8, axis=0), seed=999, step=3, streams=(seeds, [-1, 5, -1, 7, -1, p, -1, -1]))["tokens"]
    for b in (0, 2, 4, 6, 7):
        assert mixed[b] == callwide[b]
    assert int(mixed[5]) == base and mixed[1] == at5[1] and mixed[3] == at5[3]
    # injected uniforms override both streams
    u = np.random.default_rng(6).random(8).astype(np.float32)
    inj = run_ex(np.repeat(RULER, 8, axis=0), seed=999, step=3, streams=(seeds, pos), u=u)["tokens"]
    assert inj.tolist() == [int(math.floor(float(x) * 4096)) for x in u]


def test_one_seed_gives_a_uniform_stream_over_positions():
    """4096 consecutive positions of one seed, read off ruler rows.  The mean of 4096 uniforms has standard deviation
    1 / sqrt(12 * 4096): within 4 of them (the 2^-13 of reading only 12 bits is far below that).  Neighbouring positions draw
    the same 12-bit token with probability 2^-12 each: 4095 pairs give about one repeat (Poisson, mean 1) -- more than 8 has
    probability below 1e-6."""
    n = 4096
    ruler = np.zeros((1024, 4096), np.float32)                    # (four launches of 1024 rows, the positions in order)
    got = np.concatenate([run_ex(ruler, seed=1, step=0, streams=([77] * 1024, list(range(i, i + 1024))))["tokens"]
                          for i in range(0, n, 1024)])
    mean = float(np.mean((got + 0.5) / 4096.0))
    repeats = int(np.sum(got[1:] == got[:-1]))
    print("mean", mean, "neighbour repeats", repeats, "distinct", len(set(got.tolist())))
    assert abs(mean - 0.5) <= 4.0 / math.sqrt(12.0 * n)
    assert repeats <= 8


# ---- 7. defaults: everything off is mi_op_sample, bit for bit
@pytest.mark.parametrize("V", VS + EDGE_VS)
def test_everything_off_is_bit_identical_to_mi_op_sample(V):
    rng = np.random.default_rng(700 + V)
    lg = make_rows(V, rng)
    u = rng.random(B).astype(np.float32)
    k = min(5, V)
    for temp, top_p, uu in ((0.7, 0.9, u), (1.0, 1.0, u), (0.0, 1.0, u), (0.7, 0.9, None)):
        a = run_ex(lg, temp, top_p, u=uu, k=k, plain=True)
        b = run_ex(lg, temp, top_p, u=uu, k=k)
        for key in a:
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), (V, temp, top_p, key)


def test_invalid_controls_are_refused():
    for kw in (dict(top_k=-1), dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan"))):
        with pytest.raises(ValueError):
            run_ex(RULER, **kw)
    t = dev(RULER)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.float32, device="cuda")
    seeds = _dev_i64([1], np.uint64)
    rc = L.lib().mi_op_sample_ex(ptr(t), 1, 4096, 1.0, 1.0, 0, 0.0, None, None, None, None, ptr(seeds), None, 0, 0, None, 0,
                                 ptr(out), None, None, None, None, ptr(st))
    assert rc == -1 and b"row_seed" in L.lib().mi_last_error()
