"""-m gpu: the sampler's per-row logit_bias table at kernel level (``mi_op_sample_rowbias``).  Everything here is exact: one
IEEE float32 add per biased logit on the host gives the row the device must have produced, and the existing
``mi_op_sample_ex`` on that row gives every output it must report.  Semantics: mi355_decode.h (mi_kv_set_row_logit_bias),
DESIGN.md §2."""
import numpy as np
import pytest
import torch

from oracle import ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_i32, ptr  # noqa: E402

B, R, CAP, K = 8, 12, 1024, 5
VS = [37, 5000, 151936]                               # 37: the scalar walk of a row (V % 4 != 0) and counts capped by V
COUNTS = [0, 1, 7, 300, 1024, 3, 0, 64, 2, 1000, 5, 17]
ROW_MAP = [4, 0, 9, 3, 11, 2, 7, 1]                   # sampled row -> table row: neither the identity nor monotone
BAN_ROW, PUSH_ROW = 5, 6                              # sampled rows (table rows 2 and 7) with a -1e4 / +1e4 entry
OUT_KEYS = ("tokens", "logprobs", "top_ids", "top_logprobs", "row_stats")


def _dev_i64(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.int64)).cuda().contiguous()


def make_rows(V, rng, n=B):
    return (rng.standard_normal((n, V)) * 3.0).astype(np.float32)


def make_table(V, rng, lg):
    """-> (counts [R], ids [R][CAP], vals [R][CAP]).  Row r has min(COUNTS[r], V) entries with distinct ids and values in
    [-20, 20]; the slots behind a row's count hold a valid id with a huge value, which a kernel that read past the count
    would show.  The table row of sampled row BAN_ROW bans that row's unbiased arg-max, the one of PUSH_ROW pushes one id."""
    counts = np.minimum(np.asarray(COUNTS), V).astype(np.int32)
    ids = np.zeros((R, CAP), np.int32)
    vals = np.full((R, CAP), 1e6, np.float32)
    for r in range(R):
        n = int(counts[r])
        ids[r, :n] = rng.choice(V, size=n, replace=False)
        vals[r, :n] = rng.uniform(-20.0, 20.0, size=n).astype(np.float32)
    for b, v in ((BAN_ROW, -1e4), (PUSH_ROW, 1e4)):
        r = ROW_MAP[b]
        target = int(np.argmax(lg[b])) if v < 0 else int(ids[r, 0])
        hit = np.flatnonzero(ids[r, :counts[r]] == target)
        slot = int(hit[0]) if len(hit) else 0
        ids[r, slot], vals[r, slot] = target, v
    return counts, ids, vals


def host_apply(lg, counts, ids, vals, row_map):
    ref = np.array(lg, np.float32, copy=True)
    for b in range(lg.shape[0]):
        r = row_map[b] if row_map is not None else b
        n = int(counts[r])
        ref[b, ids[r, :n]] = np.float32(lg[b, ids[r, :n]] + vals[r, :n])       # one float32 add per element
    return ref


def run(lg, ctl, table=None, row_map=None, call_bias=None, ex=False):
    """One launch of mi_op_sample_rowbias (ex: of mi_op_sample_ex, which has neither list) with the controls `ctl`
    -> dict of host arrays, the logits buffer after the call included."""
    lg = np.asarray(lg, np.float32)
    n, V = lg.shape
    t = dev(lg)
    u = ctl.get("u")
    ud = dev(np.asarray(u, np.float32)) if u is not None else None
    streams = ctl.get("streams")
    rs, rq = (_dev_i64(streams[0], np.uint64), _dev_i64(streams[1], np.int64)) if streams else (None, None)
    toks = torch.zeros(n, dtype=torch.int32, device="cuda")
    lp = torch.zeros(n, dtype=torch.float32, device="cuda")
    p0 = torch.zeros(n, dtype=torch.float32, device="cuda")
    ki = torch.zeros((n, K), dtype=torch.int32, device="cuda")
    kl = torch.zeros((n, K), dtype=torch.float32, device="cuda")
    st = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    head = (ptr(t), n, V, ctl.get("temp", 0.0), ctl.get("top_p", 1.0), ctl.get("top_k", 0), 0.0, None, None, None, None,
            ptr(rs), ptr(rq), ctl.get("seed", 0), ctl.get("step", 0), ptr(ud), K, ptr(toks), ptr(lp), ptr(p0), ptr(ki), ptr(kl),
            ptr(st))
    keep = []
    if ex:
        torch.cuda.synchronize()
        L.check(L.lib().mi_op_sample_ex(*head))
    else:
        nb, bi, bv = 0, None, None
        if call_bias is not None:
            bi, bv = dev_i32(call_bias[0]), dev(np.asarray(call_bias[1], np.float32))
            nb = len(call_bias[0])
        tc = ti = tv = None
        if table is not None:
            tc, ti, tv = dev_i32(table[0]), dev_i32(table[1]), dev(table[2])
        mp = dev_i32(row_map) if row_map is not None else None
        keep += [bi, bv, tc, ti, tv, mp]
        torch.cuda.synchronize()
        L.check(L.lib().mi_op_sample_rowbias(*head, nb, ptr(bi), ptr(bv), ptr(tc), ptr(ti), ptr(tv),
                                             R if table is not None else 0, CAP if table is not None else 0, ptr(mp)))
    return {"tokens": toks.cpu().numpy(), "logprobs": lp.cpu().numpy(), "probs_row0": p0.cpu().numpy(),
            "top_ids": ki.cpu().numpy(), "top_logprobs": kl.cpu().numpy(), "row_stats": st.cpu().numpy(),
            "logits": t.cpu().numpy()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def controls(rng):
    return {
        "greedy": dict(temp=0.0),
        "nucleus": dict(temp=0.8, top_p=0.9, u=rng.random(B).astype(np.float32)),
        # per-row streams (no injected uniforms: they would take precedence over every stream)
        "top_k_streams": dict(temp=1.0, top_k=40, seed=11, step=3,
                              streams=(rng.integers(0, 2 ** 63, size=B, dtype=np.uint64), np.arange(B, dtype=np.int64) % 3 - 1)),
    }


@pytest.fixture(scope="module", params=VS)
def case(request):
    """Logits, table and the host's biased rows for one V, shared by the tests below (none of them changes it)."""
    V = request.param
    rng = np.random.default_rng(1000 + V)
    lg = make_rows(V, rng)
    counts, ids, vals = make_table(V, rng, lg)
    ref = host_apply(lg, counts, ids, vals, ROW_MAP)
    return dict(V=V, rng=rng, lg=lg, table=(counts, ids, vals), ref=ref, ctl=controls(rng))


# ---- 1. exact differential against mi_op_sample_ex on the host-biased rows
@pytest.mark.parametrize("which", ["greedy", "nucleus", "top_k_streams"])
def test_table_rows_equal_the_host_biased_rows_bit_for_bit(case, which):
    ctl = case["ctl"][which]
    got = run(case["lg"], ctl, table=case["table"], row_map=ROW_MAP)
    want = run(case["ref"], ctl, ex=True)
    assert same_bits(got["logits"], case["ref"])               # the logits changed in place, to exactly the host's rows
    for key in OUT_KEYS + ("probs_row0",):
        assert same_bits(got[key], want[key]), key
    # the two marked rows did what they are there for
    unbiased = int(np.argmax(case["lg"][BAN_ROW]))
    assert got["tokens"][BAN_ROW] != unbiased and unbiased not in got["top_ids"][BAN_ROW]
    pushed = int(case["table"][1][ROW_MAP[PUSH_ROW], 0])
    assert got["tokens"][PUSH_ROW] == pushed and got["logprobs"][PUSH_ROW] > -1e-3


def test_identity_map_is_null(case):
    """row_map = NULL: sampled row b reads table row b."""
    ctl = case["ctl"]["nucleus"]
    got = run(case["lg"], ctl, table=case["table"], row_map=None)
    ref = host_apply(case["lg"], *case["table"], None)
    want = run(ref, ctl, ex=True)
    assert same_bits(got["logits"], ref)
    for key in OUT_KEYS:
        assert same_bits(got[key], want[key]), key


# ---- 2. both lists, and no race between them
def test_call_wide_list_first_then_the_row_list(case):
    V, lg, (counts, ids, vals) = case["V"], case["lg"], case["table"]
    rng = np.random.default_rng(7)
    b = 3                                                      # sampled row 3 = table row 3 (300 entries; V = 37: 37)
    r = ROW_MAP[b]
    shared = ids[r, :3]
    others = np.setdiff1d(np.arange(V), ids[r, :counts[r]])
    extra = rng.choice(others, size=min(5, len(others)), replace=False) if len(others) else np.zeros(0, np.int64)
    call_ids = np.concatenate([shared, extra]).astype(np.int32)
    call_vals = rng.uniform(-20.0, 20.0, size=len(call_ids)).astype(np.float32)
    ref = np.array(lg, np.float32, copy=True)
    ref[:, call_ids] = np.float32(ref[:, call_ids] + call_vals[None, :])        # every row, first
    ref = host_apply(ref, counts, ids, vals, ROW_MAP)                            # then the row's own entries
    assert not same_bits(ref[b, shared], host_apply(lg, counts, ids, vals, ROW_MAP)[b, shared])
    ctl = case["ctl"]["nucleus"]
    want = run(ref, ctl, ex=True)
    first = None
    for _ in range(20):                                        # a missing barrier would show as a difference between launches
        got = run(lg, ctl, table=case["table"], row_map=ROW_MAP, call_bias=(call_ids, call_vals))
        assert same_bits(got["logits"], ref)
        for key in OUT_KEYS:
            assert same_bits(got[key], want[key]), key
        first = first or got
        assert all(same_bits(got[key], first[key]) for key in first)


# ---- 3. greedy against the oracle, one row at a time with that row's dict
def test_greedy_tokens_equal_the_oracle_row_by_row(case):
    lg, (counts, ids, vals) = case["lg"], case["table"]
    got = run(lg, dict(temp=0.0), table=case["table"], row_map=ROW_MAP)
    for b in range(B):
        r = ROW_MAP[b]
        bias = {int(i): float(v) for i, v in zip(ids[r, :counts[r]], vals[r, :counts[r]])}
        want = ref_sample.sample(lg[b:b + 1], temp=0.0, logit_bias=bias)
        assert int(got["tokens"][b]) == int(want["tokens"][0, 0]), b


# ---- 4. the null cases
@pytest.mark.parametrize("which", ["greedy", "nucleus", "top_k_streams"])
def test_without_a_table_the_op_is_mi_op_sample_ex(case, which):
    ctl = case["ctl"][which]
    got = run(case["lg"], ctl)                                 # NULL table, n_bias = 0
    want = run(case["lg"], ctl, ex=True)
    for key in want:
        assert same_bits(got[key], want[key]), key
    assert same_bits(got["logits"], case["lg"])


def test_a_row_with_count_zero_in_a_table_is_unbiased(case):
    ctl = case["ctl"]["nucleus"]
    got = run(case["lg"], ctl, table=case["table"], row_map=ROW_MAP)
    plain = run(case["lg"], ctl, ex=True)
    empties = [b for b in range(B) if case["table"][0][ROW_MAP[b]] == 0]
    assert empties == [1]                                      # sampled row 1 = table row 0
    for b in empties:
        assert same_bits(got["logits"][b], case["lg"][b])
        for key in OUT_KEYS:
            assert same_bits(got[key][b], plain[key][b]), key


def test_bad_table_arguments_are_refused():
    lg = make_rows(37, np.random.default_rng(0), 1)
    t, cnt = dev(lg), dev_i32([1])
    toks = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    head = (ptr(t), 1, 37, 0.0, 1.0, 0, 0.0, None, None, None, None, None, None, 0, 0, None, 0, ptr(toks), None, None, None, None,
            ptr(st))
    for tail in ((0, None, None, ptr(cnt), None, None, 1, CAP, None),          # counts without ids / values
                 (0, None, None, ptr(cnt), ptr(cnt), ptr(t), 0, CAP, None),    # no rows
                 (0, None, None, ptr(cnt), ptr(cnt), ptr(t), 1, 0, None),      # no capacity
                 (2, None, None, None, None, None, 0, 0, None),                # a call-wide count without its arrays
                 (-1, None, None, None, None, None, 0, 0, None)):
        assert L.lib().mi_op_sample_rowbias(*head, *tail) == -1
