"""-m gpu: the sampler's per-row logprobs settings at kernel level (``mi_op_sample_rowlp``).  Everything here is exact: the
yardstick is the k-round form with the call-wide count -- ``mi_op_sample_ex`` at ``top_logprobs = k_b`` (plain log-softmax)
and, for rows that report under softmax(logits / T), the same launch with the call-wide flag (``mi_op_sample_rowlp`` with no
row setting, which is that launch) -- and every row's entries, token and logprob must equal it bit for bit, whichever of the
two methods found them.  Semantics: mi355_decode.h (mi_kv_set_row_logprobs), mi355_ops.h, DESIGN.md §2 / §3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import dev, dev_i32, ptr  # noqa: E402

B, R, STRIDE = 5, 7, L.MI_MAX_TOP_LOGPROBS
KS = [0, 1, 20, 5, 0]                                 # 1: below the crossover (k rounds), 5 and 20: the selection
FLAGS = [1, 0, 1, 0, 0]                               # rows 0 and 2 report under softmax(logits / T)
ROW_MAP = [4, 0, 6, 3, 2]                             # sampled row -> table row: neither the identity nor monotone
VS = [5, 33, 1000, 32000, 151936]                     # k > V; V % 4 != 0 (the scalar walks); V below one pass of 1024 threads
KINDS = ["gaussian", "ints", "equal", "special", "bf16"]
# The widths on either side of the tie table's capacity (TIE_TBL = 1024 entries of one (chunk of 1024 lanes, wave) each, i.e. 64
# chunks): 65535 ids in the scalar walk and 262144 in the vector walk fill it exactly; 65537 and 262148 need a 65th chunk, so the
# selection declines and the rounds answer.  gaussian and bf16 only: ints / equal make tie groups of tens of thousands of ids
# there, which the sampler's rank loop beyond the table walks once per tie rank.
EDGE_VS = [65535, 65537, 262144, 262148]
EDGE_KINDS = ["gaussian", "bf16"]
CASES = [(V, kind) for V in VS for kind in KINDS] + [(V, kind) for V in EDGE_VS for kind in EDGE_KINDS]
TEMPS = [0.0, 0.7, 1.0]


def make_rows(kind, V, rng):
    if kind == "gaussian":
        return (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
    if kind == "ints":                                # the boundary of every k lies in a tie group of about V / 4 ids
        return rng.integers(0, 4, size=(B, V)).astype(np.float32)
    if kind == "equal":
        return np.full((B, V), 1.5, np.float32)
    if kind == "bf16":
        x = torch.from_numpy((rng.standard_normal((B, V)) * 3.0).astype(np.float32))
        return x.to(torch.bfloat16).to(torch.float32).numpy()
    # special: ordinary negative values with NaN, -inf and zeros of both signs among them (the zeros are the largest
    # comparable values, so k = 5 cuts inside their tie group and k = 20 runs past it); rows 0 and 1 also hold +inf
    lg = (-np.abs(rng.standard_normal((B, V))) - 1.0).astype(np.float32)
    for b in range(B):
        vals = [np.nan, -np.inf, -0.0, 0.0, np.nan] + [0.0 if i % 2 else -0.0 for i in range(10)] + [-np.inf, np.nan]
        if b < 2:
            vals += [np.inf, np.inf]
        n = min(V, len(vals))
        for p, v in zip(rng.choice(V, size=n, replace=False), vals[:n]):
            lg[b, p] = v
    return lg


def launch(lg, temp, u, *, k_call=0, at_temp_call=0, tab=None, method=0, ex=False):
    """One sampler launch over the rows `lg`.  tab = (k [R], flag [R], n_settings): mi_op_sample_rowlp with the settings
    (top arrays [B][20]); tab None: the call-wide count k_call, through mi_op_sample_ex (ex) or mi_op_sample_rowlp without
    a setting (top arrays [B][k_call])."""
    n, V = lg.shape
    t = dev(lg)
    ud = dev(np.asarray(u, np.float32)) if (u is not None and temp > 0) else None
    toks = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    lp = torch.zeros(n, dtype=torch.float32, device="cuda")
    ki = torch.full((n * STRIDE,), -9, dtype=torch.int32, device="cuda")
    kl = torch.full((n * STRIDE,), 123.0, dtype=torch.float32, device="cuda")
    st = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    head = (ptr(t), n, V, float(temp), 1.0, 0, 0.0, None, None, None, None, None, None, 0, 0, ptr(ud), int(k_call), ptr(toks),
            ptr(lp), None, ptr(ki), ptr(kl), ptr(st))
    torch.cuda.synchronize()
    if ex:
        L.check(L.lib().mi_op_sample_ex(*head))
        width = k_call
    else:
        tk = tf = mp = None
        n_set = 0
        if tab is not None:
            tk, tf, mp, n_set = dev_i32(tab[0]), dev_i32(tab[1]), dev_i32(ROW_MAP), int(tab[2])
        L.check(L.lib().mi_op_sample_rowlp(*head, 0, None, None, None, None, None, R if tab is not None else 0, 0, ptr(mp),
                                           ptr(tk), ptr(tf), n_set, int(at_temp_call), int(method)))
        width = STRIDE if n_set > 0 else k_call
    ids, lps = ki.cpu().numpy(), kl.cpu().numpy()
    return {"tokens": toks.cpu().numpy(), "logprobs": lp.cpu().numpy(), "row_stats": st.cpu().numpy(),
            "top_ids": ids[:n * width].reshape(n, width), "top_logprobs": lps[:n * width].reshape(n, width),
            "tail_ids": ids[n * width:], "tail_lps": lps[n * width:]}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def table(ks=KS, flags=FLAGS):
    k = np.full(R, -1, np.int32)
    f = np.full(R, 1, np.int32)                       # (the flag of a row without a setting is never read)
    n = 0
    for b, t in enumerate(ROW_MAP):
        if ks[b] is not None:
            k[t], f[t] = ks[b], flags[b]
            n += 1
    return k, f, n


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"V{p[0]}-{p[1]}")
def case(request):
    """The rows of one (V, kind) and, per temperature, the yardstick outputs for every (k, flag) the settings use."""
    V, kind = request.param
    rng = np.random.default_rng(77 * V + KINDS.index(kind))
    lg = make_rows(kind, V, rng)
    u = rng.random(B).astype(np.float32)
    want = {}
    for temp in TEMPS:
        for k, flag in sorted({(max(k, 1), f) for k, f in zip(KS, FLAGS)}):
            if flag:
                want[temp, k, flag] = launch(lg, temp, u, k_call=k, at_temp_call=1)
            else:
                want[temp, k, flag] = launch(lg, temp, u, k_call=k, ex=True)
    return dict(V=V, kind=kind, lg=lg, u=u, want=want)


@pytest.mark.parametrize("method", [0, 1, 2], ids=["dispatch", "rounds", "selection"])
def test_rows_equal_the_call_wide_count_bit_for_bit(case, method):
    """ids, logprobs, the token and logprob_out of every row against the yardstick at (k_b, flag_b): under the dispatch
    k = 1 runs k rounds and k = 5 / 20 the selection (both sides of the crossover), and each method forced on every row."""
    lg, u = case["lg"], case["u"]
    for temp in TEMPS:
        got = launch(lg, temp, u, tab=table(), method=method)
        assert got["top_ids"].shape == (B, STRIDE)
        for b in range(B):
            k, flag = KS[b], FLAGS[b]
            ref = case["want"][temp, max(k, 1), flag]
            where = (case["V"], case["kind"], temp, method, b, k)
            assert got["tokens"][b] == ref["tokens"][b], where
            assert bits(got["logprobs"][b]) == bits(ref["logprobs"][b]), where
            assert np.array_equal(got["top_ids"][b, :k], ref["top_ids"][b, :k]), (where, got["top_ids"][b, :k], ref["top_ids"][b, :k])
            assert bits(got["top_logprobs"][b, :k]) == bits(ref["top_logprobs"][b, :k]), where
            # entries past the row's count (all 20 of a row with k = 0): the documented filler
            assert np.all(got["top_ids"][b, k:] == -1), where
            assert np.all(np.isneginf(got["top_logprobs"][b, k:])), where
        assert bits(got["row_stats"]) == bits(case["want"][temp, 1, 0]["row_stats"])


def test_rows_without_a_setting_keep_the_calls_count_and_flag(case):
    """Only sampled row 2 has a setting (20, plain); the others report the call's 3 entries under the call's flag."""
    lg, u, temp = case["lg"], case["u"], 0.7
    ks = [None, None, 20, None, None]
    got = launch(lg, temp, u, k_call=3, at_temp_call=1, tab=table(ks, [0] * B))
    ref3 = launch(lg, temp, u, k_call=3, at_temp_call=1)
    ref20 = launch(lg, temp, u, k_call=20, ex=True)
    for b in range(B):
        ref, k = (ref20, 20) if b == 2 else (ref3, 3)
        assert got["tokens"][b] == ref["tokens"][b]
        assert bits(got["logprobs"][b]) == bits(ref["logprobs"][b]), b
        assert np.array_equal(got["top_ids"][b, :k], ref["top_ids"][b, :k]), b
        assert bits(got["top_logprobs"][b, :k]) == bits(ref["top_logprobs"][b, :k]), b
        assert np.all(got["top_ids"][b, k:] == -1)


def test_a_table_without_a_setting_takes_the_old_launch(case):
    """The arrays allocated, every row without a setting, n_row_settings = 0: the outputs and the [B][k] layout of
    mi_op_sample_ex, and nothing written behind them."""
    lg, u = case["lg"], case["u"]
    empty = (np.full(R, -1, np.int32), np.zeros(R, np.int32), 0)
    for temp in (0.0, 0.7):
        got = launch(lg, temp, u, k_call=5, tab=empty)
        ref = case["want"][temp, 5, 0]
        for key in ("tokens", "logprobs", "top_ids", "top_logprobs", "row_stats"):
            assert got[key].shape == ref[key].shape and bits(got[key]) == bits(ref[key]), (key, temp)
        assert np.all(got["tail_ids"] == -9) and np.all(got["tail_lps"] == 123.0)


def test_refusals():
    lg = dev(np.zeros((2, 8), np.float32))
    toks = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    k = dev_i32([1, 1])
    head = (ptr(lg), 2, 8, 0.0, 1.0, 0, 0.0, None, None, None, None, None, None, 0, 0, None, 0, ptr(toks), None, None)
    tail = (ptr(st), 0, None, None, None, None, None, 2, 0, None)
    torch.cuda.synchronize()
    # settings without the top-k outputs, without the flag array, a negative count of settings, an unknown method
    assert L.lib().mi_op_sample_rowlp(*head, None, None, *tail, ptr(k), ptr(k), 1, 0, 0) == -1
    ki = torch.zeros(40, dtype=torch.int32, device="cuda")
    kl = torch.zeros(40, dtype=torch.float32, device="cuda")
    assert L.lib().mi_op_sample_rowlp(*head, ptr(ki), ptr(kl), *tail, ptr(k), None, 1, 0, 0) == -1
    assert L.lib().mi_op_sample_rowlp(*head, ptr(ki), ptr(kl), *tail, ptr(k), ptr(k), -1, 0, 0) == -1
    assert L.lib().mi_op_sample_rowlp(*head, ptr(ki), ptr(kl), *tail, ptr(k), ptr(k), 1, 0, 3) == -1
    assert L.lib().mi_op_sample_rowlp(*head, ptr(ki), ptr(kl), *tail, ptr(k), ptr(k), 1, 0, 0) == 0
