"""Kernel-level tests (-m gpu) of csrc/moe.hip through mi_op_moe_route / mi_op_moe_linear / mi_op_moe_mlp (include/mi355_ops.h).

* route: integer-valued xn and Wg (every sum exact, so the gate logits are numpy's bit for bit): sel equal to numpy under the
  tie rule (lower expert index), lists equal, scores within 1 ulp of T of numpy's float32 softmax; rows with exact ties, a
  router that sends every row to one expert and none to another.
* grouped linear: integer-valued operands, |sums| < 2^24: bit-equal to numpy for bf16, f16 and float32 activations, over an
  empty expert and experts with 1, 16, 17 and 40 pairs (the row-tile edges), both matrix shapes of the block.
* MLP: random data against the twin's arithmetic (tests/moe_ref.py) under the bound tests/test_gpu_skinny.py applies to its
  SwiGLU epilogues.
* a row's outputs are bit-equal whether it runs alone or among 39 others.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.numerics import matmul_nt, round_to
from oracle.ref_model import Linear

pytestmark = pytest.mark.gpu

import moe_ref  # noqa: E402
from gpu_helpers import MIDT, dev, dev_i32, host, ptr  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from test_gpu_skinny import _assert_close  # noqa: E402  (the bound of its SwiGLU epilogues)

# (activation dtype T, weight dtype): 16-bit activations meet weights of their own dtype, float32 ones either
TYPES = [("bfloat16", "bfloat16"), ("float16", "float16"), ("float32", "bfloat16"), ("float32", "float16")]
IDS = [f"{a}-{w}" for a, w in TYPES]
ONE_ULP = {"float32": 2.0 ** -23, "bfloat16": 2.0 ** -7, "float16": 2.0 ** -10}      # of a value in [1, 2)


def op_route(xn_d, R, H, act, wg_d, wdt, E, k, rnd=0):
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[act]
    sel = torch.full((R, k), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((R, k), dtype=tdt, device="cuda")
    meta = torch.full((2 * E,), -7, dtype=torch.int32, device="cuda")
    lst = torch.full((R * k,), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().mi_op_moe_route(ptr(xn_d), H, R, H, MIDT[act], rnd, ptr(wg_d), MIDT[wdt], E, k, ptr(sel), ptr(score), ptr(meta),
                                    ptr(lst), 0, None))
    return sel, score, meta, lst


def op_linear(x_d, ldx, x_rows, x_shift, act, w_d, wdt, E, N, K, meta_d, list_d, pairs, out_d, rnd=0, check=True):
    rc = L.lib().mi_op_moe_linear(ptr(x_d), ldx, x_rows, x_shift, MIDT[act], rnd, ptr(w_d), MIDT[wdt], E, N, K, ptr(meta_d), ptr(list_d),
                                  pairs, ptr(out_d), N, 0, None)
    if check:
        L.check(rc)
    return rc


def op_mlp(xn_d, R, H, I, act, wdt, E, k, wg_d, wu_d, wd_d, meta_d, list_d, score_d, resid_d, out_d, rnd=0):
    L.check(L.lib().mi_op_moe_mlp(ptr(xn_d), H, R, H, I, MIDT[act], rnd, MIDT[wdt], E, k, ptr(wg_d), ptr(wu_d), ptr(wd_d), ptr(meta_d),
                                  ptr(list_d), ptr(score_d), ptr(resid_d), H, ptr(out_d), H, 0, None))


def _lists(sel, E):
    """numpy's work lists: (cnt [E], off [E], list [R k]) with the pairs of every expert ascending."""
    flat = np.asarray(sel).reshape(-1)
    runs = [np.nonzero(flat == e)[0] for e in range(E)]
    cnt = np.array([len(r) for r in runs], np.int32)
    return cnt, (np.cumsum(cnt) - cnt).astype(np.int32), np.concatenate(runs).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# route

@pytest.mark.parametrize("act,wdt", TYPES, ids=IDS)
def test_route_selection_lists_and_scores(act, wdt):
    rng = np.random.default_rng(11)
    H = 128
    for R in (1, 16, 17, 40):
        for E in (1, 4, 8, 16):
            for k in (1, 2):
                if k > E:
                    continue
                for router in ("random", "ties", "one_sided"):
                    x = rng.integers(-4, 5, size=(R, H)).astype(np.float32)
                    wg = rng.integers(-3, 4, size=(E, H)).astype(np.float32)
                    if router == "ties" and E >= 2:
                        wg[E - 1] = wg[0]                              # every row ties experts 0 and E - 1 exactly
                        if E >= 4:
                            wg[2] = wg[1]
                    if router == "one_sided" and E >= 2:
                        x[:, 0] = 4.0                                  # expert 0 takes every row, expert E - 1 none (k < E)
                        wg[0, 0], wg[E - 1, 0] = 2000.0, -2000.0     # 8000 against at most 127 * 12
                    g = round_to(matmul_nt(x, wg), act)                # integer sums below 2^24: exact, then one rounding to T
                    sel_w, soft_w, _m, _a = moe_ref.route(g, k)
                    sel_d, score_d, meta_d, list_d = op_route(dev(x, act), R, H, act, dev(wg, wdt), wdt, E, k)
                    what = (act, R, E, k, router)
                    sel = host(sel_d).astype(np.int64)
                    assert np.array_equal(sel, sel_w), what
                    cnt, off, lst = _lists(sel_w, E)
                    meta = host(meta_d).astype(np.int32)
                    assert np.array_equal(meta[:E], cnt) and np.array_equal(meta[E:], off), what
                    assert np.array_equal(host(list_d).astype(np.int32), lst), what
                    if router == "one_sided" and E >= 2:
                        assert cnt[0] == R and (cnt[E - 1] == 0 or k == E), what
                    if router == "ties" and E >= 2:
                        assert np.all((sel[(sel == E - 1).any(axis=1)] == 0).any(axis=1)), what      # the twin of expert 0 never goes first
                    got = host(score_d).astype(np.float64)
                    # one ulp of T at the value (float16: never below its subnormal spacing 2^-24)
                    tol = ONE_ULP[act] * np.exp2(np.floor(np.log2(np.maximum(soft_w, 2.0 ** -120)))) if act == "float32" else moe_ref.ulp(soft_w, act)
                    assert np.all(np.abs(got - soft_w.astype(np.float64)) <= tol), (what, np.abs(got - soft_w).max())


def test_route_refuses_bad_shapes():
    x, wg = dev(np.zeros((4, 128), np.float32), "bfloat16"), dev(np.zeros((4, 128), np.float32), "bfloat16")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    sc = torch.zeros(64, dtype=torch.bfloat16, device="cuda")

    def rc(H=128, E=4, k=2, act=L.MI_BF16, wdt=L.MI_BF16):
        return L.lib().mi_op_moe_route(ptr(x), H, 4, H, act, 0, ptr(wg), wdt, E, k, ptr(i32), ptr(sc), ptr(i32), ptr(i32), 0, None)

    assert rc() == 0
    assert rc(E=17) == -3 and rc(E=0) == -3 and rc(k=3) == -3 and rc(E=1, k=2) == -3 and rc(H=96) == -3
    assert rc(act=L.MI_BF16, wdt=L.MI_F16) == -3 and rc(wdt=L.MI_F32) == -3


# ---------------------------------------------------------------------------------------------------------------------------
# grouped linear

COUNTS = [0, 1, 16, 17, 40]            # an empty expert, then the row-tile edges


def _routing(rng, counts, spare=0):
    """A routing with exactly counts[e] pairs on expert e (+ `spare` pairs on no list): -> (pairs, meta, list)."""
    pairs = sum(counts) + spare
    owner = np.concatenate([np.full(c, e) for e, c in enumerate(counts)] + [np.full(spare, -1)]).astype(np.int64)
    rng.shuffle(owner)
    cnt, off, lst = _lists(owner, len(counts))
    return pairs, owner, np.concatenate([cnt, off]).astype(np.int32), np.concatenate([lst, np.zeros(spare, np.int32)]).astype(np.int32)


@pytest.mark.parametrize("act,wdt", TYPES, ids=IDS)
@pytest.mark.parametrize("N,K", [(192, 128), (64, 128), (64, 192), (128, 192)])       # [E][I][H] and [E][H][I] at H = 128 / 64, I = 192
@pytest.mark.parametrize("x_shift", [0, 1])
def test_grouped_linear_is_bit_equal_to_numpy(act, wdt, N, K, x_shift):
    rng = np.random.default_rng(N * 7 + K + x_shift)
    E = len(COUNTS)
    pairs, owner, meta, lst = _routing(rng, COUNTS, spare=3)
    x_rows = (pairs + (1 << x_shift) - 1) >> x_shift
    x = rng.integers(-8, 9, size=(x_rows, K)).astype(np.float32)
    w = rng.integers(-8, 9, size=(E, N, K)).astype(np.float32)                    # |sum| <= 192 * 64 < 2^24
    out = torch.full((pairs, N), 7.0, dtype=dev(x[:1], act).dtype, device="cuda")
    op_linear(dev(x, act), K, x_rows, x_shift, act, dev(w, wdt), wdt, E, N, K, dev_i32(meta), dev_i32(lst), pairs, out)
    got = host(out)
    want = np.full((pairs, N), 7.0, np.float32)                                   # a pair on no list is not written
    for p in range(pairs):
        if owner[p] >= 0:
            want[p] = round_to(matmul_nt(x[p >> x_shift][None], w[owner[p]]), act)[0]
    assert np.array_equal(got, want), (act, N, K, x_shift, np.argwhere(got != want)[:4])


def test_grouped_linear_refuses_lists_that_leave_the_call():
    rng = np.random.default_rng(3)
    pairs, _owner, meta, lst = _routing(rng, [2, 3])
    x, w = dev(np.zeros((pairs, 128), np.float32), "bfloat16"), dev(np.zeros((2, 64, 128), np.float32), "bfloat16")
    out = torch.zeros((pairs, 64), dtype=torch.bfloat16, device="cuda")

    def rc(meta_, lst_, x_rows=pairs, x_shift=0, N=64, K=128):
        return op_linear(x, K, x_rows, x_shift, "bfloat16", w, "bfloat16", 2, N, K, dev_i32(meta_), dev_i32(lst_), pairs, out, check=False)

    assert rc(meta, lst) == 0
    assert rc(np.array([2, 4, 0, 2], np.int32), lst) == -1                         # a run past the list array
    assert rc(meta, np.array([0, 1, 2, 3, 5], np.int32)) == -1                     # an entry that is no pair
    assert rc(meta, lst, x_rows=pairs - 1) == -1                                   # a pair whose row of x does not exist
    assert rc(meta, lst, N=96) == -3 and rc(meta, lst, K=96) == -3


# ---------------------------------------------------------------------------------------------------------------------------
# the whole block behind the route

def _block_data(rng, act, wdt, R, H, I, E):
    x = round_to(rng.standard_normal((R, H)).astype(np.float32), act)
    wr = round_to(rng.standard_normal((E, H)).astype(np.float32) * 0.3, wdt)
    wg = round_to(rng.standard_normal((E, I, H)).astype(np.float32) / np.sqrt(H), wdt)
    wu = round_to(rng.standard_normal((E, I, H)).astype(np.float32) / np.sqrt(H), wdt)
    wd = round_to(rng.standard_normal((E, H, I)).astype(np.float32) / np.sqrt(I), wdt)
    h = round_to(rng.standard_normal((R, H)).astype(np.float32), act)
    return x, wr, wg, wu, wd, h


def _device_block(act, wdt, x, wr, wg, wu, wd, h, E, k):
    R, H = x.shape
    I = wg.shape[1]
    xd = dev(x, act)
    sel, score, meta, lst = op_route(xd, R, H, act, dev(wr, wdt), wdt, E, k)
    out = torch.zeros((R, H), dtype=xd.dtype, device="cuda")
    op_mlp(xd, R, H, I, act, wdt, E, k, dev(wg, wdt), dev(wu, wdt), dev(wd, wdt), meta, lst, score, dev(h, act) if h is not None else None, out)
    return host(sel).astype(np.int64), host(score), host(out)


@pytest.mark.parametrize("act,wdt", TYPES, ids=IDS)
@pytest.mark.parametrize("R,E,k", [(40, 8, 2), (17, 4, 1), (1, 4, 2), (33, 1, 1)])
def test_mlp_matches_the_twins_arithmetic(act, wdt, R, E, k):
    rng = np.random.default_rng(100 * R + 10 * E + k)
    H, I = 128, 192
    x, wr, wg, wu, wd, h = _block_data(rng, act, wdt, R, H, I, E)
    sel, score, out = _device_block(act, wdt, x, wr, wg, wu, wd, h, E, k)
    # the twin: g and the routing, the experts' SwiGLU MLPs, the weighted sum, the residual
    odt = "float32" if act == "float32" else act
    g = round_to(matmul_nt(x, wr), odt)
    sel_w, soft, margin, at = moe_ref.route(g, k)
    clear = margin >= 8 * moe_ref.ulp(at, "bfloat16" if act == "float32" else act) if act != "float32" else margin >= 1e-4
    assert (R < 16 or clear.mean() >= 0.8) and np.array_equal(sel[clear], sel_w[clear])        # (a near-tie may go either way: those rows are left out)
    scores = round_to(soft, odt)
    terms = []
    for j in range(k):
        y = np.zeros((R, H), np.float32)
        for e in range(E):
            rows = np.nonzero(sel_w[:, j] == e)[0]
            if rows.size:
                lin = [Linear(dtype=wdt, weight=m[e]) for m in (wg, wu, wd)]
                y[rows] = moe_ref.swiglu_mlp(lin[0], lin[1], lin[2], x[rows], act)[0]
        terms.append(round_to(y * scores[:, j:j + 1], odt))
    r = terms[0] if k == 1 else round_to(terms[0] + terms[1], odt)
    want = round_to(h + r, odt)
    _assert_close(out[clear], want[clear], act, scale=float(np.sqrt(np.mean(np.square(r)))) + 1e-12)


@pytest.mark.parametrize("act,wdt", TYPES, ids=IDS)
def test_a_rows_outputs_do_not_depend_on_its_neighbours(act, wdt):
    rng = np.random.default_rng(77)
    R, H, I, E, k = 40, 128, 192, 8, 2
    x, wr, wg, wu, wd, h = _block_data(rng, act, wdt, R, H, I, E)
    sel, score, out = _device_block(act, wdt, x, wr, wg, wu, wd, h, E, k)
    for row in (0, 7, 39):
        s1, c1, o1 = _device_block(act, wdt, x[row:row + 1], wr, wg, wu, wd, h[row:row + 1], E, k)
        assert np.array_equal(s1[0], sel[row]) and np.array_equal(c1[0], score[row]) and np.array_equal(o1[0], out[row]), (act, row)
