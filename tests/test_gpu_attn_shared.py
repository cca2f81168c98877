"""Shared-prefix decode attention (-m gpu): mi_op_attention_shared against a float64 attention over every row's own block table.
One layout (16-token blocks, Hkv = 2, MPG = 16 // G): set A of 2 rows sharing 19 blocks (304 keys: several chunks and rounds), tails
1 and 33; set B of MPG + 1 rows sharing ONE other block (a second column group of one member), tails 1 (the new key only), 17,
300, then 5; one row of 40 keys that shares nothing.  Block ids are permuted; block 0 holds a finite decoy."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import attn_shape, dev, dev_i32, host, ptr
from attn16_cases import assert_rule
from mlx_parallm_amd import _lib as L
from oracle.numerics import round_to

pytestmark = pytest.mark.gpu

BS, HKV = 16, 2
CASES = [(t, D, G) for t in ("bfloat16", "float16", "float32") for D, G in [(64, 1), (128, 4), (128, 8), (64, 3), (128, 5)]]


@functools.lru_cache(maxsize=None)
def layout(G):
    mpg = 16 // G
    sets = [(19 * BS, [1, 33]), (BS, ([1, 17, 300] + [5] * mpg)[:mpg + 1]), (0, [40])]
    stride = (19 * BS + 300) // BS + 2
    run, n_keys, ptr_, tab, nxt = [], [], [0], [], 1
    for r, tails in sets:
        shared = list(range(nxt, nxt + r // BS))
        nxt += len(shared)
        for t in tails:
            own = list(range(nxt, nxt + -(-(r + t) // BS) - len(shared)))
            nxt += len(own)
            tab.append((shared + own + [0] * stride)[:stride])
            run.append(r)
            n_keys.append(r + t)
        ptr_.append(len(run))
    perm = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(nxt - 1)])      # logical -> physical block
    return dict(run=run, n_keys=n_keys, ptr=ptr_, set_run=[r for r, _ in sets], tab=perm[np.array(tab)], nblk=nxt,
                max_members=max(len(t) for _, t in sets), max_tail=max(max(t) for _, t in sets))


def launch(lay, D, G, dtype, q, karena, varena, repeat=1):
    B, Hq = len(lay["run"]), HKV * G
    s = attn_shape(B, 1, Hq, HKV, D, dtype, dtype, 0, lay["tab"].shape[1] * BS)
    tab_d, off_d = dev_i32(lay["tab"]), dev_i32(np.array(lay["n_keys"]) - 1)
    sp_d, sm_d, sr_d = dev_i32(lay["ptr"]), dev_i32(np.arange(B)), dev_i32(lay["set_run"])
    q_d, k_d, v_d = dev(q.reshape(B, Hq * D), dtype), dev(karena, dtype), dev(varena, dtype)
    part = torch.zeros(B * Hq * 16 * (D + 2), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(B * HKV, dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(repeat):
        out = torch.zeros((B, Hq * D), dtype=q_d.dtype, device="cuda")
        torch.cuda.synchronize()
        L.check(L.lib().mi_op_attention_shared(C.byref(s), ptr(tab_d), lay["tab"].shape[1], 4, ptr(q_d), ptr(k_d), ptr(v_d), ptr(off_d),
                                               ptr(sp_d), ptr(sm_d), ptr(sr_d), len(lay["set_run"]), 2, lay["max_members"], max(lay["set_run"]),
                                               lay["max_tail"], ptr(out), float(D ** -0.5), ptr(part), ptr(ctr), 1, None))
        torch.cuda.synchronize()
        assert not ctr.cpu().numpy().any()                 # the tickets are back at zero
        outs.append(host(out).reshape(B, Hq, D))
    return outs


@pytest.mark.parametrize("dtype,D,G", CASES)
def test_exact_key_selection(dtype, D, G):
    """One-hot q and K: head g of a set's m-th row owns hot dimension (5 (m G + g) + 1) mod D and selects ONE key (first / last key
    of the run, both sides of a cut, first tail key, the new key, ...), 520 score units above the rest: the output IS its V row."""
    lay = layout(G)
    B, Hq = len(lay["run"]), HKV * G
    rng = np.random.default_rng(11 + D + G)
    varena = round_to(rng.standard_normal((lay["nblk"], HKV, BS, D)).astype(np.float32), dtype)
    karena = np.zeros_like(varena)
    karena[0], varena[0] = 7.0, 7.0
    q = np.zeros((B, Hq, D), np.float32)
    want = np.zeros((B, Hq, D), np.float32)
    picked = set()
    for si in range(len(lay["set_run"])):
        for m, b in enumerate(range(lay["ptr"][si], lay["ptr"][si + 1])):
            run, n = lay["run"][b], lay["n_keys"][b]
            cand = sorted({k for k in (0, run - 1, run, n - 1, run // 2, 111, 112, 127, 128, 159, 160, 255, 256, run + 16, run + 150)
                           if 0 <= k < n})
            for h in range(Hq):
                kh, g = h // G, h % G
                key, d = cand[(m * G + g + 3 * kh) % len(cand)], (5 * (m * G + g) + 1) % D
                q[b, h, d] = 64.0
                karena[lay["tab"][b, key // BS], kh, key % BS, d] = 64.0
                want[b, h] = varena[lay["tab"][b, key // BS], kh, key % BS]
                picked |= {"run" if key < run else "new" if key == n - 1 else "tail", ("first", key == 0), ("last of run", key == run - 1)}
    assert picked >= {"run", "tail", "new", ("first", True), ("last of run", True)}
    got, = launch(lay, D, G, dtype, q, karena, varena)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:8]


@pytest.mark.parametrize("dtype,D,G", CASES)
def test_random_data(dtype, D, G):
    """Random data against float64 softmax(q K^T / sqrt(D)) V (16-bit: assert_rule; float32: rtol 1e-5, atol 2e-6); two launches, same bits."""
    lay = layout(G)
    B, Hq = len(lay["run"]), HKV * G
    rng = np.random.default_rng(23 + D + G)
    karena = round_to(rng.standard_normal((lay["nblk"], HKV, BS, D)).astype(np.float32), dtype)
    varena = round_to(rng.standard_normal((lay["nblk"], HKV, BS, D)).astype(np.float32), dtype)
    karena[0], varena[0] = 7.0, 7.0
    q = round_to(rng.standard_normal((B, Hq, D)).astype(np.float32), dtype)
    want = np.zeros((B, Hq, D), np.float64)
    for b, n in enumerate(lay["n_keys"]):
        for h in range(Hq):
            idx = (lay["tab"][b, np.arange(n) // BS], h // G, np.arange(n) % BS)      # row b's first n K / V rows through its table
            sc = karena[idx].astype(np.float64) @ q[b, h].astype(np.float64) * D ** -0.5
            w = np.exp(sc - sc.max())
            want[b, h] = (w / w.sum()) @ varena[idx].astype(np.float64)
    got, again = launch(lay, D, G, dtype, q, karena, varena, repeat=2)
    assert np.array_equal(got, again)
    if dtype == "float32":
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    else:
        assert_rule(got.reshape(B, Hq * D), round_to(want.astype(np.float32), dtype).reshape(B, Hq * D), dtype, f"shared D {D} G {G} {dtype}")
