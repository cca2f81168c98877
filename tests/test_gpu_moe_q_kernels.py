"""Kernel-level tests (-m gpu) of csrc/moe_q.hip through mi_op_moe_linear_q / mi_op_moe_mlp_q.  The exact test's terms are
multiples of 0.25 with 4 |y| < 2^24 (float32 sums exact, one rounding to T); W_hat values such as 1003.75 fit no 16-bit float,
so a kernel that dequantises to bf16 / f16 fails it.  Its last case is the steady state: K = 1152 is 9 int4 / 18 int8 blocks (3 / 5
rounds of a wave's block loop: prefetch ring, clamped tail) and an expert of 70 pairs takes two passes over the row tiles; biases
up to 248 there: 4 * 1152 * 4 * 503 and, for the offset form, 4 (1152 * 4 * 264 + 18 * 7936) stay below 2^24."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ref_quant
from oracle.numerics import round_to
from oracle.ref_model import Linear

pytestmark = pytest.mark.gpu

import moe_ref  # noqa: E402
from gpu_helpers import MIDT, dev, dev_i32, dev_u32, host, ptr  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from moe_q_ref import expert_linears  # noqa: E402
from test_gpu_moe_kernels import COUNTS, IDS, TYPES, _block_data, _routing, op_route  # noqa: E402
from test_gpu_skinny import _assert_close  # noqa: E402


def op_linear_q(x_d, K, x_rows, x_shift, act, q, sdt, bits, E, N, meta_d, list_d, pairs, out_d, group=64, x_ptr=None):
    return L.lib().mi_op_moe_linear_q(x_ptr or ptr(x_d), K, x_rows, x_shift, MIDT[act], 0, ptr(q[0]), ptr(q[1]), ptr(q[2]), MIDT[sdt], bits,
                                      group, E, N, K, ptr(meta_d), ptr(list_d), pairs, ptr(out_d), N, 0, None)


def dev_q(packed, scales, biases, sdt):
    return dev_u32(packed), dev(scales, sdt), dev(biases, sdt)


@pytest.mark.parametrize("act,sdt", TYPES, ids=IDS)
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("N,K", [(256, 128), (64, 128), (64, 256), (128, 256), (64, 1152)])
@pytest.mark.parametrize("x_shift", [0, 1])
def test_grouped_linear_is_bit_equal_to_numpy(act, sdt, bits, N, K, x_shift):
    rng = np.random.default_rng(N * 7 + K + x_shift + bits)
    counts, bmax = (COUNTS, 125) if K < 1152 else (COUNTS + [70], 31)
    E = len(counts)
    pairs, owner, meta, lst = _routing(rng, counts, spare=3)
    x_rows = (pairs + (1 << x_shift) - 1) >> x_shift
    x = rng.integers(-4, 5, size=(x_rows, K)).astype(np.float32)
    codes = rng.integers(0, 1 << bits, size=(E, N, K)).astype(np.uint32)
    scales = rng.choice([0.25, 0.5, 1.0], size=(E, N, K // 64)).astype(np.float32)
    biases = (8 * rng.integers(-bmax, bmax + 1, size=(E, N, K // 64))).astype(np.float32)
    per = 32 // bits
    packed = np.bitwise_or.reduce(codes.reshape(E, N, K // per, per) << (np.arange(per, dtype=np.uint32) * bits), axis=-1).astype(np.uint32)
    w_hat = np.repeat(scales, 64, axis=-1).astype(np.float64) * codes + np.repeat(biases, 64, axis=-1)
    out = torch.full((pairs, N), 7.0, dtype=dev(x[:1], act).dtype, device="cuda")
    L.check(op_linear_q(dev(x, act), K, x_rows, x_shift, act, dev_q(packed, scales, biases, sdt), sdt, bits, E, N, dev_i32(meta), dev_i32(lst),
                        pairs, out))
    want = np.full((pairs, N), 7.0, np.float32)                                   # a pair on no list keeps its contents
    for p in range(pairs):
        if owner[p] >= 0:
            want[p] = round_to((x[p >> x_shift].astype(np.float64) @ w_hat[owner[p]].T).astype(np.float32)[None], act)[0]
    got = host(out)
    assert np.array_equal(got, want), (act, bits, N, K, x_shift, np.argwhere(got != want)[:4])


def _q_block(act, sdt, bits, data, E, k):
    x, wr, wg, wu, wd, h = data
    (R, H), I = x.shape, wg.shape[1]
    qs = [[np.stack(t) for t in zip(*(ref_quant.quantize(m[e], 64, bits, sdt) for e in range(E)))] for m in (wg, wu, wd)]
    xd = dev(x, act)
    sel, score, meta, lst = op_route(xd, R, H, act, dev(wr, sdt), sdt, E, k)
    out = torch.zeros((R, H), dtype=xd.dtype, device="cuda")
    d = [t for q in qs for t in dev_q(*q, sdt)]
    L.check(L.lib().mi_op_moe_mlp_q(ptr(xd), H, R, H, I, MIDT[act], 0, MIDT[sdt], bits, 64, E, k, *[ptr(t) for t in d], ptr(meta), ptr(lst),
                                    ptr(score), ptr(dev(h, act)), H, ptr(out), H, 0, None))
    return (host(sel).astype(np.int64), host(score), host(out)), [expert_linears(*q, sdt, bits) for q in qs]


@pytest.mark.parametrize("act,sdt", TYPES, ids=IDS)
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("R,E,k", [(40, 8, 2), (17, 4, 1), (1, 4, 2)])
def test_mlp_matches_the_twins_arithmetic(act, sdt, bits, R, E, k):
    H, I = 128, 256
    data = _block_data(np.random.default_rng(100 * R + 10 * E + k + bits), act, sdt, R, H, I, E)
    x, wr, h = data[0], data[1], data[5]
    (sel, score, out), lins = _q_block(act, sdt, bits, data, E, k)
    w = {"model.layers.0.block_sparse_moe.gate": Linear(dtype=sdt, weight=wr)}
    w.update({f"model.layers.0.block_sparse_moe.experts.{e}.{n}": lins[j][e] for j, n in enumerate(("gate_proj", "up_proj", "down_proj")) for e in range(E)})
    twin = SimpleNamespace(w=w, top_k=k, n_experts=E, margins=[])
    r = moe_ref.MoeRefModel._mlp(twin, 0, x[None], act)[0][0]
    _i, margin, at = twin.margins[0]
    clear = margin >= 8 * moe_ref.ulp(at, act) if act != "float32" else margin >= 1e-4        # (a near-tie may go either way)
    assert R < 16 or clear.mean() >= 0.8
    _assert_close(out[clear], round_to(h + r, act)[clear], act, scale=float(np.sqrt(np.mean(np.square(r)))) + 1e-12)


@pytest.mark.parametrize("act,sdt", TYPES, ids=IDS)
@pytest.mark.parametrize("bits", [4, 8])
def test_a_rows_outputs_do_not_depend_on_its_neighbours(act, sdt, bits):
    R, H, I, E, k = 40, 128, 256, 8, 2
    x, wr, wg, wu, wd, h = _block_data(np.random.default_rng(77), act, sdt, R, H, I, E)
    (sel, score, out), _l = _q_block(act, sdt, bits, (x, wr, wg, wu, wd, h), E, k)
    for row in (0, 7, 39):
        (s1, c1, o1), _l1 = _q_block(act, sdt, bits, (x[row:row + 1], wr, wg, wu, wd, h[row:row + 1]), E, k)
        assert np.array_equal(s1[0], sel[row]) and np.array_equal(c1[0], score[row]) and np.array_equal(o1[0], out[row]), (act, bits, row)


def test_refusals():
    rng = np.random.default_rng(3)
    pairs, _owner, meta, lst = _routing(rng, [2, 3])
    x = dev(np.zeros((pairs + 1, 256), np.float32), "bfloat16")
    q = dev_q(np.zeros((2, 64, 32), np.uint32), np.zeros((2, 64, 8), np.float32), np.zeros((2, 64, 8), np.float32), "bfloat16")
    out = torch.zeros((pairs, 64), dtype=torch.bfloat16, device="cuda")

    def rc(meta_=meta, K=128, **kw):
        return op_linear_q(x, K, pairs, 0, "bfloat16", q, "bfloat16", 4, 2, 64, dev_i32(meta_), dev_i32(lst), pairs, out, **kw)

    assert rc() == 0
    assert rc(group=32) == -3 and b"groups of 64" in L.lib().mi_last_error()
    assert rc(K=192) == -3 and b"128" in L.lib().mi_last_error()                    # int4 runs on whole 128-k blocks
    assert rc(x_ptr=x.data_ptr() + 2) == -1 and b"misaligned" in L.lib().mi_last_error()
    assert rc(meta_=np.array([2, 4, 0, 2], np.int32)) == -1                         # a run past the list array
