"""mi_op_kv_copy_tokens (-m gpu): the one-launch tail copy of mi_kv_fork_row against NumPy, bit for bit.  Every layer, KV head
and both caches get the span; everything else -- the sentinels around the destination spans, the other heads' tails, the
other blocks / rows, the source -- keeps its bits."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from gpu_helpers import MIDT, ptr  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402

LAYERS = 2
NP_INT = {"float32": np.int32, "bfloat16": np.int16}


def _copy(k, v, dtype, layer_elems, Hkv, D, head_stride, src_off, dst_off, n, check=True):
    torch.cuda.synchronize()
    rc = L.lib().mi_op_kv_copy_tokens(ptr(k), ptr(v), MIDT[dtype], LAYERS, layer_elems, Hkv, D, head_stride, src_off, dst_off, n)
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


def _caches(dtype, elems, seed):
    """K and V of LAYERS x elems elements as raw bit patterns (every pattern is legal: the kernel moves bytes)."""
    rng = np.random.default_rng(seed)
    it = NP_INT[dtype]
    info = np.iinfo(it)
    k = rng.integers(info.min, info.max, size=(LAYERS, elems), endpoint=True).astype(it)
    v = rng.integers(info.min, info.max, size=(LAYERS, elems), endpoint=True).astype(it)
    return k, v


def _expected(a, Hkv, D, head_stride, src_off, dst_off, n):
    want = a.copy()
    for h in range(Hkv):
        s, d = src_off + h * head_stride, dst_off + h * head_stride
        want[:, d:d + n * D] = a[:, s:s + n * D]
    return want


@pytest.mark.parametrize("n", [1, 15, 63])
@pytest.mark.parametrize("Hkv", [1, 3])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_paged_tail_copy(dtype, D, Hkv, n):
    """Arena [block][Hkv][64][D], 5 blocks: the first n tokens of block 3 go to block 1."""
    bs, nblocks, src_blk, dst_blk = 64, 5, 3, 1
    head, blk = bs * D, Hkv * bs * D
    k, v = _caches(dtype, nblocks * blk, seed=D + Hkv + n)
    kd, vd = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    _copy(kd, vd, dtype, nblocks * blk, Hkv, D, head, src_blk * blk, dst_blk * blk, n)
    for got, a in ((kd, k), (vd, v)):
        want = _expected(a, Hkv, D, head, src_blk * blk, dst_blk * blk, n)
        assert not np.array_equal(want, a)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 17, 100])
@pytest.mark.parametrize("Hkv", [1, 3])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_contiguous_row_copy(dtype, D, Hkv, n):
    """Cache [row][Hkv][cap][D], 3 rows of capacity 104: the first n tokens of row 0 go to row 2."""
    cap, rows, src, dst = 104, 3, 0, 2
    head, row = cap * D, Hkv * cap * D
    k, v = _caches(dtype, rows * row, seed=7 * D + Hkv + n)
    kd, vd = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    _copy(kd, vd, dtype, rows * row, Hkv, D, head, src * row, dst * row, n)
    for got, a in ((kd, k), (vd, v)):
        assert np.array_equal(got.cpu().numpy(), _expected(a, Hkv, D, head, src * row, dst * row, n))


def test_a_span_longer_than_one_pass_of_the_grid():
    """The grid is capped at 32 workgroups of 256 lanes per (layer, head, cache): 1000 tokens of 128 float32 are 32000 pieces,
    four rounds of the stride loop, the last one partial."""
    D, Hkv, cap, n = 128, 2, 1000, 1000
    head, row = cap * D, Hkv * cap * D
    k, v = _caches("float32", 2 * row, seed=3)
    kd, vd = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    _copy(kd, vd, "float32", 2 * row, Hkv, D, head, row, 0, n)
    for got, a in ((kd, k), (vd, v)):
        assert np.array_equal(got.cpu().numpy(), _expected(a, Hkv, D, head, row, 0, n))


def test_refusals_launch_nothing():
    D, Hkv, bs = 64, 2, 64
    head, blk = bs * D, Hkv * bs * D
    k, v = _caches("bfloat16", 4 * blk, seed=5)
    kd, vd = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    bad = [
        dict(D=4, n=1),                                  # an 8-byte span: no 16-byte piece
        dict(src_off=blk + 4),                           # an offset off the 16-byte grid
        dict(dst_off=3 * blk, n=bs + 1),                 # a span longer than the head
        dict(dst_off=3 * blk + head),                    # the last head's span leaves the layer
        dict(dst_off=blk + head),                        # head 0's destination is head 1's source
        dict(dst_off=blk + 8 * D, n=16),                 # source and destination overlap inside the head
        dict(n=0), dict(layers_elems_zero=True),
    ]
    for case in bad:
        a = dict(D=D, src_off=blk, dst_off=2 * blk, n=4, layer_elems=4 * blk)
        if case.pop("layers_elems_zero", False):
            a["layer_elems"] = 0
        a.update(case)
        rc = _copy(kd, vd, "bfloat16", a["layer_elems"], Hkv, a["D"], head, a["src_off"], a["dst_off"], a["n"], check=False)
        assert rc in (-1, -3), (case, rc)                # MI_ERR_INVALID / MI_ERR_UNSUPPORTED
        assert L.lib().mi_last_error().decode().startswith("kv_copy_tokens"), case
    assert _copy(kd, vd, "bfloat16", 4 * blk, Hkv, D, head, blk, 2 * blk, 4, check=False) == 0      # (the base case is good)
    want = _expected(k, Hkv, D, head, blk, 2 * blk, 4)
    assert np.array_equal(kd.cpu().numpy(), want)        # and nothing else was ever written
    with pytest.raises(ValueError):
        L.check(L.lib().mi_op_kv_copy_tokens(ptr(kd), ptr(vd), 7, LAYERS, 4 * blk, Hkv, D, head, blk, 2 * blk, 4))
