"""Float32-KV decode attention (-m gpu): the head of the kernel -- where a workgroup learns its cache row and KV length.

The engine passes both in the kernel arguments (AttnDecodeCall::host_row / host_off, B <= 32); the op-level entry
mi_op_attention_decode and row-subset steps leave them to two dependent device loads (rows[b], then offsets[row]).
mi_op_attention_decode_host reaches both lookups at kernel level:

* the two lookups agree bit for bit (outputs and both caches), on a cache of 12 rows addressed through a non-identity
  permutation, and both meet the float64 oracle at the bound test_gpu_kernels.py holds for this kernel (rtol 1e-5, atol 2e-6).
  The host-lookup call gets no device `rows` and a zeroed device `offsets`: a kernel that ignored either host array fails;
* the same call twice on the same buffers gives the same output, and the arrival tickets are back at zero.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ref_model

pytestmark = pytest.mark.gpu

from gpu_helpers import attention_decode, attn_shape, dev, dev_i32, host, rope_tables  # noqa: E402

ACT = "float32"
LENS = [0, 1, 15, 16, 17, 127, 128, 129]               # cached keys of batch entry b
ROWS = [7, 2, 11, 0, 5, 9, 3, 6]                       # ... which lives in this row of a 12-row cache
NROWS = 12
GEOMS = [(8, 2, 128), (5, 1, 128)]                     # G = 4: the 16-block loop; G = 5: the 16x16x4 loop


def _i32(a):
    return (C.c_int32 * len(a))(*a)


def _decode(c, nsplit, lookup, kc_d, vc_d, repeat=1):
    """lookup "device": rows[b] and offsets[row] are loaded by the kernel, "host": both come with the arguments."""
    Hq, Hkv, D = c["geom"]
    s = attn_shape(len(LENS), 1, Hq, Hkv, D, ACT, ACT, 0, c["cap"])
    if lookup == "host":
        off_d, rows_d, hrow, hoff = dev_i32(np.zeros(NROWS)), None, _i32(ROWS), _i32(LENS)
    else:
        off_d, rows_d, hrow, hoff = dev_i32(c["row_lens"]), dev_i32(ROWS), None, None
    cos, sin = rope_tables(D, max(LENS) + 16, 1e4)
    return attention_decode(s, dev(c["qkv"]), kc_d, vc_d, off_d, cos, sin, nsplit, rows_d=rows_d, hrow=hrow, hoff=hoff,
                            repeat=repeat)


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, D):
    """Inputs and the oracle's output / cache rows, computed once and shared by every test (never modified)."""
    B, cap, max_pos = len(LENS), max(LENS) + 8, max(LENS) + 16
    rng = np.random.default_rng(977 + Hq + D)
    c_ref, s_ref = ref_model.rope_tables(D, 1e4, 1.0, max_pos)
    nqkv = (Hq + 2 * Hkv) * D
    kc = rng.standard_normal((NROWS, Hkv, cap, D)).astype(np.float32)
    vc = rng.standard_normal((NROWS, Hkv, cap, D)).astype(np.float32)
    qkv = rng.standard_normal((B, 1, nqkv)).astype(np.float32)
    q = qkv[..., :Hq * D].reshape(B, 1, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, 1, Hkv, D)
    v = qkv[..., (Hq + Hkv) * D:].reshape(B, 1, Hkv, D).transpose(0, 2, 1, 3)
    pos = np.array([[o] for o in LENS])
    q = ref_model.rope(q.transpose(0, 2, 1, 3), ACT, pos, c_ref, s_ref)
    k = ref_model.rope(k.transpose(0, 2, 1, 3), ACT, pos, c_ref, s_ref)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    want = np.zeros((B, Hq * D), np.float32)
    row_lens = np.full(NROWS, 3, np.int32)                 # rows outside the call: a length nobody may act on
    for b, (r, n) in enumerate(zip(ROWS, LENS)):
        row_lens[r] = n
        kc_ref[r, :, n:n + 1] = k[b]
        vc_ref[r, :, n:n + 1] = v[b]
        o, _ = ref_model.sdpa(q[b:b + 1], kc_ref[r:r + 1, :, :n + 1], vc_ref[r:r + 1, :, :n + 1], D ** -0.5, None, ACT, ACT)
        want[b] = o[0].transpose(1, 0, 2).reshape(Hq * D)
    for a in (kc, vc, qkv, kc_ref, vc_ref, want, row_lens):
        a.setflags(write=False)
    return dict(geom=(Hq, Hkv, D), cap=cap, kc=kc, vc=vc, qkv=qkv.reshape(B, nqkv), kc_ref=kc_ref, vc_ref=vc_ref,
                want=want, row_lens=row_lens)


@pytest.mark.parametrize("nsplit", [1, 4])
@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
def test_host_and_device_lookup_agree_bit_for_bit(Hq, Hkv, D, nsplit):
    c = _case(Hq, Hkv, D)
    res = {}
    for lookup in ("device", "host"):
        kc_d, vc_d = dev(c["kc"]), dev(c["vc"])
        res[lookup] = (_decode(c, nsplit, lookup, kc_d, vc_d), host(kc_d), host(vc_d))
    (od, kd, vd), (oh, kh, vh) = res["device"], res["host"]
    assert np.array_equal(oh, od), np.abs(oh - od).max()
    assert np.array_equal(kh, kd) and np.array_equal(vh, vd)
    for b, (r, n) in enumerate(zip(ROWS, LENS)):
        assert np.allclose(kh[r, :, n], c["kc_ref"][r, :, n], rtol=2e-5, atol=4e-5)    # (RoPE in float32 against float64 tables)
        kh[r, :, n] = c["kc_ref"][r, :, n]
    assert np.array_equal(kh, c["kc_ref"]) and np.array_equal(vh, c["vc_ref"])      # nothing but the new rows was written
    for name, o in (("device", od), ("host", oh)):
        err = np.abs(o - c["want"]).max()
        print(f"Hq {Hq} Hkv {Hkv} D {D} nsplit {nsplit} {name} lookup: max |err| {err:.3e}")
        assert np.allclose(o, c["want"], rtol=1e-5, atol=2e-6), (name, err)


@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
def test_same_call_twice_on_the_same_buffers(Hq, Hkv, D):
    """Nothing of the first launch's prologue (q in LDS, partials, tickets) may reach the second: equal outputs, tickets at
    zero after each (checked inside), the oracle's bound on both."""
    c = _case(Hq, Hkv, D)
    first, second = _decode(c, 4, "host", dev(c["kc"]), dev(c["vc"]), repeat=2)
    assert np.array_equal(first, second), np.abs(first - second).max()
    assert np.allclose(second, c["want"], rtol=1e-5, atol=2e-6), np.abs(second - c["want"]).max()
