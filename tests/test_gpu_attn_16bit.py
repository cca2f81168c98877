"""bfloat16 / float16 attention kernels (-m gpu): the matrix-core prefill kernels of attn_prefill.hip (LDS-DMA and
register-staged), the fused decode kernels of attn_decode.hip (matrix-core variant 0, VALU variant 1) and the unfused
attn_kernel + attn_combine_kernel of attn.hip, at every (head_dim, Hq / Hkv) instantiation: D in {32, 64, 128} x G in
{1, 2, 4, 5, 8}, both dtypes.  Inputs, expectations and the rule live in tests/attn16_cases.py; what they rest on is checked
without a device in tests/test_attn_16bit_cases.py.

1. Prefill, exact: one-hot queries and keys select exactly one V row per (query, head) -- the diagonal key, the class of the
   first masked key (a mask that leaks one key returns another row), distances 1, 2, D/2, 3, 5, 7, 15, 17, 31 -- in every
   query slot of a tile, offsets on both sides of the diagonal-block condition, a long row that walks the K / V ring.  Both
   kernels, bit for bit.
2. Fused decode, exact: per row and split count a sweep over both sides of every split cut (0 .. 1099 cached keys, 1 / 3 / 8
   splits: cuts inside a 16-key tile and a wave's 32 keys, empty splits beside occupied ones), every wave's span, a second
   round, the last cached key and the new key, with stale decoy rows at pos and pos + 1; the cache receives exactly the new
   row and the tickets are back at zero.  The unfused kernels on the same inputs over an extended cache.
3. Random data against the float64 oracle under a rule with a bound on the worst element (cases.assert_rule): every output
   finite, every element within 1 unit of 2^-7 / 2^-10 x max(|want|, |got|, rms(want) of the output row), at most 2 % of a
   case's elements beyond half a unit.
4. The cache-row and length lookups of mi_op_attention_decode_host (device rows + offsets against host_row + host_off, as
   the engine's decode step passes them) on 16-bit caches: bit-identical, under the rule, and repeatable.

Measured on an MI355X (worst element / worst fraction beyond half a unit over all cases of part 3 and 4):
  prefill, LDS-DMA = register-staged   bf16 0.985 unit / 0.26 %    f16 0.981 unit / 0.26 %   (0.26 %: L = 2, one of 384
                                                                                             elements; L = 17 / 50: <= 0.09 %)
  fused decode, matrix-core (0)        bf16 0.623 unit / 0.033 %   f16 0.583 unit / 0.026 %
  fused decode, VALU (1)               bf16 0.019 unit / 0 %       f16 0.583 unit / 0.026 %
The oracle's own float32-accumulating envelopes on the same inputs: <= 0.99 unit / <= 0.036 %; with P rounded to one 16-bit
value: 5.4 - 9.3 % beyond half a unit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn16_cases as cases  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import attention, attention_decode, attn_shape, dev, dev_i32, host, identity_rope, ptr, rope_tables  # noqa: E402

ACTS = ["bfloat16", "float16"]
DS = [32, 64, 128]
GS = [1, 2, 4, 5, 8]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. prefill: exact key selection and the causal edge

@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("act", ACTS)
def test_prefill_one_hot_selects_one_v_row_bit_for_bit(act, D, G):
    Hq, Hkv = 2 * G, 2
    c = cases.prefill_one_hot(Hq, Hkv, D, act)
    cases.assert_prefill_coverage(c, D)
    if (D, G) == (128, 4):                                 # the expectation does not rest on the winner arithmetic alone
        assert np.array_equal(cases.prefill_oracle(c["q"], c["k"], c["v"], cases.PREFILL_OFFS, cases.PREFILL_L, D, act), c["want"])
    B, L_ = len(cases.PREFILL_OFFS), cases.PREFILL_L
    s = attn_shape(B, L_, Hq, Hkv, D, act, act, 0, cases.PREFILL_CAP)
    q_d, kc_d, vc_d = dev(c["q"].reshape(B * L_, Hq * D), act), dev(c["k"], act), dev(c["v"], act)
    off_d = dev_i32(cases.PREFILL_OFFS)
    outs = {dma: attention(s, q_d, kc_d, vc_d, off_d, dma=dma) for dma in ("1", "0")}
    for dma, out in outs.items():
        got = host(out).reshape(B, L_, Hq, D)
        bad = [(b, t, h, int(c["winner"][b, t, h])) for b in range(B) for t in range(L_) for h in range(Hq)
               if not np.array_equal(got[b, t, h], c["want"][b, t, h])]
        assert not bad, (dma, bad[:8], len(bad))
    assert torch.equal(outs["1"], outs["0"])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. fused decode: exact key selection, the split cut, stale rows

@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("act", ACTS)
def test_decode_one_hot_selects_one_v_row_bit_for_bit(act, D, G, nsplit):
    Hq, Hkv = 2 * G, 2
    B = len(cases.DECODE_POS)
    cand, launches = cases.decode_launches(Hq, Hkv, D, nsplit)
    cases.assert_decode_coverage(cand, launches, D)
    vc, vnew = cases.decode_values(Hkv, D, act)
    cos, sin = identity_rope(cases.DECODE_CAP + 1, D)
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cases.DECODE_CAP)
    off_d, vc0_d = dev_i32(cases.DECODE_POS), dev(vc, act)
    rows_i, pos_i = torch.arange(B, device="cuda"), torch.tensor(cases.DECODE_POS, device="cuda")
    vca_d = vc0_d.clone()                                  # the caches the call must leave behind: the new rows at pos
    vca_d[rows_i, :, pos_i] = dev(vnew, act).reshape(B, Hkv, D)
    for p, (key, d) in enumerate(launches):
        qkv, kc, want = cases.decode_one_hot(Hq, Hkv, D, key, d, vc, vnew, after=False)
        qkv_d, kc0_d = dev(qkv, act), dev(kc, act)
        kca_d = kc0_d.clone()
        kca_d[rows_i, :, pos_i] = qkv_d[:, Hq * D:(Hq + Hkv) * D].reshape(B, Hkv, D)
        for variant in (0, 1):
            kc_d, vc_d = kc0_d.clone(), vc0_d.clone()
            got = attention_decode(s, qkv_d, kc_d, vc_d, off_d, cos, sin, nsplit, variant).reshape(B, Hq, D)
            bad = [(b, h, int(key[b, h])) for b in range(B) for h in range(Hq) if not np.array_equal(got[b, h], want[b, h])]
            assert not bad, (variant, p, bad[:8], len(bad))
            # the new K / V row at pos, nothing else
            assert torch.equal(kc_d, kca_d) and torch.equal(vc_d, vca_d), (variant, p)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 128), (8, 1, 64), (10, 2, 32)])
@pytest.mark.parametrize("act", ACTS)
def test_unfused_decode_one_hot_selects_one_v_row_bit_for_bit(act, Hq, Hkv, D, nsplit):
    """mi_op_attention with L = 1: attn_kernel + attn_combine_kernel over a cache that already holds the new row (only the
    decoy at pos + 1 is left of the stale rows)."""
    B = len(cases.DECODE_POS)
    cand, launches = cases.decode_launches(Hq, Hkv, D, nsplit)
    cases.assert_decode_coverage(cand, launches, D)
    vc, vnew = cases.decode_values(Hkv, D, act)
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cases.DECODE_CAP)
    off_d = dev_i32(cases.DECODE_POS)
    for p, (key, d) in enumerate(launches):
        qkv, _, want, kc_after, vc_after = cases.decode_one_hot(Hq, Hkv, D, key, d, vc, vnew)
        q_d = dev(qkv[:, :Hq * D], act)
        got = host(attention(s, q_d, dev(kc_after, act), dev(vc_after, act), off_d, nsplit)).reshape(B, Hq, D)
        bad = [(b, h, int(key[b, h])) for b in range(B) for h in range(Hq) if not np.array_equal(got[b, h], want[b, h])]
        assert not bad, (p, bad[:8], len(bad))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. random data against the float64 oracle

@functools.lru_cache(maxsize=None)
def _random_decode_case(Hq, Hkv, D, norm, act):
    """Inputs and the oracle's outputs / caches, computed once and shared by every variant and split count (read-only)."""
    lens = cases.RANDOM_DECODE_LENS
    inp = cases.random_inputs(Hq, Hkv, D, act, len(lens), 1, len(lens), max(lens) + 8, seed=31)
    want, kc_ref, vc_ref = cases.attention_oracle(inp, Hq, Hkv, D, act, norm, lens)
    for a in (want, kc_ref, vc_ref):
        a.setflags(write=False)
    return inp, want[:, 0], kc_ref, vc_ref


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", cases.RANDOM_GEOMS)
def test_decode_random_rows_under_the_rule(Hq, Hkv, D, norm, act, variant, nsplit):
    inp, want, kc_ref, vc_ref = _random_decode_case(Hq, Hkv, D, norm, act)
    lens = cases.RANDOM_DECODE_LENS
    B, cap = len(lens), max(lens) + 8
    cos, sin = rope_tables(D, cap + 8, cases.rope_base(norm))
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cap)
    kc_d, vc_d = dev(inp["kc"], act), dev(inp["vc"], act)
    qn_d, kn_d = (dev(inp["qn"], act), dev(inp["kn"], act)) if norm else (None, None)
    got = attention_decode(s, dev(inp["qkv"][:, 0], act), kc_d, vc_d, dev_i32(lens), cos, sin, nsplit, variant,
                           qn_d=qn_d, kn_d=kn_d)
    cases.check_new_rows(host(kc_d), host(vc_d), kc_ref, vc_ref, range(B), lens, act)
    cases.assert_rule(got, want, act, f"decode variant {variant} ({Hq},{Hkv},{D}) {act} nsplit {nsplit}")


@functools.lru_cache(maxsize=None)
def _random_prefill_case(Hq, Hkv, D, norm, act, L_):
    offs = cases.RANDOM_PREFILL_OFFS
    inp = cases.random_inputs(Hq, Hkv, D, act, len(offs), L_, len(offs), cases.RANDOM_PREFILL_CAP, seed=47)
    want, kc_ref, vc_ref = cases.attention_oracle(inp, Hq, Hkv, D, act, norm, offs)
    for a in (want, kc_ref, vc_ref):
        a.setflags(write=False)
    return inp, want, kc_ref, vc_ref


@pytest.mark.parametrize("L_", cases.RANDOM_PREFILL_L)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", cases.RANDOM_GEOMS)
def test_prefill_random_rows_under_the_rule(Hq, Hkv, D, norm, act, L_):
    """mi_op_rope_append, then both prefill kernels over the cache it extended."""
    inp, want, kc_ref, vc_ref = _random_prefill_case(Hq, Hkv, D, norm, act, L_)
    offs = cases.RANDOM_PREFILL_OFFS
    B, cap, max_pos = len(offs), cases.RANDOM_PREFILL_CAP, cases.RANDOM_PREFILL_CAP + 8
    nqkv = (Hq + 2 * Hkv) * D
    cos, sin = rope_tables(D, max_pos, cases.rope_base(norm))
    s = attn_shape(B, L_, Hq, Hkv, D, act, act, 0, cap)
    qkv_d, kc_d, vc_d = dev(inp["qkv"].reshape(B * L_, nqkv), act), dev(inp["kc"], act), dev(inp["vc"], act)
    q_d = torch.zeros((B * L_, Hq * D), dtype=qkv_d.dtype, device="cuda")
    off_d = dev_i32(offs)
    qn_d, kn_d = (dev(inp["qn"], act), dev(inp["kn"], act)) if norm else (None, None)
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_rope_append(C.byref(s), ptr(qkv_d), ptr(q_d), ptr(kc_d), ptr(vc_d), ptr(off_d), ptr(qn_d), ptr(kn_d),
                                      cases.EPS, ptr(cos), ptr(sin), max_pos))
    torch.cuda.synchronize()
    assert np.array_equal(host(vc_d), vc_ref)
    outs = {dma: attention(s, q_d, kc_d, vc_d, off_d, dma=dma) for dma in ("1", "0")}
    assert torch.equal(outs["1"], outs["0"])
    cases.assert_rule(host(outs["1"]).reshape(B, L_, Hq * D), want, act, f"prefill ({Hq},{Hkv},{D}) {act} L {L_}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. cache-row and length lookups

def _i32(a):
    return (C.c_int32 * len(a))(*a)


@functools.lru_cache(maxsize=None)
def _lookup_case(Hq, Hkv, D, act):
    """12 cache rows, 8 batch entries addressed through a non-identity permutation; rows outside the call carry a length
    nobody may act on."""
    lens, rows = cases.LOOKUP_LENS, cases.LOOKUP_ROWS
    inp = cases.random_inputs(Hq, Hkv, D, act, len(lens), 1, cases.LOOKUP_NROWS, cases.LOOKUP_CAP, seed=53)
    want, kc_ref, vc_ref = cases.attention_oracle(inp, Hq, Hkv, D, act, False, lens, rows)
    row_lens = np.full(cases.LOOKUP_NROWS, 3, np.int32)
    row_lens[rows] = lens
    for a in (want, kc_ref, vc_ref, row_lens):
        a.setflags(write=False)
    return inp, want[:, 0], kc_ref, vc_ref, row_lens


def _lookup_args(lookup, row_lens):
    """-> (device offsets, device rows, host_row, host_off); "host": no device rows and a zeroed device offsets array, so a
    kernel that ignored either host array fails."""
    if lookup == "host":
        return dev_i32(np.zeros(cases.LOOKUP_NROWS)), None, _i32(cases.LOOKUP_ROWS), _i32(cases.LOOKUP_LENS)
    return dev_i32(row_lens), dev_i32(cases.LOOKUP_ROWS), None, None


@pytest.mark.parametrize("nsplit", [1, 4])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D", cases.LOOKUP_GEOMS)
def test_host_and_device_lookup_agree_bit_for_bit(Hq, Hkv, D, act, variant, nsplit):
    inp, want, kc_ref, vc_ref, row_lens = _lookup_case(Hq, Hkv, D, act)
    B = len(cases.LOOKUP_LENS)
    cos, sin = rope_tables(D, cases.LOOKUP_CAP + 8, cases.rope_base(False))
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cases.LOOKUP_CAP)
    qkv_d = dev(inp["qkv"][:, 0], act)
    res = {}
    for lookup in ("device", "host"):
        kc_d, vc_d = dev(inp["kc"], act), dev(inp["vc"], act)
        off_d, rows_d, hrow, hoff = _lookup_args(lookup, row_lens)
        first, second = attention_decode(s, qkv_d, kc_d, vc_d, off_d, cos, sin, nsplit, variant, rows_d=rows_d, hrow=hrow,
                                         hoff=hoff, repeat=2)
        assert np.array_equal(first, second), lookup       # the same call twice on the same buffers
        res[lookup] = (second, host(kc_d), host(vc_d))
    (od, kd, vd), (oh, kh, vh) = res["device"], res["host"]
    assert np.array_equal(oh, od)
    assert np.array_equal(kh, kd) and np.array_equal(vh, vd)
    cases.check_new_rows(kh, vh, kc_ref, vc_ref, cases.LOOKUP_ROWS, cases.LOOKUP_LENS, act)
    for name, o in (("device", od), ("host", oh)):
        cases.assert_rule(o, want, act, f"decode variant {variant} ({Hq},{Hkv},{D}) {act} nsplit {nsplit} {name} lookup")
