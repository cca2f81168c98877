"""GQA groups of 3 and 6 query heads per KV head (-m gpu) in every attention kernel: the matrix-core prefill kernels of
attn_prefill.hip (LDS-DMA, register-staged, the float32 pair), the fused decode kernels of attn_decode.hip (matrix-core
variant 0, VALU variant 1; 16-bit and float32 caches) and the unfused attn_kernel + attn_combine_kernel of attn.hip.

* 16-bit caches: the one-hot and random-data tests of tests/test_gpu_attn_16bit.py -- the same functions, called at the new
  geometries (tests/attn_gqa_cases.py); what they rest on is checked without a device in tests/test_attn_gqa_cases.py.
* float32 caches: the ragged and the long batch of tests/test_gpu_attn_f32_blocks.py against the float64 oracle at that
  file's bound, on both decode variants; the two prefill forms (two-term operands, MI_ATTN_PREFILL_F32_EXACT=1) at the bounds
  tests/test_gpu_kernels.py::test_prefill_attention_many_blocks holds for them; the unfused kernel.
* G = 7 is still refused by every entry with MI_ERR_UNSUPPORTED, and the output keeps its sentinel.

(The kernel-level C ABI takes contiguous caches only; the block-paged instantiations of these groups run in
tests/test_gpu_gqa_models.py, bit for bit against the contiguous ones.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_model

pytestmark = pytest.mark.gpu

import attn16_cases as cases  # noqa: E402
import attn_gqa_cases as gqa  # noqa: E402
import test_gpu_attn_16bit as base16  # noqa: E402
import attn_f32_cases as f32  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import attention, attention_decode, attn_shape, dev, dev_i32, host, identity_rope, ptr, rope_tables  # noqa: E402

ACTS = ["bfloat16", "float16"]
MI_ERR_UNSUPPORTED = -3


# ---------------------------------------------------------------------------------------------------------------------------
# 16-bit caches

@pytest.mark.parametrize("G", gqa.GS)
@pytest.mark.parametrize("D", gqa.DS)
@pytest.mark.parametrize("act", ACTS)
def test_prefill_one_hot_selects_one_v_row_bit_for_bit(act, D, G):
    base16.test_prefill_one_hot_selects_one_v_row_bit_for_bit(act, D, G)


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("G", gqa.GS)
@pytest.mark.parametrize("D", gqa.DS)
@pytest.mark.parametrize("act", ACTS)
def test_decode_one_hot_selects_one_v_row_bit_for_bit(act, D, G, nsplit):
    base16.test_decode_one_hot_selects_one_v_row_bit_for_bit(act, D, G, nsplit)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("Hq,Hkv,D", gqa.UNFUSED_GEOMS)
@pytest.mark.parametrize("act", ACTS)
def test_unfused_decode_one_hot_selects_one_v_row_bit_for_bit(act, Hq, Hkv, D, nsplit):
    base16.test_unfused_decode_one_hot_selects_one_v_row_bit_for_bit(act, Hq, Hkv, D, nsplit)


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", gqa.RANDOM_GEOMS)
def test_decode_random_rows_under_the_rule(Hq, Hkv, D, norm, act, variant, nsplit):
    base16.test_decode_random_rows_under_the_rule(Hq, Hkv, D, norm, act, variant, nsplit)


@pytest.mark.parametrize("L_", cases.RANDOM_PREFILL_L)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", gqa.RANDOM_GEOMS)
def test_prefill_random_rows_under_the_rule(Hq, Hkv, D, norm, act, L_):
    base16.test_prefill_random_rows_under_the_rule(Hq, Hkv, D, norm, act, L_)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 caches

@pytest.mark.parametrize("nsplit", [1, 3, 4, 8])
@pytest.mark.parametrize("batch", ["ragged", "long"])
@pytest.mark.parametrize("variant,Hq,Hkv,D", [(v, *g) for v, gs in gqa.F32_DECODE_GEOMS.items() for g in gs])
def test_f32_decode_random_rows_against_the_oracle(variant, Hq, Hkv, D, batch, nsplit):
    """tests/test_gpu_attn_f32_blocks.py::test_random_rows_against_the_oracle (its batches, its oracle, its bound) with the
    variant as a parameter: 0 = the 16x16x4 matrix-core loop at G = 6, 1 = the vector-ALU kernel at G = 3 and 6."""
    c = f32.random_case(Hq, Hkv, D, batch)
    cos, sin = rope_tables(D, f32.max_pos(batch), f32.ROPE_BASE)
    B = len(c["offs"])
    s = attn_shape(B, 1, Hq, Hkv, D, "float32", "float32", 0, c["cap"])
    kc_d, vc_d = dev(c["kc"]), dev(c["vc"])
    got = attention_decode(s, dev(c["qkv"]), kc_d, vc_d, dev_i32(c["offs"]), cos, sin, nsplit, variant)
    gk, gv = host(kc_d), host(vc_d)
    for b, o in enumerate(c["offs"]):
        assert np.allclose(gk[b, :, o], c["kc_ref"][b, :, o], rtol=2e-5, atol=4e-5)      # (RoPE in float32 against float64 tables)
        gk[b, :, o] = c["kc_ref"][b, :, o]
    assert np.array_equal(gk, c["kc_ref"]) and np.array_equal(gv, c["vc_ref"])      # nothing but the new row was written
    err = np.abs(got - c["want"])
    print(f"F32 decode variant {variant} ({Hq},{Hkv},{D}) {batch} nsplit {nsplit}: max |err| {err.max():.3e}, "
          f"max err / (1e-5 |want| + 2e-6) {float((err / (1e-5 * np.abs(c['want']) + 2e-6)).max()):.3f}")
    assert np.allclose(got, c["want"], rtol=1e-5, atol=2e-6), err.max()


@pytest.mark.parametrize("L_", gqa.F32_PREFILL_L)
@pytest.mark.parametrize("Hq,Hkv,D", gqa.F32_PREFILL_GEOMS)
def test_f32_prefill_both_forms_against_the_oracle(Hq, Hkv, D, L_):
    """attn_prefill_f32s_kernel (two-term bf16 operands, the default) within rtol 1e-4 / atol 2e-5 of the float64 oracle and
    attn_prefill_f32_kernel (MI_ATTN_PREFILL_F32_EXACT=1, exact products) within rtol 1e-5 / atol 2e-6: the bounds of
    tests/test_gpu_kernels.py::test_prefill_attention_many_blocks, here on every query."""
    kc, vc, q, want = f32.prefill_case(Hq, Hkv, D, L_)
    offs, B = gqa.F32_PREFILL_OFFS, len(gqa.F32_PREFILL_OFFS)
    s = attn_shape(B, L_, Hq, Hkv, D, "float32", "float32", 0, gqa.F32_PREFILL_CAP)
    q_d, kc_d, vc_d, off_d = dev(q.reshape(B * L_, Hq * D)), dev(kc), dev(vc), dev_i32(offs)
    two = host(attention(s, q_d, kc_d, vc_d, off_d, exact="0")).reshape(B, L_, Hq, D)
    exact = host(attention(s, q_d, kc_d, vc_d, off_d, exact="1")).reshape(B, L_, Hq, D)
    print(f"F32 prefill ({Hq},{Hkv},{D}) L {L_}: max |err| two-term {np.abs(two - want).max():.3e}, exact {np.abs(exact - want).max():.3e}")
    assert np.allclose(two, want, rtol=1e-4, atol=2e-5), np.abs(two - want).max()
    assert np.allclose(exact, want, rtol=1e-5, atol=2e-6), np.abs(exact - want).max()


@pytest.mark.parametrize("nsplit", [1, 3])
def test_f32_unfused_decode_against_the_oracle(nsplit):
    """mi_op_attention with L = 1 on float32 caches (attn_kernel + attn_combine_kernel) over the caches the fused kernel leaves
    behind, at the bound tests/test_gpu_kernels.py holds for this kernel (rtol 1e-4, atol 2e-5)."""
    Hq, Hkv, D = gqa.F32_UNFUSED_GEOM
    c = f32.random_case(Hq, Hkv, D, "ragged")
    B = len(c["offs"])
    s = attn_shape(B, 1, Hq, Hkv, D, "float32", "float32", 0, c["cap"])
    # (the unfused kernel takes q after RoPE: rotated here with the oracle's tables)
    c_ref, s_ref = ref_model.rope_tables(D, 1e4, 1.0, max(c["offs"]) + 16)
    q = c["qkv"][:, :Hq * D].reshape(B, 1, Hq, D).transpose(0, 2, 1, 3)
    q = ref_model.rope(q, "float32", np.array([[o] for o in c["offs"]]), c_ref, s_ref).transpose(0, 2, 1, 3).reshape(B, Hq * D)
    got = host(attention(s, dev(q), dev(c["kc_ref"]), dev(c["vc_ref"]), dev_i32(c["offs"]), nsplit))
    print(f"F32 unfused ({Hq},{Hkv},{D}) nsplit {nsplit}: max |err| {np.abs(got - c['want']).max():.3e}")
    assert np.allclose(got, c["want"], rtol=1e-4, atol=2e-5), np.abs(got - c["want"]).max()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals

@pytest.mark.parametrize("act", ["bfloat16", "float16", "float32"])
def test_seven_query_heads_per_kv_head_are_still_refused(act):
    """Hq / Hkv = 7: MI_ERR_UNSUPPORTED from the unfused kernel, the prefill kernels and both fused decode variants (device
    and host lookups); nothing is launched, so the output buffer keeps its sentinel."""
    Hq, Hkv, D, B, cap = 7, 1, 64, 2, 40
    nqkv = (Hq + 2 * Hkv) * D
    rng = np.random.default_rng(5)
    kc_d, vc_d = dev(rng.standard_normal((B, Hkv, cap, D)), act), dev(rng.standard_normal((B, Hkv, cap, D)), act)
    off_d = dev_i32([5, 9])
    cos, sin = identity_rope(cap + 1, D)
    lib = L.lib()
    for L_ in (1, 18):
        s = attn_shape(B, L_, Hq, Hkv, D, act, act, 0, cap)
        q_d = dev(rng.standard_normal((B * L_, Hq * D)), act)
        out = torch.full((B * L_, Hq * D), 7.0, dtype=q_d.dtype, device="cuda")
        part = torch.zeros((B * L_ * Hq * 3 * (D + 2),), dtype=torch.float32, device="cuda")
        for nsplit in ((1, 3) if L_ == 1 else (1,)):
            torch.cuda.synchronize()
            rc = lib.mi_op_attention(C.byref(s), ptr(q_d), ptr(kc_d), ptr(vc_d), ptr(off_d), ptr(out), float(D ** -0.5), nsplit, ptr(part))
            assert rc == MI_ERR_UNSUPPORTED and b"1, 2, 3, 4, 5, 6 or 8" in lib.mi_last_error(), (L_, nsplit, rc, lib.mi_last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all())
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cap)
    qkv_d = dev(rng.standard_normal((B, nqkv)), act)
    kc0, vc0 = kc_d.clone(), vc_d.clone()
    out = torch.full((B, Hq * D), 7.0, dtype=qkv_d.dtype, device="cuda")
    part = torch.zeros((B * Hq * 3 * (D + 2),), dtype=torch.float32, device="cuda")
    ctr = torch.zeros((B * Hkv,), dtype=torch.int32, device="cuda")
    hrow, hoff = (C.c_int32 * B)(0, 1), (C.c_int32 * B)(5, 9)
    for variant in (0, 1):
        for nsplit in (1, 3):
            args = (C.byref(s), ptr(qkv_d), ptr(kc_d), ptr(vc_d), ptr(off_d), None, None, cases.EPS, ptr(cos), ptr(sin), ptr(out),
                    float(D ** -0.5), 0, nsplit, ptr(part), ptr(ctr), variant, 1, None)
            torch.cuda.synchronize()
            for rc in (lib.mi_op_attention_decode(*args), lib.mi_op_attention_decode_host(*args, None, hrow, hoff)):
                assert rc == MI_ERR_UNSUPPORTED, (variant, nsplit, rc, lib.mi_last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and torch.equal(kc_d, kc0) and torch.equal(vc_d, vc0) and not ctr.cpu().numpy().any()
