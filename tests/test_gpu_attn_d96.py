"""head_dim 96 (Phi-3's width) with 1, 2 and 4 query heads per KV head (-m gpu) in every attention kernel: the matrix-core
prefill kernels of attn_prefill.hip (LDS-DMA, register-staged, the float32 two-term form), the fused decode kernels of
attn_decode.hip (matrix-core variant 0, VALU variant 1; 16-bit and float32 caches) and the unfused attn_kernel +
attn_combine_kernel of attn.hip.

* 16-bit caches: the one-hot and random-data tests of tests/test_gpu_attn_16bit.py -- the same functions, called at the new
  geometries (tests/attn_d96_cases.py); what they rest on is checked without a device in tests/test_attn_d96_cases.py.  The
  VALU decode kernel (variant 1) serves 16-bit caches at this width, so the random-data decode test runs on both variants.
* float32 caches: the ragged and the long batch of tests/test_gpu_attn_f32_blocks.py against the float64 oracle at that
  file's bound, on both decode variants; the two-term prefill at the bound tests/test_gpu_kernels.py holds for it; the
  exact-product prefill (MI_ATTN_PREFILL_F32_EXACT=1) refuses this width before it launches; the unfused kernel.
* D = 96 with 3, 5, 6 or 8 query heads per KV head, and D = 48 / 80, are refused by every entry with MI_ERR_UNSUPPORTED;
  outputs, caches and ticket counters keep their sentinels.

(The kernel-level C ABI takes contiguous caches only; the block-paged instantiations run in tests/test_gpu_phi3_models.py,
bit for bit against the contiguous ones.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_model

pytestmark = pytest.mark.gpu

import attn16_cases as cases  # noqa: E402
import attn_d96_cases as d96  # noqa: E402
import test_gpu_attn_16bit as base16  # noqa: E402
import attn_f32_cases as f32  # noqa: E402
import test_gpu_attn_gqa as gqa_tests  # noqa: E402
from mlx_parallm_amd import _lib as L  # noqa: E402
from gpu_helpers import attention, attn_shape, dev, dev_i32, host, identity_rope, ptr  # noqa: E402

ACTS = ["bfloat16", "float16"]
MI_ERR_UNSUPPORTED = -3


# ---------------------------------------------------------------------------------------------------------------------------
# 16-bit caches

@pytest.mark.parametrize("G", d96.GS)
@pytest.mark.parametrize("D", d96.DS)
@pytest.mark.parametrize("act", ACTS)
def test_prefill_one_hot_selects_one_v_row_bit_for_bit(act, D, G):
    base16.test_prefill_one_hot_selects_one_v_row_bit_for_bit(act, D, G)


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("G", d96.GS)
@pytest.mark.parametrize("D", d96.DS)
@pytest.mark.parametrize("act", ACTS)
def test_decode_one_hot_selects_one_v_row_bit_for_bit(act, D, G, nsplit):
    base16.test_decode_one_hot_selects_one_v_row_bit_for_bit(act, D, G, nsplit)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("Hq,Hkv,D", d96.UNFUSED_GEOMS)
@pytest.mark.parametrize("act", ACTS)
def test_unfused_decode_one_hot_selects_one_v_row_bit_for_bit(act, Hq, Hkv, D, nsplit):
    base16.test_unfused_decode_one_hot_selects_one_v_row_bit_for_bit(act, Hq, Hkv, D, nsplit)


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", d96.RANDOM_GEOMS)
def test_decode_random_rows_under_the_rule(Hq, Hkv, D, norm, act, variant, nsplit):
    base16.test_decode_random_rows_under_the_rule(Hq, Hkv, D, norm, act, variant, nsplit)


@pytest.mark.parametrize("L_", cases.RANDOM_PREFILL_L)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", d96.RANDOM_GEOMS)
def test_prefill_random_rows_under_the_rule(Hq, Hkv, D, norm, act, L_):
    base16.test_prefill_random_rows_under_the_rule(Hq, Hkv, D, norm, act, L_)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 caches

@pytest.mark.parametrize("nsplit", [1, 3, 4, 8])
@pytest.mark.parametrize("batch", ["ragged", "long"])
@pytest.mark.parametrize("variant,Hq,Hkv,D", [(v, *g) for v, gs in d96.F32_DECODE_GEOMS.items() for g in gs])
def test_f32_decode_random_rows_against_the_oracle(variant, Hq, Hkv, D, batch, nsplit):
    """tests/test_gpu_attn_f32_blocks.py::test_random_rows_against_the_oracle (its batches, its oracle, its bound: rtol 1e-5,
    atol 2e-6) with the variant as a parameter: 0 = the 16-block matrix-core loop with its 64 + 32 split of a V row, 1 = the
    vector-ALU kernel, a second opinion that shares none of that tiling."""
    gqa_tests.test_f32_decode_random_rows_against_the_oracle(variant, Hq, Hkv, D, batch, nsplit)


@pytest.mark.parametrize("L_", d96.F32_PREFILL_L)
@pytest.mark.parametrize("Hq,Hkv,D", d96.F32_PREFILL_GEOMS)
def test_f32_prefill_two_term_against_the_oracle_and_exact_form_refused(Hq, Hkv, D, L_):
    """attn_prefill_f32s_kernel (two-term bf16 operands, the default) within rtol 1e-4 / atol 2e-5 of the float64 oracle on
    every query.  attn_prefill_f32_kernel (MI_ATTN_PREFILL_F32_EXACT=1) builds its V image from 64-wide halves of a row: it
    refuses D = 96 with MI_ERR_UNSUPPORTED (NotImplementedError through the binding) before it launches."""
    kc, vc, q, want = f32.prefill_case(Hq, Hkv, D, L_)
    offs, B = d96.F32_PREFILL_OFFS, len(d96.F32_PREFILL_OFFS)
    s = attn_shape(B, L_, Hq, Hkv, D, "float32", "float32", 0, d96.F32_PREFILL_CAP)
    q_d, kc_d, vc_d, off_d = dev(q.reshape(B * L_, Hq * D)), dev(kc), dev(vc), dev_i32(offs)
    two = host(attention(s, q_d, kc_d, vc_d, off_d, exact="0")).reshape(B, L_, Hq, D)
    print(f"F32 prefill ({Hq},{Hkv},{D}) L {L_}: max |err| two-term {np.abs(two - want).max():.3e}")
    assert np.allclose(two, want, rtol=1e-4, atol=2e-5), np.abs(two - want).max()
    with pytest.raises(NotImplementedError, match="exact float32 form"):
        attention(s, q_d, kc_d, vc_d, off_d, exact="1")


@pytest.mark.parametrize("nsplit", [1, 3])
def test_f32_unfused_decode_against_the_oracle(nsplit):
    """mi_op_attention with L = 1 on float32 caches (attn_kernel + attn_combine_kernel) over the caches the fused kernel leaves
    behind, at the bound tests/test_gpu_kernels.py holds for this kernel (rtol 1e-4, atol 2e-5)."""
    Hq, Hkv, D = d96.F32_UNFUSED_GEOM
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
@pytest.mark.parametrize("Hq,Hkv,D", d96.REFUSED_GEOMS)
def test_other_groups_at_96_and_other_widths_are_refused(Hq, Hkv, D, act):
    """D = 96 with Hq / Hkv of 3, 5, 6 or 8, and D = 48 / 80: MI_ERR_UNSUPPORTED from the unfused kernel, the prefill kernels and
    both fused decode variants (device and host lookups); nothing is launched, so outputs, caches and ticket counters keep
    what they held."""
    B, cap = 2, 40
    nqkv = (Hq + 2 * Hkv) * D
    rng = np.random.default_rng(5)
    kc_d, vc_d = dev(rng.standard_normal((B, Hkv, cap, D)), act), dev(rng.standard_normal((B, Hkv, cap, D)), act)
    kc0, vc0 = kc_d.clone(), vc_d.clone()
    off_d = dev_i32([5, 9])
    cos, sin = identity_rope(cap + 1, D)
    lib = L.lib()
    for L_ in (1, 18):
        s = attn_shape(B, L_, Hq, Hkv, D, act, act, 0, cap)
        q_d = dev(rng.standard_normal((B * L_, Hq * D)), act)
        out = torch.full((B * L_, Hq * D), 7.0, dtype=q_d.dtype, device="cuda")
        part = torch.full((B * L_ * Hq * 3 * (D + 2),), 7.0, dtype=torch.float32, device="cuda")
        for nsplit in ((1, 3) if L_ == 1 else (1,)):
            torch.cuda.synchronize()
            rc = lib.mi_op_attention(C.byref(s), ptr(q_d), ptr(kc_d), ptr(vc_d), ptr(off_d), ptr(out), float(D ** -0.5), nsplit, ptr(part))
            assert rc == MI_ERR_UNSUPPORTED, (L_, nsplit, rc, lib.mi_last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and bool((part == 7.0).all())
    s = attn_shape(B, 1, Hq, Hkv, D, act, act, 0, cap)
    qkv_d = dev(rng.standard_normal((B, nqkv)), act)
    out = torch.full((B, Hq * D), 7.0, dtype=qkv_d.dtype, device="cuda")
    part = torch.full((B * Hq * 3 * (D + 2),), 7.0, dtype=torch.float32, device="cuda")
    ctr = torch.full((B * Hkv,), 7, dtype=torch.int32, device="cuda")
    hrow, hoff = (C.c_int32 * B)(0, 1), (C.c_int32 * B)(5, 9)
    for variant in (0, 1):
        for nsplit in (1, 3):
            args = (C.byref(s), ptr(qkv_d), ptr(kc_d), ptr(vc_d), ptr(off_d), None, None, cases.EPS, ptr(cos), ptr(sin), ptr(out),
                    float(D ** -0.5), 0, nsplit, ptr(part), ptr(ctr), variant, 1, None)
            torch.cuda.synchronize()
            for rc in (lib.mi_op_attention_decode(*args), lib.mi_op_attention_decode_host(*args, None, hrow, hoff)):
                assert rc == MI_ERR_UNSUPPORTED, (variant, nsplit, rc, lib.mi_last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and bool((part == 7.0).all()) and bool((ctr == 7).all())
    assert torch.equal(kc_d, kc0) and torch.equal(vc_d, vc0)
