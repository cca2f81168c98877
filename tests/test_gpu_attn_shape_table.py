"""Which head shapes the attention entries serve (-m gpu): every dtype x head_dim x Hq/Hkv, through mi_op_attention (one new
token: the unfused kernel; 18: the prefill kernels) and mi_op_attention_decode (variant 0: the matrix-core kernel where it
applies; 1: the vector-ALU kernel).  Only the return code is looked at: MI_OK for a served shape, MI_ERR_UNSUPPORTED for
any other -- and then nothing may have been launched, so the output keeps its sentinel.  The table is written out here, not
read from the library's source: a kernel family that loses (or gains) a shape by accident shows up as one line of this test.

One sequence, one kv head, a cache of 40 with 5 keys in it: a launch is one workgroup.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_helpers import attention, attention_decode, attn_shape, dev, dev_i32, identity_rope  # noqa: E402

MI_OK, MI_ERR_UNSUPPORTED = 0, -3
ACTS = ["float32", "bfloat16", "float16"]
DS = [16, 32, 48, 64, 80, 96, 128]
GS = [1, 2, 3, 4, 5, 6, 7, 8]
CAP, KEYS, SENTINEL = 40, 5, 7.0

GROUPS = {16: [1, 2, 3, 4, 5, 6, 8], 32: [1, 2, 3, 4, 5, 6, 8], 64: [1, 2, 3, 4, 5, 6, 8], 96: [1, 2, 4],
          128: [1, 2, 3, 4, 5, 6, 8]}


def served(entry, act, D, G):
    """The table: head_dim 16, 32, 64, 96 and 128 with the groups above; the fused decode kernels have no 16-wide head on
    16-bit caches."""
    if entry == "decode" and act != "float32" and D == 16:
        return False
    return G in GROUPS.get(D, [])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("act", ACTS)
def test_served_and_refused_shapes(act, D):
    rng = np.random.default_rng(D)
    off_d = dev_i32([KEYS])
    cos, sin = identity_rope(CAP + 1, D)
    answers, table = {}, {}
    for G in GS:
        Hq, Hkv = G, 1
        kc_d, vc_d = dev(rng.standard_normal((1, Hkv, CAP, D)), act), dev(rng.standard_normal((1, Hkv, CAP, D)), act)
        for L_ in (1, 18):
            s = attn_shape(1, L_, Hq, Hkv, D, act, act, 0, CAP)
            q_d = dev(rng.standard_normal((L_, Hq * D)), act)
            out = torch.full((L_, Hq * D), SENTINEL, dtype=q_d.dtype, device="cuda")
            rc = attention(s, q_d, kc_d, vc_d, off_d, out=out, check=False)
            answers["attention", L_, G] = rc, rc == MI_OK or bool((out == SENTINEL).all())
            table["attention", L_, G] = served("attention", act, D, G)
        s = attn_shape(1, 1, Hq, Hkv, D, act, act, 0, CAP)
        qkv_d = dev(rng.standard_normal((1, (Hq + 2 * Hkv) * D)), act)
        for variant in (0, 1):
            out = torch.full((1, Hq * D), SENTINEL, dtype=qkv_d.dtype, device="cuda")
            rc = attention_decode(s, qkv_d, kc_d.clone(), vc_d.clone(), off_d, cos, sin, 1, variant, out=out, check=False)
            answers["decode", variant, G] = rc, rc == MI_OK or bool((out == SENTINEL).all())
            table["decode", variant, G] = served("decode", act, D, G)
    want = {k: (MI_OK if ok else MI_ERR_UNSUPPORTED, True) for k, ok in table.items()}
    wrong = {k: (answers[k], want[k]) for k in want if answers[k] != want[k]}
    assert not wrong, wrong
