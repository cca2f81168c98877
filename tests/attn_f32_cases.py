"""Random float32-KV decode batches and the float64 oracle's answers for them, shared (read-only) by
tests/test_gpu_attn_f32_blocks.py, tests/test_gpu_attn_gqa.py and tests/test_gpu_attn_d96.py; the float32 prefill case of the
last two.  No device: the kernel's RoPE tables come from
gpu_helpers.rope_tables(D, max_pos(batch), ROPE_BASE)."""
import functools

import numpy as np

import attn16_cases as cases
import attn_gqa_cases as gqa
from oracle import ref_model

ACT = "float32"
ROPE_BASE = 1e4
BATCHES = {"ragged": [0, 1, 15, 16, 17, 127, 128, 129], "long": [1100, 2047]}


def max_pos(batch):
    return max(BATCHES[batch]) + 16


@functools.lru_cache(maxsize=None)
def random_case(Hq, Hkv, D, batch):
    """Inputs and the oracle's output / cache rows, computed once and shared by every split count (never modified)."""
    offs = BATCHES[batch]
    B, cap = len(offs), max(offs) + 8
    rng = np.random.default_rng(4321 + Hq + D + len(offs))
    c_ref, s_ref = ref_model.rope_tables(D, ROPE_BASE, 1.0, max_pos(batch))
    nqkv = (Hq + 2 * Hkv) * D
    kc = rng.standard_normal((B, Hkv, cap, D)).astype(np.float32)
    vc = rng.standard_normal((B, Hkv, cap, D)).astype(np.float32)
    qkv = rng.standard_normal((B, 1, nqkv)).astype(np.float32)
    q = qkv[..., :Hq * D].reshape(B, 1, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, 1, Hkv, D)
    v = qkv[..., (Hq + Hkv) * D:].reshape(B, 1, Hkv, D).transpose(0, 2, 1, 3)
    pos = np.array([[o] for o in offs])
    q = ref_model.rope(q.transpose(0, 2, 1, 3), ACT, pos, c_ref, s_ref)
    k = ref_model.rope(k.transpose(0, 2, 1, 3), ACT, pos, c_ref, s_ref)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    want = np.zeros((B, Hq * D), np.float32)
    for b in range(B):
        kc_ref[b, :, offs[b]:offs[b] + 1] = k[b]
        vc_ref[b, :, offs[b]:offs[b] + 1] = v[b]
        n = offs[b] + 1
        o, _ = ref_model.sdpa(q[b:b + 1], kc_ref[b:b + 1, :, :n], vc_ref[b:b + 1, :, :n], D ** -0.5, None, ACT, ACT)
        want[b] = o[0].transpose(1, 0, 2).reshape(Hq * D)
    for a in (kc, vc, qkv, kc_ref, vc_ref, want):
        a.setflags(write=False)
    return dict(offs=offs, cap=cap, kc=kc, vc=vc, qkv=qkv.reshape(B, nqkv), kc_ref=kc_ref, vc_ref=vc_ref, want=want)


@functools.lru_cache(maxsize=None)
def prefill_case(Hq, Hkv, D, L_):
    """A cache that already holds the call's keys, the queries and the float64 oracle's outputs (read-only, shared)."""
    offs, cap = gqa.F32_PREFILL_OFFS, gqa.F32_PREFILL_CAP
    rng = np.random.default_rng(977 + 10 * Hq + D + L_)
    B = len(offs)
    kc = rng.standard_normal((B, Hkv, cap, D)).astype(np.float32)
    vc = rng.standard_normal((B, Hkv, cap, D)).astype(np.float32)
    q = rng.standard_normal((B, L_, Hq, D)).astype(np.float32)
    want = cases.prefill_oracle(q, kc, vc, offs, L_, D, "float32")
    for a in (kc, vc, q, want):
        a.setflags(write=False)
    return kc, vc, q, want
