"""Float32-KV decode attention (-m gpu), variant 0 of mi_op_attention_decode: the lane maps of its matrix-core loop, the
per-wave trip count and the cut of the cached keys over the splits in whole 16-key tiles.

* Exact lane-map test: one-hot queries and keys make every softmax weight exactly 0 or 1, so a head's output row must be
  one V row bit for bit; each head has its own (key, d), so a permuted or transposed operand map cannot pass.
* Random data against the float64 oracle at the bound test_gpu_kernels.py holds for this kernel (rtol 1e-5, atol 2e-6).
* Engine-level decode runs whose KV length crosses a 16-key and a 128 x nsplit boundary: 32 rows at one split, and 8 rows at
  2 splits and across a change of the split count (3 -> 4).
"""
import numpy as np
import pytest

from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

import attn_f32_cases as f32  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from gpu_helpers import attention_decode, attn_shape, dev, dev_i32, host, identity_rope, rope_tables  # noqa: E402

ACT = "float32"


# ---------------------------------------------------------------------------------------------------------------------------
# exact lane maps

LANE_POS = [1099, 640, 300, 129, 128, 17, 16, 0]       # cached keys per row: three rounds at 4 splits ... the new key alone


def _lane_keys(pos, nsplit):
    """Keys that exercise every place of the kernel's walk for a row of `pos` cached keys: per split the first, a middle and
    the last key of its first tile, a key of wave 3, a key of the second round (wave 1), the last tile's first and last key
    (the ragged one), and the new key."""
    chunk = -(-pos // (16 * nsplit)) * 16
    keys = []
    for sp in range(nsplit):
        s0, send = sp * chunk, min(sp * chunk + chunk, pos)
        for k in (s0, s0 + 7, s0 + 15, s0 + 16 * 3 + 5, s0 + 128 + 16 + 1, (send - 1) // 16 * 16, send - 1):
            if s0 <= k < send and k not in keys:
                keys.append(k)
    return keys + [pos]


@pytest.mark.parametrize("nsplit", [1, 3, 4])
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 2, 128), (6, 2, 128), (2, 2, 64), (5, 1, 128)])
def test_one_hot_scores_select_one_v_row_bit_for_bit(Hq, Hkv, D, nsplit):
    """q[h] = 64 e_d, K[key_h][d_h] = 64, everything else 0, identity RoPE: head h's score is 4096 x scale x log2(e) >= 522 at
    key_h and 0 elsewhere, exp2(-522) is 0 in float32, so every weight, correction factor and sum is exactly 0 or 1 and the
    output row of head h IS V[key_h] (the new value row where key_h is the new key) -- whatever the split count."""
    B, G = len(LANE_POS), Hq // Hkv
    cap = max(LANE_POS) + 8
    rng = np.random.default_rng(99)
    nqkv = (Hq + 2 * Hkv) * D
    vc = rng.standard_normal((B, Hkv, cap, D)).astype(np.float32)
    vnew = rng.standard_normal((B, Hkv * D)).astype(np.float32)
    cand = [_lane_keys(pos, nsplit) for pos in LANE_POS]
    cos, sin = identity_rope(cap + 1, D)
    s = attn_shape(B, 1, Hq, Hkv, D, ACT, ACT, 0, cap)
    vc_d, off_d = dev(vc), dev_i32(LANE_POS)
    seen_keys, seen_d = set(), set()
    for p in range(-(-max(len(c) for c in cand) // Hq)):              # launches until every candidate key has had a head
        kc = np.zeros((B, Hkv, cap, D), np.float32)
        qkv = np.zeros((B, nqkv), np.float32)
        qkv[:, (Hq + Hkv) * D:] = vnew
        want = np.zeros((B, Hq, D), np.float32)
        for b, pos in enumerate(LANE_POS):
            for h in range(Hq):
                kh, g = h // G, h % G
                key = cand[b][(p * Hq + h) % len(cand[b])]
                d = (5 * (b * Hkv + kh) + 37 * g + 3 * p) % D           # distinct within a GQA group (37 g mod 64 / 128, g < 5)
                qkv[b, h * D + d] = 64.0
                if key == pos:
                    qkv[b, (Hq + kh) * D + d] = 64.0                    # the new key: from the q|k|v row
                    want[b, h] = vnew[b, kh * D:(kh + 1) * D]
                else:
                    kc[b, kh, key, d] = 64.0
                    want[b, h] = vc[b, kh, key]
                seen_keys.add((b, key))
                seen_d.add(((d % 16) // 4, d // 64))
        got = attention_decode(s, dev(qkv), dev(kc), vc_d, off_d, cos, sin, nsplit).reshape(B, Hq, D)
        bad = [(b, h) for b in range(B) for h in range(Hq) if not np.array_equal(got[b, h], want[b, h])]
        assert not bad, (p, bad[:8], len(bad))
    # the sweep reached every candidate key of every row, every lane-group quarter of d and every 64-half
    assert seen_keys == {(b, k) for b in range(B) for k in cand[b]}
    assert seen_d == {(q, hf) for q in range(4) for hf in range(D // 64)}


# ---------------------------------------------------------------------------------------------------------------------------
# random data against the float64 oracle

GEOMS = [(8, 2, 128), (6, 2, 128), (5, 1, 128), (2, 2, 64)]


@pytest.mark.parametrize("nsplit", [1, 3, 4, 8, 16])
@pytest.mark.parametrize("batch", ["ragged", "long"])
@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
def test_random_rows_against_the_oracle(Hq, Hkv, D, batch, nsplit):
    """Ragged rows around the 16-key tile and the 128-key round (waves and whole splits without keys, one ragged tile), 1100
    keys (a third round on two waves only at 4 splits) and 2047 (sixteen rounds at one split); the cache receives exactly the
    new K / V row."""
    c = f32.random_case(Hq, Hkv, D, batch)
    cos, sin = rope_tables(D, f32.max_pos(batch), f32.ROPE_BASE)
    B = len(c["offs"])
    s = attn_shape(B, 1, Hq, Hkv, D, ACT, ACT, 0, c["cap"])
    kc_d, vc_d = dev(c["kc"]), dev(c["vc"])
    got = attention_decode(s, dev(c["qkv"]), kc_d, vc_d, dev_i32(c["offs"]), cos, sin, nsplit)
    gk, gv = host(kc_d), host(vc_d)
    for b, o in enumerate(c["offs"]):
        assert np.allclose(gk[b, :, o], c["kc_ref"][b, :, o], rtol=2e-5, atol=4e-5)      # (RoPE in float32 against float64 tables)
        gk[b, :, o] = c["kc_ref"][b, :, o]
    assert np.array_equal(gk, c["kc_ref"]) and np.array_equal(gv, c["vc_ref"])      # nothing but the new row was written
    err = np.abs(got - c["want"]).max()
    print(f"Hq {Hq} Hkv {Hkv} D {D} {batch} nsplit {nsplit}: max |err| {err:.3e}")
    assert np.allclose(got, c["want"], rtol=1e-5, atol=2e-6), err


# ---------------------------------------------------------------------------------------------------------------------------
# engine level

def test_engine_decode_across_tile_and_round_boundaries(tmp_path):
    """A float32 model of its own (one layer, 16 query / 8 kv heads of 64: G = 2, the matrix-core kernel) in the float32-KV
    mode, 32 rows: 256 (row, kv head) pairs fill the CUs, so the engine takes one split, and the KV length runs from 123 to
    133 -- over the 16-key tile boundary at 128, which is also the 128 x nsplit boundary where a second round begins.
    Teacher-forced against the oracle as in test_gpu_engine.py: token ids equal, logprobs within the mode's 1e-3.
    (Multi-split launches of 8 rows through the engine, attn_decode_mfma_qs_kernel included, are held against the oracle by
    tests/test_gpu_golden_wide.py at the Mistral-7B width: B = 8, float32 KV 1024 -> 1100, 4 splits.)"""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(str(tmp_path), seed=12, vocab_size=256, dtype="float32", quantize_model=False, hidden_size=64, layers=1,
                           heads=16, kv_heads=8, intermediate_size=128, head_dim=64, tie_word_embeddings=False, with_tokenizer=False)
    model = utils.load_model(str(tmp_path), max_positions=256)
    ref = ref_generate.load(str(tmp_path), max_pos=256)
    B, L0, steps = 32, 122, 10
    rng = np.random.default_rng(11)
    y = rng.integers(3, cfg["vocab_size"], size=(B, L0)).astype(np.int32)
    kv = model.engine.new_kv(B, capacity=L0 + steps + 1, kv_dtype="float32")
    cache = ref.make_cache(B, paged=True)
    lp_err = 0.0
    for s in range(steps):
        res = model.engine.decode_sample(kv, y.astype(np.int32), SampleArgs(temp=0.0))
        want = ref_sample.sample(ref(y, cache=cache)[:, -1], temp=0.0)
        assert np.array_equal(res["tokens"], want["tokens"][:, 0]), (s, res["tokens"], want["tokens"][:, 0])
        lp_err = max(lp_err, float(np.abs(res["logprobs"] - want["logprobs"]).max()))
        y = want["tokens"].astype(np.int32)
    assert kv.offsets == [L0 + steps - 1] * B, kv.offsets
    assert lp_err <= 1e-3, lp_err
    model.engine.close()


@pytest.mark.parametrize("kv_heads", [16, 8])
def test_engine_decode_of_8_rows_across_tile_round_and_split_boundaries(tmp_path, kv_heads):
    """A bf16 model of its own (two layers, G = 2 query heads of 64 per kv head: the matrix-core kernel) in the float32-KV
    mode, 8 rows, KV length 251 -> 262 over the 16-key tile boundary at 256.  16 kv heads: 128 (row, kv head) pairs, so
    choose_nsplit takes 2 splits and 256 is also the 128 x nsplit boundary where a split's second round begins.  8 kv heads:
    64 pairs, 3 splits below 256 keys and 4 from there on (the float32 rule: the count that fills the CUs).  8 rows of
    float32 activations on bf16 weights is the shape whose second layer may take the q|k|v partial rows in the attention
    prologue (attn_decode_mfma_qs_kernel; tests/test_gpu_golden_wide.py holds that kernel against the oracle at the Mistral-7B
    width, B = 8, KV 1024 -> 1100, 4 splits).  Teacher-forced against the oracle as test_gpu_engine.py does for 16-bit models
    in this mode: token ids equal except for at most one near-tie inside the oracle's 2e-3 margin, logprobs within 1e-3."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(str(tmp_path), seed=12, vocab_size=256, dtype="bfloat16", quantize_model=False, hidden_size=256, layers=2,
                           heads=2 * kv_heads, kv_heads=kv_heads, intermediate_size=256, head_dim=64, tie_word_embeddings=False,
                           with_tokenizer=False, norm_jitter=0.1)
    model = utils.load_model(str(tmp_path), max_positions=320)
    ref = ref_generate.load(str(tmp_path), max_pos=320)
    B, L0, steps = 8, 250, 12
    rng = np.random.default_rng(11)
    y = rng.integers(3, cfg["vocab_size"], size=(B, L0)).astype(np.int32)
    kv = model.engine.new_kv(B, capacity=L0 + steps + 1, kv_dtype="float32")
    cache = ref.make_cache(B, paged=True)
    near, lp_err = 0, 0.0
    for s in range(steps):
        res = model.engine.decode_sample(kv, y.astype(np.int32), SampleArgs(temp=0.0))
        logits = ref(y, cache=cache)[:, -1]
        want = ref_sample.sample(logits, temp=0.0)
        for b in range(B):
            wt, gt = int(want["tokens"][b, 0]), int(res["tokens"][b])
            if wt != gt:
                margin = float(logits[b, wt] - logits[b, gt])
                assert 0 <= margin <= 2e-3, f"step {s} row {b}: token {gt} != {wt}, oracle margin {margin}"
                near += 1
            else:
                lp_err = max(lp_err, abs(float(res["logprobs"][b]) - float(want["logprobs"][b])))
        y = want["tokens"].astype(np.int32)
    assert kv.offsets == [L0 + steps - 1] * B, kv.offsets
    assert near <= 1 and lp_err <= 1e-3, (near, lp_err)
    model.engine.close()
