"""What tests/test_gpu_attn_16bit.py rests on and needs no device (tests/attn16_cases.py):

* the one-hot constructions: the float64 oracle returns exactly the V rows the test's own winner arithmetic expects, and the
  probes / candidate keys cover what they claim to cover;
* the rule of the random-data tests as a condition on the REFERENCE: on the very inputs the device tests use, the oracle's
  float32-accumulating envelopes (numerics.set_accum) pass it with a wide margin, and the same envelopes with the softmax
  numerators rounded to ONE 16-bit value (numerics.set_sdpa_p16) break its 2 % cap -- so the cap separates a kernel that
  feeds P to the matrix core as hi + lo from one that rounds it;
* gpu_helpers.close_frac counts a non-finite output as far.
"""
import numpy as np
import pytest

from oracle import numerics, ref_model

import attn16_cases as cases
from gpu_helpers import close_frac

ACTS = ["bfloat16", "float16"]


# ---------------------------------------------------------------------------------------------------------------------------
# one-hot constructions

@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 2, 128), (5, 1, 32), (2, 1, 64)])
def test_prefill_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D):
    c = cases.prefill_one_hot(Hq, Hkv, D, act)
    got = cases.prefill_oracle(c["q"], c["k"], c["v"], cases.PREFILL_OFFS, cases.PREFILL_L, D, act)
    assert np.array_equal(got, c["want"])


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 5, 8])
def test_prefill_one_hot_coverage(D, G):
    c = cases.prefill_one_hot(2 * G, 2, D, "bfloat16")
    cases.assert_prefill_coverage(c, D)
    offs = np.array(cases.PREFILL_OFFS)[:, None, None]
    t = np.arange(cases.PREFILL_L)[None, :, None]
    assert (c["winner"] <= offs + t).all() and (c["winner"] > offs + t - D).all() and (c["winner"] >= 0).all()


def test_decode_candidates_hold_both_sides_of_every_cut():
    for pos in cases.DECODE_POS:
        for nsplit in (1, 3, 8):
            keys = cases.decode_candidates(pos, nsplit)
            assert keys[-1] == pos and len(set(keys)) == len(keys) and all(0 <= k <= pos for k in keys)
            chunk = -(-pos // nsplit)
            for sp in range(nsplit):
                s0, send = sp * chunk, min(sp * chunk + chunk, pos)
                if s0 < send:
                    assert s0 in keys and send - 1 in keys
    assert {k // 32 for k in cases.decode_candidates(1099, 1) if k < 256} == set(range(8))     # every wave's span of a round
    assert any(256 <= k < 512 for k in cases.decode_candidates(1099, 3))                        # a second round
    assert len(cases.decode_candidates(2, 8)) == 3 and len(cases.decode_candidates(5, 8)) == 6  # empty splits beside full ones


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("nsplit", [1, 3, 8])
def test_decode_one_hot_coverage(D, G, nsplit):
    cand, launches = cases.decode_launches(2 * G, 2, D, nsplit)
    cases.assert_decode_coverage(cand, launches, D)
    for _, d in launches:                                  # distinct hot dimensions within a GQA group
        assert all(len(set(row[kh * G:(kh + 1) * G])) == G for row in d for kh in range(2))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,nsplit", [(4, 2, 128, 3), (8, 1, 64, 8), (10, 2, 32, 1)])
def test_decode_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D, nsplit):
    """The first launch of the sweep through the float64 oracle, over the cache the kernel must leave behind."""
    _, launches = cases.decode_launches(Hq, Hkv, D, nsplit)
    vc, vnew = cases.decode_values(Hkv, D, act)
    key, d = launches[0]
    qkv, _, want, kc_after, vc_after = cases.decode_one_hot(Hq, Hkv, D, key, d, vc, vnew)
    for b, pos in enumerate(cases.DECODE_POS):
        q = qkv[b, :Hq * D].reshape(1, Hq, 1, D)
        o, _ = ref_model.sdpa(q, kc_after[b:b + 1, :, :pos + 1], vc_after[b:b + 1, :, :pos + 1], D ** -0.5, None, act, act)
        assert np.array_equal(o[0, :, 0], want[b]), (b, pos)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule on the reference side

def _envelopes(oracle):
    """The exact oracle's output and [(name, output)] of the float32-accumulating envelopes without / with 16-bit P."""
    want = oracle()
    out = []
    try:
        for p16 in (False, True):
            numerics.set_sdpa_p16(p16)
            for mode in ("f32_seq32", "f32_pairwise"):
                numerics.set_accum(mode)
                out.append((mode, p16, oracle()))
    finally:
        numerics.set_accum("exact")
        numerics.set_sdpa_p16(False)
    return want, out


def _check_envelopes(want, envs, act, what):
    for mode, p16, got in envs:
        worst, frac = cases.rule_stats(got, want, act)
        print(f"{what} {mode} P16 {p16}: worst {worst:.3f} unit, {100 * frac:.3f} % beyond half a unit")
        if p16:
            assert frac > 0.02, (what, mode, frac)         # single-term P: on the far side of the cap
        else:
            assert worst <= 1.0 and frac <= 0.001, (what, mode, worst, frac)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", cases.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_decode(act, Hq, Hkv, D, norm):
    lens = cases.RANDOM_DECODE_LENS
    inp = cases.random_inputs(Hq, Hkv, D, act, len(lens), 1, len(lens), max(lens) + 8, seed=31)
    want, envs = _envelopes(lambda: cases.attention_oracle(inp, Hq, Hkv, D, act, norm, lens)[0])
    _check_envelopes(want, envs, act, f"decode ({Hq},{Hkv},{D}) {act}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", cases.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_prefill(act, Hq, Hkv, D, norm):
    offs = cases.RANDOM_PREFILL_OFFS
    for L in (17, 50):                                     # (L = 2: six queries, too few elements for a fraction of 2 %)
        inp = cases.random_inputs(Hq, Hkv, D, act, len(offs), L, len(offs), cases.RANDOM_PREFILL_CAP, seed=47)
        want, envs = _envelopes(lambda: cases.attention_oracle(inp, Hq, Hkv, D, act, norm, offs)[0])
        _check_envelopes(want, envs, act, f"prefill L {L} ({Hq},{Hkv},{D}) {act}")


def test_rule_counts_non_finite_outputs_as_far():
    want = np.linspace(-2, 2, 64).astype(np.float32)
    assert cases.rule_stats(want, want, "bfloat16") == (0.0, 0.0)
    got = want.copy()
    got[3] = np.nan
    worst, frac = cases.rule_stats(got, want, "bfloat16")
    assert worst == np.inf and frac == 1 / 64
    with pytest.raises(AssertionError):
        cases.assert_rule(got, want, "bfloat16")
    got[3] = np.inf
    assert cases.rule_stats(got, want, "float16")[0] == np.inf
    step = want * (1 + 2.0 ** -8)                          # one bfloat16 step at most: inside one unit, beyond half of one
    worst, frac = cases.rule_stats(step, want, "bfloat16")
    assert 0.49 < worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# gpu_helpers.close_frac

def test_close_frac_counts_non_finite_outputs_as_far():
    want = np.array([1.0, -2.0, 0.5, 0.0, 3.0, 100.0, -0.25, 8.0], np.float32)
    assert close_frac(np.full_like(want, np.nan), want, "bfloat16", atol=1e-3) == 1.0
    assert close_frac(np.full_like(want, np.inf), want, "float16") == 1.0
    got = want.copy()
    got[2] = np.nan
    assert close_frac(got, want, "bfloat16", atol=1e-3) == 1 / 8
    # finite values: as before -- far means |got - want| > 2^-7 max(|want|, |got|) + atol
    assert close_frac(want, want, "bfloat16") == 0.0
    got = want * np.array([1, 1 + 2.0 ** -8, 1 + 2.0 ** -6, 1, 1 - 2.0 ** -6, 1 + 2.0 ** -9, 1, 1], np.float32)
    assert close_frac(got, want, "bfloat16") == 2 / 8
    assert close_frac(got, want, "float16") == 4 / 8
    got = want + np.float32(5e-4)
    assert close_frac(got, want, "float16", atol=1e-3) == 0.0
    assert close_frac(got, want, "float16", atol=0.0) == 3 / 8        # 5e-4 > 2^-10 |x| for |x| < 0.51: 0.5, 0 and -0.25
