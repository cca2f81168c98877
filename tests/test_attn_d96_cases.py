"""What tests/test_gpu_attn_d96.py rests on and needs no device, at head_dim 96 with 1, 2 and 4 query heads per KV head:

* the one-hot probes and candidate keys of tests/attn16_cases.py cover what they claim to cover at D = 96 (the hot
  dimensions 37 g mod 96 stay distinct within a group of 4), and the float64 oracle returns the expected V rows;
* the rule of the random-data tests as a condition on the REFERENCE, on exactly the geometries and inputs the device tests
  use: the oracle's float32-accumulating envelopes pass it, the same envelopes with 16-bit P break its 2 % cap.
"""
import pytest

import attn_d96_cases as d96
import test_attn_16bit_cases as base

ACTS = ["bfloat16", "float16"]


@pytest.mark.parametrize("D", d96.DS)
@pytest.mark.parametrize("G", d96.GS)
def test_prefill_one_hot_coverage(D, G):
    base.test_prefill_one_hot_coverage(D, G)


@pytest.mark.parametrize("D", d96.DS)
@pytest.mark.parametrize("G", d96.GS)
@pytest.mark.parametrize("nsplit", [1, 3, 8])
def test_decode_one_hot_coverage(D, G, nsplit):
    base.test_decode_one_hot_coverage(D, G, nsplit)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 96), (4, 1, 96)])
def test_prefill_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D):
    base.test_prefill_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,nsplit", [(2, 2, 96, 3), (4, 1, 96, 8)])
def test_decode_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D, nsplit):
    base.test_decode_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D, nsplit)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", d96.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_decode(act, Hq, Hkv, D, norm):
    base.test_reference_envelopes_under_the_rule_decode(act, Hq, Hkv, D, norm)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", d96.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_prefill(act, Hq, Hkv, D, norm):
    base.test_reference_envelopes_under_the_rule_prefill(act, Hq, Hkv, D, norm)


def test_geometries_are_head_dim_96_with_groups_of_one_two_and_four():
    geoms = [g[:3] for g in d96.RANDOM_GEOMS] + d96.UNFUSED_GEOMS + d96.F32_PREFILL_GEOMS + [d96.F32_UNFUSED_GEOM] + \
        [g for v in d96.F32_DECODE_GEOMS.values() for g in v]
    assert {Hq // Hkv for Hq, Hkv, _ in geoms} == {1, 2, 4} and all(Hq % Hkv == 0 and D == 96 for Hq, Hkv, D in geoms)
    assert all(D != 96 or Hq // Hkv not in (1, 2, 4) for Hq, Hkv, D in d96.REFUSED_GEOMS)
