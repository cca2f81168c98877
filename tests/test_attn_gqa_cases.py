"""What tests/test_gpu_attn_gqa.py rests on and needs no device, for GQA groups of 3 and 6 query heads per KV head:

* the one-hot probes and candidate keys of tests/attn16_cases.py cover what they claim to cover at G = 3 and 6 (the hot
  dimensions 37 g mod D stay distinct within a group of 6), and the float64 oracle returns the expected V rows;
* the rule of the random-data tests as a condition on the REFERENCE, on exactly the geometries and inputs the device tests
  use: the oracle's float32-accumulating envelopes pass it, the same envelopes with 16-bit P break its 2 % cap.
"""
import pytest

import attn_gqa_cases as gqa
import test_attn_16bit_cases as base

ACTS = ["bfloat16", "float16"]


@pytest.mark.parametrize("D", gqa.DS)
@pytest.mark.parametrize("G", gqa.GS)
def test_prefill_one_hot_coverage(D, G):
    base.test_prefill_one_hot_coverage(D, G)


@pytest.mark.parametrize("D", gqa.DS)
@pytest.mark.parametrize("G", gqa.GS)
@pytest.mark.parametrize("nsplit", [1, 3, 8])
def test_decode_one_hot_coverage(D, G, nsplit):
    base.test_decode_one_hot_coverage(D, G, nsplit)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D", [(6, 2, 128), (12, 2, 32)])
def test_prefill_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D):
    base.test_prefill_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,nsplit", [(6, 2, 128, 3), (6, 1, 64, 8)])
def test_decode_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D, nsplit):
    base.test_decode_one_hot_oracle_returns_the_expected_rows(act, Hq, Hkv, D, nsplit)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", gqa.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_decode(act, Hq, Hkv, D, norm):
    base.test_reference_envelopes_under_the_rule_decode(act, Hq, Hkv, D, norm)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Hq,Hkv,D,norm", gqa.RANDOM_GEOMS)
def test_reference_envelopes_under_the_rule_prefill(act, Hq, Hkv, D, norm):
    base.test_reference_envelopes_under_the_rule_prefill(act, Hq, Hkv, D, norm)


def test_geometries_are_groups_of_three_and_six():
    geoms = [g[:3] for g in gqa.RANDOM_GEOMS] + gqa.UNFUSED_GEOMS + gqa.F32_PREFILL_GEOMS + [gqa.F32_UNFUSED_GEOM] + \
        [g for v in gqa.F32_DECODE_GEOMS.values() for g in v]
    assert {Hq // Hkv for Hq, Hkv, _ in geoms} == {3, 6} and all(Hq % Hkv == 0 for Hq, Hkv, _ in geoms)
