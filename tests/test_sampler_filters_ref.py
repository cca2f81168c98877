"""The CPU definition of top-k / min-p (tests/sampler_filters_ref.py) against the oracle it is built from (no GPU)."""
import numpy as np
import pytest

import sampler_filters_ref as sfr
from oracle import ref_sample
from oracle.numerics import round_to

RNG = np.random.default_rng(20)


def _rows(V, bf=False, B=6):
    lg = (RNG.standard_normal((B, V)) * (1.3 if bf else 3.0)).astype(np.float32)
    return round_to(lg, "bfloat16") if bf else lg


@pytest.mark.parametrize("V,bf", [(37, False), (5000, False), (32000, True)])
@pytest.mark.parametrize("temp,top_p", [(1.0, 1.0), (0.7, 0.9), (1.3, 0.3)])
def test_all_controls_off_is_the_oracle_sampler(V, bf, temp, top_p):
    lg = _rows(V, bf)
    u = RNG.random(len(lg))
    want = ref_sample.sample(lg, temp=temp, top_p=top_p, uniforms=u)["tokens"][:, 0]
    assert np.array_equal(sfr.sample(lg, temp, u, top_p=top_p), want)
    assert np.array_equal(sfr.sample(lg, temp, u, top_p=top_p, top_k=V, min_p=0.0), want)     # top_k >= V is off too


@pytest.mark.parametrize("V,bf", [(37, False), (32000, True)])
def test_top_k_1_is_greedy(V, bf):
    lg = _rows(V, bf)
    lg[0, 7] = lg[0, 3] = lg[0].max() + 1.0             # a tie at the top: the lowest id
    u = RNG.random(len(lg))
    greedy = ref_sample.sample(lg, temp=0.0)["tokens"][:, 0]
    assert greedy[0] == 3
    for temp, top_p, min_p in ((1.0, 1.0, 0.0), (1.5, 0.9, 0.0), (0.7, 1.0, 0.3)):
        assert np.array_equal(sfr.sample(lg, temp, u, top_p=top_p, top_k=1, min_p=min_p), greedy)
    assert np.array_equal(sfr.sample(lg, 1.0, u, min_p=1.0)[1:], greedy[1:])                 # min_p = 1: the arg-max ties only


@pytest.mark.parametrize("V,bf", [(37, False), (5000, False), (32000, True)])
def test_kept_set_is_a_nonempty_prefix_of_the_order(V, bf):
    lg = _rows(V, bf, B=3)
    for row in lg:
        order = sfr.oracle_order(row)
        for temp, top_p, top_k, min_p in ((1.0, 1.0, 7, 0.0), (0.7, 0.9, 50, 0.0), (1.0, 0.3, 5, 0.0), (1.0, 1.0, 0, 0.05),
                                          (1.3, 1.0, 0, 0.01), (0.7, 0.9, 64, 0.2), (1.0, 0.001, 1000, 0.5), (1.0, 1.0, 0, 1.0)):
            ids, pr = sfr.kept_candidates(row, temp, top_p, top_k, min_p)
            n = len(ids)
            assert n >= 1 and np.array_equal(ids, order[:n])
            assert abs(pr.sum() - 1.0) < 1e-12 and np.all(np.diff(pr) <= 0)
            if 0 < top_k < V:
                assert n <= top_k


def test_top_k_cut_inside_a_tie_group_keeps_the_lowest_ids():
    row = np.zeros(16, np.float32)
    row[[9, 2, 12]] = 1.0
    ids, pr = sfr.kept_candidates(row, 1.0, top_k=2)
    assert ids.tolist() == [2, 9] and np.allclose(pr, 0.5)
    ids, _ = sfr.kept_candidates(row, 1.0, top_k=5)
    assert ids.tolist() == [2, 9, 12, 0, 1]
