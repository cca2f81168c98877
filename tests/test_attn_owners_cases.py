"""The owner map of the decode attention's prologue (tests/attn_owner_cases.py), checked without a device, and held against
the lines of attn_decode.hip and the group table of attn_dispatch.h it restates."""
import os
import re

import pytest

import attn_owner_cases as own

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlx_parallm_amd", "csrc")
SRC = os.path.join(CSRC, "attn_decode.hip")


@pytest.mark.parametrize("owner_split", [True, False])
@pytest.mark.parametrize("G,D", [(G, D) for D in own.DS for G in own.GS if own.served(D, G)])
def test_every_vector_has_exactly_one_owner(G, D, owner_split):
    names = own.vectors(G, owner_split)
    assert len(names) == (G + 2 if owner_split else G)
    owners = {}
    for w in range(own.NWV):
        for g in range(own.GROUPS):
            v = own.vector_of(w, g, G, owner_split)
            if v is not None:
                owners.setdefault(v, []).append((w, g))
    assert sorted(owners) == list(range(len(names)))                       # every vector is owned ...
    assert all(o == [own.owner_of(v)] for v, o in owners.items())           # ... by exactly one lane group, the packed one
    # the rotated vectors are the query heads and the new key
    assert [n for v, n in enumerate(names) if own.rotates(v, G)] == [n for n in names if n != "v_new"]


@pytest.mark.parametrize("owner_split", [True, False])
@pytest.mark.parametrize("G", own.GS)
def test_idle_waves_are_what_the_branch_assumes(G, owner_split):
    """The kernel's wave-uniform test is wave * 4 < nvec with nvec = G + 2 in the owning split and G elsewhere."""
    nvec = G + 2 if owner_split else G
    assert own.idle_waves(G, owner_split) == [w for w in range(own.NWV) if not w * 4 < nvec]
    assert 0 not in own.idle_waves(G, owner_split)                          # wave 0 (thread 0 writes the debug stamps) owns q0
    assert own.NWV - 1 in own.idle_waves(G, owner_split)                    # the wave that scores the new key / writes slot 8


def test_the_issue_s_examples():
    assert own.idle_waves(2, True) == [1, 2, 3, 4, 5, 6, 7]                 # G = 2: four vectors fill wave 0
    assert own.idle_waves(4, True) == [2, 3, 4, 5, 6, 7]
    assert own.idle_waves(6, True) == [2, 3, 4, 5, 6, 7] and own.idle_waves(8, True) == [3, 4, 5, 6, 7]
    assert own.idle_waves(4, False) == [1, 2, 3, 4, 5, 6, 7] and own.idle_waves(8, False) == [2, 3, 4, 5, 6, 7]
    # the G + 2 vectors end inside wave 0, at its end, inside wave 1, at its end, in wave 2
    assert [own.owner_of(G + 1) for G in own.GS] == [(0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 1)]


def test_the_source_says_the_same():
    src = open(SRC).read()
    body = src[src.index("void attn_decode_mfma_body("):src.index("void attn_decode_mfma_kernel(")]
    assert "constexpr int NWV = 8;" in src
    for line in ("const int vi = wave * 4 + gq;",
                 "const int nvec = owner ? G + 2 : G;",
                 "const bool is_q = vi < G, is_k = owner && vi == G, is_v = owner && vi == G + 1;",
                 "const bool has_vec = vi < nvec, rot = is_q || is_k;",
                 "const bool wave_owns = __builtin_amdgcn_readfirstlane(wave) * 4 < nvec;",
                 "const bool owner = split == c.nsplit - 1;"):
        assert line in body, line
    # every prologue load and every instruction behind it stands under the two tests
    assert body.count("if (wave_owns) if (has_vec)") == 3
    table = open(os.path.join(CSRC, "attn_dispatch.h")).read()
    rest = re.search(r"template <int D>\s*struct AttnGroups : std::integer_sequence<int, ([\d, ]+)>", table).group(1)
    d96 = re.search(r"struct AttnGroups<96> : std::integer_sequence<int, ([\d, ]+)>", table).group(1)
    rest, d96 = [int(x) for x in rest.split(",")], [int(x) for x in d96.split(",")]
    assert rest == own.GS and d96 == [g for g in own.GS if own.served(96, g)]
    assert table.count("struct AttnGroups") == 2                             # 96 is the only width with a table of its own
    # the slice classes of the consumer_combine prologue
    for ks, cls in ((2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        assert own.slice_class(ks) == cls
    assert re.search(r"if \(c\.qkv_ksplit <= 2\) return launch_mfma_qs<D, G, NORM, PAGED, 2>", src)
    assert re.search(r"if \(c\.qkv_ksplit <= 4\) return launch_mfma_qs<D, G, NORM, PAGED, 4>", src)
    assert re.search(r"return launch_mfma_qs<D, G, NORM, PAGED, 8>", src)
