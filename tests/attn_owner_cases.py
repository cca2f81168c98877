"""Who owns which prologue vector in the matrix-core decode attention (attn_decode.hip: attn_decode_mfma_body), restated in
Python for tests/test_attn_owners_cases.py (no device) and tests/test_gpu_attn_owners.py.

A workgroup has NWV = 8 waves of 4 lane groups (16 lanes each).  Its prologue vectors are the G query heads of the kv head
(vector g < G), the new key (G) and the new value (G + 1); the last two exist only in the split that owns the new position
(the last split).  Vector v belongs to lane group v % 4 of wave v // 4 -- packed from wave 0 up.
"""
NWV, GROUPS = 8, 4
GS = [1, 2, 3, 4, 5, 6, 8]                  # query heads per kv head served by the decode kernels
DS = [32, 64, 96, 128]                      # head_dim of the matrix-core kernel (float32 caches: 64, 96, 128)


def served(D, G):
    """AttnGroups (attn_dispatch.h): head_dim 96 has the groups 1, 2 and 4 only."""
    return G in ((1, 2, 4) if D == 96 else GS)


def vectors(G, owner_split):
    """Names of the prologue vectors of a split, in vector order."""
    return [f"q{g}" for g in range(G)] + (["k_new", "v_new"] if owner_split else [])


def owner_of(v):
    """-> (wave, lane group) that loads, norms / rotates and stores vector v."""
    return v // GROUPS, v % GROUPS


def vector_of(wave, group, G, owner_split):
    """The vector of a lane group, or None: what the kernel computes as vi = 4 wave + gq, has_vec = vi < nvec."""
    vi = GROUPS * wave + group
    return vi if vi < len(vectors(G, owner_split)) else None


def rotates(v, G):
    """Query heads and the new key are normed and rotated (and load cos / sin); the new value is stored as it is."""
    return v <= G


def idle_waves(G, owner_split):
    """Waves in which no lane group owns a vector: they go from row and length straight to the first K / V loads."""
    return [w for w in range(NWV) if all(vector_of(w, g, G, owner_split) is None for g in range(GROUPS))]


def slice_class(ksplit):
    """K slices of the q|k|v launch -> slices the consumer_combine prologue fetches (launch_mfma_qs_n)."""
    assert 2 <= ksplit <= 8
    return 2 if ksplit <= 2 else 4 if ksplit <= 4 else 8
