"""-m gpu: the consumer_combine prologue of the float32-KV decode attention fetches exactly the class of K slices that the
q|k|v launch published (2, 3..4, 5..8 -> attn_decode_mfma_qs_kernel<.., 2 / 4 / 8>), in the lane groups that own a vector.

Two-layer bf16 models from build_tiny_model (layer 0 is the rounded call and keeps the ordinary launch, layer 1 takes the
offer), hidden sizes 512 .. 2048 -- the q|k|v planner cuts K = hidden into 2, 3, 4, 6 and 8 slices there --, query groups of
2, 3, 4, 5 and 8 heads, head_dim 64 and 128, batch 1, 3 and 8, contiguous and block-paged float32 caches.  KV length
252 -> 258: across the 16-key tile at 256.  Tokens and logprobs of every step must be EXACTLY equal with consumer_combine 0
and 1 (the additions, their order and the row scale are those of the linear's last arriver).

The slice counts are asked from the planner itself (mi_op_gemm_skinny's ksplit_used, the value the engine's offer uses) for
each model's q|k|v shape and batch; the test asserts that they reach 2, 4, a count that is no power of two and one in 5..8.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from gpu_helpers import dev, gemm_skinny, op_linear, to_tiled  # noqa: E402

# hidden size -> (query heads, kv heads, head_dim)
MODELS = {512: (4, 2, 64), 768: (6, 2, 128), 1024: (8, 2, 128), 1536: (5, 1, 64), 2048: (16, 2, 64)}
BATCHES = (1, 3, 8)
L0, STEPS, MAX_POS = 252, 6, 320
VOCAB = 256


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    root, cache = tmp_path_factory.mktemp("owners"), {}

    def get(hidden):
        if hidden not in cache:
            for m in cache.values():                       # one engine at a time
                m.engine.close()
            cache.clear()
            heads, kv_heads, head_dim = MODELS[hidden]
            build_tiny_model(str(root / str(hidden)), seed=20 + hidden, vocab_size=VOCAB, dtype="bfloat16", quantize_model=False,
                             hidden_size=hidden, layers=2, heads=heads, kv_heads=kv_heads, intermediate_size=hidden,
                             head_dim=head_dim, tie_word_embeddings=False, with_tokenizer=False, norm_jitter=0.1)
            cache[hidden] = utils.load_model(str(root / str(hidden)), max_positions=MAX_POS)
        return cache[hidden]

    yield get
    for m in cache.values():
        m.engine.close()


def _run(engine, cc, B, paged):
    engine.set_option("consumer_combine", cc)
    if paged:
        kv = engine.new_paged_kv(B, block_tokens=64, max_tokens_per_row=MAX_POS, kv_dtype="float32")
    else:
        kv = engine.new_kv(B, capacity=MAX_POS, kv_dtype="float32")
    y = np.random.default_rng(300 + B).integers(3, VOCAB, size=(B, L0)).astype(np.int32)
    out = []
    for _ in range(1 + STEPS):                             # the prefill call, then STEPS decode steps
        out.append(engine.decode_sample(kv, y, SampleArgs(temp=0.0)))
        y = out[-1]["tokens"][:, None].astype(np.int32)
    kv.close()
    return out[1:]


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hidden", sorted(MODELS))
def test_tokens_and_logprobs_are_equal_with_and_without_the_prologue_sum(models, hidden, B, paged):
    engine = models(hidden).engine
    try:
        base, got = _run(engine, 0, B, paged), _run(engine, 1, B, paged)
    finally:
        engine.set_option("consumer_combine", 0)
    assert len(base) == len(got) == STEPS
    for s, (a, b) in enumerate(zip(base, got)):
        for k in ("tokens", "logprobs"):
            assert np.array_equal(a[k], b[k]), (hidden, B, paged, "step", s, k, a[k], b[k])


def _planned_slices(hidden, B):
    heads, kv_heads, head_dim = MODELS[hidden]
    N = (heads + 2 * kv_heads) * head_dim
    rng = np.random.default_rng(hidden + B)
    wd = dev(rng.standard_normal((N, hidden)) * 0.05, "bfloat16")
    ol, keep = op_linear("bf16", N, hidden, wd), [wd]
    assert to_tiled(ol, keep)
    out = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    used, _ = gemm_skinny(ol, dev(rng.standard_normal((B, hidden))), B, "float32", epi=L.EPI_STORE, out=out, ldo=N)
    return used


def test_the_models_reach_every_class_of_slice_counts():
    counts = {(h, B): _planned_slices(h, B) for h in sorted(MODELS) for B in BATCHES}
    print("q|k|v K slices per (hidden, batch):", counts)
    reached = set(counts.values())
    missing = [what for what, ok in (("2", 2 in reached), ("4", 4 in reached),
                                     ("a count that is no power of two", any(2 <= c <= 8 and c & (c - 1) for c in reached)),
                                     ("a count in 5..8", any(5 <= c <= 8 for c in reached))) if not ok]
    if missing:
        pytest.skip(f"the q|k|v planner gives no slice count of: {', '.join(missing)} at these widths ({sorted(reached)})")
    assert all(2 <= c <= 8 for c in reached), counts          # every model's layer 1 can take the offer
