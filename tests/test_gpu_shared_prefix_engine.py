"""Engine option "shared_prefix_attention" = 64 (-m gpu): tiny models at head_dim 64 (Hq/Hkv 2 and 5), 64-token blocks, float32 KV.
A prompt of 2 blocks + 5 tokens forked into rows 1..3, 12 teacher-forced steps against the oracle; unrelated rows keep their bits."""
import numpy as np
import pytest

from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

V, BLOCK, STEPS, ROWS = 512, 64, 12, 4
P = 2 * BLOCK + 5


def _kv(eng):
    return eng.new_paged_kv(ROWS, block_tokens=BLOCK, n_blocks=24, max_tokens_per_row=3 * BLOCK, kv_dtype="float32")


def _forced(seed):
    f = np.random.default_rng(seed).integers(3, V, size=(STEPS, ROWS, 1)).astype(np.int32)
    for r in range(1, ROWS):
        f[:, r] = 3 + (f[:, 0] - 3 + 100 * r) % (V - 3)      # no two rows get the same token
    return f


def _step(eng, kv, rows, tokens):
    res = eng.step_wait(eng.step_enqueue_rows(kv, rows, tokens, SampleArgs(temp=0.0, top_logprobs=20)), len(rows), 20)
    return {k: np.array(res[k]) for k in ("tokens", "logprobs", "top_ids", "top_logprobs")}


@pytest.mark.parametrize("name", ["llama_f16", "qwen3_bf16"])
def test_forked_rows_decode_through_attn_shared(tiny_dirs, name):
    d, cfg = tiny_dirs[name]
    eng = utils.load_model(d, max_positions=256).engine
    ref = ref_generate.load(d, max_pos=256)
    prompt = np.random.default_rng(3).integers(3, V, size=P).astype(np.int32)
    eng.set_option("shared_prefix_attention", 64)
    kv = _kv(eng)
    _step(eng, kv, [0], prompt[None])
    for r in range(1, ROWS):
        kv.fork_row(0, r, P)
    cache = ref.make_cache(ROWS, paged=True)
    ref(np.tile(prompt, (ROWS, 1)), cache=cache)
    eng.profile_select("attn_shared")
    worst = 0.0
    for s, t in enumerate(_forced(17)):
        # in turn: every row (mi_decode_sample), a row-subset step in another order, a subset of the set next to a one-row step
        order = [[0, 1, 2, 3], [2, 0, 3, 1], [1, 2, 3]][s % 3]
        if s % 3 == 2:
            _step(eng, kv, [0], t[:1])                         # (shares with nobody in its step: the fused launch)
        got = eng.decode_sample(kv, t, SampleArgs(temp=0.0)) if s % 3 == 0 else _step(eng, kv, order, t[order])
        want = ref_sample.sample(ref(t, cache=cache)[:, -1], temp=0.0)
        for i, r in enumerate(order):
            assert int(got["tokens"][i]) == int(want["tokens"][r, 0]), (s, r)
            worst = max(worst, abs(float(got["logprobs"][i]) - float(want["logprobs"][r])))
    n, _ = eng.profile_read()
    assert worst <= 1e-3
    assert n == cfg["num_hidden_layers"] * STEPS
    assert kv.offsets == [P + STEPS] * ROWS
    eng.close()


def test_unrelated_rows_keep_their_launches_and_their_bits(tiny_dirs):
    d, cfg = tiny_dirs["llama_f16"]
    eng = utils.load_model(d, max_positions=256).engine
    prompts = np.random.default_rng(4).integers(3, V, size=(ROWS, P)).astype(np.int32)
    runs = {}
    for opt in (64, 0):
        eng.set_option("shared_prefix_attention", opt)
        kv = _kv(eng)
        for r in range(ROWS):
            _step(eng, kv, [r], prompts[r][None])
        eng.profile_select("attn_shared")
        runs[opt] = [_step(eng, kv, [0, 1, 2, 3], t) if s % 2 == 0 else {"logits": eng.forward(t, kv)} for s, t in enumerate(_forced(19))]
        assert eng.profile_read()[0] == 0
        kv.close()
    for a, b in zip(runs[64], runs[0]):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        eng.set_option("shared_prefix_attention", -1)
    eng.close()
