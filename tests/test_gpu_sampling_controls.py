"""-m gpu: top_k / min_p / seed end to end on the tiny models -- ``generate_step`` in both KV modes and the continuous
scheduler on a real engine.  What one request draws in DIFFERENT batch compositions is not compared: bit-equal logits across
batch sizes are not promised; slot independence of the random streams is a kernel-level property
(tests/test_gpu_sampler_filters.py)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

PROMPT = np.asarray([[5, 17, 200, 31, 9, 77, 140, 3, 12]], dtype=np.int32)


@pytest.fixture(scope="module")
def loaded(tiny_dirs):
    d, cfg = tiny_dirs["llama_bf16_gqa"]
    utils._kv_pool.clear()
    model, tok = utils.load(d)
    yield model, tok, cfg
    utils._kv_pool.clear()
    model.engine.close()


def _ids(model, n, paged=True, prompts=PROMPT, **kw):
    cache = utils._kv_pool.get(model.head_dim, [model.n_kv_heads] * len(model.layers), prompts.shape[0], paged=paged)
    steps = utils.generate_step(prompts, model, cache=cache, **kw)
    out = [t[:, 0].copy() for _, (t, _p) in zip(range(n), steps)]
    steps.close()
    return np.stack(out, axis=1)


@pytest.mark.parametrize("paged", [True, False])
def test_top_k_1_is_greedy(loaded, paged):
    model, _tok, _cfg = loaded
    prompts = np.concatenate([PROMPT, PROMPT[:, ::-1]], axis=0)
    greedy = _ids(model, 16, paged, prompts, temp=0.0)
    assert np.array_equal(_ids(model, 16, paged, prompts, temp=1.0, top_k=1, seed=3), greedy)
    assert np.array_equal(_ids(model, 16, paged, prompts, temp=1.5, top_k=1, min_p=0.3, top_p=0.9, seed=4), greedy)
    assert np.array_equal(_ids(model, 16, paged, prompts, temp=0.0, top_k=7, min_p=0.5), greedy)      # greedy ignores the controls


def test_seed_reproduces_and_seeds_differ(loaded):
    model, _tok, _cfg = loaded
    kw = dict(temp=1.5, top_k=50, min_p=0.01)
    a = _ids(model, 32, seed=11, **kw)
    assert np.array_equal(a, _ids(model, 32, seed=11, **kw))
    assert not np.array_equal(a, _ids(model, 32, seed=12, **kw))


def _scheduled(model, tok, requests):
    """All requests are queued before the scheduler starts, so every run admits and steps them alike."""
    from mlx_parallm_amd.server.scheduler import ContinuousScheduler

    sched = ContinuousScheduler(model, tok, max_slots=4, kv_dtype="model", chunk_tokens=16, block_tokens=16, prefix_cache=False)
    done, ev = {}, threading.Event()

    def sink(name):
        def f(seq, delta, reason):
            if reason is not None:
                done[name] = (list(seq.generated), reason)
                if len(done) == len(requests):
                    ev.set()
        return f

    for name, (prompt, temp, top_p, kw) in requests.items():
        sched.submit(prompt, 12, temp, top_p, sink(name), **kw)
    sched.start()
    assert ev.wait(timeout=120)
    rows = sched.max_rows_seen
    sched.stop()
    assert all(r[1] in ("stop", "length") for r in done.values()), done
    return {k: v[0] for k, v in done.items()}, rows


def test_scheduler_runs_four_different_requests_reproducibly(loaded):
    model, tok, _cfg = loaded
    requests = {
        "a": (list(range(40, 63)), 1.0, 1.0, dict(top_k=1, seed=1)),
        "b": (list(range(70, 82)), 0.8, 0.9, dict(top_k=40, seed=2)),
        "c": (list(range(100, 131)), 1.3, 1.0, dict(min_p=0.05, seed=3)),
        "d": (list(range(150, 157)), 1.5, 0.95, dict(top_k=100, min_p=0.01, seed=4)),
    }
    first, rows = _scheduled(model, tok, requests)
    assert rows == 4                                             # they did run together
    again, _ = _scheduled(model, tok, requests)
    assert again == first
    # the top_k = 1 request against its own greedy output in the same company
    greedy = dict(requests, a=(requests["a"][0], 0.0, 1.0, dict(seed=1)))
    assert _scheduled(model, tok, greedy)[0]["a"] == first["a"]
    assert len({tuple(v) for v in first.values()}) == 4


def test_invalid_values_are_refused_and_change_nothing(loaded):
    from mlx_parallm_amd.server.scheduler import Sequence

    model, _tok, _cfg = loaded
    eng = model.engine
    kv = eng.new_kv(2, capacity=64, kv_dtype="model")
    toks = np.concatenate([PROMPT, PROMPT], axis=0)
    bad = [SampleArgs(temp=1.0, top_k=-1), SampleArgs(temp=1.0, min_p=1.5), SampleArgs(temp=1.0, min_p=-0.25),
           SampleArgs(temp=1.0, min_p=float("nan"))]
    rows = SampleArgs(temp=1.0)
    rows.set_row_filters([3, -2], None)
    bad.append(rows)
    rows = SampleArgs(temp=1.0)
    rows.set_row_filters(None, [0.5, 2.0])
    bad.append(rows)
    half = SampleArgs(temp=1.0)
    half.set_row_streams([1, 2], [0, 0])
    half.c.row_position = None                                   # a seed array without its partner
    bad.append(half)
    for sp in bad:
        with pytest.raises(ValueError, match="top_k|min_p|row_seed"):
            eng.decode_sample(kv, toks, sp)
        with pytest.raises(ValueError):
            eng.step_enqueue_mixed(kv, [0, 1], [list(PROMPT[0]), list(PROMPT[0])], [1, 1], sp)
        assert kv.offsets == [0, 0]
    res = eng.decode_sample(kv, toks, SampleArgs(temp=1.0, top_k=5, min_p=0.1, seed=1))      # and the engine still works
    assert kv.offsets == [PROMPT.shape[1]] * 2 and res["tokens"].shape == (2,)
    kv.close()
    with pytest.raises(ValueError):
        Sequence([1, 2], 4, 1.0, 1.0, lambda *a: None, None, top_k=-3)
    with pytest.raises(ValueError):
        next(utils.generate_step(PROMPT, model, temp=1.0, min_p=7.0))
