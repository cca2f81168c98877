"""-m gpu: the per-row logprobs settings of a KV cache (``mi_kv_set_row_logprobs``) through the engine binding, on the tiny
float32 models (dense and int4) with a 4-slot cache in both forms and both KV dtypes.  The setting belongs to the cache row:
rows 1 and 3 get (3, at temperature) and (20, plain), the steps they share with rows that have none return every row's
tokens unchanged, and their lists are the ones a twin cache without settings returns under the call-wide count.
Semantics: mi355_decode.h, DESIGN.md §2."""
import numpy as np
import pytest

from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

V, SLOTS, LP, STEPS, STRIDE = 512, 4, 9, 5, 20
RNG = np.random.default_rng(7)
PROMPTS = RNG.integers(3, V, size=(SLOTS, LP)).astype(np.int32)
LONG = RNG.integers(3, V, size=21).astype(np.int32)          # row 3's prompt in the mixed steps, in chunks of 16 + 5
TEMP = {0: 0.0, 1: 0.7, 2: 1.0, 3: 0.0}                       # per cache row; row 1 reports under softmax(logits / 0.7)
UNIF = RNG.random((STEPS + 2, SLOTS)).astype(np.float32)      # [step][cache row]
SETTINGS = {1: (3, True), 3: (20, False)}
ORDER = [3, 0, 1]


@pytest.fixture(scope="module", params=["llama_f32", "llama_q4_f32"])
def env(tiny_dirs, request):
    d, _cfg = tiny_dirs[request.param]
    model = utils.load_model(str(d), max_positions=256)
    ref = ref_generate.load(str(d), max_pos=256)
    yield model.engine, ref
    model.engine.close()


@pytest.fixture(params=["contiguous-model", "contiguous-float32", "paged-model", "paged-float32"])
def kv(env, request):
    form, dt = request.param.split("-")
    eng = env[0]
    if form == "paged":
        c = eng.new_paged_kv(SLOTS, block_tokens=16, n_blocks=4 * SLOTS + 1, max_tokens_per_row=64, kv_dtype=dt)
    else:
        c = eng.new_kv(SLOTS, capacity=64, kv_dtype=dt)
    yield c
    c.close()


def args(rows, step, k_call=0, at_call=False):
    sp = SampleArgs(top_logprobs=k_call, logprobs_at_temperature=at_call, uniforms=[UNIF[step, r] for r in rows])
    sp.set_row_params([TEMP[r] for r in rows], [1.0] * len(rows))
    return sp


def run_rows(eng, kv, settings, k_call=0, at_call=False):
    """Fresh rows, the settings, then STEPS steps on ORDER: the prompts, then the device-resident token feed."""
    kv.reset()
    for r, (k, f) in settings.items():
        kv.set_row_logprobs(r, k, f)
    out = [eng.step_wait(eng.step_enqueue_rows(kv, ORDER, PROMPTS[ORDER], args(ORDER, 0, k_call, at_call)), len(ORDER), k_call)]
    for s in range(1, STEPS):
        out.append(eng.step_wait(eng.step_enqueue_rows(kv, ORDER, None, args(ORDER, s, k_call, at_call)), len(ORDER), k_call))
    return out, [ORDER] * STEPS


def run_mixed(eng, kv, settings, k_call=0, at_call=False):
    """Rows 0 and 1 decode while row 3's prompt arrives in two chunks; then all three decode.  -> (results, sampled rows)."""
    kv.reset()
    for r, (k, f) in settings.items():
        kv.set_row_logprobs(r, k, f)
    a = lambda rows, s: args(rows, s, k_call, at_call)                                         # noqa: E731
    res = eng.step_wait(eng.step_enqueue_rows(kv, [0, 1], PROMPTS[[0, 1]], a([0, 1], 0)), 2, k_call)
    out, who = [res], [[0, 1]]
    res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 3], [[res["tokens"][0]], [res["tokens"][1]], LONG[:16]], [1, 1, 0],
                                               a([0, 1], 1)), 2, k_call)
    out.append(res); who.append([0, 1])
    res = eng.step_wait(eng.step_enqueue_mixed(kv, [1, 0, 3], [[res["tokens"][1]], [res["tokens"][0]], LONG[16:]], [1, 1, 1],
                                               a([1, 0, 3], 2)), 3, k_call)
    out.append(res); who.append([1, 0, 3])
    res = eng.step_wait(eng.step_enqueue_mixed(kv, [3, 1, 0], [[res["tokens"][2]], [res["tokens"][0]], [res["tokens"][1]]],
                                               [1, 1, 1], a([3, 1, 0], 3)), 3, k_call)
    out.append(res); who.append([3, 1, 0])
    return out, who


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def oracle_logprobs(ref, prompt, generated, temp):
    """Teacher-forced log-softmax (of logits / temp when temp is given) of every generated token."""
    seq = np.concatenate([prompt, generated[:-1]]).astype(np.int32)[None]
    lg = np.asarray(ref(seq, cache=ref.make_cache(1, paged=True)), np.float32)[0, len(prompt) - 1:]
    if temp:
        lg = lg * np.float32(1.0 / temp)
    lsm = ref_sample.log_softmax(lg)
    return lsm[np.arange(len(generated)), generated], lsm


@pytest.mark.parametrize("run", [run_rows, run_mixed], ids=["rows_device_feed", "mixed_chunked_prompt"])
def test_rows_with_settings_share_steps_with_rows_without(env, kv, run):
    eng, ref = env
    base, who = run(eng, kv, {})                              # the twin: no settings, no lists
    twin3, _ = run(eng, kv, {}, 3, True)                      # ... the call-wide count of row 1, under its flag
    twin20, _ = run(eng, kv, {}, 20, False)                   # ... and of row 3
    got, _ = run(eng, kv, SETTINGS)
    gen = {r: [] for r in range(SLOTS)}
    lps = {r: [] for r in range(SLOTS)}
    for s, rows in enumerate(who):
        assert "top_counts" in got[s] and "top_counts" not in base[s] and "top_ids" not in base[s]
        assert got[s]["top_ids"].shape == (len(rows), STRIDE)
        assert list(got[s]["top_counts"]) == [SETTINGS.get(r, (0,))[0] for r in rows]
        for key in ("tokens", "probs_row0"):
            assert bits(got[s][key]) == bits(base[s][key]), (s, key)
        for i, r in enumerate(rows):
            gen[r].append(int(got[s]["tokens"][i])); lps[r].append(float(got[s]["logprobs"][i]))
            k, twin = {1: (3, twin3), 3: (20, twin20)}.get(r, (0, base))
            assert bits(got[s]["logprobs"][i]) == bits(twin[s]["logprobs"][i]), (s, r)
            if k:
                assert np.array_equal(got[s]["top_ids"][i, :k], twin[s]["top_ids"][i]), (s, r)
                assert bits(got[s]["top_logprobs"][i, :k]) == bits(twin[s]["top_logprobs"][i]), (s, r)
            assert np.all(got[s]["top_ids"][i, k:] == -1) and np.all(np.isneginf(got[s]["top_logprobs"][i, k:])), (s, r)
    worst = 0.0
    for r in (1, 3):                                          # the project's tiny-model contract against the oracle
        prompt = LONG if (run is run_mixed and r == 3) else PROMPTS[r]
        want, lsm = oracle_logprobs(ref, prompt, np.asarray(gen[r]), TEMP[r] if SETTINGS[r][1] else None)
        worst = max(worst, float(np.max(np.abs(np.asarray(lps[r]) - want))))
    print(f"max |logprob - oracle| = {worst:.3e}")
    assert worst <= 1e-3


def test_step_enqueue_and_decode_sample_obey_the_settings(env, kv):
    eng = env[0]

    def run(settings, k_call, entry):
        kv.reset()
        for r, (k, f) in settings.items():
            kv.set_row_logprobs(r, k, f)
        rows = list(range(SLOTS))
        sp = args(rows, 0, k_call, False)
        if entry == "decode_sample":
            return eng.decode_sample(kv, PROMPTS, sp)
        return eng.step_wait(eng.step_enqueue(kv, PROMPTS, sp), SLOTS, k_call)

    for entry in ("step_enqueue", "decode_sample"):
        want = run({}, 20, entry)
        got = run({3: (20, False)}, 2, entry)                 # the others keep the call's 2
        assert bits(got["tokens"]) == bits(want["tokens"])
        assert list(got["top_counts"]) == [2, 2, 2, 20]
        assert bits(got["top_ids"][3]) == bits(want["top_ids"][3]) and bits(got["top_logprobs"][3]) == bits(want["top_logprobs"][3])
        for r in range(3):
            assert bits(got["top_ids"][r, :2]) == bits(want["top_ids"][r, :2]) and np.all(got["top_ids"][r, 2:] == -1)


def test_reset_clears_and_reserve_and_prefix_calls_keep_the_setting(env, kv):
    eng = env[0]

    def step(rows=(1,)):
        rows = list(rows)
        return eng.step_wait(eng.step_enqueue_rows(kv, rows, PROMPTS[rows], args(rows, 0)), len(rows))

    kv.reset()
    kv.set_row_logprobs(1, 4, False)
    assert list(step()["top_counts"]) == [4]
    kv.reset_row(1)
    assert "top_counts" not in step()                         # cleared with the row: the layout of a cache without settings
    kv.set_row_logprobs(1, 4, False)
    kv.set_row_logprobs(2, 0, True)
    kv.reset()
    assert "top_counts" not in step() and "top_counts" not in step([2])
    kv.reset()
    kv.set_row_logprobs(1, 4, False)
    kv.set_row_logprobs(1, 0, False)                          # (0, False) clears too
    assert "top_counts" not in step()
    kv.reset()
    kv.set_row_logprobs(1, 4, False)
    if hasattr(kv, "prefix_attach"):
        assert kv.prefix_attach(1, PROMPTS[1]) == 0
        res = step()
        kv.prefix_publish(1, PROMPTS[1])
    else:
        kv.ensure(kv.capacity + 64)                           # mi_kv_reserve grows the cache
        res = step()
    assert list(res["top_counts"]) == [4] and np.all(res["top_ids"][0, :4] >= 0) and np.all(res["top_ids"][0, 4:] == -1)
    res = eng.step_wait(eng.step_enqueue_rows(kv, [1], res["tokens"][:, None], args([1], 1)), 1)
    assert list(res["top_counts"]) == [4] and np.all(res["top_ids"][0, :4] >= 0)


def test_violations_are_refused_and_the_previous_setting_stays(env, kv):
    eng = env[0]
    kv.reset()
    kv.set_row_logprobs(1, 4, False)
    for row, k, what in ((SLOTS, 3, "row out of range"), (-1, 3, "row out of range"), (1, 21, "top_logprobs must be"),
                         (1, -1, "top_logprobs must be")):
        with pytest.raises(ValueError, match=what):
            kv.set_row_logprobs(row, k, False)
    from mlx_parallm_amd import _lib as L
    with pytest.raises(ValueError, match="at_temperature must be"):
        L.check(L.lib().mi_kv_set_row_logprobs(kv._h, 1, 3, 2))
    res = eng.step_wait(eng.step_enqueue_rows(kv, [1, 0], PROMPTS[[1, 0]], args([1, 0], 0)), 2)
    assert list(res["top_counts"]) == [4, 0]
    assert np.all(res["top_ids"][0, :4] >= 0) and np.all(res["top_ids"][0, 4:] == -1) and np.all(res["top_ids"][1] == -1)
