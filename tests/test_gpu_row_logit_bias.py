"""-m gpu: the per-row logit_bias of a KV cache (``mi_kv_set_row_logit_bias``) through the C ABI, on a tiny float32 model
(2 layers, hidden 64, vocab 320) with a 4-slot cache in both forms.  The bias belongs to the cache row: it is set once and every
entry point that samples through the cache obeys it; rows without one, and caches without a biased row, are untouched bit for
bit.  Semantics: mi355_decode.h, DESIGN.md §2."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_generate

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

V, SLOTS, LP, STEPS = 320, 4, 9, 8
T = 123                                              # the token a +1e4 entry forces
RNG = np.random.default_rng(42)
PROMPTS = RNG.integers(3, V, size=(SLOTS, LP)).astype(np.int32)       # one prompt per slot, equal lengths: no padding
ORDER = [3, 0, 1]                                    # the rows of the subset steps, in this order
GREEDY = dict(temp=0.0)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("rowbias_gpu") / "tiny"
    build_tiny_model(d, seed=11, vocab_size=V, hidden_size=64, layers=2, heads=4, kv_heads=4, intermediate_size=128,
                     quantize_model=False, dtype="float32")
    model = utils.load_model(str(d), max_positions=256)
    ref = ref_generate.load(str(d), max_pos=256)
    yield model.engine, ref
    model.engine.close()


@pytest.fixture(params=["contiguous", "paged"])
def kv(env, request):
    eng = env[0]
    if request.param == "paged":
        c = eng.new_paged_kv(SLOTS, block_tokens=16, n_blocks=4 * SLOTS + 1, max_tokens_per_row=64, kv_dtype="float32")
    else:
        c = eng.new_kv(SLOTS, capacity=64, kv_dtype="float32")
    yield c
    c.close()


def subset_run(eng, kv, biases, device_feed, rows=ORDER, steps=STEPS):
    """Fresh rows, `biases` {row: dict} set, then `steps` greedy steps on `rows`: the prompts, then the sampled tokens
    (explicit, or the device-resident feed) -> (tokens [steps][n], logprobs [steps][n])."""
    kv.reset()
    for r, b in biases.items():
        kv.set_row_logit_bias(r, b)
    toks, lps = [], []
    res = eng.step_wait(eng.step_enqueue_rows(kv, rows, PROMPTS[rows], SampleArgs(**GREEDY)), len(rows))
    for _ in range(steps - 1):
        toks.append(res["tokens"].copy()); lps.append(res["logprobs"].copy())
        nxt = None if device_feed else res["tokens"][:, None]
        res = eng.step_wait(eng.step_enqueue_rows(kv, rows, nxt, SampleArgs(**GREEDY)), len(rows))
    toks.append(res["tokens"].copy()); lps.append(res["logprobs"].copy())
    return np.stack(toks), np.stack(lps)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. subset steps
@pytest.mark.parametrize("device_feed", [False, True])
def test_subset_steps_bias_only_the_rows_that_have_one(env, kv, device_feed):
    eng = env[0]
    base_t, base_l = subset_run(eng, kv, {}, device_feed)
    first3 = int(base_t[0, ORDER.index(3)])
    got_t, got_l = subset_run(eng, kv, {1: {T: 1e4}, 3: {first3: -1e4}}, device_feed)
    i0, i1, i3 = ORDER.index(0), ORDER.index(1), ORDER.index(3)
    assert bits(got_t[:, i0]) == bits(base_t[:, i0]) and bits(got_l[:, i0]) == bits(base_l[:, i0])     # row 0: untouched
    assert (got_t[:, i1] == T).all() and (got_l[:, i1] > -1e-3).all()
    assert (got_t[:, i3] != first3).all()
    assert not (base_t[:, i1] == T).all()


# ---- 2. one bias on every row is the call-wide list
@pytest.mark.parametrize("entry", ["step_enqueue", "decode_sample"])
def test_the_same_bias_on_every_row_equals_the_call_wide_list(env, kv, entry):
    eng = env[0]
    bias = {5: 3.0, 17: -2.5, 100: 8.0, 319: 6.25, 0: -7.0}

    def run(row_bias, call_bias):
        kv.reset()
        for r in range(SLOTS):
            kv.set_row_logit_bias(r, row_bias)
        y, toks, lps = PROMPTS, [], []
        for _ in range(STEPS):
            sp = SampleArgs(logit_bias=call_bias, **GREEDY)
            if entry == "decode_sample":
                res = eng.decode_sample(kv, y, sp)
            else:
                res = eng.step_wait(eng.step_enqueue(kv, y, sp), SLOTS)
            toks.append(res["tokens"].copy()); lps.append(res["logprobs"].copy())
            y = res["tokens"][:, None]
        return np.stack(toks), np.stack(lps)

    want_t, want_l = run(None, bias)
    got_t, got_l = run(bias, None)
    assert bits(got_t) == bits(want_t) and bits(got_l) == bits(want_l)
    plain_t, _ = run(None, None)
    assert not np.array_equal(plain_t, want_t)                         # the bias does change what this model says


# ---- 3. mixed steps
def test_a_chunked_prompt_obeys_its_rows_bias_and_the_decode_rows_are_unchanged(env, kv):
    eng = env[0]
    long_prompt = RNG.integers(3, V, size=21).astype(np.int32)

    def run(bias2):
        kv.reset()
        if bias2:
            kv.set_row_logit_bias(2, bias2)
        sp = lambda: SampleArgs(**GREEDY)                                                   # noqa: E731
        res = eng.step_wait(eng.step_enqueue_rows(kv, [0, 1], PROMPTS[[0, 1]], sp()), 2)    # two live decode rows
        out = [res]
        res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 2], [[res["tokens"][0]], [res["tokens"][1]], long_prompt[:16]],
                                                   [1, 1, 0], sp()), 2)                      # inner chunk: nothing sampled for row 2
        out.append(res)
        res = eng.step_wait(eng.step_enqueue_mixed(kv, [1, 0, 2], [[res["tokens"][1]], [res["tokens"][0]], long_prompt[16:]],
                                                   [1, 1, 1], sp()), 3)                      # last chunk: row 2's first token
        out.append(res)
        res = eng.step_wait(eng.step_enqueue_mixed(kv, [2, 1, 0], [[res["tokens"][2]], [res["tokens"][0]], [res["tokens"][1]]],
                                                   [1, 1, 1], sp()), 3)                      # all three decode
        out.append(res)
        return out

    base, got = run(None), run({T: 1e4})
    for b, g in zip(base[:2], got[:2]):
        assert bits(b["tokens"]) == bits(g["tokens"]) and bits(b["logprobs"]) == bits(g["logprobs"])
    assert bits(base[2]["tokens"][:2]) == bits(got[2]["tokens"][:2]) and bits(base[2]["logprobs"][:2]) == bits(got[2]["logprobs"][:2])
    assert int(got[2]["tokens"][2]) == T and got[2]["logprobs"][2] > -1e-3 and int(base[2]["tokens"][2]) != T
    assert int(got[3]["tokens"][0]) == T                               # ... and it keeps obeying it, as sampled row 0 of the step
    assert bits(base[3]["tokens"][1:]) == bits(got[3]["tokens"][1:]) and bits(base[3]["logprobs"][1:]) == bits(got[3]["logprobs"][1:])


# ---- 4. ordering
def test_a_bias_set_behind_an_enqueued_step_applies_from_the_next_step(env, kv):
    eng = env[0]
    base_t, base_l = subset_run(eng, kv, {}, False, rows=[2], steps=3)
    kv.reset()
    ticket = eng.step_enqueue_rows(kv, [2], PROMPTS[[2]], SampleArgs(**GREEDY))
    kv.set_row_logit_bias(2, {T: 1e4})                                 # enqueued, not waited: the step must not see it
    res = eng.step_wait(ticket, 1)
    assert bits(res["tokens"]) == bits(base_t[0]) and bits(res["logprobs"]) == bits(base_l[0]) and int(res["tokens"][0]) != T
    res = eng.step_wait(eng.step_enqueue_rows(kv, [2], res["tokens"][:, None], SampleArgs(**GREEDY)), 1)
    assert int(res["tokens"][0]) == T
    kv.set_row_logit_bias(2, None)                                     # cleared: behind that step, ahead of the next
    eng.step_wait(eng.step_enqueue_rows(kv, [2], [[int(base_t[1, 0])]], SampleArgs(**GREEDY)), 1)
    # reset_row + the same prompt: the unbiased tokens again
    kv.set_row_logit_bias(2, {T: 1e4})
    kv.reset_row(2)
    again_t, again_l = [], []
    res = eng.step_wait(eng.step_enqueue_rows(kv, [2], PROMPTS[[2]], SampleArgs(**GREEDY)), 1)
    for _ in range(2):
        again_t.append(res["tokens"].copy()); again_l.append(res["logprobs"].copy())
        res = eng.step_wait(eng.step_enqueue_rows(kv, [2], res["tokens"][:, None], SampleArgs(**GREEDY)), 1)
    again_t.append(res["tokens"].copy()); again_l.append(res["logprobs"].copy())
    assert bits(np.stack(again_t)) == bits(base_t) and bits(np.stack(again_l)) == bits(base_l)


def test_kv_reset_clears_every_row(env, kv):
    eng = env[0]
    rows = [0, 1, 2, 3]
    base_t, base_l = subset_run(eng, kv, {}, False, rows=rows, steps=3)
    forced_t, _ = subset_run(eng, kv, {r: {T + r: 1e4} for r in rows}, False, rows=rows, steps=3)
    assert (forced_t == np.asarray([T + r for r in rows])[None, :]).all()
    after_t, after_l = subset_run(eng, kv, {}, False, rows=rows, steps=3)       # (subset_run starts with kv.reset())
    assert bits(after_t) == bits(base_t) and bits(after_l) == bits(base_l)


# ---- 5. validation
def test_violations_are_refused_and_the_previous_bias_stays(env, kv):
    eng = env[0]
    kv.reset()
    kv.set_row_logit_bias(1, {T: 1e4})
    for row, bias, what in ((SLOTS, {5: 1.0}, "row out of range"), (-1, {5: 1.0}, "row out of range"), (1, {-1: 1.0}, r"ids\[0\]"),
                            (1, {4: 1.0, V: 1.0}, r"ids\[1\]"), (1, {5: float("nan")}, r"values\[0\]"),
                            (1, {5: float("inf")}, r"values\[0\]"), (1, {4: 1.0, 5: 1e39}, r"values\[1\]")):
        with pytest.raises(ValueError, match=what):
            kv.set_row_logit_bias(row, bias)
    raw = L.lib().mi_kv_set_row_logit_bias
    I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ids = np.arange(L.MI_MAX_ROW_LOGIT_BIAS + 1, dtype=np.int32) % V
    vals = np.full(L.MI_MAX_ROW_LOGIT_BIAS + 1, 0.5, np.float32)
    pi, pv = ids.ctypes.data_as(I32), vals.ctypes.data_as(F32)
    dup = np.asarray([7, 9, 7], dtype=np.int32)
    for args, what in (((pi, pv, L.MI_MAX_ROW_LOGIT_BIAS + 1), "n must be"), ((pi, pv, -1), "n must be"),
                       ((dup.ctypes.data_as(I32), pv, 3), "token 7 twice"), ((None, None, 2), "null ids")):
        with pytest.raises(ValueError, match=what):       # (what a Python dict cannot say goes through the C entry point)
            L.check(raw(kv._h, 1, *args))
    # the earlier bias is still in force
    res = eng.step_wait(eng.step_enqueue_rows(kv, [1, 0], PROMPTS[[1, 0]], SampleArgs(**GREEDY)), 2)
    assert int(res["tokens"][0]) == T and res["logprobs"][0] > -1e-3
    # the largest list is taken, and replaces the row's bias
    full = {int(i): 0.0 for i in range(V)}
    full[T + 1] = 1e4
    kv.set_row_logit_bias(1, full)
    res = eng.step_wait(eng.step_enqueue_rows(kv, [1, 0], res["tokens"][:, None], SampleArgs(**GREEDY)), 2)
    assert int(res["tokens"][0]) == T + 1


# ---- 6. parity with the oracle, one row at a time with that row's dict
def test_two_rows_with_different_dicts_match_the_oracle(env, kv):
    eng, ref = env
    dicts = {0: {5: 4.0, 17: -3.0, 200: 6.5, 64: 2.25}, 2: {9: 5.5, 250: -8.0, 33: 3.75}}
    rows = [2, 0]
    got_t, got_l = subset_run(eng, kv, dicts, False, rows=rows, steps=STEPS)
    plain_t, _ = subset_run(eng, kv, {}, False, rows=rows, steps=STEPS)
    worst = 0.0
    for i, r in enumerate(rows):
        gen = ref_generate.generate_step(PROMPTS[r][None], ref, temp=0.0, logit_bias=dicts[r], paged=True, return_logits=True)
        for s, (y, _p, _lg, lp) in zip(range(STEPS), gen):
            assert int(got_t[s, i]) == int(y[0, 0]), (r, s)
            worst = max(worst, abs(float(got_l[s, i]) - float(lp[0])))
        gen.close()
    print(f"max |logprob - oracle| = {worst:.3e}")
    assert worst <= 1e-3
    assert not np.array_equal(got_t, plain_t)                          # the dicts matter on this model
