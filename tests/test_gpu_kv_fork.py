"""mi_kv_fork_row through the engine (-m gpu): a row takes the first tokens of another row.  Tiny models at head_dim 64 and 96,
a paged cache with 16-token blocks and a contiguous one, KV in float32 and in the model's dtype.

"The next step's logits" are full logits: Engine.forward steps every row of the cache and returns them, so the probes feed a
token to all rows and compare the row in question (these rows are shorter than 64 tokens: one KV split whatever the other
rows hold, and every kernel computes a row from that row alone).  A row-subset step next to it adds what the sampler reports:
the greedy token, its logprob and the 20 top entries."""
import numpy as np
import pytest

from oracle import ref_generate

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402

V = 512
MODELS = {
    "d64_bf16": dict(seed=41, vocab_size=V, dtype="bfloat16", quantize_model=False, hidden_size=128, layers=2, heads=4, kv_heads=2,
                     intermediate_size=256, head_dim=64, tie_word_embeddings=False, norm_jitter=0.1),
    "d96_bf16": dict(seed=42, vocab_size=V, dtype="bfloat16", quantize_model=False, hidden_size=384, layers=2, heads=4, kv_heads=2,
                     intermediate_size=768, head_dim=96, tie_word_embeddings=False, norm_jitter=0.1),
    "d64_f32": dict(seed=43, vocab_size=V, dtype="float32", quantize_model=False, hidden_size=128, layers=2, heads=2, kv_heads=1,
                    intermediate_size=256, head_dim=64, tie_word_embeddings=False, norm_jitter=0.1),
}
KINDS = [("paged", "model"), ("paged", "float32"), ("contiguous", "model"), ("contiguous", "float32")]
NBLOCKS = 16


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("kv_fork")
    out = {}
    for name, kw in MODELS.items():
        build_tiny_model(root / name, **kw)
        out[name] = str(root / name)
    return out


@pytest.fixture(scope="module")
def engines(dirs):
    models = {name: utils.load_model(d, max_positions=256) for name, d in dirs.items()}
    yield {name: m.engine for name, m in models.items()}
    for m in models.values():
        m.engine.close()


def _kv(eng, kind, kvd, rows=2, n_blocks=NBLOCKS):
    if kind == "paged":
        return eng.new_paged_kv(rows, block_tokens=16, n_blocks=n_blocks, max_tokens_per_row=96, kv_dtype=kvd)
    return eng.new_kv(rows, capacity=96, kv_dtype=kvd)


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(3, V, size=n).astype(np.int32)


GREEDY20 = dict(temp=0.0, top_logprobs=20)


def _step(eng, kv, rows, tokens):
    """One step on `rows`: what the sampler saw of every row's logits."""
    res = eng.step_wait(eng.step_enqueue_rows(kv, rows, tokens, SampleArgs(**GREEDY20)), len(rows), 20)
    return {k: np.array(res[k]) for k in ("tokens", "logprobs", "top_ids", "top_logprobs")}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def _six_steps(eng, kv, seed):
    """Six decode steps on rows [0, 1], forced tokens that differ per row: row-subset steps (logprobs) and forward calls
    (full logits) in turn."""
    forced = np.random.default_rng(seed).integers(3, V, size=(6, 2, 1)).astype(np.int32)
    forced[:, 1] = 3 + (forced[:, 0] - 3 + 100) % (V - 3)      # row 1 never gets row 0's token
    assert (forced[:, 0] != forced[:, 1]).all() and forced.min() >= 3 and forced.max() < V
    out = []
    for i, t in enumerate(forced):
        out.append(_step(eng, kv, [0, 1], t) if i % 2 == 0 else {"logits": eng.forward(t, kv)})
    return out


@pytest.mark.parametrize("P", [15, 16, 17, 33])
@pytest.mark.parametrize("kind,kvd", KINDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_a_fork_at_full_length_is_invisible(engines, name, kind, kvd, P):
    eng = engines[name]
    prompt = _prompt(P, 100 + P)
    runs = []
    for fork in (False, True):
        kv = _kv(eng, kind, kvd)
        first = _step(eng, kv, [0], prompt[None])
        if fork:
            kv.fork_row(0, 1, P)
            assert kv.offsets == [P, P]
        else:
            _same(first, _step(eng, kv, [1], prompt[None]), "two identical one-row prefills")
        runs.append(_six_steps(eng, kv, 7 * P))
        assert kv.offsets == [P + 6, P + 6]
        kv.close()
    for i, (c, t) in enumerate(zip(*runs)):
        _same(c, t, (name, kind, kvd, P, "step", i))


@pytest.mark.parametrize("kind,kvd", KINDS)
@pytest.mark.parametrize("name", ["d64_bf16", "d96_bf16"])
@pytest.mark.parametrize("who", ["src appends", "dst appends"])
def test_the_two_rows_are_isolated(engines, name, kind, kvd, who):
    """After the fork one row takes 20 more tokens (through the rest of its tail block and two more blocks); the other row's
    next steps -- one on its own, one with every row through Engine.forward: full logits -- give what they give on an identical
    run without those appends."""
    eng = engines[name]
    prompt, more, probe = _prompt(21, 5), _prompt(20, 6), np.array([[77]], dtype=np.int32)
    busy, quiet = (0, 1) if who == "src appends" else (1, 0)
    seen = []
    for appends in (False, True):
        kv = _kv(eng, kind, kvd)
        _step(eng, kv, [0], prompt[None])
        kv.fork_row(0, 1, 21)
        if appends:
            _step(eng, kv, [busy], more[None, :5])   # a chunk, three single tokens, a longer chunk
            for i in (5, 6, 7):
                _step(eng, kv, [busy], more[None, i:i + 1])
            _step(eng, kv, [busy], more[None, 8:])
            assert kv.offsets[busy] == 41 and kv.offsets[quiet] == 21
        seen.append(dict(_step(eng, kv, [quiet], probe), logits=eng.forward(np.array([[78], [78]], dtype=np.int32), kv)[quiet]))
        assert seen[-1]["logits"].shape == (V,) and np.isfinite(seen[-1]["logits"]).all()
        kv.close()
    _same(seen[0], seen[1], (name, kind, kvd, who))


@pytest.mark.parametrize("kind,kvd", KINDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_a_prefix_fork_from_a_row_that_is_decoding(dirs, engines, name, kind, kvd):
    """n_tokens = P - 1 from a row that has decoded 5 tokens; dst runs the last prompt token and 8 greedy steps.  Bounds of
    test_gpu_engine.py::test_prefix_reuse_on_the_paged_cache against the oracle's solo run: the ids are the oracle's, except
    that a 16-bit model may leave them at a step where the oracle's own top-2 margin is <= 0.13 (nothing is compared behind
    it).  The logprobs of the steps compared hold the bars of test_gpu_engine.py: 1e-3 on a float32 model, 0.1 on a 16-bit
    model with 16-bit KV; a 16-bit model with float32 KV is held to 8e-3 -- a logprob is a logit minus the log-sum-exp of the
    logits, and that mode's logits are held to 4e-3 each (test_float32_kv_prefill_through_the_tile_gemm)."""
    eng = engines[name]
    exact = name.endswith("f32")
    lp_tol = 1e-3 if exact else (8e-3 if kvd == "float32" else 0.1)
    P = 37
    prompt = _prompt(P, 11)
    ref = ref_generate.load(dirs[name], max_pos=256)
    cache = ref.make_cache(1, paged=(kvd == "float32"))
    y, want, margins, want_lp = prompt[None], [], [], []
    for _ in range(9):
        lg = ref(y, cache=cache)[:, -1].astype(np.float64)
        top2 = np.sort(lg[0])[-2:]
        margins.append(float(top2[1] - top2[0]))
        y = np.argmax(lg, axis=-1)[:, None]
        want.append(int(y[0, 0]))
        want_lp.append(float(lg[0, want[-1]] - (lg[0].max() + np.log(np.exp(lg[0] - lg[0].max()).sum()))))
    kv = _kv(eng, kind, kvd)
    t = _step(eng, kv, [0], prompt[None])["tokens"]
    for _ in range(5):
        t = _step(eng, kv, [0], t[:, None])["tokens"]
    assert kv.offsets[0] == P + 5
    kv.fork_row(0, 1, P - 1)
    assert kv.offsets == [P + 5, P - 1]
    got, got_lp = [], []
    r = _step(eng, kv, [1], prompt[None, P - 1:])
    for i in range(9):
        got.append(int(r["tokens"][0])); got_lp.append(float(r["logprobs"][0]))
        if i < 8:
            r = _step(eng, kv, [1], r["tokens"][:, None])
    kv.close()
    print(name, kind, kvd, "ids", got, want, "max |logprob diff|", max(abs(a - b) for a, b in zip(got_lp, want_lp)))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            assert not exact and margins[i] <= 0.13, (i, got, want, margins[i])
            break
        assert abs(got_lp[i] - want_lp[i]) <= lp_tol, (i, got_lp[i], want_lp[i])


@pytest.mark.parametrize("kvd", ["model", "float32"])
@pytest.mark.parametrize("name", ["d64_bf16", "d96_bf16"])
def test_block_bookkeeping(engines, name, kvd):
    eng = engines[name]
    kv = _kv(eng, "paged", kvd, rows=3)
    free0 = kv.stats()["free_blocks"]
    assert free0 == NBLOCKS - 1
    prompt = _prompt(40, 21)
    first = _step(eng, kv, [0], prompt[None])
    assert kv.stats()["free_blocks"] == free0 - 3
    for n, tail in ((40, 1), (32, 0), (16, 0), (17, 1), (1, 1)):
        for order in ((0, 1), (1, 0)):
            before = kv.stats()["free_blocks"]
            kv.fork_row(0, 1, n)
            assert kv.stats()["free_blocks"] == before - tail and kv.offsets[:2] == [40, n], (n, order)
            for r in order:
                kv.reset_row(r)
            assert kv.stats()["free_blocks"] == free0 and kv.offsets == [0, 0, 0]
            assert kv.stats() == dict(kv.stats(), cached_blocks=0, evictions=0)
            _same(first, _step(eng, kv, [0], prompt[None]), "the same prefill again")
    # fork, then the source goes: dst decodes as the source would have
    want = _step(eng, kv, [0], [[5]])
    kv.reset_row(0)
    _step(eng, kv, [0], prompt[None])
    kv.fork_row(0, 1, 40)
    kv.reset_row(0)
    _step(eng, kv, [2], _prompt(48, 22)[None])           # somebody else takes the blocks that src gave back
    assert kv.offsets == [0, 40, 48]
    _same(want, _step(eng, kv, [1], [[5]]), "dst after the reset of src")
    kv.close()


@pytest.mark.parametrize("kind,kvd", [("paged", "model"), ("contiguous", "float32")])
def test_refusals_name_their_argument_and_change_nothing(engines, kind, kvd):
    import ctypes as C

    from mlx_parallm_amd import _lib as L

    eng = engines["d64_bf16"]
    runs = []
    for refuse in (False, True):
        kv = _kv(eng, kind, kvd, rows=3, n_blocks=6)         # 5 usable blocks
        _step(eng, kv, [0], _prompt(20, 31)[None])           # 2 blocks
        _step(eng, kv, [2], _prompt(5, 32)[None])            # 1 block
        if refuse:
            state = (kv.offsets, kv.stats() if kind == "paged" else None)
            for args, word in (((-1, 1, 4), "src"), ((3, 1, 4), "src"), ((0, -1, 4), "dst"), ((0, 3, 4), "dst"), ((0, 0, 4), "same row"),
                               ((0, 2, 4), "dst must be empty"), ((0, 1, 0), "n_tokens"), ((0, 1, -3), "n_tokens"), ((0, 1, 21), "n_tokens")):
                with pytest.raises(ValueError) as e:
                    kv.fork_row(*args)
                assert "mi_kv_fork_row" in str(e.value) and word in str(e.value), (args, str(e.value))
                assert (kv.offsets, kv.stats() if kind == "paged" else None) == state, args
            assert L.lib().mi_kv_fork_row(None, 0, 1, 4) == -1 and b"null kv" in L.lib().mi_last_error()
            for bad in (True, 1.5, "1", 2 ** 31):
                with pytest.raises(ValueError):
                    kv.fork_row(0, 1, bad)
            if kind == "paged":                              # no block for the tail: the two free blocks go to row 1 first
                _step(eng, kv, [1], _prompt(32, 33)[None])
                assert kv.stats()["free_blocks"] == 0
                kv.reset_row(2)                              # (its block is free again; take it with row 1's next token)
                _step(eng, kv, [1], [[9]])
                full = (kv.offsets, kv.stats())
                assert full[1]["free_blocks"] == 0 and full[1]["evictable_blocks"] == 0
                with pytest.raises(RuntimeError) as e:
                    kv.fork_row(0, 2, 20)
                assert "mi_kv_fork_row" in str(e.value) and "no block for the tail" in str(e.value)
                assert (kv.offsets, kv.stats()) == full
                kv.fork_row(0, 2, 16)                        # full blocks need none
                assert kv.offsets == [20, 33, 16] and kv.stats()["free_blocks"] == 0
        kv.reset_row(2); kv.reset_row(1)                     # both runs end alike: src as it was, the other rows empty
        assert kv.offsets == [20, 0, 0]
        runs.append(dict(_step(eng, kv, [0], [[11]]), logits=eng.forward(np.array([[12], [12], [12]], dtype=np.int32), kv)[0]))
        kv.close()
    _same(runs[0], runs[1], "the next steps of src: the sampler's report, then the full logits")
