"""Full-size checks (-m gpu) at BASELINE.json's headline configuration -- Mistral-7B shape, bf16 (and int4-g64),
batch 8, context up to 1024 -- where the oracle is far too slow to run.  They use properties that do not
depend on the size:

  * the exact-fp32 VALU kernels (oracle-verified element by element at small sizes, test_gpu_kernels.py) and
    the MFMA kernels are two implementations of the same model: their logits must agree to 16-bit rounding
    noise and their greedy tokens must be equal wherever the top-2 margin exceeds that noise;
  * rows of a batch are independent: a sequence decodes to the same tokens alone, in a batch of 8, and
    next to different neighbours -- bit for bit;
  * prefill (tile GEMM + flash-style attention) and token-by-token decode (skinny GEMV + decode attention)
    are two routes to the same KV state: the logits after them agree to rounding noise;
  * the M <= 16 GEMV kernels, the VALU decode attention and the chunked prefill are noise-equal
    alternatives of the default path (the options of mi_engine_set_option);
  * determinism: the same call twice gives identical bits.

Weights are bench.py's synthetic N(0, 0.02^2) tensors (seeded), so the runs are reproducible.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from mlx_parallm_amd.engine import Engine, SampleArgs  # noqa: E402

# Two implementations that round to bf16 at the same points differ only through fp32 summation order, i.e. through
# 1-ulp flips of intermediate roundings; over 32 layers of a random-weight model that grows to (measured,
# tools/fullsize_stats.py) RMS 0.07 / max 0.34 on logits of std 1.28, cosine >= 0.998, and either path's argmax
# is within the other's top 2.  The bounds below leave a factor ~1.7.
RMS_NOISE, MAX_NOISE, MIN_COS, MAX_RANK = 0.12, 0.6, 0.995, 3


@pytest.fixture(scope="module", params=["mistral-7b-bf16", "mistral-7b-int4", "qwen3-14b-bf16", "qwen3-14b-int4"])
def big(request):
    family, prec = request.param.rsplit("-", 1)
    quant = 4 if prec == "int4" else 0
    cfg = dict(bench.SHAPES[family])
    if quant:
        cfg["quantization"] = {"group_size": 64, "bits": quant}
    eng = Engine(cfg, device=0, max_positions=2048, act_dtype="bfloat16")
    bench.load_synthetic(eng, cfg, 0, quant, 0, 1, None)
    yield eng, cfg
    eng.close()


def _greedy(eng, prompts, steps, **opts):
    """Prefill + `steps` greedy steps; -> (tokens [steps+1, B], logits of the first decode input [B, V])."""
    for k, v in opts.items():
        eng.set_option(k, v)
    B = prompts.shape[0]
    kv = eng.new_kv(B, capacity=prompts.shape[1] + steps + 2, kv_dtype="model")
    lg = eng.forward(prompts, kv)
    toks = [np.argmax(lg, axis=-1).astype(np.int32)]
    for _ in range(steps):
        lg2 = eng.forward(toks[-1][:, None], kv)
        toks.append(np.argmax(lg2, axis=-1).astype(np.int32))
    kv.close()
    for k in opts:
        eng.set_option(k, {"force_generic_gemv": 0, "fused_decode_attention": 1, "prefill_gemm": 1,
                           "decode_attention_mfma": 1, "skinny_gemm": 1, "short_prefill_skinny": 1}[k])
    return np.stack(toks), lg


def _noise_equal(la, lb):
    err = la - lb
    assert np.sqrt((err ** 2).mean()) <= RMS_NOISE and np.abs(err).max() <= MAX_NOISE, (np.sqrt((err ** 2).mean()), np.abs(err).max())
    for r in range(la.shape[0]):
        cos = float(np.dot(la[r], lb[r]) / np.linalg.norm(la[r]) / np.linalg.norm(lb[r]))
        assert cos >= MIN_COS, (r, cos)
        assert int((la[r] > la[r, np.argmax(lb[r])]).sum()) <= MAX_RANK and int((lb[r] > lb[r, np.argmax(la[r])]).sum()) <= MAX_RANK


def _same_tokens_up_to_near_ties(a, b, la, lb):
    """Same logits up to rounding noise; token sequences may only part where the deciding logits were a near-tie
    (checked on the first step, whose logits are at hand; a flip there legitimately changes the continuation)."""
    _noise_equal(la, lb)
    for r in range(a.shape[1]):
        if a[0, r] != b[0, r]:
            top2 = np.sort(la[r])[-2:]
            assert top2[1] - top2[0] <= MAX_NOISE, (r, top2)


def test_mfma_path_agrees_with_exact_valu_path(big):
    eng, cfg = big
    rng = np.random.default_rng(3)
    prompts = rng.integers(0, cfg["vocab_size"], size=(8, 96)).astype(np.int32)
    fast, lf = _greedy(eng, prompts, 6)
    exact, le = _greedy(eng, prompts, 6, force_generic_gemv=1, fused_decode_attention=0, prefill_gemm=0, decode_attention_mfma=0)
    assert np.isfinite(lf).all() and lf.std() > 0.05
    _same_tokens_up_to_near_ties(fast, exact, lf, le)
    assert (fast[0] == exact[0]).mean() >= 0.5           # most first tokens agree outright (measured 6-7 of 8)


def test_rows_are_independent_and_runs_are_deterministic(big):
    eng, cfg = big
    rng = np.random.default_rng(4)
    # Rows of ONE call are independent bit for bit; which kernels a call takes depends on its size (<= 128 rows in all: the
    # weight-streaming kernel, test_short_prefill_on_the_streaming_kernel; a few hundred rows: K-split tiles; thousands: plain
    # tiles), so the same sequence in calls of different shapes agrees to rounding noise.
    p = rng.integers(0, cfg["vocab_size"], size=(8, 160)).astype(np.int32)
    p[5] = p[2]                                           # the same sequence twice in one batch
    a, la = _greedy(eng, p, 8)
    b, lb = _greedy(eng, p, 8)
    assert np.array_equal(a, b) and np.array_equal(la, lb)                      # determinism
    assert np.array_equal(a[:, 5], a[:, 2]) and np.array_equal(la[5], la[2])   # same row content, other row index
    # alone: the same model through other launch shapes (160 rows: the 128 x 128 tile with K split over workgroups; 1280
    # rows: no split) -- another summation order, so rounding noise apart, not bit for bit
    solo, ls = _greedy(eng, p[2:3], 8)
    _same_tokens_up_to_near_ties(solo, a[:, 2:3], ls, la[2:3])
    q = p.copy()
    q[[0, 1, 3, 4, 6, 7]] = rng.integers(0, cfg["vocab_size"], size=(6, 160))
    c, lc = _greedy(eng, q, 8)
    assert np.array_equal(c[:, 2], a[:, 2]) and np.array_equal(lc[2], la[2])   # other neighbours


def test_short_prefill_on_the_streaming_kernel(big):
    """A short prompt (dense weights: <= 64 rows, quantised: <= 96 / 128) goes through the decode steps' weight-streaming
    kernel (one read of W, split K) instead of the tile GEMM: same model, another summation order -- the logits agree to
    rounding noise with the tile-GEMM route (option short_prefill_skinny = 0), and it is the faster route at that size
    (measured crossovers: the routes of gemv_rows in engine_linear.hip)."""
    import time

    eng, cfg = big
    rng = np.random.default_rng(8)
    p = rng.integers(0, cfg["vocab_size"], size=(1, 48)).astype(np.int32)
    fast, lf = _greedy(eng, p, 4)
    tile, lt = _greedy(eng, p, 4, short_prefill_skinny=0)
    _same_tokens_up_to_near_ties(fast, tile, lf, lt)

    def timed(**opts):
        for k, v in opts.items():
            eng.set_option(k, v)
        best = 1e9
        for _ in range(3):
            kv = eng.new_kv(1, capacity=128, kv_dtype="model")
            eng.sync(); t0 = time.perf_counter()
            eng.forward(p, kv)
            best = min(best, time.perf_counter() - t0)
            kv.close()
        eng.set_option("short_prefill_skinny", 1)
        return best

    t_fast, t_tile = timed(), timed(short_prefill_skinny=0)
    print(f"48-token prefill: streaming kernel {t_fast * 1e3:.2f} ms, tile GEMM {t_tile * 1e3:.2f} ms")
    assert t_fast < 1.1 * t_tile


def test_prefill_and_stepwise_decode_reach_the_same_state(big):
    eng, cfg = big
    rng = np.random.default_rng(5)
    L0 = 40
    p = rng.integers(0, cfg["vocab_size"], size=(8, L0)).astype(np.int32)
    kv1 = eng.new_kv(8, capacity=64, kv_dtype="model")
    l_prefill = eng.forward(p, kv1)                        # tile GEMM + flash-style attention
    kv2 = eng.new_kv(8, capacity=64, kv_dtype="model")
    for t in range(L0):                                    # skinny GEMV + decode attention, one token at a time
        l_step = eng.forward(p[:, t:t + 1], kv2)
    assert kv1.offsets == kv2.offsets == [L0] * 8
    _noise_equal(l_prefill, l_step)
    nxt = np.argmax(l_prefill, axis=-1).astype(np.int32)[:, None]
    a, b = eng.forward(nxt, kv1), eng.forward(nxt, kv2)    # and both caches continue alike
    _noise_equal(a, b)
    kv1.close()
    kv2.close()


def test_alternative_kernels_agree(big):
    """The M <= 16 GEMV kernels, the VALU decode attention and the chunked prefill give the default path's tokens up to
    near-ties of its logits."""
    eng, cfg = big
    rng = np.random.default_rng(6)
    p = rng.integers(0, cfg["vocab_size"], size=(8, 300)).astype(np.int32)    # 300 keys: split-KV attention
    base, lb = _greedy(eng, p, 5)
    single, ls = _greedy(eng, p, 5, skinny_gemm=0)
    _same_tokens_up_to_near_ties(base, single, lb, ls)                        # the two streaming kernels
    valu, lv = _greedy(eng, p, 5, decode_attention_mfma=0)
    _same_tokens_up_to_near_ties(base, valu, lb, lv)
    chunked, lc = _greedy(eng, p, 5, prefill_gemm=0)
    _same_tokens_up_to_near_ties(base, chunked, lb, lc)


def test_sampling_with_logprobs_config3(big):
    """BASELINE config 3 semantics at full size: top-p 0.9 sampling with log-probabilities -- the sampled token
    must lie in the nucleus computed on the host from the same logits, its logprob must be log_softmax."""
    eng, cfg = big
    rng = np.random.default_rng(7)
    p = rng.integers(0, cfg["vocab_size"], size=(8, 32)).astype(np.int32)
    kv = eng.new_kv(8, capacity=48, kv_dtype="model")
    lg = eng.forward(p, kv).astype(np.float64)
    kv2 = eng.new_kv(8, capacity=48, kv_dtype="model")
    u = rng.random(8).astype(np.float32)
    res = eng.decode_sample(kv2, p, SampleArgs(temp=1.0, top_p=0.9, uniforms=u, top_logprobs=5))
    lsm = lg - lg.max(-1, keepdims=True)
    lsm = lsm - np.log(np.exp(lsm).sum(-1, keepdims=True))
    for b in range(8):
        order = np.argsort(-lsm[b], kind="stable")
        cum = np.cumsum(np.exp(lsm[b][order]))
        nucleus = set(order[:max(1, int(np.searchsorted(cum, 0.9 + 1e-6)) + 1)].tolist())
        assert int(res["tokens"][b]) in nucleus
        assert abs(float(res["logprobs"][b]) - lsm[b, res["tokens"][b]]) <= 1e-3
        assert np.allclose(res["top_logprobs"][b], np.sort(lsm[b])[::-1][:5], atol=1e-3)
    kv.close()
    kv2.close()
