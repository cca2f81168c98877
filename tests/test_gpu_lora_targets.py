"""LoRA on every projection of a block (-m gpu): q, k and v together, gate_proj, up_proj -- the engine against the oracle.

The reference wraps whatever `lora_parameters.keys` names (rl_training/lora_init.py:72,95-96; mlx-lm load_adapters), so an
adapter trained on all seven linears of a block must load.  Per adapted projection  y = T(acc [+ b]),  y = T(y + T(scale (x A) B))
with float32 factors (oracle/ref_model.py:92-108); for gate and up this happens BEFORE silu(gate) * up.

Adapters: the recipe of test_gpu_engine.py::test_lora_adapter_applied (rank 16, scale 10, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2),
float32) on the LAST TWO blocks -- every tiny model has two or three, so layer 0 of the two-layer ones (with its logical
rounding in the float32-KV mode) is adapted.  A projection's factors are the same in every subset adapter of a model.

Bounds (the project's own, tests/test_gpu_engine.py):
  float32-KV (oracle: paged cache)  greedy ids exact, logprobs within 1e-3 over the prompt + 3 decode steps; logits within 4e-3
  model-dtype KV                    logits within 0.08
The oracle's own float32-accumulating variants stay within 1.2e-6 (float32-KV) of the exact oracle with these adapters and
equal it in the model-KV mode; the largest |logit| is 2.3-3.1.

Every new term must be seen: on the oracle alone, the full adapter's logits differ from the same adapter without k_proj, without
gate_proj and without up_proj by at least 5 x the tolerance of the mode under test."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import biased_ref
from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from mlx_parallm_amd.weight_updater import apply_lora_update  # noqa: E402

MAX_POS = 256
RANK, SCALE, NLAYERS = 16, 10.0, 2
ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
       "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
QKV = ALL[:3]
MODELS = ["llama_q4_bf16", "qwen3_bf16", "llama_q8_f16", "llama_f16", "llama_f32"]
REGIME_MODELS = ["llama_q4_bf16", "qwen3_bf16"]
# mode -> (kv dtype of the engine, oracle paged cache, logit tolerance)
MODES = {"float32": ("float32", True, 4e-3), "model": ("model", False, 0.08)}
LOGPROB_TOL_F32KV = 1e-3
MODEL_KV_LOGPROB_TOL, MODEL_KV_MARGIN = 0.1, 0.13       # mixed steps return no logits: test_gpu_engine.py's bounds on what they return


def _dims(cfg):
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D = cfg.get("head_dim") or H // nh
    I = cfg["intermediate_size"]
    # key -> (K, n)
    return {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}


def _factors(cfg, seed):
    """{tensor name: float32 array} for all seven keys of the last NLAYERS blocks; one generator per (layer, key)"""
    dims = _dims(cfg)
    nl = cfg["num_hidden_layers"]
    w = {}
    for i in range(nl - NLAYERS, nl):
        for ki, key in enumerate(ALL):
            K, n = dims[key]
            rng = np.random.default_rng([seed, i, ki])
            w[f"model.layers.{i}.{key}.lora_a"] = (rng.uniform(-1, 1, (K, RANK)) / np.sqrt(K)).astype(np.float32)
            w[f"model.layers.{i}.{key}.lora_b"] = (rng.standard_normal((RANK, n)) * 0.05).astype(np.float32)
    return w


def _write(dst, factors, keys, scale=SCALE):
    dst.mkdir(parents=True, exist_ok=True)
    w = {k: torch.from_numpy(v) for k, v in factors.items() if any(f".{key}.lora_" in k for key in keys)}
    save_file(w, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": NLAYERS,
        "lora_parameters": {"rank": RANK, "scale": scale, "dropout": 0.0, "keys": list(keys)}}))
    return str(dst)


class Bank:
    """Adapter directories and oracles, made on first use and shared (read-only) by the tests of this module."""

    def __init__(self, tiny_dirs, root):
        self.tiny, self.root = tiny_dirs, root
        self._fac, self._dir, self._ref = {}, {}, {}

    def cfg(self, name):
        return self.tiny[name][1]

    def factors(self, name, seed=5):
        if (name, seed) not in self._fac:
            self._fac[(name, seed)] = _factors(self.cfg(name), seed)
        return self._fac[(name, seed)]

    def adapter(self, name, keys, seed=5):
        k = (name, tuple(keys), seed)
        if k not in self._dir:
            self._dir[k] = _write(self.root / f"{name}_{len(self._dir)}", self.factors(name, seed), keys)
        return self._dir[k]

    def ref(self, name, keys, seed=5):
        k = (name, tuple(keys), seed)
        if k not in self._ref:
            self._ref[k] = ref_generate.load(self.tiny[name][0], adapter_path=self.adapter(name, keys, seed), max_pos=MAX_POS)
        return self._ref[k]

    def engine_model(self, name, keys=None, seed=5):
        model = utils.load_model(self.tiny[name][0], max_positions=MAX_POS)
        if keys:
            utils.load_adapters(model, self.adapter(name, keys, seed))
        return model


@pytest.fixture(scope="module")
def bank(tiny_dirs, tmp_path_factory):
    return Bank(tiny_dirs, tmp_path_factory.mktemp("lora_targets"))


def _prompts(cfg, B, L0, seed):
    rng = np.random.default_rng([seed, B, L0])
    toks = rng.integers(3, cfg["vocab_size"], size=(B, L0))
    for b in range(B):
        toks[b, : int(rng.integers(0, L0 // 2))] = 1          # left padding; pads are attended
    return toks.astype(np.int32)


def _logits_run(model, ref, toks, mode, steps, all_positions=False):
    """forward logits of the prompt and of `steps` teacher-forced decode steps -> max |engine - oracle|"""
    kvd, paged, _ = MODES[mode]
    B, L0 = toks.shape
    kv = model.engine.new_kv(B, capacity=L0 + steps + 1, kv_dtype=kvd)
    cache = ref.make_cache(B, paged=paged)
    got = model.engine.forward(toks, kv, all_positions=all_positions)
    want = ref(toks, cache=cache)
    err = float(np.abs(got - (want if all_positions else want[:, -1])).max())
    nxt = np.argmax(want[:, -1], axis=-1)[:, None]
    for _ in range(steps):
        got = model.engine.forward(nxt.astype(np.int32), kv)
        want = ref(nxt, cache=cache)[:, -1]
        err = max(err, float(np.abs(got - want).max()))
        nxt = np.argmax(want, axis=-1)[:, None]
    kv.close()
    return err


def _greedy_run(model, ref, toks, mode, steps):
    """generate_step's path (forward + sampler), teacher-forced: -> (ids that differ from the oracle's, max |logprob - oracle|)"""
    kvd, paged, _ = MODES[mode]
    B, L0 = toks.shape
    kv = model.engine.new_kv(B, capacity=L0 + steps + 1, kv_dtype=kvd)
    cache = ref.make_cache(B, paged=paged)
    y, wrong, lp_err = toks, 0, 0.0
    for _ in range(steps + 1):
        res = model.engine.decode_sample(kv, y.astype(np.int32), SampleArgs(temp=0.0))
        want = ref_sample.sample(ref(y, cache=cache)[:, -1], temp=0.0)
        wrong += int((res["tokens"] != want["tokens"][:, 0]).sum())
        same = res["tokens"] == want["tokens"][:, 0]
        if same.any():
            lp_err = max(lp_err, float(np.abs(res["logprobs"] - want["logprobs"].reshape(-1))[same].max()))
        y = want["tokens"]
    kv.close()
    return wrong, lp_err


def _check(model, ref, toks, mode, steps=3, all_positions=False, what=""):
    err = _logits_run(model, ref, toks, mode, steps, all_positions)
    print(f"{what} {mode}: max |logit - oracle| = {err:.3e}")
    assert err <= MODES[mode][2], (what, mode, err)
    if mode == "float32":
        wrong, lp_err = _greedy_run(model, ref, toks, mode, steps)
        print(f"{what} {mode}: ids off {wrong}, max |logprob - oracle| = {lp_err:.3e}")
        assert wrong == 0 and lp_err <= LOGPROB_TOL_F32KV, (what, wrong, lp_err)


# ------------------------------------------------------------------------------------ all seven keys, every model
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", MODELS)
def test_all_seven_projections(bank, name, mode):
    cfg = bank.cfg(name)
    toks = _prompts(cfg, 2, 7, seed=1)
    full = bank.ref(name, ALL)
    _, paged, tol = MODES[mode]
    want = full(toks, cache=full.make_cache(2, paged=paged))[:, -1]
    for drop in ("self_attn.k_proj", "mlp.gate_proj", "mlp.up_proj"):          # every new term is seen (oracle alone)
        less = bank.ref(name, [k for k in ALL if k != drop])
        effect = float(np.abs(want - less(toks, cache=less.make_cache(2, paged=paged))[:, -1]).max())
        print(f"{name} {mode}: effect of {drop} on the oracle's logits = {effect:.3f}")
        assert effect >= 5 * tol, (drop, effect)
    model = bank.engine_model(name, ALL)
    _check(model, full, toks, mode, what=f"{name} all-seven")
    model.engine.close()


# ------------------------------------------------------------------------------------ row regimes
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", REGIME_MODELS)
def test_row_regimes(bank, name, mode):
    """prefill 2 x 7 and decode at B = 2; decode at B = 12 (the 9..128-row kernel); a prefill of 3 x 60 = 180 rows (above the
    streaming kernels' limit: the tile GEMM and the up-add behind it, all positions); one mixed step."""
    cfg, ref = bank.cfg(name), bank.ref(name, ALL)
    model = bank.engine_model(name, ALL)
    _check(model, ref, _prompts(cfg, 2, 7, seed=2), mode, what=f"{name} 2x7")
    _check(model, ref, _prompts(cfg, 12, 3, seed=3), mode, what=f"{name} B=12")
    _check(model, ref, _prompts(cfg, 3, 60, seed=4), mode, steps=1, all_positions=True, what=f"{name} 3x60")
    model.engine.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", REGIME_MODELS)
def test_mixed_step(bank, name, mode):
    """mi_step_enqueue_mixed: two decode rows plus a 5-token chunk of a third sequence in one pass over the weights; then one
    plain forward over the three rows (its logits depend on the K / V the mixed step wrote)."""
    cfg, ref = bank.cfg(name), bank.ref(name, ALL)
    kvd, paged, tol = MODES[mode]
    model = bank.engine_model(name, ALL)
    eng = model.engine
    rng = np.random.default_rng(9)
    P = [rng.integers(3, cfg["vocab_size"], size=n).astype(np.int32) for n in (6, 4, 5)]
    greedy = SampleArgs(temp=0.0)
    kv = eng.new_kv(3, capacity=32, kv_dtype=kvd)
    caches = [ref.make_cache(1, paged=paged) for _ in P]

    def oracle(i, toks):
        lg = ref(np.asarray(toks, dtype=np.int32)[None], cache=caches[i])[0, -1]
        return lg, ref_sample.sample(lg[None], temp=0.0)

    def compare(res, wants):
        for j, (lg, w) in enumerate(wants):
            gt, wt = int(res["tokens"][j]), int(w["tokens"][0, 0])
            if mode == "float32":
                assert gt == wt, (j, gt, wt)
                assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= LOGPROB_TOL_F32KV
            else:
                assert gt == wt or float(lg[wt] - lg[gt]) <= MODEL_KV_MARGIN, (j, gt, wt)
                if gt == wt:
                    assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= MODEL_KV_LOGPROB_TOL

    res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1], [P[0], P[1]], [1, 1], greedy), 2)      # the two live rows' prompts
    w0, w1 = oracle(0, P[0]), oracle(1, P[1])
    compare(res, [w0, w1])
    t0, t1 = int(w0[1]["tokens"][0, 0]), int(w1[1]["tokens"][0, 0])
    res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 2], [[t0], [t1], P[2]], [1, 1, 1], greedy), 3)   # THE mixed step
    assert kv.offsets == [7, 5, 5]
    wants = [oracle(0, [t0]), oracle(1, [t1]), oracle(2, P[2])]
    compare(res, wants)
    nxt = np.asarray([[int(w[1]["tokens"][0, 0])] for w in wants], dtype=np.int32)
    got = eng.forward(nxt, kv)
    want = np.stack([oracle(i, nxt[i])[0] for i in range(3)])
    err = float(np.abs(got - want).max())
    print(f"{name} {mode}: forward behind the mixed step, max |logit - oracle| = {err:.3e}")
    assert err <= tol, err
    kv.close()
    eng.close()


# ------------------------------------------------------------------------------------ subsets
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("keys", [QKV, ("mlp.gate_proj",), ("mlp.up_proj",), ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")],
                         ids=["qkv", "gate", "up", "gate_up_down"])
@pytest.mark.parametrize("name", REGIME_MODELS)
def test_subsets(bank, name, keys, mode):
    cfg = bank.cfg(name)
    model = bank.engine_model(name, keys)
    _check(model, bank.ref(name, keys), _prompts(cfg, 2, 7, seed=6), mode, steps=2, what=f"{name} {'+'.join(keys)}")
    model.engine.close()


# ------------------------------------------------------------------------------------ a rank of its own per projection
MIXED_RANKS = {"self_attn.q_proj": 1, "self_attn.k_proj": 5, "self_attn.v_proj": 64, "self_attn.o_proj": 16}


@pytest.mark.parametrize("mode", list(MODES))
def test_q_k_v_at_three_ranks_plus_o(tiny_dirs, tmp_path, mode):
    """One engine-wide adapter whose q, k and v have ranks 1, 5 and 64 (the scalar and the vector walk of the down kernel in
    one launch over the three parts of q|k|v) and whose o has rank 16: every part of the table carries its own rank."""
    name = "qwen3_bf16"
    path, cfg = tiny_dirs[name]
    fac, dims, nl = {}, _dims(cfg), cfg["num_hidden_layers"]
    for i in range(nl - NLAYERS, nl):
        for ki, (key, rank) in enumerate(MIXED_RANKS.items()):
            K, n = dims[key]
            rng = np.random.default_rng([21, i, ki, rank])
            fac[f"model.layers.{i}.{key}.lora_a"] = (rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32)
            fac[f"model.layers.{i}.{key}.lora_b"] = (rng.standard_normal((rank, n)) * 0.05).astype(np.float32)
    full = ref_generate.load(path, adapter_path=_write(tmp_path / "full", fac, list(MIXED_RANKS)), max_pos=MAX_POS)
    no_k = [k for k in MIXED_RANKS if k != "self_attn.k_proj"]
    less = ref_generate.load(path, adapter_path=_write(tmp_path / "no_k", fac, no_k), max_pos=MAX_POS)
    toks = _prompts(cfg, 3, 9, seed=15)
    _, paged, tol = MODES[mode]
    want = full(toks, cache=full.make_cache(3, paged=paged))[:, -1]
    effect = float(np.abs(want - less(toks, cache=less.make_cache(3, paged=paged))[:, -1]).max())
    print(f"{name} {mode}: effect of the rank-5 k_proj on the oracle's logits = {effect:.3f}")
    assert effect >= 5 * tol, effect
    model = utils.load_model(path, max_positions=MAX_POS)
    utils.load_adapters(model, str(tmp_path / "full"))
    _check(model, full, toks, mode, steps=3, what=f"{name} q r1 + k r5 + v r64 + o r16")
    model.engine.close()


# ------------------------------------------------------------------------------------ live changes
def _bits(model, cfg, seed=8):
    """logits of a prefill, a decode step at B = 2 and one at B = 12, both KV modes -- for bit-for-bit comparisons"""
    out = []
    for kvd in ("float32", "model"):
        for B, L0 in ((2, 7), (12, 3)):
            toks = _prompts(cfg, B, L0, seed)
            kv = model.engine.new_kv(B, capacity=L0 + 2, kv_dtype=kvd)
            out.append(model.engine.forward(toks, kv, all_positions=True))
            out.append(model.engine.forward(toks[:, -1:], kv))
            kv.close()
    return out


def _assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), float(np.abs(x - y).max())


@pytest.mark.parametrize("name", REGIME_MODELS)
def test_k_arrives_after_q_and_v(bank, name):
    """A finalized engine with q / v adapted, already used, receives k through apply_lora_update: the same routes, hence the
    same bits, as a fresh engine loaded with q + k + v."""
    cfg = bank.cfg(name)
    live = bank.engine_model(name, ("self_attn.q_proj", "self_attn.v_proj"))
    before = _bits(live, cfg)
    apply_lora_update(live, bank.adapter(name, ("self_attn.k_proj",)))
    after = _bits(live, cfg)
    assert any(not np.array_equal(x, y) for x, y in zip(before, after))          # k changed the outputs
    fresh = bank.engine_model(name, QKV)
    _assert_same_bits(after, _bits(fresh, cfg))
    live.engine.close(); fresh.engine.close()


@pytest.mark.parametrize("name", REGIME_MODELS)
def test_gate_arrives_on_a_live_engine_and_is_hot_swapped(bank, name):
    """An unadapted finalized engine (dense bf16: its row-interleaved gate|up copy is built and has served decode steps) receives
    gate, then gate again with new factors: each time bit-equal to a fresh engine loaded with that adapter."""
    cfg = bank.cfg(name)
    live = bank.engine_model(name)
    plain = _bits(live, cfg)
    for seed in (5, 11):                                                          # first arrival, then one hot-swap
        apply_lora_update(live, bank.adapter(name, ("mlp.gate_proj",), seed))
        got = _bits(live, cfg)
        assert any(not np.array_equal(x, y) for x, y in zip(plain, got))
        fresh = bank.engine_model(name, ("mlp.gate_proj",), seed)
        _assert_same_bits(got, _bits(fresh, cfg))
        fresh.engine.close()
        plain = got
    live.engine.close()


def test_adapter_change_invalidates_published_prefixes(bank):
    """K / V computed without the k adapter must not be served to a request that runs with it."""
    name = "llama_q4_bf16"
    cfg = bank.cfg(name)
    model = bank.engine_model(name, ("self_attn.q_proj", "self_attn.v_proj"))
    eng = model.engine
    kv = eng.new_paged_kv(2, block_tokens=16, n_blocks=12, max_tokens_per_row=64, kv_dtype="model")
    toks = np.random.default_rng(3).integers(3, cfg["vocab_size"], size=40).astype(np.int32)     # two full blocks + 8 tokens
    eng.step_wait(eng.step_enqueue_rows(kv, [0], toks[None], SampleArgs(temp=0.0)), 1)
    kv.prefix_publish(0, toks)
    assert kv.prefix_attach(1, toks) == 32
    kv.reset_row(1)
    last = cfg["num_hidden_layers"] - 1
    fac = bank.factors(name)
    eng.set_lora(last, "self_attn.k_proj", fac[f"model.layers.{last}.self_attn.k_proj.lora_a"],
                 fac[f"model.layers.{last}.self_attn.k_proj.lora_b"], SCALE)
    assert kv.prefix_attach(1, toks) == 0
    kv.close()
    eng.close()


# ------------------------------------------------------------------------------------ biases, traditional RoPE
SHAPE = dict(vocab_size=512, dtype="bfloat16", hidden_size=128, heads=8, kv_heads=2, intermediate_size=256, head_dim=16,
             tie_word_embeddings=False, norm_jitter=0.1, with_tokenizer=False, layers=2)


@pytest.mark.parametrize("quantized", [False, True], ids=["bf16", "q4_bf16"])
def test_biased_checkpoint_all_seven(tmp_path, quantized):
    """attention_bias + mlp_bias: y = T(acc + b) (dense) / T(T(acc) + b) (quantised) FIRST, then the LoRA term; float32-KV,
    ids exact and logprobs within 1e-3, logits within 4e-3 (reference linears: tests/biased_ref.py)."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(tmp_path / "m", attention_bias=True, mlp_bias=True, quantize_model=quantized, seed=31, **SHAPE)
    ad = _write(tmp_path / "ad", _factors(cfg, 5), ALL)
    ref = biased_ref.load(str(tmp_path / "m"), adapter_path=ad, max_pos=MAX_POS)
    plain = ref_generate.load(str(tmp_path / "m"), adapter_path=ad, max_pos=MAX_POS)
    toks = _prompts(cfg, 2, 7, seed=12)
    a = ref(toks, cache=ref.make_cache(2, paged=True))[:, -1]
    b = plain(toks, cache=plain.make_cache(2, paged=True))[:, -1]
    assert np.abs(a - b).max() > 0.1                                              # the biases matter
    model = utils.load_model(str(tmp_path / "m"), max_positions=MAX_POS)
    utils.load_adapters(model, ad)
    _check(model, ref, toks, "float32", what="biased all-seven")
    _check(model, ref, _prompts(cfg, 12, 3, seed=13), "float32", what="biased all-seven B=12")
    model.engine.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_traditional_rope_with_q_k_v_adapted(tmp_path, mode):
    """rope_traditional regroups the rows of q / k at load time and the columns of their LoRA B with them -- k in the third
    place included.  Oracle: the pi-permuted checkpoint and adapter in the half-split convention (biased_ref.py)."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(tmp_path / "trad", rope_traditional=True, quantize_model=False, seed=32, **SHAPE)
    ad = _write(tmp_path / "ad", _factors(cfg, 5), QKV)
    biased_ref.permuted_checkpoint(str(tmp_path / "trad"), str(tmp_path / "perm"), ad, str(tmp_path / "ad_perm"))
    ref = ref_generate.load(str(tmp_path / "perm"), adapter_path=str(tmp_path / "ad_perm"), max_pos=MAX_POS)
    model = utils.load_model(str(tmp_path / "trad"), max_positions=MAX_POS)
    utils.load_adapters(model, ad)
    _check(model, ref, _prompts(cfg, 2, 7, seed=14), mode, what="rope_traditional q+k+v")
    model.engine.close()


# ------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_engine_as_it_was(bank):
    name = "llama_q4_bf16"
    cfg = bank.cfg(name)
    model = bank.engine_model(name, ALL)
    eng = model.engine
    before = _bits(model, cfg)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    last = cfg["num_hidden_layers"] - 1
    rng = np.random.default_rng(1)
    a16 = torch.from_numpy(rng.standard_normal((H, RANK)).astype(np.float32)).to(torch.bfloat16).cuda()
    b16 = torch.from_numpy(rng.standard_normal((RANK, I)).astype(np.float32)).to(torch.bfloat16).cuda()
    torch.cuda.synchronize()
    rc = L.lib().mi_engine_set_lora(eng._h, last, b"mlp.gate_proj", C.c_void_p(a16.data_ptr()), C.c_void_p(b16.data_ptr()),
                                    RANK, 10.0, L.MI_BF16, 1)                     # 16-bit factors
    assert rc == -3 and b"16-bit" in L.lib().mi_last_error()
    with pytest.raises(NotImplementedError, match="rank"):
        eng.set_lora(last, "mlp.up_proj", rng.standard_normal((H, 65)).astype(np.float32),
                     rng.standard_normal((65, I)).astype(np.float32), 10.0)
    for proj in ("lm_head", "model.embed_tokens", "embed_tokens", "mlp.gate"):
        with pytest.raises(NotImplementedError, match="not supported"):
            eng.set_lora(last, proj, rng.standard_normal((H, RANK)).astype(np.float32),
                         rng.standard_normal((RANK, cfg["vocab_size"])).astype(np.float32), 10.0)
    _assert_same_bits(before, _bits(model, cfg))
    eng.close()
