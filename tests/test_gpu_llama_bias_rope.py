"""End-to-end parity (-m gpu) of llama checkpoints with linear biases (attention_bias, mlp_bias) and traditional RoPE
(rope_traditional) -- llama.py:59-67,77-82,155-162 -- through utils.load_model and the C ABI, against tests/biased_ref.py.

Checkpoints (module fixture): hidden 128, 8 heads / 2 kv heads of 16, intermediate 256, vocabulary 512, untied; dense bf16
(3 layers) and int4-g64 bf16 (2 layers).  Each is built with both bias flags AND rope_traditional ("trad"); its pi-permuted
copy with the flag cleared ("perm", biased_ref.permuted_checkpoint) is the same model in the half-split convention: the oracle
on "perm" is the oracle of both, "perm" on the engine exercises the biases alone, "trad" the load-time regrouping.

Bounds are those of tests/test_gpu_engine.py: float32-KV mode ids equal but for at most one near-tie under 2e-3, logprobs within
1e-3 (test_greedy_float32_kv_mode_16bit_models); model-KV mode ids equal where the oracle's margin exceeds 0.13, logprobs within
0.1 (test_greedy_model_dtype_kv_16bit_models)."""
import json
import shutil

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

import biased_ref

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import Engine, SampleArgs  # noqa: E402
from test_gpu_engine import MODEL_KV_LOGPROB_TOL, _left_pad_prompts, _teacher_forced_greedy  # noqa: E402

RNG = np.random.default_rng(77)
MAX_POS = 256
SHAPE = dict(vocab_size=512, dtype="bfloat16", hidden_size=128, heads=8, kv_heads=2, intermediate_size=256, head_dim=16,
             tie_word_embeddings=False, norm_jitter=0.1, with_tokenizer=False)
VARIANTS = {"bf16": dict(quantize_model=False, layers=3, seed=21), "q4_bf16": dict(quantize_model=True, layers=2, seed=22)}


def _write_adapter(dst, cfg, seed, keys=("self_attn.q_proj", "self_attn.v_proj"), rank=16):
    H, nh, nkv, D = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    rng = np.random.default_rng(seed)
    last = cfg["num_hidden_layers"] - 1
    w = {}
    for key in keys:
        n = nh * D if key.endswith("q_proj") else nkv * D
        w[f"model.layers.{last}.{key}.lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (H, rank)) / np.sqrt(H)).astype(np.float32))
        w[f"model.layers.{last}.{key}.lora_b"] = torch.from_numpy(rng.standard_normal((rank, n)).astype(np.float32) * 0.05)
    dst.mkdir(parents=True, exist_ok=True)
    save_file(w, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": 1,
        "lora_parameters": {"rank": rank, "scale": 10.0, "dropout": 0.0, "keys": list(keys)}}))


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """variant -> {"trad", "perm", "adapter", "adapter_perm", "adapter2", "adapter2_perm": directories, "cfg", "ref": oracle}"""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    root = tmp_path_factory.mktemp("bias_rope")
    out = {}
    for name, kw in VARIANTS.items():
        d = root / name
        cfg = build_tiny_model(d / "trad", attention_bias=True, mlp_bias=True, rope_traditional=True, **SHAPE, **kw)
        _write_adapter(d / "adapter", cfg, seed=5)
        _write_adapter(d / "adapter2", cfg, seed=6, keys=("self_attn.q_proj",))
        biased_ref.permuted_checkpoint(str(d / "trad"), str(d / "perm"), str(d / "adapter"), str(d / "adapter_perm"))
        biased_ref.permuted_checkpoint(str(d / "trad"), str(d / "perm"), str(d / "adapter2"), str(d / "adapter2_perm"))
        out[name] = {k: str(d / k) for k in ("trad", "perm", "adapter", "adapter_perm", "adapter2", "adapter2_perm")}
        out[name]["cfg"] = cfg
        out[name]["ref"] = biased_ref.load(str(d / "perm"), max_pos=MAX_POS)          # one oracle per variant, shared, read-only
    return out


def _engine_model(path):
    return utils.load_model(path, max_positions=MAX_POS)


def _check_row(logits_row, tok, logprob, margin_eps=2e-3, lp_tol=1e-3):
    lg = logits_row.astype(np.float64)
    lse = np.log(np.exp(lg - lg.max()).sum()) + lg.max()
    assert lg.max() - lg[tok] <= margin_eps, (tok, int(np.argmax(lg)), float(lg.max() - lg[tok]))
    assert abs((lg[tok] - lse) - float(logprob)) <= lp_tol, (float(lg[tok] - lse), float(logprob))


# ------------------------------------------------------------------------------------------------ biases
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_float32_kv_greedy(ckpts, variant):
    c = ckpts[variant]
    model = _engine_model(c["perm"])
    near, total, lp_err = _teacher_forced_greedy(model, c["ref"], c["cfg"], "float32", True, B=4, L0=12, steps=24,
                                                 margin_eps=2e-3)
    print(f"{variant}: near ties {near}/{total}, max |logprob - oracle| = {lp_err:.2e}")
    assert near <= 1 and lp_err <= 1e-3, (near, total, lp_err)
    # the biases matter: the oracle without them is another model
    plain = biased_ref.ref_generate.load(c["perm"], max_pos=MAX_POS)
    toks = _left_pad_prompts(c["cfg"], 2, 8)
    a = c["ref"](toks, cache=c["ref"].make_cache(2, paged=True))[:, -1]
    b = plain(toks, cache=plain.make_cache(2, paged=True))[:, -1]
    assert np.abs(a - b).max() > 0.1
    model.engine.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_model_kv_greedy(ckpts, variant):
    c = ckpts[variant]
    model = _engine_model(c["perm"])
    near, total, lp_err = _teacher_forced_greedy(model, c["ref"], c["cfg"], "model", False, B=4, L0=12, steps=24,
                                                 margin_eps=0.13)
    print(f"{variant}: near ties {near}/{total}, max |logprob - oracle| = {lp_err:.4f}")
    assert near <= max(2, total // 10), (near, total)
    assert lp_err <= MODEL_KV_LOGPROB_TOL, lp_err
    model.engine.close()


@pytest.mark.parametrize("B", [11, 40])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_decode_steps_of_many_rows(ckpts, variant, B):
    """11 rows: the 16-row instantiations of the split-K streaming kernel; 40: its 32-row / 48-row ones (int4: row slabs)"""
    c = ckpts[variant]
    model = _engine_model(c["perm"])
    near, total, lp_err = _teacher_forced_greedy(model, c["ref"], c["cfg"], "float32", True, B=B, L0=6, steps=4, margin_eps=2e-3)
    assert near <= 1 and lp_err <= 1e-3, (near, total, lp_err)
    near, total, lp_err = _teacher_forced_greedy(model, c["ref"], c["cfg"], "model", False, B=B, L0=6, steps=4, margin_eps=0.13)
    assert near <= max(2, total // 10) and lp_err <= MODEL_KV_LOGPROB_TOL, (near, total, lp_err)
    model.engine.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_prefill_through_the_tile_gemm(ckpts, variant):
    """4 x 40 tokens = 160 rows: the tile GEMM in both modes (float32 activations: over the split image); all-position logits,
    bounds of test_float32_kv_prefill_through_the_tile_gemm / test_prefill_and_decode_logits"""
    c = ckpts[variant]
    model, ref = _engine_model(c["perm"]), c["ref"]
    toks = _left_pad_prompts(c["cfg"], 4, 40)
    for kvd, paged, tol, rms_tol in (("float32", True, 4e-3, 2e-4), ("model", False, 0.08, None)):
        kv = model.engine.new_kv(4, capacity=48, kv_dtype=kvd)
        got = model.engine.forward(toks, kv, all_positions=True)
        want = ref(toks, cache=ref.make_cache(4, paged=paged))
        err = np.abs(got - want)
        print(f"{variant} {kvd}: max {err.max():.2e} rms {np.sqrt((err ** 2).mean()):.2e}")
        assert err.max() <= tol, (kvd, err.max())
        if rms_tol is not None:
            assert np.sqrt((err ** 2).mean()) <= rms_tol
        kv.close()
    model.engine.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_mixed_step(ckpts, variant):
    """mi_step_enqueue_mixed: a 20-token chunk next to two decode rows, float32-KV mode; every row against the oracle run of its
    own sequence (rows are independent)"""
    c = ckpts[variant]
    model, ref = _engine_model(c["perm"]), c["ref"]
    eng, V = model.engine, c["cfg"]["vocab_size"]
    greedy = SampleArgs(temp=0.0)
    kv = eng.new_kv(3, capacity=64, kv_dtype="float32")
    p02 = RNG.integers(3, V, size=(2, 6)).astype(np.int32)
    p1 = RNG.integers(3, V, size=20).astype(np.int32)
    r = eng.step_wait(eng.step_enqueue_rows(kv, [0, 2], p02, greedy), 2)
    caches = [ref.make_cache(1, paged=True) for _ in range(3)]
    for i, row in enumerate((0, 2)):
        _check_row(ref(p02[i:i + 1], cache=caches[row])[0, -1], int(r["tokens"][i]), r["logprobs"][i])
    t0, t2 = int(r["tokens"][0]), int(r["tokens"][1])
    m = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 2, 1], [[t0], [t2], p1], [1, 1, 1], greedy), 3)
    for i, (row, toks) in enumerate(((0, [t0]), (2, [t2]), (1, p1))):
        lg = ref(np.asarray(toks)[None], cache=caches[row])[0, -1]
        _check_row(lg, int(m["tokens"][i]), m["logprobs"][i])
    assert kv.offsets == [7, 20, 7]
    eng.close()


@pytest.mark.parametrize("kvd", ["model", "float32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_paged_kv_is_bit_identical_to_contiguous_kv(ckpts, variant, kvd):
    c = ckpts[variant]
    model = _engine_model(c["perm"])
    eng = model.engine
    toks = RNG.integers(3, c["cfg"]["vocab_size"], size=(3, 37)).astype(np.int32)
    flat = eng.new_kv(3, capacity=128, kv_dtype=kvd)
    paged = eng.new_paged_kv(3, block_tokens=16, n_blocks=40, max_tokens_per_row=128, kv_dtype=kvd)
    a, b = eng.forward(toks, flat, all_positions=True), eng.forward(toks, paged, all_positions=True)
    assert np.array_equal(a, b)
    nxt = np.argmax(a[:, -1], axis=-1).astype(np.int32)[:, None]
    for _ in range(6):
        a, b = eng.forward(nxt, flat), eng.forward(nxt, paged)
        assert np.array_equal(a, b)
        nxt = np.argmax(a, axis=-1).astype(np.int32)[:, None]
    eng.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_biases_with_lora_on_q_and_v(ckpts, variant):
    """LoRALinear wraps the biased linear: y = T(acc + b) first, then y = T(y + T(z)) -- float32-KV mode, logprobs 1e-3"""
    c = ckpts[variant]
    model = _engine_model(c["perm"])
    utils.load_adapters(model, c["adapter_perm"])
    ref = biased_ref.load(c["perm"], adapter_path=c["adapter_perm"], max_pos=MAX_POS)
    near, total, lp_err = _teacher_forced_greedy(model, ref, c["cfg"], "float32", True, B=4, L0=12, steps=8, margin_eps=2e-3)
    assert near <= 1 and lp_err <= 1e-3, (near, total, lp_err)
    toks = _left_pad_prompts(c["cfg"], 2, 8)       # the adapter really changes the logits
    a = ref(toks, cache=ref.make_cache(2, paged=True))[:, -1]
    b = c["ref"](toks, cache=c["ref"].make_cache(2, paged=True))[:, -1]
    assert np.abs(a - b).max() > 0.01
    model.engine.close()


# ------------------------------------------------------------------------------------------------ traditional RoPE
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rope_traditional_matches_the_oracle_on_the_permuted_copy(ckpts, variant):
    """q.k summed exactly does not depend on the order of the head's elements, so the oracle on the pi-permuted checkpoint is
    the traditional model's oracle"""
    c = ckpts[variant]
    assert c["cfg"]["rope_traditional"] is True
    model = _engine_model(c["trad"])
    near, total, lp_err = _teacher_forced_greedy(model, c["ref"], c["cfg"], "float32", True, B=4, L0=12, steps=24,
                                                 margin_eps=2e-3)
    assert near <= 1 and lp_err <= 1e-3, (near, total, lp_err)
    model.engine.close()


def _logit_trace(eng, toks, kvd, steps=8):
    kv = eng.new_kv(toks.shape[0], capacity=toks.shape[1] + steps + 1, kv_dtype=kvd)
    out = [eng.forward(toks, kv, all_positions=True).reshape(-1)]
    nxt = np.argmax(out[0].reshape(toks.shape[0], toks.shape[1], -1)[:, -1], axis=-1).astype(np.int32)[:, None]
    for _ in range(steps):
        lg = eng.forward(nxt, kv)
        out.append(lg.reshape(-1))
        nxt = np.argmax(lg, axis=-1).astype(np.int32)[:, None]
    kv.close()
    return np.concatenate(out)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rope_traditional_is_the_load_time_permutation_bit_for_bit(ckpts, variant):
    """the engine on the flagged checkpoint against the engine on its permuted copy (flag off): identical logits over a prefill
    and 8 decode steps in both KV modes; then with a q_proj + v_proj adapter, and after a hot-swap to a q_proj adapter"""
    c = ckpts[variant]
    trad, perm = _engine_model(c["trad"]), _engine_model(c["perm"])
    toks = _left_pad_prompts(c["cfg"], 3, 9)
    base = {}
    for kvd in ("float32", "model"):
        a, b = _logit_trace(trad.engine, toks, kvd), _logit_trace(perm.engine, toks, kvd)
        assert np.array_equal(a, b), kvd
        base[kvd] = a
    # the flag is not a no-op: the same tensors read WITHOUT it are another model
    cfg_off = dict(c["cfg"], rope_traditional=False)
    off = Engine(dict(cfg_off, model_type="llama"), max_positions=MAX_POS, act_dtype="bfloat16")
    off.load_tensors(load_file(c["trad"] + "/model.safetensors").items())
    off.finalize()
    assert np.abs(_logit_trace(off, toks, "float32") - base["float32"]).max() > 0.05
    off.close()
    for ad in ("adapter", "adapter2"):                    # the second load swaps q_proj's adapter on the live engines
        utils.load_adapters(trad, c[ad])
        utils.load_adapters(perm, c[ad + "_perm"])
        for kvd in ("float32", "model"):
            a, b = _logit_trace(trad.engine, toks, kvd), _logit_trace(perm.engine, toks, kvd)
            assert np.array_equal(a, b), (ad, kvd)
            assert not np.array_equal(a, base[kvd]), (ad, kvd)
            base[kvd] = a
    trad.engine.close(); perm.engine.close()


# ------------------------------------------------------------------------------------------------ errors
def test_a_missing_bias_tensor_fails_finalize_with_its_name(ckpts, tmp_path):
    c = ckpts["bf16"]
    w = load_file(c["perm"] + "/model.safetensors")
    gone = "model.layers.1.mlp.up_proj.bias"
    assert gone in w
    (tmp_path / "m").mkdir()
    save_file({k: v.contiguous() for k, v in w.items() if k != gone}, str(tmp_path / "m" / "model.safetensors"), metadata={"format": "mlx"})
    shutil.copy(c["perm"] + "/config.json", tmp_path / "m" / "config.json")
    with pytest.raises(FileNotFoundError, match=r"model\.layers\.1\.mlp\.up_proj\.bias"):
        utils.load_model(tmp_path / "m", max_positions=MAX_POS)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_bias_fed_to_an_engine_without_the_flag_is_skipped(ckpts, variant, tmp_path):
    """the reference filters unmatched tensors: with attention_bias / mlp_bias off, `.bias` names are unknown (counted as
    skipped) and the logits are those of the unbiased checkpoint bit for bit"""
    c = ckpts[variant]
    w = load_file(c["perm"] + "/model.safetensors")
    cfg = dict(json.loads(open(c["perm"] + "/config.json").read()), attention_bias=False, mlp_bias=False)
    n_bias = sum(k.endswith(".bias") for k in w)
    assert n_bias == 7 * cfg["num_hidden_layers"]
    for name, keep_bias in (("with", True), ("without", False)):
        (tmp_path / name).mkdir()
        save_file({k: v.contiguous() for k, v in w.items() if keep_bias or not k.endswith(".bias")},
                  str(tmp_path / name / "model.safetensors"), metadata={"format": "mlx"})
        (tmp_path / name / "config.json").write_text(json.dumps(cfg))
    eng = Engine(dict(cfg, model_type="llama"), max_positions=MAX_POS, act_dtype="bfloat16")
    assert eng.load_tensors(load_file(str(tmp_path / "with" / "model.safetensors")).items()) == n_bias
    eng.finalize()
    plain = _engine_model(tmp_path / "without")
    toks = _left_pad_prompts(c["cfg"], 3, 9)
    a, b = _logit_trace(eng, toks, "float32", steps=2), _logit_trace(plain.engine, toks, "float32", steps=2)
    assert np.array_equal(a, b)
    biased_model = _engine_model(c["perm"])
    assert np.abs(_logit_trace(biased_model.engine, toks, "float32", steps=2) - a).max() > 0.1
    eng.close(); plain.engine.close(); biased_model.engine.close()


def test_qwen3_with_rope_traditional_is_refused():
    cfg = {"model_type": "qwen3", "hidden_size": 128, "num_hidden_layers": 1, "intermediate_size": 256, "num_attention_heads": 4,
           "num_key_value_heads": 2, "head_dim": 32, "rms_norm_eps": 1e-6, "vocab_size": 128, "rope_traditional": True}
    with pytest.raises(NotImplementedError, match="rope_traditional"):
        Engine(cfg)
    Engine(dict(cfg, rope_traditional=False)).close()
