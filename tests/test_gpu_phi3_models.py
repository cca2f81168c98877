"""Phi-3 checkpoints (fused qkv_proj / gate_up_proj, head_dim 96) through utils.load_model -> engine -> C ABI (the device tests
are marked gpu; the oracle-side checks of the same fixtures run without a device).

The oracle has no Phi-3 loader and needs none: a Phi-3 checkpoint with its two fused matrices split is a Llama checkpoint.
Wherever a test below hands one directory to both sides, the device loads the Phi-3 form and the oracle its Llama-form twin
("<directory>-llama", the same tensors of the same seed).

* tests/golden/d96/*.npz (tests/golden/d96/make_golden_d96.py): 4 / 4 and 8 / 8 heads of 96 as Phi-3 checkpoints, 4 / 2 and
  4 / 1 heads of 96 as Llama checkpoints with head_dim 96; the oracle reproduces the files, the device matches them under the
  assertions of tests/test_gpu_golden.py.
* fused == split: the Phi-3-form and the Llama-form engine of one seed give equal tokens and bit-equal logprobs; LoRA on the
  fused names equals the column-sliced adapters on the split names, hot-swap included.
* On the 384-wide Phi-3 model, in both KV modes: block-paged == contiguous, chunked prefill next to decode rows, row-subset
  steps, consumer_combine on == off, fused against unfused decode attention.
* batch_generate, convert, and the errors of the new arch.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import ref_generate

D96 = Path(__file__).resolve().parent / "golden" / "d96"
sys.path.insert(0, str(D96))

import make_golden_d96 as gen  # noqa: E402
import test_golden as cpu_golden  # noqa: E402
import test_gpu_consumer_combine as cc_base  # noqa: E402
import test_gpu_engine as eng_base  # noqa: E402
import test_gpu_generate_api as api_base  # noqa: E402
import test_gpu_golden as gpu_golden  # noqa: E402
import test_gpu_gqa_models as gqa_models  # noqa: E402
from mlx_parallm_amd import tiny_model, utils  # noqa: E402
from mlx_parallm_amd.engine import Engine, SampleArgs  # noqa: E402
from mlx_parallm_amd.models.phi3 import ModelArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402

gpu = pytest.mark.gpu
SMALL = sorted(p for p in D96.glob("*.npz") if not p.stem.startswith("wide_"))
KVDS = ["model", "float32"]


@pytest.fixture(autouse=True)
def _oracle_reads_the_llama_twin(monkeypatch):
    real = ref_generate.load

    def load(path, *a, **kw):
        twin = Path(str(path) + "-llama")
        return real(str(twin) if twin.exists() else path, *a, **kw)

    monkeypatch.setattr(ref_generate, "load", load)


def _build_both(root, name, **extra):
    """The Phi-3 form at root/name and its Llama-form twin at root/name-llama: -> (directory, Phi-3 config)."""
    kw = dict(gen.SMALL_MODELS[name], **extra)
    build_tiny_model(root / f"{name}-llama", **kw)
    return str(root / name), build_tiny_model(root / name, **gen.phi3_kwargs(kw))


# ---------------------------------------------------------------------------------------------------------------------------
# committed goldens, configs, the checkpoint builder (no device)

def test_d96_golden_files_present():
    assert {p.stem for p in SMALL} == set(gen.SMALL), "run tests/golden/d96/make_golden_d96.py --small"
    for p in SMALL:
        m = json.loads(str(np.load(p)["spec"]))["model"]
        assert m["head_dim"] == 96 and m["heads"] // m["kv_heads"] in (1, 2, 4) and not m["tie_word_embeddings"]
        assert p.stem.startswith("d96_") or m["hidden_size"] // m["heads"] == 96


@pytest.mark.parametrize("path", SMALL, ids=[p.stem for p in SMALL])
def test_oracle_reproduces_d96_golden(path):
    cpu_golden.test_oracle_reproduces_golden(path)


# every key of Phi-3-mini-4k-instruct's config.json; the values of the sizes are shrunk below
PHI3_CONFIG = {
    "_name_or_path": "Phi-3-mini-4k-instruct", "architectures": ["Phi3ForCausalLM"], "attention_bias": False, "attention_dropout": 0.0,
    "auto_map": {"AutoConfig": "configuration_phi3.Phi3Config", "AutoModelForCausalLM": "modeling_phi3.Phi3ForCausalLM"},
    "bos_token_id": 1, "embd_pdrop": 0.0, "eos_token_id": 32000, "hidden_act": "silu", "hidden_size": 3072,
    "initializer_range": 0.02, "intermediate_size": 8192, "max_position_embeddings": 4096, "model_type": "phi3",
    "num_attention_heads": 32, "num_hidden_layers": 32, "num_key_value_heads": 32, "original_max_position_embeddings": 4096,
    "pad_token_id": 32000, "resid_pdrop": 0.0, "rms_norm_eps": 1e-05, "rope_scaling": None, "rope_theta": 10000.0,
    "sliding_window": 2047, "tie_word_embeddings": False, "torch_dtype": "bfloat16", "transformers_version": "4.40.2",
    "use_cache": True, "vocab_size": 32064, "quantization": {"group_size": 64, "bits": 4},
}
SHRUNK = dict(num_hidden_layers=2, hidden_size=384, intermediate_size=768, num_attention_heads=4, num_key_value_heads=4,
              vocab_size=1024, bos_token_id=256, eos_token_id=256, pad_token_id=256)


def test_phi3_config_keys_are_accepted():
    a = ModelArgs.from_dict(dict(PHI3_CONFIG, **SHRUNK))
    assert (a.hidden_size // a.num_attention_heads, a.num_key_value_heads, a.rope_scaling) == (96, 4, None)
    full = ModelArgs.from_dict(PHI3_CONFIG)
    assert (full.num_attention_heads, full.num_key_value_heads, full.hidden_size // full.num_attention_heads) == (32, 32, 96)
    c = {k: v for k, v in PHI3_CONFIG.items() if k != "num_key_value_heads"}
    assert ModelArgs.from_dict(c).num_key_value_heads == 32                    # phi3.py:28-29
    model_cls, args_cls = utils._get_classes(PHI3_CONFIG)
    assert args_cls is ModelArgs and model_cls._ARCH == "phi3"


def test_rope_scaling_su_refused_linear_served_unknown_dropped(capsys):
    su = dict(PHI3_CONFIG, rope_scaling={"type": "su", "short_factor": [1.0] * 48, "long_factor": [1.0] * 48})
    with pytest.raises(NotImplementedError, match="su"):
        ModelArgs.from_dict(su)
    with pytest.raises(ValueError, match="long_factor"):                       # phi3.py:32-34
        ModelArgs.from_dict(dict(PHI3_CONFIG, rope_scaling={"type": "linear", "factor": 2.0}))
    lin = ModelArgs.from_dict(dict(PHI3_CONFIG, rope_scaling={"type": "linear", "factor": 4.0, "long_factor": [1.0]}))
    assert lin.rope_scaling["type"] == "linear"
    capsys.readouterr()
    other = ModelArgs.from_dict(dict(PHI3_CONFIG, rope_scaling={"type": "yarn", "long_factor": [1.0]}))
    assert other.rope_scaling is None and "[WARNING] rope_scaling 'type' currently only supports" in capsys.readouterr().out


@pytest.mark.parametrize("name", ["phi3_h384_bf16", "phi3_h384_int4"])
def test_tiny_phi3_checkpoint_holds_the_llama_numbers(tmp_path, name):
    import torch
    from safetensors.torch import load_file

    d, cfg = _build_both(tmp_path, name)
    assert cfg["model_type"] == "phi3" and "head_dim" not in cfg and "tie_word_embeddings" not in cfg and "attention_bias" not in cfg
    assert cfg == json.loads((Path(d) / "config.json").read_text())
    fused, split = load_file(str(Path(d) / "model.safetensors")), load_file(str(tmp_path / f"{name}-llama" / "model.safetensors"))
    assert any("qkv_proj" in k for k in fused) and not any("q_proj" in k or "gate_proj" in k or ".up_proj" in k for k in fused)
    assert fused["model.layers.0.self_attn.qkv_proj.weight"].shape[0] == 3 * 384
    back = tiny_model.split_phi3(fused, cfg)
    assert set(back) == set(split) and all(torch.equal(back[k], split[k]) for k in split)
    with pytest.raises(ValueError):
        build_tiny_model(tmp_path / "tied", model_type="phi3", tie_word_embeddings=True, with_tokenizer=False, vocab_size=1024)


# ---------------------------------------------------------------------------------------------------------------------------
# device against golden

@gpu
@pytest.mark.parametrize("path", SMALL, ids=[p.stem for p in SMALL])
def test_device_matches_d96_golden(path, monkeypatch):
    """tests/test_gpu_golden.py's assertions: float32-KV ids equal and logprobs within 1e-3, model-KV ids equal wherever the
    oracle's margin exceeds 0.13.  The phi3_* files load from the fused Phi-3-form checkpoint, the d96_* ones from the Llama form."""
    if path.stem.startswith("phi3_"):
        monkeypatch.setattr(gpu_golden, "build_tiny_model", lambda d, **kw: build_tiny_model(d, **gen.phi3_kwargs(kw)))
    gpu_golden.test_device_matches_golden(path)


# ---------------------------------------------------------------------------------------------------------------------------
# the 384-wide models: fused == split, LoRA, arena, mixed steps, row subsets, consumer_combine, unfused attention

@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """name -> (Phi-3 checkpoint directory, config) of the 384-wide checkpoints of the goldens, built once with their twins."""
    root = tmp_path_factory.mktemp("phi3")
    return {name: _build_both(root, name) for name in ("phi3_h384_bf16", "phi3_h384_int4")}


def _steps(eng, kvd, vocab):
    """A 10-token prefill + 12 greedy steps, then 12 seeded top-p 0.9 steps: every step's outputs."""
    rng = np.random.default_rng(31)
    kv = eng.new_kv(4, capacity=48, kv_dtype=kvd)
    y = rng.integers(3, vocab, size=(4, 10)).astype(np.int32)
    out = []
    for s in range(25):
        sp = SampleArgs(temp=0.0, top_logprobs=5) if s < 13 else SampleArgs(temp=1.0, top_p=0.9, seed=5, stream_position=s, top_logprobs=5)
        out.append(eng.decode_sample(kv, y, sp))
        y = out[-1]["tokens"][:, None].astype(np.int32)
    kv.close()
    return out


def _assert_same_steps(a, b, what):
    for s, (ra, rb) in enumerate(zip(a, b)):
        for k in ("tokens", "logprobs", "top_ids", "top_logprobs"):
            assert np.array_equal(ra[k], rb[k]), (what, s, k)


@gpu
@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", ["phi3_h384_bf16", "phi3_h384_int4"])
def test_fused_checkpoint_equals_split_checkpoint_bit_for_bit(dirs, name, kvd):
    d, cfg = dirs[name]
    fused, split = utils.load_model(d, max_positions=256), utils.load_model(d + "-llama", max_positions=256)
    try:
        assert fused.engine.desc.arch == 2 and split.engine.desc.arch == 0 and fused.engine.desc.head_dim == split.engine.desc.head_dim == 96
        _assert_same_steps(_steps(fused.engine, kvd, cfg["vocab_size"]), _steps(split.engine, kvd, cfg["vocab_size"]), (name, kvd))
    finally:
        fused.engine.close(); split.engine.close()


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_lora_on_the_fused_names_equals_column_slices_on_the_split_names(dirs, kvd):
    """A rank-8 adapter on self_attn.qkv_proj + mlp.gate_up_proj + o_proj + down_proj of the last block of the Phi-3 engine
    against the column-sliced adapters on the Llama-form engine: every output bit-equal, also after a hot-swap to a second one."""
    d, cfg = dirs["phi3_h384_bf16"]
    H, I, rank, last = cfg["hidden_size"], cfg["intermediate_size"], 8, cfg["num_hidden_layers"] - 1
    fused, split = utils.load_model(d, max_positions=256), utils.load_model(d + "-llama", max_positions=256)
    rng = np.random.default_rng(13)
    try:
        base = _steps(fused.engine, kvd, cfg["vocab_size"])
        prev = base
        for swap in range(2):
            for proj, K, parts in (("self_attn.qkv_proj", H, (("self_attn.q_proj", H), ("self_attn.k_proj", H), ("self_attn.v_proj", H))),
                                   ("mlp.gate_up_proj", H, (("mlp.gate_proj", I), ("mlp.up_proj", I))),
                                   ("self_attn.o_proj", H, (("self_attn.o_proj", H),)), ("mlp.down_proj", I, (("mlp.down_proj", H),))):
                N = sum(n for _, n in parts)
                a = (rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32)
                b = (rng.standard_normal((rank, N)) * 0.3).astype(np.float32)
                fused.engine.set_lora(last, proj, a, b, 4.0)
                c0 = 0
                for nm, n in parts:
                    split.engine.set_lora(last, nm, a, np.ascontiguousarray(b[:, c0:c0 + n]), 4.0)
                    c0 += n
            got = _steps(fused.engine, kvd, cfg["vocab_size"])
            _assert_same_steps(got, _steps(split.engine, kvd, cfg["vocab_size"]), ("lora", kvd, swap))
            assert any(not np.array_equal(x["logprobs"], y["logprobs"]) for x, y in zip(got, prev)), "the adapter changed nothing"
            prev = got
        with pytest.raises(NotImplementedError):
            fused.engine.set_lora(last, "self_attn.q_proj", np.zeros((H, rank), np.float32), np.zeros((rank, H), np.float32), 1.0)
    finally:
        fused.engine.close(); split.engine.close()


@gpu
@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", ["phi3_h384_bf16", "phi3_h384_int4"])
def test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd):
    eng_base.test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd)


def _as_gqa(dirs):
    return {"h384_bf16": dirs["phi3_h384_bf16"], "h384_int4": dirs["phi3_h384_int4"]}


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_chunked_prefill_next_to_two_decode_rows(dirs, kvd):
    gqa_models.test_chunked_prefill_next_to_two_decode_rows(_as_gqa(dirs), kvd)


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_row_subset_steps_equal_independent_sequences(dirs, kvd):
    gqa_models.test_row_subset_steps_equal_independent_sequences(_as_gqa(dirs), kvd)


@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_consumer_combine_on_equals_off(dirs, paged):
    """At head_dim 96 the engine routes such steps as with consumer_combine = 0 (the q|k|v linear gets no offer): on == off."""
    gqa_models.test_consumer_combine_on_equals_off(_as_gqa(dirs), paged)


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_fused_and_unfused_decode_attention_agree(dirs, kvd):
    """tests/test_gpu_engine.py::test_fused_and_unfused_decode_attention_agree (its shapes, its 0.08 for a 16-bit model) in both
    KV modes: the one-launch decode attention against rope_append + attn_kernel + attn_combine_kernel at head_dim 96."""
    model, ref, cfg = eng_base._load_pair(dirs, "phi3_h384_bf16")
    B, L0 = 2, 200
    toks = eng_base._left_pad_prompts(cfg, B, L0, ragged=False)
    outs = []
    for fused in (1, 0):
        model.engine.set_option("fused_decode_attention", fused)
        kv = model.engine.new_kv(B, capacity=256, kv_dtype=kvd)
        model.engine.forward(toks, kv, want_logits=False)
        y, steps = toks[:, -1:], []
        for _ in range(4):
            lg = model.engine.forward(y, kv)
            steps.append(lg)
            y = np.argmax(lg, axis=-1)[:, None].astype(np.int32)
        outs.append(np.stack(steps))
        kv.close()
    print(f"fused against unfused decode attention, {kvd} KV: max |logit difference| {np.abs(outs[0] - outs[1]).max():.3e}")
    assert np.abs(outs[0] - outs[1]).max() <= 0.08, np.abs(outs[0] - outs[1]).max()
    cache = ref.make_cache(B, paged=kvd == "float32")
    ref(toks, cache=cache)
    want = ref(toks[:, -1:], cache=cache)[:, -1]
    assert np.abs(outs[0][0] - want).max() <= 0.08
    model.engine.close()


# ---------------------------------------------------------------------------------------------------------------------------
# API, conversion, errors

@gpu
@pytest.mark.parametrize("format_prompts", [False, True])
def test_phi3_batch_generate_equals_the_oracle_host_loop(tmp_path, monkeypatch, format_prompts):
    d, cfg = _build_both(tmp_path, "phi3_h384_int4", with_tokenizer=True)
    utils._kv_pool.clear()
    monkeypatch.setattr(utils, "DEFAULT_KV_DTYPE", "float32")      # the reference's pool hands out PagedKVCache
    model, tok = utils.load(d, max_positions=512)
    ref = ref_generate.load(d, max_pos=512)
    try:
        assert model.model_type == "phi3" and model.head_dim == 96 and model.engine.desc.tie_word_embeddings == 0
        api_base.test_batch_generate_equals_the_oracle_host_loop((model, tok, ref), format_prompts)
    finally:
        utils._kv_pool.clear()
        model.engine.close()


@gpu
def test_converted_phi3_checkpoint_loads_and_matches_the_oracle(tmp_path):
    """convert(quantize=True) is name-agnostic: the fused matrices are quantised like any other linear (groups run along K, so
    quantising the stacked rows is stacking the quantised rows), and the result matches the oracle on the converted twin."""
    from mlx_parallm_amd import convert as cv

    d, cfg = _build_both(tmp_path, "phi3_h384_bf16")
    cv.convert(d, str(tmp_path / "q4"), quantize=True, q_group_size=64, q_bits=4, dtype="bfloat16")
    cv.convert(d + "-llama", str(tmp_path / "q4-llama"), quantize=True, q_group_size=64, q_bits=4, dtype="bfloat16")
    conv = json.loads((tmp_path / "q4" / "config.json").read_text())
    assert conv["model_type"] == "phi3" and conv["quantization"] == {"group_size": 64, "bits": 4}
    model = utils.load_model(str(tmp_path / "q4"), max_positions=256)
    ref = ref_generate.load(str(tmp_path / "q4"), max_pos=256)
    toks = eng_base._left_pad_prompts(cfg, 2, 7)
    kv = model.engine.new_kv(2, capacity=16, kv_dtype="model")
    got = model.engine.forward(toks, kv)
    want = ref(toks, cache=ref.make_cache(2, paged=False))[:, -1]
    assert model.engine.desc.quant_bits == 4 and np.abs(got - want).max() <= 0.08, np.abs(got - want).max()
    kv.close()
    model.engine.close()


@gpu
def test_phi3_arch_errors():
    import torch

    cfg = dict(PHI3_CONFIG, **SHRUNK)
    cfg.pop("quantization")
    eng = Engine(cfg, max_positions=64)
    try:
        w = torch.zeros((384, 384), dtype=torch.bfloat16)
        with pytest.raises(FileNotFoundError, match="q_proj"):               # the split names are unknown on this arch
            eng.set_tensor("model.layers.0.self_attn.q_proj.weight", w)
        with pytest.raises(FileNotFoundError, match="gate_proj"):
            eng.set_tensor("model.layers.0.mlp.gate_proj.weight", torch.zeros((768, 384), dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="qkv_proj.weight"):             # 3 x 384 rows are wanted
            eng.set_tensor("model.layers.0.self_attn.qkv_proj.weight", w)
        with pytest.raises(ValueError, match="gate_up_proj.weight"):
            eng.set_tensor("model.layers.0.mlp.gate_up_proj.weight", torch.zeros((768, 384), dtype=torch.bfloat16))
        eng.set_tensor("model.layers.0.self_attn.qkv_proj.weight", torch.zeros((3 * 384, 384), dtype=torch.bfloat16))
    finally:
        eng.close()
    for flag in ("attention_bias", "mlp_bias", "tie_word_embeddings"):
        with pytest.raises(ValueError, match="phi3"):
            Engine(dict(cfg, **{flag: True}), max_positions=64)
    with pytest.raises(NotImplementedError, match="su"):
        Engine(dict(cfg, rope_scaling={"type": "su", "short_factor": [1.0] * 48, "long_factor": [1.0] * 48}), max_positions=64)
    lin = Engine(dict(cfg, rope_scaling={"type": "linear", "factor": 4.0, "long_factor": [1.0]}), max_positions=64)
    assert lin.desc.rope_scale == 0.25 and lin.desc.head_dim == 96
    lin.close()
    ignored = Engine(dict(cfg, head_dim=128), max_positions=64)               # the reference ignores a head_dim key (phi3.py:53)
    assert ignored.desc.head_dim == 96
    ignored.close()
