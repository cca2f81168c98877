"""Models with 3 and 6 query heads per KV head through utils.load_model -> engine -> C ABI (the device tests are marked gpu;
the oracle-side checks of the same fixtures run without a device).

* tests/golden/gqa/gqa_*.npz (tests/golden/gqa/make_golden_gqa.py): tiny llama checkpoints -- hidden 192 with 6 / 2 heads of
  32, hidden 384 with 6 / 2 heads of 64, hidden 768 with 12 / 2 heads of 64; bf16 and int4 g64 with tied embeddings, the
  384-wide one also f16 -- 4 left-padded prompts, 12 greedy steps, both KV modes.  The oracle reproduces the files (CPU) and
  the device matches them under the assertions of tests/test_gpu_golden.py.
* The config.json key set of Llama-3.2-3B-Instruct-4bit, shrunk to 2 layers, hidden 384 and vocabulary 1024: it loads, and
  batch_generate equals the oracle's host loop (tests/test_gpu_generate_api.py).
* On the 384-wide model, in both KV modes: block-paged == contiguous bit for bit, a 40-token prompt entered in 16 / 16 / 8
  token chunks next to two live decode rows, row-subset steps, and consumer_combine on == off.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import ref_generate, ref_model

GQA = Path(__file__).resolve().parent / "golden" / "gqa"
sys.path.insert(0, str(GQA))

import make_golden_gqa as gen  # noqa: E402
import test_golden as cpu_golden  # noqa: E402
import test_gpu_consumer_combine as cc_base  # noqa: E402
import test_gpu_engine as eng_base  # noqa: E402
import test_gpu_generate_api as api_base  # noqa: E402
import test_gpu_golden as gpu_golden  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from mlx_parallm_amd.models.llama import ModelArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402

gpu = pytest.mark.gpu
SMALL = sorted(GQA.glob("gqa_*.npz"))
KVDS = ["model", "float32"]


# ---------------------------------------------------------------------------------------------------------------------------
# committed goldens

def test_gqa_golden_files_present():
    assert {p.stem for p in SMALL} == set(gen.SMALL), "run tests/golden/gqa/make_golden_gqa.py --small"
    for p in SMALL:
        m = json.loads(str(np.load(p)["spec"]))["model"]
        assert m["heads"] // m["kv_heads"] in (3, 6) and m["tie_word_embeddings"]


@pytest.mark.parametrize("path", SMALL, ids=[p.stem for p in SMALL])
def test_oracle_reproduces_gqa_golden(path):
    cpu_golden.test_oracle_reproduces_golden(path)


@gpu
@pytest.mark.parametrize("path", SMALL, ids=[p.stem for p in SMALL])
def test_device_matches_gqa_golden(path):
    """tests/test_gpu_golden.py's assertions: float32-KV ids equal and logprobs within 1e-3, model-KV ids equal wherever the
    oracle's margin exceeds 0.13."""
    gpu_golden.test_device_matches_golden(path)


# ---------------------------------------------------------------------------------------------------------------------------
# the Llama-3.2-3B config.json

# every key of the checkpoint's config.json; the values of the sizes are shrunk below
LLAMA32_CONFIG = {
    "architectures": ["LlamaForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "bos_token_id": 128000,
    "eos_token_id": [128001, 128008, 128009], "head_dim": 128, "hidden_act": "silu", "hidden_size": 3072,
    "initializer_range": 0.02, "intermediate_size": 8192, "max_position_embeddings": 131072, "mlp_bias": False,
    "model_type": "llama", "num_attention_heads": 24, "num_hidden_layers": 28, "num_key_value_heads": 8, "pretraining_tp": 1,
    "quantization": {"group_size": 64, "bits": 4}, "rms_norm_eps": 1e-05,
    "rope_scaling": {"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0, "original_max_position_embeddings": 8192,
                     "rope_type": "llama3"},
    "rope_theta": 500000.0, "tie_word_embeddings": True, "torch_dtype": "bfloat16", "transformers_version": "4.45.0.dev0",
    "use_cache": True, "vocab_size": 128256,
}
SHRUNK = dict(num_hidden_layers=2, hidden_size=384, intermediate_size=1024, num_attention_heads=6, num_key_value_heads=2, head_dim=64,
              vocab_size=1024, bos_token_id=256, eos_token_id=[256])


def _build_llama32(dst):
    """A checkpoint of the shrunk shape whose config.json holds exactly the keys above."""
    c = dict(LLAMA32_CONFIG, **SHRUNK)
    built = build_tiny_model(dst, seed=61, vocab_size=c["vocab_size"], dtype="bfloat16", quantize_model=True, hidden_size=c["hidden_size"],
                             layers=c["num_hidden_layers"], heads=c["num_attention_heads"], kv_heads=c["num_key_value_heads"],
                             intermediate_size=c["intermediate_size"], head_dim=c["head_dim"], tie_word_embeddings=True,
                             rope_theta=c["rope_theta"], rms_norm_eps=c["rms_norm_eps"], norm_jitter=0.1)
    assert all(built[k] == c[k] for k in built if k in c and k not in ("rope_scaling", "max_position_embeddings"))
    (Path(dst) / "config.json").write_text(json.dumps(c, indent=4, sort_keys=True))
    return c


def test_llama32_config_keys_are_accepted_on_both_sides():
    """ModelArgs (the product) and RefConfig (the oracle) take the key set: 3 query heads per KV head, head_dim from the config,
    rope_type "llama3" left unscaled (as the reference leaves it), tied embeddings."""
    c = dict(LLAMA32_CONFIG, **SHRUNK)
    assert set(c) == set(LLAMA32_CONFIG)
    a = ModelArgs.from_dict(c)
    assert a.num_attention_heads // a.num_key_value_heads == 3 and a.tie_word_embeddings
    r = ref_model.RefConfig.from_dict(c)
    assert (r.head_dim, r.rope_scale, r.rope_theta, r.tie_word_embeddings) == (64, 1.0, 500000.0, True)
    full = ModelArgs.from_dict(LLAMA32_CONFIG)
    assert (full.num_attention_heads, full.num_key_value_heads) == (24, 8)


@gpu
@pytest.mark.parametrize("format_prompts", [False, True])
def test_llama32_config_loads_and_batch_generate_equals_the_oracle_host_loop(tmp_path, monkeypatch, format_prompts):
    c = _build_llama32(tmp_path)
    assert set(json.loads((tmp_path / "config.json").read_text())) == set(LLAMA32_CONFIG)
    utils._kv_pool.clear()
    monkeypatch.setattr(utils, "DEFAULT_KV_DTYPE", "float32")      # the reference's pool hands out PagedKVCache
    model, tok = utils.load(str(tmp_path), max_positions=512)
    ref = ref_generate.load(str(tmp_path), max_pos=512)
    try:
        assert model.engine.desc.num_heads // model.engine.desc.num_kv_heads == 3 and model.engine.desc.rope_scale == 1.0
        api_base.test_batch_generate_equals_the_oracle_host_loop((model, tok, ref), format_prompts)
    finally:
        utils._kv_pool.clear()
        model.engine.close()
    assert c["rope_scaling"]["rope_type"] == "llama3"


# ---------------------------------------------------------------------------------------------------------------------------
# the 384-wide model: arena, mixed steps, row subsets, consumer_combine

@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """name -> (checkpoint directory, config) of the 384-wide checkpoints of the goldens, built once."""
    root = tmp_path_factory.mktemp("gqa")
    return {name: (str(root / name), build_tiny_model(root / name, **gen.SMALL_MODELS[name])) for name in ("h384_bf16", "h384_int4")}


def _alone(ref, p, n, paged):
    """The oracle's greedy run of one sequence: -> (tokens, top-2 margins)."""
    cache = ref.make_cache(1, paged=paged)
    y, out, margins = np.asarray(p)[None], [], []
    for _ in range(n):
        lg = ref(y, cache=cache)[:, -1]
        top2 = np.sort(lg[0])[-2:]
        margins.append(float(top2[1] - top2[0]))
        y = np.argmax(lg, axis=-1)[:, None]
        out.append(int(y[0, 0]))
    return out, margins


def _assert_sequences(ref, prompts, got, paged):
    """Every sequence produces what it produces alone; a differing token only at an oracle margin inside the mode's bound (it
    changes the continuation, so the comparison of that sequence ends there)."""
    for nm, p in prompts.items():
        want, margins = _alone(ref, p, len(got[nm]), paged)
        for i, (g, w) in enumerate(zip(got[nm], want)):
            if g != w:
                assert margins[i] <= (2e-3 if paged else 0.13), (nm, i, got[nm], want, margins[i])
                break


@gpu
@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", ["h384_bf16", "h384_int4"])
def test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd):
    eng_base.test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd)


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_chunked_prefill_next_to_two_decode_rows(dirs, kvd):
    """mi_step_enqueue_mixed: a 40-token prompt enters row 0 in chunks of 16 / 16 / 8 tokens while rows 1 and 2 keep decoding in
    the same steps.  Under the rule of tests/test_gpu_engine.py::test_mixed_steps_chunked_prefill_next_to_decode_rows: every
    sequence produces what it produces alone, inner chunks return nothing, and the chunked prompt's cache equals a one-shot
    prefill's -- the logits of the same next token within 4e-3 (float32 KV) / 0.1 (model KV)."""
    model, ref, cfg = eng_base._load_pair(dirs, "h384_bf16")
    eng, paged = model.engine, kvd == "float32"
    rng = np.random.default_rng(23)
    P = {"A": rng.integers(3, cfg["vocab_size"], size=9), "B": rng.integers(3, cfg["vocab_size"], size=6),
         "C": rng.integers(3, cfg["vocab_size"], size=40)}
    kv = eng.new_kv(3, capacity=64, kv_dtype=kvd)
    greedy = SampleArgs(temp=0.0)
    got = {k: [] for k in P}

    def mixed(rows, names, toks, want):
        res = eng.step_wait(eng.step_enqueue_mixed(kv, rows, toks, want, greedy), sum(want))
        for nm, t in zip([n for n, w in zip(names, want) if w], res["tokens"]):
            got[nm].append(int(t))

    mixed([1, 2], ["A", "B"], [P["A"], P["B"]], [1, 1])
    for lo, hi in ((0, 16), (16, 32), (32, 40)):
        mixed([1, 2, 0], ["A", "B", "C"], [[got["A"][-1]], [got["B"][-1]], P["C"][lo:hi]], [1, 1, int(hi == 40)])
        assert kv.offsets == [hi, 9 + len(got["A"]) - 1, 6 + len(got["B"]) - 1] and len(got["C"]) == int(hi == 40)
    # the next decode step of all three rows as a forward call: row 0's logits against a one-shot prefill of the prompt
    kv2 = eng.new_kv(1, capacity=64, kv_dtype=kvd)
    eng.forward(P["C"][None].astype(np.int32), kv2, want_logits=False)
    a = eng.forward(np.asarray([[got["C"][0]]], np.int32), kv2)
    b = eng.forward(np.asarray([[got["C"][-1]], [got["A"][-1]], [got["B"][-1]]], np.int32), kv)
    err = float(np.abs(a.reshape(1, -1) - b.reshape(3, -1)[0:1]).max())
    print(f"chunked 16 / 16 / 8 against one-shot prefill, {kvd} KV: max |logit difference| {err:.3e}")
    assert err <= (4e-3 if paged else 0.1), err
    for nm, t in zip(["C", "A", "B"], np.argmax(b.reshape(3, -1), axis=-1)):
        got[nm].append(int(t))
    for _ in range(2):
        mixed([0, 1, 2], ["C", "A", "B"], [[got["C"][-1]], [got["A"][-1]], [got["B"][-1]]], [1, 1, 1])
    assert kv.offsets == [43, 15, 12]                     # 40 + 3; 9 + 6; 6 + 6: three chunk steps, the forward call, two steps
    _assert_sequences(ref, P, got, paged)
    kv.close(); kv2.close()
    eng.close()


@gpu
@pytest.mark.parametrize("kvd", KVDS)
def test_row_subset_steps_equal_independent_sequences(dirs, kvd):
    """mi_step_enqueue_rows over changing row sets and a recycled slot, as tests/test_gpu_engine.py runs it, in both KV modes."""
    model, ref, cfg = eng_base._load_pair(dirs, "h384_int4")
    eng, paged = model.engine, kvd == "float32"
    rng = np.random.default_rng(29)
    P = {"A": rng.integers(3, cfg["vocab_size"], size=7), "B": rng.integers(3, cfg["vocab_size"], size=5),
         "C": rng.integers(3, cfg["vocab_size"], size=40)}
    kv = eng.new_kv(4, capacity=64, kv_dtype=kvd)
    greedy = SampleArgs(temp=0.0)
    got = {k: [] for k in P}

    def step(rows, names, tokens):
        res = eng.step_wait(eng.step_enqueue_rows(kv, rows, tokens, greedy), len(rows))
        for nm, t in zip(names, res["tokens"]):
            got[nm].append(int(t))

    step([2], ["A"], P["A"][None])
    step([2], ["A"], [[got["A"][-1]]])
    step([0], ["B"], P["B"][None])
    step([2, 0], ["A", "B"], [[got["A"][-1]], [got["B"][-1]]])
    step([2, 0], ["A", "B"], None)                                  # same row set: tokens stay on the device
    step([2, 0], ["A", "B"], None)
    assert kv.offsets == [8, 0, 11, 0]
    kv.reset_row(2)
    step([2], ["C"], P["C"][None])
    step([0, 2], ["B", "C"], [[got["B"][-1]], [got["C"][-1]]])
    step([0, 2], ["B", "C"], None)
    assert kv.offsets == [10, 0, 42, 0]
    _assert_sequences(ref, P, got, paged)
    kv.close()
    eng.close()


@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_consumer_combine_on_equals_off(dirs, paged):
    """Float32-KV decode steps of 8 rows with the engine option consumer_combine on and off: every output of every step equal,
    with no tolerance (the bound of tests/test_gpu_consumer_combine.py)."""
    d, cfg = dirs["h384_bf16"]
    model = utils.load_model(d, max_positions=cc_base.MAX_POS)
    try:
        for L0 in (40, 200):
            base = cc_base._run(model.engine, 0, 8, L0, paged, cfg["vocab_size"])
            cc_base._assert_equal(base, cc_base._run(model.engine, 1, 8, L0, paged, cfg["vocab_size"]), ("gqa", paged, L0))
    finally:
        model.engine.close()
