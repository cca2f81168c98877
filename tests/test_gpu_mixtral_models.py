"""Mixtral checkpoints through utils.load_model -> engine -> C ABI (-m gpu), against the oracle twin of the block
(tests/moe_ref.py; its CPU-side checks are tests/test_mixtral_host.py).

* tests/golden/moe/*.npz under the assertions of tests/test_gpu_golden.py (float32-KV: ids equal, logprobs within 1e-3; model-KV:
  ids equal wherever the oracle's margin exceeds 0.13).  The files' inputs keep the oracle's router away from a tie.
* stacked checkpoint == per-expert checkpoint, block-paged == contiguous: bit for bit.
* chunked prefill next to decode rows and row-subset steps: the bodies of tests/test_gpu_gqa_models.py.
* E = 1, k = 1 against the Llama checkpoint that holds the same MLP; LoRA on q/k/v/o against the twin with the same adapter;
  utils.load + batch_generate against the oracle host loop; one /v1/completions request; the errors of the arch.
"""
import json
import os
import signal
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ref_generate

MOE = Path(__file__).resolve().parent / "golden" / "moe"
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(MOE))

import make_golden_moe as gen  # noqa: E402
import moe_ref  # noqa: E402
import test_gpu_engine as eng_base  # noqa: E402
import test_gpu_generate_api as api_base  # noqa: E402
import test_gpu_golden as gpu_golden  # noqa: E402
import test_gpu_gqa_models as gqa_models  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import Engine, SampleArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = sorted(MOE.glob("*.npz"))
KVDS = ["model", "float32"]


@pytest.fixture(autouse=True)
def _oracle_loads_the_twin(monkeypatch):
    monkeypatch.setattr(ref_generate, "load", moe_ref.load)


def _kw(name, seed, **extra):
    return dict(gen.MODELS[name][0], seed=seed, **extra)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """name -> (checkpoint directory, config): E = 4 in bfloat16 (stacked and per-expert names) and E = 8 in float16."""
    root = tmp_path_factory.mktemp("mixtral")
    out = {"e4_bf16": (str(root / "e4"), build_tiny_model(root / "e4", **_kw("moe_e4k2_bf16", 41))),
           "e4_bf16_per_expert": (str(root / "e4p"), build_tiny_model(root / "e4p", expert_names="per_expert", **_kw("moe_e4k2_bf16", 41))),
           "e8_f16": (str(root / "e8"), build_tiny_model(root / "e8", **_kw("moe_e8k2_f16", 42)))}
    # (the reused bodies name their two checkpoints like this)
    out["h384_bf16"], out["h384_int4"] = out["e4_bf16"], out["e8_f16"]
    return out


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_device_matches_moe_golden(path):
    gpu_golden.test_device_matches_golden(path)


def _steps(eng, kvd, vocab, B=4, L0=10):
    """A prefill + 8 greedy steps, then 6 seeded top-p 0.9 steps: every step's outputs."""
    rng = np.random.default_rng(31)
    kv = eng.new_kv(B, capacity=48, kv_dtype=kvd)
    y = rng.integers(3, vocab, size=(B, L0)).astype(np.int32)
    out = []
    for s in range(15):
        sp = SampleArgs(temp=0.0, top_logprobs=5) if s < 9 else SampleArgs(temp=1.0, top_p=0.9, seed=5, stream_position=s, top_logprobs=5)
        out.append(eng.decode_sample(kv, y, sp))
        y = out[-1]["tokens"][:, None].astype(np.int32)
    kv.close()
    return out


@pytest.mark.parametrize("kvd", KVDS)
def test_stacked_checkpoint_equals_per_expert_checkpoint_bit_for_bit(dirs, kvd):
    a, b = utils.load_model(dirs["e4_bf16"][0], max_positions=256), utils.load_model(dirs["e4_bf16_per_expert"][0], max_positions=256)
    try:
        assert a.engine.desc.arch == 3 and (a.engine.desc.num_local_experts, a.engine.desc.num_experts_per_tok) == (4, 2)
        ra, rb = _steps(a.engine, kvd, 1024), _steps(b.engine, kvd, 1024)
        for s, (x, y) in enumerate(zip(ra, rb)):
            for k in ("tokens", "logprobs", "top_ids", "top_logprobs"):
                assert np.array_equal(x[k], y[k]), (kvd, s, k)
    finally:
        a.engine.close(); b.engine.close()


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", ["e4_bf16", "e8_f16"])
def test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd):
    eng_base.test_paged_kv_is_bit_identical_to_contiguous_kv(dirs, name, kvd)


@pytest.mark.parametrize("kvd", KVDS)
def test_chunked_prefill_next_to_two_decode_rows(dirs, kvd):
    gqa_models.test_chunked_prefill_next_to_two_decode_rows(dirs, kvd)


@pytest.mark.parametrize("kvd", KVDS)
def test_row_subset_steps_equal_independent_sequences(dirs, kvd):
    gqa_models.test_row_subset_steps_equal_independent_sequences(dirs, kvd)


@pytest.mark.parametrize("kvd", KVDS)
def test_score_tokens_matches_the_twin(dirs, kvd):
    """mi_score_tokens (every position through the block and the head in one call) against the twin's log-softmax."""
    model, ref, cfg = eng_base._load_pair(dirs, "e4_bf16")
    rng = np.random.default_rng(5)
    toks = rng.integers(3, cfg["vocab_size"], size=(2, 9)).astype(np.int32)
    kv = model.engine.new_kv(2, capacity=16, kv_dtype=kvd)
    got = model.engine.score_tokens(kv, toks[:, :-1], toks[:, 1:])["logprobs"]
    lg = ref(toks[:, :-1], cache=ref.make_cache(2, paged=kvd == "float32")).astype(np.float64)
    lp = lg - np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True)) - lg.max(-1, keepdims=True)
    want = np.take_along_axis(lp, toks[:, 1:, None].astype(np.int64), axis=-1)[..., 0]
    err = float(np.abs(got - want).max())
    print(f"score_tokens against the twin, {kvd} KV: max |logprob difference| {err:.3e}")
    assert err <= (1e-3 if kvd == "float32" else 0.13), err
    kv.close()
    model.engine.close()


def _llama_twin_of_e1(src, dst):
    """The Llama checkpoint that holds the one expert of an E = 1 Mixtral checkpoint as its dense MLP."""
    from safetensors.torch import load_file, save_file

    dst.mkdir(parents=True, exist_ok=True)
    w = {}
    for k, t in load_file(str(Path(src) / "model.safetensors")).items():
        if ".block_sparse_moe.switch_mlp." in k:
            w[k.replace(".block_sparse_moe.switch_mlp.", ".mlp.")] = t[0].contiguous()
        elif ".block_sparse_moe.gate." not in k:
            w[k] = t
    save_file(w, str(dst / "model.safetensors"), metadata={"format": "mlx"})
    cfg = json.loads((Path(src) / "config.json").read_text())
    cfg = {k: v for k, v in cfg.items() if k not in ("num_local_experts", "num_experts_per_tok")}
    cfg["model_type"] = "llama"
    (dst / "config.json").write_text(json.dumps(cfg, indent=4, sort_keys=True))
    return str(dst)


@pytest.mark.parametrize("kvd", KVDS)
def test_one_expert_is_the_dense_llama_mlp(tmp_path, kvd):
    """E = 1, k = 1: s = 1 and the block is down(T(T(silu(gate xn)) up xn)) -- the Llama checkpoint with that MLP, on the dense
    kernels.  Teacher-forced with the Llama engine's tokens: ids equal, logprobs within the bound tests/test_gpu_golden.py applies
    in the KV mode (1e-3 float32-KV; model-KV: 0.13, an id may differ where the top-2 margin is inside it)."""
    build_tiny_model(tmp_path / "moe", **_kw("moe_e4k1_bf16", 43, num_local_experts=1))
    moe = utils.load_model(str(tmp_path / "moe"), max_positions=128)
    dense = utils.load_model(_llama_twin_of_e1(tmp_path / "moe", tmp_path / "llama"), max_positions=128)
    eps = 1e-3 if kvd == "float32" else 0.13
    try:
        assert (moe.engine.desc.arch, dense.engine.desc.arch) == (3, 0)
        rng = np.random.default_rng(8)
        y = rng.integers(3, 1024, size=(3, 7)).astype(np.int32)
        ka, kb = moe.engine.new_kv(3, capacity=32, kv_dtype=kvd), dense.engine.new_kv(3, capacity=32, kv_dtype=kvd)
        worst = 0.0
        for s in range(8):
            ra = moe.engine.decode_sample(ka, y, SampleArgs(temp=0.0, top_logprobs=2))
            rb = dense.engine.decode_sample(kb, y, SampleArgs(temp=0.0, top_logprobs=2))
            for b in range(3):
                margin = rb["top_logprobs"][b, 0] - rb["top_logprobs"][b, 1]
                if ra["tokens"][b] != rb["tokens"][b]:
                    assert kvd == "model" and margin <= eps, (s, b, margin)
                else:
                    worst = max(worst, abs(float(ra["logprobs"][b] - rb["logprobs"][b])))
            y = rb["tokens"][:, None].astype(np.int32)
        print(f"E = 1 Mixtral against its Llama twin, {kvd} KV: max |logprob difference| {worst:.3e}")
        assert worst <= eps, worst
    finally:
        moe.engine.close(); dense.engine.close()


def _write_adapter(dst, cfg, keys, seed=5, rank=8, scale=4.0):
    from safetensors.torch import save_file

    H, nh, nkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    D = H // nh
    dims = {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D), "self_attn.o_proj": (nh * D, H)}
    w = {}
    for i in range(cfg["num_hidden_layers"]):
        for ki, key in enumerate(keys):
            K, n = dims[key]
            rng = np.random.default_rng([seed, i, ki])
            w[f"model.layers.{i}.{key}.lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32))
            w[f"model.layers.{i}.{key}.lora_b"] = torch.from_numpy((rng.standard_normal((rank, n)) * 0.3).astype(np.float32))
    dst.mkdir(parents=True, exist_ok=True)
    save_file(w, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": cfg["num_hidden_layers"],
        "lora_parameters": {"rank": rank, "scale": scale, "dropout": 0.0, "keys": list(keys)}}))
    return str(dst)


def test_lora_on_the_attention_projections_matches_the_twin(dirs, tmp_path):
    d, cfg = dirs["e4_bf16"]
    keys = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj"]
    ad = _write_adapter(tmp_path / "adapter", cfg, keys)
    model = utils.load_model(d, max_positions=128)
    ref = moe_ref.load(d, adapter_path=ad, max_pos=128)
    try:
        rng = np.random.default_rng(17)
        toks = rng.integers(3, cfg["vocab_size"], size=(2, 8)).astype(np.int32)

        def logits():
            kv = model.engine.new_kv(2, capacity=16, kv_dtype="float32")
            out = model.engine.forward(toks, kv)
            kv.close()
            return out

        base = logits()
        utils.load_adapters(model, ad)
        got = logits()
        want = ref(toks, cache=ref.make_cache(2, paged=True))[:, -1]
        assert np.abs(got - base).max() > 0.05, "the adapter changed nothing"
        # (float32-KV: float32 accumulation noise only, unless a router flips -- the margins say how near one came)
        margin = min(float(np.min(m)) for _l, m, _a in ref.margins)
        err = float(np.abs(got - want).max())
        print(f"LoRA on q/k/v/o against the twin: max |logit difference| {err:.3e}, smallest router margin {margin:.3e}")
        assert margin < 1e-3 or err <= 4e-3, (err, margin)
        for proj in ("block_sparse_moe.gate", "block_sparse_moe.switch_mlp.gate_proj", "block_sparse_moe.experts.0.w1", "mlp.gate_proj"):
            with pytest.raises(NotImplementedError):
                model.engine.set_lora(0, proj, np.zeros((128, 4), np.float32), np.zeros((4, 192), np.float32), 1.0)
    finally:
        model.engine.close()


@pytest.mark.parametrize("format_prompts", [False, True])
def test_mixtral_batch_generate_equals_the_oracle_host_loop(tmp_path, monkeypatch, format_prompts):
    d = str(tmp_path / "tok")
    build_tiny_model(d, **_kw("moe_e4k2_bf16", 44, with_tokenizer=True))
    utils._kv_pool.clear()
    monkeypatch.setattr(utils, "DEFAULT_KV_DTYPE", "float32")      # the reference's pool hands out PagedKVCache
    model, tok = utils.load(d, max_positions=512)
    ref = ref_generate.load(d, max_pos=512)
    try:
        assert model.model_type == "mixtral" and model.head_dim == 32 and model.engine.desc.tie_word_embeddings == 0
        api_base.test_batch_generate_equals_the_oracle_host_loop((model, tok, ref), format_prompts)
    finally:
        utils._kv_pool.clear()
        model.engine.close()


def test_one_completion_through_the_server(tmp_path):
    import requests

    from mlx_parallm_amd.tokenizer_utils import load_tokenizer

    d = str(tmp_path / "served")
    build_tiny_model(d, **_kw("moe_e4k2_bf16", 45, with_tokenizer=True))
    port = api_free_port()
    env = os.environ.copy()
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    log_path = tmp_path / "server.log"
    args = [sys.executable, "-m", "mlx_parallm_amd.cli", "--model-path", d, "--host", "127.0.0.1", "--port", str(port),
            "--max-batch-size", "4", "--batch-timeout", "0.1", "--diverse-mode", "false"]
    with open(log_path, "w", buffering=1) as lf:
        proc = subprocess.Popen(args, cwd=str(ROOT), stdout=lf, stderr=subprocess.STDOUT, text=True, env=env)
    base = f"http://127.0.0.1:{port}"
    try:
        deadline, ok = time.time() + 600, False
        while time.time() < deadline and proc.poll() is None:
            try:
                if requests.get(f"{base}/health", timeout=2).ok:
                    ok = True
                    break
            except Exception:
                time.sleep(0.5)
        assert ok, "server did not come up:\n" + log_path.read_text()[-3000:]
        tok = load_tokenizer(d)
        prompt = "Say hello in one word."
        ids = np.asarray(tok.encode(prompt))[None]
        ref = moe_ref.load(d, max_pos=512)
        want, margins = gqa_models._alone(ref, ids[0], 8, paged=False)
        r = requests.post(f"{base}/v1/completions", json={"model": d, "prompt": prompt, "max_tokens": 8, "temperature": 0.0}, timeout=120)
        assert r.status_code == 200, r.text[:500]
        j = r.json()
        assert j["usage"]["prompt_tokens"] == ids.shape[1] and 1 <= j["usage"]["completion_tokens"] <= 8
        # greedy ids are the twin's up to the first step whose top-2 margin is inside the 16-bit bound (or an eos)
        n = next((i for i, m in enumerate(margins) if m <= 0.13), 8)
        if tok.eos_token_id in want[:n]:
            n = want.index(tok.eos_token_id)
        assert j["choices"][0]["text"].startswith(tok.decode(want[:n], skip_special_tokens=True)), (j["choices"][0]["text"], want, margins)
    finally:
        proc.send_signal(signal.SIGTERM)
        try:
            proc.wait(timeout=20)
        except subprocess.TimeoutExpired:
            proc.kill()


def api_free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return int(s.getsockname()[1])


def test_mixtral_arch_errors(dirs):
    cfg = dict(dirs["e4_bf16"][1])
    bf = torch.bfloat16
    eng = Engine(cfg, max_positions=64)
    try:
        p = "model.layers.0.block_sparse_moe."
        with pytest.raises(FileNotFoundError, match="mlp.gate_proj"):          # the dense names are unknown on this arch
            eng.set_tensor("model.layers.0.mlp.gate_proj.weight", torch.zeros((192, 128), dtype=bf))
        with pytest.raises(ValueError, match="switch_mlp.gate_proj.weight"):
            eng.set_tensor(p + "switch_mlp.gate_proj.weight", torch.zeros((4, 128, 192), dtype=bf))
        with pytest.raises(ValueError, match="switch_mlp.down_proj.weight"):
            eng.set_tensor(p + "switch_mlp.down_proj.weight", torch.zeros((128, 192), dtype=bf))
        with pytest.raises(ValueError, match="experts.1.w2.weight"):
            eng.set_tensor(p + "experts.1.w2.weight", torch.zeros((192, 128), dtype=bf))
        with pytest.raises(ValueError, match="gate.weight"):
            eng.set_tensor(p + "gate.weight", torch.zeros((8, 128), dtype=bf))
        with pytest.raises(FileNotFoundError, match="experts.4.w1"):
            eng.set_tensor(p + "experts.4.w1.weight", torch.zeros((192, 128), dtype=bf))
        with pytest.raises(NotImplementedError, match="dtype"):
            eng.set_tensor(p + "experts.0.w1.weight", torch.zeros((192, 128), dtype=torch.float16))
        with pytest.raises(NotImplementedError, match="quantised"):
            eng.set_tensor(p + "switch_mlp.gate_proj.scales", torch.zeros((4, 192, 2), dtype=bf))
        # every tensor but expert 2's up matrix of block 1: finalize names the slot
        from safetensors.torch import load_file

        from mlx_parallm_amd import tiny_model

        w = tiny_model.unstack_experts(load_file(str(Path(dirs["e4_bf16"][0]) / "model.safetensors")))
        missing = "model.layers.1.block_sparse_moe.experts.2.w3.weight"
        eng.load_tensors([(k, t) for k, t in w.items() if k != missing], strict=True)
        with pytest.raises(FileNotFoundError, match=r"layers\.1\.block_sparse_moe.*experts\.2\.w3"):
            eng.finalize()
        eng.set_tensor(missing, w[missing])
        eng.finalize()
    finally:
        eng.close()
    with pytest.raises(NotImplementedError, match="quantization"):
        Engine(dict(cfg, quantization={"group_size": 64, "bits": 4}), max_positions=64)
    for flag in ("attention_bias", "mlp_bias", "tie_word_embeddings"):
        with pytest.raises(ValueError, match="mixtral"):
            Engine(dict(cfg, **{flag: True}), max_positions=64)
    for over, word in ((dict(num_local_experts=17), "num_local_experts"), (dict(num_experts_per_tok=3), "num_experts_per_tok"),
                       (dict(intermediate_size=160), "intermediate_size")):
        with pytest.raises(NotImplementedError, match=word):
            Engine(dict(cfg, **over), max_positions=64)
    with pytest.raises(NotImplementedError, match="act_dtype"):
        Engine(cfg, max_positions=64, act_dtype="float32")
    ignored = Engine(dict(cfg, rope_scaling={"type": "linear", "factor": 4.0}, head_dim=64), max_positions=64)   # mixtral.py:38,57-61
    assert ignored.desc.rope_scale == 1.0 and ignored.desc.head_dim == 32
    ignored.close()
