"""Adapters merged into the base weights, end to end (-m gpu), against the oracle-side twin tests/merge_ref.py: tiny
checkpoints, both KV modes, the assertions of tests/test_gpu_golden.py -- teacher-forced on the twin's greedy tokens, the
device's token is the twin's unless the twin's top-2 margin is inside the mode's bound (1e-3 float32-KV, 0.13 model-KV;
counted, must stay rare), chosen-token logprobs within 1e-3 (float32-KV) / 0.13 where the margin clears it (model-KV).

* merge at load (``utils.load(..., merge_adapter=True)``) against ``merge_ref.load``: Llama bf16 with q/v and with all seven
  projections, f16, int4 and int8 bases (re-quantised), attention_bias, rope_traditional, Phi-3's fused projections, Mixtral's
  attention projections, one DoRA adapter; the merged outputs differ from the base model's; the merged engine launches no
  adapter kernel (profile family ``lora_rows``, which the same adapter loaded beside the weights does launch).
* the merge tool's output directory, loaded plainly, equals merge-at-load bit for bit over the 15 steps of
  ``test_gpu_mixtral_models._steps``; ``--de-quantize`` gives a dense checkpoint that matches its twin.
* a merged model refuses further adapters (ValueError), an expert key is NotImplementedError, and one ``/v1/completions``
  request against a server started with ``--lora-path ... --merge-lora`` follows the twin."""
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
from safetensors.torch import load_file, save_file

import merge_cases as mc
import merge_ref
from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden" / "d96"))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden" / "moe"))

from mlx_parallm_amd import utils, weight_updater  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from mlx_parallm_amd.tools import merge_lora as tool  # noqa: E402

MAX_POS = 128
MODES = ["float32", "model"]
QV = ("self_attn.q_proj", "self_attn.v_proj")
ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
PHI3 = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")
SMALL = dict(vocab_size=512, dtype="bfloat16", quantize_model=False, hidden_size=128, layers=2, heads=4, kv_heads=2,
             intermediate_size=256, head_dim=32, tie_word_embeddings=False, norm_jitter=0.1)


def _dims(cfg):
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D = cfg.get("head_dim") or H // nh
    inter = cfg["intermediate_size"]
    return {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, inter), "mlp.up_proj": (H, inter), "mlp.down_proj": (inter, H),
            "self_attn.qkv_proj": (H, (nh + 2 * nkv) * D), "mlp.gate_up_proj": (H, 2 * inter)}


def write_adapter(dst, model_dir, cfg, keys, *, kind="lora", rank=8, scale=10.0, n_layers=None, seed=5):
    """A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2) on ``keys`` of the last ``n_layers`` blocks; DoRA: m = ||W|| (1 + 0.2 noise)."""
    dst = Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    nl = cfg["num_hidden_layers"]
    n_layers = n_layers or nl
    base = ref_generate.load_weights(model_dir, cfg) if kind == "dora" else None
    t = {}
    for i in range(nl - n_layers, nl):
        for ki, key in enumerate(keys):
            K, n = _dims(cfg)[key]
            rng = np.random.default_rng([seed, i, ki])
            name = f"model.layers.{i}.{key}"
            t[name + ".lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32))
            t[name + ".lora_b"] = torch.from_numpy((rng.standard_normal((rank, n)) * 0.05).astype(np.float32))
            if kind == "dora":
                norm = np.sqrt((base[name].weight.astype(np.float64) ** 2).sum(axis=1))
                t[name + ".m"] = torch.from_numpy((norm * (1.0 + 0.2 * rng.standard_normal(n))).astype(np.float32))
    save_file(t, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({"fine_tune_type": kind, "num_layers": n_layers, "lora_parameters": {
        "rank": rank, "scale": scale, "dropout": 0.0, "keys": list(keys)}}))
    return str(dst)


def against_twin(eng, ref, vocab, mode, what, B=2, L0=7, steps=4, router=False):
    """the assertions of test_gpu_golden.test_device_matches_golden, the twin computed here -> the device's first logits"""
    paged = mode == "float32"
    eps = 1e-3 if paged else 0.13
    y = np.random.default_rng([11, B, L0]).integers(3, vocab, size=(B, L0)).astype(np.int32)
    cache = ref.make_cache(B, paged=paged)
    kv = eng.new_kv(B, capacity=L0 + steps + 1, kv_dtype=mode)
    near, min_margin, lp_err = 0, np.inf, 0.0
    for _s in range(steps):
        lg = ref(y, cache=cache)[:, -1]
        ws = ref_sample.sample(lg, temp=0.0)
        res = eng.decode_sample(kv, y, SampleArgs(temp=0.0))
        top2 = np.sort(lg, axis=-1)[:, -2:]
        margins = top2[:, 1] - top2[:, 0]
        min_margin = min(min_margin, float(margins.min()))
        flipped = router and min(float(np.min(m)) for _l, m, _a in ref.margins) < 1e-3    # (a router within 1e-3 of a flip voids the step)
        for b in range(B):
            want = int(ws["tokens"][b, 0])
            if int(res["tokens"][b]) != want:
                assert margins[b] <= eps or flipped, (what, mode, b, float(margins[b]))
                near += 1
            elif (paged or margins[b] >= eps) and not flipped:
                e = abs(float(res["logprobs"][b]) - float(ws["logprobs"].reshape(-1)[b]))
                lp_err = max(lp_err, e)
                assert e <= eps, (what, mode, b, e)
        y = ws["tokens"].reshape(B, 1).astype(np.int32)
    kv.close()
    total = steps * B
    print(f"{what} {mode}: tokens off {near} of {total}, max |logprob - twin| {lp_err:.3e}, smallest twin margin {min_margin:.3e}")
    assert near <= (0 if paged and min_margin > eps and not router else max(1, total // 10)), (what, near, total)


def first_logits(eng, vocab, mode="float32", B=2, L0=7):
    y = np.random.default_rng([11, B, L0]).integers(3, vocab, size=(B, L0)).astype(np.int32)
    kv = eng.new_kv(B, capacity=L0 + 1, kv_dtype=mode)
    out = eng.forward(y, kv).copy()
    kv.close()
    return out


def launches(eng, family, vocab):
    eng.profile_select(family)
    first_logits(eng, vocab)
    n, _ms = eng.profile_read()
    eng.profile_select(None)
    return n


def merged_against_twin(model_dir, cfg, adapter, mode, what, ref=None, router=False, tokenizer=True):
    ref = ref or merge_ref.load(model_dir, adapter_path=adapter, max_pos=MAX_POS)
    if tokenizer:
        model, _tok = utils.load(model_dir, adapter_path=adapter, merge_adapter=True, max_positions=MAX_POS)
    else:                                                  # (a checkpoint directory without tokenizer files)
        model = utils.load_model(model_dir, adapter_path=adapter, merge_adapter=True, max_positions=MAX_POS)
    try:
        assert model.merged_adapter == adapter
        against_twin(model.engine, ref, cfg["vocab_size"], mode, what, router=router)
        merged = first_logits(model.engine, cfg["vocab_size"])
        assert launches(model.engine, "lora_rows", cfg["vocab_size"]) == 0
    finally:
        model.engine.close()
    base = utils.load_model(model_dir, max_positions=MAX_POS)
    try:
        assert float(np.abs(first_logits(base.engine, cfg["vocab_size"]) - merged).max()) >= 0.05, "the adapter changed nothing"
    finally:
        base.engine.close()


# ------------------------------------------------------------------------------------------------ 1. merge at load
# name -> (tiny_dirs checkpoint, keys, kind, adapted blocks)
TINY_CASES = {"llama_bf16_qv": ("llama_bf16_gqa", QV, "lora", 2), "llama_bf16_all": ("llama_bf16_gqa", ALL, "lora", 3),
              "llama_f16_all": ("llama_f16", ALL, "lora", 2), "llama_q4_bf16": ("llama_q4_bf16", ALL, "lora", 2),
              "llama_q8_f16": ("llama_q8_f16", ALL, "lora", 1), "qwen3_bf16_dora": ("qwen3_bf16", ALL, "dora", 2)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(TINY_CASES))
def test_merge_at_load_matches_the_twin(tiny_dirs, tmp_path, case, mode):
    name, keys, kind, n_layers = TINY_CASES[case]
    d, cfg = tiny_dirs[name]
    ad = write_adapter(tmp_path / "ad", d, cfg, keys, kind=kind, n_layers=n_layers)
    merged_against_twin(d, cfg, ad, mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flag", ["attention_bias", "rope_traditional"])
def test_merge_at_load_biased_and_traditional_rope(tmp_path, flag, mode):
    extra = dict(attention_bias=True, mlp_bias=True) if flag == "attention_bias" else dict(rope_traditional=True)
    cfg = build_tiny_model(tmp_path / "m", seed=12, **SMALL, **extra)
    ad = write_adapter(tmp_path / "ad", str(tmp_path / "m"), cfg, ALL, kind="dora" if flag == "attention_bias" else "lora")
    merged_against_twin(str(tmp_path / "m"), cfg, ad, mode, flag)          # (a DoRA merge is allowed on a biased projection)


@pytest.mark.parametrize("mode", MODES)
def test_merge_at_load_phi3_fused_projections(tmp_path, mode):
    import make_golden_d96 as gen

    kw = dict(gen.SMALL_MODELS["phi3_h384_bf16"])
    build_tiny_model(tmp_path / "split", **kw)
    cfg = build_tiny_model(tmp_path / "fused", **gen.phi3_kwargs(kw))
    ad = write_adapter(tmp_path / "ad", str(tmp_path / "fused"), cfg, PHI3)
    split_cfg = json.loads((tmp_path / "split" / "config.json").read_text())
    ref = merge_ref.load(str(tmp_path / "split"), adapter_path=merge_ref.split_phi3_adapter(ad, str(tmp_path / "ad_split"), split_cfg),
                         max_pos=MAX_POS)
    merged_against_twin(str(tmp_path / "fused"), cfg, ad, mode, "phi3", ref=ref, tokenizer=False)


@pytest.mark.parametrize("mode", MODES)
def test_merge_at_load_mixtral_attention(tmp_path, mode):
    import make_golden_moe as gen

    cfg = build_tiny_model(tmp_path / "e4", **dict(gen.MODELS["moe_e4k2_bf16"][0], seed=41))
    ad = write_adapter(tmp_path / "ad", str(tmp_path / "e4"), cfg, ALL[:4])
    merged_against_twin(str(tmp_path / "e4"), cfg, ad, mode, "mixtral", router=True, tokenizer=False)
    bad = write_adapter(tmp_path / "bad", str(tmp_path / "e4"), dict(cfg), ALL[:1])
    t = load_file(bad + "/adapters.safetensors")
    H, inter = cfg["hidden_size"], cfg["intermediate_size"]
    t["model.layers.0.block_sparse_moe.switch_mlp.gate_proj.lora_a"] = torch.zeros(H, 4)
    t["model.layers.0.block_sparse_moe.switch_mlp.gate_proj.lora_b"] = torch.zeros(4, inter)
    save_file(t, bad + "/adapters.safetensors")
    acfg = json.loads(Path(bad, "adapter_config.json").read_text())
    acfg["lora_parameters"]["keys"].append("block_sparse_moe.switch_mlp.gate_proj")
    Path(bad, "adapter_config.json").write_text(json.dumps(acfg))
    with pytest.raises(NotImplementedError, match=r"block_sparse_moe\.switch_mlp\.gate_proj"):
        utils.load_model(str(tmp_path / "e4"), adapter_path=bad, merge_adapter=True, max_positions=MAX_POS)


# ------------------------------------------------------------------------------------------------ 2. the tool
def _steps_equal(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert np.array_equal(x[k].view(np.uint32) if x[k].dtype == np.float32 else x[k],
                                      y[k].view(np.uint32) if y[k].dtype == np.float32 else y[k]), (s, k)


@pytest.mark.parametrize("kvd", MODES)
@pytest.mark.parametrize("name", ["llama_bf16_gqa", "llama_q4_bf16"])
def test_tool_output_equals_merge_at_load_bit_for_bit(tiny_dirs, tmp_path, name, kvd):
    from test_gpu_mixtral_models import _steps

    d, cfg = tiny_dirs[name]
    ad = write_adapter(tmp_path / "ad", d, cfg, ALL)
    out = tmp_path / "merged"
    assert tool.main(["--base-model", d, "--lora-path", ad, "--output-path", str(out)]) == 0
    assert json.loads((out / "config.json").read_text()).get("quantization") == cfg.get("quantization")
    assert (out / "tokenizer.json").exists() or any(out.glob("tokenizer*"))
    at_load, _tok = utils.load(d, adapter_path=ad, merge_adapter=True, max_positions=MAX_POS)
    plain, _tok = utils.load(str(out), max_positions=MAX_POS)
    try:
        assert plain.merged_adapter is None
        _steps_equal(_steps(at_load.engine, kvd, cfg["vocab_size"]), _steps(plain.engine, kvd, cfg["vocab_size"]))
    finally:
        at_load.engine.close(); plain.engine.close()


@pytest.mark.parametrize("mode", MODES)
def test_tool_de_quantize_gives_a_dense_checkpoint_that_matches_its_twin(tiny_dirs, tmp_path, mode):
    d, cfg = tiny_dirs["llama_q4_bf16"]
    ad = write_adapter(tmp_path / "ad", d, cfg, QV + ("mlp.down_proj",))
    out = tmp_path / "dense"
    assert tool.main(["--base-model", d, "--lora-path", ad, "--output-path", str(out), "--de-quantize"]) == 0
    assert "quantization" not in json.loads((out / "config.json").read_text())
    written = load_file(str(out / "model.safetensors"))
    assert not any(k.endswith(".scales") for k in written)
    # the twin: the written checkpoint's own tensors, the adapted ones replaced by the twin's de-quantised merge
    ref = merge_ref.load(str(out), max_pos=MAX_POS)
    twin = merge_ref.load(d, adapter_path=ad, max_pos=MAX_POS, de_quantize=True)
    differ = total = 0
    for name, a, b, _m, s in merge_ref.read_adapter(cfg["num_hidden_layers"], ad):
        got, want = ref.w[name].weight, twin.w[name].weight
        delta = merge_ref.lora_delta(a, b, s, "bfloat16")
        assert (np.abs(got.astype(np.float64) - want) <= mc.one_ulp("bfloat16", got, want, delta)).all(), name
        differ += int((got != want).sum())
        total += got.size
        ref.w[name].weight = want
    print(f"de-quantised merge: {differ} of {total} written elements differ from the twin")
    assert differ <= total // 1000
    model, _tok = utils.load(str(out), max_positions=MAX_POS)
    try:
        against_twin(model.engine, ref, cfg["vocab_size"], mode, "de-quantised")
    finally:
        model.engine.close()


# ------------------------------------------------------------------------------------------------ 3. a merged model's refusals
def test_a_merged_model_refuses_adapters_and_an_unmerged_one_launches_them(tiny_dirs, tmp_path):
    d, cfg = tiny_dirs["llama_bf16_gqa"]
    ad = write_adapter(tmp_path / "ad", d, cfg, QV)
    model, _tok = utils.load(d, adapter_path=ad, merge_adapter=True, max_positions=MAX_POS)
    try:
        before = first_logits(model.engine, cfg["vocab_size"])
        for call in (lambda: utils.load_adapters(model, ad), lambda: utils.load_adapter_into(model, 0, ad),
                     lambda: weight_updater.apply_lora_update(model, ad)):
            with pytest.raises(ValueError, match="merged into this model's weights"):
                call()
        assert np.array_equal(before.view(np.uint32), first_logits(model.engine, cfg["vocab_size"]).view(np.uint32))
    finally:
        model.engine.close()
    with pytest.raises(ValueError, match="adapter_path"):
        utils.load(d, merge_adapter=True, max_positions=MAX_POS)
    beside, _tok = utils.load(d, adapter_path=ad, max_positions=MAX_POS)         # the control of the zero-launch assertion
    try:
        assert beside.merged_adapter is None and launches(beside.engine, "lora_rows", cfg["vocab_size"]) > 0
    finally:
        beside.engine.close()


# ------------------------------------------------------------------------------------------------ 4. the server
def test_one_completion_through_a_server_started_with_merge_lora(tmp_path):
    import requests

    import test_gpu_gqa_models as gqa_models
    from mlx_parallm_amd.tokenizer_utils import load_tokenizer
    from test_gpu_mixtral_models import api_free_port

    d = str(tmp_path / "served")
    cfg = build_tiny_model(d, seed=46, **SMALL)
    ad = write_adapter(tmp_path / "ad", d, cfg, ALL)
    port = api_free_port()
    env = os.environ.copy()
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    log_path = tmp_path / "server.log"
    args = [sys.executable, "-m", "mlx_parallm_amd.cli", "--model-path", d, "--lora-path", ad, "--merge-lora", "--host", "127.0.0.1",
            "--port", str(port), "--max-batch-size", "4", "--batch-timeout", "0.1", "--diverse-mode", "false"]
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
        ref = merge_ref.load(d, adapter_path=ad, max_pos=512)
        want, margins = gqa_models._alone(ref, ids[0], 8, paged=False)
        bare, _m = gqa_models._alone(merge_ref.load(d, max_pos=512), ids[0], 8, paged=False)
        r = requests.post(f"{base}/v1/completions", json={"model": d, "prompt": prompt, "max_tokens": 8, "temperature": 0.0}, timeout=120)
        assert r.status_code == 200, r.text[:500]
        j = r.json()
        assert j["usage"]["prompt_tokens"] == ids.shape[1] and 1 <= j["usage"]["completion_tokens"] <= 8
        # greedy ids are the twin's up to the first step whose top-2 margin is inside the 16-bit bound (or an eos)
        n = next((i for i, m in enumerate(margins) if m <= 0.13), 8)
        if tok.eos_token_id in want[:n]:
            n = want.index(tok.eos_token_id)
        assert j["choices"][0]["text"].startswith(tok.decode(want[:n], skip_special_tokens=True)), (j["choices"][0]["text"], want, margins)
        print(f"served {n} tokens of the merged twin; the bare model's greedy ids are {bare}, the merged twin's {want}")
    finally:
        proc.send_signal(signal.SIGTERM)
        try:
            proc.wait(timeout=20)
        except subprocess.TimeoutExpired:
            proc.kill()
