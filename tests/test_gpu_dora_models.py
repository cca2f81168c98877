"""DoRA adapters on the engine (-m gpu), against the oracle-side twin tests/dora_ref.py: the tiny Qwen3 (bf16) and Llama (f16)
checkpoints, DoRA on all seven projections of both blocks, m = ||W|| (1 + 0.2 noise) so that the gain is far from 1, both KV modes.

Bounds (the project's own, tests/test_gpu_lora_targets.py):
  float32-KV  greedy ids exact, logprobs within 1e-3 over the prompt + 3 decode steps; logits within 4e-3
  model-KV    logprobs within 0.1 wherever the twin's top-2 margin is at least 0.13 (ids must agree there)
Prompts are chosen on the CPU: the first seed of a fixed list at which the twin's own top-2 margin exceeds twice the logit
bound (float32-KV) at every compared position, so that an id cannot flip inside the bound.

Cases: the engine-wide adapter through utils.load(adapter_path=...); per-request rows {DoRA, LoRA, DoRA of another rank, none}
in one prefill batch, decode batches and one mixed step, each row against the twin of its own adapter, the LoRA and bare rows
bit-equal to the same batch on an engine without the DoRA slots; a Phi-3 checkpoint (fused names, m cut by parts); a
rope_traditional Llama (m regrouped); Mixtral (attention projections served, block_sparse_moe.* refused); hot-swap LoRA -> DoRA -> LoRA in one slot; the refusals, each followed by a step
that shows the engine unchanged."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import dora_ref
from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

MAX_POS = 128
SCALE, NLAYERS = 10.0, 2
ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
       "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
NAMES = ["qwen3_bf16", "llama_f16"]
MODES = {"float32": ("float32", True, 4e-3), "model": ("model", False, None)}
LOGPROB_TOL_F32KV = 1e-3
MODEL_KV_LOGPROB_TOL, MODEL_KV_MARGIN = 0.1, 0.13
SEEDS = range(1, 9)
STEPS = 3
# adapter name -> (kind, rank, seed of its factors)
ADAPTERS = {"D16": ("dora", 16, 5), "L": ("lora", 16, 6), "D4": ("dora", 4, 7)}


def _dims(cfg):
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D = cfg.get("head_dim") or H // nh
    I = cfg["intermediate_size"]
    return {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}


def write_adapter(dst, model_dir, cfg, kind, rank, seed, spelling="fine_tune_type", bad_m=None):
    """rank-`rank` factors (A ~ U(+-1/sqrt(K)), B ~ N(0, 0.05^2), float32) on all seven projections of the last two blocks; a
    DoRA directory also holds m = ||W|| (1 + 0.2 noise) per projection."""
    dst.mkdir(parents=True, exist_ok=True)
    base = ref_generate.load_weights(model_dir, cfg)
    nl, dims, t = cfg["num_hidden_layers"], _dims(cfg), {}
    for i in range(nl - NLAYERS, nl):
        for ki, key in enumerate(ALL):
            K, n = dims[key]
            rng = np.random.default_rng([seed, i, ki])
            name = f"model.layers.{i}.{key}"
            t[name + ".lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32))
            t[name + ".lora_b"] = torch.from_numpy((rng.standard_normal((rank, n)) * 0.05).astype(np.float32))
            if kind == "dora":
                norm = np.sqrt((base[name].weight.astype(np.float64) ** 2).sum(axis=1))
                m = (norm * (1.0 + 0.2 * rng.standard_normal(n))).astype(np.float32)
                if bad_m == name:
                    m[3] = np.inf
                t[name + ".m"] = torch.from_numpy(m)
    save_file(t, str(dst / "adapters.safetensors"))
    cfg_out = {"num_layers": NLAYERS, "lora_parameters": {"rank": rank, "scale": SCALE, "dropout": 0.0, "keys": list(ALL)}}
    if spelling == "fine_tune_type":
        cfg_out["fine_tune_type"] = kind
    elif kind == "dora":
        cfg_out["use_dora"] = True
    (dst / "adapter_config.json").write_text(json.dumps(cfg_out))
    return str(dst)


class Bank:
    def __init__(self, tiny_dirs, root):
        self.tiny, self.root, self._dir, self._ref = tiny_dirs, root, {}, {}

    def cfg(self, name):
        return self.tiny[name][1]

    def adapter(self, name, ad):
        if (name, ad) not in self._dir:
            kind, rank, seed = ADAPTERS[ad]
            self._dir[name, ad] = write_adapter(self.root / f"{name}_{ad}", self.tiny[name][0], self.cfg(name), kind, rank, seed,
                                                spelling="use_dora" if ad == "D4" else "fine_tune_type")
        return self._dir[name, ad]

    def ref(self, name, ad):
        if (name, ad) not in self._ref:
            self._ref[name, ad] = dora_ref.load(self.tiny[name][0], adapter_path=self.adapter(name, ad) if ad else None, max_pos=MAX_POS)
        return self._ref[name, ad]

    def oracle_rows(self, name, mode, ads, B_L0):
        """every row through the twin of its own adapter, teacher-forced on its own greedy ids, for the first seed whose
        margins clear the bound -> (prompt, feeds [prompt, next ids ...], logits per feed (B, V))"""
        paged = MODES[mode][1]
        for seed in SEEDS:
            toks = np.random.default_rng([seed, *B_L0]).integers(3, self.cfg(name)["vocab_size"], size=B_L0).astype(np.int32)
            feeds, want, ok = [toks], [], True
            caches = [self.ref(name, ad).make_cache(1, paged=paged) for ad in ads]
            for _ in range(STEPS + 1):
                lg = np.stack([self.ref(name, ad)(feeds[-1][b:b + 1], cache=caches[b])[0, -1] for b, ad in enumerate(ads)])
                want.append(lg)
                top2 = np.sort(lg, axis=-1)[:, -2:]
                if mode == "float32" and float((top2[:, 1] - top2[:, 0]).min()) <= 2 * MODES[mode][2]:
                    ok = False
                    break
                feeds.append(np.argmax(lg, axis=-1)[:, None].astype(np.int32))
            if ok:
                return toks, feeds[:-1], want
        raise AssertionError("no seed of the list gives the twin a top-2 margin above the bound")


@pytest.fixture(scope="module")
def bank(tiny_dirs, tmp_path_factory):
    return Bank(tiny_dirs, tmp_path_factory.mktemp("dora_models"))


def _kv(eng, B, cap, mode, slots=None):
    kv = eng.new_kv(B, capacity=cap, kv_dtype=MODES[mode][0])
    for b, s in enumerate(slots or []):
        kv.set_row_adapter(b, s)
    return kv


def _compare(eng, mode, feeds, want, slots=None, what=""):
    """logits (float32-KV: within the bound) and the sampler's ids / logprobs against the twins -> the logits of every feed"""
    B = feeds[0].shape[0]
    cap = feeds[0].shape[1] + len(feeds) + 1
    kv = _kv(eng, B, cap, mode, slots)
    got = [eng.forward(f, kv) for f in feeds]
    kv.close()
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print(f"{what} {mode}: max |logit - twin| = {err:.3e}")
    if mode == "float32":
        assert err <= MODES[mode][2], (what, err)
    kv = _kv(eng, B, cap, mode, slots)
    wrong, lp_err = 0, 0.0
    for f, w in zip(feeds, want):
        res = eng.decode_sample(kv, f, SampleArgs(temp=0.0))
        ws = ref_sample.sample(w, temp=0.0)
        top2 = np.sort(w, axis=-1)[:, -2:]
        sure = np.ones(B, bool) if mode == "float32" else (top2[:, 1] - top2[:, 0]) >= MODEL_KV_MARGIN
        wrong += int((res["tokens"] != ws["tokens"][:, 0])[sure].sum())
        if sure.any():
            lp_err = max(lp_err, float(np.abs(res["logprobs"] - ws["logprobs"].reshape(-1))[sure].max()))
    kv.close()
    print(f"{what} {mode}: ids off {wrong}, max |logprob - twin| = {lp_err:.3e}")
    assert wrong == 0 and lp_err <= (LOGPROB_TOL_F32KV if mode == "float32" else MODEL_KV_LOGPROB_TOL), (what, wrong, lp_err)
    return got


# ------------------------------------------------------------------------------------ 1. engine-wide, utils.load end to end
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_engine_wide_dora(bank, name, mode):
    toks, feeds, want = bank.oracle_rows(name, mode, ["D16", "D16"], (2, 7))
    # the gain is seen: on the twin alone, DoRA's logits are far from those of its own factors without m
    lora_only = dora_ref.load(bank.tiny[name][0], max_pos=MAX_POS)
    ref_generate.apply_adapters(lora_only.w, bank.cfg(name)["num_hidden_layers"], bank.adapter(name, "D16"))
    lg = lora_only(toks, cache=lora_only.make_cache(2, paged=MODES[mode][1]))[:, -1]
    assert float(np.abs(lg - want[0]).max()) >= 0.05
    model, _tok = utils.load(bank.tiny[name][0], adapter_path=bank.adapter(name, "D16"), max_positions=MAX_POS)
    _compare(model.engine, mode, feeds, want, what=f"{name} engine-wide")
    model.engine.close()


# ------------------------------------------------------------------------------------ 2. per-request rows
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_rows_of_one_batch_run_dora_lora_and_nothing(bank, name, mode):
    ads = ["D16", "L", "D4", None]
    slots = [0, 1, 2, -1]
    toks, feeds, want = bank.oracle_rows(name, mode, ads, (4, 6))
    model = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    for s, ad in zip(slots[:3], ads[:3]):
        utils.load_adapter_into(model, s, bank.adapter(name, ad))
    got = _compare(model.engine, mode, feeds, want, slots, what=f"{name} rows")           # a prefill batch, then decode batches
    model.engine.close()
    # the same batch on an engine without the DoRA slots resident: the LoRA row and the bare row keep their bits
    model = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    utils.load_adapter_into(model, 1, bank.adapter(name, "L"))
    kv = _kv(model.engine, 4, 6 + len(feeds) + 1, mode, [-1, 1, -1, -1])
    for f, g in zip(feeds, got):
        base = model.engine.forward(f, kv)
        assert np.array_equal(base[1].view(np.uint32), g[1].view(np.uint32)), "the LoRA row moved"
        assert np.array_equal(base[3].view(np.uint32), g[3].view(np.uint32)), "the bare row moved"
        assert not np.array_equal(base[0], g[0]) and not np.array_equal(base[2], g[2])
    kv.close()
    model.engine.close()


# ------------------------------------------------------------------------------------ 5. hot-swap
@pytest.mark.parametrize("name", NAMES)
def test_hot_swap_lora_dora_lora(bank, name):
    cfg = bank.cfg(name)
    toks = np.random.default_rng(3).integers(3, cfg["vocab_size"], size=40).astype(np.int32)
    model = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    eng = model.engine
    kv = eng.new_paged_kv(2, block_tokens=16, n_blocks=20, max_tokens_per_row=64, kv_dtype="float32")

    def run():
        kv.reset_row(0)
        kv.set_row_adapter(0, 0)
        eng.step_wait(eng.step_enqueue_rows(kv, [0], toks[None], SampleArgs(temp=0.0)), 1)
        kv.prefix_publish(0, toks)
        kv.reset_row(1)
        kv.set_row_adapter(1, 0)
        reused = kv.prefix_attach(1, toks)
        kv.reset_row(1)
        k2 = eng.new_kv(1, capacity=48, kv_dtype="float32")
        k2.set_row_adapter(0, 0)
        out = eng.forward(toks[None, :9], k2, all_positions=True).copy()
        k2.close()
        return out, reused

    def attach_after_swap():
        kv.reset_row(1)
        kv.set_row_adapter(1, 0)
        n = kv.prefix_attach(1, toks)
        kv.reset_row(1)
        return n

    utils.load_adapter_into(model, 0, bank.adapter(name, "L"))
    first, reused = run()
    assert reused == 32
    utils.load_adapter_into(model, 0, bank.adapter(name, "D16"))
    assert attach_after_swap() == 0                                # the slot's generation moved: nothing of the old contents
    second, reused = run()
    assert reused == 32
    utils.load_adapter_into(model, 0, bank.adapter(name, "L"))
    assert attach_after_swap() == 0
    third, _ = run()
    assert np.array_equal(first.view(np.uint32), third.view(np.uint32)), "LoRA after DoRA differs from LoRA before"
    assert float(np.abs(first - second).max()) >= 0.05
    kv.close()
    eng.close()


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing(bank, tiny_dirs, tmp_path):
    name = "qwen3_bf16"
    cfg = bank.cfg(name)
    toks = np.random.default_rng(4).integers(3, cfg["vocab_size"], size=(1, 6)).astype(np.int32)
    model = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    eng = model.engine
    utils.load_adapter_into(model, 0, bank.adapter(name, "D16"))

    def logits():
        kv = _kv(eng, 1, 8, "float32", [0])
        out = eng.forward(toks, kv).copy()
        kv.close()
        return out

    before = logits()
    last = cfg["num_hidden_layers"] - 1
    bad = write_adapter(tmp_path / "bad", bank.tiny[name][0], cfg, "dora", 16, 5, bad_m=f"model.layers.{last}.mlp.down_proj")
    with pytest.raises(ValueError, match=r"mlp\.down_proj.*not finite"):
        for i, key, a, b, m, scale in utils._read_adapter(cfg["num_hidden_layers"], bad):
            if i == last and key == "mlp.down_proj":
                eng.set_adapter_dora(0, i, key, a, b, m, scale)
    K, n = _dims(cfg)["self_attn.o_proj"]
    a, b = np.zeros((K, 2), np.float32), np.zeros((2, n), np.float32)
    with pytest.raises(NotImplementedError):                                   # rank 65
        eng.set_adapter_dora(0, last, "self_attn.o_proj", np.zeros((K, 65), np.float32), np.zeros((65, n), np.float32), np.ones(n), 1.0)
    with pytest.raises(NotImplementedError, match="exclude"):                  # the engine-wide form beside resident slots
        eng.set_dora(last, "self_attn.o_proj", a, b, np.ones(n, np.float32), 1.0)
    with pytest.raises(ValueError):                                            # m of the wrong length never reaches the library
        eng.set_adapter_dora(0, last, "self_attn.o_proj", a, b, np.ones(n + 1, np.float32), 1.0)
    assert np.array_equal(before.view(np.uint32), logits().view(np.uint32))
    eng.close()
    # a quantised base
    qname = "llama_q4_bf16"
    qcfg = tiny_dirs[qname][1]
    qmodel = utils.load_model(tiny_dirs[qname][0], max_positions=MAX_POS)
    qtoks = np.random.default_rng(4).integers(3, qcfg["vocab_size"], size=(1, 6)).astype(np.int32)
    kv = qmodel.engine.new_kv(1, capacity=8, kv_dtype="float32")
    qbefore = qmodel.engine.forward(qtoks, kv).copy()
    kv.close()
    K, n = _dims(qcfg)["self_attn.o_proj"]
    with pytest.raises(NotImplementedError, match="quantised"):
        qmodel.engine.set_adapter_dora(0, 0, "self_attn.o_proj", np.zeros((K, 2), np.float32), np.zeros((2, n), np.float32),
                                       np.ones(n, np.float32), 1.0)
    kv = qmodel.engine.new_kv(1, capacity=8, kv_dtype="float32")
    assert np.array_equal(qbefore.view(np.uint32), qmodel.engine.forward(qtoks, kv).view(np.uint32))
    kv.close()
    qmodel.engine.close()
    # before finalize
    from mlx_parallm_amd.engine import Engine
    raw = Engine(json.loads(open(tiny_dirs[name][0] + "/config.json").read()), max_positions=MAX_POS)
    K, n = _dims(cfg)["self_attn.o_proj"]
    with pytest.raises(ValueError, match="finalize"):
        raw.set_adapter_dora(0, 0, "self_attn.o_proj", np.zeros((K, 2), np.float32), np.zeros((2, n), np.float32), np.ones(n, np.float32), 1.0)
    raw.close()


# ------------------------------------------------------------------------------------ 3. Phi-3: the fused projections
@pytest.mark.parametrize("kvd", ["model", "float32"])
def test_phi3_fused_names_equal_the_split_names_bit_for_bit(tmp_path_factory, kvd):
    """DoRA on self_attn.qkv_proj / mlp.gate_up_proj / o_proj / down_proj of a Phi-3 engine, m cut by parts inside the call,
    against one call per part on the Llama-form twin of the checkpoint (whose DoRA the tests above hold against the oracle)."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden" / "d96"))
    import make_golden_d96 as gen
    from mlx_parallm_amd.tiny_model import build_tiny_model

    root = tmp_path_factory.mktemp("dora_phi3")
    kw = dict(gen.SMALL_MODELS["phi3_h384_bf16"])
    build_tiny_model(root / "split", **kw)
    cfg = build_tiny_model(root / "fused", **gen.phi3_kwargs(kw))
    H, I, rank, last = cfg["hidden_size"], cfg["intermediate_size"], 8, cfg["num_hidden_layers"] - 1
    fused, split = utils.load_model(str(root / "fused"), max_positions=MAX_POS), utils.load_model(str(root / "split"), max_positions=MAX_POS)
    rng = np.random.default_rng(13)
    toks = rng.integers(3, cfg["vocab_size"], size=(3, 9)).astype(np.int32)

    def run(eng):
        kv = eng.new_kv(3, capacity=16, kv_dtype=kvd)
        out = [eng.forward(toks, kv).copy()]
        out.append(eng.forward(np.argmax(out[0], axis=-1)[:, None].astype(np.int32), kv).copy())
        kv.close()
        return out

    try:
        base = run(fused.engine)
        for proj, K, parts in (("self_attn.qkv_proj", H, (("self_attn.q_proj", H), ("self_attn.k_proj", H), ("self_attn.v_proj", H))),
                               ("mlp.gate_up_proj", H, (("mlp.gate_proj", I), ("mlp.up_proj", I))),
                               ("self_attn.o_proj", H, (("self_attn.o_proj", H),)), ("mlp.down_proj", I, (("mlp.down_proj", H),))):
            N = sum(n for _, n in parts)
            a = (rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32)
            b = (rng.standard_normal((rank, N)) * 0.3).astype(np.float32)
            m = (0.5 + rng.random(N)).astype(np.float32)
            fused.engine.set_dora(last, proj, a, b, m, 4.0)
            c0 = 0
            for nm, n in parts:
                split.engine.set_dora(last, nm, a, np.ascontiguousarray(b[:, c0:c0 + n]), np.ascontiguousarray(m[c0:c0 + n]), 4.0)
                c0 += n
        got, want = run(fused.engine), run(split.engine)
        for g, w, b0 in zip(got, want, base):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
            assert float(np.abs(g - b0).max()) >= 0.05, "the adapter changed nothing"
    finally:
        fused.engine.close(); split.engine.close()


# ------------------------------------------------------------------------------------ 4. rope_traditional: m regrouped; a biased checkpoint
@pytest.mark.parametrize("mode", list(MODES))
def test_rope_traditional_llama_regroups_m(tmp_path_factory, mode):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    root = tmp_path_factory.mktemp("dora_trad")
    cfg = build_tiny_model(root / "trad", seed=11, vocab_size=512, dtype="bfloat16", quantize_model=False, hidden_size=128, layers=2,
                           heads=4, kv_heads=2, intermediate_size=256, head_dim=32, tie_word_embeddings=False, norm_jitter=0.1,
                           rope_traditional=True)
    bank = Bank({"trad": (str(root / "trad"), cfg)}, root)
    toks, feeds, want = bank.oracle_rows("trad", mode, ["D16", "D16"], (2, 7))
    model = utils.load_model(str(root / "trad"), max_positions=MAX_POS)
    utils.load_adapters(model, bank.adapter("trad", "D16"))
    _compare(model.engine, mode, feeds, want, what="rope_traditional")
    model.engine.close()


def test_biased_projection_is_refused(tmp_path):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(tmp_path / "biased", seed=12, vocab_size=512, dtype="bfloat16", quantize_model=False, hidden_size=128,
                           layers=2, heads=4, kv_heads=2, intermediate_size=256, head_dim=32, tie_word_embeddings=False,
                           attention_bias=True, mlp_bias=False)
    model = utils.load_model(str(tmp_path / "biased"), max_positions=MAX_POS)
    eng = model.engine
    toks = np.random.default_rng(4).integers(3, cfg["vocab_size"], size=(1, 6)).astype(np.int32)

    def logits():
        kv = eng.new_kv(1, capacity=8, kv_dtype="float32")
        out = eng.forward(toks, kv).copy()
        kv.close()
        return out

    before = logits()
    dims = _dims(cfg)
    K, n = dims["self_attn.o_proj"]
    with pytest.raises(NotImplementedError, match="bias"):
        eng.set_adapter_dora(0, 1, "self_attn.o_proj", np.zeros((K, 2), np.float32), np.zeros((2, n), np.float32), np.ones(n, np.float32), 1.0)
    assert np.array_equal(before.view(np.uint32), logits().view(np.uint32))
    K, n = dims["mlp.down_proj"]                                             # mlp_bias is off: the MLP of the same model takes DoRA
    eng.set_adapter_dora(0, 1, "mlp.down_proj", np.full((K, 2), 0.01, np.float32), np.full((2, n), 0.01, np.float32), np.ones(n, np.float32), 1.0)
    eng.close()


# ------------------------------------------------------------------------------------ 2b. per-request rows in one mixed step
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_mixed_step_rows_run_their_own_adapters(bank, name, mode):
    """mi_step_enqueue_mixed, the step shape of the continuous scheduler: rows 0..2 (DoRA, LoRA, DoRA of rank 4) decode one
    token each while row 3 (no adapter) prefills a 5-token chunk, in one pass over the weights; then a plain forward over the
    four rows.  Every row against the twin of its own adapter; the LoRA row and the bare row bit-equal to the same steps on an
    engine without the DoRA slots."""
    cfg = bank.cfg(name)
    kvd, paged, _ = MODES[mode]
    ads, slots = ["D16", "L", "D4", None], [0, 1, 2, -1]
    greedy = SampleArgs(temp=0.0)
    seeds = iter(SEEDS)

    def twin_run(seed):
        """-> (prompts, wants per step [(logits, sample)], the next ids) or None when a float32-KV margin is inside the bound"""
        rng = np.random.default_rng([seed, 77])
        P = [rng.integers(3, cfg["vocab_size"], size=n).astype(np.int32) for n in (6, 4, 7, 5)]
        caches = [bank.ref(name, ad).make_cache(1, paged=paged) for ad in ads]

        def oracle(i, toks):
            lg = bank.ref(name, ads[i])(np.asarray(toks, dtype=np.int32)[None], cache=caches[i])[0, -1]
            top2 = np.sort(lg)[-2:]
            return lg, ref_sample.sample(lg[None], temp=0.0), float(top2[1] - top2[0])

        first = [oracle(i, P[i]) for i in range(3)]
        t = [int(w[1]["tokens"][0, 0]) for w in first]
        second = [oracle(i, [t[i]]) for i in range(3)] + [oracle(3, P[3])]
        nxt = np.asarray([[int(w[1]["tokens"][0, 0])] for w in second], dtype=np.int32)
        third = [oracle(i, nxt[i]) for i in range(4)]
        if mode == "float32" and min(w[2] for w in first + second + third) <= 2 * MODES[mode][2]:
            return None
        return P, first, t, second, nxt, np.stack([w[0] for w in third])

    run = None
    while run is None:
        run = twin_run(next(seeds))                    # (StopIteration: no seed of the list clears the bound)
    P, first, t, second, nxt, third = run

    def compare(res, wants):
        for j, (lg, w, _m) in enumerate(wants):
            gt, wt = int(res["tokens"][j]), int(w["tokens"][0, 0])
            if mode == "float32":
                assert gt == wt, (j, gt, wt)
                assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= LOGPROB_TOL_F32KV
            else:
                assert gt == wt or float(lg[wt] - lg[gt]) <= MODEL_KV_MARGIN, (j, gt, wt)
                if gt == wt:
                    assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= MODEL_KV_LOGPROB_TOL

    def engine_run(resident, row_slots):
        model = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
        for s, ad in resident:
            utils.load_adapter_into(model, s, bank.adapter(name, ad))
        eng = model.engine
        kv = _kv(eng, 4, 32, mode, row_slots)
        r1 = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 2], [P[0], P[1], P[2]], [1, 1, 1], greedy), 3)
        r2 = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 2, 3], [[t[0]], [t[1]], [t[2]], P[3]], [1, 1, 1, 1], greedy), 4)   # THE mixed step
        assert kv.offsets == [7, 5, 8, 5]
        lg = eng.forward(nxt, kv).copy()
        kv.close()
        eng.close()
        return r1, r2, lg

    r1, r2, lg = engine_run(list(zip(slots[:3], ads[:3])), slots)
    compare(r1, first)
    compare(r2, second)
    err = float(np.abs(lg - third).max())
    print(f"{name} {mode}: forward behind the mixed step, max |logit - twin| = {err:.3e}")
    if mode == "float32":
        assert err <= MODES[mode][2], err
    b1, b2, blg = engine_run([(1, "L")], [-1, 1, -1, -1])
    for j in (1, 3):
        assert int(b2["tokens"][j]) == int(r2["tokens"][j])
        assert np.array_equal(np.float32(b2["logprobs"][j]).view(np.uint32), np.float32(r2["logprobs"][j]).view(np.uint32)), f"row {j} moved in the mixed step"
        assert np.array_equal(blg[j].view(np.uint32), lg[j].view(np.uint32)), f"row {j} moved behind the mixed step"
    assert int(b1["tokens"][1]) == int(r1["tokens"][1]) and float(b1["logprobs"][1]) == float(r1["logprobs"][1])
    assert not np.array_equal(blg[0], lg[0]) and not np.array_equal(blg[2], lg[2])


# ------------------------------------------------------------------------------------ 6b. Mixtral: attention served, block_sparse_moe.* refused
def test_mixtral_attention_dora_and_the_moe_refusal(tmp_path):
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden" / "moe"))
    import make_golden_moe as gen
    import moe_ref
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path / "e4"
    cfg = build_tiny_model(d, **dict(gen.MODELS["moe_e4k2_bf16"][0], seed=41))
    keys = ALL[:4]
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv, D = cfg.get("num_key_value_heads") or nh, cfg.get("head_dim") or H // nh
    dims = {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D), "self_attn.o_proj": (nh * D, H)}
    ref = moe_ref.load(str(d), max_pos=MAX_POS)
    nl, rank, scale = cfg["num_hidden_layers"], 8, 4.0
    entries = []
    for i in range(nl):
        for ki, key in enumerate(keys):
            K, n = dims[key]
            rng = np.random.default_rng([23, i, ki])
            a = (rng.uniform(-1, 1, (K, rank)) / np.sqrt(K)).astype(np.float32)
            b = (rng.standard_normal((rank, n)) * 0.05).astype(np.float32)
            lin = ref.w[f"model.layers.{i}.{key}"]
            m = (np.sqrt((lin.weight.astype(np.float64) ** 2).sum(axis=1)) * (1.0 + 0.2 * rng.standard_normal(n))).astype(np.float32)
            lin.lora_a, lin.lora_b, lin.lora_scale = a, b, scale
            ref.w[f"model.layers.{i}.{key}"] = dora_ref.DoraLinear.wrap(lin, m)
            entries.append((i, key, a, b, m))
    model = utils.load_model(str(d), max_positions=MAX_POS)
    eng = model.engine
    toks = np.random.default_rng(17).integers(3, cfg["vocab_size"], size=(2, 8)).astype(np.int32)

    def logits():
        kv = eng.new_kv(2, capacity=16, kv_dtype="float32")
        out = eng.forward(toks, kv).copy()
        kv.close()
        return out

    try:
        base = logits()
        for proj, K, n in (("block_sparse_moe.gate", H, cfg["num_local_experts"]),
                           ("block_sparse_moe.switch_mlp.gate_proj", H, cfg["intermediate_size"]),
                           ("block_sparse_moe.experts.0.w1", H, cfg["intermediate_size"]), ("mlp.gate_proj", H, cfg["intermediate_size"])):
            with pytest.raises(NotImplementedError):
                eng.set_dora(0, proj, np.zeros((K, 4), np.float32), np.zeros((4, n), np.float32), np.ones(n, np.float32), 1.0)
            with pytest.raises(NotImplementedError):
                eng.set_adapter_dora(0, 0, proj, np.zeros((K, 4), np.float32), np.zeros((4, n), np.float32), np.ones(n, np.float32), 1.0)
        assert np.array_equal(base.view(np.uint32), logits().view(np.uint32)), "a refused call changed the engine"
        for i, key, a, b, m in entries:
            eng.set_dora(i, key, a, b, m, scale)
        got = logits()
        want = ref(toks, cache=ref.make_cache(2, paged=True))[:, -1]
        assert np.abs(got - base).max() > 0.05, "the adapter changed nothing"
        margin = min(float(np.min(mm)) for _l, mm, _a in ref.margins)
        err = float(np.abs(got - want).max())
        print(f"Mixtral, DoRA on q/k/v/o against the twin: max |logit difference| {err:.3e}, smallest router margin {margin:.3e}")
        assert margin < 1e-3 or err <= 4e-3, (err, margin)     # (the bound of the LoRA case: a router within 1e-3 of a flip voids it)
    finally:
        eng.close()
