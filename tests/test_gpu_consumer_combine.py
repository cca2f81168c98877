"""-m gpu: the engine option "consumer_combine"  changes where one sum of a float32-KV decode step is taken --
the K slices of q|k|v in the decode attention's prologue instead of the linear's last arriver -- and nothing else: the
additions, their order and the expression of the row scale are those of the last arriver.  So every output of every step
must be EXACTLY equal (np.array_equal, no tolerance) between consumer_combine = 0 and 1, on the same engine, weights,
prompts and seed.

Models: tests/wide_models.py (Mistral-7B and Qwen3-14B layer shapes -- q/k norm, 5 query heads per kv head, H = 5120 --
2 decoder blocks: block 0 is the rounded layer-0 call, which keeps the ordinary launch, block 1 a float32 layer), bf16
weights, float32 KV.
Cases: contiguous and block-paged caches; batch 1, 3 and 8; KV lengths 40, 200, 1023, 1024, 1100 and 2047 (1, 2, 3, 4 and, for
the short batches, up to 16 attention splits; lengths just below / at / past a multiple of 128); a LoRA adapter on q / v, a
row-subset step and an f16 model's [hi | lo] matrices (all three: the router declines, the ordinary launches run, outputs
equal); the sentinels around the buffer that the seam writes stay intact; option values other than 0 and 1 are refused.
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import wide_models  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

KV_LENGTHS = (40, 200, 1023, 1024, 1100, 2047)
STEPS = 4
MAX_POS = 2112                      # 2047 + STEPS and a block to spare
SEEDS = {"mistral-7b": 11, "qwen3-14b": 12}


class _Models:
    """One checkpoint + engine at a time (rebuilt from seeds, tests/wide_models.py)."""

    def __init__(self, root):
        self.root, self.key, self.model, self.cfgs = root, None, None, {}

    def drop(self):
        if self.model is not None:
            self.model.engine.close()
        self.model = None
        gc.collect()

    def get(self, family, lora=False):
        if self.key != (family, lora):
            self.drop()
            if family not in self.cfgs:
                self.cfgs[family] = wide_models.build_checkpoint(self.root / family, family, "bf16", SEEDS[family])
            self.model = utils.load_model(str(self.root / family), max_positions=MAX_POS)
            if lora:
                wide_models.build_adapter(self.root / family / "adapter", self.cfgs[family], 5)
                utils.load_adapters(self.model, str(self.root / family / "adapter"))
            self.key = (family, lora)
        return self.model, self.cfgs[family]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    m = _Models(tmp_path_factory.mktemp("cc"))
    yield m
    m.drop()


def _new_kv(engine, B, paged):
    if paged:
        return engine.new_paged_kv(B, block_tokens=64, max_tokens_per_row=MAX_POS, kv_dtype="float32")
    return engine.new_kv(B, capacity=MAX_POS, kv_dtype="float32")


def _run(engine, cc, B, L0, paged, vocab, rows=None):
    """Prefill of L0 tokens, then STEPS decode steps (greedy, then seeded top-p draws); every step's outputs."""
    engine.set_option("consumer_combine", cc)
    kv = _new_kv(engine, B, paged)
    prompts = wide_models.prompts_for(dict(prompt_seed=100 + B + L0, B=B, L0=L0), vocab)
    out = [engine.decode_sample(kv, prompts, SampleArgs(temp=0.0))]
    for s in range(STEPS):
        sp = SampleArgs(temp=0.0) if s < 2 else SampleArgs(temp=0.9, top_p=0.9, seed=77, stream_position=s)
        y = out[-1]["tokens"][:, None].astype(np.int32)
        if rows is not None and s == 1:                    # one row-subset step in the middle (the other rows stay behind)
            t = engine.step_enqueue_rows(kv, rows, y[rows], sp)
            r = engine.step_wait(t, len(rows))
            full = {k: out[-1][k].copy() for k in ("tokens", "logprobs", "probs_row0")}
            for k in full:
                full[k][rows] = r[k]
            out.append(full)
            # bring the other rows level again, so that the next step is a whole-batch step
            rest = [b for b in range(B) if b not in rows]
            t = engine.step_enqueue_rows(kv, rest, y[rest], sp)
            r = engine.step_wait(t, len(rest))
            for k in full:
                full[k][rest] = r[k]
            continue
        out.append(engine.decode_sample(kv, y, sp))
    kv.close()
    return out


def _assert_equal(base, other, what):
    assert len(base) == len(other)
    for s, (a, b) in enumerate(zip(base, other)):
        for k in ("tokens", "logprobs", "probs_row0"):
            assert np.array_equal(a[k], b[k]), (what, "step", s, k, a[k], b[k])


def test_seam1_buffer_guards_stay_intact(models):
    model, cfg = models.get("mistral-7b")
    for B, L0 in ((8, 1100), (3, 200), (1, 2047)):
        _run(model.engine, 1, B, L0, False, cfg["vocab_size"])
        model.engine.set_option("consumer_combine_guard", 0)        # raises when a sentinel was overwritten or the seam never ran
    model.engine.set_option("consumer_combine", 0)


def test_option_values_other_than_0_and_1_are_refused(models):
    """The former bit-mask values 2 and 3 fail loudly and leave the option as it was: the run at 1 behind them still
    publishes (the guard check raises when the seam never ran)."""
    model, cfg = models.get("mistral-7b")
    model.engine.set_option("consumer_combine", 1)
    for v in (2, 3):
        with pytest.raises(ValueError):
            model.engine.set_option("consumer_combine", v)
    kv = _new_kv(model.engine, 8, False)
    prompts = wide_models.prompts_for(dict(prompt_seed=7, B=8, L0=200), cfg["vocab_size"])
    out = model.engine.decode_sample(kv, prompts, SampleArgs(temp=0.0))
    model.engine.decode_sample(kv, out["tokens"][:, None].astype(np.int32), SampleArgs(temp=0.0))
    kv.close()
    model.engine.set_option("consumer_combine_guard", 0)
    model.engine.set_option("consumer_combine", 0)


def test_f16_hilo_qkv_declines_the_offer(tiny_dirs):
    """An f16 model in float32-KV mode: the attention side qualifies (head_dim 64 on the float32 MFMA kernel), so forward()
    offers q|k|v -- which runs on the [hi | lo] view (kx > 0), a route without the publish-only form.  The router declines:
    outputs equal those of option 0, and the seam's buffer was never made (the guard check answers NOTFOUND)."""
    d, cfg = tiny_dirs["llama_f16"]
    model = utils.load_model(d, max_positions=64)
    eng = model.engine
    try:
        prompts = np.random.default_rng(3).integers(0, cfg["vocab_size"], size=(2, 12)).astype(np.int32)
        runs = []
        for cc in (0, 1):
            eng.set_option("consumer_combine", cc)
            kv = eng.new_kv(2, capacity=32, kv_dtype="float32")
            out = [eng.decode_sample(kv, prompts, SampleArgs(temp=0.0))]
            for _ in range(3):
                out.append(eng.decode_sample(kv, out[-1]["tokens"][:, None].astype(np.int32), SampleArgs(temp=0.0)))
            kv.close()
            runs.append(out)
        _assert_equal(runs[0], runs[1], "f16 [hi | lo]")
        with pytest.raises((KeyError, FileNotFoundError)):
            eng.set_option("consumer_combine_guard", 0)
    finally:
        eng.close()


def test_row_subset_step_takes_the_ordinary_launches(models):
    model, cfg = models.get("mistral-7b")
    base = _run(model.engine, 0, 8, 1100, False, cfg["vocab_size"], rows=[0, 2, 5])
    _assert_equal(base, _run(model.engine, 1, 8, 1100, False, cfg["vocab_size"], rows=[0, 2, 5]), "rows")
    model.engine.set_option("consumer_combine", 0)


def test_lora_on_q_v_takes_the_ordinary_qkv_launch(models):
    model, cfg = models.get("mistral-7b", lora=True)
    for B, L0 in ((8, 1100), (3, 1023)):
        base = _run(model.engine, 0, B, L0, True, cfg["vocab_size"])
        _assert_equal(base, _run(model.engine, 1, B, L0, True, cfg["vocab_size"]), ("lora", B, L0))
    model.engine.set_option("consumer_combine", 0)


@pytest.mark.parametrize("B", (1, 3, 8))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("family", ("mistral-7b", "qwen3-14b"))
def test_outputs_are_bit_identical(models, family, paged, B):
    model, cfg = models.get(family)
    for L0 in KV_LENGTHS:
        base = _run(model.engine, 0, B, L0, paged, cfg["vocab_size"])
        _assert_equal(base, _run(model.engine, 1, B, L0, paged, cfg["vocab_size"]), (family, paged, B, L0))
    model.engine.set_option("consumer_combine", 0)
