"""The HIP path against the oracle at the Llama-3.2-3B layer shapes (hidden 3072, 24 query / 8 KV heads of 128 -- 3 query
heads per KV head --, intermediate 8192, vocabulary 128256, tied embeddings), 2 decoder blocks: tests/golden/gqa/wide_*.npz and
their float32-accumulation envelopes, made by tests/golden/gqa/make_golden_gqa.py.  int4 g64 in both KV modes and bf16 in float32-KV,
batch 8 with 1024-token prompts decoded over 77 steps (KV 1024 -> 1100).

The device test IS tests/test_gpu_golden_wide.py::test_device_matches_oracle_at_production_width -- the same function, pointed
at these files and at the checkpoints of this family -- so the assertions, ENVELOPE_FACTOR and MEAN_FACTOR are its own.  Also
at this width: block-paged == contiguous bit for bit (that file's test) and consumer_combine on == off (the float32 matrix-core
decode kernel that adds the q|k|v partial rows in its prologue, at G = 3).  The file checks run without a device.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GQA = Path(__file__).resolve().parent / "golden" / "gqa"
sys.path.insert(0, str(GQA))

import make_golden_gqa as gen  # noqa: E402
import test_golden as cpu_golden  # noqa: E402
import test_gpu_consumer_combine as cc_base  # noqa: E402
import test_gpu_golden_wide as wide  # noqa: E402
import wide_models  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402

gpu = pytest.mark.gpu
WIDE = sorted(GQA.glob("wide_*.npz"))
REQUIRED = {"wide_llama32_3b_int4_modelkv", "wide_llama32_3b_int4_paged", "wide_llama32_3b_bf16_paged"}


class _Checkpoints(wide._Checkpoints):
    """tests/test_gpu_golden_wide.py's holder of one checkpoint + engine at a time, building this family's checkpoints."""

    def get(self, family, precision, seed, lora, adapter_seed, layers=wide_models.LAYERS):
        assert family == gen.FAMILY and not lora and layers == wide_models.LAYERS
        key = (family, precision, seed, layers)
        if key != self.key:
            self._drop()
            if self.dir is not None:
                for f in Path(self.dir).rglob("*"):
                    if f.is_file():
                        f.unlink()
            self.dir = self.root / f"{family}-{precision}-{seed}"
            self.cfg = gen.build_checkpoint(self.dir, family, precision, seed)
            self.key = key
        if self.model is None:
            self.model = utils.load_model(str(self.dir), max_positions=cc_base.MAX_POS)
        return self.model, self.cfg


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    c = _Checkpoints(tmp_path_factory.mktemp("gqa_wide"))
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the files (no device)

def test_wide_gqa_files_present_with_their_envelopes(monkeypatch):
    assert REQUIRED <= {p.stem for p in WIDE}, "run tests/golden/gqa/make_golden_gqa.py --wide --envelope"
    monkeypatch.setattr(wide, "GOLD", GQA)
    largest = max(p.stat().st_size for p in GQA.parent.glob("wide_*.npz"))
    for p in WIDE:
        spec = json.loads(str(np.load(p)["spec"]))
        assert (spec["family"], spec["B"], spec["L0"], spec["steps"]) == (gen.FAMILY, 8, 1024, 77)
        env = wide.envelope_of(p.stem)
        assert env is not None and env["mean_lp"] > 0, p.stem
        assert p.stat().st_size <= largest and (GQA / "envelope" / p.name).stat().st_size <= largest
        # (the bound tests/test_golden.py holds for the envelopes of the 2-block cases)
        assert env["max_lp"] <= (0.1 if not spec["paged"] else 2e-2), (p.stem, env)


@pytest.mark.parametrize("path", WIDE, ids=[p.stem for p in WIDE])
def test_wide_gqa_files_are_consistent(path):
    cpu_golden.test_wide_golden_files_are_consistent(path)


def test_family_is_the_llama32_3b_layer_shapes():
    kw = gen.model_kwargs("int4", 51)
    assert (kw["hidden_size"], kw["heads"], kw["kv_heads"], kw["head_dim"], kw["intermediate_size"], kw["vocab_size"]) == \
        (3072, 24, 8, 128, 8192, 128256)
    assert (kw["rms_norm_eps"], kw["rope_theta"], kw["tie_word_embeddings"], kw["layers"]) == (1e-5, 500000.0, True, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# the device

@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_consumer_combine_on_equals_off(checkpoints, paged):
    """bf16 weights, float32 KV, 8 and 3 rows at KV 1100 / 200: outputs equal with no tolerance.  Whether the q|k|v linear took the
    publish-only route at this width is printed, not asserted (a router that declines runs the ordinary launches)."""
    model, cfg = checkpoints.get(gen.FAMILY, "bf16", 52, False, 0)
    try:
        for B, L0 in ((8, 1100), (3, 200)):
            base = cc_base._run(model.engine, 0, B, L0, paged, cfg["vocab_size"])
            cc_base._assert_equal(base, cc_base._run(model.engine, 1, B, L0, paged, cfg["vocab_size"]), ("llama-3.2-3b", paged, B, L0))
        try:
            model.engine.set_option("consumer_combine_guard", 0)
            print("consumer_combine at the Llama-3.2-3B width: q|k|v published its K slices, guards intact")
        except (KeyError, FileNotFoundError):
            print("consumer_combine at the Llama-3.2-3B width: the router declined, ordinary launches ran")
    finally:
        model.engine.set_option("consumer_combine", 0)


@gpu
@pytest.mark.parametrize("path", WIDE, ids=[p.stem for p in WIDE])
def test_device_matches_oracle_at_llama32_3b_width(checkpoints, path, monkeypatch):
    monkeypatch.setattr(wide, "GOLD", GQA)
    wide.test_device_matches_oracle_at_production_width(checkpoints, path)


@gpu
@pytest.mark.parametrize("kvd", ["model", "float32"])
def test_block_paged_arena_is_bit_identical_to_contiguous_kv(checkpoints, kvd):
    wide.test_block_paged_arena_is_bit_identical_to_contiguous_kv_at_production_width(checkpoints, gen.FAMILY, "int4", 51, False, kvd)
