"""The HIP path against the oracle at the Phi-3-mini layer shapes (hidden 3072, 32 query / 32 KV heads of 96, intermediate 8192,
vocabulary 32064, an lm_head of its own), 2 decoder blocks: tests/golden/d96/wide_*.npz and their float32-accumulation
envelopes, made by tests/golden/d96/make_golden_d96.py.  int4 g64 in both KV modes and bf16 in float32-KV, batch 8 with
1024-token prompts decoded over 77 steps (KV 1024 -> 1100).

The device test IS tests/test_gpu_golden_wide.py::test_device_matches_oracle_at_production_width -- the same function, pointed
at these files and at the checkpoints of this family -- so the assertions, ENVELOPE_FACTOR and MEAN_FACTOR are its own.  The
oracle ran the Llama form of the checkpoint; the device loads the Phi-3 form (fused qkv_proj / gate_up_proj), built here from
the same seed.  Also at this width: block-paged == contiguous bit for bit (that file's test).  The file checks run without a
device.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

D96 = Path(__file__).resolve().parent / "golden" / "d96"
sys.path.insert(0, str(D96))

import make_golden_d96 as gen  # noqa: E402
import test_golden as cpu_golden  # noqa: E402
import test_gpu_golden_wide as wide  # noqa: E402
import wide_models  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402

gpu = pytest.mark.gpu
WIDE = sorted(D96.glob("wide_*.npz"))
REQUIRED = {"wide_phi3_mini_int4_modelkv", "wide_phi3_mini_int4_paged", "wide_phi3_mini_bf16_paged"}


class _Checkpoints(wide._Checkpoints):
    """tests/test_gpu_golden_wide.py's holder of one checkpoint + engine at a time, building this family's checkpoints in
    Phi-3 form."""

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
            self.cfg = gen.build_checkpoint(self.dir, family, precision, seed, phi3=True)
            assert self.cfg["model_type"] == "phi3"
            self.key = key
        if self.model is None:
            self.model = utils.load_model(str(self.dir), max_positions=wide_models.MAX_POS)
        return self.model, self.cfg


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    c = _Checkpoints(tmp_path_factory.mktemp("phi3_wide"))
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the files (no device)

def test_wide_phi3_files_present_with_their_envelopes(monkeypatch):
    assert REQUIRED <= {p.stem for p in WIDE}, "run tests/golden/d96/make_golden_d96.py --wide --envelope"
    monkeypatch.setattr(wide, "GOLD", D96)
    largest = max(p.stat().st_size for p in D96.parent.glob("wide_*.npz"))
    for p in WIDE:
        spec = json.loads(str(np.load(p)["spec"]))
        assert (spec["family"], spec["B"], spec["L0"], spec["steps"]) == (gen.FAMILY, 8, 1024, 77)
        env = wide.envelope_of(p.stem)
        assert env is not None and env["mean_lp"] > 0, p.stem
        assert p.stat().st_size <= largest and (D96 / "envelope" / p.name).stat().st_size <= largest
        # (the bound tests/test_golden.py holds for the envelopes of the 2-block cases)
        assert env["max_lp"] <= (0.1 if not spec["paged"] else 2e-2), (p.stem, env)


@pytest.mark.parametrize("path", WIDE, ids=[p.stem for p in WIDE])
def test_wide_phi3_files_are_consistent(path):
    cpu_golden.test_wide_golden_files_are_consistent(path)


def test_family_is_the_phi3_mini_layer_shapes():
    kw = gen.model_kwargs("int4", 81)
    assert (kw["hidden_size"], kw["heads"], kw["kv_heads"], kw["head_dim"], kw["intermediate_size"], kw["vocab_size"]) == \
        (3072, 32, 32, 96, 8192, 32064)
    assert (kw["rms_norm_eps"], kw["rope_theta"], kw["tie_word_embeddings"], kw["layers"]) == (1e-5, 10000.0, False, 2)
    p = gen.phi3_kwargs(kw)
    assert p["model_type"] == "phi3" and "head_dim" not in p


# ---------------------------------------------------------------------------------------------------------------------------
# the device

@gpu
@pytest.mark.parametrize("path", WIDE, ids=[p.stem for p in WIDE])
def test_device_matches_oracle_at_phi3_mini_width(checkpoints, path, monkeypatch):
    monkeypatch.setattr(wide, "GOLD", D96)
    wide.test_device_matches_oracle_at_production_width(checkpoints, path)


@gpu
@pytest.mark.parametrize("kvd", ["model", "float32"])
def test_block_paged_arena_is_bit_identical_to_contiguous_kv(checkpoints, kvd):
    wide.test_block_paged_arena_is_bit_identical_to_contiguous_kv_at_production_width(checkpoints, gen.FAMILY, "int4", 81, False, kvd)
