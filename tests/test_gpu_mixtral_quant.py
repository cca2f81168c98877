"""Quantised tiny Mixtral checkpoints (int4 E = 4, int8 E = 8, quantised router) on the engine (-m gpu) against the twin
(tests/moe_q_ref.py), under the contract of tests/test_gpu_mixtral_models.py; name forms; the refusals at load."""
import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

import moe_q_ref
from mlx_parallm_amd import utils
from mlx_parallm_amd.engine import SampleArgs
from mlx_parallm_amd.tiny_model import build_tiny_model
from test_gpu_mixtral_models import KVDS, _steps
from test_mixtral_quant_host import B, MODELS, greedy_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("mixtral_q")
    for name, kw in MODELS.items():
        build_tiny_model(root / name, **kw)
        build_tiny_model(root / (name + "_per"), expert_names="per_expert", **kw)
    return {d.name: str(d) for d in root.iterdir()}


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_matches_the_twin(dirs, name, kvd):
    model, ref = utils.load_model(dirs[name], max_positions=256), moe_q_ref.load(dirs[name], max_pos=256)
    try:
        kv = model.engine.new_kv(B, capacity=48, kv_dtype=kvd)
        for s, (y, lp) in enumerate(greedy_run(ref, kvd == "float32")):
            got, want, top2 = model.engine.decode_sample(kv, y, SampleArgs(temp=0.0)), lp.argmax(-1), np.sort(lp, axis=-1)[:, -2:]
            clear = np.ones(B, bool) if kvd == "float32" else (top2[:, 1] - top2[:, 0]) > 0.13
            assert np.array_equal(got["tokens"][clear], want[clear]), (name, kvd, s)
            if kvd == "float32":
                err = np.abs(got["logprobs"] - lp.max(-1)).max()
                print(f"{name} step {s}: max |logprob difference| {err:.3e}")
                assert err <= 1e-3, (name, s, err)
        kv.close()
    finally:
        model.engine.close()


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_stacked_checkpoint_equals_per_expert_checkpoint_bit_for_bit(dirs, name, kvd):
    a, b = utils.load_model(dirs[name], max_positions=256), utils.load_model(dirs[name + "_per"], max_positions=256)
    try:
        for s, (x, y) in enumerate(zip(_steps(a.engine, kvd, 1024), _steps(b.engine, kvd, 1024))):
            assert all(np.array_equal(x[k], y[k]) for k in ("tokens", "logprobs", "top_ids", "top_logprobs")), (name, kvd, s)
    finally:
        a.engine.close(); b.engine.close()


def test_load_errors_name_the_tensor_and_leave_the_process_usable(dirs, tmp_path):
    w = load_file(dirs["e4_int4"] + "/model.safetensors")
    up = "model.layers.1.block_sparse_moe.switch_mlp.up_proj"
    mixed = {k: v for k, v in w.items() if not k.startswith(up + ".")}
    mixed[up + ".weight"] = torch.zeros((4, 256, 128), dtype=torch.bfloat16)            # one dense stack among quantised ones
    short = dict(w, **{up + ".scales": w[up + ".scales"][:, :, :1].contiguous()})       # one group too few
    for d, weights, word in ((tmp_path / "mixed", mixed, "all dense or all quantised"), (tmp_path / "short", short, up + ".scales")):
        d.mkdir()
        save_file(weights, str(d / "model.safetensors"), metadata={"format": "mlx"})
        (d / "config.json").write_text(open(dirs["e4_int4"] + "/config.json").read())
        with pytest.raises(Exception, match=word.replace(".", r"\.")) as info:
            utils.load_model(str(d), max_positions=64)
        assert "block_sparse_moe" in str(info.value)
    build_tiny_model(tmp_path / "dense", **dict(MODELS["e4_int4"], quantize_model=False))
    model = utils.load_model(str(tmp_path / "dense"), max_positions=64)
    try:
        assert len(_steps(model.engine, "model", 1024)) == 15
    finally:
        model.engine.close()
