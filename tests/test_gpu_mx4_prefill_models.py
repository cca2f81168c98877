"""Tiny mxfp4 checkpoints through the engine with the prefill on the packed-weight tile GEMM (-m gpu): option
"quant_prefill_tile" set to 1, 3 left-padded prompts of 140 tokens = 420 rows through qtile_mx4_kernel (gemm_qtile.hip; LoRA'd
matrices store and take their term afterwards, phi3 runs its fused qkv and gate_up), then 16 teacher-forced steps.  The
float32-KV mode does not take the route.  Checkpoints: tests/test_gpu_mx4_models.py::_pair; bounds:
tests/test_gpu_q36_models.py::_check, unchanged."""
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from oracle import ref_generate  # noqa: E402
from test_gpu_mx4_models import _pair  # noqa: E402
from test_gpu_q36_models import _adapter, _check  # noqa: E402


@pytest.mark.parametrize("model_type,lora,mode", [("llama", False, "model"), ("llama", True, "model"), ("phi3", False, "model"),
                                                  ("llama", False, "float32")])
def test_tiny_models(tmp_path, model_type, lora, mode):
    a, b, cfg = _pair(tmp_path, model_type)
    ad = _adapter(tmp_path / "adapter", cfg) if lora else None
    model = utils.load_model(Path(a), max_positions=512)
    model.engine.set_option("quant_prefill_tile", 1)
    if lora:
        utils.load_adapters(model, ad)
    _check(model, ref_generate.load(str(b), adapter_path=ad, max_pos=512), cfg, mode)
    model.engine.close()
