"""Tiny llama checkpoints at 4 / 8 bits in quantisation groups of 32 and 128 through the engine (-m gpu): a batch of 3
left-padded prompts of 140 tokens (420 rows: the prefill goes through the [hi | lo] copy of the new blocks), then 16
teacher-forced greedy steps (gemm_qg.hip in the 16-bit mode, the generic kernel on the same blocks in the float32-KV mode), tied
embedding (the gather reads the blocks).  The oracle loads the same directory (oracle/ref_generate.load honours group_size).
Bounds: those of tests/test_gpu_q36_models.py::_check."""
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from oracle import ref_generate  # noqa: E402
from test_gpu_q36_models import SHAPE, _adapter, _check  # noqa: E402


@pytest.mark.parametrize("mode", ["model", "float32"])
@pytest.mark.parametrize("bits,group,dtype,lora", [(4, 32, "bfloat16", True), (4, 128, "bfloat16", False), (8, 32, "float16", False),
                                                   (8, 128, "bfloat16", False)])
def test_tiny_llama(tmp_path, bits, group, dtype, lora, mode):
    cfg = build_tiny_model(tmp_path / "q", seed=bits + group, dtype=dtype, quantize_model=True, q_bits=bits, q_group_size=group, **SHAPE)
    assert cfg["quantization"] == {"group_size": group, "bits": bits}
    ad = _adapter(tmp_path / "adapter", cfg) if lora else None
    model = utils.load_model(Path(tmp_path / "q"), max_positions=512)
    if lora:
        utils.load_adapters(model, ad)
    ref = ref_generate.load(str(tmp_path / "q"), adapter_path=ad, max_pos=512)
    _check(model, ref, cfg, mode)
    model.engine.close()
