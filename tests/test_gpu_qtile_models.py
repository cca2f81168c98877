"""Tiny llama checkpoints at 4 and 8 bits, group 64, through the engine with the packed-weight prefill GEMM (-m gpu, option
"quant_prefill_tile" = 1, gemm_qtile.hip): the batch of test_gpu_q36_models.py -- 3 left-padded prompts of 140 tokens, 420 rows, above
the two-slab route -- then 16 teacher-forced greedy steps against the oracle, under that file's bounds.  The float32-KV mode does
not take the route (float32 activations) and must keep meeting its bounds with the option on."""
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.tiny_model import build_tiny_model  # noqa: E402
from oracle import ref_generate  # noqa: E402
from test_gpu_q36_models import SHAPE, _check  # noqa: E402


@pytest.mark.parametrize("bits,dtype,mode", [(4, "bfloat16", "model"), (4, "float16", "model"), (8, "bfloat16", "model"),
                                             (8, "float16", "model"), (4, "bfloat16", "float32")])
def test_tiny_llama(tmp_path, bits, dtype, mode):
    cfg = build_tiny_model(tmp_path / "q", seed=bits, dtype=dtype, quantize_model=True, q_bits=bits, **SHAPE)
    model = utils.load_model(Path(tmp_path / "q"), max_positions=512)
    model.engine.set_option("quant_prefill_tile", 1)
    ref = ref_generate.load(str(tmp_path / "q"), max_pos=512)
    _check(model, ref, cfg, mode)
    model.engine.close()
