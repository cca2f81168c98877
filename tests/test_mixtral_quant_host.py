"""The twin on a quantised tiny Mixtral (CPU): both name forms give the same logits, not the dense twin's, and the inputs that
tests/test_gpu_mixtral_quant.py shares (MODELS, greedy_run) keep its router margins above moe_ref.margin_shortfall's bound."""
import numpy as np
import pytest

import moe_q_ref
import moe_ref
from mlx_parallm_amd.tiny_model import build_tiny_model

B = 4
MODELS = {name: dict(model_type="mixtral", vocab_size=1024, dtype=dtype, q_bits=bits, hidden_size=128, layers=2, heads=4, kv_heads=2,
                     intermediate_size=256, tie_word_embeddings=False, with_tokenizer=False, max_position_embeddings=256,
                     num_local_experts=E, router_gain=4.0, seed=seed)
          for name, E, bits, dtype, seed in (("e4_int4", 4, 4, "bfloat16", 4), ("e8_int8", 8, 8, "float16", 1))}


def greedy_run(ref, paged):
    """The twin's prefill of 4 tokens + 8 greedy steps of B rows -> per step (the tokens fed, float64 log-softmax (B, V))."""
    cache, out = ref.make_cache(B, paged=paged), []
    y = np.random.default_rng(31).integers(3, 1024, size=(B, 4)).astype(np.int32)
    for _ in range(9):
        lg = ref(y, cache=cache)[:, -1].astype(np.float64)
        out.append((y, lg - lg.max(-1, keepdims=True) - np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True))))
        y = out[-1][1].argmax(-1)[:, None].astype(np.int32)
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_twin_reads_both_name_forms_and_keeps_its_margins(tmp_path, name):
    kw = MODELS[name]
    build_tiny_model(tmp_path / "st", **kw)
    build_tiny_model(tmp_path / "per", expert_names="per_expert", **kw)
    build_tiny_model(tmp_path / "dense", **dict(kw, quantize_model=False))
    st, per, dense = moe_q_ref.load(str(tmp_path / "st")), moe_q_ref.load(str(tmp_path / "per")), moe_ref.load(str(tmp_path / "dense"))
    (_y, a), (_y, b), (_y, c) = (greedy_run(m, True)[0] for m in (st, per, dense))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    for paged in (True, False):
        st.margins.clear()
        greedy_run(st, paged)
        assert moe_ref.margin_shortfall(st, kw["dtype"], paged) <= 0
