"""-m gpu: ``--lora-modules a=<dora dir> b=<lora dir>`` on a real engine with the continuous scheduler.  Three concurrent greedy
requests with one prompt run on the DoRA module, on the LoRA module and on the base model, share the scheduler's steps, and
each returns the greedy ids of the twin loaded with its adapter (tests/dora_ref.py).  The tiny bf16 Qwen3 checkpoint, served
with the float32 KV cache (what MLX_PARALLM_AMD_KV_DTYPE=float32 selects: the reference's PagedKVCache mode), so the twin runs
its paged cache and the prompt is the first of a fixed list at which every twin's top-2 margin exceeds twice the float32-KV
logit bound (4e-3) at every generated position: ids are compared exactly.  The byte tokenizer names only ids below 259, so
besides the token strings the logprob of every generated id is held to its twin's within the float32-KV bound (1e-3)."""
import asyncio

import httpx
import numpy as np
import pytest

import dora_ref
import test_gpu_dora_models as dm

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.cli import parse_args  # noqa: E402
from mlx_parallm_amd.server import main as srv  # noqa: E402
from mlx_parallm_amd.server.state import model_registry  # noqa: E402
from mlx_parallm_amd.tokenizer_utils import load_tokenizer  # noqa: E402

MODEL_ID = "tiny-dora-model"
PROMPTS = ["Write one sentence about the sea, then another one about the sky above it.",
           "List three colours and say which of them you like best.",
           "The quick brown fox jumps over the lazy dog, twice.",
           "Count from one to five and back again.",
           "Name a river, a mountain and a city."]
NEW = 8
MARGIN, LOGPROB_TOL = 2 * 4e-3, 1e-3


def _greedy(ref, ids, n, eos):
    """-> (ids, the smallest top-2 margin over the generated positions, the logprob of every id)"""
    cache = ref.make_cache(1, paged=True)
    y, out, margin, lps = np.asarray(ids, dtype=np.int32)[None], [], np.inf, []
    for _ in range(n):
        lg = ref(y, cache=cache)[0, -1]
        top2 = np.sort(lg)[-2:]
        margin = min(margin, float(top2[1] - top2[0]))
        t = int(np.argmax(lg))
        l64 = lg.astype(np.float64)
        lps.append(float(l64[t] - l64.max() - np.log(np.exp(l64 - l64.max()).sum())))
        out.append(t)
        if t == eos:
            break
        y = np.asarray([[t]], dtype=np.int32)
    return out, margin, lps


def test_dora_lora_and_base_requests_share_the_batch(tiny_dirs, tmp_path, monkeypatch):
    monkeypatch.setattr(utils, "DEFAULT_KV_DTYPE", "float32")
    d, cfg = tiny_dirs["qwen3_bf16"]
    dirs = {"a": dm.write_adapter(tmp_path / "a", d, cfg, "dora", 16, 5), "b": dm.write_adapter(tmp_path / "b", d, cfg, "lora", 16, 6)}
    tok = load_tokenizer(d)
    refs = {"a": dora_ref.load(d, adapter_path=dirs["a"], max_pos=512), "b": dora_ref.load(d, adapter_path=dirs["b"], max_pos=512),
            MODEL_ID: dora_ref.load(d, max_pos=512)}
    prompt = want = want_lp = None
    for p in PROMPTS:
        runs = {name: _greedy(ref, tok.encode(p), NEW, tok.eos_token_id) for name, ref in refs.items()}
        if min(r[1] for r in runs.values()) > MARGIN and len({tuple(r[0]) for r in runs.values()}) == 3:
            prompt, want, want_lp = p, {name: r[0] for name, r in runs.items()}, {name: r[2] for name, r in runs.items()}
            break
    assert prompt is not None, "no prompt of the list gives three distinct id sequences with margins above the bound"
    model = utils.load_model(d, max_positions=512)
    utils._kv_pool._pool.clear()
    model_registry.clear()
    config = parse_args(["--model-path", MODEL_ID, "--scheduler", "continuous", "--max-batch-size", "4",
                         "--lora-modules", f"a={dirs['a']}", f"b={dirs['b']}"])
    assert config.lora_modules == dirs
    app = srv.create_app(config, model=model, tokenizer=tok, model_id=MODEL_ID)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://s", timeout=120) as c:
                listed = [m["id"] for m in (await c.get("/v1/models")).json()["data"]]
                assert sorted(listed) == sorted([MODEL_ID, "a", "b"])
                body = {"prompt": prompt, "max_tokens": NEW, "temperature": 0.0, "logprobs": 1}
                names = ["a", "b", MODEL_ID]
                rs = await asyncio.gather(*[c.post("/v1/completions", json=dict(body, model=m)) for m in names])
                for name, r in zip(names, rs):
                    assert r.status_code == 200, r.text[:500]
                    got = r.json()["choices"][0]["logprobs"]["tokens"]
                    assert got == list(tok._tokenizer.convert_ids_to_tokens(want[name])), (name, got, want[name])
                    lps = r.json()["choices"][0]["logprobs"]["token_logprobs"]
                    assert len(lps) == len(want_lp[name]) and max(abs(x - y) for x, y in zip(lps, want_lp[name])) <= LOGPROB_TOL, (name, lps, want_lp[name])
                    assert r.json()["model"] == name
                assert app.state.server.scheduler.max_rows_seen >= 2          # they did share steps

    try:
        asyncio.run(go())
    finally:
        model.engine.close()
