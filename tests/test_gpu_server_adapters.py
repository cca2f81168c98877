"""-m gpu: ``--lora-modules`` on a real engine.  The app is built in-process from the CLI's own parse of the flag: three
concurrent greedy requests with one prompt name the LoRA modules p and q and the base model, share the continuous scheduler's
steps, and each returns the greedy ids of the oracle loaded with its adapter.  A tiny float32 model, so the KV cache is float32
and the ids are compared exactly."""
import asyncio

import httpx
import numpy as np
import pytest

import row_adapter_cases as cases
from oracle import ref_generate

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.cli import parse_args  # noqa: E402
from mlx_parallm_amd.server import main as srv  # noqa: E402
from mlx_parallm_amd.server.state import model_registry  # noqa: E402
from mlx_parallm_amd.tokenizer_utils import load_tokenizer  # noqa: E402

MODEL_ID = "tiny-adapters-model"
PROMPT = "Write one sentence about the sea, then another one about the sky above it."
NEW = 8


def _greedy(ref, ids, n, eos):
    cache = ref.make_cache(1, paged=False)
    y, out = np.asarray(ids, dtype=np.int32)[None], []
    for _ in range(n):
        t = int(np.argmax(ref(y, cache=cache)[0, -1]))
        out.append(t)
        if t == eos:
            break
        y = np.asarray([[t]], dtype=np.int32)
    return out


def test_three_requests_three_adapters_one_batch(tiny_dirs, tmp_path):
    d, cfg = tiny_dirs["llama_f32"]
    dirs = {"p": cases.write(tmp_path / "p", cfg, "P"), "q": cases.write(tmp_path / "q", cfg, "Q")}
    tok = load_tokenizer(d)
    ids = tok.encode(PROMPT)
    refs = {"p": ref_generate.load(d, adapter_path=dirs["p"], max_pos=512), "q": ref_generate.load(d, adapter_path=dirs["q"], max_pos=512),
            MODEL_ID: ref_generate.load(d, max_pos=512)}
    want = {name: _greedy(ref, ids, NEW, tok.eos_token_id) for name, ref in refs.items()}
    assert len({tuple(w) for w in want.values()}) == 3, want             # the adapters move the greedy ids: a mix-up would show
    model = utils.load_model(d, max_positions=512)
    utils._kv_pool._pool.clear()
    model_registry.clear()
    config = parse_args(["--model-path", MODEL_ID, "--scheduler", "continuous", "--max-batch-size", "4",
                         "--lora-modules", f"p={dirs['p']}", f"q={dirs['q']}"])
    assert config.lora_modules == dirs
    app = srv.create_app(config, model=model, tokenizer=tok, model_id=MODEL_ID)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://s", timeout=120) as c:
                listed = [m["id"] for m in (await c.get("/v1/models")).json()["data"]]
                assert sorted(listed) == sorted([MODEL_ID, "p", "q"])
                body = {"prompt": PROMPT, "max_tokens": NEW, "temperature": 0.0, "logprobs": 1}
                names = ["p", "q", MODEL_ID]
                rs = await asyncio.gather(*[c.post("/v1/completions", json=dict(body, model=m)) for m in names])
                sched = app.state.server.scheduler
                for name, r in zip(names, rs):
                    assert r.status_code == 200, r.text[:500]
                    got = r.json()["choices"][0]["logprobs"]["tokens"]
                    assert got == list(tok._tokenizer.convert_ids_to_tokens(want[name])), (name, got, want[name])
                    assert r.json()["model"] == name
                assert sched.max_rows_seen >= 2                              # they did share steps
                r = await c.post("/v1/completions", json=dict(body, model="r"))
                assert r.status_code == 404

    try:
        asyncio.run(go())
    finally:
        model.engine.close()
