"""-m gpu: ``--fork-choices`` on a real engine.  The app is built in-process from the CLI's own parse of the flag (so that the
scheduler's counters can be read): the n = 4 choices of a completion and of a chat completion come from one prompt prefill and
three forked KV rows; with the flag off the same requests fork nothing."""
import asyncio

import httpx
import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.cli import parse_args  # noqa: E402
from mlx_parallm_amd.server import main as srv  # noqa: E402
from mlx_parallm_amd.server.state import model_registry  # noqa: E402
from mlx_parallm_amd.tokenizer_utils import load_tokenizer  # noqa: E402

MODEL_ID = "tiny-fork-model"
PROMPT = "Write one sentence about the sea, then another one about the sky above it."
CHAT = [{"role": "user", "content": "Name three colours and say which one you like best."}]


@pytest.fixture(scope="module")
def parts(tiny_dirs):
    d = tiny_dirs["llama_f32"][0]
    model = utils.load_model(d, max_positions=512)
    yield model, load_tokenizer(d)
    model.engine.close()


def _serve(parts, *flags):
    utils._kv_pool._pool.clear()
    model_registry.clear()
    config = parse_args(["--model-path", MODEL_ID, "--scheduler", "continuous", "--max-batch-size", "4", *flags])
    return config, srv.create_app(config, model=parts[0], tokenizer=parts[1], model_id=MODEL_ID)


def test_n_choices_share_one_prefill_under_fork_choices(parts):
    model, tok = parts

    async def go():
        config, app = _serve(parts, "--fork-choices")
        assert config.fork_choices is True
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://s", timeout=120) as c:
                sched = app.state.server.scheduler
                assert sched.replicas[0].fork_choices and sched.forks == 0
                greedy = {"model": MODEL_ID, "prompt": PROMPT, "max_tokens": 8, "temperature": 0.0, "seed": 11, "logprobs": 1}
                one = (await c.post("/v1/completions", json=greedy)).json()
                assert sched.forks == 0                                      # n == 1: no group
                n_prompt = one["usage"]["prompt_tokens"]
                assert n_prompt >= len(tok._tokenizer.tokenize(PROMPT)) >= 10
                r = await c.post("/v1/completions", json=dict(greedy, n=4))
                assert r.status_code == 200, r.text[:500]
                j = r.json()
                assert [ch["index"] for ch in j["choices"]] == [0, 1, 2, 3]
                assert j["usage"]["prompt_tokens"] == n_prompt      # that of one prompt
                assert sched.forks == 3 and sched.fork_tokens == 3 * (n_prompt - 1)
                want = one["choices"][0]["logprobs"]["tokens"]
                assert len(want) >= 1
                for ch in j["choices"]:                                      # greedy: every choice is the n = 1 answer, id for id
                    assert ch["logprobs"]["tokens"] == want and ch["text"] == one["choices"][0]["text"]
                    assert ch["finish_reason"] == one["choices"][0]["finish_reason"]
                # seeded sampling: choice i draws from the stream of seed + i, from its own first token on
                hot = {"model": MODEL_ID, "prompt": PROMPT, "max_tokens": 8, "temperature": 0.9, "top_p": 0.95, "seed": 3, "n": 4}
                a, b = (await c.post("/v1/completions", json=hot)).json(), (await c.post("/v1/completions", json=hot)).json()
                assert sched.forks == 9 and len(a["choices"]) == 4
                assert [ch["text"] for ch in a["choices"]] == [ch["text"] for ch in b["choices"]]
                assert a["usage"]["prompt_tokens"] == n_prompt
                # chat
                chat = {"model": MODEL_ID, "messages": CHAT, "max_tokens": 8, "temperature": 0.0, "seed": 5}
                c1 = (await c.post("/v1/chat/completions", json=chat)).json()
                r = await c.post("/v1/chat/completions", json=dict(chat, n=4))
                assert r.status_code == 200, r.text[:500]
                c4 = r.json()
                assert sched.forks == 12 and len(c4["choices"]) == 4
                assert c4["usage"]["prompt_tokens"] == c1["usage"]["prompt_tokens"]
                assert c4["usage"]["completion_tokens"] == 4 * c1["usage"]["completion_tokens"]
                for ch in c4["choices"]:
                    assert ch["message"]["content"] == c1["choices"][0]["message"]["content"]
                    assert ch["finish_reason"] == c1["choices"][0]["finish_reason"]
                return one, c1

    one, c1 = asyncio.run(go())

    async def off():
        config, app = _serve(parts)
        assert config.fork_choices is False
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://s", timeout=120) as c:
                sched = app.state.server.scheduler
                r = await c.post("/v1/completions", json={"model": MODEL_ID, "prompt": PROMPT, "max_tokens": 8, "temperature": 0.0,
                                                          "seed": 11, "logprobs": 1, "n": 4})
                assert r.status_code == 200 and len(r.json()["choices"]) == 4
                assert all(ch["logprobs"]["tokens"] == one["choices"][0]["logprobs"]["tokens"] for ch in r.json()["choices"])
                r = await c.post("/v1/chat/completions", json={"model": MODEL_ID, "messages": CHAT, "max_tokens": 8,
                                                               "temperature": 0.0, "seed": 5, "n": 4})
                assert r.status_code == 200 and len(r.json()["choices"]) == 4
                assert sched.forks == 0 and sched.fork_tokens == 0 and not sched.replicas[0].fork_choices

    asyncio.run(off())
