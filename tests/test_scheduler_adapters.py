"""Per-request LoRA adapters in the continuous scheduler and the server, on CPU: the device engine is the oracle-backed fake of
fake_adapter_engine.py, whose KV rows name an adapter slot and whose steps run every row on the oracle of the row's adapter.

  * the adapter is set on the row right after its reset and ahead of the prefix lookup (K / V depend on it);
  * it is gone when the row is recycled: the next occupant runs the base model;
  * the n choices of a request share it, so --fork-choices keeps forking;
  * a `model` that is neither the base model nor a LoRA module is refused as an unknown model is today (404);
  * the paths outside the scheduler (windowed workers, exclusive logprobs / echo, perplexity) answer a LoRA module with 400."""
import asyncio
import threading
from contextlib import asynccontextmanager

import httpx
import numpy as np
import pytest

import row_adapter_cases as cases
from fake_adapter_engine import AdapterEngine, PlainKVEngine, adapter_model
from mlx_parallm_amd import cli, utils
from mlx_parallm_amd.server import main as srv
from mlx_parallm_amd.server.scheduler import ContinuousScheduler, new_group
from mlx_parallm_amd.server.state import model_registry
from mlx_parallm_amd.tokenizer_utils import load_tokenizer

MODEL_ID = "tiny-adapter-model"
P, NEW = 24, 6


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(model directory, {adapter name: directory})"""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    root = tmp_path_factory.mktemp("sched_adapters")
    cfg = build_tiny_model(root / "tiny", seed=6, vocab_size=320, hidden_size=32, layers=2, heads=2, kv_heads=2,
                           intermediate_size=64, quantize_model=False, dtype="float32")
    return str(root / "tiny"), {a: cases.write(root / a, cfg, a) for a in ("P", "Q")}


@pytest.fixture(scope="module")
def tok(tiny):
    return load_tokenizer(tiny[0])


def _prompt(tok, n=P, k=7):
    ids = [5 + (k * i) % 300 for i in range(n)]
    return [t if t != tok.eos_token_id else 4 for t in ids]


def _greedy(ref, prompt, n, eos):
    """what a sequence on this oracle generates: greedy, up to n tokens, ending at EOS"""
    cache = ref.make_cache(1, paged=False)
    y, out = np.asarray(prompt, dtype=np.int32)[None], []
    for _ in range(n):
        t = int(np.argmax(ref(y, cache=cache)[0, -1]))
        out.append(t)
        if t == eos:
            break
        y = np.asarray([[t]], dtype=np.int32)
    return out


def _run(sched, submits):
    """submits: kwargs of ContinuousScheduler.submit without the sink -> [(generated ids, finish reason)] in that order"""
    done, ev = {}, threading.Event()

    def sink_for(i):
        def sink(seq, delta, reason):
            if reason is not None:
                done[i] = (list(seq.generated), reason)
                if len(done) == len(submits):
                    ev.set()
        return sink

    for i, kw in enumerate(submits):
        sched.submit(kw.pop("prompt"), kw.pop("max_tokens", NEW), 0.0, 1.0, sink_for(i), **kw)
    sched.start()
    assert ev.wait(timeout=120), "a sequence never finished"
    sched.stop()
    return [done[i] for i in range(len(submits))]


def _model(tiny, engine_class=AdapterEngine):
    return adapter_model(tiny[0], {0: tiny[1]["P"], 1: tiny[1]["Q"]}, engine_class)


@pytest.mark.parametrize("chunk", [0, 16])
def test_rows_of_one_step_run_their_own_adapters(tiny, tok, chunk):
    model = _model(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=3, chunk_tokens=chunk)
    prompt = _prompt(tok)
    outs = _run(sched, [dict(prompt=prompt, adapter=0), dict(prompt=prompt, adapter=1), dict(prompt=prompt)])
    want = [_greedy(model.engine.refs[s], prompt, NEW, tok.eos_token_id) for s in (0, 1, -1)]
    assert [o[0] for o in outs] == want
    assert len({tuple(w) for w in want}) == 3                   # (the adapters move the greedy ids: a mix-up would show)
    assert sched.max_rows_seen == 3 or sched.steps > 0
    # right after the reset, ahead of the prefix lookup; a row without an adapter gets no call at all
    tr = model.engine.trace
    for k, e in enumerate(tr):
        if e[0] == "set_row_adapter":
            assert tr[k - 1] == ("reset_row", e[1]) and tr[k + 1] == ("prefix_attach", e[1], e[2])
    sets = [e for e in tr if e[0] == "set_row_adapter"]
    assert sorted(e[2] for e in sets) == [0, 1]
    assert [e[2] for e in tr if e[0] == "prefix_attach"].count(-1) == 1
    assert sched.kv.adapters == [-1, -1, -1]                    # recycled rows name nothing


def test_a_recycled_row_runs_the_base_model(tiny, tok):
    model = _model(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0)      # one slot: the second request gets the first one's row
    prompt = _prompt(tok)
    outs = _run(sched, [dict(prompt=prompt, adapter=1), dict(prompt=prompt)])
    assert outs[0][0] == _greedy(model.engine.refs[1], prompt, NEW, tok.eos_token_id)
    assert outs[1][0] == _greedy(model.engine.refs[-1], prompt, NEW, tok.eos_token_id)
    assert [e for e in model.engine.trace if e[0] == "set_row_adapter"] == [("set_row_adapter", 0, 1)]


def test_a_contiguous_cache_drops_the_adapter_with_the_sequence(tiny, tok):
    model = _model(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=2, chunk_tokens=0, paged=False)
    _run(sched, [dict(prompt=_prompt(tok), adapter=0)])
    assert sched.kv.adapters == [-1, -1]


@pytest.mark.parametrize("chunk", [0, 16])
def test_the_choices_of_a_group_share_the_adapter_and_still_fork(tiny, tok, chunk):
    model = _model(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=3, chunk_tokens=chunk, fork_choices=True)
    prompt, g = _prompt(tok), new_group()
    outs = _run(sched, [dict(prompt=prompt, adapter=1, group=g) for _ in range(3)])
    want = _greedy(model.engine.refs[1], prompt, NEW, tok.eos_token_id)
    assert [o[0] for o in outs] == [want] * 3
    assert sched.forks == 2 and [f[2] for f in sched.kv.forks] == [P - 1] * 2       # (the fake refuses a fork across adapters)
    tr = model.engine.trace
    for k, e in enumerate(tr):                                                      # reset, adapter, fork: nothing between
        if e[0] == "fork_row":
            assert tr[k - 2] == ("reset_row", e[2]) and tr[k - 1] == ("set_row_adapter", e[2], 1)
    assert set(model.engine.ran) == {1}                                             # no token of the request ran on anything else


def test_members_on_different_adapters_do_not_fork(tiny, tok):
    model = _model(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=2, chunk_tokens=0, fork_choices=True)
    prompt, g = _prompt(tok), new_group()
    outs = _run(sched, [dict(prompt=prompt, adapter=0, group=g), dict(prompt=prompt, adapter=1, group=g)])
    assert sched.forks == 0
    assert [o[0] for o in outs] == [_greedy(model.engine.refs[s], prompt, NEW, tok.eos_token_id) for s in (0, 1)]


def test_submit_refuses_what_the_cache_cannot_do(tiny, tok):
    sched = ContinuousScheduler(_model(tiny), tok, max_slots=1)
    for bad in (-2, 16, True, 1.0, "p"):
        with pytest.raises(ValueError, match="adapter"):
            sched.submit(_prompt(tok), NEW, 0.0, 1.0, lambda *a: None, adapter=bad)
    plain = ContinuousScheduler(_model(tiny, PlainKVEngine), tok, max_slots=1)
    with pytest.raises(ValueError, match="set_row_adapter"):
        plain.submit(_prompt(tok), NEW, 0.0, 1.0, lambda *a: None, adapter=0)
    assert not sched.pending and not plain.pending


# ------------------------------------------------------------------------------------ the server
@asynccontextmanager
async def serving(tiny, tok, **cfg):
    utils._kv_pool._pool.clear()
    model_registry.clear()
    model = adapter_model(tiny[0], {0: tiny[1]["P"], 1: tiny[1]["Q"]})
    config = srv.ServerConfig(model_path=MODEL_ID, batch_timeout=0.05, lora_modules={"p": tiny[1]["P"], "q": tiny[1]["Q"]}, **cfg)
    app = srv.create_app(config, model=model, tokenizer=tok, model_id=MODEL_ID)
    async with app.router.lifespan_context(app):
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://server", timeout=120) as c:
            yield c, app.state.server, model
    assert "p" not in model_registry and "q" not in model_registry


def test_server_routes_the_model_name_to_the_adapter(tiny, tok):
    """Three concurrent greedy requests with one prompt name p, q and the base model: the ids of the three oracles."""
    prompt = "the quick brown fox"

    async def go():
        async with serving(tiny, tok, scheduler="continuous", max_batch_size=4) as (c, state, model):
            names = [m["id"] for m in (await c.get("/v1/models")).json()["data"]]
            assert sorted(names) == sorted([MODEL_ID, "p", "q"])
            # every entry of both adapter files went into slots 0 and 1, each slot cleared first
            assert [e for e in model.engine.loaded if e[0] == "clear"] == [("clear", 0), ("clear", 1)]
            assert sum(1 for e in model.engine.loaded if e[0] == 0) == 14 and sum(1 for e in model.engine.loaded if e[0] == 1) == 14
            body = dict(prompt=prompt, max_tokens=8, temperature=0.0)
            rs = await asyncio.gather(*[c.post("/v1/completions", json=dict(body, model=m)) for m in ("p", "q", MODEL_ID)])
            assert [r.status_code for r in rs] == [200, 200, 200]
            ids = tok.encode(prompt)
            for r, slot, name in zip(rs, (0, 1, -1), ("p", "q", MODEL_ID)):
                want = _greedy(model.engine.refs[slot], ids, 8, tok.eos_token_id)
                want = want[:-1] if want[-1] == tok.eos_token_id else want
                assert r.json()["model"] == name and r.json()["choices"][0]["text"] == tok.decode(want), name
            chat = await c.post("/v1/chat/completions", json=dict(model="q", max_tokens=4, temperature=0.0,
                                                                  messages=[dict(role="user", content="hi")]))
            assert chat.status_code == 200 and chat.json()["model"] == "q"
            # an unknown name is an unknown model
            r = await c.post("/v1/completions", json=dict(body, model="r"))
            assert r.status_code == 404 and "not found" in r.json()["detail"]
            # outside the scheduler's steps a LoRA module is refused: exclusive logprobs + echo, perplexity
            r = await c.post("/v1/completions", json=dict(body, model="p", logprobs=2, echo=True))
            assert r.status_code == 400 and "continuous scheduler" in r.json()["detail"]
            r = await c.post("/v1/perplexity", json=dict(model="p", text="a b c"))
            assert r.status_code == 400 and "continuous scheduler" in r.json()["detail"]
            assert (await c.post("/v1/perplexity", json=dict(model=MODEL_ID, text="a b c"))).status_code == 200
    asyncio.run(go())


def test_windowed_paths_answer_a_lora_module_with_400(tiny, tok):
    async def go():
        async with serving(tiny, tok, scheduler="default") as (c, state, model):
            assert state.scheduler is None and state.adapters == {"p": 0, "q": 1}
            body = dict(model="p", prompt="hello", max_tokens=4, temperature=0.0)
            chat = dict(model="q", max_tokens=4, messages=[dict(role="user", content="hi")])
            for path, payload in (("/v1/completions", body), ("/v1/completions", dict(body, stream=True)),
                                  ("/v1/chat/completions", chat), ("/v1/chat/completions", dict(chat, stream=True)),
                                  ("/v1/completions", dict(body, logprobs=1)), ("/v1/perplexity", dict(model="p", text="a b"))):
                r = await c.post(path, json=payload)
                assert r.status_code == 400 and "continuous scheduler" in r.json()["detail"], (path, payload, r.status_code)
            assert (await c.post("/v1/completions", json=dict(body, model=MODEL_ID))).status_code == 200
    asyncio.run(go())


def test_lora_path_and_lora_modules_exclude_each_other(tiny, tok):
    with pytest.raises(ValueError, match="cannot be combined"):
        srv.create_app(srv.ServerConfig(model_path=MODEL_ID, lora_path="x", lora_modules={"p": "y"}))
    with pytest.raises(SystemExit):
        cli.parse_args(["--model-path", "m", "--lora-path", "x", "--lora-modules", "p=y"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--model-path", "m", "--lora-modules", "p"])
    c = cli.parse_args(["--model-path", "m", "--lora-modules", "p=/a", "q=/b", "--scheduler", "continuous"])
    assert c.lora_modules == {"p": "/a", "q": "/b"} and c.lora_path is None
    assert cli.parse_args(["--model-path", "m", "--lora-path", "x"]).lora_path == "x"
