"""-m gpu: ``logit_bias`` and ``stop`` of a request under the continuous scheduler on a real engine, through the server's own
request path (``_submit`` and the scheduled response / stream generators of server/main.py, in this process)."""
import asyncio
import json
import types

import pytest

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.server import main as srv  # noqa: E402
from mlx_parallm_amd.server.scheduler import ContinuousScheduler  # noqa: E402
from mlx_parallm_amd.server.schemas import CompletionRequest  # noqa: E402

N = 16


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """A tiny float32 model with an untied head (its greedy text is not one token repeated) and, as the logit_bias every
    request here carries unless it forces a token, -100 on every id that is not one printable ASCII character: the byte-level
    tokenizer of the tiny models then yields one visible character per token."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("bias_stop") / "tiny"
    cfg = build_tiny_model(d, seed=1, vocab_size=512, dtype="float32", quantize_model=False, tie_word_embeddings=False,
                           norm_jitter=0.1)
    utils._kv_pool.clear()
    model, tok = utils.load(str(d))
    tok = srv._wrap(tok)

    def visible(i):
        s = tok._tokenizer.decode([i])
        return len(s) == 1 and s.isascii() and s.isprintable()

    PRINTABLE.clear()
    PRINTABLE.update({str(i): -100.0 for i in range(cfg["vocab_size"]) if not visible(i)})
    yield model, tok
    utils._kv_pool.clear()
    model.engine.close()


PRINTABLE = {}


def serve(loaded, requests, stream=False):
    """The requests, all queued before the scheduler takes its first step (so they run together) -> the responses, or for
    stream=True the parsed SSE events of each request; and the largest number of rows that shared a step."""
    model, tok = loaded
    sched = ContinuousScheduler(model, tok, max_slots=4, chunk_tokens=16, block_tokens=16, kv_blocks=64, prefix_cache=False)

    async def collect(req):
        events = []
        async for line in srv._scheduled_completion_stream(state, req, tok):
            if line.strip() != "data: [DONE]":
                events.append(json.loads(line[len("data: "):]))
        return events

    async def go():
        state.stream_slots = asyncio.Semaphore(8)
        tasks = [asyncio.ensure_future(collect(r) if stream else srv._scheduled_response(state, r, tok, "m")) for r in requests]
        while len(sched.pending) < len(requests) and not any(t.done() for t in tasks):
            await asyncio.sleep(0)
        sched.start()
        return await asyncio.gather(*tasks)

    state = types.SimpleNamespace(scheduler=sched, config=types.SimpleNamespace(request_timeout_seconds=120))
    try:
        return asyncio.run(go()), sched.max_rows_seen
    finally:
        sched.stop()


def req(prompt, **kw):
    kw.setdefault("logit_bias", dict(PRINTABLE))
    return CompletionRequest(model="m", prompt=prompt, max_tokens=N, temperature=0.0, **kw)


def test_a_forcing_logit_bias_next_to_a_request_with_another_bias(loaded):
    _model, tok = loaded
    tid = int(tok.encode("Z")[-1])
    assert tid != tok.eos_token_id and tok._tokenizer.decode([tid] * N) == "Z" * N
    (solo,), _ = serve(loaded, [req("Someone else")])
    (forced, other), rows = serve(loaded, [req("Once upon a time there was", logit_bias={str(tid): 100.0}), req("Someone else")])
    assert rows == 2                                                   # they shared their steps, each with its own bias
    assert forced.choices[0].text == "Z" * N and forced.usage.completion_tokens == N
    assert other.choices[0].text == solo.choices[0].text and other.choices[0].finish_reason == solo.choices[0].finish_reason
    assert len(solo.choices[0].text) == N and solo.choices[0].text.isprintable() and len(set(solo.choices[0].text)) > 1


def test_stop_ends_before_the_stop_string_streaming_and_not(loaded):
    (free,), _ = serve(loaded, [req("Someone else")])
    full = free.choices[0].text
    assert len(full) == N and len(set(full)) > 1
    # the first pair of characters from the fifth on that does not occur earlier: what precedes it is the expected text
    at = next(i for i in range(4, N - 1) if full.find(full[i:i + 2]) == i)
    stop, want = full[at:at + 2], full[:at]
    (plain, bystander), rows = serve(loaded, [req("Someone else", stop=[stop]), req("Repeat after me")])
    assert rows == 2
    assert plain.choices[0].text == want and plain.choices[0].finish_reason == "stop"
    assert 0 < plain.usage.completion_tokens < N                       # it did not run to its length
    assert bystander.choices[0].finish_reason in ("stop", "length")
    (events, _other), _ = serve(loaded, [req("Someone else", stop=stop, stream=True), req("Repeat after me", stream=True)],
                                stream=True)
    assert all("choices" in e for e in events), events
    assert "".join(e["choices"][0].get("text") or "" for e in events) == want
    assert events[-1]["choices"][0]["finish_reason"] == "stop"
    assert all(e["choices"][0].get("finish_reason") is None for e in events[:-1])


def test_bad_values_are_http_400(loaded):
    from fastapi import HTTPException

    for bad in (req("x", stop=["a", "b", "c", "d", "e"]), req("x", logit_bias={"100000": 1.0})):     # id beyond the vocabulary
        with pytest.raises(HTTPException) as ei:
            serve(loaded, [bad])
        assert ei.value.status_code == 400
