"""Logprobs requests under the continuous scheduler, on CPU: the sequences' per-token lists, the row settings' life cycle and
the server route, with the device engine replaced by an oracle-backed fake that scores every sampled row from the reference
model and records ``set_row_logprobs``.  The GPU side of the same contract: test_gpu_row_logprobs.py,
test_gpu_server_logprobs.py."""
import asyncio
import json
import threading

import httpx
import numpy as np
import pytest

from fake_engine import FakeEngine, FakeModel, FakeSlotKV
from mlx_parallm_amd import utils
from mlx_parallm_amd.server import main as srv
from mlx_parallm_amd.server.scheduler import ContinuousScheduler
from mlx_parallm_amd.server.schemas import CompletionRequest
from mlx_parallm_amd.server.state import model_registry
from mlx_parallm_amd.tokenizer_utils import load_tokenizer
from oracle import ref_generate, ref_sample

MODEL_ID = "tiny-logprobs-model"
STRIDE = 20


class LpKV(FakeSlotKV):
    """Row-subset KV of the fake with the two per-row tables of the device cache: logit_bias and the logprobs settings."""

    def __init__(self, engine, batch_size):
        super().__init__(engine, batch_size)
        self.lp, self.bias = {}, {}

    def set_row_logprobs(self, row, top_logprobs, at_temperature=False):
        if not 0 <= int(row) < self.batch_size or not 0 <= int(top_logprobs) <= STRIDE:
            raise ValueError("set_row_logprobs: bad argument")
        self.engine.trace.append(("set_row_logprobs", int(row), int(top_logprobs), bool(at_temperature)))
        if int(top_logprobs) == 0 and not at_temperature:
            self.lp.pop(int(row), None)
        else:
            self.lp[int(row)] = (int(top_logprobs), bool(at_temperature))

    def set_row_logit_bias(self, row, bias):
        self.bias[int(row)] = dict(bias or {})

    def reset_row(self, row):
        super().reset_row(row)
        self.lp.pop(int(row), None)
        self.bias.pop(int(row), None)


class LpEngine(FakeEngine):
    """FakeEngine whose row-subset and mixed steps report what the device sampler reports: the sampled token's logprob
    (under softmax(logits / T) for a row whose setting says so), the fixed-stride top lists with (-1, -inf) behind a row's
    count, and per-row random streams (a seeded row draws from (seed, position), whoever shares the step)."""

    def new_kv(self, batch_size, capacity=256, kv_dtype="model", step=256):
        return LpKV(self, batch_size)

    def _sample(self, kv, rows, logits, sample):
        c = sample.c
        n = len(rows)
        temps, top_ps = getattr(sample, "_row", ([float(c.temperature)] * n, [float(c.top_p)] * n))
        seeds, positions = getattr(sample, "_row_streams", ([0] * n, [-1] * n))
        toks, lps = [], []
        top_i = np.full((n, STRIDE), -1, np.int32)
        top_l = np.full((n, STRIDE), -np.inf, np.float32)
        for i, r in enumerate(rows):
            u = None
            if temps[i] != 0:
                key = [int(seeds[i]), int(positions[i])] if positions[i] >= 0 else [int(c.seed), self._next, i]
                u = np.random.default_rng(key).random(1)
            k, at = kv.lp.get(r, (0, False))
            s = ref_sample.sample(logits[i], temp=float(temps[i]), top_p=float(top_ps[i]), uniforms=u,
                                  logit_bias=kv.bias.get(r), logprobs_at_temperature=at)
            toks.append(int(s["tokens"][0, 0])); lps.append(float(s["logprobs"][0]))
            lsm = s["log_softmax"][0]
            order = np.lexsort((np.arange(lsm.shape[0]), -lsm))[:k]         # (value descending, id ascending)
            top_i[i, :k], top_l[i, :k] = order, lsm[order]
        t = self._next
        self._next += 1
        res = {"tokens": np.asarray(toks, np.int32), "logprobs": np.asarray(lps, np.float32), "probs_row0": np.zeros(n, np.float32)}
        if kv.lp:
            res.update(top_ids=top_i, top_logprobs=top_l, top_counts=np.asarray([kv.lp.get(r, (0,))[0] for r in rows], np.int32))
        self._results[t] = res
        return t, toks

    def step_enqueue_rows(self, kv, rows, tokens=None, sample=None):
        rows = [int(r) for r in rows]
        if tokens is None:
            if self._last_tokens is None or len(self._last_tokens) != len(rows):
                raise ValueError("device-resident token feed needs the row set of the previous step")
            tokens = self._last_tokens
            self.trace.append(("enqueue_rows", tuple(rows), "device-tokens"))
        else:
            tokens = np.asarray(tokens)
            self.trace.append(("enqueue_rows", tuple(rows), tokens.shape))
        logits = [self.ref(tokens[i:i + 1], cache=kv.rows[r])[:, -1] for i, r in enumerate(rows)]
        t, toks = self._sample(kv, rows, logits, sample)
        self._last_tokens = np.asarray(toks)[:, None]
        return t

    def step_enqueue_mixed(self, kv, rows, token_lists, want=None, sample=None):
        rows = [int(r) for r in rows]
        want = [1] * len(rows) if want is None else [int(w) for w in want]
        self.trace.append(("enqueue_mixed", tuple(rows), tuple(len(t) for t in token_lists), tuple(want)))
        wanted, logits = [], []
        for r, tk, w in zip(rows, token_lists, want):
            lg = self.ref(np.asarray(tk).reshape(1, -1), cache=kv.rows[r])[:, -1]
            if w:
                wanted.append(r); logits.append(lg)
        self._last_tokens = None
        if not wanted:
            t = self._next
            self._next += 1
            self._results[t] = {"tokens": np.zeros(0, np.int32), "logprobs": np.zeros(0, np.float32)}
            return t
        return self._sample(kv, wanted, logits, sample)[0]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("sched_lp") / "tiny"
    build_tiny_model(d, seed=6, vocab_size=320, hidden_size=32, layers=2, heads=2, kv_heads=2,
                     intermediate_size=64, quantize_model=False, dtype="float32")
    return str(d)


@pytest.fixture()
def parts(tiny):
    utils._kv_pool._pool.clear()
    model_registry.clear()
    model = FakeModel(tiny, max_pos=2048)
    model.engine = LpEngine(model.ref)
    return model, load_tokenizer(tiny)


def _alone(tiny, ids, n, eos):
    ref = ref_generate.load(tiny, max_pos=2048)
    out = []
    for (t, _), _ in zip(ref_generate.generate_step(np.asarray(ids)[None], ref, paged=False), range(n)):
        if int(t[0, 0]) == eos:
            return out, "stop"
        out.append(int(t[0, 0]))
    return out, "length"


def _teacher_forced(tiny, prompt, generated, temp=None):
    """float64 log-softmax rows (of logits / temp when given) of every sampled position."""
    ref = ref_generate.load(tiny, max_pos=2048)
    seq = np.concatenate([np.asarray(prompt), np.asarray(generated[:-1], dtype=np.int64)]).astype(np.int32)[None]
    lg = np.asarray(ref(seq, cache=ref.make_cache(1, paged=False)), np.float32)[0, len(prompt) - 1:]
    if temp:
        lg = lg * np.float32(1.0 / temp)
    return ref_sample.log_softmax(lg)


def _run(sched, jobs, timeout=120):
    """Submit every (name, prompt, max_tokens, temp, top_p, controls); -> {name: (sequence, finish reason, text)}."""
    done, ev, texts = {}, threading.Event(), {}

    def sink_for(name):
        def sink(seq, delta, reason):
            texts[name] = texts.get(name, "") + (delta or "")
            if reason is not None:
                done[name] = (seq, reason, texts[name])
                if len(done) == len(jobs):
                    ev.set()
        return sink

    for name, prompt, n, temp, top_p, kw in jobs:
        sched.submit(prompt, n, temp, top_p, sink_for(name), **kw)
    assert ev.wait(timeout=timeout)
    return done


@pytest.mark.parametrize("chunk", [0, 8])
def test_lists_line_up_with_generated_and_settings_follow_the_slot(tiny, parts, chunk):
    model, tok = parts
    sched = ContinuousScheduler(model, tok, max_slots=2, chunk_tokens=chunk)
    sched.start()
    pa, pb, pc = tok.encode("first request, a long one"), tok.encode("second"), tok.encode("the third of them")
    done = _run(sched, [("a", pa, 9, 0.0, 1.0, dict(logprobs=3)),
                        ("b", pb, 7, 0.8, 1.0, dict(logprobs=0, logprobs_at_temperature=True, seed=5)),
                        ("c", pc, 5, 0.0, 1.0, {})])               # c takes over a slot whose setting must be gone
    sched.stop()
    a, b, c = done["a"][0], done["b"][0], done["c"][0]
    assert a.generated == _alone(tiny, pa, 9, tok.eos_token_id)[0] and c.generated == _alone(tiny, pc, 5, tok.eos_token_id)[0]
    for s in (a, b):                                               # (nothing hit EOS on this model)
        assert s.token_ids == s.generated and len(s.token_logprobs) == len(s.generated)
    assert len(a.top) == len(a.generated) and b.top == [] and c.token_ids == [] and c.top == []
    lsm = _teacher_forced(tiny, pa, a.generated)
    for j, (t, lp, (ids, lps)) in enumerate(zip(a.generated, a.token_logprobs, a.top)):
        assert abs(lp - lsm[j, t]) < 1e-5 and ids.shape == (3,) and int(ids[0]) == t          # greedy: the best entry
        assert list(ids) == list(np.lexsort((np.arange(lsm.shape[1]), -lsm[j]))[:3]) and np.allclose(lps, lsm[j, ids], atol=1e-5)
    lsm_t = _teacher_forced(tiny, pb, b.generated, temp=0.8)       # b: under softmax(logits / 0.8)
    assert np.allclose(b.token_logprobs, lsm_t[np.arange(len(b.generated)), b.generated], atol=1e-5)
    # put on at admission, right behind the row's reset and ahead of its first step; gone when the row is reset again
    tr = model.engine.trace
    sets = [e for e in tr if e[0] == "set_row_logprobs" and e[2:] != (0, False)]
    assert sorted(e[2:] for e in sets) == [(0, True), (3, False)]
    assert sorted(e[1] for e in tr if e[0] == "set_row_logprobs" and e[2:] == (0, False)) == sorted(e[1] for e in sets)
    for e in sets:
        i = tr.index(e)
        assert tr[i - 1] == ("reset_row", e[1])
    assert sched.kv.lp == {}                                       # every setting was cleared with its row
    assert sched.borrows == 0


def test_an_eos_that_ends_the_sequence_keeps_its_entry(tiny, parts):
    model, tok = parts
    sched = ContinuousScheduler(model, tok, max_slots=2)
    sched.start()
    eos = tok.eos_token_id
    done = _run(sched, [("a", tok.encode("say something"), 6, 0.0, 1.0, dict(logprobs=2, logit_bias={eos: 1e4}))])
    sched.stop()
    seq, reason, _ = done["a"]
    assert reason == "stop" and seq.generated == [] and seq.token_ids == [eos]
    assert len(seq.token_logprobs) == 1 and seq.token_logprobs[0] > -1e-3 and int(seq.top[0][0][0]) == eos


def test_tokens_behind_a_stop_hit_stay_in_the_lists(tiny, parts):
    model, tok = parts
    p = tok.encode("a prompt whose continuation is cut")
    free = _alone(tiny, p, 12, tok.eos_token_id)[0]
    text = tok.decode(free)
    stop = text[len(text) // 2:len(text) // 2 + 2]
    assert stop
    sched = ContinuousScheduler(model, tok, max_slots=2)
    sched.start()
    seq, reason, out = _run(sched, [("a", p, 12, 0.0, 1.0, dict(logprobs=1, stop=[stop]))])["a"]
    sched.stop()
    assert reason == "stop" and stop not in out and text.startswith(out)
    assert seq.generated == free[:len(seq.generated)] and seq.token_ids == seq.generated
    assert len(seq.token_logprobs) == len(seq.top) == len(seq.generated)
    assert len(tok.decode(seq.generated)) > len(out)               # the tokens of the stop string are counted and listed


def test_engines_without_the_setting_refuse_the_submit(tiny):
    utils._kv_pool._pool.clear()
    model_registry.clear()
    model, tok = FakeModel(tiny, max_pos=2048), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=2)
    with pytest.raises(ValueError, match="set_row_logprobs"):
        sched.submit(tok.encode("x"), 3, 0.0, 1.0, lambda *a: None, logprobs=2)
    with pytest.raises(ValueError, match="logprobs must be"):
        sched.submit(tok.encode("x"), 3, 0.0, 1.0, lambda *a: None, logprobs=21)
    sched.submit(tok.encode("x"), 3, 0.0, 1.0, lambda *a: None)   # (without logprobs: as before)
    sched.stop()


def _events(text):
    ev = [line[len("data: "):] for line in text.splitlines() if line.startswith("data: ")]
    assert ev and ev[-1] == "[DONE]"
    return [json.loads(e) for e in ev[:-1]]


def test_server_logprobs_requests_ride_the_shared_steps(tiny, parts):
    model, tok = parts
    hf = tok._tokenizer

    async def go():
        config = srv.ServerConfig(model_path=MODEL_ID, scheduler="continuous", max_batch_size=4)
        app = srv.create_app(config, model=model, tokenizer=tok, model_id=MODEL_ID)
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://s", timeout=120) as c:
                sched = app.state.server.scheduler
                # ---- a logprobs request arrives while another sequence is mid-generation: nobody takes the engine
                long_prompt = "keep going for a long while"
                long_task = asyncio.create_task(c.post("/v1/completions", json={
                    "model": MODEL_ID, "prompt": long_prompt, "max_tokens": 150, "temperature": 0.0}))
                await asyncio.sleep(0.05)
                body = {"model": MODEL_ID, "prompt": "Hello world", "max_tokens": 6, "temperature": 0.0, "logprobs": 2, "n": 2}
                r = await c.post("/v1/completions", json=body)
                assert r.status_code == 200, r.text[:300]
                assert sched.borrows == 0 and sched.max_rows_seen >= 2
                j = r.json()
                ids = np.asarray(hf(["Hello world"], return_tensors="np")["input_ids"])[0]
                want, reason = _alone(tiny, ids, 6, tok.eos_token_id)
                assert len(j["choices"]) == 2 and j["usage"]["completion_tokens"] == 2 * len(want)
                for ch in j["choices"]:
                    lp = ch["logprobs"]
                    assert ch["finish_reason"] == reason and ch["text"] == tok.decode(want)
                    assert lp["tokens"] == list(hf.convert_ids_to_tokens(want)) and lp["text_offset"] == [0] * len(want)
                    assert len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(want)
                    assert all(len(d) in (1, 2) and max(d, key=d.get) == t for d, t in zip(lp["top_logprobs"], lp["tokens"]))
                lj = (await long_task).json()
                lids = np.asarray(hf([long_prompt], return_tensors="np")["input_ids"])[0]
                assert lj["choices"][0]["text"] == tok.decode(_alone(tiny, lids, 150, tok.eos_token_id)[0])
                assert sched.borrows == 0
                # ---- a greedy request: the tokens and logprobs of the exclusive path on the same fake
                one = dict(body, n=1, logprobs=3, temperature=0.7)         # (temperature > 0, top_p = 1: greedy, logprobs at T)
                got = (await c.post("/v1/completions", json=one)).json()["choices"][0]["logprobs"]
                excl = srv.completion_with_logprobs(model, tok, MODEL_ID, CompletionRequest(**one)).choices[0].logprobs
                assert got["tokens"] == excl["tokens"] and got["text_offset"] == excl["text_offset"]
                assert np.allclose(got["token_logprobs"], excl["token_logprobs"], atol=1e-6)
                for d, e in zip(got["top_logprobs"], excl["top_logprobs"]):
                    assert list(d) == list(e) and np.allclose(list(d.values()), list(e.values()), atol=1e-6)
                assert sched.borrows == 0
                # ---- n = 3 with a seed: three different choices, the same three again
                seeded = dict(body, n=3, seed=11, temperature=1.0, top_p=0.95, max_tokens=8, logprobs=1)
                r1, r2 = (await c.post("/v1/completions", json=seeded)).json(), (await c.post("/v1/completions", json=seeded)).json()
                toks1 = [ch["logprobs"]["tokens"] for ch in r1["choices"]]
                assert toks1 == [ch["logprobs"]["tokens"] for ch in r2["choices"]]
                assert len({tuple(t) for t in toks1}) == 3
                assert [ch["logprobs"]["token_logprobs"] for ch in r1["choices"]] == [ch["logprobs"]["token_logprobs"] for ch in r2["choices"]]
                # ---- stop and logit_bias are honoured
                r = (await c.post("/v1/completions", json=dict(body, n=1, logit_bias={str(int(want[0])): -100}))).json()
                assert r["choices"][0]["logprobs"]["tokens"][0] != hf.convert_ids_to_tokens([int(want[0])])[0]
                assert sched.borrows == 0
                # ---- echo and stream keep the exclusive path; more than 20 stays 400
                r = await c.post("/v1/completions", json=dict(body, n=1, echo=True))
                assert r.status_code == 200 and r.json()["choices"][0]["logprobs"]["tokens"] and sched.borrows == 1
                r = await c.post("/v1/completions", json=dict(body, n=1, stream=True))
                assert r.status_code == 200 and sched.borrows == 2
                assert (await c.post("/v1/completions", json=dict(body, logprobs=21))).status_code == 400
    asyncio.run(go())
