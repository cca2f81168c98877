"""Per-request ``logit_bias`` and ``stop`` through the host layers, without a GPU: the ``StopMatcher``, what the continuous
scheduler does with a row's bias between the row's reset and its first sampling step (a recording cache / engine over the
oracle-backed fake), the refusal on a cache without the bias table, and the request schemas / ``_submit``."""
import asyncio
import threading
import types

import numpy as np
import pytest

from fake_engine import FakeEngine, FakeModel, FakeSlotKV
from mlx_parallm_amd.server.schemas import ChatCompletionRequest, ChatMessage, CompletionRequest
from mlx_parallm_amd.server.scheduler import ContinuousScheduler, Sequence, StopMatcher
from mlx_parallm_amd.tokenizer_utils import load_tokenizer


# ---- 1. StopMatcher
def _feed_all(stops, deltas):
    """-> (emitted pieces, hit) after feeding the deltas in order (stopping at the hit), flushing when nothing hit."""
    m, out = StopMatcher(stops), []
    for d in deltas:
        text, hit = m.feed(d)
        out.append(text)
        if hit:
            return out, True
    out.append(m.flush())
    return out, False


def test_stop_string_split_over_three_deltas():
    out, hit = _feed_all(["END"], ["abE", "N", "D and more"])
    assert hit and out == ["ab", "", ""]                       # the "E" and the "N" were held back, never shown


def test_the_earliest_starting_stop_wins_whatever_its_place_in_the_list():
    out, hit = _feed_all(["xyz", "wxy"], ["a wxyz b"])         # "wxy" starts at 2, "xyz" at 3
    assert hit and "".join(out) == "a "
    out, hit = _feed_all(["wxy", "xyz"], ["a wxyz b"])
    assert hit and "".join(out) == "a "


def test_a_held_prefix_that_does_not_complete_is_released():
    m = StopMatcher(["END"])
    assert m.feed("aEN") == ("a", False)
    assert m.feed("x") == ("ENx", False)
    assert m.feed("E") == ("", False)
    assert m.feed("EN") == ("E", False)                        # the first E can no longer start a match, "EN" still can
    assert m.feed("D") == ("", True)
    assert m.feed("more") == ("", True)                        # nothing after the hit


def test_flush_hands_out_the_held_text_at_length_or_eos():
    m = StopMatcher(["</s>", "\n\n"])
    assert m.feed("line\n") == ("line", False)
    assert m.flush() == "\n" and m.flush() == ""
    assert m.feed(None) == ("", False)
    with pytest.raises(ValueError):
        StopMatcher(["ok", ""])


def test_no_emitted_text_contains_or_ends_with_the_start_of_a_completed_stop():
    """Random texts over a small alphabet, cut into random deltas: the emitted text is the text up to the first stop that
    completes (of those completed by the same delta: the earliest start), and every partial emission is a prefix of it."""
    rng = np.random.default_rng(0)
    for _ in range(300):
        stops = ["".join(rng.choice(list("ab"), size=rng.integers(1, 5))) for _ in range(rng.integers(1, 4))]
        text = "".join(rng.choice(list("abc"), size=rng.integers(0, 24), p=[0.35, 0.35, 0.3]))
        cuts = sorted(rng.integers(0, len(text) + 1, size=rng.integers(0, 6)))
        deltas = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
        want, want_hit, seen = text, False, ""
        for d in deltas:                                       # the definition, on the whole text so far
            seen += d
            starts = [seen.find(s) for s in stops if s in seen]
            if starts:
                want, want_hit = seen[:min(starts)], True
                break
        m, got, hit = StopMatcher(stops), "", False
        for d in deltas:
            piece, hit = m.feed(d)
            got += piece
            assert want.startswith(got), (stops, deltas, got, want)
            if hit:
                break
        if not hit:
            got += m.flush()
        assert (got, hit) == (want, want_hit), (stops, deltas)
        if hit:
            assert all(s not in got for s in stops)


# ---- 2. the scheduler over a recording cache
class RecordingKV(FakeSlotKV):
    """FakeSlotKV + the per-row bias table of the engine's cache: reset_row clears the row's bias, like mi_kv_reset_row."""

    def __init__(self, engine, batch_size):
        super().__init__(engine, batch_size)
        self.bias = {}

    def reset_row(self, row):
        super().reset_row(row)
        self.bias.pop(row, None)
        self.engine.events.append(("reset", int(row)))

    def set_row_logit_bias(self, row, bias):
        if bias:
            self.bias[int(row)] = dict(bias)
        else:
            self.bias.pop(int(row), None)
        self.engine.events.append(("bias", int(row), dict(bias or {})))


class RecordingEngine(FakeEngine):
    """Records the cache calls and, per sampling step, the bias in force on every sampled row."""

    def __init__(self, ref_model):
        super().__init__(ref_model)
        self.events = []

    def new_kv(self, batch_size, capacity=256, kv_dtype="model", step=256):
        return RecordingKV(self, batch_size)

    def step_enqueue_rows(self, kv, rows, tokens=None, sample=None):
        self.events.append(("sample", {int(r): dict(kv.bias.get(int(r), {})) for r in rows}))
        return super().step_enqueue_rows(kv, rows, tokens, sample)

    def step_enqueue_mixed(self, kv, rows, token_lists, want=None, sample=None):
        w = [1] * len(rows) if want is None else list(want)
        sampled = {int(r): dict(kv.bias.get(int(r), {})) for r, x in zip(rows, w) if x}
        if sampled:
            self.events.append(("sample", sampled))
        return super().step_enqueue_mixed(kv, rows, token_lists, want, sample)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("rowbias") / "tiny"
    build_tiny_model(d, seed=6, vocab_size=320, hidden_size=32, layers=2, heads=2, kv_heads=2,
                     intermediate_size=64, quantize_model=False, dtype="float32")
    return str(d)


def _model(tiny, engine_cls=RecordingEngine):
    model = FakeModel(tiny, max_pos=2048)
    model.engine = engine_cls(model.ref)
    return model


def _run_all(sched, requests):
    """requests: name -> (prompt, max_tokens, kwargs), all queued before the scheduler starts (admitted in this order)
    -> {name: (Sequence, text, finish_reason)}."""
    out, parts, ev = {}, {n: [] for n in requests}, threading.Event()

    def sink_for(name):
        def sink(seq, delta, reason):
            if delta:
                parts[name].append(delta)
            if reason is not None:
                out[name] = (seq, "".join(parts[name]), reason)
                if len(out) == len(requests):
                    ev.set()
        return sink

    for name, (prompt, max_tokens, kw) in requests.items():
        sched.submit(prompt, max_tokens, 0.0, 1.0, sink_for(name), **kw)
    sched.start()
    assert ev.wait(timeout=120)
    sched.stop()
    return out


@pytest.mark.parametrize("chunk", [0, 8])
def test_bias_is_set_between_the_reset_and_the_first_sampling_step(tiny, chunk):
    """One slot, two requests after each other: the first one's bias reaches the row after the row's reset and before the
    row is sampled (the whole prefill, or the last of its chunks); the second one, without a bias, finds the row cleared."""
    model, tok = _model(tiny), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=chunk)
    prompt = tok.encode("a prompt that is longer than one chunk of eight tokens")
    assert len(prompt) > 8
    bias = {7: 2.5, 300: -100.0}
    out = _run_all(sched, {"a": (prompt, 5, dict(logit_bias=bias)), "b": (prompt, 4, {})})
    assert out["a"][2] == out["b"][2] == "length" and out["a"][0].slot == out["b"][0].slot == 0
    ev = model.engine.events
    sets = [i for i, e in enumerate(ev) if e[0] == "bias"]
    assert len(sets) == 1 and ev[sets[0]] == ("bias", 0, bias)
    resets = [i for i, e in enumerate(ev) if e == ("reset", 0)]
    samples = [i for i, e in enumerate(ev) if e[0] == "sample"]
    assert resets[0] < sets[0] < samples[0]                            # reset, bias, then the row's first sampling step
    second = next(i for i in resets if i > sets[0])                    # b's admission
    a_steps = [ev[i][1] for i in samples if i < second]
    b_steps = [ev[i][1] for i in samples if i > second]
    assert len(a_steps) >= 5 and all(s == {0: bias} for s in a_steps)
    assert len(b_steps) >= 4 and all(s == {0: {}} for s in b_steps)    # no stale bias for the next occupant


def test_two_slots_keep_their_own_bias(tiny):
    model, tok = _model(tiny), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=2, chunk_tokens=8)
    out = _run_all(sched, {"a": (tok.encode("first request"), 6, dict(logit_bias={5: 1.0})),
                           "b": (tok.encode("second request, unbiased"), 6, {})})
    sa, sb = out["a"][0].slot, out["b"][0].slot
    assert sa != sb
    steps = [e[1] for e in model.engine.events if e[0] == "sample"]
    assert any(len(s) == 2 for s in steps)                             # they did share steps
    assert all(s[sa] == {5: 1.0} for s in steps if sa in s) and all(s[sb] == {} for s in steps if sb in s)


def test_stop_finishes_the_sequence_frees_the_slot_and_counts_the_sampled_tokens(tiny):
    model, tok = _model(tiny), load_tokenizer(tiny)
    prompt = tok.encode("tell me something")
    free = _run_all(ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0), {"free": (prompt, 24, {})})["free"]
    assert free[2] == "length" and len(free[1]) >= 8
    full = free[1]
    cut = len(full) // 2
    stop = full[cut:cut + 3]
    at = full.find(stop)
    model2 = _model(tiny)
    sched = ContinuousScheduler(model2, tok, max_slots=1, chunk_tokens=0)
    out = _run_all(sched, {"s": (prompt, 24, dict(stop=["never-there", stop])), "next": (prompt, 3, {})})
    seq, text, reason = out["s"]
    assert reason == "stop" and seq.finished == "stop" and text == full[:at]
    assert 0 < len(seq.generated) < 24
    assert seq.generated == free[0].generated[:len(seq.generated)]     # every sampled token is counted, the stop's included
    assert stop in tok.decode(seq.generated)
    assert out["next"][2] == "length" and out["next"][0].slot == seq.slot == 0     # the one slot was released
    assert all(s is None or s.finished for s in sched.slots)


def test_a_stop_that_never_completes_changes_nothing(tiny):
    model, tok = _model(tiny), load_tokenizer(tiny)
    prompt = tok.encode("tell me something")
    plain = _run_all(ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0), {"p": (prompt, 12, {})})["p"]
    # a stop whose first character ends the text is held back at every step and flushed at the end
    held = _run_all(ContinuousScheduler(_model(tiny), tok, max_slots=1, chunk_tokens=0),
                    {"p": (prompt, 12, dict(stop=[plain[1][-1] + "\x00never"]))})["p"]
    assert held[2] == "length" and held[1] == plain[1] and held[0].generated == plain[0].generated


# ---- 3. a cache without the table, and the values submit refuses
def test_plain_fake_cache_refuses_a_biased_request_and_runs_an_unbiased_one(tiny):
    model, tok = _model(tiny, FakeEngine), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0)
    assert not hasattr(sched.kv, "set_row_logit_bias")
    with pytest.raises(ValueError, match="logit_bias"):
        sched.submit([1, 2, 3], 4, 0.0, 1.0, lambda *a: None, logit_bias={5: 1.0})
    assert not sched.pending
    out = _run_all(sched, {"u": ([1, 2, 3], 4, dict(logit_bias={}, stop=None))})
    assert out["u"][2] in ("stop", "length")


def test_submit_refuses_bad_bias_and_stop_values(tiny):
    model, tok = _model(tiny), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0)
    bad = [dict(logit_bias={-1: 1.0}), dict(logit_bias={"7": 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={True: 1.0}),
           dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")}), dict(logit_bias={i: 0.5 for i in range(1025)}),
           dict(stop=["a", "b", "c", "d", "e"]), dict(stop=["ok", ""]), dict(stop=[3])]
    for kw in bad:
        with pytest.raises(ValueError, match="logit_bias|stop"):
            sched.submit([1, 2, 3], 4, 0.0, 1.0, lambda *a: None, **kw)
    assert not sched.pending
    ok = sched.submit([1, 2, 3], 4, 0.0, 1.0, lambda *a: None, logit_bias={i: 0.5 for i in range(1024)}, stop=["a", "b", "c", "d"])
    assert len(ok.logit_bias) == 1024 and ok.stop == ["a", "b", "c", "d"]
    s = Sequence([1, 2, 3], 4, 0.5, 0.9, lambda *a: None, None)          # the positional signature stays
    assert s.logit_bias == {} and s.stop == [] and s.stopper is None
    sched.stop()


# ---- 4. schemas and _submit
def test_completion_request_takes_stop_as_a_string_or_a_list():
    assert CompletionRequest(model="m", prompt="p").stop is None
    assert CompletionRequest(model="m", prompt="p", stop="\n").stop == "\n"
    assert CompletionRequest(model="m", prompt="p", stop=["a", "b"]).stop == ["a", "b"]
    assert ChatCompletionRequest(model="m", messages=[ChatMessage(role="user", content="x")], stop="###").stop == "###"


class _StubScheduler:
    def __init__(self):
        self.calls = []

    def submit(self, prompt_ids, max_tokens, temp, top_p, sink, **kw):
        self.calls.append(kw)
        return types.SimpleNamespace(generated=[], finished=None, cancel=lambda: None)


def _submit_once(state, tok, req):
    from mlx_parallm_amd.server import main as srv

    async def go():
        return srv._submit(state, srv._wrap(tok), "some prompt", req)
    return asyncio.run(go())


def test_submit_hands_the_parsed_bias_and_the_stop_list_to_the_scheduler(tiny):
    from fastapi import HTTPException

    tok = load_tokenizer(tiny)
    stub = _StubScheduler()
    state = types.SimpleNamespace(scheduler=stub)
    chat = ChatCompletionRequest(model="m", messages=[ChatMessage(role="user", content="x")], logit_bias={"17": -100.0, "5": 2.0},
                                 stop="###")
    comp = CompletionRequest(model="m", prompt="p", logit_bias={"9": 1.5}, stop=["\n\n", "END"])
    none = CompletionRequest(model="m", prompt="p")
    for req in (chat, comp, none):
        _submit_once(state, tok, req)
    assert [(c["logit_bias"], c["stop"]) for c in stub.calls] == [({17: -100.0, 5: 2.0}, ["###"]), ({9: 1.5}, ["\n\n", "END"]),
                                                                 (None, [])]
    for bad in (CompletionRequest(model="m", prompt="p", stop=["a", "b", "c", "d", "e"]),
                ChatCompletionRequest(model="m", messages=[ChatMessage(role="user", content="x")], stop=["1", "2", "3", "4", "5"]),
                CompletionRequest(model="m", prompt="p", stop=[""]),
                CompletionRequest(model="m", prompt="p", logit_bias={str(i): 1.0 for i in range(1025)})):
        with pytest.raises(HTTPException) as ei:
            _submit_once(state, tok, bad)
        assert ei.value.status_code == 400
    assert len(stub.calls) == 3


def test_a_scheduler_refusal_becomes_http_400(tiny):
    """The cache of the CPU double has no bias table: the scheduler's ValueError reaches the client as 400."""
    from fastapi import HTTPException

    model, tok = _model(tiny, FakeEngine), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=1, chunk_tokens=0)
    state = types.SimpleNamespace(scheduler=sched)
    with pytest.raises(HTTPException) as ei:
        _submit_once(state, tok, CompletionRequest(model="m", prompt="p", logit_bias={"9": 1.5}))
    assert ei.value.status_code == 400 and "logit_bias" in ei.value.detail
    sched.stop()
