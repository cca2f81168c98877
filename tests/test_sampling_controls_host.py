"""top_k / min_p / seed through the host layers, without a GPU: the request schemas, ``SampleArgs`` and the ABI struct, and
what the continuous scheduler hands to the engine per step (a recording engine over the oracle-backed fake)."""
import ctypes as C
import re
import threading
from pathlib import Path

import numpy as np
import pytest

from fake_engine import FakeEngine, FakeModel
from mlx_parallm_amd import _lib as L
from mlx_parallm_amd.engine import SampleArgs
from mlx_parallm_amd.server.schemas import ChatCompletionRequest, ChatMessage, CompletionRequest
from mlx_parallm_amd.server.scheduler import ContinuousScheduler, Sequence
from mlx_parallm_amd.tokenizer_utils import load_tokenizer

ROOT = Path(__file__).resolve().parent.parent


def test_schemas_accept_and_default_the_three_fields():
    c = CompletionRequest(model="m", prompt="p")
    assert (c.top_k, c.min_p, c.seed) == (0, 0.0, None)
    c = CompletionRequest(model="m", prompt="p", top_k=40, min_p=0.05, seed=7)
    assert (c.top_k, c.min_p, c.seed) == (40, 0.05, 7)
    ch = ChatCompletionRequest(model="m", messages=[ChatMessage(role="user", content="x")])
    assert (ch.top_k, ch.min_p, ch.seed) == (0, 0.0, None)
    ch = ChatCompletionRequest(model="m", messages=[ChatMessage(role="user", content="x")], top_k=5, min_p=1.0, seed=2 ** 40)
    assert (ch.top_k, ch.min_p, ch.seed) == (5, 1.0, 2 ** 40)
    for bad in (dict(top_k=-1), dict(min_p=-0.1), dict(min_p=1.5)):
        with pytest.raises(ValueError):
            CompletionRequest(model="m", prompt="p", **bad)
        with pytest.raises(ValueError):
            ChatCompletionRequest(model="m", messages=[], **bad)


def test_sample_args_fill_the_struct():
    sp = SampleArgs(temp=0.7, top_p=0.9, top_k=50, min_p=0.05, seed=3)
    assert sp.c.struct_size == C.sizeof(L.SampleParams)
    assert sp.c.top_k == 50 and abs(sp.c.min_p - 0.05) < 1e-8
    assert not sp.c.row_top_k and not sp.c.row_min_p and not sp.c.row_seed and not sp.c.row_position
    d = SampleArgs()
    assert d.c.top_k == 0 and d.c.min_p == 0.0                      # the defaults are "off"
    sp.set_row_filters([1, 0, 7], [0.0, 0.5, 1.0])
    sp.set_row_streams([5, 2 ** 64 - 1, 0], [0, 9, -1])
    assert [sp.c.row_top_k[i] for i in range(3)] == [1, 0, 7]
    assert [sp.c.row_min_p[i] for i in range(3)] == [0.0, 0.5, 1.0]
    assert [sp.c.row_seed[i] for i in range(3)] == [5, 2 ** 64 - 1, 0]
    assert [sp.c.row_position[i] for i in range(3)] == [0, 9, -1]
    sp.set_row_filters(None, [0.25])                                # each array on its own
    assert not sp.c.row_top_k and sp.c.row_min_p[0] == 0.25
    with pytest.raises(ValueError):
        sp.set_row_filters([1, 2], [0.1])
    with pytest.raises(ValueError):
        sp.set_row_streams([1, 2], [0])


def test_struct_matches_the_header():
    """sizeof and the offsets of the appended fields, from a compiled probe of include/mi355_decode.h; ABI version 4."""
    import subprocess
    import tempfile

    names = ["top_k", "min_p", "row_top_k", "row_min_p", "row_seed", "row_position", "stream_position", "row_top_p"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi355_decode.h"\nint main(void){printf("%d %zu", MI_ABI_VERSION, '
           'sizeof(mi_sample_params));' + "".join(f'printf(" %zu", offsetof(mi_sample_params, {n}));' for n in names) +
           'return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(Path(td) / "p.c"), "-o", str(Path(td) / "p")], check=True)
        out = [int(x) for x in subprocess.run([str(Path(td) / "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 4 == L.MI_ABI_VERSION
    assert out[1] == C.sizeof(L.SampleParams)
    assert out[2:] == [getattr(L.SampleParams, n).offset for n in names]
    assert L.SampleParams.stream_position.offset == 72 and L.SampleParams.top_k.offset == 80     # the ABI 3 offsets stay
    header = (ROOT / "include" / "mi355_ops.h").read_text()
    assert re.search(r"\bmi_op_sample_ex\s*\(", header) and "mi_op_sample_ex" in L.SIGNATURES


class RecordingEngine(FakeEngine):
    """Records, per sampling step, what the scheduler passed for each wanted row: (sequence row, top_k, min_p, seed, position)."""

    def __init__(self, ref_model):
        super().__init__(ref_model)
        self.steps = []
        self.on_step = None            # called with each recorded step (on the scheduler's thread)

    def _record(self, rows, sample):
        c = sample.c
        n = len(rows)
        assert c.struct_size == C.sizeof(L.SampleParams)
        assert c.row_top_k and c.row_min_p and c.row_seed and c.row_position and c.row_temperature and c.row_top_p
        self.steps.append([(int(rows[i]), int(c.row_top_k[i]), float(c.row_min_p[i]), int(c.row_seed[i]), int(c.row_position[i]))
                           for i in range(n)])
        if self.on_step is not None:
            self.on_step(self.steps[-1])

    def step_enqueue_rows(self, kv, rows, tokens=None, sample=None):
        self._record(list(rows), sample)
        return super().step_enqueue_rows(kv, rows, tokens, sample)

    def step_enqueue_mixed(self, kv, rows, token_lists, want=None, sample=None):
        w = [1] * len(rows) if want is None else list(want)
        if sample is not None:
            self._record([r for r, x in zip(rows, w) if x], sample)
        return super().step_enqueue_mixed(kv, rows, token_lists, want, sample)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("controls") / "tiny"
    build_tiny_model(d, seed=6, vocab_size=320, hidden_size=32, layers=2, heads=2, kv_heads=2,
                     intermediate_size=64, quantize_model=False, dtype="float32")
    return str(d)


def _recording_model(tiny):
    model = FakeModel(tiny, max_pos=2048)
    model.engine = RecordingEngine(model.ref)
    return model


def _run(sched, first, second):
    """(name, prompt, max_tokens, temp, kwargs) twice: the second request is submitted when the engine has seen the first
    one's fourth sampling step, i.e. while it is decoding -> {name: Sequence}; returns when both have finished."""
    done, ev, seqs = set(), threading.Event(), {}

    def on_step(step):
        if second[0] not in seqs and any(t[4] >= 3 for t in step):
            seqs[second[0]] = sched.submit(second[1], second[2], second[3], 1.0, sink_for(second[0]), **second[4])

    def sink_for(name):
        def sink(seq, delta, reason):
            if reason is not None:
                done.add(name)
                if len(done) == 2:
                    ev.set()
        return sink

    sched.model.engine.on_step = on_step
    sched.start()
    seqs[first[0]] = sched.submit(first[1], first[2], first[3], 1.0, sink_for(first[0]), **first[4])
    assert ev.wait(timeout=120)
    sched.stop()
    return seqs


@pytest.mark.parametrize("chunk", [0, 8])
def test_scheduler_passes_per_row_controls_and_stream_positions(tiny, chunk):
    """A seeded sequence sees positions 0, 1, 2, ... of its own seed, an unseeded one -1, whatever slot and step they are in
    -- also across the admission of the second one in mid-flight; top_k / min_p travel per row."""
    model, tok = _recording_model(tiny), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=2, chunk_tokens=chunk)
    a, b = tok.encode("first request, a long one"), tok.encode("second")
    seqs = _run(sched, ("a", a, 24, 0.0, dict(top_k=40, min_p=0.05, seed=1234)), ("b", b, 6, 0.0, dict(top_k=3)))
    steps = model.engine.steps
    sa = [t for step in steps for t in step if t[1] == 40]
    sb = [t for step in steps for t in step if t[1] == 3]
    assert sum(len(step) for step in steps) == len(sa) + len(sb)
    assert len(seqs["a"].generated) > 3 and any(len(step) == 2 for step in steps)              # they did share steps
    first_b = next(i for i, step in enumerate(steps) if any(t[1] == 3 for t in step))
    assert first_b > 2 and any(t[1] == 40 for step in steps[first_b + 1:] for t in step)       # b arrived in mid-flight
    assert all(abs(t[2] - 0.05) < 1e-8 and t[3] == 1234 for t in sa)
    assert [t[4] for t in sa] == list(range(len(sa))) and len(sa) >= len(seqs["a"].generated)
    assert all(t[2] == 0.0 and t[4] == -1 for t in sb) and len(sb) >= len(seqs["b"].generated)
    assert seqs["a"].sample_steps == len(sa)


def test_n_choices_use_consecutive_seeds(tiny):
    """The server gives choice i of a seeded request the stream of seed + i (server/main.py _submit)."""
    import asyncio
    import types

    from mlx_parallm_amd.server import main as srv

    model, tok = _recording_model(tiny), load_tokenizer(tiny)
    sched = ContinuousScheduler(model, tok, max_slots=4, chunk_tokens=0)
    sched.start()
    state = types.SimpleNamespace(scheduler=sched, config=types.SimpleNamespace(request_timeout_seconds=120))
    req = CompletionRequest(model="m", prompt="three choices", max_tokens=4, temperature=0.0, n=3, seed=100, top_k=9)
    resp = asyncio.run(srv._scheduled_response(state, req, srv._wrap(tok), "m"))
    sched.stop()
    assert len(resp.choices) == 3
    seeds = sorted({t[3] for step in model.engine.steps for t in step})
    assert seeds == [100, 101, 102]
    assert all(t[1] == 9 and t[4] >= 0 for step in model.engine.steps for t in step)


def test_sequence_keeps_its_positional_signature_and_refuses_bad_values():
    s = Sequence([1, 2, 3], 4, 0.5, 0.9, lambda *a: None, None)
    assert (s.top_k, s.min_p, s.seed, s.sample_steps) == (0, 0.0, None, 0)
    for bad in (dict(top_k=-1), dict(min_p=1.5), dict(min_p=-0.5), dict(min_p=float("nan"))):
        with pytest.raises(ValueError):
            Sequence([1], 1, 0.0, 1.0, lambda *a: None, None, **bad)
