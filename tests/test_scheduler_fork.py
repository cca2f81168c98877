"""``ContinuousScheduler(fork_choices=True)`` on CPU: the choices of one request (``submit(..., group=g)``) share one prompt
prefill.  The device engine is the oracle-backed fake; its KV gets a ``fork_row`` (a copy of the donor row's oracle cache cut
to ``n_tokens``) and the engine records, per fed segment, the row, the position it was fed at and its length, so that the
prompt tokens a run fed can be counted: the tokens fed at positions below the prompt length."""
import copy
import threading

import numpy as np
import pytest

from fake_engine import FakeEngine, FakeModel, FakeSlotKV
from mlx_parallm_amd.server.scheduler import ContinuousScheduler, ReplicaPool, new_group
from mlx_parallm_amd.tokenizer_utils import load_tokenizer

P, N, NEW = 40, 4, 6


class ForkKV(FakeSlotKV):
    def __init__(self, engine, batch_size):
        super().__init__(engine, batch_size)
        self.forks = []                       # (src, dst, n_tokens, length of src at the time)

    def fork_row(self, src, dst, n_tokens):
        offs = self.offsets
        if src == dst or offs[dst] != 0 or not 1 <= n_tokens <= offs[src]:
            raise ValueError("fork_row: bad argument")
        self.forks.append((src, dst, n_tokens, offs[src]))
        self.engine.trace.append(("fork_row", src, dst, n_tokens))
        row = copy.deepcopy(self.rows[src])
        for c in row:                         # the oracle's cache appends at `offset`: what lies behind it is overwritten
            c.offset = n_tokens
        self.rows[dst] = row


class CountingEngine(FakeEngine):
    """FakeEngine + ``fed``: one (row, position, length) per segment of every step."""

    kv_class = ForkKV

    def __init__(self, ref_model):
        super().__init__(ref_model)
        self.fed = []

    def new_kv(self, batch_size, capacity=256, kv_dtype="model", step=256):
        return self.kv_class(self, batch_size)

    def step_enqueue_rows(self, kv, rows, tokens=None, sample=None):
        offs = kv.offsets
        L = 1 if tokens is None else np.asarray(tokens).shape[1]
        self.fed += [(int(r), offs[int(r)], L) for r in rows]
        return super().step_enqueue_rows(kv, rows, tokens, sample)

    def step_enqueue_mixed(self, kv, rows, token_lists, want=None, sample=None):
        offs = kv.offsets
        self.fed += [(int(r), offs[int(r)], len(t)) for r, t in zip(rows, token_lists)]
        return super().step_enqueue_mixed(kv, rows, token_lists, want, sample)


class PlainEngine(CountingEngine):
    kv_class = FakeSlotKV                     # a KV without fork_row


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from mlx_parallm_amd.tiny_model import build_tiny_model

    d = tmp_path_factory.mktemp("sched_fork") / "tiny"
    build_tiny_model(d, seed=6, vocab_size=320, hidden_size=32, layers=2, heads=2, kv_heads=2,
                     intermediate_size=64, quantize_model=False, dtype="float32")
    return str(d)


@pytest.fixture(scope="module")
def tok(tiny):
    return load_tokenizer(tiny)


def _model(tiny, engine_class=CountingEngine):
    m = FakeModel(tiny, max_pos=2048)
    m.engine = engine_class(m.ref)
    return m


def _prompt(tok, n=P):
    ids = [5 + (7 * i) % 300 for i in range(n)]
    return [t if t != tok.eos_token_id else 4 for t in ids]


def _run(tiny, tok, *, fork, chunk, slots=N, n=N, prompt_len=P, engine_class=CountingEngine, group=True, new=NEW, hook=None):
    """n choices of one prompt, submitted together; -> (model, scheduler, [generated ids per choice], [finish reasons])."""
    model = _model(tiny, engine_class)
    sched = ContinuousScheduler(model, tok, max_slots=slots, chunk_tokens=chunk, fork_choices=fork)
    done, ev = {}, threading.Event()

    def sink_for(i):
        def sink(seq, delta, reason):
            if reason is not None:
                done[i] = (list(seq.generated), reason)
                if len(done) == n:
                    ev.set()
        return sink

    g = new_group() if group else None
    prompt = _prompt(tok, prompt_len)
    limits = new if isinstance(new, (list, tuple)) else [new] * n
    seqs = [sched.submit(prompt, limits[i], 0.0, 1.0, sink_for(i), group=g) for i in range(n)]     # all queued before the thread starts
    if hook is not None:
        hook(sched, seqs)
    sched.start()
    assert ev.wait(timeout=120), "a sequence never finished"
    sched.stop()
    return model, sched, [done[i][0] for i in range(n)], [done[i][1] for i in range(n)]


def _prompt_tokens_fed(engine, prompt_len=P):
    return sum(max(0, min(pos + n, prompt_len) - pos) for _row, pos, n in engine.fed)


@pytest.mark.parametrize("chunk", [0, 16, 256])
def test_the_choices_of_a_group_share_one_prompt_prefill(tiny, tok, chunk):
    model, sched, outs, reasons = _run(tiny, tok, fork=True, chunk=chunk)
    base_model, base, base_outs, base_reasons = _run(tiny, tok, fork=False, chunk=chunk)
    print("prompt tokens fed: fork", _prompt_tokens_fed(model.engine), "no fork", _prompt_tokens_fed(base_model.engine))
    assert _prompt_tokens_fed(base_model.engine) == N * P and base.forks == 0 and base.fork_tokens == 0
    assert _prompt_tokens_fed(model.engine) == P + (N - 1)                # one prefill, then one last prompt token per sibling
    assert sched.forks == N - 1 and sched.fork_tokens == (N - 1) * (P - 1)
    assert [f[2] for f in sched.kv.forks] == [P - 1] * (N - 1) and all(f[0] != f[1] for f in sched.kv.forks)
    assert outs == base_outs and reasons == base_reasons                  # the fake computes row by row: identical outputs
    assert all(o == outs[0] for o in outs) and len(outs[0]) > 0           # greedy choices of one prompt
    tr = model.engine.trace
    for k, e in enumerate(tr):                                            # reset the slot, then fork into it: nothing between
        if e[0] == "fork_row":
            touched = [f for f in tr[:k] if f == ("reset_row", e[2]) or (f[0] in ("enqueue_rows", "enqueue_mixed") and e[2] in f[1])]
            assert touched and touched[-1] == ("reset_row", e[2])


@pytest.mark.parametrize("chunk", [0, 16])
def test_later_siblings_fork_from_a_donor_that_is_already_decoding(tiny, tok, chunk):
    limits = [NEW, NEW + 4, NEW + 8, NEW + 12]                            # 2 slots: a choice leaves while its neighbour still decodes
    model, sched, outs, reasons = _run(tiny, tok, fork=True, chunk=chunk, slots=2, new=limits)
    _, _, base_outs, base_reasons = _run(tiny, tok, fork=False, chunk=chunk, slots=2, new=limits)
    assert outs == base_outs and reasons == base_reasons == ["length"] * N
    # choice 1 forks as soon as choice 0 has prefilled; 2 gets the slot of 0 while 1 is decoding, 3 the slot of 1 while 2 is:
    # they take the first P - 1 tokens of a row that is longer than the prompt by then
    assert sched.forks == N - 1 and [f[2] for f in sched.kv.forks] == [P - 1] * (N - 1)
    assert [src_len > P for _s, _d, _n, src_len in sched.kv.forks] == [False, True, True]
    assert _prompt_tokens_fed(model.engine) == P + (N - 1)


def test_a_donor_cancelled_mid_prefill_leaves_the_others_to_normal_admission(tiny, tok):
    def hook(sched, seqs):
        # the donor goes away after its first chunk: cancel it from inside the engine, between two steps
        eng = sched.model.engine
        inner = eng.step_enqueue_mixed

        def mixed(kv, rows, token_lists, want=None, sample=None):
            t = inner(kv, rows, token_lists, want, sample)
            if len(eng.fed) == 1:
                seqs[0].cancel()
            return t
        eng.step_enqueue_mixed = mixed

    model, sched, outs, reasons = _run(tiny, tok, fork=True, chunk=16, hook=hook)
    assert reasons[0] == "cancelled" and reasons[1:] == ["length"] * (N - 1)          # nobody hangs
    _, _, base_outs, _ = _run(tiny, tok, fork=False, chunk=16)
    assert outs[1:] == base_outs[1:]
    # choice 1 found no live member and prefilled on its own; 2 and 3 waited for it and forked
    assert sched.forks == N - 2 and [f[2] for f in sched.kv.forks] == [P - 1] * (N - 2)
    assert _prompt_tokens_fed(model.engine) == 16 + P + (N - 2)


def test_a_one_token_prompt_is_not_forked(tiny, tok):
    model, sched, outs, reasons = _run(tiny, tok, fork=True, chunk=16, prompt_len=1)
    assert sched.forks == 0 and sched.kv.forks == [] and _prompt_tokens_fed(model.engine, 1) == N
    assert all(o == outs[0] for o in outs)


@pytest.mark.parametrize("chunk", [0, 16])
@pytest.mark.parametrize("how", ["flag off", "kv without fork_row", "no group"])
def test_without_the_switch_the_call_sequence_is_todays(tiny, tok, chunk, how):
    kw = {"flag off": dict(fork=False), "kv without fork_row": dict(fork=True, engine_class=PlainEngine),
          "no group": dict(fork=True, group=False)}[how]
    model, sched, outs, _ = _run(tiny, tok, chunk=chunk, **kw)
    # today's: the same scheduler on the plain fake, without a group -- nothing of this feature in play
    ref_model, ref_sched, ref_outs, _ = _run(tiny, tok, fork=False, chunk=chunk, engine_class=PlainEngine, group=False)
    assert model.engine.trace == ref_model.engine.trace and model.engine.fed == ref_model.engine.fed
    assert outs == ref_outs and sched.forks == 0 and sched.fork_choices == (how == "no group")
    assert not [e for e in model.engine.trace if e[0] == "fork_row"]


def test_a_replica_pool_keeps_a_group_on_one_replica(tiny, tok):
    models = [_model(tiny), _model(tiny)]
    pool = ReplicaPool(models, tok, max_slots=N, chunk_tokens=16, fork_choices=True)
    done, ev = [], threading.Event()

    def sink(seq, delta, reason):
        if reason is not None:
            done.append(reason)
            if len(done) == N:
                ev.set()

    g = pool.new_group()
    for _ in range(N):                        # without the pin the least-loaded rule would alternate between the two replicas
        pool.submit(_prompt(tok), NEW, 0.0, 1.0, sink, group=g)
    assert g.replica is pool.replicas[0] and len(pool.replicas[0].pending) == N and len(pool.replicas[1].pending) == 0
    pool.start()
    assert ev.wait(timeout=120)
    pool.stop()
    assert pool.forks == N - 1 and pool.fork_tokens == (N - 1) * (P - 1) and pool.replicas[1].forks == 0


def test_a_replica_pool_that_does_not_fork_spreads_a_group_as_ever(tiny, tok):
    """With the switch off a group is inert: its members go to the least loaded replica one by one, exactly as sequences
    without a group do."""
    placed = {}
    for grouped in (False, True):
        pool = ReplicaPool([_model(tiny), _model(tiny)], tok, max_slots=N, chunk_tokens=16)          # fork_choices off
        g = pool.new_group() if grouped else None
        for _ in range(N):
            pool.submit(_prompt(tok), NEW, 0.0, 1.0, lambda *a: None, **({"group": g} if grouped else {}))
        placed[grouped] = [len(r.pending) for r in pool.replicas]
        assert g is None or g.replica is None
        for r in pool.replicas:
            r.kv.close()
    assert placed[True] == placed[False] == [N // 2, N // 2]


class FailingForkKV(ForkKV):
    message = ""

    def fork_row(self, src, dst, n_tokens):
        raise RuntimeError(self.message)


@pytest.mark.parametrize("message,falls_back", [("mi_kv_fork_row: the block arena has no block for the tail (every block is held)", True),
                                                ("mi_kv_fork_row: hipMemsetD32Async failed", False)])
def test_only_an_exhausted_arena_falls_back_to_a_prefill(tiny, tok, message, falls_back):
    class Engine(CountingEngine):
        kv_class = type("KV", (FailingForkKV,), {"message": message})

    model, sched, outs, reasons = _run(tiny, tok, fork=True, chunk=16, n=2, engine_class=Engine)
    if falls_back:                                       # the sibling prefills its own prompt, as with the switch off
        _, _, base_outs, base_reasons = _run(tiny, tok, fork=False, chunk=16, n=2)
        assert (outs, reasons) == (base_outs, base_reasons) and sched.forks == 0 and _prompt_tokens_fed(model.engine) == 2 * P
    else:                                                # any other failure is the step's: nobody carries on as if blocks were short
        assert "error" in reasons and sched.forks == 0
