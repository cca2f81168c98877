"""Continuous (admit-on-step) scheduler over the engine's row-subset steps.

The reference's ``--scheduler continuous`` (server/main.py:1404-1726) unifies streaming and non-streaming
requests in one batch and admits between batches by rebuilding it.  This scheduler keeps what that mode is
for -- a request does not wait for the running batch to finish -- and does it on a slot model instead:

  * the KV cache has ``max_slots`` rows; a sequence owns one row from admission to its last token;
  * admission = reset the row, prefill the prompt on that row alone (no padding: other rows are not part
    of the call, ``mi_step_enqueue_rows`` with n = 1), emit its first token;
  * every decode step runs on exactly the rows that are alive, each with its own temperature / top_p / top_k / min_p
    (``mi_sample_params.row_temperature / row_top_p / row_top_k / row_min_p``); a sequence submitted with a ``seed`` draws
    from its own random stream (``row_seed`` = the seed, ``row_position`` = how many sampling steps the sequence has had), so
    its draws do not depend on the slot it got or on who else is alive;
  * a request's ``logit_bias`` is set on its row at admission (``KVCache.set_row_logit_bias``, right after the row's reset) and
    stays on the device until the row is reset for its next occupant; its ``stop`` strings are matched on the detokenised
    generated text (``StopMatcher``): the sequence finishes with reason "stop" at that step boundary, as for EOS;
  * a request's ``logprobs`` (0..20 top entries per sampled token, optionally under ``softmax(logits / T)``) are set on its row
    at admission next to the bias (``KVCache.set_row_logprobs``) and cleared with the row; the sequence collects, per sampled
    token, the id, its logprob and its top list from the results of the shared steps, so such a request never takes the
    engine away from the others;
  * a request's LoRA adapter (``submit(..., adapter=slot)``, a slot of ``Engine.set_adapter_lora``; -1 = the base model) is set
    on its row at admission (``KVCache.set_row_adapter``), right after the reset and ahead of the fork and the prefix lookup --
    K / V depend on it -- and goes with the row's reset; requests on different adapters share the steps;
  * with ``fork_choices`` the ``n`` choices of one request (``submit(..., group=new_group())``) share one prompt prefill: the
    first member prefills, the others wait for it at the head of the queue and then get its row's first ``P - 1`` tokens
    (``KVCache.fork_row``: full blocks shared, the tail copied) and run the last prompt token themselves -- ``P + (n - 1)``
    prompt tokens instead of ``n * P``;
  * while the row set is stable the next step is enqueued before the current one is read back, sampled tokens
    stay on the device (the same one-step-ahead pipelining as generate_step, utils.py:420-427); when a sequence
    finishes or a request is waiting, the step already in flight completes, its tokens for finished rows are
    dropped, and the next step starts from explicit tokens on the new row set.

The scheduler runs on its own thread and owns the engine while it steps; other users of the same engine
(logprobs / echo / perplexity) take ``engine_mutex`` and are let in between steps.  Results are delivered
through a per-sequence ``sink(sequence, delta_text, finish_reason)`` callback invoked on the scheduler thread.
"""
from __future__ import annotations

import collections
import itertools
import logging
import math
import os
import threading
import time
from typing import Callable, Deque, Dict, List, Optional

import numpy as np

from ..tokenizer_utils import NaiveStreamingDetokenizer, TokenizerWrapper

log = logging.getLogger("mlx_parallm_amd.scheduler")

Sink = Callable[["Sequence", Optional[str], Optional[str]], None]


MAX_ROW_LOGIT_BIAS = 1024      # MI_MAX_ROW_LOGIT_BIAS (mi355_decode.h): entries of one request's logit_bias
MAX_STOP_SEQUENCES = 4         # as the OpenAI API
MAX_TOP_LOGPROBS = 20          # MI_MAX_TOP_LOGPROBS (mi355_decode.h)
MAX_ADAPTERS = 16              # MI_MAX_ADAPTERS


class StopMatcher:
    """Stop sequences over the detokenised text of ONE generation (never its prompt).

    ``feed(delta) -> (text_to_emit, hit)``: the new text of a step goes in, what may be shown comes out.  The first stop string
    that completes ends the generation -- when several complete in the same delta, the one that STARTS earliest -- and the
    emitted text ends just before it.  While nothing has completed, the longest suffix of the text that is a proper prefix
    of any stop string is held back, so a client never sees the beginning of a stop string that then completes; ``flush()``
    hands the held text out when the generation ends for another reason (EOS, length)."""

    def __init__(self, stops):
        self.stops = [str(s) for s in stops]
        if any(not s for s in self.stops):
            raise ValueError("stop: an empty stop string")
        self.hit = False
        self._held = ""

    def feed(self, delta: Optional[str]):
        if self.hit:
            return "", True
        buf = self._held + (delta or "")
        starts = [i for i in (buf.find(s) for s in self.stops) if i >= 0]
        if starts:
            self.hit, self._held = True, ""
            return buf[:min(starts)], True
        hold = 0
        for s in self.stops:
            for k in range(min(len(s) - 1, len(buf)), hold, -1):
                if buf.endswith(s[:k]):
                    hold = k
                    break
        self._held = buf[len(buf) - hold:]
        return buf[:len(buf) - hold], False

    def flush(self) -> str:
        out, self._held = self._held, ""
        return out


def check_logit_bias(logit_bias) -> Dict[int, float]:
    """A request's logit_bias as {token id: value}: ids are ints >= 0, values finite, at most MAX_ROW_LOGIT_BIAS entries
    (ValueError otherwise; ids beyond the vocabulary are the engine's to refuse)."""
    if not logit_bias:
        return {}
    if not isinstance(logit_bias, dict):
        raise ValueError("logit_bias must be a dict of token id -> bias")
    if len(logit_bias) > MAX_ROW_LOGIT_BIAS:
        raise ValueError(f"logit_bias has {len(logit_bias)} entries, at most {MAX_ROW_LOGIT_BIAS} are supported")
    out: Dict[int, float] = {}
    for k, v in logit_bias.items():
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 0:
            raise ValueError(f"logit_bias: token id {k!r} is not an int >= 0")
        try:
            fv = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"logit_bias[{k}]: {v!r} is not a number") from None
        if not math.isfinite(fv):
            raise ValueError(f"logit_bias[{k}] = {v!r} is not finite")
        out[int(k)] = fv
    return out


def check_stop(stop) -> List[str]:
    """A request's stop list: at most MAX_STOP_SEQUENCES non-empty strings (ValueError otherwise)."""
    if stop is None:
        return []
    if isinstance(stop, str):
        stop = [stop]
    stop = list(stop)
    if len(stop) > MAX_STOP_SEQUENCES:
        raise ValueError(f"stop: at most {MAX_STOP_SEQUENCES} stop sequences are supported, got {len(stop)}")
    for s in stop:
        if not isinstance(s, str) or not s:
            raise ValueError("stop: every stop sequence must be a non-empty string")
    return stop


class Group:
    """What the sequences of one request's ``n`` choices share (``new_group()``, ``submit(..., group=g)``): a scheduler with
    ``fork_choices`` prefills their common prompt once and forks the KV row for the others."""
    __slots__ = ("replica",)

    def __init__(self):
        self.replica = None            # ReplicaPool with fork_choices: the replica of the first member (a row is forked inside one cache)


def new_group() -> Group:
    return Group()


class Sequence:
    _ids = itertools.count()

    def __init__(self, prompt_ids, max_tokens: int, temp: float, top_p: float, sink: Sink, detok, *, top_k: int = 0,
                 min_p: float = 0.0, seed: Optional[int] = None, logit_bias: Optional[Dict[int, float]] = None,
                 stop: Optional[List[str]] = None, logprobs: int = 0, logprobs_at_temperature: bool = False,
                 group: Optional[Group] = None, adapter: int = -1):
        self.group = group
        if isinstance(adapter, bool) or not isinstance(adapter, (int, np.integer)) or not -1 <= int(adapter) < MAX_ADAPTERS:
            raise ValueError(f"adapter must be a slot in [0, {MAX_ADAPTERS}) or -1 (none)")
        self.adapter = int(adapter)        # slot of the engine's per-request adapter table, set on the sequence's cache row at admission
        if int(top_k) < 0:
            raise ValueError("top_k must be >= 0 (0 = off)")
        if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not 0 <= int(logprobs) <= MAX_TOP_LOGPROBS:
            raise ValueError(f"logprobs must be an int in [0, {MAX_TOP_LOGPROBS}]")
        # per sampled token, in sampling order (an EOS that ends the sequence included, tokens behind a stop hit included):
        # its id, its logprob and -- logprobs > 0 -- its top list as (ids, logprobs) arrays of that length
        self.logprobs, self.logprobs_at_temperature = int(logprobs), bool(logprobs_at_temperature)
        self.token_ids: List[int] = []
        self.token_logprobs: List[float] = []
        self.top: List[tuple] = []
        if not 0.0 <= float(min_p) <= 1.0:
            raise ValueError("min_p must be in [0, 1] (0 = off)")
        self.logit_bias = check_logit_bias(logit_bias)     # set on the sequence's cache row at admission
        self.stop = check_stop(stop)
        self.stopper = StopMatcher(self.stop) if self.stop else None
        self.id = next(Sequence._ids)
        self.prompt = np.ascontiguousarray(prompt_ids, dtype=np.int32).reshape(-1)
        self.max_tokens = int(max_tokens)
        self.temp, self.top_p = float(temp), float(top_p)
        self.top_k, self.min_p = int(top_k), float(min_p)
        self.seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.sample_steps = 0              # sampling steps enqueued for this sequence so far: the position in its stream
        self.sink = sink
        self.detok = detok
        self.generated: List[int] = []
        self.slot: Optional[int] = None
        self.finished: Optional[str] = None
        self.last_token = -1
        self.t_submit = time.perf_counter()
        self.cancelled = False
        self.prefill_pos = 0               # prompt tokens already in the KV cache (chunked prefill)
        self.prefilled = False             # the whole prompt is in the cache and the first token has been sampled

    def cancel(self) -> None:
        """Ask the scheduler to drop this sequence (client gone / request timed out): it stops taking decode steps
        at the next step boundary, its slot is released and its sink gets finish_reason "cancelled"."""
        self.cancelled = True


class ContinuousScheduler:
    def __init__(self, model, tokenizer, max_slots: int = 8, kv_dtype: Optional[str] = None, capacity: int = 1024,
                 metrics=None, chunk_tokens: int = 256, paged: bool = True, block_tokens: int = 64,
                 kv_blocks: Optional[int] = None, prefix_cache: bool = True, step_rows: int = 256,
                 fork_choices: bool = False):
        from ..engine import SampleArgs      # noqa: F401  (fail early if the library is missing)
        from ..utils import DEFAULT_KV_DTYPE

        self.model = model
        self.tok = tokenizer if isinstance(tokenizer, TokenizerWrapper) else TokenizerWrapper(tokenizer)
        self.max_slots = int(max_slots)
        # KV: a block-paged arena (rows grow without copies, cost memory for what they hold and share the blocks of a
        # common prompt prefix); engines without it (the CPU test double) get the contiguous per-row slabs
        eng = model.engine
        self.paged = bool(paged) and hasattr(eng, "new_paged_kv")
        if self.paged:
            if kv_blocks is None:
                kv_blocks = self._default_blocks(eng, block_tokens, kv_dtype or DEFAULT_KV_DTYPE)
            self.kv = eng.new_paged_kv(self.max_slots, block_tokens=block_tokens, n_blocks=kv_blocks,
                                       max_tokens_per_row=eng.max_positions, kv_dtype=kv_dtype or DEFAULT_KV_DTYPE)
        else:
            self.kv = eng.new_kv(self.max_slots, capacity=capacity, kv_dtype=kv_dtype or DEFAULT_KV_DTYPE)
        self.prefix_cache = bool(prefix_cache) and self.paged
        self.prefix_hit_tokens = 0
        # the choices of one request (submit(..., group=)) share one prompt prefill: a member admitted while another one
        # holds the prompt in its row gets that row's first P - 1 tokens (KVCache.fork_row) and runs the last prompt token
        # itself, so every choice samples its first token from its own stream.  Off by default: the forked member's last
        # prompt token goes through the decode-shaped path, not through a prefill of its own.
        self.fork_choices = bool(fork_choices) and hasattr(self.kv, "fork_row")
        self.forks = 0                     # rows forked from a group member instead of prefilled
        self.fork_tokens = 0               # prompt tokens they did not have to run
        self.slots: List[Optional[Sequence]] = [None] * self.max_slots
        self.pending: Deque[Sequence] = collections.deque()
        self.cv = threading.Condition()
        self.engine_mutex = threading.Lock()
        self._waiters = 0
        self._step_pending = False         # a step that reads the device-resident token feed is enqueued but not read
        self._stop = False
        self._thread: Optional[threading.Thread] = None
        self._seed = int.from_bytes(os.urandom(4), "little")
        self.metrics = metrics
        self.steps = 0                     # decode steps executed
        self.prefills = 0
        self.max_rows_seen = 0
        self.borrows = 0                   # times somebody took the engine away from the steps (borrow_engine)
        # chunked prefill: an arriving prompt enters the cache in chunks of at most `chunk_tokens` tokens, each chunk in
        # the SAME pass over the weights as the live rows' decode step (engine.step_enqueue_mixed).  0 = the older
        # behaviour: the whole prompt is prefilled alone while the live rows wait.
        self.chunk_tokens = int(chunk_tokens) if hasattr(model.engine, "step_enqueue_mixed") else 0
        # tokens per mixed step (decode rows + chunk tokens): the chunk budget of a step is what the live rows leave of this.
        # 256: at that size the engine's K-split tile GEMM still reads every weight matrix once per step and the marginal
        # prompt token costs ~20 us (Mistral-7B bf16: 5.8 ms at 128 rows, 8.2 ms at 256); quantised models stream W once per
        # 96 / 128 rows (two slabs at 256)
        self.step_rows = int(step_rows)
        self.mixed_steps = 0               # steps that carried prompt chunks next to decode rows
        self.chunks = 0

    def _default_blocks(self, eng, block_tokens: int, kv_dtype: str) -> int:
        """Arena size: every slot at full length if that fits in 80 % of the device memory that is free now, else what
        fits (requests then wait for blocks instead of for slots: _fits)."""
        per_row = (eng.max_positions + block_tokens - 1) // block_tokens
        full = self.max_slots * per_row + 1
        try:
            import torch

            free, _total = torch.cuda.mem_get_info(eng.device)
            d = eng.desc
            esz = 4 if kv_dtype == "float32" else (4 if eng.act_dtype == "float32" else 2)
            block_bytes = 2 * d.num_layers * d.num_kv_heads * block_tokens * d.head_dim * esz
            return int(max(2 * per_row + 1, min(full, int(0.8 * free) // block_bytes)))
        except Exception:            # (no torch / no device query: the full size, and the allocation says if it is too much)
            return full

    def _fits(self, seq: "Sequence") -> bool:
        """Admission control on the block arena: the prompt and everything the sequence may generate must find blocks now
        (free ones, or published prefix blocks that NO live row maps: a live row publishes its own prompt blocks as soon as
        its prefill is done, and those can never be evicted while it runs -- `evictable_blocks`, not `cached_blocks`) --
        a step that runs out of blocks would fail every live row."""
        if not self.paged:
            return True
        st = self.kv.stats()
        bt = self.kv.block_tokens
        need = (len(seq.prompt) + seq.max_tokens + bt - 1) // bt
        growth = 0                   # blocks the live sequences may still ask for
        offs = self.kv.offsets
        for s in self.slots:
            if s is not None and not s.finished:
                end = len(s.prompt) + s.max_tokens
                growth += max(0, (end + bt - 1) // bt - (offs[s.slot] + bt - 1) // bt)
        return need + growth <= st["free_blocks"] + st["evictable_blocks"]

    # ------------------------------------------------------------------ client side (any thread)
    def submit(self, prompt_ids, max_tokens: int, temp: float, top_p: float, sink: Sink, *, top_k: int = 0,
               min_p: float = 0.0, seed: Optional[int] = None, logit_bias: Optional[Dict[int, float]] = None,
               stop: Optional[List[str]] = None, logprobs: int = 0, logprobs_at_temperature: bool = False,
               group: Optional[Group] = None, adapter: int = -1) -> Sequence:
        seq = Sequence(prompt_ids, max_tokens, temp, top_p, sink, NaiveStreamingDetokenizer(self.tok._tokenizer),
                       top_k=top_k, min_p=min_p, seed=seed, logit_bias=logit_bias, stop=stop, logprobs=logprobs,
                       logprobs_at_temperature=logprobs_at_temperature, group=group, adapter=adapter)
        if seq.adapter >= 0 and not hasattr(self.kv, "set_row_adapter"):
            raise ValueError("adapter: this KV cache has no per-row adapter (set_row_adapter)")
        if (seq.logprobs or seq.logprobs_at_temperature) and not hasattr(self.kv, "set_row_logprobs"):
            raise ValueError("logprobs: this KV cache has no per-row logprobs setting (set_row_logprobs)")
        if seq.logit_bias:
            if not hasattr(self.kv, "set_row_logit_bias"):
                raise ValueError("logit_bias: this KV cache has no per-row logit_bias (set_row_logit_bias)")
            # (refused here, on the client's thread: at admission the engine's refusal would fail the whole step)
            vocab = getattr(getattr(self.model.engine, "desc", None), "vocab_size", None)
            if vocab is not None and max(seq.logit_bias) >= int(vocab):
                raise ValueError(f"logit_bias: token id {max(seq.logit_bias)} is outside the vocabulary [0, {int(vocab)})")
        if len(seq.prompt) == 0:
            raise ValueError("empty prompt")
        if len(seq.prompt) + seq.max_tokens > self.model.engine.max_positions:
            raise ValueError(f"prompt ({len(seq.prompt)}) + max_tokens ({seq.max_tokens}) exceeds the engine's "
                             f"max_positions ({self.model.engine.max_positions})")
        with self.cv:
            self.pending.append(seq)
            self.cv.notify_all()
        return seq

    def start(self) -> None:
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, name="mi355-scheduler", daemon=True)
            self._thread.start()

    def stop(self) -> None:
        with self.cv:
            self._stop = True
            self.cv.notify_all()
        if self._thread is not None:
            self._thread.join(timeout=30)
            self._thread = None
        try:
            self.kv.close()
        except Exception:          # pragma: no cover
            pass

    class _Borrow:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            # A borrower overwrites the engine's device-resident token feed (d_next / last_n), so it may only get
            # the engine when no enqueued step is still going to read that feed.  The scheduler publishes that in
            # _step_pending (written while it holds the mutex); once _waiters > 0 it drains before every release.
            s = self.s
            with s.cv:
                s._waiters += 1
                s.borrows += 1
                s.cv.notify_all()
            while True:
                with s.cv:
                    while s._step_pending and not s._stop:
                        s.cv.wait(timeout=0.05)
                s.engine_mutex.acquire()
                with s.cv:
                    clear = not s._step_pending
                if clear:
                    return self
                s.engine_mutex.release()

        def __exit__(self, *exc):
            with self.s.cv:
                self.s._waiters -= 1
            self.s.engine_mutex.release()

    def borrow_engine(self):
        """``with scheduler.borrow_engine(): ...`` -- exclusive use of the engine between two scheduler steps."""
        return ContinuousScheduler._Borrow(self)

    # ------------------------------------------------------------------ scheduler thread
    def _emit(self, seq: Sequence, delta: Optional[str], reason: Optional[str]) -> None:
        try:
            seq.sink(seq, delta, reason)
        except Exception:          # a broken consumer must not stop the batch
            log.exception("sequence %d: sink failed", seq.id)

    def _finish(self, seq: Sequence, reason: str) -> None:
        seq.detok.finalize()
        tail = seq.detok.last_segment
        if seq.stopper is not None:            # the last text may complete a stop string; else what was held back goes out
            tail, hit = seq.stopper.feed(tail)
            if hit:
                reason = "stop"
            else:
                tail += seq.stopper.flush()
        seq.finished = reason
        self._emit(seq, tail if tail else None, reason)

    def _on_token(self, seq: Sequence, tok: int, res=None, i: int = 0) -> None:
        """Sampled row ``i`` of the step results ``res`` gave ``seq`` the token ``tok``."""
        eos = self.tok.eos_token_id
        seq.last_token = tok
        if res is not None and (seq.logprobs or seq.logprobs_at_temperature):
            seq.token_ids.append(tok)
            seq.token_logprobs.append(float(res["logprobs"][i]))
            if seq.logprobs:               # (the row's own count of entries, at the front of its fixed-stride list)
                seq.top.append((np.array(res["top_ids"][i, :seq.logprobs]), np.array(res["top_logprobs"][i, :seq.logprobs])))
        if tok == eos:
            self._finish(seq, "stop")
            return
        seq.generated.append(tok)
        seq.detok.add_token(tok)
        delta = seq.detok.last_segment
        if seq.stopper is not None:
            delta, hit = seq.stopper.feed(delta)
            if hit:                            # the text ends just before the stop string; its tokens stay counted in `generated`
                seq.finished = "stop"
                self._emit(seq, delta or None, "stop")
                return
        if len(seq.generated) >= seq.max_tokens:
            seq.detok.finalize()
            tail = seq.detok.last_segment
            reason = "length"
            if seq.stopper is not None:        # the detokenizer's tail may complete a stop string; else the held text goes out
                tail, hit = seq.stopper.feed(tail)
                if hit:
                    reason = "stop"
                else:
                    tail += seq.stopper.flush()
            seq.finished = reason
            self._emit(seq, (delta or "") + (tail or "") or None, reason)
        elif delta:
            self._emit(seq, delta, None)

    def _sample_args(self, seqs: List[Sequence]):
        from ..engine import SampleArgs

        self._seed = (self._seed + 1) & 0xFFFFFFFF
        sp = SampleArgs(temp=seqs[0].temp, top_p=seqs[0].top_p, seed=self._seed)
        sp.set_row_params([s.temp for s in seqs], [s.top_p for s in seqs])
        sp.set_row_filters([s.top_k for s in seqs], [s.min_p for s in seqs])
        # a seeded sequence: its own stream, at the number of sampling steps it has had; the others: the step's stream
        sp.set_row_streams([s.seed or 0 for s in seqs], [-1 if s.seed is None else s.sample_steps for s in seqs])
        for s in seqs:
            s.sample_steps += 1
        return sp

    def new_group(self) -> Group:
        return new_group()

    def _group_live(self, seq: Sequence) -> List[Sequence]:
        """The members of ``seq``'s group that hold a row and are still running, with the same prompt."""
        if not self.fork_choices or seq.group is None or len(seq.prompt) < 2:
            return []
        return [s for s in self.slots if s is not None and s is not seq and s.group is seq.group and not s.finished
                and not s.cancelled and s.adapter == seq.adapter and np.array_equal(s.prompt, seq.prompt)]

    def _fork_donor(self, seq: Sequence) -> Optional[Sequence]:
        """A live member whose row already holds the first P - 1 prompt tokens (it may be decoding by now)."""
        need = len(seq.prompt) - 1
        return next((s for s in self._group_live(seq) if s.prefill_pos >= need), None)

    def _waits_for_donor(self, seq: Sequence) -> bool:
        """A member is still prefilling the prompt: ``seq`` stays at the head of ``pending`` until it is through (a donor that
        is cancelled or finishes meanwhile is no longer live, and ``seq`` is admitted the normal way)."""
        live = self._group_live(seq)
        return bool(live) and self._fork_donor(seq) is None

    def _admit(self, seq: Sequence, slot: int) -> None:
        eng = self.model.engine
        seq.slot = slot
        self.slots[slot] = seq
        if seq.max_tokens <= 0:
            self._finish(seq, "length")
            return
        self.kv.reset_row(slot)                   # (also clears the bias and the adapter of the row's previous occupant)
        if seq.adapter >= 0:                      # while the row is empty, ahead of the fork and of prefix_attach: K / V depend on it
            self.kv.set_row_adapter(slot, seq.adapter)
        if seq.logit_bias:                        # ahead of the row's first sampling step: the prefill below, or the last chunk
            self.kv.set_row_logit_bias(slot, seq.logit_bias)
        if seq.logprobs or seq.logprobs_at_temperature:
            self.kv.set_row_logprobs(slot, seq.logprobs, seq.logprobs_at_temperature)
        seq.prefill_pos = 0
        donor = self._fork_donor(seq)
        if donor is not None:                     # a sibling's row holds the prompt: its first P - 1 tokens, the last one runs here
            try:
                self.kv.fork_row(donor.slot, slot, len(seq.prompt) - 1)
                seq.prefill_pos = len(seq.prompt) - 1
                self.forks += 1
                self.fork_tokens += seq.prefill_pos
            except RuntimeError as e:             # no block for the tail, nothing has changed: the prompt runs as any other
                if "no block for the tail" not in str(e):
                    raise                         # (a failed launch is the step's failure, not an arena shortage)
                log.warning("sequence %d: fork_row found no block, prefilling the prompt", seq.id)
                donor = None
        if donor is None and self.prefix_cache:   # full blocks of an earlier prompt with the same prefix are mapped, not recomputed
            seq.prefill_pos = self.kv.prefix_attach(slot, seq.prompt)
            self.prefix_hit_tokens += seq.prefill_pos
        if self.chunk_tokens > 0:                 # the prompt enters the cache chunk by chunk, inside the decode steps
            return
        t0 = time.perf_counter()
        res = eng.step_wait(eng.step_enqueue_rows(self.kv, [slot], seq.prompt[None, seq.prefill_pos:], self._sample_args([seq])), 1)
        self.prefills += 1
        seq.prefill_pos, seq.prefilled = len(seq.prompt), True
        if self.prefix_cache:
            self.kv.prefix_publish(slot, seq.prompt)
        if self.metrics is not None:
            self.metrics.record_throughput({"prompt_tokens": float(len(seq.prompt)), "prompt_time": time.perf_counter() - t0})
        self._on_token(seq, int(res["tokens"][0]), res, 0)

    def _mixed_step(self, decoding: List[Sequence], prefilling: List[Sequence]) -> None:
        """One pass over the weights: every live row decodes one token AND up to `chunk_tokens` prompt tokens of the
        arriving sequences (oldest first) enter the cache.  A sequence whose prompt is complete gets its first token
        from this same step."""
        eng = self.model.engine
        rows, toks, want, who = [], [], [], []
        for s in decoding:
            rows.append(s.slot); toks.append([s.last_token]); want.append(1); who.append(s)
        budget = self.chunk_tokens
        if self.step_rows > 0:
            budget = min(budget, max(16, self.step_rows - len(decoding)))
        n_chunk_tokens = 0
        for s in prefilling:
            if budget <= 0:
                break
            n = min(len(s.prompt) - s.prefill_pos, budget)
            last = s.prefill_pos + n == len(s.prompt)
            rows.append(s.slot); toks.append(s.prompt[s.prefill_pos:s.prefill_pos + n]); want.append(1 if last else 0); who.append(s)
            budget -= n
            n_chunk_tokens += n
        # one-token segments first (the engine's decode group): a 1-token chunk is a decode-shaped segment too
        order = sorted(range(len(rows)), key=lambda i: 0 if len(toks[i]) == 1 else 1)
        rows, toks, want, who = [rows[i] for i in order], [toks[i] for i in order], [want[i] for i in order], [who[i] for i in order]
        wanted = [s for s, w in zip(who, want) if w]
        sp = self._sample_args(wanted) if wanted else None
        t0 = time.perf_counter()
        ticket = eng.step_enqueue_mixed(self.kv, rows, toks, want, sp)
        res = eng.step_wait(ticket, len(wanted))
        dt = time.perf_counter() - t0
        self.steps += 1
        self.mixed_steps += 1
        for s, tk in zip(who, toks):
            if s in prefilling:
                s.prefill_pos += len(tk)
                self.chunks += 1
                if self.prefix_cache and s.prefill_pos == len(s.prompt):
                    self.kv.prefix_publish(s.slot, s.prompt)      # (enqueued above: later readers are ordered behind it)
        for i, (s, t) in enumerate(zip(wanted, res["tokens"] if wanted else [])):
            if s in prefilling:
                s.prefilled = True
                self.prefills += 1
            if not s.finished:
                self._on_token(s, int(t), res, i)
        if self.metrics is not None:
            self.metrics.record_throughput({"decode_tokens": float(len(decoding)), "decode_time": dt,
                                            "prompt_tokens": float(n_chunk_tokens), "prompt_time": dt})

    def _release_finished(self) -> None:
        for i, s in enumerate(self.slots):
            if s is not None and s.cancelled and not s.finished:
                s.finished = "cancelled"
                self._emit(s, None, "cancelled")
            if s is not None and s.finished:
                self.slots[i] = None
                if self.paged:                 # the row's blocks go back to the arena now (waiting requests count on them)
                    self.kv.reset_row(i)       # (its logprobs setting goes with them)
                elif s.logprobs or s.logprobs_at_temperature:
                    self.kv.set_row_logprobs(i, 0, False)     # a contiguous row is reset at its next admission: clear now
                if not self.paged and s.adapter >= 0:
                    self.kv.reset_row(i)       # (an adapter can only leave an empty row: the reset clears it)

    def _drop_cancelled_pending(self) -> None:
        with self.cv:
            gone = [s for s in self.pending if s.cancelled]
            for s in gone:
                self.pending.remove(s)
        for s in gone:
            s.finished = "cancelled"
            self._emit(s, None, "cancelled")

    def _run(self) -> None:
        eng = self.model.engine
        inflight = None                      # (ticket, seqs) of a decode step that has been enqueued but not read
        sp_keep = []                         # SampleArgs of the steps in flight (their host arrays must stay alive)

        def drain():
            nonlocal inflight
            if inflight is not None:
                ticket, seqs = inflight
                res = eng.step_wait(ticket, len(seqs))
                for i, (s, t) in enumerate(zip(seqs, res["tokens"])):
                    if not s.finished:
                        self._on_token(s, int(t), res, i)
                inflight = None
                sp_keep.clear()
            with self.cv:
                self._step_pending = False
                self.cv.notify_all()

        while True:
            with self.cv:
                # (a finished sequence still in its slot is work too: its row gives its KV blocks back below, not at the next arrival)
                while not self._stop and not self.pending and inflight is None and not any(
                        s is not None for s in self.slots) and self._waiters == 0:
                    self.cv.wait(timeout=0.5)
                if self._stop:
                    break
                if self._waiters > 0 and inflight is None:
                    self.cv.wait(timeout=0.002)          # let the borrower take the mutex
            try:
                with self.engine_mutex:
                    # ---- admissions: one prefill per new sequence, on its own row
                    if inflight is not None and any(s.cancelled and not s.finished for s in inflight[1]):
                        drain()                              # the row set changes: finish the step in flight first
                    self._release_finished()
                    self._drop_cancelled_pending()
                    while True:
                        with self.cv:
                            free = [i for i, s in enumerate(self.slots) if s is None]
                            seq = self.pending[0] if (free and self.pending) else None
                            if seq is not None and self._waits_for_donor(seq):
                                seq = None                   # wait for the sibling's prefill: its row is forked then
                            elif seq is not None and not self._fits(seq):
                                if any(s is not None and not s.finished for s in self.slots):
                                    seq = None               # wait for blocks: a live sequence will give some back
                                else:
                                    self.pending.popleft()   # nothing is running and it still does not fit: it never will
                                    seq.finished = "error"
                                    self._emit(seq, "\n\nError during generation: prompt + max_tokens exceed the KV arena", "error")
                                    continue
                            elif seq is not None:
                                self.pending.popleft()
                        if seq is None:
                            break
                        drain()
                        self._admit(seq, free[0])
                        self._release_finished()
                    active = [s for s in self.slots if s is not None and not s.finished]
                    if not active:
                        drain()
                        continue
                    self.max_rows_seen = max(self.max_rows_seen, len(active))
                    prefilling = [s for s in active if not s.prefilled]
                    if prefilling:                           # chunked prefill rides in the live rows' decode step
                        drain()
                        prefilling.sort(key=lambda q: q.id)
                        self._mixed_step([s for s in active if s.prefilled and not s.finished], prefilling)
                        with self.cv:
                            self._step_pending = False
                            self.cv.notify_all()
                        continue
                    rows = [s.slot for s in active]
                    t0 = time.perf_counter()
                    if inflight is None:
                        sp = self._sample_args(active)
                        sp_keep.append(sp)
                        inflight = (eng.step_enqueue_rows(self.kv, rows, [[s.last_token] for s in active], sp), active)
                    # one step ahead while nothing asks for a change of the row set
                    nxt = None
                    with self.cv:
                        stable = not self.pending and self._waiters == 0
                    if stable and all(len(s.generated) + 2 <= s.max_tokens for s in active):
                        sp = self._sample_args(active)
                        sp_keep.append(sp)
                        nxt = (eng.step_enqueue_rows(self.kv, rows, None, sp), active)
                    ticket, seqs = inflight
                    res = eng.step_wait(ticket, len(seqs))
                    self.steps += 1
                    for i, (s, t) in enumerate(zip(seqs, res["tokens"])):
                        if not s.finished:
                            self._on_token(s, int(t), res, i)
                    inflight = nxt
                    if len(sp_keep) > 2:
                        del sp_keep[0]
                    if inflight is not None and any(s.finished for s in active):
                        drain()                              # the row set changes: finish the step in flight first
                    if self.metrics is not None:
                        self.metrics.record_throughput({"decode_tokens": float(len(active)),
                                                        "decode_time": time.perf_counter() - t0})
                    with self.cv:
                        must_yield = self._waiters > 0
                    if must_yield:
                        drain()
                    with self.cv:                            # (still inside the mutex: see _Borrow.__enter__)
                        self._step_pending = inflight is not None
                        self.cv.notify_all()
            except Exception as e:          # engine failure: fail every sequence, keep the thread alive
                log.exception("scheduler step failed")
                inflight = None
                with self.cv:
                    self._step_pending = False
                    self.cv.notify_all()
                for i, s in enumerate(self.slots):
                    if s is not None and not s.finished:
                        s.finished = "error"
                        self._emit(s, f"\n\nError during generation: {e}", "error")
                    if s is not None and self.paged:
                        try:
                            self.kv.reset_row(i)             # the row's blocks go back to the arena
                        except Exception:
                            log.exception("could not release the KV row of a failed sequence")
                    self.slots[i] = None
        # shutdown: anything still queued or running is cut
        for s in list(self.pending) + [x for x in self.slots if x is not None]:
            if not s.finished:
                s.finished = "error"
                self._emit(s, None, "error")


class ReplicaPool:
    """One ContinuousScheduler per model replica (one replica per GPU, SURVEY §8e: sequences are independent, every
    GPU holds the full weights and its own KV rows, nothing crosses GPUs during decode).  A new sequence goes to
    the replica with the fewest sequences in flight; each replica steps on its own host thread."""

    def __init__(self, models, tokenizer, max_slots: int = 8, metrics=None, **kw):
        self.replicas: List[ContinuousScheduler] = [ContinuousScheduler(m, tokenizer, max_slots=max_slots, metrics=metrics, **kw)
                                                    for m in models]
        self._lock = threading.Lock()

    def _load(self, r: ContinuousScheduler) -> int:
        return len(r.pending) + sum(1 for s in r.slots if s is not None and not s.finished)

    def submit(self, prompt_ids, max_tokens: int, temp: float, top_p: float, sink: Sink, **controls) -> Sequence:
        with self._lock:                      # (choice and enqueue together, so concurrent submits spread out)
            group = controls.get("group")
            if group is not None and group.replica is not None:
                r = group.replica             # the members of a group share one cache: where the first one went
            else:
                r = min(self.replicas, key=self._load)
                if group is not None and r.fork_choices:      # (a replica that does not fork: its members spread as ever)
                    group.replica = r
            return r.submit(prompt_ids, max_tokens, temp, top_p, sink, **controls)

    def new_group(self) -> Group:
        return new_group()

    @property
    def forks(self) -> int:
        return sum(r.forks for r in self.replicas)

    @property
    def fork_tokens(self) -> int:
        return sum(r.fork_tokens for r in self.replicas)

    def start(self) -> None:
        for r in self.replicas:
            r.start()

    def stop(self) -> None:
        for r in self.replicas:
            r.stop()

    def borrow_engine(self):
        """Exclusive use of replica 0's engine (the model object the registry exposes)."""
        return self.replicas[0].borrow_engine()

    @property
    def max_rows_seen(self) -> int:
        return max(r.max_rows_seen for r in self.replicas)

    @property
    def borrows(self) -> int:
        return sum(r.borrows for r in self.replicas)
