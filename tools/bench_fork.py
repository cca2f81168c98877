#!/usr/bin/env python3
"""What forking KV rows buys the n choices of one request.

    python tools/bench_fork.py [--fork-choices] [--reps 4] [--out bench_out/fork.json]

The Mistral-7B-shaped random bf16 model of bench.py with 16-bit KV, a ContinuousScheduler with 8 slots and its defaults
(paged arena of 64-token blocks, 256-token chunks, prefix cache on).  One request: n = 8 greedy choices of one 1024-token
prompt, 64 tokens each, submitted together.  Reported per repetition (the first one also warms the engine up):
  first_token_ms   from the first submit to the moment the LAST choice's sink has its first token
  blocks_in_use    arena blocks held right after that (usable - free, read between two steps)
  prompt_steps     mixed steps that carried prompt tokens
and, with --fork-choices, fork_row_us: the wall time of one KVCache.fork_row of 1023 tokens (15 shared blocks, a 63-token
tail copied) from call to the engine's stream being idle again, median and range of 20.

Without --fork-choices nothing of the fork interface is touched: the same file measures the commit before it."""
import argparse
import json
import statistics
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, PROMPT, NEW = 8, 1024, 64


class StubTokenizer:
    """Token ids in, one character per token out: the scheduler only needs decode() and an EOS id (none here)."""
    eos_token_id = -1

    def decode(self, ids, **kw):
        return "x" * len(ids)


def one_request(sched, prompt, fork):
    first, lock, all_first, all_done = {}, threading.Lock(), threading.Event(), threading.Event()
    done = [0]

    def sink(seq, delta, reason):                     # the stub decodes every token to one character: a delta per token
        with lock:
            if seq.id not in first:
                first[seq.id] = time.perf_counter()
                if len(first) == N:
                    all_first.set()
            if reason is not None:
                done[0] += 1
                if done[0] == N:
                    all_done.set()

    steps0, forks0 = sched.mixed_steps, getattr(sched, "forks", 0)
    kw = {"group": sched.new_group()} if fork else {}
    t0 = time.perf_counter()
    for _ in range(N):
        sched.submit(prompt, NEW, 0.0, 1.0, sink, **kw)
    assert all_first.wait(timeout=300)
    t_first = max(first.values())
    with sched.borrow_engine():
        st = sched.kv.stats()
        prompt_steps = sched.mixed_steps - steps0
    assert all_done.wait(timeout=300)
    deadline = time.perf_counter() + 60
    while True:                                       # the finished rows give their blocks back: what is still held is the cache's
        with sched.borrow_engine():
            now = sched.kv.stats()
        if now["usable_blocks"] - now["free_blocks"] == now["cached_blocks"]:
            break
        assert time.perf_counter() < deadline, now
        threading.Event().wait(0.005)
    return {"first_token_ms": round((t_first - t0) * 1e3, 2), "blocks_in_use": st["usable_blocks"] - st["free_blocks"],
            "prompt_steps": prompt_steps, "forks": getattr(sched, "forks", 0) - forks0}


def fork_launch_us(sched, prompt):
    eng, kv = sched.model.engine, sched.kv
    from mlx_parallm_amd.engine import SampleArgs

    with sched.borrow_engine():
        kv.reset_row(0)
        eng.step_wait(eng.step_enqueue_rows(kv, [0], prompt[None, :PROMPT - 1], SampleArgs(temp=0.0)), 1)
        us = []
        for _ in range(21):
            kv.reset_row(1)
            eng.sync()
            t0 = time.perf_counter()
            kv.fork_row(0, 1, PROMPT - 1)
            eng.sync()
            us.append((time.perf_counter() - t0) * 1e6)
        kv.reset_row(0); kv.reset_row(1)
    us = us[1:]
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fork-choices", action="store_true")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "fork.json"))
    a = ap.parse_args()
    import numpy as np

    import bench
    from mlx_parallm_amd.models.llama import Model, ModelArgs
    from mlx_parallm_amd.server.scheduler import ContinuousScheduler

    cfg = dict(bench.SHAPES["mistral-7b"])
    model = Model(ModelArgs.from_dict(cfg), config=cfg, dtype="bfloat16", max_positions=2048)
    bench.load_synthetic(model.engine, cfg, 0, 0, 0, 1, None)
    kw = {"fork_choices": True} if a.fork_choices else {}
    sched = ContinuousScheduler(model, StubTokenizer(), max_slots=N, kv_dtype="model", **kw)
    sched.start()
    rng = np.random.default_rng(1)
    V = model.engine.desc.vocab_size
    res = {"fork_choices": bool(a.fork_choices), "reps": []}
    for _ in range(a.reps):                           # a new prompt each time: nothing comes from the prefix cache
        res["reps"].append(one_request(sched, rng.integers(3, V, size=PROMPT).astype(np.int32), a.fork_choices))
    if a.fork_choices:
        res["fork_row_us"] = fork_launch_us(sched, rng.integers(3, V, size=PROMPT).astype(np.int32))
    res["workload"] = (f"mistral-7b bf16 random weights, 16-bit KV, n = {N} greedy choices of one {PROMPT}-token prompt, "
                       f"{NEW} tokens each, scheduler defaults")
    sched.stop()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    model.engine.close()


if __name__ == "__main__":
    main()
