#!/usr/bin/env python3
"""What logprobs requests cost the OTHER rows of a continuous batch.

    python tools/bench_scheduler_logprobs.py [--out bench_out/scheduler_logprobs.json]

The Mistral-7B-shaped random bf16 model of bench.py, a ContinuousScheduler with 8 slots.  Four plain greedy sequences
(128-token prompts, 256 tokens each) run next to four clients that keep asking for 64 tokens with ``logprobs: 5``
(128-token prompts, greedy) until the plain sequences are done.  Two legs on one engine:
  scheduled  the four clients submit to the scheduler: their sequences are rows of the shared steps
  exclusive  the four clients do what the server did before: one at a time, ``borrow_engine()`` and a batch-1
             ``generate_step`` with ``top_logprobs = 5``, between two scheduler steps
Reported per leg: tokens/s of the four plain rows (4 x 256 / the time until the last of them finishes) and the logprobs
tokens the clients got in that time."""
import argparse
import json
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PLAIN, CLIENTS, PROMPT, N_PLAIN, N_LP, K = 4, 4, 128, 256, 64, 5


class StubTokenizer:
    """Token ids in, one character per token out: the scheduler only needs decode() and an EOS id (none here)."""
    eos_token_id = -1

    def decode(self, ids, **kw):
        return "x" * len(ids)


def leg(model, tok, mode, rng):
    import numpy as np

    from mlx_parallm_amd.server.scheduler import ContinuousScheduler
    from mlx_parallm_amd.utils import _take, generate_step

    V = model.engine.desc.vocab_size
    sched = ContinuousScheduler(model, tok, max_slots=PLAIN + CLIENTS, kv_dtype="float32", prefix_cache=False)
    left, all_done, lock = [PLAIN], threading.Event(), threading.Lock()
    lp_tokens = [0]
    t_end = [0.0]

    def plain_sink(seq, delta, reason):
        if reason is not None:
            with lock:
                left[0] -= 1
                if left[0] == 0:
                    t_end[0] = time.perf_counter()
                    all_done.set()

    def client(i):
        r = np.random.default_rng(100 + i)
        while not all_done.is_set():
            prompt = r.integers(3, V, size=PROMPT).astype(np.int32)
            if mode == "scheduled":
                ev = threading.Event()
                seq = sched.submit(prompt, N_LP, 0.0, 1.0, lambda s, d, why: ev.set() if why is not None else None, logprobs=K)
                while not ev.wait(timeout=0.05):
                    if all_done.is_set():
                        seq.cancel()
                n = len(seq.token_ids)
            else:
                with excl, sched.borrow_engine():
                    steps = generate_step(prompt[None], model, temp=0.0, top_p=1.0, cache=model.make_cache(1), top_logprobs=K,
                                          return_details=True)
                    n = sum(1 for _ in _take(steps, N_LP))
                    steps.close()
            with lock:
                if not all_done.is_set():
                    lp_tokens[0] += n

    excl = threading.Lock()
    prompts = [rng.integers(3, V, size=PROMPT).astype(np.int32) for _ in range(PLAIN)]
    sched.start()
    threads = [threading.Thread(target=client, args=(i,)) for i in range(CLIENTS)]
    t0 = time.perf_counter()
    for p in prompts:
        sched.submit(p, N_PLAIN, 0.0, 1.0, plain_sink)
    for th in threads:
        th.start()
    assert all_done.wait(timeout=600)
    for th in threads:
        th.join(timeout=120)
    out = {"plain_tokens_per_s": round(PLAIN * N_PLAIN / (t_end[0] - t0), 1), "seconds": round(t_end[0] - t0, 3),
           "logprobs_tokens_in_that_time": lp_tokens[0], "borrows": sched.borrows, "max_rows_seen": sched.max_rows_seen}
    sched.stop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "scheduler_logprobs.json"))
    a = ap.parse_args()
    import numpy as np

    import bench
    from mlx_parallm_amd.models.llama import Model, ModelArgs

    cfg = dict(bench.SHAPES["mistral-7b"])
    model = Model(ModelArgs.from_dict(cfg), config=cfg, dtype="bfloat16", max_positions=4096)
    bench.load_synthetic(model.engine, cfg, 0, 0, 0, 1, None)
    tok = StubTokenizer()
    res = {}
    for mode in ("scheduled", "exclusive", "scheduled", "exclusive"):       # (the first pair also warms the engine up)
        res.setdefault(mode, []).append(leg(model, tok, mode, np.random.default_rng(1)))
    res["workload"] = (f"mistral-7b bf16 random weights, {PLAIN} plain rows x {N_PLAIN} tokens next to {CLIENTS} clients asking "
                       f"{N_LP} tokens with logprobs {K}, prompts of {PROMPT} tokens, float32 KV")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    model.engine.close()


if __name__ == "__main__":
    main()
