#!/usr/bin/env python3
"""Shared-prefix decode attention measured where it runs: a Mistral-7B-shaped engine (bench.py's random weights), a paged cache
of 64-token blocks, B rows that share a prompt of RUN + 5 tokens (prefilled once in row 0, forked into the others) or, with
--unrelated, share ONE block and hold the rest of their RUN + 5 tokens alone (what leaving the fused kernel costs rows that
share next to nothing).  Every layer has its own K/V, so no launch re-reads what the one before it read.

Per (kv dtype, run): decode steps alternate in blocks of `--block` steps between the option off and on (profiler off): the
median, lowest and highest ms per step of the `--reps` blocks of each.  Then, under the profiler, us per launch of the
families the two paths run: `attn` (the fused launch, option off) against `rope_append` + `attn_shared` (option on).  The
tails grow from 6 keys to about 6 + 2 reps block + 16 while this runs.

--tree DIR runs another checkout's package and library (the parent commit's: it has no option, so only its `off` numbers)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--runs", default="64,256,1024,4096")
    ap.add_argument("--kv", default="model,float32")
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--unrelated", action="store_true")
    ap.add_argument("--no-option", action="store_true", help="never set the option (a tree that does not have it)")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.tree)
    import bench
    from mlx_parallm_amd.engine import Engine, SampleArgs

    cfg = dict(bench.SHAPES["mistral-7b"])
    eng = Engine(cfg, device=0, max_positions=8192, act_dtype="bfloat16")
    bench.load_synthetic(eng, cfg, 1, 0, 0, 1, None)
    B, greedy = a.B, SampleArgs(temp=0.0)
    rng = np.random.default_rng(2)
    modes = ["off"] if a.no_option else ["off", "on"]

    def set_mode(m, run):
        if not a.no_option:
            eng.set_option("shared_prefix_attention", (64 if a.unrelated else max(run, 1)) if m == "on" else 0)

    for kvd in a.kv.split(","):
        for run in [int(x) for x in a.runs.split(",")]:
            P = run + 5
            kv = eng.new_paged_kv(B, block_tokens=64, max_tokens_per_row=P + 2 * a.reps * a.block + 96, kv_dtype=kvd)
            set_mode("off", run)
            first = 64 if a.unrelated else P                 # --unrelated: one shared block, then RUN + 5 - 64 tokens of each row's own
            eng.step_wait(eng.step_enqueue_rows(kv, [0], rng.integers(3, 32000, size=(1, first)).astype(np.int32), greedy), 1, 0)
            for r in range(1, B):
                kv.fork_row(0, r, first)
            for r in range(B if a.unrelated and P > first else 0):
                eng.step_wait(eng.step_enqueue_rows(kv, [r], rng.integers(3, 32000, size=(1, P - first)).astype(np.int32), greedy), 1, 0)
            tok = rng.integers(3, 32000, size=(B, 1)).astype(np.int32)
            for m in modes:                                  # warm both paths
                set_mode(m, run)
                eng.decode_sample(kv, tok, greedy)
            ms = {m: [] for m in modes}
            for _ in range(a.reps):
                for m in modes:
                    set_mode(m, run)
                    eng.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.block):
                        eng.decode_sample(kv, tok, greedy)
                    ms[m].append((time.perf_counter() - t0) * 1e3 / a.block)
            us = {}
            for m, fams in (("off", ["attn"]), ("on", ["rope_append", "attn_shared", "attn"])):
                if m not in modes:
                    continue
                set_mode(m, run)
                for fam in fams:
                    eng.profile_select(fam)
                    for _ in range(4):
                        eng.decode_sample(kv, tok, greedy)
                    n, tot = eng.profile_read()
                    us[f"{m}:{fam}"] = (n, tot * 1e3 / n if n else 0.0)
                eng.profile_select(None)
            steps = "  ".join(f"{m} {statistics.median(v):.3f} ms/step [{min(v):.3f} .. {max(v):.3f}]" for m, v in ms.items())
            launches = "  ".join(f"{k} {v[1]:.1f} us x{v[0]}" for k, v in us.items())
            print(f"kv {kvd:8s} {'unrelated' if a.unrelated else 'one set':9s} B {B} run {run:5d} keys {kv.offsets[0] + 1:4d} | {steps} | {launches}",
                  flush=True)
            kv.close()
    eng.close()


if __name__ == "__main__":
    main()
