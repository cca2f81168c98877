#!/usr/bin/env python3
"""Launch time of the sampler's top-k logprobs, per form (the table next to LP_SELECT_MIN_K in csrc/misc.hip).

    python tools/bench_sampler_rowlp.py [--out bench_out/sampler_rowlp_launch_times.txt]

Runs itself as a child under ``rocprofv3 --kernel-trace`` and reads the kernel durations from the trace: greedy rows of
Gaussian logits, B in {8, 64} x V in {32000, 151936} x k in {0, 1, 5, 20} (and 2, 3, 4, 8, which locate the crossover),
REPS launches per cell after WARM warm-ups, the median duration of the sample_kernel launches of each cell.  Forms:
  rounds     k rounds of arg-max, the call-wide count (mi_op_sample_ex): what every launch ran before the row settings,
             and what a step costs in which the call-wide count makes every row pay for the most demanding one
  select     the selection on every row (mi_op_sample_rowlp, method 2, every row at k)
  mixed_row  half the rows at k, half at 0, per-row settings with the dispatch the engine uses (method 0)"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

BS, VS, KS = [8, 64], [32000, 151936], [0, 1, 2, 3, 4, 5, 8, 20]
FORMS = ["rounds", "select", "mixed_row"]
WARM, REPS = 3, 20


def child(plan_path):
    import numpy as np
    import torch

    from gpu_helpers import dev, dev_i32, ptr
    from mlx_parallm_amd import _lib as L

    rng = np.random.default_rng(0)
    plan = []
    for B in BS:
        for V in VS:
            lg = dev((rng.standard_normal((B, V)) * 3.0).astype(np.float32))
            toks = torch.zeros(B, dtype=torch.int32, device="cuda")
            lp = torch.zeros(B, dtype=torch.float32, device="cuda")
            ki = torch.zeros(B * 20, dtype=torch.int32, device="cuda")
            kl = torch.zeros(B * 20, dtype=torch.float32, device="cuda")
            st = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
            flag = dev_i32(np.zeros(B, np.int32))
            for k in KS:
                every = dev_i32(np.full(B, k, np.int32))
                half = dev_i32(np.where(np.arange(B) % 2 == 0, k, 0).astype(np.int32))

                def head(k_call):
                    return (ptr(lg), B, V, 0.0, 1.0, 0, 0.0, None, None, None, None, None, None, 0, 0, None, k_call, ptr(toks),
                            ptr(lp), None, ptr(ki), ptr(kl), ptr(st))

                for form in FORMS:
                    torch.cuda.synchronize()
                    for _ in range(WARM + REPS):
                        if form == "rounds":
                            L.check(L.lib().mi_op_sample_ex(*head(k)))
                        else:
                            tab, method = (every, 2) if form == "select" else (half, 0)
                            L.check(L.lib().mi_op_sample_rowlp(*head(0), 0, None, None, None, None, None, B, 0, None, ptr(tab),
                                                               ptr(flag), B, 0, method))
                    plan.append({"B": B, "V": V, "k": k, "form": form, "launches": WARM + REPS})
    Path(plan_path).write_text(json.dumps(plan))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "sampler_rowlp_launch_times.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    with tempfile.TemporaryDirectory() as d:
        plan_path = os.path.join(d, "plan.json")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(d, "trace"), "-o", "run", "--",
               sys.executable, str(Path(__file__).resolve()), "--child", plan_path]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        plan = json.loads(Path(plan_path).read_text())
        rows = []
        for f in Path(d, "trace").rglob("*_kernel_trace.csv"):
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    if "sample_kernel" in r["Kernel_Name"]:
                        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != sum(p["launches"] for p in plan):
        raise SystemExit(f"trace has {len(rows)} sampler launches, the plan {sum(p['launches'] for p in plan)}")
    us, at = {}, 0
    for p in plan:
        durs = [(e - s) / 1e3 for s, e in rows[at + WARM:at + p["launches"]]]
        at += p["launches"]
        us[p["B"], p["V"], p["k"], p["form"]] = statistics.median(durs)
    lines = [f"# sample_kernel launch time, us (median of {REPS} launches after {WARM} warm-ups; rocprofv3 --kernel-trace; greedy rows)",
             "# rounds = k rounds, call-wide count (also what a mixed step costs when the call-wide count makes every row pay);",
             "# select = the selection on every row; mixed_row = half the rows at k and half at 0, per-row settings, engine dispatch",
             f"{'B':>3} {'V':>7} {'k':>3} {'rounds':>9} {'select':>9} {'mixed_row':>10}"]
    for B in BS:
        for V in VS:
            for k in KS:
                lines.append(f"{B:>3} {V:>7} {k:>3} " + " ".join(f"{us[B, V, k, f]:>{w}.1f}" for f, w in zip(FORMS, (9, 9, 10))))
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
