#!/usr/bin/env python3
"""Launch time of the sampler, per instantiation of sample_kernel and per form of its top-k logprobs (the
table next to LP_SELECT_MIN_K in csrc/sampler.hip).

    python tools/bench_sampler.py [--out bench_out/sampler_launch_times.txt] [--ks 0,1,5,20] [--save-outputs cells.npz]

Runs itself as a child under ``rocprofv3 --kernel-trace`` and reads the kernel durations from the trace: rows of Gaussian
logits, B in {8, 64} x V in {32000, 151936}, REPS launches per cell after WARM warm-ups, the median duration of the
sample_kernel launches of each cell.  The library is the one ``MLX_PARALLM_AMD_LIB`` names, else the tree's own.
Draw cells (no top entries; the uniforms are injected, so a cell draws the same tokens under every library):
  greedy     mi_op_sample at T = 0: sample_kernel<false>, what the benchmark's decode step launches
  top_p      mi_op_sample at T = 0.7, top_p = 0.9: sample_kernel<false> with two descents
  ex         mi_op_sample_ex at T = 0.7, top_k = 50, min_p = 0.05: sample_kernel<true>
  rowbias    mi_op_sample_rowbias, greedy, 16 entries per row in the per-row table: sample_kernel<false, true>
Top-k logprobs cells, greedy rows, k in --ks (default: 0, 1, 5, 20 and 2, 3, 4, 8, which locate the crossover):
  rounds     k rounds of arg-max, the call-wide count (mi_op_sample_ex): what every launch ran before the row settings,
             and what a step costs in which the call-wide count makes every row pay for the most demanding one
  select     the selection on every row (mi_op_sample_rowlp, method 2, every row at k)
  mixed_row  half the rows at k, half at 0, per-row settings with the dispatch the engine uses (method 0)
--save-outputs keeps what the last launch of every cell wrote (tokens, logprobs, top ids and logprobs, row statistics): the
cells are seeded, so two libraries that compute the same write the same arrays."""
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
DRAWS = ["greedy", "top_p", "ex", "rowbias"]
FORMS = ["rounds", "select", "mixed_row"]
WARM, REPS = 3, 20
BIAS_CAP = 16


def child(plan_path, ks, save):
    import numpy as np
    import torch

    from gpu_helpers import dev, dev_i32, ptr
    from mlx_parallm_amd import _lib as L

    lib = L.lib()
    rng = np.random.default_rng(0)
    plan, saved = [], {}
    for B in BS:
        for V in VS:
            rows = (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
            lg = dev(rows)
            u = dev(rng.random(B).astype(np.float32))
            toks = torch.zeros(B, dtype=torch.int32, device="cuda")
            lp = torch.zeros(B, dtype=torch.float32, device="cuda")
            ki = torch.zeros(B * 20, dtype=torch.int32, device="cuda")
            kl = torch.zeros(B * 20, dtype=torch.float32, device="cuda")
            st = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
            flag = dev_i32(np.zeros(B, np.int32))
            # the per-row bias table: BIAS_CAP distinct ids per row, small values (every launch adds them to its own copy again)
            biased = dev(rows)
            b_cnt = dev_i32(np.full(B, BIAS_CAP, np.int32))
            b_ids = dev_i32(np.stack([rng.choice(V, size=BIAS_CAP, replace=False) for _ in range(B)]).astype(np.int32))
            b_val = dev(rng.uniform(-0.25, 0.25, size=(B, BIAS_CAP)).astype(np.float32))

            def ex_args(logits, temp, top_p, top_k, min_p, ud, k_call):
                return (ptr(logits), B, V, temp, top_p, top_k, min_p, None, None, None, None, None, None, 0, 0, ptr(ud), k_call,
                        ptr(toks), ptr(lp), None, ptr(ki), ptr(kl), ptr(st))

            def run(cell, k, launch):
                torch.cuda.synchronize()
                for _ in range(WARM + REPS):
                    L.check(launch())
                plan.append({"B": B, "V": V, "k": k, "form": cell, "launches": WARM + REPS})
                if save:
                    torch.cuda.synchronize()
                    for name, arr in (("tokens", toks), ("logprobs", lp), ("top_ids", ki), ("top_logprobs", kl), ("row_stats", st)):
                        saved[f"B{B}_V{V}_k{k}_{cell}/{name}"] = arr.cpu().numpy().copy()

            run("greedy", 0, lambda: lib.mi_op_sample(ptr(lg), B, V, 0.0, 1.0, None, 0, ptr(toks), ptr(lp), None, ptr(ki), ptr(kl), ptr(st)))
            run("top_p", 0, lambda: lib.mi_op_sample(ptr(lg), B, V, 0.7, 0.9, ptr(u), 0, ptr(toks), ptr(lp), None, ptr(ki), ptr(kl), ptr(st)))
            run("ex", 0, lambda: lib.mi_op_sample_ex(*ex_args(lg, 0.7, 1.0, 50, 0.05, u, 0)))
            run("rowbias", 0, lambda: lib.mi_op_sample_rowbias(*ex_args(biased, 0.0, 1.0, 0, 0.0, None, 0), 0, None, None, ptr(b_cnt),
                                                               ptr(b_ids), ptr(b_val), B, BIAS_CAP, None))
            for k in ks:
                every = dev_i32(np.full(B, k, np.int32))
                half = dev_i32(np.where(np.arange(B) % 2 == 0, k, 0).astype(np.int32))
                head0 = ex_args(lg, 0.0, 1.0, 0, 0.0, None, 0)
                run("rounds", k, lambda: lib.mi_op_sample_ex(*ex_args(lg, 0.0, 1.0, 0, 0.0, None, k)))
                run("select", k, lambda: lib.mi_op_sample_rowlp(*head0, 0, None, None, None, None, None, B, 0, None, ptr(every),
                                                                ptr(flag), B, 0, 2))
                run("mixed_row", k, lambda: lib.mi_op_sample_rowlp(*head0, 0, None, None, None, None, None, B, 0, None, ptr(half),
                                                                   ptr(flag), B, 0, 0))
    if save:
        np.savez(save, **saved)
    Path(plan_path).write_text(json.dumps(plan))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "sampler_launch_times.txt"))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="counts of top entries of the logprobs cells")
    ap.add_argument("--save-outputs", help="write every cell's outputs to this .npz")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",") if k != ""]
    if a.child:
        return child(a.child, ks, a.save_outputs)
    with tempfile.TemporaryDirectory() as d:
        plan_path = os.path.join(d, "plan.json")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(d, "trace"), "-o", "run", "--",
               sys.executable, str(Path(__file__).resolve()), "--child", plan_path, "--ks", a.ks]
        if a.save_outputs:
            Path(a.save_outputs).parent.mkdir(parents=True, exist_ok=True)
            cmd += ["--save-outputs", str(Path(a.save_outputs).resolve())]
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
    lines = [f"# sample_kernel launch time, us (median of {REPS} launches after {WARM} warm-ups; rocprofv3 --kernel-trace)",
             "# draw cells: greedy / top_p (T 0.7, top_p 0.9) = mi_op_sample; ex = top_k 50 + min_p 0.05; rowbias = greedy + a 16-entry row table",
             f"{'B':>3} {'V':>7} " + " ".join(f"{c:>9}" for c in DRAWS)]
    for B in BS:
        for V in VS:
            lines.append(f"{B:>3} {V:>7} " + " ".join(f"{us[B, V, 0, c]:>9.1f}" for c in DRAWS))
    lines += ["# top-k logprobs cells, greedy rows: rounds = k rounds, call-wide count (also what a mixed step costs when the call-wide",
              "# count makes every row pay); select = the selection on every row; mixed_row = half the rows at k and half at 0, per-row",
              "# settings, engine dispatch",
              f"{'B':>3} {'V':>7} {'k':>3} {'rounds':>9} {'select':>9} {'mixed_row':>10}"]
    for B in BS:
        for V in VS:
            for k in ks:
                lines.append(f"{B:>3} {V:>7} {k:>3} " + " ".join(f"{us[B, V, k, f]:>{w}.1f}" for f, w in zip(FORMS, (9, 9, 10))))
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
