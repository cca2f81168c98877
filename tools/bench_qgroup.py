#!/usr/bin/env python3
"""A Mistral-7B-shaped engine at batch 8, KV 1024 -> 1100, 16-bit KV, int4 and int8 weights in quantisation groups of 32, 64
and 128, all from this build in one job: ms per step, tokens/s and the time of the gate|up launches (bench.py's timing protocol,
imported from it; its synthetic loader quantises in groups of 64, so the group is set on quant.quantize for the load)."""
import argparse
import functools
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

import bench
from mlx_parallm_amd import quant
from mlx_parallm_amd.engine import Engine, SampleArgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="4,8")
    ap.add_argument("--groups", default="32,64,128")
    ap.add_argument("--kv", default="model")
    ap.add_argument("--steps", type=int, default=76)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--out", default=None, help="also write the results as JSON lines to this file")
    args = ap.parse_args()
    a = bench.parse_args(["--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)])
    a.batch, a.no_prefill_timing, a.profile_kernel = 8, True, "gemv_gate_up"
    B, K, W, ctx = 8, args.steps, args.warmup, args.context
    cap = ctx + 2 * (K + W) + 136
    plain, lines = quant.quantize, []
    for bits in (int(b) for b in args.bits.split(",")):
        for group in (int(g) for g in args.groups.split(",")):
            cfg = dict(bench.SHAPES["mistral-7b"], quantization={"group_size": group, "bits": bits})
            eng = Engine(cfg, device=0, max_positions=max(cap, 2048), act_dtype="bfloat16")
            quant.quantize = functools.wraps(plain)(lambda t, _g, b, g=group: plain(t, g, b))
            try:
                bench.load_synthetic(eng, cfg, 0, bits, 0, 1, None)
            finally:
                quant.quantize = plain
            prompts = np.random.default_rng(23).integers(0, cfg["vocab_size"], size=(B, ctx)).astype(np.int32)
            for kvm in args.kv.split(","):
                leg = bench.decode_leg(eng, cfg, a, kvm, prompts, SampleArgs(temp=0.0), None, 1, cap, instrument=True)
                n = bench.numbers(cfg, bits, B, K, W, ctx, leg, kvm, "gemv_gate_up", 1)
                r = {"bits": bits, "group": group, "kv": kvm, "ms_per_step": round(n["ms_per_step"], 4),
                     "tokens_per_s": round(n["value"], 1), "gate_up_us": round(n["avg_ms"] * 1e3, 2), "launches": leg["n_launch"]}
                lines.append(r)
                print(json.dumps(r), flush=True)
            eng.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
