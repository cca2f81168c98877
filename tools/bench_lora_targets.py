#!/usr/bin/env python3
"""What LoRA on more projections costs per decode step: bench.py's synthetic weights, device-synchronised step times.

For each workload (default: Qwen3-14B int4 at B = 64 in the model-dtype KV mode -- BASELINE config 5's regime -- and
Mistral-7B bf16 at B = 8 in both KV modes) one engine is loaded once and adapted in stages on the last --layers blocks:

    none  ->  {q, v}  ->  {q, k, v}  ->  all seven linears

(rank 16, scale 10, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.01^2): bench.py's apply_lora recipe).  After every stage: a prefill of
--context tokens, --warmup steps, then the median over --reps of (--steps decode steps between two device syncs).  The
difference between {q, k, v} and {q, v} is the third q|k|v range (lora_down3_kernel instead of lora_down_kernel, one
lora_up_add3_kernel launch per adapted block); between all seven and {q, k, v}: o and down in their epilogues and the adapted
gate|up -- plain-store linear + swiglu_rows_kernel instead of the fused SwiGLU epilogue.

    python tools/bench_lora_targets.py [--out profiles/lora_targets_step_times.json]
    python tools/bench_lora_targets.py --only qwen3-14b-int4:64:model --stages all7 --reps 1     (one case: for a profiler)
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import bench
from mlx_parallm_amd.engine import Engine, SampleArgs

STAGES = {"qv": ("self_attn.q_proj", "self_attn.v_proj"),
          "qkv": ("self_attn.k_proj",),
          "all7": ("self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}      # what each stage ADDS
DEFAULT_CASES = ["qwen3-14b-int4:64:model", "mistral-7b-bf16:8:model", "mistral-7b-bf16:8:float32"]


def add_keys(eng, cfg, keys, layers, gen):
    H, nh, nkv, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["intermediate_size"]
    D = cfg.get("head_dim") or H // nh
    dims = {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}
    for li in range(cfg["num_hidden_layers"] - layers, cfg["num_hidden_layers"]):
        for key in keys:
            K, n = dims[key]
            a = (torch.rand((K, 16), generator=gen) * 2 - 1) / (K ** 0.5)
            b = torch.randn((16, n), generator=gen) * 0.01
            eng.set_lora(li, key, a, b, 10.0)


def step_ms(eng, cfg, B, kvd, ctx, steps, warmup, reps, sample):
    prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], size=(B, ctx)).astype(np.int32)
    kv = eng.new_kv(B, capacity=ctx + warmup + reps * steps + 8, kv_dtype=kvd)
    eng.step_wait(eng.step_enqueue(kv, prompts, sample), B)
    for _ in range(warmup):
        last = eng.step_enqueue(kv, None, sample)
    eng.step_wait(last, B)
    times = []
    for _ in range(reps):
        eng.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            last = eng.step_enqueue(kv, None, sample)          # tokens stay on the device
        eng.step_wait(last, B)
        eng.sync()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    kv.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="workload:batch:kv_dtype (repeatable); default: %s" % " ".join(DEFAULT_CASES))
    ap.add_argument("--stages", default="none,qv,qkv,all7", help="which stages are TIMED (all are applied in order up to the last one named)")
    ap.add_argument("--layers", type=int, default=8, help="adapted blocks (the last N)")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    timed = args.stages.split(",")
    order = ["none"] + list(STAGES)
    last_stage = max(order.index(s) for s in timed)
    cases = {}
    for c in args.only or DEFAULT_CASES:
        wl, B, kvd = c.split(":")
        cases.setdefault(wl, []).append((int(B), kvd))
    torch.cuda.set_device(0)
    rows = []
    for wl, legs in cases.items():
        family, prec = wl.rsplit("-", 1)
        qb = {"int4": 4, "int8": 8}.get(prec, 0)
        cfg = dict(bench.SHAPES[family])
        if qb:
            cfg["quantization"] = {"group_size": 64, "bits": qb}
        eng = Engine(cfg, device=0, max_positions=4096, act_dtype="bfloat16")
        bench.load_synthetic(eng, cfg, 0, qb, 0, 1, None)
        # bench.py's samplers: top-p 0.9 with logprobs for the int4 configuration, greedy for bf16
        sample = SampleArgs(temp=1.0, top_p=0.9, seed=0) if qb else SampleArgs(temp=0.0)
        gen = torch.Generator().manual_seed(99)
        for stage in order[: last_stage + 1]:
            if stage != "none":
                add_keys(eng, cfg, STAGES[stage], args.layers, gen)
            if stage not in timed:
                continue
            for B, kvd in legs:
                t = step_ms(eng, cfg, B, kvd, args.context, args.steps, args.warmup, args.reps, sample)
                row = dict(workload=wl, batch=B, kv_dtype=kvd, adapted=stage, adapted_layers=args.layers if stage != "none" else 0,
                           context=args.context, steps=args.steps, ms_per_step_median=round(statistics.median(t), 4),
                           ms_per_step_min=round(min(t), 4), ms_per_step_max=round(max(t), 4))
                rows.append(row)
                print(json.dumps(row), flush=True)
        eng.close()
        del eng
    if args.out:
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
