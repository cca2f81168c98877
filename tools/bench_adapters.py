#!/usr/bin/env python3
"""What per-request LoRA adapters cost per decode step: bench.py's synthetic weights, device-synchronised step times.

Three engines of one model live side by side -- one that never saw an adapter, one with the engine-wide adapter of
mi_engine_set_lora (the table's private column, which every row runs), one with four adapters in the per-request slots of the
table (mi_engine_set_adapter_lora) -- every adapter rank 16 on
all seven linears of every block (scale 10, A ~ U(+-1/sqrt(K)), B ~ N(0, 0.01^2): bench.py's apply_lora recipe).  Five
configurations, ALTERNATED inside every repetition so that drift hits them alike:

    a  no adapter                          the plain engine
    b  engine-wide adapter                 the launches of d (per adapted block 4 down + 4 up-add launches and the SwiGLU: 9)
    c  table resident, every row on -1     must equal a: such a step runs the launches of an engine without adapters
    d  table, every row on adapter 0       must equal b
    e  table, rows spread over 4 adapters

Per configuration: a prefill of --context tokens, --warmup steps, then --reps x (--steps decode steps between two device
syncs); reported: median, min and max ms per step, the run-to-run spread (max - min of a), c - a, d - b, e - b, and (d - a)
per LoRA launch.

    python tools/bench_adapters.py [--out profiles/adapters_step_times.json]
    python tools/bench_adapters.py --only mistral-7b-bf16:8:model --reps 1          (one case: for a profiler)
    python tools/bench_adapters.py --twin       (adds a2: a SECOND engine without adapters -- what two instances of one
                                                 model differ by, the yardstick for c - a)
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

KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
        "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
DEFAULT_CASES = ["mistral-7b-bf16:8:model", "mistral-7b-bf16:8:float32", "qwen3-14b-int4:64:model"]
RANK, N_TABLE = 16, 4
LORA_LAUNCHES = 9                                   # per adapted block beside the four linears: 4 down, 4 up-add, the SwiGLU


def adapt(eng, cfg, gen, slot=None):
    """rank 16 on all seven linears of every block: the engine-wide adapter (slot None) or slot `slot` of the table"""
    H, nh, nkv, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["intermediate_size"]
    D = cfg.get("head_dim") or H // nh
    dims = {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}
    for li in range(cfg["num_hidden_layers"]):
        for key in KEYS:
            K, n = dims[key]
            a = (torch.rand((K, RANK), generator=gen) * 2 - 1) / (K ** 0.5)
            b = torch.randn((RANK, n), generator=gen) * 0.01
            if slot is None:
                eng.set_lora(li, key, a, b, 10.0)
            else:
                eng.set_adapter_lora(slot, li, key, a, b, 10.0)


class Leg:
    """One configuration: its engine, a cache of its own whose rows name `slots`, prefilled and warmed up."""

    def __init__(self, eng, cfg, B, kvd, slots, ctx, total_steps, sample):
        self.eng, self.B, self.sample = eng, B, sample
        self.kv = eng.new_kv(B, capacity=ctx + total_steps + 8, kv_dtype=kvd)
        for row, s in enumerate(slots):
            self.kv.set_row_adapter(row, s)
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], size=(B, ctx)).astype(np.int32)
        eng.step_wait(eng.step_enqueue(self.kv, prompts, sample), B)

    def run(self, steps):
        """`steps` decode steps between two device syncs -> ms per step (tokens stay on the device)"""
        self.eng.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            last = self.eng.step_enqueue(self.kv, None, self.sample)
        self.eng.step_wait(last, self.B)
        self.eng.sync()
        return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="workload:batch:kv_dtype (repeatable); default: %s" % " ".join(DEFAULT_CASES))
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin", action="store_true", help="add configuration a2: a second engine that never saw an adapter")
    ap.add_argument("--out")
    args = ap.parse_args()
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
        engines = {}
        for name in ("plain", "wide", "table") + (("twin",) if args.twin else ()):
            engines[name] = Engine(cfg, device=0, max_positions=4096, act_dtype="bfloat16")
            bench.load_synthetic(engines[name], cfg, 0, qb, 0, 1, None)
        gen = torch.Generator().manual_seed(99)
        adapt(engines["wide"], cfg, gen)
        for slot in range(N_TABLE):
            adapt(engines["table"], cfg, torch.Generator().manual_seed(99 + slot), slot)       # (slot 0 = the engine-wide factors)
        # bench.py's samplers: top-p 0.9 for the int4 configuration, greedy for bf16
        sample = SampleArgs(temp=1.0, top_p=0.9, seed=0) if qb else SampleArgs(temp=0.0)
        for B, kvd in legs:
            total = args.warmup + args.reps * args.steps
            conf = {"a": ("plain", [-1] * B), "b": ("wide", [-1] * B), "c": ("table", [-1] * B), "d": ("table", [0] * B),
                    "e": ("table", [i % N_TABLE for i in range(B)])}
            if args.twin:
                conf["a2"] = ("twin", [-1] * B)
            leg = {k: Leg(engines[e], cfg, B, kvd, slots, args.context, total, sample) for k, (e, slots) in conf.items()}
            for k in leg:
                leg[k].run(args.warmup)
            times = {k: [] for k in leg}
            for _ in range(args.reps):
                for k in leg:                                   # alternated: a b c d e, a b c d e, ...
                    times[k].append(leg[k].run(args.steps))
            for k in leg:
                leg[k].kv.close()
            med = {k: statistics.median(t) for k, t in times.items()}
            nl = cfg["num_hidden_layers"]
            row = dict(workload=wl, batch=B, kv_dtype=kvd, rank=RANK, adapted_layers=nl, context=args.context, steps=args.steps,
                       reps=args.reps, ms_per_step={k: dict(median=round(med[k], 4), min=round(min(t), 4), max=round(max(t), 4))
                                                    for k, t in times.items()},
                       spread_a_ms=round(max(times["a"]) - min(times["a"]), 4), c_minus_a_ms=round(med["c"] - med["a"], 4),
                       lora_launches_per_block=LORA_LAUNCHES,
                       d_minus_b_ms=round(med["d"] - med["b"], 4), e_minus_b_ms=round(med["e"] - med["b"], 4),
                       d_minus_a_us_per_lora_launch=round((med["d"] - med["a"]) * 1e3 / (nl * LORA_LAUNCHES), 3))
            if args.twin:
                row["a2_minus_a_ms"] = round(med["a2"] - med["a"], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        for e in engines.values():
            e.close()
        del engines
    if args.out:
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
