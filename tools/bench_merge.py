#!/usr/bin/env python3
"""What merging an adapter saves per decode step: bench.py's synthetic Qwen3-14B int4 weights, a rank-8 LoRA adapter on all
seven projections of every block, once riding beside the weights (the by-row adapter path: two small launches around every
adapted linear, gate|up unfused) and once merged into them (``mi_lora_merge``, re-quantised: a plain model).

Two engines live side by side on one device; after a prefill of --context tokens and --warmup steps each, the timed windows
(--steps decode steps between two device syncs) ALTERNATE between them --reps times, so both see the same machine state.
Prints one JSON line per window, then the medians, the difference per adapted layer and what the merge itself took.

    python tools/bench_merge.py [--out profiles/merge_step_times.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import bench
from mlx_parallm_amd import _lib as L
from mlx_parallm_amd.engine import Engine, SampleArgs

KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def dims(cfg):
    H, nh, nkv, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["intermediate_size"]
    D = cfg.get("head_dim") or H // nh
    return {"self_attn.q_proj": (H, nh * D), "self_attn.k_proj": (H, nkv * D), "self_attn.v_proj": (H, nkv * D),
            "self_attn.o_proj": (nh * D, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}


def factors(cfg, rank, layers):
    """(layer, key) -> (A (K, r), B (r, N)) on the device: bench.py's apply_lora recipe at the given rank"""
    gen = torch.Generator().manual_seed(99)
    out = {}
    for li in range(cfg["num_hidden_layers"] - layers, cfg["num_hidden_layers"]):
        for key in KEYS:
            K, n = dims(cfg)[key]
            out[li, key] = (((torch.rand((K, rank), generator=gen) * 2 - 1) / (K ** 0.5)).cuda(), (torch.randn((rank, n), generator=gen) * 0.01).cuda())
    return out


class MergingEngine:
    """What bench.load_synthetic feeds instead of the engine: the packed triple of an adapted projection is held back until it
    is complete, merged on the device and handed on re-quantised."""

    def __init__(self, engine, adapter, scale, bits):
        self.engine, self.adapter, self.scale, self.bits = engine, adapter, scale, bits
        self.parts, self.merged, self.seconds = {}, 0, 0.0

    def set_tensor(self, name, t):
        base, _, leaf = name.rpartition(".")
        li_key = None
        if base.startswith("model.layers."):
            _m, _l, li, key = base.split(".", 3)
            li_key = (int(li), key)
        if li_key not in self.adapter or leaf not in ("weight", "scales", "biases"):
            return self.engine.set_tensor(name, t)
        held = self.parts.setdefault(li_key, {})
        held[leaf] = t
        if len(held) < 3:
            return None
        w, sc, bi = held["weight"].contiguous(), held["scales"].contiguous(), held["biases"].contiguous()
        a, b = self.adapter[li_key]
        N, K = int(w.shape[0]), int(w.shape[1]) * 32 // self.bits
        ow, osc, obi = torch.empty_like(w), torch.empty_like(sc), torch.empty_like(bi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = lambda x: C.c_void_p(x.data_ptr())                                  # noqa: E731
        L.check(L.lib().mi_lora_merge(0, N, K, int(a.shape[1]), L.MI_BF16, self.bits, 64, P(w), P(sc), P(bi), P(a), P(b), None,
                                      float(self.scale), 1, P(ow), P(osc), P(obi)))
        self.seconds += time.perf_counter() - t0
        self.merged += 1
        del self.parts[li_key]
        for leaf2, out in (("weight", ow), ("scales", osc), ("biases", obi)):
            self.engine.set_tensor(f"{base}.{leaf2}", out)
        return None

    def finalize(self):
        assert not self.parts, "an adapted projection never got its triple"
        self.engine.finalize()


def prepare(eng, cfg, B, kvd, ctx, warmup, window, reps, sample):
    prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], size=(B, ctx)).astype(np.int32)
    kv = eng.new_kv(B, capacity=ctx + warmup + reps * window + 8, kv_dtype=kvd)
    eng.step_wait(eng.step_enqueue(kv, prompts, sample), B)
    for _ in range(warmup):
        last = eng.step_enqueue(kv, None, sample)
    eng.step_wait(last, B)
    return kv


def window_ms(eng, kv, B, steps, sample):
    eng.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = eng.step_enqueue(kv, None, sample)              # tokens stay on the device
    eng.step_wait(last, B)
    eng.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="qwen3-14b")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--layers", type=int, default=None, help="adapted blocks (the last N; default: all)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--kv-dtype", default="model")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = dict(bench.SHAPES[args.workload])
    cfg["quantization"] = {"group_size": 64, "bits": args.bits}
    layers = args.layers or cfg["num_hidden_layers"]
    adapter = factors(cfg, args.rank, layers)
    sample = SampleArgs(temp=1.0, top_p=0.9, seed=0)          # bench.py's sampler of the int4 configuration

    by_row = Engine(cfg, device=0, max_positions=4096, act_dtype="bfloat16")
    bench.load_synthetic(by_row, cfg, 0, args.bits, 0, 1, None)
    for (li, key), (a, b) in adapter.items():
        by_row.set_lora(li, key, a, b, args.scale)
    merged = Engine(cfg, device=0, max_positions=4096, act_dtype="bfloat16")
    feeder = MergingEngine(merged, adapter, args.scale, args.bits)
    bench.load_synthetic(feeder, cfg, 0, args.bits, 0, 1, None)
    assert feeder.merged == len(adapter)

    engines = {"by_row": by_row, "merged": merged}
    kvs = {k: prepare(e, cfg, args.batch, args.kv_dtype, args.context, args.warmup, args.steps, args.reps, sample) for k, e in engines.items()}
    times = {k: [] for k in engines}
    rows = []
    for rep in range(args.reps):
        for k, e in engines.items():                           # alternating
            ms = window_ms(e, kvs[k], args.batch, args.steps, sample)
            times[k].append(ms)
            rows.append(dict(engine=k, rep=rep, ms_per_step=round(ms, 4)))
            print(json.dumps(rows[-1]), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    summary = dict(workload=f"{args.workload}-int{args.bits}", batch=args.batch, kv_dtype=args.kv_dtype, rank=args.rank,
                   adapted_layers=layers, adapted_projections=len(adapter), context=args.context, steps=args.steps, reps=args.reps,
                   by_row_ms_median=round(med["by_row"], 4), by_row_ms_min=round(min(times["by_row"]), 4), by_row_ms_max=round(max(times["by_row"]), 4),
                   merged_ms_median=round(med["merged"], 4), merged_ms_min=round(min(times["merged"]), 4), merged_ms_max=round(max(times["merged"]), 4),
                   saved_us_per_adapted_layer=round((med["by_row"] - med["merged"]) * 1e3 / layers, 2),
                   merge_seconds_total=round(feeder.seconds, 3), merge_ms_per_projection=round(feeder.seconds * 1e3 / len(adapter), 3))
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(dict(summary=summary, windows=rows), indent=1) + "\n")
    for kv in kvs.values():
        kv.close()
    by_row.close(); merged.close()


if __name__ == "__main__":
    main()
