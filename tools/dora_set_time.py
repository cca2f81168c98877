"""What a hot-swap of one adapter costs: wall time around ``utils.load_adapter_into`` for a DoRA adapter and for the same factors
as plain LoRA (DESIGN §5 "DoRA", set time).  A bench.py workload shape with random-init bf16 weights, rank-16 factors on all
seven projections of every block, read from an adapter directory as a serving process or an RL loop would.

    python tools/dora_set_time.py [--shape mistral-7b] [--rank 16] [--reps 3]

Prints one line per kind: the repetitions and their median, in milliseconds (the first load of each kind allocates the tables)."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
from safetensors.torch import save_file

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import Engine  # noqa: E402

KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def write(dst: Path, cfg: dict, rank: int, kind: str) -> str:
    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv, D, I = cfg["num_key_value_heads"], cfg.get("head_dim") or H // nh, cfg["intermediate_size"]
    dims = dict(zip(KEYS, ((H, nh * D), (H, nkv * D), (H, nkv * D), (nh * D, H), (H, I), (H, I), (I, H))))
    g = torch.Generator().manual_seed(1)
    t = {}
    for i in range(cfg["num_hidden_layers"]):
        for key in KEYS:
            K, n = dims[key]
            base = f"model.layers.{i}.{key}"
            t[base + ".lora_a"] = torch.randn((K, rank), generator=g) * 0.01
            t[base + ".lora_b"] = torch.randn((rank, n), generator=g) * 0.01
            if kind == "dora":
                t[base + ".m"] = 0.5 + torch.rand(n, generator=g)
    dst.mkdir(parents=True, exist_ok=True)
    save_file(t, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": kind, "num_layers": cfg["num_hidden_layers"],
        "lora_parameters": {"rank": rank, "scale": 10.0, "dropout": 0.0, "keys": list(KEYS)}}))
    return str(dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="mistral-7b", choices=sorted(bench.SHAPES))
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    cfg = dict(bench.SHAPES[args.shape])
    eng = Engine(cfg, device=0, max_positions=2048, act_dtype="bfloat16")
    bench.load_synthetic(eng, cfg, 0, 0, 0, 1, None)
    model = SimpleNamespace(layers=[None] * cfg["num_hidden_layers"], engine=eng)
    with tempfile.TemporaryDirectory() as td:
        dirs = {kind: write(Path(td) / kind, cfg, args.rank, kind) for kind in ("lora", "dora")}
        times = {"lora": [], "dora": []}
        for _ in range(args.reps + 1):                     # (the first round allocates the tables: dropped)
            for kind in ("lora", "dora"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                utils.load_adapter_into(model, 0, dirs[kind])
                eng.sync()
                times[kind].append((time.perf_counter() - t0) * 1e3)
    for kind, ts in times.items():
        print(f"{args.shape} bf16, rank {args.rank}, {len(KEYS)} projections x {cfg['num_hidden_layers']} blocks, load_adapter_into as {kind}: "
              f"{', '.join(f'{t:.0f}' for t in ts[1:])} ms (median {statistics.median(ts[1:]):.0f} ms; first load {ts[0]:.0f} ms)")
    eng.close()


if __name__ == "__main__":
    main()
