#!/usr/bin/env python3
"""mxfp4 (gemm_mx4.hip) against affine int4 in groups of 32 (gemm_qg.hip) and 64 (gemm_skinny.hip / gemm_q4.hip), one build.

Kernels (default): mi_op_gemm_skinny at the three Mistral-7B linear shapes, 1 / 8 / 64 rows of bf16 activations.  A sample is
the mean of --iters back-to-back launches behind a warm one (HIP events inside the call); --rounds samples per case, the kinds
ALTERNATING inside a round; reported: the median and the lowest / highest sample, and the weight bytes over the median.  The
launches repeat on one matrix that stays in the last-level cache: cache rates, not HBM rates.

--step: a Mistral-7B-shaped engine at batch 8, 16-bit KV 1024 -> 1100, on mxfp4 and on int4 group-32 weights (random codes and
scales set directly, as a checkpoint would give them), bench.py's timing protocol, --rounds legs per engine, alternating.

--prefill: the four Mistral-7B linears with their epilogues (q|k|v store, o residual, gate|up SwiGLU, down residual) at 256 ..
8192 rows of bf16 activations, per launch: mi_op_gemm_prefill_q on the packed mxfp4 matrix (qtile_mx4_kernel), mi_op_gemm_prefill
on the same matrix (the bf16 copy written per call + the dense tile GEMM) and mi_op_gemm_prefill on a dense bf16 matrix of the
same shape; the routes ALTERNATE inside a round, medians of --rounds samples.  A sample is at least --iters launches (default
20 in this mode) and at least ~5 ms of work (counted at 1 PFLOP/s), so the small shapes repeat a few hundred times; the residual
epilogues start every sample from a zeroed stream.

--fp8: the 8-bit family instead -- mxfp8 (gemm_mx8.hip) against affine int8 in groups of 32 (gemm_qg.hip) and 64
(gemm_skinny.hip), in the kernel mode (with the o shape added) and in --step."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import bench
from mlx_parallm_amd import _lib as L
from mlx_parallm_amd.engine import Engine, SampleArgs

SHAPES = {"qkv": (6144, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
KINDS = {"mxfp4": ("mx4_bf16", 32), "int4_g32": ("q4_bf16", 32), "int4_g64": ("q4_bf16", 64)}
SHAPES8 = dict(SHAPES, o=(4096, 4096))
KINDS8 = {"mxfp8": ("mx8_bf16", 32), "int8_g32": ("q8_bf16", 32), "int8_g64": ("q8_bf16", 64)}


def bits_of(kind):
    return 8 if kind[:3] in ("mx8", "q8_") else 4


def random_linear(kind, group, N, K, gen):
    """-> [codes, scales(, biases)] as a checkpoint holds them (weights of about N(0, 0.02^2)), on the device"""
    bits = bits_of(kind)
    t = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K * bits // 32), dtype=torch.int32, generator=gen).cuda()]
    if kind.startswith("mx8"):
        t[0] &= -16843010                                    # 0xfefefefe: no byte is a NaN code (0x7f / 0xff)
        return t + [torch.randint(111, 114, (N, K // 32), dtype=torch.uint8, generator=gen).cuda()]
    if kind.startswith("mx4"):
        return t + [torch.randint(117, 120, (N, K // 32), dtype=torch.uint8, generator=gen).cuda()]
    s = (torch.rand((N, K // group), generator=gen) * 0.004 + 0.004).to(torch.bfloat16) / (16 if bits == 8 else 1)
    return t + [s.cuda(), (s * -(2 ** (bits - 1) - 0.5)).cuda()]


def tiled(kind, group, N, K):
    keep = random_linear(kind, group, N, K, torch.Generator().manual_seed(N + K))
    ol = L.OpLinear()
    ol.wk, ol.N, ol.K, ol.group = L.WK[kind], N, K, group
    ol.w, ol.scales = keep[0].data_ptr(), keep[1].data_ptr()
    ol.biases = keep[2].data_ptr() if len(keep) > 2 else 0
    dst = torch.zeros(int(L.lib().mi_op_tiled_bytes(C.byref(ol))), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_repack_tiled(C.byref(ol), C.c_void_p(dst.data_ptr())))
    ol.w, ol.scales, ol.biases, ol.layout = dst.data_ptr(), 0, 0, 1
    return ol, dst, N * K * bits_of(kind) // 8 + N * (K // group) * (1 if kind.startswith("mx") else 4)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def kernels(args, emit):
    for shape, (N, K) in (SHAPES8 if args.fp8 else SHAPES).items():
        lin = {name: tiled(kind, group, N, K) for name, (kind, group) in (KINDS8 if args.fp8 else KINDS).items()}
        for M in (int(r) for r in args.rows.split(",")):
            x = torch.randn((M, K), dtype=torch.bfloat16, device="cuda")
            out = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
            a = L.OpGemvArgs()
            a.x, a.ldx, a.M, a.act, a.ldo, a.out = x.data_ptr(), K, M, L.MI_BF16, N, out.data_ptr()
            torch.cuda.synchronize()
            us = {name: [] for name in lin}
            for _ in range(args.rounds):
                for name, (ol, _, _) in lin.items():
                    used, ms = C.c_int(0), C.c_float(0.0)
                    L.check(L.lib().mi_op_gemm_skinny(C.byref(ol), C.byref(a), 0, C.byref(used), args.iters, C.byref(ms)))
                    us[name].append(ms.value * 1e3)
            for name, v in us.items():
                emit({"shape": shape, "kind": name, "rows": M, "us": spread(v),
                      "weight_GBps": round(lin[name][2] / (statistics.median(v) * 1e-6) / 1e9, 1)})


PREFILL = {"qkv": (6144, 4096, "store"), "o": (4096, 4096, "resid"), "gate_up": (28672, 4096, "swiglu"), "down": (4096, 14336, "resid")}


def prefill(args, emit):
    lib = L.lib()
    for shape, (N, K, epi) in PREFILL.items():
        mx, mx_keep, _ = tiled("mx4_bf16", 32, N, K)
        wd = (torch.randn((N, K), generator=torch.Generator().manual_seed(N), dtype=torch.float32) * 0.02).to(torch.bfloat16).cuda()
        dn = L.OpLinear()
        dn.wk, dn.N, dn.K, dn.group, dn.w = L.WK["bf16"], N, K, 64, wd.data_ptr()
        dt = torch.zeros(int(lib.mi_op_tiled_bytes(C.byref(dn))), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        L.check(lib.mi_op_repack_tiled(C.byref(dn), C.c_void_p(dt.data_ptr())))
        dn.w, dn.layout = dt.data_ptr(), 1
        routes = {"tile_mx4": (lib.mi_op_gemm_prefill_q, mx), "copy_mx4": (lib.mi_op_gemm_prefill, mx), "dense_bf16": (lib.mi_op_gemm_prefill, dn)}
        for M in (int(r) for r in args.rows.split(",")):
            x = torch.randn((M, K), dtype=torch.bfloat16, device="cuda")
            No = N // 2 if epi == "swiglu" else N
            out = torch.zeros((M, No), dtype=torch.bfloat16, device="cuda")
            a = L.OpGemvArgs()
            a.x, a.ldx, a.M, a.act, a.ldo = x.data_ptr(), K, M, L.MI_BF16, No
            a.epi = {"store": L.EPI_STORE, "resid": L.EPI_RESID, "swiglu": L.EPI_SWIGLU}[epi]
            a.pair_offset = No if epi == "swiglu" else 0
            if epi == "resid":
                a.resid = out.data_ptr()
            else:
                a.out = out.data_ptr()
            iters = max(args.iters, int(5e-3 / (2.0 * M * N * K / 1e15)))
            us = {name: [] for name in routes}
            for _ in range(args.rounds):
                for name, (fn, ol) in routes.items():
                    ms = C.c_float(0.0)
                    out.zero_()
                    torch.cuda.synchronize()
                    L.check(fn(C.byref(ol), C.byref(a), iters, C.byref(ms)))
                    us[name].append(ms.value * 1e3)
            for name, v in us.items():
                emit({"prefill": shape, "route": name, "rows": M, "iters": iters, "us": spread(v),
                      "TFLOPs": round(2.0 * M * N * K / (statistics.median(v) * 1e-6) / 1e12, 1)})


def engine_with(kind, group, cap):
    mode = {"mode": "mxfp4" if kind.startswith("mx4") else "mxfp8"} if kind.startswith("mx") else {}
    cfg = dict(bench.SHAPES["mistral-7b"], quantization=dict({"group_size": group, "bits": bits_of(kind)}, **mode))
    eng = Engine(cfg, device=0, max_positions=max(cap, 2048), act_dtype="bfloat16")
    H, I, V, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["hidden_size"] // cfg["num_attention_heads"]
    KV, gen, ones = cfg["num_key_value_heads"] * D, torch.Generator().manual_seed(1), torch.ones(H, dtype=torch.bfloat16)
    mats = [("model.embed_tokens", V, H), ("lm_head", V, H)]
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        mats += [(p + "self_attn.q_proj", H, H), (p + "self_attn.k_proj", KV, H), (p + "self_attn.v_proj", KV, H), (p + "self_attn.o_proj", H, H),
                 (p + "mlp.gate_proj", I, H), (p + "mlp.up_proj", I, H), (p + "mlp.down_proj", H, I)]
        eng.set_tensor(p + "input_layernorm.weight", ones)
        eng.set_tensor(p + "post_attention_layernorm.weight", ones)
    eng.set_tensor("model.norm.weight", ones)
    for name, N, K in mats:
        for suf, t in zip((".weight", ".scales", ".biases"), random_linear(kind, group, N, K, gen)):
            eng.set_tensor(name + suf, t)
    eng.finalize()
    return eng, cfg


def step(args, emit):
    B, K, W, ctx = 8, args.steps, args.warmup, 1024
    cap = ctx + 2 * (K + W) + 136
    a = bench.parse_args(["--gpus", "1", "--steps", str(K), "--warmup", str(W)])
    a.batch, a.no_prefill_timing, a.profile_kernel = B, True, "gemv_gate_up"
    kinds = KINDS8 if args.fp8 else {n: KINDS[n] for n in ("mxfp4", "int4_g32")}
    engines = {name: engine_with(*kg, cap) for name, kg in kinds.items()}
    prompts = np.random.default_rng(23).integers(0, 32000, size=(B, ctx)).astype(np.int32)
    ms, gu = {n: [] for n in engines}, {n: [] for n in engines}
    for _ in range(args.rounds):
        for name, (eng, cfg) in engines.items():
            leg = bench.decode_leg(eng, cfg, a, "model", prompts, SampleArgs(temp=0.0), None, 1, cap, instrument=True)
            n = bench.numbers(cfg, 8 if args.fp8 else 4, B, K, W, ctx, leg, "model", "gemv_gate_up", 1)
            ms[name].append(n["ms_per_step"]); gu[name].append(n["avg_ms"] * 1e3)
    for name in engines:
        emit({"step": name, "ms_per_step": spread(ms[name]), "tokens_per_s": round(B / statistics.median(ms[name]) * 1e3, 1),
              "gate_up_us": spread(gu[name])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--fp8", action="store_true", help="mxfp8 against int8 (kernel mode and --step)")
    ap.add_argument("--iters", type=int, default=None, help="launches per sample (default 200; --prefill: 20)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", default=None, help="default 1,8,64; --prefill: 256,512,1024,2048,4096,8192")
    ap.add_argument("--steps", type=int, default=76)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the results as JSON lines to this file")
    args = ap.parse_args()
    args.iters = args.iters or (20 if args.prefill else 200)
    args.rows = args.rows or ("256,512,1024,2048,4096,8192" if args.prefill else "1,8,64")
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)
    (step if args.step else prefill if args.prefill else kernels)(args, emit)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
