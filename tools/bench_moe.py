#!/usr/bin/env python3
"""One Mixtral MoE block at the 8x7B shape (H 4096, I 14336, E 8, k 2), launch by launch (mi_op_moe_route / mi_op_moe_mlp):
1, 8 and 32 decode rows and 1024 prefill rows under uniform random routing, in both activation modes (bf16, and float32 = the
float32-KV mode).  Prints us per launch and the bytes of DISTINCT expert weights a launch touches per us; beside them what the
dense gate|up and down launches of a Mistral-7B block reach per byte in the same job (the yardstick: the same H and I, one
matrix instead of eight).  Launches of one call repeat back to back on the same data: whatever fits the 256 MiB Infinity Cache
(the two experts of a 1-row call, a dense matrix) is partly served from it, on both sides of the comparison."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from mlx_parallm_amd import _lib as L

DEV = "cuda"
TDT = {"bfloat16": torch.bfloat16, "float32": torch.float32}
MIDT = {"bfloat16": L.MI_BF16, "float32": L.MI_F32}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def moe_case(w, act, R, H, I, E, k, iters, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    xn = torch.randn((R, H), device=DEV, generator=g).to(TDT[act])
    sel = torch.zeros((R, k), dtype=torch.int32, device=DEV)
    score = torch.zeros((R, k), dtype=TDT[act], device=DEV)
    meta = torch.zeros(2 * E, dtype=torch.int32, device=DEV)
    lst = torch.zeros(R * k, dtype=torch.int32, device=DEV)
    out = torch.zeros((R, H), dtype=TDT[act], device=DEV)
    torch.cuda.synchronize()
    ms = C.c_float(0)
    L.check(L.lib().mi_op_moe_route(_p(xn), H, R, H, MIDT[act], 0, _p(w["router"]), L.MI_BF16, E, k, _p(sel), _p(score), _p(meta),
                                    _p(lst), iters, C.byref(ms)))
    stage = (C.c_float * 3)()
    L.check(L.lib().mi_op_moe_mlp(_p(xn), H, R, H, I, MIDT[act], 0, L.MI_BF16, E, k, _p(w["gate"]), _p(w["up"]), _p(w["down"]), _p(meta),
                                  _p(lst), _p(score), None, H, _p(out), H, iters, stage))
    cnt = meta[:E].cpu().tolist()
    touched = sum(1 for c in cnt if c > 0)
    one = I * H * 2                                          # bytes of one expert's matrix
    us = {"route": ms.value * 1e3, "gate_up": stage[0] * 1e3, "down": stage[1] * 1e3, "combine": stage[2] * 1e3}
    return {"act": act, "rows": R, "experts_touched": touched, "pairs_per_expert": cnt, "us": us,
            "gate_up_bytes_per_us": 2 * touched * one / us["gate_up"], "down_bytes_per_us": touched * one / us["down"]}


def dense_case(act, R, H, I, iters):
    """The dense gate|up (SwiGLU) and down launches on R rows: the decode GEMV (<= 16 rows of 16-bit activations), the one-pass
    float32 GEMV (<= 8 float32 rows), the split-K streaming GEMM above."""
    res = {"act": act, "rows": R}
    for name, N, K, epi in (("gate_up", 2 * I, H, L.EPI_SWIGLU), ("down", H, I, L.EPI_STORE)):
        wt = (torch.randn((N, K), device=DEV) * 0.02).to(torch.bfloat16)
        ol = L.OpLinear()
        ol.wk, ol.N, ol.K, ol.group, ol.w = L.WK["bf16"], N, K, 64, wt.data_ptr()
        dst = torch.zeros(int(L.lib().mi_op_tiled_bytes(C.byref(ol))), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        L.check(L.lib().mi_op_repack_tiled(C.byref(ol), _p(dst)))
        ol.w, ol.layout = dst.data_ptr(), 1
        x = torch.randn((R, K), device=DEV).to(TDT[act])
        n_out = N // 2 if epi == L.EPI_SWIGLU else N
        out = torch.zeros((R, n_out), dtype=TDT[act], device=DEV)
        a = L.OpGemvArgs()
        a.x, a.ldx, a.M, a.act, a.rnd, a.pro, a.epi = x.data_ptr(), K, R, MIDT[act], 0, L.PRO_NONE, epi
        a.ldo, a.out, a.pair_offset = n_out, out.data_ptr(), (N // 2 if epi == L.EPI_SWIGLU else 0)
        torch.cuda.synchronize()
        ms, used = C.c_float(0), C.c_int(0)
        if act == "float32" and R <= 8:
            L.check(L.lib().mi_op_gemv_f32(C.byref(ol), C.byref(a), iters, C.byref(ms)))
        elif act != "float32" and R <= 16:
            L.check(L.lib().mi_op_gemv_bench(C.byref(ol), C.byref(a), iters, C.byref(ms)))
        else:
            L.check(L.lib().mi_op_gemm_skinny(C.byref(ol), C.byref(a), 0, C.byref(used), iters, C.byref(ms)))
        res[name + "_us"] = ms.value * 1e3
        res[name + "_bytes_per_us"] = N * K * 2 / (ms.value * 1e3)
        del wt, dst
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,32,1024")
    ap.add_argument("--acts", default="bfloat16,float32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--intermediate", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--per-tok", type=int, default=2)
    ap.add_argument("--dense", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the results as JSON lines to this file")
    args = ap.parse_args()
    H, I, E, k = args.hidden, args.intermediate, args.experts, args.per_tok
    w = {"router": (torch.randn((E, H), device=DEV) * 0.02).to(torch.bfloat16)}       # small logits: near-uniform random routing
    for name, shape in (("gate", (E, I, H)), ("up", (E, I, H)), ("down", (E, H, I))):
        w[name] = (torch.randn(shape, device=DEV, dtype=torch.bfloat16) * 0.02)
    lines = []
    for act in args.acts.split(","):
        for R in (int(r) for r in args.rows.split(",")):
            r = moe_case(w, act, R, H, I, E, k, args.iters if R <= 64 else max(2, args.iters // 4), seed=R)
            lines.append({"moe": r})
            u = r["us"]
            print(f"moe   {act:8s} rows {R:5d}  experts touched {r['experts_touched']}  route {u['route']:8.1f}  gate|up {u['gate_up']:9.1f}  "
                  f"down {u['down']:9.1f}  combine {u['combine']:7.1f} us   gate|up {r['gate_up_bytes_per_us'] / 1e6:6.2f}  down "
                  f"{r['down_bytes_per_us'] / 1e6:6.2f} TB/s of distinct expert weights", flush=True)
    if args.dense:
        for act in args.acts.split(","):
            for R in (int(r) for r in args.rows.split(",") if int(r) <= 64):
                try:
                    r = dense_case(act, R, H, I, args.iters)
                except Exception as ex:                                    # (a route that refuses the shape: say so, go on)
                    print(f"dense {act:8s} rows {R:5d}  not measured: {ex}", flush=True)
                    continue
                lines.append({"dense": r})
                print(f"dense {act:8s} rows {R:5d}  gate|up {r['gate_up_us']:9.1f}  down {r['down_us']:9.1f} us   gate|up "
                      f"{r['gate_up_bytes_per_us'] / 1e6:6.2f}  down {r['down_bytes_per_us'] / 1e6:6.2f} TB/s", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
