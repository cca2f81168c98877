#!/usr/bin/env python3
"""Outputs of every linear route's epilogue on seeded inputs, for a bit-for-bit comparison of two builds of the library.

    python tools/linear_epilogue_outputs.py --save FILE.npz                  # one build (MLX_PARALLM_AMD_LIB selects another)
    python tools/linear_epilogue_outputs.py --compare A.npz B.npz            # cell count, array count, differing arrays

One fresh process per library.  A cell is one call of an mi_op_* entry point (or one forward pass of an adapted tiny model:
the LoRA term of lora_rows.hip behind every route's plain store, which no mi_op_* reaches); what it wrote is kept as raw bits (16-bit outputs as uint16).  A call that the
library refuses is kept as its error text, so a refusal that changes shows up as a differing array too.

Shapes are the smallest that reach every path: N = 144 output columns (nine tiles: a second tile group with spare waves),
K = 512 (two chunks), intermediate size 144 for the paired forms.  The prefill GEMM's thresholds (launch_gemm_prefill): the
128-row tile below 256 rows, its K split from 16 K tiles (K = 1024; three float32 terms reach it at K = 512), the 256-row tile
with the K split at 256 rows, and without it -- its own epilogues, the residual one included -- from 192 tiles, which at
N = 144 means 49152 rows (24576 for SwiGLU)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from mlx_parallm_amd import _lib as L
from mlx_parallm_amd.quant import quantize

N, K, I = 144, 512, 144
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MIDT = {"f32": L.MI_F32, "bf16": L.MI_BF16, "f16": L.MI_F16}
EPIS = {"store": L.EPI_STORE, "resid": L.EPI_RESID, "swiglu": L.EPI_SWIGLU}
OUT = {}
KEEP = []


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy()


def weight(kind, n, k, seed):
    """tile-major op_linear of `kind` (bf16, f16, q4_bf16, q8_f16, ...) with seeded values"""
    sdt = TDT[kind.split("_")[-1]]
    w = (rand((n, k), seed, 0.05)).to(sdt).cuda()
    ol = L.OpLinear()
    ol.wk, ol.N, ol.K, ol.group = L.WK[kind], n, k, 64
    if kind.startswith("q"):
        packed, scales, biases = quantize(w, 64, int(kind[1]))
        KEEP.extend([packed, scales, biases])
        ol.w, ol.scales, ol.biases = packed.data_ptr(), scales.data_ptr(), biases.data_ptr()
    else:
        KEEP.append(w)
        ol.w = w.data_ptr()
    nbytes = int(L.lib().mi_op_tiled_bytes(C.byref(ol)))
    dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_repack_tiled(C.byref(ol), C.c_void_p(dst.data_ptr())))
    KEEP.append(dst)
    ol.w, ol.scales, ol.biases, ol.layout = dst.data_ptr(), 0, 0, 1
    return ol


def cell(name, call, kind, act, M, epi, *, bias=False, rnd=0, norm=False, k=K, generic=0, seed=0):
    """one launch: call(ol, args) -> rc; keeps the array the epilogue wrote"""
    sw = epi == "swiglu"
    n_w, n_out = (2 * I, I) if sw else (N, N)
    ol = weight(kind, n_w, k, 1000 + seed)
    if bias:
        b = rand((n_w,), 2000 + seed, 0.5).to(torch.bfloat16 if act == "f32" else TDT[act]).to(torch.float32).cuda()
        KEEP.append(b)
        ol.bias = b.data_ptr()
    x = rand((M, k), 3000 + seed).to(TDT[act]).cuda()
    nw = (1.0 + rand((k,), 4000 + seed, 0.1)).to(TDT[act]).cuda()
    out = (rand((M, n_out), 5000 + seed)).to(TDT[act]).cuda()        # the residual stream of EPI_RESID; overwritten otherwise
    a = L.OpGemvArgs()
    a.x, a.ldx, a.M, a.act, a.rnd = x.data_ptr(), k, M, MIDT[act], rnd
    a.pro, a.norm_w, a.eps = (L.PRO_NORM if norm else L.PRO_NONE), (nw.data_ptr() if norm else 0), 1e-5
    a.epi, a.ldo, a.out, a.resid = EPIS[epi], n_out, out.data_ptr(), out.data_ptr()
    a.pair_offset, a.force_generic = (I if sw else 0), generic
    torch.cuda.synchronize()
    rc = call(ol, a)
    torch.cuda.synchronize()
    key = f"{name}|{kind}|{act}|M{M}|{epi}|bias{int(bias)}|rnd{rnd}|norm{int(norm)}|K{k}"
    assert key not in OUT, key
    if rc != 0:
        OUT[key] = np.frombuffer(L.lib().mi_last_error()[:200], dtype=np.uint8).copy()
    else:
        OUT[key] = bits(out)
    del KEEP[:]


def op(fn, *extra):
    return lambda ol, a: getattr(L.lib(), fn)(C.byref(ol), C.byref(a), *extra)


def skinny(ksplit):
    return lambda ol, a: L.lib().mi_op_gemm_skinny(C.byref(ol), C.byref(a), ksplit, None, 0, None)


def kernel_cells(big):
    for epi in EPIS:
        for bias in (False, True):
            # mi_op_gemv: matrix-core and forced generic at 4 rows
            for act in ("bf16", "f16"):
                for kind in (act, f"q4_{act}"):
                    cell("gemv_mfma", op("mi_op_gemv"), kind, act, 4, epi, bias=bias)
                for kind in (act, f"q4_{act}", f"q8_{act}"):
                    cell("gemv_generic", op("mi_op_gemv"), kind, act, 4, epi, bias=bias, generic=1)
            for rnd in (0, L.RND_BF16):
                cell("gemv_generic", op("mi_op_gemv"), "bf16", "f32", 4, epi, bias=bias, rnd=rnd, generic=1)
            # mi_op_gemm_skinny, forced ksplit 1 and 2
            for ks in (1, 2):
                for act in ("bf16", "f16"):
                    for M in (12, 24):
                        cell(f"skinny_ks{ks}", skinny(ks), act, act, M, epi, bias=bias)
                    for q in ("q4", "q8"):
                        for M in (4, 24):
                            cell(f"skinny_ks{ks}", skinny(ks), f"{q}_{act}", act, M, epi, bias=bias)
                for kind in ("bf16", "q4_bf16", "q8_bf16"):
                    for M in (4, 24):
                        for rnd, norm in ((0, False), (0, True), (L.RND_BF16, False)):
                            cell(f"skinny_ks{ks}", skinny(ks), kind, "f32", M, epi, bias=bias, rnd=rnd, norm=norm)
            # the tile GEMM: 128-row tile (K = 512 whole, K = 1024 split), 256-row tile with the K split
            for act in ("bf16", "f16"):
                for kind in (act, f"q4_{act}"):
                    for M, k in ((40, 512), (40, 1024), (256, 1024)):
                        cell("prefill", op("mi_op_gemm_prefill", 0, None), kind, act, M, epi, bias=bias, k=k)
            for kind in ("bf16", "q4_bf16"):
                for M in (40, 256):
                    for norm in (False, True):
                        cell("prefill_f32", op("mi_op_gemm_prefill_f32", 3, 0, None), kind, "f32", M, epi, bias=bias, norm=norm)
            if big:      # the 256-row tile without the K split: its own epilogues (LDS-DMA form and, MI_GEMM_DMA=0, the register-staged one)
                M = 24576 if epi == "swiglu" else 49152
                cell("prefill256", op("mi_op_gemm_prefill", 0, None), "bf16", "bf16", M, epi, bias=bias)
                cell("prefill256_f32", op("mi_op_gemm_prefill_f32", 3, 0, None), "bf16", "f32", M, epi, bias=bias)
                os.environ["MI_GEMM_DMA"] = "0"
                cell("prefill256_nodma", op("mi_op_gemm_prefill", 0, None), "f16", "f16", M, epi, bias=bias)
                del os.environ["MI_GEMM_DMA"]
            # gemv_f32.hip's three forms
            for fn in ("mi_op_gemv_f32", "mi_op_gemv_f32_whole", "mi_op_gemv_f32_resident"):
                for norm in (False, True):
                    cell(fn[6:], op(fn, 0, None), "bf16", "f32", 4, epi, bias=bias, norm=norm)
        # no bias on these routes (refused): the row-interleaved gate|up copy, gemm_q4.hip under a forced plan at 40 rows
        for act in ("bf16", "f16"):
            for ks in (1, 2):
                cell(f"gemm_q4_ks{ks}", skinny(-(ks << 11)), f"q4_{act}", act, 40, epi)
    for act in ("bf16", "f16"):
        cell("gemv_gu8", op("mi_op_gemv_gu8"), act, act, 4, "swiglu")
    cell("skinny_slabs", skinny(0), "q4_bf16", "bf16", 72, "swiglu")
    cell("skinny_slabs", skinny(0), "q4_bf16", "bf16", 72, "swiglu", bias=True)
    # mi_op_swiglu_rows
    for act, rnds in (("f32", (0, L.RND_BF16, L.RND_F16)), ("bf16", (0,)), ("f16", (0,))):
        for rnd in rnds:
            x = rand((5, 2 * I), 7, 3.0).to(TDT[act]).cuda()
            out = torch.zeros((5, I), dtype=TDT[act], device="cuda")
            torch.cuda.synchronize()
            L.check(L.lib().mi_op_swiglu_rows(x.data_ptr(), 2 * I, out.data_ptr(), I, 5, I, MIDT[act], rnd))
            torch.cuda.synchronize()
            OUT[f"swiglu_rows|{act}|rnd{rnd}"] = bits(out)


# ---- the LoRA term (lora_rows.hip: down by row, the route's plain store, up-add by row), through the engine: the tiny models
# of tests/test_gpu_lora_targets.py under the engine-wide adapter (rank 16, scale 10, all seven projections of the last two
# blocks)
KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
        "mlp.down_proj")
TINY = {
    "llama_q4_bf16": dict(seed=3, vocab_size=512, dtype="bfloat16", quantize_model=True, hidden_size=128, layers=2, heads=8,
                          kv_heads=2, intermediate_size=256, head_dim=16, tie_word_embeddings=False, norm_jitter=0.1),
    "qwen3_bf16": dict(seed=4, model_type="qwen3", vocab_size=512, dtype="bfloat16", quantize_model=False, hidden_size=128,
                       layers=2, heads=5, kv_heads=1, intermediate_size=256, head_dim=64, tie_word_embeddings=False,
                       norm_jitter=0.1),
}


def write_adapter(dst, cfg):
    from safetensors.torch import save_file

    H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    nkv = cfg.get("num_key_value_heads") or nh
    D, inter = cfg.get("head_dim") or H // nh, cfg["intermediate_size"]
    dims = dict(zip(KEYS, ((H, nh * D), (H, nkv * D), (H, nkv * D), (nh * D, H), (H, inter), (H, inter), (inter, H))))
    w, nl = {}, cfg["num_hidden_layers"]
    for i in range(nl - 2, nl):
        for ki, key in enumerate(KEYS):
            k, n = dims[key]
            rng = np.random.default_rng([5, i, ki])
            w[f"model.layers.{i}.{key}.lora_a"] = torch.from_numpy((rng.uniform(-1, 1, (k, 16)) / np.sqrt(k)).astype(np.float32))
            w[f"model.layers.{i}.{key}.lora_b"] = torch.from_numpy((rng.standard_normal((16, n)) * 0.05).astype(np.float32))
    dst.mkdir(parents=True, exist_ok=True)
    save_file(w, str(dst / "adapters.safetensors"))
    (dst / "adapter_config.json").write_text(json.dumps({
        "fine_tune_type": "lora", "num_layers": 2,
        "lora_parameters": {"rank": 16, "scale": 10.0, "dropout": 0.0, "keys": list(KEYS)}}))


def engine_cells():
    from mlx_parallm_amd import utils
    from mlx_parallm_amd.tiny_model import build_tiny_model

    with tempfile.TemporaryDirectory() as tmp:
        for name, kw in TINY.items():
            d = Path(tmp) / name
            cfg = build_tiny_model(d, **kw)
            write_adapter(d / "adapter", cfg)
            model = utils.load_model(str(d), max_positions=256)
            utils.load_adapters(model, str(d / "adapter"))
            for kvd in ("float32", "model"):
                for what, B, L0 in (("decode", 4, 3), ("decode", 12, 3), ("decode", 40, 3), ("prefill", 3, 60)):
                    rng = np.random.default_rng([9, B, L0])
                    toks = rng.integers(3, cfg["vocab_size"], size=(B, L0)).astype(np.int32)
                    kv = model.engine.new_kv(B, capacity=L0 + 4, kv_dtype=kvd)
                    got = [model.engine.forward(toks, kv, all_positions=(what == "prefill"))]
                    for step in range(2 if what == "decode" else 0):
                        got.append(model.engine.forward(np.argmax(got[-1], axis=-1)[:, None].astype(np.int32), kv))
                    kv.close()
                    for i, g in enumerate(got):
                        OUT[f"engine|{name}|kv_{kvd}|{what}|B{B}|pass{i}"] = np.asarray(g, dtype=np.float32)
            model.engine.close()


def same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8) if a.dtype != np.uint8 else a, b.view(np.uint8) if b.dtype != np.uint8 else b)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    diff = [n for n in names if n not in a.files or n not in b.files or not same(a[n], b[n])]
    refused = [n for n in a.files if a[n].dtype == np.uint8]
    cells = len({n.rsplit("|pass", 1)[0] for n in names})
    values = sum(int(a[n].size) for n in a.files if a[n].dtype != np.uint8)
    nonfinite = sum(int((~np.isfinite(a[n].astype(np.float32))).sum()) for n in a.files if a[n].dtype == np.float32)
    print(f"{cells} cells, {len(names)} arrays, {values} values ({nonfinite} non-finite float32), "
          f"{len(refused)} refused calls: differing arrays: {len(diff)}")
    for n in refused:
        print(f"  refused  {n}: {bytes(a[n]).decode('utf-8', 'replace')}")
    for n in diff:
        print(f"  DIFFERS  {n}")
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", help="write every cell's outputs to this .npz")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    ap.add_argument("--no-big", action="store_true", help="skip the 49152-row cells of the prefill GEMM")
    ap.add_argument("--no-engine", action="store_true", help="skip the adapted tiny models")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    kernel_cells(not a.no_big)
    if not a.no_engine:
        engine_cells()
    print(f"{len(OUT)} arrays from {L.LIB_PATH}")
    if a.save:
        Path(a.save).parent.mkdir(parents=True, exist_ok=True)
        np.savez(a.save, **OUT)


if __name__ == "__main__":
    main()
