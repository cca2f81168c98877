#!/usr/bin/env python3
"""head_dim 96 (Phi-3-mini) against head_dim 128, the yardstick: attention launches and end-to-end decode.

* decode attention (mi_op_attention_decode, matrix-core variant): B = 8, 32 query / 32 KV heads, 1024 keys, bf16 and float32
  caches, at D = 96 and D = 128.  Timed by the library with HIP events around `--iters` back-to-back launches behind a
  warm-up one; rotates over `--layers` K/V buffers so that re-reads are not served by the Infinity Cache; the two widths
  alternate inside every repeat, and the spread of the repeats is printed next to the median.  The split count is the one
  the engine's choose_nsplit would take for a (8, 32)-workgroup launch, 1, and 2 / 4 for comparison.
* prefill attention (mi_op_attention, L = 1024 new tokens on empty caches) likewise, with device events around the calls.
* --model: tokens/s of decode steps of a Phi-3-mini-shaped model (32 blocks, int4 g64, random weights) at B = 8 from KV 1024,
  in both KV modes: host clock around `--steps` steps, each ending in a device synchronise, behind `--warmup` untimed ones.

    python tools/head96_timing.py [--model] [--out bench_out/head96_timing.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from mlx_parallm_amd import _lib as L  # noqa: E402

B, H, S = 8, 32, 1024
DT = {"bfloat16": (torch.bfloat16, L.MI_BF16), "float32": (torch.float32, L.MI_F32)}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _shape(L_, D, mi_dt, cap):
    sh = L.OpAttnShape()
    sh.B, sh.L, sh.Hq, sh.Hkv, sh.D, sh.act, sh.kv, sh.rnd, sh.cap = B, L_, H, H, D, mi_dt, mi_dt, 0, cap
    return sh


class Decode:
    def __init__(self, D, kv, layers):
        dt, mi_dt = DT[kv]
        cap = S + 64
        self.D, self.layers = D, layers
        self.kcs = [torch.randn((B, H, cap, D), device="cuda", dtype=torch.float32).to(dt) for _ in range(layers)]
        self.vcs = [torch.randn((B, H, cap, D), device="cuda", dtype=torch.float32).to(dt) for _ in range(layers)]
        self.qkv = torch.randn((B, 3 * H * D), device="cuda", dtype=torch.float32).to(dt)
        self.out = torch.zeros((B, H * D), device="cuda", dtype=dt)
        self.offs = torch.full((B,), S, device="cuda", dtype=torch.int32)
        self.cos = torch.zeros((cap + 1, D // 2), device="cuda", dtype=torch.float32)
        self.sin = torch.zeros_like(self.cos)
        torch.cuda.synchronize()
        L.check(L.lib().mi_op_rope_tables(_p(self.cos), _p(self.sin), cap + 1, D, 1e4, 1.0))
        self.sh = _shape(1, D, mi_dt, cap)
        self.bytes = 2 * B * H * S * D * self.kcs[0].element_size()

    def run(self, nsplit, iters):
        """-> mean microseconds of one launch (HIP events around `iters` launches per buffer, averaged over the buffers)."""
        part = torch.zeros((B * H * nsplit * (self.D + 2),), device="cuda", dtype=torch.float32)
        ctr = torch.zeros((B * H,), device="cuda", dtype=torch.int32)
        torch.cuda.synchronize()
        tot = 0.0
        for i in range(self.layers):
            ms = C.c_float(0)
            L.check(L.lib().mi_op_attention_decode(
                C.byref(self.sh), _p(self.qkv), _p(self.kcs[i]), _p(self.vcs[i]), _p(self.offs), None, None, 1e-6, _p(self.cos),
                _p(self.sin), _p(self.out), float(self.D ** -0.5), 0, nsplit, _p(part), _p(ctr), 0, iters, C.byref(ms)))
            tot += ms.value
        return tot / self.layers * 1e3


class Prefill:
    def __init__(self, D, kv):
        dt, mi_dt = DT[kv]
        self.D = D
        self.kc = torch.randn((B, H, S, D), device="cuda", dtype=torch.float32).to(dt)
        self.vc = torch.randn((B, H, S, D), device="cuda", dtype=torch.float32).to(dt)
        self.q = torch.randn((B * S, H * D), device="cuda", dtype=torch.float32).to(dt)
        self.out = torch.zeros_like(self.q)
        self.offs = torch.zeros((B,), device="cuda", dtype=torch.int32)
        self.sh = _shape(S, D, mi_dt, S)
        self.flops = 2.0 * 2.0 * B * H * D * S * (S + 1) / 2          # causal: q.k and p.v over S (S + 1) / 2 pairs

    def call(self):
        L.check(L.lib().mi_op_attention(C.byref(self.sh), _p(self.q), _p(self.kc), _p(self.vc), _p(self.offs), _p(self.out),
                                        float(self.D ** -0.5), 1, None))

    def run(self, iters):
        self.call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            self.call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3


def _summary(xs):
    return dict(median_us=round(statistics.median(xs), 2), min_us=round(min(xs), 2), max_us=round(max(xs), 2), repeats=len(xs))


def attention(a):
    rows = []
    for kv in ("bfloat16", "float32"):
        dec = {D: Decode(D, kv, a.layers) for D in (128, 96)}
        for ns in a.splits:
            t = {D: [] for D in dec}
            for _ in range(a.repeats):
                for D in (128, 96):                      # alternating inside a repeat
                    t[D].append(dec[D].run(ns, a.iters))
            for D in (128, 96):
                r = dict(kind="decode", kv=kv, D=D, nsplit=ns, **_summary(t[D]))
                r["GBps"] = round(dec[D].bytes / r["median_us"] / 1e3, 1)
                rows.append(r)
                print(json.dumps(r), flush=True)
        del dec
        torch.cuda.empty_cache()
        pre = {D: Prefill(D, kv) for D in (128, 96)}
        t = {D: [] for D in pre}
        for _ in range(a.repeats):
            for D in (128, 96):
                t[D].append(pre[D].run(max(4, a.iters // 4)))
        for D in (128, 96):
            r = dict(kind="prefill", kv=kv, D=D, **_summary(t[D]))
            r["TFLOPs"] = round(pre[D].flops / r["median_us"] / 1e6, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
        del pre
        torch.cuda.empty_cache()
    return rows


PHI3_MINI = dict(model_type="phi3", hidden_size=3072, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32,
                 intermediate_size=8192, vocab_size=32064, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=4096,
                 quantization={"group_size": 64, "bits": 4})


def model(a):
    """Random N(0, 0.02^2) weights, MLX-affine int4 g64, handed to a Phi-3 engine under the fused names."""
    import numpy as np

    from mlx_parallm_amd.engine import Engine, SampleArgs
    from mlx_parallm_amd.quant import quantize

    cfg = dict(PHI3_MINI)
    Hd, I, V, NL = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_hidden_layers"]
    eng = Engine(cfg, device=0, max_positions=2048, act_dtype="bfloat16")
    gen = torch.Generator(device="cuda").manual_seed(7)

    def mat(name, n, k):
        w = (torch.randn((n, k), generator=gen, device="cuda", dtype=torch.float32) * 0.02).to(torch.bfloat16)
        packed, scales, biases = quantize(w, 64, 4)
        for suf, t in ((".weight", packed), (".scales", scales), (".biases", biases)):
            eng.set_tensor(name + suf, t)

    ones = torch.ones((Hd,), device="cuda", dtype=torch.bfloat16)
    mat("model.embed_tokens", V, Hd)
    for i in range(NL):
        p = f"model.layers.{i}."
        mat(p + "self_attn.qkv_proj", 3 * Hd, Hd)
        mat(p + "self_attn.o_proj", Hd, Hd)
        mat(p + "mlp.gate_up_proj", 2 * I, Hd)
        mat(p + "mlp.down_proj", Hd, I)
        eng.set_tensor(p + "input_layernorm.weight", ones)
        eng.set_tensor(p + "post_attention_layernorm.weight", ones)
    eng.set_tensor("model.norm.weight", ones)
    mat("lm_head", V, Hd)
    eng.finalize()
    rows = []
    prompts = np.random.default_rng(3).integers(3, V, size=(B, S)).astype(np.int32)
    for kvd in ("model", "float32"):
        kv = eng.new_kv(B, capacity=S + a.warmup + a.steps * a.repeats + 8, kv_dtype=kvd)
        y = eng.decode_sample(kv, prompts, SampleArgs(temp=0.0))["tokens"][:, None].astype(np.int32)
        for _ in range(a.warmup):
            y = eng.decode_sample(kv, y, SampleArgs(temp=0.0))["tokens"][:, None].astype(np.int32)
        rates = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                y = eng.decode_sample(kv, y, SampleArgs(temp=0.0))["tokens"][:, None].astype(np.int32)
            eng.sync()
            rates.append(B * a.steps / (time.perf_counter() - t0))
        r = dict(kind="phi3-mini int4 decode", kv=kvd, batch=B, context=S, steps=a.steps, tokens_per_s=round(statistics.median(rates), 1),
                 min=round(min(rates), 1), max=round(max(rates), 1), repeats=len(rates))
        rows.append(r)
        print(json.dumps(r), flush=True)
        kv.close()
    eng.close()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8, help="K/V buffers a decode timing rotates over")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--splits", type=lambda s: [int(x) for x in s.split(",")], default=[1, 2, 4])
    ap.add_argument("--model", action="store_true", help="also the end-to-end decode of the Phi-3-mini-shaped model")
    ap.add_argument("--model-only", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("head96_timing: no GPU (there is nothing to time without one)")
    rows = [] if a.model_only else attention(a)
    if a.model or a.model_only:
        rows += model(a)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
