#!/usr/bin/env python3
"""Where the time of a gemm_skinny launch goes (debug build only).

Build the library with -DMI_SK_TRACE (tools/debug/build_trace_lib.sh), then on a GPU box:

    MLX_PARALLM_AMD_LIB=$PWD/mlx_parallm_amd/csrc/alt/libmi355_trace.so \
        python tools/debug/skinny_trace.py --workload mistral-7b-int4 [--kv float32]

Runs bench.py's decode leg (4 timed steps), dumps the per-workgroup wall-clock stamps (100 MHz s_memrealtime) of the
last launches and prints, per linear of the decode step, the average of:
  ramp    first workgroup's entry -> last workgroup's entry
  stage_norm / w0..w7 / stage   entry -> row statistics known / wave w has written its share of the first activation
          chunk / the chunk is complete (barrier)
  stream  the K slice (weights streamed, MFMA)
  publish partial tile stored write-through + drained
  count   arrival counter
  combine (last arriver) the ksplit partials read back and added
  epi     (last arriver) epilogue
  total   first entry -> last exit; `to next` = last exit -> first entry of the NEXT skinny launch (whatever runs between)
"""
import argparse
import ctypes as C
import struct
import sys
from collections import OrderedDict, defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

TICK_US = 0.01          # s_memrealtime: 100 MHz


def read_dump(path):
    recs = []
    with open(path, "rb") as f:
        (n,) = struct.unpack("l", f.read(8))
        for _ in range(n):
            hdr = struct.unpack("12i", f.read(48))
            grid = hdr[4]
            import numpy as np

            st = np.frombuffer(f.read(grid * 128), dtype=np.uint64).reshape(grid, 16).astype(np.int64)
            recs.append((hdr, st))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral-7b-int4")
    ap.add_argument("--kv", default="model")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default="gpurun_out/skinny_trace.bin")
    ap.add_argument("--opt", action="append", default=[], help="engine option key=value, passed on to bench.py")
    ap.add_argument("--attention-side", action="store_true",
                    help="float32-KV step: one row per distinct stamped launch (q|k|v, decode attention, o, down), attention stamps included")
    args = ap.parse_args()

    import bench

    argv = ["--workload", args.workload, "--full", "--no-cpu-baseline", "--steps", str(args.steps), "--warmup", "2", "--batch", str(args.batch),
            "--no-prefill-timing"]
    argv += ["--kv-dtype", args.kv, "--no-second-leg", "--no-other-configs"] if args.attention_side else ["--no-second-leg"] if args.kv == "model" else []
    for o in args.opt:
        argv += ["--opt", o]
    sys.argv = ["bench.py"] + argv
    bench.main()
    from mlx_parallm_amd import _lib as L

    lib = C.CDLL(str(L.LIB_PATH))
    if not hasattr(lib, "mi_debug_sk_trace_dump"):
        raise SystemExit("this build has no trace (compile gemm_skinny.hip with -DMI_SK_TRACE)")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    rc = lib.mi_debug_sk_trace_dump(str(args.out).encode())
    if rc:
        raise SystemExit(f"dump failed: {rc}")
    if args.attention_side:
        report_attention_side(args.out, args.steps)
    else:
        report(args.out, args.steps)


def report_attention_side(path, steps):
    """The float32-KV decode step as the stamps see it: gate|up and lm_head run on gemv_f32.hip (no stamps), so a layer is
    q|k|v -> decode attention -> o -> down.  One row per distinct launch signature over the last `steps` steps, in the order
    of first appearance.  Linears: stage = entry -> first chunk staged, stream = the K slice, tail = last MFMA -> the
    workgroup's last stamp (publish-only: its stores; otherwise publish / count and, for the last arriver, combine + epilogue).
    Attention (kind -2; -3 = it adds the q|k|v slices): landed = entry -> every prologue load has arrived (16-bit caches: the
    first round's K / V are in front of them; float32: behind them, still in flight), prologue = -> the barrier behind norm /
    RoPE / append, rounds = -> last MFMA, store = -> the
    partial (or the output) is stored, tail = -> end (ticket, and for the last arriver the combine).  A second table gives each
    attention launch's stamps, one per round of a float32 cache included, for the median workgroup and for the one that
    ends last.  All in us, means over workgroups and launches; total = first entry -> last end of the launch; to_next = -> first entry of the next stamped launch."""
    import numpy as np

    recs = read_dump(path)
    sig = lambda h: (h[7], h[1], h[2], h[3], h[4], h[5], h[8], h[11], h[6])   # kind, N, K, ksplit, grid, epi, pro, cc form, M
    lin = lambda h: (h[7], h[1], h[3], h[4], h[5], h[8], h[11], h[6])          # attention: without K (the context grows per step)
    key_of = lambda h: lin(h) if h[7] in (-2, -3) else sig(h)
    last = key_of(recs[-1][0])
    ends = [i for i, (h, _) in enumerate(recs) if key_of(h) == last]
    per = ends[-1] - ends[-2]                                  # stamped launches per layer
    layers = 0
    for i in range(len(ends) - 1, 0, -1):                     # layers per step: the run of equal distances from the end
        if ends[i] - ends[i - 1] != per:
            break
        layers += 1
    layers += 1
    n = min(len(recs), steps * layers * per)
    sel = recs[len(recs) - n:]
    print(f"{len(recs)} launches in the dump; {per} stamped launches per layer, ~{layers} layers per step; analysing the last {n}")
    acc, order = defaultdict(lambda: defaultdict(list)), []
    for j, (h, st) in enumerate(sel):
        k = key_of(h)
        if k not in acc:
            order.append(k)
        a = acc[k]
        s0 = st[:, 0].min()
        if h[7] in (-2, -3):
            a["landed"].append(np.mean(st[:, 1] - st[:, 0]) * TICK_US)
            a["prologue"].append(np.mean(st[:, 2] - st[:, 1]) * TICK_US)
            a["rounds"].append(np.mean(st[:, 3] - st[:, 2]) * TICK_US)
            a["store"].append(np.mean(st[:, 4] - st[:, 3]) * TICK_US)
            a["tail"].append(np.mean(st[:, 5] - st[:, 4]) * TICK_US)
            end = st[:, 5].max()
            # the workgroup's own timeline, from its entry: median workgroup and the one that ends last.  Round stamps
            # (6 + r, float32 caches) are wave 0's; a slot the launch did not write holds an older launch's stamp.
            # issued (slot 15) = the first round's K / V and the prologue's loads are all in the queue: the cache row and
            # the KV length are known and every address is computed.
            rel = (st - st[:, :1]) * TICK_US
            lastwg = int(np.argmax(st[:, 5]))
            pts = [("issued", 15), ("landed", 1), ("barrier", 2)] + [(f"round{r}", 6 + r) for r in range(9)] + [("last_mfma", 3), ("stored", 4), ("end", 5)]
            for name, col in pts:
                okm = (st[:, col] >= st[:, 0]) & (st[:, col] <= st[:, 5])
                if col >= 6 and okm.sum() * 2 < len(okm):                  # a round that fewer than half of the workgroups reach
                    if okm[lastwg]:
                        a["tl_last_" + name].append(rel[lastwg, col])
                    continue
                a["tl_med_" + name].append(float(np.median(rel[okm, col])))
                if okm[lastwg]:
                    a["tl_last_" + name].append(rel[lastwg, col])
            a["tl_last_entry"].append((st[lastwg, 0] - s0) * TICK_US)
            a["tl_med_entry"].append(float(np.median(st[:, 0] - s0)) * TICK_US)
        else:
            a["stage"].append(np.mean(st[:, 2] - st[:, 0]) * TICK_US)
            a["stream"].append(np.mean(st[:, 3] - st[:, 2]) * TICK_US)
            if h[11] == 1:                                     # publish-only: stamp 4 is the workgroup's end
                wg_end = st[:, 4]
            elif h[3] > 1:                                     # split K: everyone reaches 5, the last arriver 6 and 7
                lastm = (st[:, 7] >= st[:, 5]) & (st[:, 5] >= s0)
                wg_end = np.where(lastm, st[:, 7], st[:, 5])
            else:
                wg_end = st[:, 7]
            a["tail"].append(np.mean(wg_end - st[:, 3]) * TICK_US)
            a["last_tail"].append((wg_end.max() - st[:, 3].max()) * TICK_US)
            end = wg_end.max()
        a["ramp"].append((st[:, 0].max() - s0) * TICK_US)
        a["total"].append((end - s0) * TICK_US)
        if j + 1 < len(sel):
            a["to_next"].append((sel[j + 1][1][:, 0].min() - end) * TICK_US)
    f = lambda a, c: f"{np.mean(a[c]):>9.2f}" if a[c] else f"{'-':>9}"
    cols = ["ramp", "stage", "stream", "tail", "last_tail", "landed", "prologue", "rounds", "store", "total", "to_next"]
    print(f"{'kind':>5}{'N':>7}{'K':>7}{'split':>6}{'grid':>6}{'pro':>4}{'cc':>3}{'M':>3}{'count':>7} " + " ".join(f"{c:>9}" for c in cols))
    for k in order:
        a = acc[k]
        if k[0] in (-2, -3):
            kind, N, ks, grid, epi, pro, cc, M = k
            K = "-"
            ks = epi
        else:
            kind, N, K, ks, grid, epi, pro, cc, M = k
        print(f"{kind:>5}{N:>7}{K:>7}{ks:>6}{grid:>6}{pro:>4}{cc:>3}{M:>3}{len(a['total']):>7} " + " ".join(f(a, c) for c in cols))
    for k in order:
        if k[0] not in (-2, -3):
            continue
        a = acc[k]
        names = ["entry", "issued", "landed", "barrier"] + [f"round{r}" for r in range(9)] + ["last_mfma", "stored", "end"]
        names = [n for n in names if a["tl_med_" + n] or a["tl_last_" + n]]
        print(f"attention kind {k[0]}, {k[4]} splits, grid {k[3]}: a workgroup's stamps in us from its own entry (entry: from the launch's first entry)")
        print(f"{'':>10} " + " ".join(f"{n:>9}" for n in names))
        print(f"{'median wg':>10} " + " ".join(f(a, "tl_med_" + n) for n in names))
        print(f"{'last wg':>10} " + " ".join(f(a, "tl_last_" + n) for n in names))


def report(path, steps):
    import numpy as np

    recs = read_dump(path)
    # launches of one decode step: signature sequence repeats; take the steps of the TIMED region = the `steps` steps in front of
    # the last `steps` (instrumented) ones of the last leg
    sig = lambda h: (h[1], h[2], h[5], h[8], h[7], h[9], h[6])      # N, K, epi, pro, qb, act, M
    last_sig = sig(recs[-1][0])
    ends = [i for i, (h, _) in enumerate(recs) if sig(h) == last_sig]
    # step length = distance between consecutive occurrences of the last launch (lm_head)
    per = ends[-1] - ends[-2]
    hi = ends[-1] + 1 - steps * per
    lo = hi - steps * per
    sel = recs[lo:hi]
    print(f"{len(recs)} launches in the dump, {per} skinny launches per decode step, analysing launches {lo}..{hi - 1}")
    rows = OrderedDict()
    acc = defaultdict(lambda: defaultdict(list))
    for j, (h, st) in enumerate(sel):
        pos = j % per
        layer_pos = pos if pos >= per - 1 else pos % 4           # q|k|v, o, gate|up, down x layers, then lm_head
        key = ("head" if pos == per - 1 else ("qkv", "o", "gate_up", "down")[layer_pos], h[1], h[2], h[3], h[4], h[10])
        if j < per:
            rows.setdefault(key, None)
        s0 = st[:, 0].min()
        a = acc[key]
        a["ramp"].append((st[:, 0].max() - s0) * TICK_US)
        a["stage"].append(np.mean(st[:, 2] - st[:, 0]) * TICK_US)
        a["stage_norm"].append(np.mean(st[:, 1] - st[:, 0]) * TICK_US)
        for w in range(8):
            a[f"w{w}"].append(np.mean(st[:, 8 + w] - st[:, 0]) * TICK_US)
        a["stream"].append(np.mean(st[:, 3] - st[:, 2]) * TICK_US)
        if h[3] > 1:
            a["publish"].append(np.mean(st[:, 4] - st[:, 3]) * TICK_US)
            a["count"].append(np.mean(st[:, 5] - st[:, 4]) * TICK_US)
            lastm = st[:, 6] >= st[:, 5]
            lastm &= st[:, 5] >= s0
            a["combine"].append(np.mean((st[:, 6] - st[:, 5])[lastm]) * TICK_US if lastm.any() else 0.0)
            a["epi"].append(np.mean((st[:, 7] - st[:, 6])[lastm]) * TICK_US if lastm.any() else 0.0)
            end = max(st[:, 5].max(), st[:, 7][lastm].max() if lastm.any() else 0)
        else:
            a["publish"].append(0.0); a["count"].append(0.0); a["combine"].append(0.0)
            a["epi"].append(np.mean(st[:, 7] - st[:, 3]) * TICK_US)
            end = st[:, 7].max()
        a["total"].append((end - s0) * TICK_US)
        a["last_stream_end"].append((st[:, 3].max() - s0) * TICK_US)
        if j + 1 < len(sel):
            a["to_next"].append((sel[j + 1][1][:, 0].min() - end) * TICK_US)
    cols = ["ramp", "stage_norm", "w0", "w1", "w2", "w3", "w4", "w5", "w6", "w7", "stage", "stream", "last_stream_end", "publish", "count", "combine", "epi", "total", "to_next"]
    print(f"{'linear':<10}{'N':>7}{'K':>7}{'ksplit':>7}{'grid':>6}{'mt':>3} " + " ".join(f"{c:>7}" for c in cols))
    for key in rows:
        a = acc[key]
        print(f"{key[0]:<10}{key[1]:>7}{key[2]:>7}{key[3]:>7}{key[4]:>6}{key[5]:>3} " + " ".join(f"{np.mean(a[c]):>7.2f}" for c in cols))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    else:
        main()
