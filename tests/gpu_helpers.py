"""Helpers for the -m gpu tests: move oracle-side NumPy data to the device and call the
kernel-level C ABI (include/mi355_ops.h) through ctypes."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np
import torch

from mlx_parallm_amd import _lib as L

TDT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
MIDT = {"float32": L.MI_F32, "bfloat16": L.MI_BF16, "float16": L.MI_F16}
ULP = {"float32": 2.0 ** -20, "bfloat16": 2.0 ** -7, "float16": 2.0 ** -10}     # 2 ulp of the dtype


def dev(a: np.ndarray, dtype: str = "float32") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TDT[dtype]).cuda().contiguous()


def dev_u32(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda().contiguous()


def dev_i32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda().contiguous()


def host(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.float32).cpu().numpy()


def ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def wk_code(kind: str) -> int:
    return L.WK[kind]


def op_linear(kind: str, N: int, K: int, w, scales=None, biases=None, group: int = 64) -> L.OpLinear:
    ol = L.OpLinear()
    ol.wk, ol.N, ol.K, ol.group = wk_code(kind), N, K, group
    ol.w, ol.scales, ol.biases = w.data_ptr(), (scales.data_ptr() if scales is not None else 0), \
        (biases.data_ptr() if biases is not None else 0)
    return ol


def to_tiled(ol: L.OpLinear, keep: list) -> bool:
    """Repack a row-major op_linear into the tile-major layout in place (the tiled buffer is appended
    to `keep`).  Returns False when the matrix is not eligible (then it stays row-major)."""
    nbytes = int(L.lib().mi_op_tiled_bytes(C.byref(ol)))
    if nbytes == 0:
        return False
    dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_repack_tiled(C.byref(ol), C.c_void_p(dst.data_ptr())))
    keep.append(dst)
    ol.w, ol.scales, ol.biases, ol.layout = dst.data_ptr(), 0, 0, 1
    return True


def gemv(ol: L.OpLinear, x, M, act, *, rnd=0, pro=0, norm_w=None, eps=0.0, epi=0, out=None, ldo=0, resid=None,
         pair_offset=0, force_generic=0, ldx=None):
    a = L.OpGemvArgs()
    a.x = x.data_ptr(); a.ldx = ldx if ldx is not None else x.shape[-1]; a.M = M
    a.act = MIDT[act]; a.rnd = rnd; a.pro = pro; a.epi = epi
    a.norm_w = norm_w.data_ptr() if norm_w is not None else 0
    a.eps = eps; a.ldo = ldo
    a.out = out.data_ptr() if out is not None else 0
    a.resid = resid.data_ptr() if resid is not None else 0
    a.pair_offset = pair_offset; a.force_generic = force_generic
    torch.cuda.synchronize()
    used_mfma = L.lib().mi_op_gemv_uses_mfma(C.byref(ol), C.byref(a))
    L.check(L.lib().mi_op_gemv(C.byref(ol), C.byref(a)))
    return bool(used_mfma)


def gemv_args(x, M, act, *, pro=0, norm_w=None, eps=0.0, epi=0, out=None, ldo=0, resid=None, pair_offset=0, ldx=None) -> L.OpGemvArgs:
    a = L.OpGemvArgs()
    a.x = x.data_ptr(); a.ldx = ldx if ldx is not None else x.shape[-1]; a.M = M
    a.act = MIDT[act]; a.rnd = 0; a.pro = pro; a.epi = epi
    a.norm_w = norm_w.data_ptr() if norm_w is not None else 0
    a.eps = eps; a.ldo = ldo
    a.out = out.data_ptr() if out is not None else 0
    a.resid = resid.data_ptr() if resid is not None else 0
    a.pair_offset = pair_offset; a.force_generic = 0
    return a


def gemv_gu8(ol: L.OpLinear, a: L.OpGemvArgs, check=True) -> int:
    """mi_op_gemv_gu8: the SwiGLU launch of gemv_mfma.hip on the row-interleaved gate|up copy (made inside the call)
    -> the return code when check is False."""
    torch.cuda.synchronize()
    rc = L.lib().mi_op_gemv_gu8(C.byref(ol), C.byref(a))
    if check:
        L.check(rc)
    return rc


def attn_shape(B, L_, Hq, Hkv, D, act, kv, rnd, cap) -> L.OpAttnShape:
    s = L.OpAttnShape()
    s.B, s.L, s.Hq, s.Hkv, s.D, s.act, s.kv, s.rnd, s.cap = B, L_, Hq, Hkv, D, MIDT[act], MIDT[kv], rnd, cap
    return s


def identity_rope(max_pos, D):
    cos = torch.ones((max_pos, D // 2), dtype=torch.float32, device="cuda")
    return cos, torch.zeros_like(cos)


@functools.lru_cache(maxsize=None)
def rope_tables(D, max_pos, base):
    """mi_op_rope_tables, computed once per (D, max_pos, base) and shared (read-only)."""
    cos = torch.zeros((max_pos, D // 2), dtype=torch.float32, device="cuda")
    sin = torch.zeros_like(cos)
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_rope_tables(ptr(cos), ptr(sin), max_pos, D, base, 1.0))
    return cos, sin


def _raw(t) -> C.c_void_p:
    return t if isinstance(t, C.c_void_p) else ptr(t)


def attention(s, q_d, kc_d, vc_d, off_d, nsplit=1, *, dma=None, exact=None, out=None, check=True):
    """mi_op_attention -> the output tensor (the return code when check is False).  dma "1" / "0": the LDS-DMA / the
    register-staged 16-bit prefill kernel; exact "1" / "0": exact float32 products / two-term operands in the float32 prefill
    (both are read by the library per call: set for this call only)."""
    if out is None:
        out = torch.zeros((s.B * s.L, s.Hq * s.D), dtype=q_d.dtype, device="cuda")
    part = torch.zeros((s.B * s.L * s.Hq * nsplit * (s.D + 2),), dtype=torch.float32, device="cuda")
    env = {k: v for k, v in (("MI_ATTN_PREFILL_DMA", dma), ("MI_ATTN_PREFILL_F32_EXACT", exact)) if v is not None}
    os.environ.update(env)
    try:
        torch.cuda.synchronize()
        rc = L.lib().mi_op_attention(C.byref(s), ptr(q_d), ptr(kc_d), ptr(vc_d), ptr(off_d), ptr(out), float(s.D ** -0.5),
                                     nsplit, ptr(part))
        torch.cuda.synchronize()
    finally:
        for k in env:
            del os.environ[k]
    if not check:
        return rc
    L.check(rc)
    return out


def attention_decode(s, qkv_d, kc, vc, off_d, cos, sin, nsplit, variant=0, *, qn_d=None, kn_d=None, rows_d=None, hrow=None,
                     hoff=None, repeat=1, out=None, read=None, check=True):
    """mi_op_attention_decode, or mi_op_attention_decode_host when device rows (rows_d) or the host lookup (hrow, hoff: ctypes
    int32 arrays) are given; `repeat` launches on the same buffers -> the output of each as float32 NumPy (a list when
    repeat > 1).  The arrival tickets must be back at zero after every launch.  kc, vc and out are tensors or raw pointers
    (buffers the caller fences); `read` replaces the read-back of out after a launch.  check False: one launch -> its
    return code."""
    part = torch.zeros((s.B * s.Hq * nsplit * (s.D + 2),), dtype=torch.float32, device="cuda")
    ctr = torch.zeros((s.B * s.Hkv,), dtype=torch.int32, device="cuda")
    if out is None:
        out = torch.zeros((s.B, s.Hq * s.D), dtype=qkv_d.dtype, device="cuda")
    args = (C.byref(s), ptr(qkv_d), _raw(kc), _raw(vc), ptr(off_d), ptr(qn_d), ptr(kn_d), 1e-6, ptr(cos), ptr(sin), _raw(out),
            float(s.D ** -0.5), 0, nsplit, ptr(part), ptr(ctr), variant, 1, None)
    outs = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        if rows_d is None and hrow is None:
            rc = L.lib().mi_op_attention_decode(*args)
        else:
            rc = L.lib().mi_op_attention_decode_host(*args, ptr(rows_d), hrow, hoff)
        if check:
            L.check(rc)
        torch.cuda.synchronize()
        assert not ctr.cpu().numpy().any()                 # tickets are handed back for the next launch
        if not check:
            return rc
        outs.append(read() if read is not None else host(out))
    return outs if repeat > 1 else outs[0]


def _addr(v) -> int:
    return 0 if v is None else (int(v) if isinstance(v, int) else v.data_ptr())


def lora_rows(*, stages, M, act, rnd, row_adapter, parts, table, t, x=None, ldx=0, K=0, pro=0, norm_w=None, eps=0.0, y=None, ldy=0,
              resid=None, ldr=0, n_parts=None, check=True):
    """mi_op_lora_rows: lora_down_by_row_kernel (stages & 1) and lora_up_add_by_row_kernel (stages & 2) of csrc/lora_rows.hip on
    the caller's buffers -> the return code.  parts: [(row0, n), ...]; table: {(part, column): (A, B, rank, scale)} with A / B
    tensors, raw addresses or None -- every other entry is null; buffers: tensors, raw addresses or None."""
    cols = L.MI_MAX_ADAPTERS + 1
    n_parts = len(parts) if n_parts is None else n_parts
    slots = max(len(parts), 3) * cols
    ta, tb = (C.c_void_p * slots)(), (C.c_void_p * slots)()
    tr, ts = (C.c_int32 * slots)(), (C.c_float * slots)()
    for (r, col), (a, b, rank, scale) in table.items():
        ta[r * cols + col], tb[r * cols + col], tr[r * cols + col], ts[r * cols + col] = _addr(a) or None, _addr(b) or None, rank, scale
    row0 = (C.c_int32 * 3)(*([p[0] for p in parts] + [0] * (3 - len(parts))))
    n = (C.c_int32 * 3)(*([p[1] for p in parts] + [0] * (3 - len(parts))))
    torch.cuda.synchronize()
    rc = L.lib().mi_op_lora_rows(_addr(x) or None, int(ldx), int(M), int(K), int(act), int(rnd), int(pro), _addr(norm_w) or None,
                                 float(eps), _addr(row_adapter) or None, int(n_parts), row0, n, ta, tb, tr, ts, _addr(t) or None,
                                 _addr(y) or None, int(ldy), _addr(resid) or None, int(ldr), int(stages))
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return rc


def close_frac(got: np.ndarray, want: np.ndarray, dtype: str, atol: float = 0.0) -> float:
    """Fraction of elements further than 2 ulp(dtype) (relative) + atol from the oracle.  A non-finite `got` is far."""
    with np.errstate(invalid="ignore"):
        tol = ULP[dtype] * np.maximum(np.abs(want), np.abs(got)) + atol
        far = ~(np.abs(got - want) <= tol)
    return float(np.mean(far | ~np.isfinite(got)))


def q4_force(mt=0, tw=0, kw=0, ksplit=0, ns=0) -> int:
    """`ksplit` argument of gemm_skinny() that forces gemm_q4.hip's plan (include/mi355_ops.h): row tiles per workgroup, tile
    units x K lanes (= compute waves), K slices over workgroups, staging waves; 0 = the cost model's choice."""
    return -(mt | tw << 3 | kw << 7 | ksplit << 11 | ns << 15)


def gemm_skinny(ol: L.OpLinear, x, M, act, *, epi=0, out=None, ldo=0, resid=None, pair_offset=0, ksplit=0, iters=0, ldx=None,
                rnd=0, norm_w=None, eps=0.0, check=True):
    """gemm_skinny.hip / gemm_q4.hip on its own (17..128 rows) -> (ksplit used, mean launch ms or None); the return code when
    check is False.  norm_w: RMSNorm in front (int4 weights above 16 rows: gemm_q4.hip's preparation pass applies it; float32
    activations without rounding: the deferred norm, norm_w float32).  A linear bias rides on ol.bias (float32 [N])."""
    a = L.OpGemvArgs()
    a.x = x.data_ptr(); a.ldx = ldx if ldx is not None else x.shape[-1]; a.M = M
    a.act = MIDT[act]; a.rnd = rnd; a.pro = 1 if norm_w is not None else 0; a.epi = epi
    a.norm_w = norm_w.data_ptr() if norm_w is not None else 0; a.eps = eps; a.ldo = ldo
    a.out = out.data_ptr() if out is not None else 0
    a.resid = resid.data_ptr() if resid is not None else 0
    a.pair_offset = pair_offset; a.force_generic = 0
    torch.cuda.synchronize()
    used, ms = C.c_int(0), C.c_float(0.0)
    rc = L.lib().mi_op_gemm_skinny(C.byref(ol), C.byref(a), int(ksplit), C.byref(used), int(iters), C.byref(ms))
    if not check:
        return rc
    L.check(rc)
    return used.value, (ms.value if iters >= 1 else None)


def gemm_prefill(ol: L.OpLinear, x, M, act, *, epi=0, out=None, ldo=0, resid=None, pair_offset=0, iters=0, ldx=None):
    """gemm_prefill.hip on its own (the tile GEMM of the prefill call) -> mean launch ms or None."""
    a = gemv_args(x, M, act, epi=epi, out=out, ldo=ldo, resid=resid, pair_offset=pair_offset, ldx=ldx)
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    L.check(L.lib().mi_op_gemm_prefill(C.byref(ol), C.byref(a), int(iters), C.byref(ms)))
    return ms.value if iters >= 1 else None


def gemm_prefill_f32(ol: L.OpLinear, x, M, *, x_terms=3, epi=0, out=None, ldo=0, resid=None, pair_offset=0, norm_w=None, eps=0.0,
                     iters=0, ldx=None, check=True):
    """gemm_prefill.hip on float32 activations (the split of x, then the tile GEMM over its image) -> the return code when
    check is False, else the mean launch ms or None."""
    a = gemv_args(x, M, "float32", pro=1 if norm_w is not None else 0, norm_w=norm_w, eps=eps, epi=epi, out=out, ldo=ldo,
                  resid=resid, pair_offset=pair_offset, ldx=ldx)
    torch.cuda.synchronize()
    ms = C.c_float(0.0)
    rc = L.lib().mi_op_gemm_prefill_f32(C.byref(ol), C.byref(a), int(x_terms), int(iters), C.byref(ms))
    if not check:
        return rc
    L.check(rc)
    return ms.value if iters >= 1 else None


def split_rows(x, rows, K, terms, out, *, norm_w=None, eps=0.0, ldx=None):
    """launch_split3_rows on its own: float32 rows -> out[rows][terms x K] bf16 bit patterns (out: an int16 tensor)."""
    torch.cuda.synchronize()
    L.check(L.lib().mi_op_split_rows(ptr(x), int(ldx if ldx is not None else x.shape[-1]), ptr(norm_w), float(eps), int(rows),
                                     int(K), int(terms), ptr(out)))
