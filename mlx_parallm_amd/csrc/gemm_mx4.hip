// gemm_mx4.hip -- nn.QuantizedLinear in MLX's "mxfp4" mode (OCP Microscaling FP4: E2M1 codes, one E8M0 power-of-two scale per
// 32 weights, no bias) for 1..128 rows of bf16 activations: y[M][N] = x[M][K] . W_hat[N][K]^T with W_hat = code x 2^(s - 127),
// the products on v_mfma_f32_16x16x32_bf16, float32 accumulation.  W_hat is exact in bf16 (two significant bits, float32's
// exponent range), so the project's numerics contract holds with no rounding of its own: the reference's dequantised weights.
//
// The weights stay packed: a block (16 rows x 128 k) is 1024 bytes of codes and one dword of four scale bytes per row, 1088
// bytes (repack.hip; byte map in include/mi355_ops.h) -- 4.25 bits per weight against 5 for affine int4 in groups of 32.
//
//   * gfx950 converts in hardware: v_cvt_scalef32_pk_bf16_fp4 turns the two codes of one byte and a float32 scale into two bf16
//     values.  A lane's dword T of a block holds k = 32 T + 8 g + e with code e at nibble e (the checkpoint's own order), so four
//     conversions with byte_sel 0..3 ARE the eight values of the MFMA B operand of step T: 0.5 VALU per code (affine int4: 1),
//     and the operand is already the dequantised weight.
//   * ONE MFMA STEP IS ONE MX GROUP.  Its scale is byte T of the row's dword, (dw >> 8 T & 0xff) << 23 as float32 bits, handed
//     to the conversion.  There is no bias term, so no group sums of x, and nothing is folded in float32: the four steps of a
//     block and all blocks of a K slice chain through one MFMA accumulator per tile.  (Scale byte 0 gives an exponent field of
//     0 here; include/mi355_ops.h says what that means.  Byte 255 gives +inf, as everywhere.)
//   * x is staged to LDS as a plain copy in fragment order: no permutation, no sums, no DPP adds.
//
// Shape of a launch (that of gemm_qg.hip): a workgroup = 4 waves, wave = one tile UNIT of two 16-row tiles of W (SwiGLU: gate +
// up; neighbours otherwise) so that every A fragment read from LDS feeds two MFMAs; MT = 1 or 2 row tiles
// of x (rows above 32 run as 32-row slabs on grid.y, which find the weights in L2); K is split over workgroups through the
// engine's workspace and arrival counters (the last arriver adds the slices in slice order: deterministic).
//
// Bytes in flight, per wave and K step: codes and scales of the NEXT block of all tiles of the unit, issued together in front of
// the current block's arithmetic.  The next block's x (MT x 16 B per thread) is requested BEFORE those weight loads: results
// come back in issue order, so the LDS write of x at the end of the step waits for x alone and the weight loads stay in flight
// across the barrier.  The stream is CLAMPED (a prefetch past the slice re-reads its last block), so the buffer carries no
// padding: a kernel of this file never reads past mi_op_tiled_bytes.
#include <algorithm>
#include <atomic>

#include "gemv_phase.h"
#include "mx4_cvt.h"

namespace mi {

int gemv_cu_count();

namespace {

using namespace gemv;

constexpr int MX_NW = 4;        // waves per workgroup = tile units per workgroup
constexpr int MX_TN = 2;        // tiles per unit

struct MxParams {
  const void* x; int ldx, M;
  const uint8_t* w; int N, K, nblk;
  int epi; void* out; int ldo; void* resid; int pair_offset;
  int ntu, ntiles, ksplit;
  float* ws; unsigned* ctr;
  const float* bias;
};

// a lane's share of one block: its 32 codes and the four scale bytes of its row of the tile
struct MxRegs { u32x4 q; uint32_t sc; };

template <int MT>
__global__ __launch_bounds__(MX_NW * 64) void mx4_kernel(const MxParams p) {
  constexpr int TN = MX_TN, MB = 16 * MT;
  constexpr int XBUF = 4 * MT * 1024;                        // a block of x as fragments [T][mt][lane] x 16 B
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XBUF];
  __shared__ int last_sh;

  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.y, row0 = slab * MB;
  const int grp = blockIdx.x / p.ksplit, s = blockIdx.x - grp * p.ksplit;
  const int tu = grp * MX_NW + wave;
  const bool valid = tu < p.ntu;                             // (uniform) a spare wave stages x, keeps the barriers and loads no weight
  const bool swiglu = p.epi == EPI_SWIGLU;
  int tile[TN];
  tile[0] = swiglu ? tu : 2 * tu;
  tile[1] = swiglu ? tu + (p.pair_offset >> 4) : 2 * tu + 1;
  const bool have[TN] = {valid, valid && (swiglu || tile[1] < p.ntiles)};     // (odd tile count: the last unit holds one tile)
  const int b0 = (s * p.nblk) / p.ksplit, b1 = ((s + 1) * p.nblk) / p.ksplit;      // this workgroup's 128-k blocks (b1 > b0: ksplit <= nblk)

  // ---- x: thread t owns pieces t, t + 256, .. of the block's 16 MT rows x 16 pieces (8 k each); a plain copy
  const bf16* x = (const bf16*)p.x;
  auto load_x = [&](int b, u32x4 (&xv)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int pc = tid + 256 * i, row = row0 + (pc >> 4);
      xv[i] = u32x4{0u, 0u, 0u, 0u};
      if (row < p.M) xv[i] = *(const u32x4*)(x + (size_t)row * p.ldx + (size_t)b * 128 + (pc & 15) * 8);
    }
  };
  auto store_x = [&](unsigned char* buf, const u32x4 (&xv)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int pc = tid + 256 * i, row = pc >> 4, kp = pc & 15;
      *(u32x4*)(buf + ((((kp >> 2) * MT + (row >> 4)) * 64) + (kp & 3) * 16 + (row & 15)) * 16) = xv[i];
    }
  };

  // ---- weights: the lane's share of block b of tile a (tile[a] < N / 16 and b < nblk: inside the matrix).  One slab: the codes
  // are read once -- streaming (non-temporal) loads.  Several slabs read the same codes and the later ones are meant to find them
  // in L2: plain loads there.
  const bool stream = gridDim.y == 1;
  auto load_w = [&](int a, int b, MxRegs& r) {
    const uint8_t* blk = p.w + ((size_t)tile[a] * p.nblk + b) * MX4_BLOCK;
    r.q = stream ? __builtin_nontemporal_load((const u32x4*)(blk + lane * 16)) : *(const u32x4*)(blk + lane * 16);
    r.sc = *(const uint32_t*)(blk + 1024 + c16 * 4);
  };

  f32x4 acc[TN][MT];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one block of all tiles against all row tiles: step T is MX group T of the block, its scale byte T of the row's dword
  auto block_mfma = [&](const MxRegs (&wr)[TN], const unsigned char* buf) {
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      u32x4 wq[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) wq[a] = mx_operand(wr[a].q[T], mx_scale(wr[a].sc, T));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const u32x4 a0 = *(const u32x4*)(buf + ((T * MT + mt) * 64 + lane) * 16);
#pragma unroll
        for (int a = 0; a < TN; ++a) acc[a][mt] = mfma16<bf16>(a0, wq[a], acc[a][mt]);
      }
    }
  };

  // ================= the slice: block b is multiplied while block b + 1 (x first, then the weights) is in flight
  unsigned char* cur = smem;
  unsigned char* nxt = smem + XBUF;
  MxRegs wa[TN] = {}, wb[TN] = {};
  u32x4 xv[MT];
  load_x(b0, xv);
#pragma unroll
  for (int a = 0; a < TN; ++a) if (have[a]) load_w(a, b0, wa[a]);
  store_x(cur, xv);
  __syncthreads();
  auto step = [&](int b, const MxRegs (&wc)[TN], MxRegs (&wn)[TN]) {
    const int bn = min(b + 1, b1 - 1);                       // (clamped: the last step re-reads its own block and drops it)
    load_x(bn, xv);
#pragma unroll
    for (int a = 0; a < TN; ++a) if (have[a]) load_w(a, bn, wn[a]);
    if (valid) block_mfma(wc, cur);
    store_x(nxt, xv);
    __syncthreads();                                         // the next block of x is complete; this block's buffer is free
    unsigned char* t = cur; cur = nxt; nxt = t;
  };
  for (int b = b0; b < b1; b += 2) {
    step(b, wa, wb);
    if (b + 1 < b1) step(b + 1, wb, wa);                     // (uniform over the workgroup)
  }

  // ================= K split over workgroups, as gemm_qg.hip: write-through partial tiles, every wave drains its stores, one
  // counter per (tile group, slab), the last arriver adds the slices in slice order from zero
  if (p.ksplit > 1) {
    if (valid) {
      unsigned long long* wp = (unsigned long long*)(p.ws + (((size_t)((slab * p.ksplit + s) * p.ntu + tu) * (TN * MT)) * 64 + lane) * 4);
#pragma unroll
      for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const f32x4 v = acc[a][mt];
          unsigned long long lo = ((unsigned long long)__float_as_uint(v.y) << 32) | __float_as_uint(v.x);
          unsigned long long hi = ((unsigned long long)__float_as_uint(v.w) << 32) | __float_as_uint(v.z);
          __hip_atomic_store(wp + (size_t)(a * MT + mt) * 128, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(wp + (size_t)(a * MT + mt) * 128 + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      unsigned* cp = &p.ctr[grp * gridDim.y + slab];
      const unsigned old = __hip_atomic_fetch_add(cp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == (unsigned)(p.ksplit - 1);
      if (last) __hip_atomic_store(cp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_sh = last;
    }
    __syncthreads();
    if (!last_sh) return;
    if (valid) {
#pragma unroll
      for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s2 = 0; s2 < p.ksplit; ++s2) {
        const float* rp = p.ws + (((size_t)((slab * p.ksplit + s2) * p.ntu + tu) * (TN * MT)) * 64 + lane) * 4;
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const u32x4 pv = load16_agent(rp + (size_t)(a * MT + mt) * 256);
            acc[a][mt].x += __uint_as_float(pv.x); acc[a][mt].y += __uint_as_float(pv.y);
            acc[a][mt].z += __uint_as_float(pv.z); acc[a][mt].w += __uint_as_float(pv.w);
          }
      }
    }
  }
  if (!valid) return;

  // ================= epilogue (linear_epilogue.h): lane (c16, g) holds y[row0 + 16 mt + 4 g + r][16 tile + c16]
  bf16* out = (bf16*)p.out;
  const bool has_bias = p.bias != nullptr;
  if (swiglu) {
    const int n = tile[0] * 16 + c16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + mt * 16 + g * 4 + r;
        if (m >= p.M) continue;
        const float gt = linear_value<bf16>(acc[0][mt][r], has_bias, p.bias, n, 1, RND_NONE);
        const float up = linear_value<bf16>(acc[1][mt][r], has_bias, p.bias, n + p.pair_offset, 1, RND_NONE);
        out[(size_t)m * p.ldo + n] = (bf16)swiglu_value<bf16>(gt, up, RND_NONE);
      }
    return;
  }
#pragma unroll
  for (int a = 0; a < TN; ++a) {
    if (!have[a]) break;                                     // (odd tile count: the unit's second tile does not exist)
    const int n = tile[a] * 16 + c16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + mt * 16 + g * 4 + r;
        if (m >= p.M) continue;
        const float y = linear_value<bf16>(acc[a][mt][r], has_bias, p.bias, n, 1, RND_NONE);
        if (p.epi == EPI_STORE) out[(size_t)m * p.ldo + n] = (bf16)y;
        else if (p.epi == EPI_STORE_F32) ((float*)p.out)[(size_t)m * p.ldo + n] = y;
        else { bf16* h = (bf16*)p.resid + (size_t)m * p.ldo + n; *h = (bf16)((float)*h + y); }
      }
  }
}

struct MxPlan { int mt, nslab, ntiles, ntu, ngroups, nblk, ksplit; size_t ws_bytes; };

// K slices: enough workgroups for two per CU, at least two blocks per slice, at most 8 slices (gemm_qg.hip's rule)
MxPlan mx_plan(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) {
  MxPlan pl{};
  const bool sw = c.epi == EPI_SWIGLU;
  pl.ntiles = (sw ? c.pair_offset : W.N) / 16;
  pl.ntu = sw ? pl.ntiles : (pl.ntiles + 1) / 2;
  pl.ngroups = (pl.ntu + MX_NW - 1) / MX_NW;
  pl.nblk = W.K / 128;
  const int mt_all = (int)((rows + 15) / 16);
  pl.mt = std::min(mt_all, 2);
  pl.nslab = (mt_all + pl.mt - 1) / pl.mt;
  if (ksplit > 0) pl.ksplit = std::min(ksplit, pl.nblk);
  else {
    const int wgs = pl.ngroups * pl.nslab, want = 2 * gemv_cu_count();
    pl.ksplit = std::max(1, std::min({(want + wgs - 1) / wgs, 8, pl.nblk / 2}));
  }
  pl.ws_bytes = pl.ksplit > 1 ? (size_t)pl.nslab * pl.ksplit * pl.ntu * MX_TN * pl.mt * 1024 : 0;
  return pl;
}

}  // namespace

bool gemm_mx4_supported(const LinearW& W, const GemvCall& c, size_t rows) {
  if (c.force_v1 || W.layout != 1 || c.rnd != RND_NONE || W.wk != WK_MX4_BF16 || W.group != 32 || W.K % 128 != 0) return false;
  if (c.act != MI_BF16) return false;
  if (rows < 1 || rows > 128 || c.ldx % 8 != 0 || c.kx != 0) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID && c.epi != EPI_SWIGLU) return false;
  if (c.lora_t != nullptr) return false;                     // (adapters ride beside the linear: lora_rows.hip)
  const int n = c.epi == EPI_SWIGLU ? c.pair_offset : W.N;
  return n % 16 == 0 && W.N % 16 == 0 && (c.epi != EPI_SWIGLU || W.N == 2 * c.pair_offset);
}

int gemm_mx4_ksplit(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return mx_plan(W, c, rows, ksplit).ksplit; }
size_t gemm_mx4_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return mx_plan(W, c, rows, ksplit).ws_bytes; }
int gemm_mx4_groups(const LinearW& W, const GemvCall& c, size_t rows) {
  const MxPlan pl = mx_plan(W, c, rows, 0);
  return pl.ngroups * pl.nslab;
}

int launch_gemm_mx4(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr, int ksplit) {
  if (!gemm_mx4_supported(W, c, rows)) return fail(MI_ERR_INVALID, "gemm_mx4: unsupported call");
  if (c.pro != PRO_NONE) return fail(MI_ERR_INVALID, "gemm_mx4: normalise the activations first");
  const MxPlan pl = mx_plan(W, c, rows, ksplit);
  if (pl.ksplit > 1 && (ws == nullptr || ctr == nullptr)) return fail(MI_ERR_INVALID, "gemm_mx4: workspace missing");
  // the over-read rule (include/mi355_ops.h): every block a wave addresses is a block of the matrix -- tiles below N / 16,
  // blocks inside a slice's own [b0, b1), prefetches clamped to b1 - 1; that the buffer holds tiled_bytes is the caller's contract
  MxParams p{};
  p.x = c.x; p.ldx = c.ldx; p.M = (int)rows;
  p.w = (const uint8_t*)W.w; p.N = W.N; p.K = W.K; p.nblk = pl.nblk;
  p.epi = c.epi; p.out = c.out; p.ldo = c.ldo; p.resid = c.resid; p.pair_offset = c.epi == EPI_SWIGLU ? c.pair_offset : 0;
  p.ntu = pl.ntu; p.ntiles = pl.ntiles; p.ksplit = pl.ksplit;
  p.ws = (float*)ws; p.ctr = ctr; p.bias = W.bias;
  const dim3 grid(pl.ngroups * pl.ksplit, pl.nslab), block(MX_NW * 64);
  if (pl.mt == 1) hipLaunchKernelGGL(mx4_kernel<1>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(mx4_kernel<2>, grid, block, 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
