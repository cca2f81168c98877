// gemm_qg.hip -- nn.QuantizedLinear at 4 and 8 bits in quantisation groups of 32 and 128 (MLX-affine; group 64 has kernels of
// its own: gemm_skinny.hip, gemm_q4.hip) for 1..128 rows of 16-bit activations: y[M][N] = x[M][K] . W_hat[N][K]^T with
// W_hat = scale * q + bias per group, in the project's quantised form y += s * sum((OFFS + q) x) + (b - OFFS s) * sum(x) per
// group, the code products on v_mfma_f32_16x16x32_{bf16,f16}.
//
// The weights stay packed: a block (16 rows x 128 k) is its codes (1 KiB at 4 bits, 2 KiB at 8), then 128 / GROUP scales per
// row, then as many biases -- 1280 / 1088 bytes at 4 bits, 2304 / 2112 at 8 (repack.hip; byte map in include/mi355_ops.h).
//
//   * a lane's 32 codes of a block sit in the order the MFMA B operand takes them: dword T (int4) or the 8 bytes of step T
//     (int8) hold k = 32 T + 8 g + e, and an int4 dword keeps e = 2 w at nibble w, e = 2 w + 1 at nibble w + 4 -- the order in
//     which unpack_q4 (gemv_phase.h) hands the codes out.  x therefore needs NO permutation: its A fragment is 16 contiguous
//     bytes of a row, and staging a K block is a copy with the group sums taken on the way (4 lanes = one 32-group of a row,
//     16 lanes = one 128-group: DPP adds, no LDS round).
//   * unpack: int4 is unpack_q4's magic offset (bf16: 0x4180 | q << 3 = 16 + q, OFFS = 16 folded into the bias; f16: 1024 + q
//     less 1024), 1 VALU per code; int8 is unpack_q8's conversion (0..255 are exact in both formats, OFFS = 0).
//   * THE GROUP SIZE SETS THE INNER LOOP.  One MFMA step covers 32 k.  At group 32 a step is exactly one quantisation group: its
//     4 x 4 products per lane are folded into the accumulators right away (2 FMA per accumulator element and step, against 2
//     per TWO steps at group 64), and the block needs four group sums per row.  At group 128 the four steps of a block chain
//     through one MFMA accumulator and are folded once, with one group sum per row: a quarter of group 32's float32 fold.
//     The fold of step T depends on the MFMA of step T alone and the MFMA of step T + 1 on neither, so the matrix pipe can run
//     under the fold; how far it does at group 32 is a measurement.
//
// Shape of a launch (that of gemm_q36.hip): a workgroup = 4 waves, wave = one tile UNIT (two 16-row tiles of W: gate + up for
// SwiGLU, neighbours otherwise) so that every A fragment read from LDS feeds two MFMAs; MT = 1 or 2 row tiles of x (rows above
// 32 run as 32-row slabs on grid.y, which find the weights in L2); K is split over workgroups through the engine's workspace
// and arrival counters (the last arriver adds the slices in slice order: deterministic).
//
// Bytes in flight, per wave and K step: codes, scales and biases of the NEXT block of both tiles, issued together in front of
// the current block's arithmetic.  The next block's x (MT x 16 B per thread) is requested BEFORE those weight loads: results
// come back in issue order, so the LDS write of x at the end of the step waits for x alone and the weight loads stay in flight
// across the barrier.  The stream is CLAMPED (a prefetch past the slice re-reads its last block), so the buffer carries no
// padding: a kernel of this file never reads past mi_op_tiled_bytes.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "gemv_phase.h"

namespace mi {

int gemv_cu_count();

namespace {

using namespace gemv;

constexpr int QG_NW = 4;        // waves per workgroup = tile units per workgroup
constexpr int QG_TN = 2;        // tiles per unit

struct QgParams {
  const void* x; int ldx, M;
  const uint8_t* w; int N, K, nblk;
  int epi; void* out; int ldo; void* resid; int pair_offset;
  int ntu, ntiles, ksplit;
  float* ws; unsigned* ctr;
  const float* bias;
};

// sums over 4 / 16 neighbouring lanes (common.h lane8_sum is the step between them)
__device__ __forceinline__ float lane4_sum(float v) {
  v += __builtin_amdgcn_update_dpp(0.f, v, 0xB1, 0xf, 0xf, false);    // quad_perm:[1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0.f, v, 0x4E, 0xf, 0xf, false);    // quad_perm:[2,3,0,1]
  return v;
}
__device__ __forceinline__ float lane16_sum(float v) {
  v = lane8_sum(v);
  v += __builtin_amdgcn_update_dpp(0.f, v, 0x140, 0xf, 0xf, false);   // row_mirror
  return v;
}

// a lane's share of one block: its codes (one 16-byte piece at 4 bits, two at 8), the scales and biases of its row of the tile
// (group 32: four 16-bit values each; group 128: one, in the low half of .x)
template <int BITS> struct QgRegs { u32x4 q[BITS / 4]; u32x2 sc, bi; };

// the B operand of MFMA step T: codes k = 32 T + 8 g + 0..7 as 16-bit floats
template <typename AT, int BITS>
__device__ __forceinline__ u32x4 qg_operand(const u32x4 (&q)[BITS / 4], int T) {
  if constexpr (BITS == 4) return unpack_q4<AT>(q[0][T]);
  else return unpack_q8<AT>(q[T >> 1][2 * (T & 1)], q[T >> 1][2 * (T & 1) + 1]);
}

// 16-bit element `grp` (0 / 1) of a scale / bias dword
template <typename AT>
__device__ __forceinline__ float half_of(uint32_t dw, int grp) {
  if constexpr (std::is_same<AT, bf16>::value) return __uint_as_float(grp ? (dw & 0xffff0000u) : (dw << 16));
  else return (float)__builtin_bit_cast(f16, (unsigned short)(dw >> (16 * grp)));
}

template <typename AT, int BITS, int GROUP, int MT>
__global__ __launch_bounds__(QG_NW * 64) void qg_kernel(const QgParams p) {
  constexpr int TN = QG_TN, MB = 16 * MT, NG = 128 / GROUP, CB = qg_code_bytes(BITS), BLK = qg_block_bytes(BITS, GROUP);
  constexpr int XBUF = 4 * MT * 1024, SBUF = NG * MB * 4;    // a block of x as fragments [T][mt][lane] x 16 B; sums [group][row]
  constexpr float OFFS = BITS == 4 ? Magic<AT>::offs : 0.f;
  using Regs = QgRegs<BITS>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (XBUF + SBUF)];
  __shared__ int last_sh;

  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.y, row0 = slab * MB;
  const int grp = blockIdx.x / p.ksplit, s = blockIdx.x - grp * p.ksplit;
  const int tu = grp * QG_NW + wave;
  const bool valid = tu < p.ntu;                             // (uniform) a spare wave stages x, keeps the barriers and loads no weight
  const bool swiglu = p.epi == EPI_SWIGLU;
  int tile[TN];
  tile[0] = swiglu ? tu : 2 * tu;
  tile[1] = swiglu ? tu + (p.pair_offset >> 4) : 2 * tu + 1;
  const bool have[TN] = {valid, valid && (swiglu || tile[1] < p.ntiles)};
  const int b0 = (s * p.nblk) / p.ksplit, b1 = ((s + 1) * p.nblk) / p.ksplit;      // this workgroup's 128-k blocks (b1 > b0: ksplit <= nblk)

  // ---- x: thread t owns pieces t, t + 256, .. of the block's 16 MT rows x 16 pieces (8 k each); 4 neighbouring threads hold
  // one 32-group of one row, 16 a 128-group
  const AT* x = (const AT*)p.x;
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
      const AT* e = (const AT*)&xv[i];
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += (float)e[j];
      sum = GROUP == 32 ? lane4_sum(sum) : lane16_sum(sum);
      *(u32x4*)(buf + ((((kp >> 2) * MT + (row >> 4)) * 64) + (kp & 3) * 16 + (row & 15)) * 16) = xv[i];
      if ((kp & (GROUP / 8 - 1)) == 0) *(float*)(buf + XBUF + ((kp >> 2) / (4 / NG) * MB + row) * 4) = sum;
    }
  };

  // ---- weights: the lane's share of block b of tile a; codes, scales and biases of a block are one contiguous run.
  // One slab: the codes are read once -- streaming (non-temporal) loads.  Several slabs read the same codes at about the same
  // time and the later ones are meant to find them in L2: plain loads there, so the hint does not work against the reuse.
  const bool stream = gridDim.y == 1;
  auto ld4 = [&](const void* q) { return stream ? __builtin_nontemporal_load((const u32x4*)q) : *(const u32x4*)q; };
  auto load_w = [&](int a, int b, Regs& r) {
    const uint8_t* blk = p.w + ((size_t)tile[a] * p.nblk + b) * BLK;
#pragma unroll
    for (int h = 0; h < BITS / 4; ++h) r.q[h] = ld4(blk + h * 1024 + lane * 16);
    if constexpr (NG == 4) {
      r.sc = *(const u32x2*)(blk + CB + c16 * 8);
      r.bi = *(const u32x2*)(blk + CB + 128 + c16 * 8);
    } else {
      r.sc = u32x2{*(const unsigned short*)(blk + CB + c16 * 2), 0u};
      r.bi = u32x2{*(const unsigned short*)(blk + CB + 32 + c16 * 2), 0u};
    }
  };

  f32x4 acc[TN][MT];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one block of both tiles against all row tiles.  Group 32: an MFMA step IS a quantisation group -- its product is folded at
  // once, acc += s d + (b - OFFS s) sum(x) on the lane's four rows (quant_accumulate), four folds per block; the fold of step T
  // reads nothing the MFMA of step T + 1 writes, so the two pipes overlap.  Group 128: the four steps chain into one d, one fold.
  auto block_mfma = [&](const Regs (&wr)[TN], const unsigned char* buf) {
    f32x4 d[TN][MT];
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      const int gi = T / (4 / NG);                              // the step's quantisation group in the block
      const bool first = T % (4 / NG) == 0, last = T % (4 / NG) == 4 / NG - 1;
      u32x4 wq[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) wq[a] = qg_operand<AT, BITS>(wr[a].q, T);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const u32x4 a0 = *(const u32x4*)(buf + ((T * MT + mt) * 64 + lane) * 16);
#pragma unroll
        for (int a = 0; a < TN; ++a) {
          if (first) d[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
          d[a][mt] = mfma16<AT>(a0, wq[a], d[a][mt]);
        }
      }
      if (!last) continue;
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const float sc = half_of<AT>(wr[a].sc[gi >> 1], gi & 1);
        const float bb = fmaf(-OFFS, sc, half_of<AT>(wr[a].bi[gi >> 1], gi & 1));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const f32x4 sx = *(const f32x4*)(buf + XBUF + (gi * MB + mt * 16 + g * 4) * 4);
          quant_accumulate(acc[a][mt], sc, bb, d[a][mt], sx);
        }
      }
    }
  };

  // ================= the slice: block b is multiplied while block b + 1 (x first, then the weights) is in flight
  unsigned char* cur = smem;
  unsigned char* nxt = smem + XBUF + SBUF;
  Regs wa[TN] = {}, wb[TN] = {};
  u32x4 xv[MT];
  load_x(b0, xv);
#pragma unroll
  for (int a = 0; a < TN; ++a) if (have[a]) load_w(a, b0, wa[a]);
  store_x(cur, xv);
  __syncthreads();
  auto step = [&](int b, const Regs (&wc)[TN], Regs (&wn)[TN]) {
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

  // ================= K split over workgroups, as gemm_q36.hip: write-through partial tiles, every wave drains its stores, one
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
  AT* out = (AT*)p.out;
  const bool has_bias = p.bias != nullptr;
  if (swiglu) {
    const int n = tile[0] * 16 + c16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + mt * 16 + g * 4 + r;
        if (m >= p.M) continue;
        const float gt = linear_value<AT>(acc[0][mt][r], has_bias, p.bias, n, 1, RND_NONE);
        const float up = linear_value<AT>(acc[1][mt][r], has_bias, p.bias, n + p.pair_offset, 1, RND_NONE);
        out[(size_t)m * p.ldo + n] = (AT)swiglu_value<AT>(gt, up, RND_NONE);
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
        const float y = linear_value<AT>(acc[a][mt][r], has_bias, p.bias, n, 1, RND_NONE);
        if (p.epi == EPI_STORE) out[(size_t)m * p.ldo + n] = (AT)y;
        else if (p.epi == EPI_STORE_F32) ((float*)p.out)[(size_t)m * p.ldo + n] = y;
        else { AT* h = (AT*)p.resid + (size_t)m * p.ldo + n; *h = (AT)((float)*h + y); }
      }
  }
}

struct QgPlan { int mt, nslab, ntiles, ntu, ngroups, nblk, ksplit; size_t ws_bytes; };

// K slices: enough workgroups for two per CU, at least two blocks per slice, at most 8 slices (a slice's partial tiles are
// written and read once; more slices than that cost more than the idle CUs they fill)
QgPlan qg_plan(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) {
  QgPlan pl{};
  const bool sw = c.epi == EPI_SWIGLU;
  pl.ntiles = (sw ? c.pair_offset : W.N) / 16;
  pl.ntu = sw ? pl.ntiles : (pl.ntiles + 1) / 2;
  pl.ngroups = (pl.ntu + QG_NW - 1) / QG_NW;
  pl.nblk = W.K / 128;
  const int mt_all = (int)((rows + 15) / 16);
  pl.mt = std::min(mt_all, 2);
  pl.nslab = (mt_all + pl.mt - 1) / pl.mt;
  if (ksplit > 0) pl.ksplit = std::min(ksplit, pl.nblk);
  else {
    const int wgs = pl.ngroups * pl.nslab, want = 2 * gemv_cu_count();
    pl.ksplit = std::max(1, std::min({(want + wgs - 1) / wgs, 8, pl.nblk / 2}));
  }
  pl.ws_bytes = pl.ksplit > 1 ? (size_t)pl.nslab * pl.ksplit * pl.ntu * QG_TN * pl.mt * 1024 : 0;
  return pl;
}

template <typename AT, int BITS, int GROUP>
int qg_launch(const QgParams& p, const QgPlan& pl, hipStream_t st) {
  const dim3 grid(pl.ngroups * pl.ksplit, pl.nslab), block(QG_NW * 64);
  if (pl.mt == 1) hipLaunchKernelGGL((qg_kernel<AT, BITS, GROUP, 1>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((qg_kernel<AT, BITS, GROUP, 2>), grid, block, 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
template <typename AT>
int qg_launch_kind(int bits, int group, const QgParams& p, const QgPlan& pl, hipStream_t st) {
  if (bits == 4) return group == 32 ? qg_launch<AT, 4, 32>(p, pl, st) : qg_launch<AT, 4, 128>(p, pl, st);
  return group == 32 ? qg_launch<AT, 8, 32>(p, pl, st) : qg_launch<AT, 8, 128>(p, pl, st);
}

}  // namespace

bool gemm_qg_supported(const LinearW& W, const GemvCall& c, size_t rows) {
  if (c.force_v1 || W.layout != 1 || c.rnd != RND_NONE || !wk_is_qg(W.wk, W.group) || W.K % 128 != 0) return false;
  const int sdt = wk_scale_dtype(W.wk);
  if (sdt != c.act || (c.act != MI_BF16 && c.act != MI_F16)) return false;       // 16-bit activations in the scales' dtype
  if (rows < 1 || rows > 128 || c.ldx % 8 != 0 || c.kx != 0) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID && c.epi != EPI_SWIGLU) return false;
  if (c.lora_t != nullptr) return false;                     // (adapters ride beside the linear: lora_rows.hip)
  const int n = c.epi == EPI_SWIGLU ? c.pair_offset : W.N;
  return n % 16 == 0 && W.N % 16 == 0 && (c.epi != EPI_SWIGLU || W.N == 2 * c.pair_offset);
}

int gemm_qg_ksplit(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return qg_plan(W, c, rows, ksplit).ksplit; }
size_t gemm_qg_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return qg_plan(W, c, rows, ksplit).ws_bytes; }
int gemm_qg_groups(const LinearW& W, const GemvCall& c, size_t rows) {
  const QgPlan pl = qg_plan(W, c, rows, 0);
  return pl.ngroups * pl.nslab;
}

int launch_gemm_qg(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr, int ksplit) {
  if (!gemm_qg_supported(W, c, rows)) return fail(MI_ERR_INVALID, "gemm_qg: unsupported call");
  if (c.pro != PRO_NONE) return fail(MI_ERR_INVALID, "gemm_qg: normalise the activations first");
  const QgPlan pl = qg_plan(W, c, rows, ksplit);
  if (pl.ksplit > 1 && (ws == nullptr || ctr == nullptr)) return fail(MI_ERR_INVALID, "gemm_qg: workspace missing");
  const int bits = wk_bits(W.wk);
  // the over-read rule of these kinds (include/mi355_ops.h): every block a wave addresses is a block of the matrix -- tiles
  // below N / 16, blocks inside a slice's own [b0, b1), prefetches clamped to b1 - 1 -- so the stream ends where tiled_bytes
  // ends; that the caller's buffer holds tiled_bytes is the caller's contract (LinearW carries no size to check it against)
  QgParams p{};
  p.x = c.x; p.ldx = c.ldx; p.M = (int)rows;
  p.w = (const uint8_t*)W.w; p.N = W.N; p.K = W.K; p.nblk = pl.nblk;
  p.epi = c.epi; p.out = c.out; p.ldo = c.ldo; p.resid = c.resid; p.pair_offset = c.epi == EPI_SWIGLU ? c.pair_offset : 0;
  p.ntu = pl.ntu; p.ntiles = pl.ntiles; p.ksplit = pl.ksplit;
  p.ws = (float*)ws; p.ctr = ctr; p.bias = W.bias;
  if (c.act == MI_BF16) return qg_launch_kind<bf16>(bits, W.group, p, pl, st);
  return qg_launch_kind<f16>(bits, W.group, p, pl, st);
}

}  // namespace mi
