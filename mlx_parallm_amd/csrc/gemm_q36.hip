// gemm_q36.hip -- nn.QuantizedLinear at 3 and 6 bits (MLX-affine, group 64) for 1..128 rows of 16-bit activations:
// y[M][N] = x[M][K] . W_hat[N][K]^T with W_hat = scale * q + bias per group of 64, in the project's quantised form
// y += s * sum((OFFS + q) x) + (b - OFFS s) * sum(x) per group, the code products on v_mfma_f32_16x16x32_{bf16,f16}.
//
// The weights stay packed: a block (16 rows x 128 k) is 1664 bytes at 6 bits and 896 at 3 -- codes as BIT PLANES, scales and
// biases behind them (repack.hip; byte map in include/mi355_ops.h).  The planes are cut for the unpack, not for the checkpoint:
//
//   * a lane's 32 codes of a block sit in the order the MFMA B operand takes them -- step T, dword w, half-word h hold
//     k = 32 T + 8 g + 2 w + h -- so x needs NO permutation: its A fragment is 16 contiguous bytes of a row, and the staging of
//     a K block is a copy with the group sums taken on the way (8 lanes = one 64-group of a row: lane8_sum, no LDS).
//   * every plane keeps the two codes of an operand dword 16 bits apart.  One operand dword is then
//         int6:  ((nib >> a) & 0x000F000F << SH | MAGIC)  then  ((hi2 >> b) & 0x00030003 << (SH + 4) | that)
//         int3:  ((lo2 >> a) & 0x00030003 << SH | MAGIC)  then  ((hi1 >> b) & 0x00010001 << (SH + 2) | that)
//     = two shifts + two v_and_or_b32 for two codes, all shift counts compile-time, no shift ever crosses a dword.  That is
//     2 VALU per code against int4's 1 (gemv_phase.h unpack_q4); f16 adds the exact v_pk_add_f16 of -1024 per dword.
//   * MAGIC / SH put the code into the mantissa of a 16-bit float whose exponent is the code's own width, the smallest offset
//     that holds it (gemv_phase.h: a larger one costs cancellation error): bf16 int6 0x4280 | q << 1 = 64 + q, bf16 int3
//     0x4100 | q << 4 = 8 + q; f16 0x6400 | q = 1024 + q, less 1024 -> q itself, OFFS = 0.
//
// Shape of a launch: a workgroup = 4 waves, wave = one tile UNIT (two 16-row tiles of W: gate + up for SwiGLU, neighbours
// otherwise) so that every A fragment read from LDS feeds two MFMAs; MT = 1 or 2 row tiles of x (rows above 32 run as 32-row
// slabs on grid.y, which find the weights in L2); K is split over workgroups through the engine's workspace and arrival
// counters when the tile groups alone leave CUs idle (the last arriver adds the slices in slice order).
//
// Bytes in flight, per wave and K step: both planes, the scales and the biases of the NEXT block of both tiles -- 2 x 1664 B
// (int6) or 2 x 896 B (int3) in 8 load instructions that are issued together, in front of the current block's arithmetic; the
// block's planes are neighbours in memory (1 KiB + 512 B, or 512 + 256 B) and the first use of either waits for all of them,
// so both land with ONE wait.  The next block's x (MT x 16 B per thread) is requested BEFORE those weight loads: results come
// back in issue order, so the LDS write of x at the end of the step waits for x alone and the weight loads stay in flight
// across the barrier.  The unpack of one MFMA step does not depend on the MFMAs of the step before (no data flows back), so
// the scheduler is free to overlap them; how far the VALU work (2 per code) hides behind the matrix pipe has NOT been measured
// (DESIGN §5), and the ring is one block deep with compiler-placed waits where gemm_q4.hip keeps three with counted ones
// (DESIGN §8).  The stream is CLAMPED (a prefetch past the slice re-reads its last block), so the buffer carries no padding.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "gemv_phase.h"

namespace mi {

int gemv_cu_count();

namespace {

using namespace gemv;

constexpr int Q36_NW = 4;        // waves per workgroup = tile units per workgroup
constexpr int Q36_TN = 2;        // tiles per unit

struct Q36Params {
  const void* x; int ldx, M;
  const uint8_t* w; int N, K, nblk;
  int epi; void* out; int ldo; void* resid; int pair_offset;
  int ntu, ntiles, ksplit;
  float* ws; unsigned* ctr;
  const float* bias;
};

template <typename AT, int BITS> struct Q36Magic;
template <> struct Q36Magic<bf16, 6> { static constexpr uint32_t magic = 0x42804280u; static constexpr int sh = 1; static constexpr float offs = 64.f; };
template <> struct Q36Magic<bf16, 3> { static constexpr uint32_t magic = 0x41004100u; static constexpr int sh = 4; static constexpr float offs = 8.f; };
template <> struct Q36Magic<f16, 6> { static constexpr uint32_t magic = 0x64006400u; static constexpr int sh = 0; static constexpr float offs = 0.f; };
template <> struct Q36Magic<f16, 3> { static constexpr uint32_t magic = 0x64006400u; static constexpr int sh = 0; static constexpr float offs = 0.f; };

template <int N>
__device__ __forceinline__ uint32_t shr(uint32_t v) {      // v >> N, a negative N shifts left
  if constexpr (N >= 0) return v >> N;
  else return v << (-N);
}
__device__ __forceinline__ uint32_t and_or(uint32_t x, uint32_t mask, uint32_t base) {
  uint32_t o;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(mask), "v"(base));     // (both constants in registers: gemv_phase.h)
  return o;
}

// the planes of one block as a lane holds them: int6 lo = 4 nibble dwords, hi = 2 dwords of 2-bit fields; int3 lo = 2 dwords
// of 2-bit fields (lo.x, lo.y), hi.x = the dword of top bits
struct Q36Regs { u32x4 lo; u32x2 hi; uint32_t sc, bi; };

// operand dword w of MFMA step T: codes k = 32 T + 8 g + 2 w (low half) and + 1 (high half)
template <typename AT, int BITS, int T, int W>
__device__ __forceinline__ uint32_t q36_dword(const Q36Regs& r) {
  using M = Q36Magic<AT, BITS>;
  constexpr int F = 2 * (4 * (T & 1) + W);                  // the 2-bit field of (T, w) in its plane dword
  uint32_t v;
  if constexpr (BITS == 6) {
    v = and_or(shr<4 * W - M::sh>(r.lo[T]), 0x000F000Fu << M::sh, M::magic);
    v = and_or(shr<F - M::sh - 4>(r.hi[T >> 1]), 0x00030003u << (M::sh + 4), v);
  } else {
    v = and_or(shr<F - M::sh>(r.lo[T >> 1]), 0x00030003u << M::sh, M::magic);
    v = and_or(shr<4 * T + W - M::sh - 2>(r.hi.x), 0x00010001u << (M::sh + 2), v);
  }
  if constexpr (std::is_same<AT, f16>::value) {
    const f16x2 off = {(_Float16)1024.f, (_Float16)1024.f};
    v = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, v) - off);
  }
  return v;
}
template <typename AT, int BITS, int T>
__device__ __forceinline__ u32x4 q36_operand(const Q36Regs& r) {
  return u32x4{q36_dword<AT, BITS, T, 0>(r), q36_dword<AT, BITS, T, 1>(r), q36_dword<AT, BITS, T, 2>(r), q36_dword<AT, BITS, T, 3>(r)};
}

// 16-bit element `grp` (0 / 1) of a scale / bias dword
template <typename AT>
__device__ __forceinline__ float half_of(uint32_t dw, int grp) {
  if constexpr (std::is_same<AT, bf16>::value) return __uint_as_float(grp ? (dw & 0xffff0000u) : (dw << 16));
  else return (float)__builtin_bit_cast(f16, (unsigned short)(dw >> (16 * grp)));
}

template <typename AT, int BITS, int MT>
__global__ __launch_bounds__(Q36_NW * 64) void q36_kernel(const Q36Params p) {
  constexpr int TN = Q36_TN, MB = 16 * MT, BLK = q36_block_bytes(BITS);
  constexpr int XBUF = 4 * MT * 1024, SBUF = 2 * MB * 4;     // a block of x as fragments [T][mt][lane] x 16 B; sums [group][row]
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (XBUF + SBUF)];
  __shared__ int last_sh;

  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.y, row0 = slab * MB;
  const int grp = blockIdx.x / p.ksplit, s = blockIdx.x - grp * p.ksplit;
  const int tu = grp * Q36_NW + wave;
  const bool valid = tu < p.ntu;                             // (uniform) a spare wave stages x, keeps the barriers and loads no weight
  const bool swiglu = p.epi == EPI_SWIGLU;
  int tile[TN];
  tile[0] = swiglu ? tu : 2 * tu;
  tile[1] = swiglu ? tu + (p.pair_offset >> 4) : 2 * tu + 1;
  const bool have[TN] = {valid, valid && (swiglu || tile[1] < p.ntiles)};
  const int b0 = (s * p.nblk) / p.ksplit, b1 = ((s + 1) * p.nblk) / p.ksplit;      // this workgroup's 128-k blocks (b1 > b0: ksplit <= nblk)

  // ---- x: thread t owns pieces t, t + 256, .. of the block's 16 MT rows x 16 pieces (8 k each); 8 neighbouring threads hold
  // one 64-group of one row
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
      sum = lane8_sum(sum);
      *(u32x4*)(buf + ((((kp >> 2) * MT + (row >> 4)) * 64) + (kp & 3) * 16 + (row & 15)) * 16) = xv[i];
      if ((tid & 7) == 0) *(float*)(buf + XBUF + ((kp >> 3) * MB + row) * 4) = sum;
    }
  };

  // ---- weights: the lane's share of block b of tile a; the planes, scales and biases of a block are one contiguous run
  // One slab: the planes are read once -- streaming (non-temporal) loads.  Several slabs read the same planes at about the same
  // time and the later ones are meant to find them in L2: plain loads there, so the hint does not work against the reuse.
  const bool stream = gridDim.y == 1;
  auto ld4 = [&](const void* q) { return stream ? __builtin_nontemporal_load((const u32x4*)q) : *(const u32x4*)q; };
  auto ld2 = [&](const void* q) { return stream ? __builtin_nontemporal_load((const u32x2*)q) : *(const u32x2*)q; };
  auto ld1 = [&](const void* q) { return stream ? __builtin_nontemporal_load((const uint32_t*)q) : *(const uint32_t*)q; };
  auto load_w = [&](int a, int b, Q36Regs& r) {
    const uint8_t* blk = p.w + ((size_t)tile[a] * p.nblk + b) * BLK;
    if constexpr (BITS == 6) {
      r.lo = ld4(blk + lane * 16);
      r.hi = ld2(blk + 1024 + lane * 8);
      r.sc = *(const uint32_t*)(blk + 1536 + c16 * 4);
      r.bi = *(const uint32_t*)(blk + 1600 + c16 * 4);
    } else {
      const u32x2 l2 = ld2(blk + lane * 8);
      r.lo = u32x4{l2.x, l2.y, 0u, 0u};
      r.hi = u32x2{ld1(blk + 512 + lane * 4), 0u};
      r.sc = *(const uint32_t*)(blk + 768 + c16 * 4);
      r.bi = *(const uint32_t*)(blk + 832 + c16 * 4);
    }
  };

  f32x4 acc[TN][MT];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one block of both tiles against all row tiles: per 64-group two MFMA steps per (tile, row tile), then
  // acc += s d + (b - OFFS s) sum(x) on the lane's four rows (quant_accumulate)
  auto block_mfma = [&](const Q36Regs (&wr)[TN], const unsigned char* buf) {
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
      u32x4 wq[TN][2];
      float sc[TN], bb[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        if (sg == 0) { wq[a][0] = q36_operand<AT, BITS, 0>(wr[a]); wq[a][1] = q36_operand<AT, BITS, 1>(wr[a]); }
        else { wq[a][0] = q36_operand<AT, BITS, 2>(wr[a]); wq[a][1] = q36_operand<AT, BITS, 3>(wr[a]); }
        sc[a] = half_of<AT>(wr[a].sc, sg);
        bb[a] = fmaf(-Q36Magic<AT, BITS>::offs, sc[a], half_of<AT>(wr[a].bi, sg));
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const u32x4 a0 = *(const u32x4*)(buf + (((2 * sg + 0) * MT + mt) * 64 + lane) * 16);
        const u32x4 a1 = *(const u32x4*)(buf + (((2 * sg + 1) * MT + mt) * 64 + lane) * 16);
        const f32x4 sx = *(const f32x4*)(buf + XBUF + (sg * MB + mt * 16 + g * 4) * 4);
#pragma unroll
        for (int a = 0; a < TN; ++a) {
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
          d = mfma16<AT>(a0, wq[a][0], d);
          d = mfma16<AT>(a1, wq[a][1], d);
          quant_accumulate(acc[a][mt], sc[a], bb[a], d, sx);
        }
      }
    }
  };

  // ================= the slice: block b is multiplied while block b + 1 (x first, then the weights) is in flight
  unsigned char* cur = smem;
  unsigned char* nxt = smem + XBUF + SBUF;
  Q36Regs wa[TN] = {}, wb[TN] = {};
  u32x4 xv[MT];
  load_x(b0, xv);
#pragma unroll
  for (int a = 0; a < TN; ++a) if (have[a]) load_w(a, b0, wa[a]);
  store_x(cur, xv);
  __syncthreads();
  auto step = [&](int b, const Q36Regs (&wc)[TN], Q36Regs (&wn)[TN]) {
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

  // ================= K split over workgroups, as gemm_q4.hip: write-through partial tiles, every wave drains its stores, one
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

struct Q36Plan { int mt, nslab, ntiles, ntu, ngroups, nblk, ksplit; size_t ws_bytes; };

// K slices: enough workgroups for two per CU, at least two blocks per slice, at most 8 slices (a slice's partial tiles are
// written and read once; more slices than that cost more than the idle CUs they fill)
Q36Plan q36_plan(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) {
  Q36Plan pl{};
  const bool sw = c.epi == EPI_SWIGLU;
  pl.ntiles = (sw ? c.pair_offset : W.N) / 16;
  pl.ntu = sw ? pl.ntiles : (pl.ntiles + 1) / 2;
  pl.ngroups = (pl.ntu + Q36_NW - 1) / Q36_NW;
  pl.nblk = W.K / 128;
  const int mt_all = (int)((rows + 15) / 16);
  pl.mt = std::min(mt_all, 2);
  pl.nslab = (mt_all + pl.mt - 1) / pl.mt;
  if (ksplit > 0) pl.ksplit = std::min(ksplit, pl.nblk);
  else {
    const int wgs = pl.ngroups * pl.nslab, want = 2 * gemv_cu_count();
    pl.ksplit = std::max(1, std::min({(want + wgs - 1) / wgs, 8, pl.nblk / 2}));
  }
  pl.ws_bytes = pl.ksplit > 1 ? (size_t)pl.nslab * pl.ksplit * pl.ntu * Q36_TN * pl.mt * 1024 : 0;
  return pl;
}

template <typename AT, int BITS>
int q36_launch(const Q36Params& p, const Q36Plan& pl, hipStream_t st) {
  const dim3 grid(pl.ngroups * pl.ksplit, pl.nslab), block(Q36_NW * 64);
  if (pl.mt == 1) hipLaunchKernelGGL((q36_kernel<AT, BITS, 1>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((q36_kernel<AT, BITS, 2>), grid, block, 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace

bool gemm_q36_supported(const LinearW& W, const GemvCall& c, size_t rows) {
  if (c.force_v1 || W.layout != 1 || c.rnd != RND_NONE || !wk_is_q36(W.wk) || W.group != 64 || W.K % 128 != 0) return false;
  const int sdt = wk_scale_dtype(W.wk);
  if (sdt != c.act || (c.act != MI_BF16 && c.act != MI_F16)) return false;       // 16-bit activations in the scales' dtype
  if (rows < 1 || rows > 128 || c.ldx % 8 != 0 || c.kx != 0) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID && c.epi != EPI_SWIGLU) return false;
  if (c.lora_t != nullptr) return false;                     // (adapters ride beside the linear: lora_rows.hip)
  const int n = c.epi == EPI_SWIGLU ? c.pair_offset : W.N;
  return n % 16 == 0 && W.N % 16 == 0 && (c.epi != EPI_SWIGLU || W.N == 2 * c.pair_offset);
}

int gemm_q36_ksplit(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return q36_plan(W, c, rows, ksplit).ksplit; }
size_t gemm_q36_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return q36_plan(W, c, rows, ksplit).ws_bytes; }
int gemm_q36_groups(const LinearW& W, const GemvCall& c, size_t rows) {
  const Q36Plan pl = q36_plan(W, c, rows, 0);
  return pl.ngroups * pl.nslab;
}

int launch_gemm_q36(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr, int ksplit) {
  if (!gemm_q36_supported(W, c, rows)) return fail(MI_ERR_INVALID, "gemm_q36: unsupported call");
  if (c.pro != PRO_NONE) return fail(MI_ERR_INVALID, "gemm_q36: normalise the activations first");
  const Q36Plan pl = q36_plan(W, c, rows, ksplit);
  if (pl.ksplit > 1 && (ws == nullptr || ctr == nullptr)) return fail(MI_ERR_INVALID, "gemm_q36: workspace missing");
  const int bits = wk_bits(W.wk);
  // the over-read rule of these kinds (include/mi355_ops.h): every block a wave addresses is a block of the matrix -- tiles
  // below N / 16, blocks inside a slice's own [b0, b1), prefetches clamped to b1 - 1 -- so the stream ends where tiled_bytes
  // ends; that the caller's buffer holds tiled_bytes is the caller's contract (LinearW carries no size to check it against)
  Q36Params p{};
  p.x = c.x; p.ldx = c.ldx; p.M = (int)rows;
  p.w = (const uint8_t*)W.w; p.N = W.N; p.K = W.K; p.nblk = pl.nblk;
  p.epi = c.epi; p.out = c.out; p.ldo = c.ldo; p.resid = c.resid; p.pair_offset = c.epi == EPI_SWIGLU ? c.pair_offset : 0;
  p.ntu = pl.ntu; p.ntiles = pl.ntiles; p.ksplit = pl.ksplit;
  p.ws = (float*)ws; p.ctr = ctr; p.bias = W.bias;
  if (c.act == MI_BF16) return bits == 6 ? q36_launch<bf16, 6>(p, pl, st) : q36_launch<bf16, 3>(p, pl, st);
  return bits == 6 ? q36_launch<f16, 6>(p, pl, st) : q36_launch<f16, 3>(p, pl, st);
}

}  // namespace mi
