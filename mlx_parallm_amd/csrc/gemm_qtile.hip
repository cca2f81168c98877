// gemm_qtile.hip -- the prefill tile GEMM on PACKED quantised weights: nn.QuantizedLinear (MLX-affine int4 / int8, group 64) over
// many rows,  Y[M][N] = X[M][K] . W_hat[N][K]^T  with  W_hat = scale * q + bias  per group of 64, 16-bit activations.
// gemm_prefill.hip serves such a matrix through a dense [hi | lo] 16-bit copy written per call (4 bytes per weight) and a
// walk over 2 K; here the codes are unpacked in registers while the tile multiplies: no copy, one walk of K.
//
// Arithmetic (that of gemm_q4.hip and moe_q.hip), per output element in float32:
//     acc = sum over groups g of ( s_g * sum_{k in g} (OFFS + q_k) x_k  +  (b_g - OFFS s_g) * sum_{k in g} x_k )
// The (OFFS + q) x products run on v_mfma_f32_16x16x32 with OFFS + q an exact 16-bit value (qt_offs below); every group's
// chain starts from a zero C operand and is folded in by quant_accumulate (linear_epilogue.h).  s_g, b_g are the block's
// 16-bit values widened to float32; the group sums of x come from qtile_sums_kernel, once per launch.  No atomics: the same
// inputs give the same bits, and a row's bits depend on that row of x only.
//
// Shape.  Workgroup = 256 threads = 4 waves as 2 (M) x 2 (N); wave tile 64 x 64 = 4 x 4 MFMA tiles (64 accumulator
// registers), block tile 128 x 128, K step 64 = ONE quantisation group; two waves per SIMD (the .res report has the
// numbers).
//   * W comes straight from global memory, packed, and is unpacked in registers -- no LDS.  In the tile-major blocks of
//     repack.hip lane 16 g + r owns 16 bytes of codes of row r.  int8 (a 1088-byte block = one group): the lane's own 16 bytes
//     are its share of the B operands of the group's two MFMA steps (dwords 2t, 2t + 1 for step t).  int4 (a 1152-byte block =
//     two groups): a lane takes 8 bytes per group -- dwords {0, 4, 2, 6}[g] + {0, 1} of the group, the pairing of gemm_q4.hip,
//     fetched from the lane of the block that owns them, so there are no lane swaps -- and one shift + one v_and_or per
//     output dword turns them into 16-bit values.  Each wave unpacks its own four N tiles; the two waves that share them
//     (wm = 0 / 1) both do it -- 8 B operands per group step against 32 MFMAs -- instead of a pass through LDS and a second
//     barrier.  The next step's packed bytes (8 / 16 B + scale + bias per lane and N tile) are in flight while this one multiplies.
//   * X tiles (128 x 64) go global -> registers -> LDS as in gemm_tile_kernel (rows padded to 144 B, double-buffered, the
//     next tile's loads issued ahead of this step's MFMAs).  The k order inside an MFMA step is free as long as A and B
//     agree, so A follows the codes: lane group g of step t reads the 16-byte chunk qt_chunk(g, t) of the row, and for int4
//     the 8 elements of a chunk are stored as (e0 e4 e1 e5 e2 e6 e3 e7) -- the order unpack_q4 leaves the nibbles in.
//   * the group sums of x ride with the X tile: 128 floats per step, staged next to it.
//   * few (M, N) blocks (a prompt of a few hundred rows): K is split over gridDim.z workgroups; slice z leaves a float32
//     partial tile in ws[z][M][N] and qtile_splitk_kernel adds the slices in slice order and applies the epilogue.
//
// mxfp4 (MI_WK_MX4_BF16, bf16 activations) runs qtile_mx4_kernel: the same tiles, X staging, K split and epilogues around FP4
// codes converted in registers by the hardware (mx4_cvt.h) and ONE accumulator chain per tile -- its notes stand at the kernel.
#include <algorithm>

#include "gemv_phase.h"
#include "mx4_cvt.h"

namespace mi {

int gemv_cu_count();      // gemv_mfma.hip

namespace {

using namespace gemv;

constexpr int QBM = 128, QBN = 128, QBK = 64;
constexpr int QLDA = 72;   // LDS row stride in elements (144 B)

struct QtParams {
  const void* x; int ldx; int M;
  const void* w; int N, K;          // W tile-major, packed; N = rows of W (SWIGLU: gate rows = pair_offset)
  const float* sx; int Mpad;        // sums of x per (group of 64, row): [K / 64][Mpad], rows past M are zero
  int epi; void* out; int ldo; void* resid; int pair_offset;
  int ksplit; float* ws;            // K slices over gridDim.z; partial tiles [ksplit][M][N]
  const float* bias;                // LinearW::bias ([N] float32 or null): T(T(acc) + b)
};

// OFFS: what the unpacked 16-bit value carries on top of the code
template <typename AT, int BITS> struct QtOffs;
template <> struct QtOffs<bf16, 4> { static constexpr float v = 16.f; };     // unpack_q4<bf16>: 0x4180 | q << 3
template <> struct QtOffs<f16, 4> { static constexpr float v = 1024.f; };    // 0x6400 | q
template <> struct QtOffs<bf16, 8> { static constexpr float v = 0.f; };      // converted: 0..255 are exact in bf16
template <> struct QtOffs<f16, 8> { static constexpr float v = 1024.f; };    // 0x6400 | q

__device__ __forceinline__ uint32_t qt_and_or(uint32_t x, uint32_t mask, uint32_t magic) {
  uint32_t o;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(mask), "v"(magic));     // (both constants in registers: gemv_phase.h)
  return o;
}

// 8 int4 codes (one dword) -> the B operand of one MFMA step: element 2p <- nibble p, element 2p + 1 <- nibble p + 4
template <typename AT>
__device__ __forceinline__ u32x4 qt_unpack4(uint32_t v) {
  if constexpr (std::is_same<AT, bf16>::value) return unpack_q4<bf16>(v);
  else {
    const uint32_t mask = 0x000F000Fu, magic = 0x64006400u;
    return u32x4{qt_and_or(v, mask, magic), qt_and_or(v >> 4, mask, magic), qt_and_or(v >> 8, mask, magic), qt_and_or(v >> 12, mask, magic)};
  }
}
// 8 int8 codes (two dwords, k order) -> the B operand of one MFMA step, k order
template <typename AT>
__device__ __forceinline__ u32x4 qt_unpack8(uint32_t lo, uint32_t hi) {
  u32x4 r;
  if constexpr (std::is_same<AT, bf16>::value) {
    auto two = [](uint32_t a, uint32_t b) {        // bf16(a) | bf16(b) << 16: the top halves of the float32 (8 significant bits)
      return (__float_as_uint((float)a) >> 16) | (__float_as_uint((float)b) & 0xffff0000u);
    };
    r.x = two(lo & 255u, (lo >> 8) & 255u); r.y = two((lo >> 16) & 255u, lo >> 24);
    r.z = two(hi & 255u, (hi >> 8) & 255u); r.w = two((hi >> 16) & 255u, hi >> 24);
  } else {
    auto two = [](uint32_t v) { return (v & 0xffu) | ((v & 0xff00u) << 8) | 0x64006400u; };
    r.x = two(lo); r.y = two(lo >> 16); r.z = two(hi); r.w = two(hi >> 16);
  }
  return r;
}

// the 16-byte chunk (of the 8 in a 64-k group) that lane group g reads as its A operand of MFMA step t
template <int BITS>
__device__ __forceinline__ int qt_chunk(int g, int t) {
  if constexpr (BITS == 4) return ((g & 1) * 4 + (g >> 1) * 2) + t;       // dwords {0, 4, 2, 6}[g] + t of the group (gemm_q4.hip)
  else return 2 * g + t;                                                  // codes 16 g + 8 t ..
}

// 16-bit scale / bias of the block -> float32
template <typename AT>
__device__ __forceinline__ float qt_widen(uint32_t bits16) {
  if constexpr (std::is_same<AT, bf16>::value) return __uint_as_float(bits16 << 16);
  else return (float)__builtin_bit_cast(f16, (unsigned short)bits16);
}

// sx[group][row] = sum of the group's 64 activations of the row, float32, in a fixed order (8 consecutive, then a
// butterfly over the 8 threads of the group); rows [M, Mpad) are written as zeros.  One workgroup per row.
template <typename AT>
__global__ __launch_bounds__(256) void qtile_sums_kernel(const AT* x, int ldx, int M, int Mpad, int K, float* sx) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const bool live = row < M;
  const AT* xr = x + (size_t)(live ? row : 0) * ldx;
  for (int k = tid * 8; k < K; k += 2048) {
    float sum = 0.f;
    if (live) {
      const u32x4 v = *(const u32x4*)(xr + k);
      const AT* e = (const AT*)&v;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += (float)e[j];
    }
    sum = lane8_sum(sum);
    if ((tid & 7) == 0) sx[(size_t)(k >> 6) * Mpad + row] = sum;
  }
}

template <typename AT>
__device__ __forceinline__ void qt_store_plain(const QtParams& p, int m, int n, float acc) {
  const float y = linear_value<AT>(acc, p.bias != nullptr, p.bias, n, 1, RND_NONE);
  if (p.epi == EPI_STORE) ((AT*)p.out)[(size_t)m * p.ldo + n] = (AT)y;
  else if (p.epi == EPI_STORE_F32) ((float*)p.out)[(size_t)m * p.ldo + n] = y;
  else { AT* h = (AT*)p.resid; h[(size_t)m * p.ldo + n] = (AT)((float)h[(size_t)m * p.ldo + n] + y); }
}

// ---- the X tile of one K step (128 rows x 64 k), shared by the tile kernels of this file: 128 rows x 8 chunks of 16 B, thread ->
// chunks tid, tid + 256, ..; straight-line loads (rows past M read row M - 1 and are zeroed on the way into LDS)
template <typename AT>
struct QtXTile {
  u32x4 areg[4];
  const AT* arow[4];
  int live;                        // rows of the tile inside the matrix
  __device__ __forceinline__ QtXTile(const AT* x, int ldx, int M, int m0, int tid) : live(M - m0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i, row = c >> 3, kq = c & 7;
      arow[i] = x + (size_t)min(m0 + row, M - 1) * ldx + kq * 8;
    }
  }
  __device__ __forceinline__ void load(int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) areg[i] = *(const u32x4*)(arow[i] + s * QBK);
  }
  // PERM (int4): the 8 elements of a chunk go (e0 e1 | e2 e3 | e4 e5 | e6 e7) -> (e0 e4 | e1 e5 | e2 e6 | e3 e7)
  template <bool PERM>
  __device__ __forceinline__ void store(AT (*As)[QLDA], int tid) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i, row = c >> 3, kq = c & 7;
      u32x4 v = row < live ? areg[i] : u32x4{0u, 0u, 0u, 0u};
      if constexpr (PERM)
        v = u32x4{(v.x & 0xffffu) | (v.z << 16), (v.x >> 16) | (v.z & 0xffff0000u), (v.y & 0xffffu) | (v.w << 16), (v.y >> 16) | (v.w & 0xffff0000u)};
      *(u32x4*)&As[row][kq * 8] = v;
    }
  }
};

// ---- the end of a tile kernel: lane (c16, g) holds C[m = 4 g + r][n = c16] of every 16 x 16 tile of its wave's 64 x 64.
// A K slice of a split leaves its float32 partial tile for qtile_splitk_kernel; otherwise the epilogue stores.
template <typename AT, bool SWIGLU>
__device__ __forceinline__ void qt_finish(const QtParams& p, const f32x4 (&acc)[4][4], int m0, int bn, int wm, int wn, int c16, int g) {
  if constexpr (!SWIGLU) {
    if (p.ksplit > 1) {
      float* wz = p.ws + (size_t)blockIdx.z * p.M * p.N;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 64 + mt * 16 + 4 * g + r;
          if (m >= p.M) continue;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int n = bn * QBN + wn * 64 + nt * 16 + c16;
            if (n < p.N) wz[(size_t)m * p.N + n] = acc[mt][nt][r];
          }
        }
      return;
    }
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm * 64 + mt * 16 + 4 * g + r;
      if (m >= p.M) continue;
      if constexpr (SWIGLU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = bn * 64 + wn * 32 + j * 16 + c16;
          if (n >= p.pair_offset) continue;
          const float gt = linear_value<AT>(acc[mt][j][r], p.bias != nullptr, p.bias, n, 1, RND_NONE);
          const float up = linear_value<AT>(acc[mt][j + 2][r], p.bias != nullptr, p.bias, n + p.pair_offset, 1, RND_NONE);
          ((AT*)p.out)[(size_t)m * p.ldo + n] = (AT)swiglu_value<AT>(gt, up, RND_NONE);
        }
      } else {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int n = bn * QBN + wn * 64 + nt * 16 + c16;
          if (n < p.N) qt_store_plain<AT>(p, m, n, acc[mt][nt][r]);
        }
      }
    }
}

// grid: (m blocks, n blocks, K slices).  SWIGLU: a block covers 64 gate columns + the 64 matching up columns.
template <typename AT, int BITS, bool SWIGLU>
__global__ __launch_bounds__(256, 2) void qtile_kernel(QtParams p) {
  constexpr int BLK = BITS == 4 ? 1152 : 1088;         // bytes of a block of W; scales at 1024, biases behind them
  constexpr int BOFF = BITS == 4 ? 1088 : 1056;
  constexpr int CW = BITS == 4 ? 2 : 4;                // packed dwords of a lane per (N tile, group step)
  __shared__ __attribute__((aligned(16))) AT As[2][QBM][QLDA];
  __shared__ __attribute__((aligned(16))) float Sx[2][QBM];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int c16 = lane & 15, g = lane >> 4;
  // blockIdx.x = M block (fastest): the blocks that run together share the same W blocks in L2
  const int bm = blockIdx.x, bn = blockIdx.y;
  const int m0 = bm * QBM;
  const int nsteps = p.K / QBK;                        // group steps of the whole K
  const int s0 = (int)(((long)blockIdx.z * nsteps) / p.ksplit), s1 = (int)(((long)(blockIdx.z + 1) * nsteps) / p.ksplit);
  const AT* x = (const AT*)p.x;

  // the wave's four N tiles (16 rows of W each; wave-uniform); a tile past the matrix re-reads the last one and stores nothing
  const int ntiles_w = p.N / 16;
  const char* wbase[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    int t;
    if constexpr (!SWIGLU) t = (bn * QBN + wn * 64 + nt * 16) / 16;
    else t = (bn * 64 + wn * 32 + (nt & 1) * 16 + (nt >> 1) * p.pair_offset) / 16;
    wbase[nt] = (const char*)p.w + (size_t)min(t, ntiles_w - 1) * (p.K / (BITS == 4 ? 128 : 64)) * BLK;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- X tile (QtXTile).  The tile's 128 group sums: one float per thread of the first two waves.
  QtXTile<AT> xt(x, p.ldx, p.M, m0, tid);
  float sreg = 0.f;
  const float* srow = p.sx + m0 + (tid & (QBM - 1));          // (m0 + 127 < Mpad)
  auto load_a = [&](int s) {
    xt.load(s);
    sreg = srow[(size_t)s * p.Mpad];
  };
  auto store_a = [&](int buf) {
    xt.template store<BITS == 4>(As[buf], tid);
    if (tid < QBM) Sx[buf][tid] = sreg;
  };

  // ---- W: the packed codes of group step s that this lane multiplies, + the scale and bias of its column c16.
  // int4: the group's 8 dwords of row r lie in the lanes 16 (2 h + j) + r of the block (h = the group's half of the block, j = 0 / 1)
  // as 4 dwords each; lane group g takes the dwords {0, 4, 2, 6}[g] + {0, 1} = lane 16 (2 h + (g & 1)) + r, dwords 2 (g >> 1) + {0, 1}
  // -- an 8-byte load, the two steps' operands (the pairing of gemm_q4.hip, without its lane swaps).  int8: the lane's own 16 bytes.
  uint32_t wr[4][CW], sr[4], br[4];
  const int coff = BITS == 4 ? (((g & 1) * 16 + c16) * 16 + (g >> 1) * 8) : lane * 16;
  const int soff = 1024 + c16 * (BITS == 4 ? 4 : 2);
  auto load_w = [&](int s) {
    const int h = BITS == 4 ? (s & 1) : 0;
    const size_t boff = (size_t)(BITS == 4 ? (s >> 1) : s) * BLK;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const char* blk = wbase[nt] + boff;
      if constexpr (BITS == 4) {
        const u32x2 v = *(const u32x2*)(blk + h * 512 + coff);
        wr[nt][0] = v.x; wr[nt][1] = v.y;
      } else {
        const u32x4 v = *(const u32x4*)(blk + coff);
        wr[nt][0] = v.x; wr[nt][1] = v.y; wr[nt][2] = v.z; wr[nt][3] = v.w;
      }
      sr[nt] = *(const uint16_t*)(blk + soff + 2 * h);
      br[nt] = *(const uint16_t*)(blk + soff + 2 * h + (BOFF - 1024));
    }
  };

  const int ach0 = qt_chunk<BITS>(g, 0) * 8, ach1 = qt_chunk<BITS>(g, 1) * 8;

  // one group step out of LDS buffer `cur`; the next step's X tile and packed codes are in flight meanwhile
  auto step = [&](int s, int cur) {
    load_a(min(s + 1, s1 - 1));
    u32x4 bq[4][2];
    float sc[4], bb[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if constexpr (BITS == 4) {
        bq[nt][0] = qt_unpack4<AT>(wr[nt][0]);
        bq[nt][1] = qt_unpack4<AT>(wr[nt][1]);
      } else {
        bq[nt][0] = qt_unpack8<AT>(wr[nt][0], wr[nt][1]);
        bq[nt][1] = qt_unpack8<AT>(wr[nt][2], wr[nt][3]);
      }
      sc[nt] = qt_widen<AT>(sr[nt]);
      bb[nt] = fmaf(-QtOffs<AT, BITS>::v, sc[nt], qt_widen<AT>(br[nt]));
    }
    __builtin_amdgcn_sched_barrier(0);
    load_w(min(s + 1, s1 - 1));                    // (the registers are free: their codes are unpacked)
    __builtin_amdgcn_sched_barrier(0);             // the loads stay ahead of this step's MFMAs
    // 8 items of (row tile mt, N tile pair): the item's four MFMAs (two chains of two, from a zero C operand) are issued, then
    // the PREVIOUS item's partials are folded into the accumulators -- their MFMAs finished while these were issued.  Left to
    // hipcc every fold sat right behind its own MFMA and waited out its latency (measured: 0.6 PFLOP/s at 8192 rows).  The order
    // is pinned item by item; the A fragments and group sums of the next row tile are read one row tile ahead.
    u32x4 af[2][2];
    f32x4 sxr[2], pd[2], psx;
    auto rd = [&](int mt, int slot) {
      const int row = wm * 64 + mt * 16;
      af[slot][0] = *(const u32x4*)&As[cur][row + c16][ach0];
      af[slot][1] = *(const u32x4*)&As[cur][row + c16][ach1];
      sxr[slot] = *(const f32x4*)&Sx[cur][row + 4 * g];            // the C layout: lane (c16, g) holds rows 4 g + r
    };
    rd(0, 0);
#pragma unroll
    for (int it = 0; it < 9; ++it) {
      const int mt = it >> 1, n0 = (it & 1) * 2, sl = mt & 1;
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
      if (it < 8) {
        if ((it & 1) == 0 && mt + 1 < 4) rd(mt + 1, sl ^ 1);
        d0 = mfma16<AT>(af[sl][0], bq[n0][0], d0);
        d1 = mfma16<AT>(af[sl][0], bq[n0 + 1][0], d1);
        d0 = mfma16<AT>(af[sl][1], bq[n0][1], d0);
        d1 = mfma16<AT>(af[sl][1], bq[n0 + 1][1], d1);
      }
      if (it > 0) {
        const int pmt = (it - 1) >> 1, pn = ((it - 1) & 1) * 2;
        quant_accumulate(acc[pmt][pn], sc[pn], bb[pn], pd[0], psx);
        quant_accumulate(acc[pmt][pn + 1], sc[pn + 1], bb[pn + 1], pd[1], psx);
      }
      pd[0] = d0; pd[1] = d1; psx = sxr[sl];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (s + 1 < s1) {
      store_a(cur ^ 1);         // buffer cur ^ 1 was last read one step ago; the barrier of that step separates
      __syncthreads();
    }
  };

  load_a(s0);
  load_w(s0);
  store_a(0);
  __syncthreads();
  for (int s = s0; s < s1; s += 2) {               // two steps per trip: the LDS buffer is a compile-time index
    step(s, 0);
    if (s + 1 < s1) step(s + 1, 1);
  }

  qt_finish<AT, SWIGLU>(p, acc, m0, bn, wm, wn, c16, g);
}

// ---- mxfp4 (MI_WK_MX4_BF16, tile-major blocks of 16 rows x 128 k = 1088 bytes), bf16 activations.  Same grid, waves, tiles,
// X staging and end as qtile_kernel; what differs is everything about W:
//   * a lane's own 16 bytes of a block ARE its B operands of the block's four MFMA steps: dword T holds k = 32 T + 8 g + e, code
//     e at nibble e, and mx_operand (four v_cvt_scalef32_pk_bf16_fp4) makes step T's eight dequantised bf16 values from it and
//     scale byte T of the row's dword.  The k order is the natural one: lane group g of step t of an X tile reads chunk 4 t + g.
//   * a step of 32 k is one MX group and there is no bias: nothing is folded outside the MFMA chain, acc = mfma(a, b, acc) over
//     the whole K slice, 16 independent chains per wave and step.  No group sums of x, no workspace but the K split's.
//   * the conversions are software-pipelined one MFMA step ahead, also across the block edge: while the 16 MFMAs of step T issue
//     (four items of one row tile x four N tiles), item i converts N tile i's operand of step T + 1 into the other half of bq.
//     After the prologue no MFMA waits for a conversion of its own step.  The order is pinned item by item.
//   * two blocks of codes + scales are in registers: wq (being converted) and wqn (the block after it).  When step 3's operands
//     are converted -- behind the items of step 2 -- wq takes wqn and the block after that is requested into wqn.  Nothing reads
//     wqn before the next block's move; the first wait that covers its loads is the vmcnt(0) of the next X tile's store, whose
//     own loads are younger: 48 MFMAs per wave after the request (read in the ISA; DESIGN 3 has what it took).  The stream is clamped to the slice's last block, the N tiles to the matrix's
//     last tile: the kernel addresses nothing beyond mi_op_tiled_bytes.
// K slices are whole blocks: slice z covers blocks [z nblk / ksplit, (z + 1) nblk / ksplit).  A trip of the loop is one block =
// two X tiles of 64 k, LDS buffers 0 and 1 (37 KB; the choice against 128-k tiles: DESIGN 3).
template <bool SWIGLU>
__global__ __launch_bounds__(256, 2) void qtile_mx4_kernel(QtParams p) {
  __shared__ __attribute__((aligned(16))) bf16 As[2][QBM][QLDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int c16 = lane & 15, g = lane >> 4;
  const int bm = blockIdx.x, bn = blockIdx.y;
  const int m0 = bm * QBM;
  const int nblk = p.K / 128;
  const int b0 = (int)(((long)blockIdx.z * nblk) / p.ksplit), b1 = (int)(((long)(blockIdx.z + 1) * nblk) / p.ksplit);
  const int slast = 2 * b1 - 1;                        // the slice's last X tile

  // the wave's four N tiles (wave-uniform); a tile past the matrix re-reads the last one and stores nothing
  const int ntiles_w = p.N / 16;
  const char* wbase[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    int t;
    if constexpr (!SWIGLU) t = (bn * QBN + wn * 64 + nt * 16) / 16;
    else t = (bn * 64 + wn * 32 + (nt & 1) * 16 + (nt >> 1) * p.pair_offset) / 16;
    wbase[nt] = (const char*)p.w + (size_t)min(t, ntiles_w - 1) * nblk * MX4_BLOCK + lane * 16;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  QtXTile<bf16> xt((const bf16*)p.x, p.ldx, p.M, m0, tid);

  u32x4 wq[4], wqn[4];            // codes: this block's, the next block's
  uint32_t sc[4], scn[4];         // the four scale bytes of the lane's row of W
  const int soff = 1024 + c16 * 4 - lane * 16;
  auto load_w = [&](int b, u32x4 (&q)[4], uint32_t (&s)[4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const char* blk = wbase[nt] + (size_t)b * MX4_BLOCK;
      q[nt] = *(const u32x4*)blk;
      s[nt] = *(const uint32_t*)(blk + soff);
    }
  };
  u32x4 bq[2][4];                 // B operands: [step parity][N tile]
  auto convert = [&](int T, int nt) {
    u32x4 r = mx_operand(wq[nt][T], mx_scale(sc[nt], T));
    // (an empty statement that holds the conversion where it is written: left alone, hipcc sank step 0's conversions of the next
    // block out of step 3's items to behind the tile's barrier, where no MFMA covers them)
    asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
    bq[T & 1][nt] = r;
  };

  // X tile s = half h of block b, out of LDS buffer h: MFMA steps T = 2 h, 2 h + 1 of the block
  auto half = [&](int b, int h) {
    const int s = 2 * b + h;
    xt.load(min(s + 1, slast));
    __builtin_amdgcn_sched_barrier(0);                 // the loads stay ahead of this tile's MFMAs
    u32x4 af[2];
    auto rd = [&](int it, int slot) {                  // item it = (step t, row tile mt): the A fragment, one item ahead
      const int t = it >> 2, mt = it & 3;
      af[slot] = *(const u32x4*)&As[h][wm * 64 + mt * 16 + c16][(4 * t + g) * 8];
    };
    rd(0, 0);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int T = 2 * h + (it >> 2), mt = it & 3, sl = it & 1;
      if (it + 1 < 8) rd(it + 1, sl ^ 1);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16<bf16>(af[sl], bq[T & 1][nt], acc[mt][nt]);
      convert((T + 1) & 3, mt);                        // N tile mt's operand of the next step (step 3: the next block's step 0)
      __builtin_amdgcn_sched_barrier(0);
      if (T == 2 && mt == 3) {                         // wq is converted to its end: the next block moves up, the one after it is requested
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          wq[nt] = wqn[nt]; sc[nt] = scn[nt];
          // (holds the move HERE: left alone, hipcc loaded into fresh registers and moved them at the end of the same trip, behind
          // a wait for loads that were ~16 MFMAs old)
          asm volatile("" : "+v"(wq[nt].x), "+v"(wq[nt].y), "+v"(wq[nt].z), "+v"(wq[nt].w), "+v"(sc[nt]));
        }
        load_w(min(b + 2, b1 - 1), wqn, scn);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (s < slast) {
      xt.template store<false>(As[h ^ 1], tid);        // buffer h ^ 1 was last read one tile ago; that tile's barrier separates
      __syncthreads();
    }
  };

  xt.load(2 * b0);
  load_w(b0, wq, sc);
  load_w(min(b0 + 1, b1 - 1), wqn, scn);
  xt.template store<false>(As[0], tid);
  __syncthreads();
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) convert(0, nt);
  for (int b = b0; b < b1; ++b) {
    half(b, 0);
    half(b, 1);
  }
  qt_finish<bf16, SWIGLU>(p, acc, m0, bn, wm, wn, c16, g);
}

// the K slices of qtile_kernel, added in slice order, + the epilogue (store / float32 store / residual); 4 columns per thread
template <typename AT>
__global__ __launch_bounds__(256) void qtile_splitk_kernel(QtParams p) {
  const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total4 = (size_t)p.M * p.N / 4;
  if (i4 >= total4) return;
  const size_t e0 = i4 * 4;
  const int m = (int)(e0 / p.N), n = (int)(e0 % p.N);
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < p.ksplit; ++z) a += *(const f32x4*)(p.ws + (size_t)z * p.M * p.N + e0);
#pragma unroll
  for (int j = 0; j < 4; ++j) qt_store_plain<AT>(p, m, n + j, a[j]);
}

// the front of the workspace: the group sums of x (mxfp4 has none: one unused line, so that no caller meets a size of zero)
size_t qt_sx_bytes(const LinearW& W, size_t rows) {
  if (wk_is_mx4(W.wk)) return 256;
  const size_t mpad = (rows + QBM - 1) / QBM * QBM;
  return ((size_t)(W.K / 64) * mpad * sizeof(float) + 255) & ~(size_t)255;
}

// K slices for a call whose (M, N) grid alone leaves CUs idle: ~512 workgroups in all (two per CU), at least 8 steps of 64 k
// per slice (mxfp4: four blocks, its slices being whole blocks), plain / float32 / residual epilogues (W.N % 4 == 0 for the reduce kernel), and the partial tiles within `cap`
int qt_ksplit(const LinearW& W, const GemvCall& c, size_t rows, size_t cap) {
  if (c.epi == EPI_SWIGLU || W.N % 4 != 0) return 1;
  const long blocks = (long)((rows + QBM - 1) / QBM) * ((W.N + QBN - 1) / QBN);
  constexpr long target = 512;
  if (blocks >= target) return 1;
  int ks = (int)std::min<long>(8, std::max<long>(1, target / blocks));
  ks = std::min(ks, (W.K / QBK) / 8);
  while (ks > 1 && (size_t)ks * rows * W.N * sizeof(float) > cap) --ks;
  return std::max(ks, 1);
}

template <typename AT, int BITS>
void qt_launch(const QtParams& p, bool sw, dim3 grid, hipStream_t st) {
  if (sw) hipLaunchKernelGGL((qtile_kernel<AT, BITS, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((qtile_kernel<AT, BITS, false>), grid, dim3(256), 0, st, p);
}

}  // namespace

// int4 / int8 (group 64, tile-major) weights, 16-bit activations in the scales' dtype, or mxfp4 (MI_WK_MX4_BF16, tile-major)
// weights, bf16 activations; no prologue (the caller normalises first), any row count; store / float32 store / residual / SwiGLU epilogues, linear bias
bool gemm_qtile_supported(const LinearW& W, const GemvCall& c, size_t rows) {
  if (c.force_v1 || c.rnd != RND_NONE || W.layout != 1 || c.pro != PRO_NONE || c.kx != 0) return false;
  const bool q4 = ((W.wk == WK_Q4_BF16 && c.act == MI_BF16) || (W.wk == WK_Q4_F16 && c.act == MI_F16)) && W.group == 64 && W.K % 128 == 0;
  const bool q8 = ((W.wk == WK_Q8_BF16 && c.act == MI_BF16) || (W.wk == WK_Q8_F16 && c.act == MI_F16)) && W.group == 64 && W.K % 64 == 0;
  const bool mx = W.wk == WK_MX4_BF16 && c.act == MI_BF16 && W.group == 32 && W.K % 128 == 0;
  if ((!q4 && !q8 && !mx) || rows < 1 || W.K < 64 || c.ldx % 8 != 0) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID && c.epi != EPI_SWIGLU) return false;
  // an adapted matrix: the caller adds the LoRA term to the stored output afterwards (launch_lora_up_add)
  if ((W.lora_b[0] != nullptr || W.lora_b[1] != nullptr) && c.epi != EPI_STORE) return false;
  if (c.epi == EPI_SWIGLU) return c.pair_offset > 0 && c.pair_offset % 16 == 0 && W.N == 2 * c.pair_offset;
  return W.N % 16 == 0;
}

// the group sums of x (mxfp4: none), and behind them the partial tiles of the K split the call would like (at most 128 MiB of them)
size_t gemm_qtile_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows) {
  const int ks = qt_ksplit(W, c, rows, (size_t)128 << 20);
  return qt_sx_bytes(W, rows) + (ks > 1 ? (size_t)ks * rows * W.N * sizeof(float) : 0);
}

int launch_gemm_qtile(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, size_t ws_cap) {
  if (!gemm_qtile_supported(W, c, rows)) return fail(MI_ERR_INVALID, "gemm_qtile: unsupported call");
  const size_t sxb = qt_sx_bytes(W, rows);
  if (ws == nullptr || ws_cap < sxb) return fail(MI_ERR_INVALID, "gemm_qtile: workspace missing (gemm_qtile_ws_bytes)");
  QtParams p{};
  p.x = c.x; p.ldx = c.ldx; p.M = (int)rows; p.w = W.w; p.N = W.N; p.K = W.K;
  p.sx = (const float*)ws; p.Mpad = (int)((rows + QBM - 1) / QBM * QBM);
  p.epi = c.epi; p.out = c.out; p.ldo = c.ldo; p.resid = c.resid; p.pair_offset = c.pair_offset;
  p.bias = W.bias;
  p.ksplit = qt_ksplit(W, c, rows, ws_cap - sxb);
  p.ws = (float*)((char*)ws + sxb);
  const bool b16 = c.act == MI_BF16, sw = c.epi == EPI_SWIGLU, mx = wk_is_mx4(W.wk);
  if (!mx) {                                        // (mxfp4 has no bias term: no sums, p.sx is the unused line and is never read)
    if (b16) hipLaunchKernelGGL(qtile_sums_kernel<bf16>, dim3(p.Mpad), dim3(256), 0, st, (const bf16*)c.x, c.ldx, p.M, p.Mpad, W.K, (float*)ws);
    else hipLaunchKernelGGL(qtile_sums_kernel<f16>, dim3(p.Mpad), dim3(256), 0, st, (const f16*)c.x, c.ldx, p.M, p.Mpad, W.K, (float*)ws);
  }
  MI_HIP(hipGetLastError());
  const int ncols = sw ? c.pair_offset : W.N, bnc = sw ? 64 : QBN;
  const dim3 grid((unsigned)(p.Mpad / QBM), (unsigned)((ncols + bnc - 1) / bnc), (unsigned)p.ksplit);
  const bool q4 = wk_bits(W.wk) == 4;
  if (mx) {
    if (sw) hipLaunchKernelGGL(qtile_mx4_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(qtile_mx4_kernel<false>, grid, dim3(256), 0, st, p);
  } else if (b16) { if (q4) qt_launch<bf16, 4>(p, sw, grid, st); else qt_launch<bf16, 8>(p, sw, grid, st); }
  else { if (q4) qt_launch<f16, 4>(p, sw, grid, st); else qt_launch<f16, 8>(p, sw, grid, st); }
  MI_HIP(hipGetLastError());
  if (p.ksplit > 1) {
    const size_t total4 = rows * (size_t)W.N / 4;
    const dim3 rg((unsigned)((total4 + 255) / 256));
    if (b16) hipLaunchKernelGGL(qtile_splitk_kernel<bf16>, rg, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(qtile_splitk_kernel<f16>, rg, dim3(256), 0, st, p);
    MI_HIP(hipGetLastError());
  }
  return MI_OK;
}

}  // namespace mi
