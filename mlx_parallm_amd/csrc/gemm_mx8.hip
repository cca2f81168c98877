// gemm_mx8.hip -- nn.QuantizedLinear in MLX's "mxfp8" mode (OCP Microscaling FP8: one E4M3 code byte per weight, one E8M0
// power-of-two scale per 32 weights, no bias) for 1..128 rows of bf16 activations: y[M][N] = x[M][K] . W_hat[N][K]^T with
// W_hat = code x 2^(s - 127), the products on v_mfma_f32_16x16x32_bf16, float32 accumulation.  W_hat is exact in bf16 (four
// significant bits, float32's exponent range), so the numerics contract holds with no rounding of its own, as for mxfp4.
//
// The contract is gemm_mx4.hip's: ONE MFMA STEP IS ONE MX GROUP (scale byte T of the row's dword, s << 23 as float32 bits, goes
// into the conversion), all steps of a K slice chain through one float32 accumulator per tile, x is staged to LDS as a plain copy
// in fragment order, K is split over workgroups through the engine's workspace and arrival counters (the last arriver adds the
// slices in slice order), spare waves load no weights, and the stream is CLAMPED: no kernel of this file reads past
// mi_op_tiled_bytes.  A workgroup = 4 waves, a wave = one unit of two 16-row tiles of W (SwiGLU: gate + up), MT = 1 or 2 row
// tiles of x, rows above 32 as 32-row slabs on grid.y.
//
// What the format changes: a block (16 rows x 128 k) is 2048 bytes of codes + 64 of scales = 2112 (8.25 bits per weight; affine
// int8 in groups of 32: 9), and a lane's share of it is 32 bytes, not 16.
//
//   * Layout (repack.hip; include/mi355_ops.h): that of gemm_qg.hip's int8 codes -- two halves of 1 KiB, half T / 2 holds bytes
//     8 (T % 2) + e of the lane's 16, e in the checkpoint's byte order.  Both loads of a lane are 16-byte and lane-linear, and
//     the eight codes of step T are two whole dwords: v_cvt_scalef32_pk_bf16_fp8 on the low and the high word of each gives the
//     MFMA B operand of the step in four instructions, 0.5 VALU per code (int8 needs an unpack and a multiply-add per code and
//     the bias term's group sums of x on top).  One 32-byte run per lane would make the loads stride 32 bytes between lanes.
//   * Bytes in flight: WHOLE BLOCKS, TWO DEEP -- the block being multiplied sits in registers, the next one of both tiles is in
//     flight, 4224 bytes per wave (mxfp4: 2176).  The loads are issued scales first, then the first halves of both tiles, then
//     the second halves; results return in issue order, so steps 0 and 1 wait for the first halves only (a counted vmcnt that
//     leaves the two second halves outstanding) and steps 2 and 3 for the rest.  That is the gain a ring of 64-k half blocks
//     would bring, without halving what a wave has outstanding; a ring of half blocks two deep would hold 2112 bytes per wave,
//     less than mxfp4 streams with.  The next block's x is requested in front of all of them, so the LDS write at the end of
//     a step waits for x alone and the weights stay in flight across the barrier.  The compiler does none of this unasked:
//     the loop is shaped for it (no branch around a load, one entry state, one back edge, one exit) and two scheduling fences
//     per step keep the prefetch in front of the arithmetic and the wait for x behind it -- the comment at the loop has the
//     waits as the ISA shows them.
//   * A unit stays at two tiles: each A fragment read from LDS feeds two MFMAs, and two blocks of two tiles are 36 VGPRs; four
//     tiles would hold 72 for the weights alone and halve the units a launch has to spread over the CUs.
//   * The conversions of a step sit directly in front of its MFMAs (8 conversions, then 2 MT MFMAs): the operands live for one
//     step, and the scheduler overlaps step T + 1's conversions with step T's MFMAs.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "gemv_phase.h"
#include "mx4_cvt.h"

namespace mi {

int gemv_cu_count();

namespace {

using namespace gemv;

constexpr int M8_NW = 4;        // waves per workgroup = tile units per workgroup
constexpr int M8_TN = 2;        // tiles per unit

struct Mx8Params {
  const void* x; int ldx, M;
  const uint8_t* w; int N, K, nblk;
  int epi; void* out; int ldo; void* resid; int pair_offset;
  int ntu, ntiles, ksplit;
  float* ws; unsigned* ctr;
  const float* bias;
};

// a lane's share of one block: its 16 codes of each half and the four scale bytes of its row of the tile
struct Mx8Regs { u32x4 q[2]; uint32_t sc; };

template <int MT, bool STREAM>
__global__ __launch_bounds__(M8_NW * 64) void mx8_kernel(const Mx8Params p) {
  constexpr int TN = M8_TN, MB = 16 * MT;
  constexpr int XBUF = 4 * MT * 1024;                        // a block of x as fragments [T][mt][lane] x 16 B
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XBUF];
  __shared__ int last_sh;

  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.y, row0 = slab * MB;
  const int grp = blockIdx.x / p.ksplit, s = blockIdx.x - grp * p.ksplit;
  const int tu = grp * M8_NW + wave;
  const bool valid = tu < p.ntu;                             // (uniform) a spare wave stages x, keeps the barriers and loads no weight
  const bool swiglu = p.epi == EPI_SWIGLU;
  int tile[TN];
  tile[0] = swiglu ? tu : 2 * tu;
  tile[1] = swiglu ? tu + (p.pair_offset >> 4) : 2 * tu + 1;
  const bool have[TN] = {valid, valid && (swiglu || tile[1] < p.ntiles)};     // (odd tile count: the last unit holds one tile)
  const int b0 = (s * p.nblk) / p.ksplit, b1 = ((s + 1) * p.nblk) / p.ksplit;      // this workgroup's 128-k blocks (b1 > b0: ksplit <= nblk)

  // ---- x: thread t owns pieces t, t + 256, .. of the block's 16 MT rows x 16 pieces (8 k each); a plain copy.  Rows past M
  // read row M - 1 and are stored as zeros: an unconditional load (see the waits below)
  const bf16* x = (const bf16*)p.x;
  auto load_x = [&](int b, u32x4 (&xv)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int pc = tid + 256 * i, row = min(row0 + (pc >> 4), p.M - 1);
      xv[i] = *(const u32x4*)(x + (size_t)row * p.ldx + (size_t)b * 128 + (pc & 15) * 8);
    }
  };
  auto store_x = [&](unsigned char* buf, const u32x4 (&xv)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int pc = tid + 256 * i, row = pc >> 4, kp = pc & 15;
      *(u32x4*)(buf + ((((kp >> 2) * MT + (row >> 4)) * 64) + (kp & 3) * 16 + (row & 15)) * 16) =
          row0 + row < p.M ? xv[i] : u32x4{0u, 0u, 0u, 0u};
    }
  };

  // ---- weights: block b of both tiles of a unit that has any (wt[a] < N / 16 and b < nblk: inside the matrix), in the order
  // the steps need them -- scale dwords, first halves, second halves.  A unit whose second tile does not exist reads its first
  // tile twice and drops the copy, so the loads are UNCONDITIONAL: with a branch around any of them the compiler cannot count
  // what is outstanding and waits for everything (vmcnt(0)) at every use.  STREAM (one slab: the codes are read once):
  // non-temporal loads; several slabs read the same codes and the later ones are meant to find them in L2: plain loads.
  const int wt[TN] = {tile[0], have[1] ? tile[1] : tile[0]};
  auto load_w = [&](int b, Mx8Regs (&r)[TN]) {
    const uint8_t* blk[TN];
#pragma unroll
    for (int a = 0; a < TN; ++a) blk[a] = p.w + ((size_t)wt[a] * p.nblk + b) * MX8_BLOCK;
#pragma unroll
    for (int a = 0; a < TN; ++a) r[a].sc = *(const uint32_t*)(blk[a] + 2048 + c16 * 4);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const u32x4* src = (const u32x4*)(blk[a] + h * 1024 + lane * 16);
        r[a].q[h] = STREAM ? __builtin_nontemporal_load(src) : *src;
      }
  };

  f32x4 acc[TN][MT];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[a][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one block of all tiles against all row tiles: step T is MX group T of the block -- dwords 2 (T % 2), 2 (T % 2) + 1 of half
  // T / 2, scale byte T of the row's dword
  auto block_mfma = [&](const Mx8Regs (&wr)[TN], const unsigned char* buf) {
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      u32x4 wq[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a)
        wq[a] = mx8_operand(wr[a].q[T >> 1][2 * (T & 1)], wr[a].q[T >> 1][2 * (T & 1) + 1], mx_scale(wr[a].sc, T));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const u32x4 a0 = *(const u32x4*)(buf + ((T * MT + mt) * 64 + lane) * 16);
#pragma unroll
        for (int a = 0; a < TN; ++a) acc[a][mt] = mfma16<bf16>(a0, wq[a], acc[a][mt]);
      }
    }
  };

  // ================= the slice: block b is multiplied while block b + 1 (x first, then the weights) is in flight.  A wave
  // with a unit runs the loop with weights, a spare wave the same loop without them: the same barriers, no weight load, and
  // no branch inside either loop.
  // Waits, read from the ISA of all three instantiations: the loop head has no wait; a step issues its MT + 6 loads first (the
  // scheduling fences below hold them there), then waits for its own block with vmcnt(MT + 11) .. vmcnt(MT + 8) in front of
  // MFMA steps 0 / 1 (scales, first halves; the second halves still outstanding) and vmcnt(MT + 7), vmcnt(MT + 6) in front of
  // steps 2 / 3; the LDS write of x behind the arithmetic waits with vmcnt(6) -- x alone, the six weight loads cross the
  // barrier in flight.  The odd last block runs behind the loop without a prefetch of weights and ends on vmcnt(0).
  unsigned char* cur = smem;
  unsigned char* nxt = smem + XBUF;
  auto slice = [&](auto with_w) {
    constexpr bool WW = decltype(with_w)::value;
    Mx8Regs wa[TN] = {}, wb[TN] = {};
    u32x4 xv[MT];
    load_x(b0, xv);
    if constexpr (WW) load_w(b0, wa);
    store_x(cur, xv);
    __syncthreads();
    auto step = [&](int b, const Mx8Regs (&wc)[TN], Mx8Regs (&wn)[TN]) {
      const int bn = min(b + 1, b1 - 1);                     // (clamped: the last step re-reads its own block and drops it)
      load_x(bn, xv);
      if constexpr (WW) {
        load_w(bn, wn);
        __builtin_amdgcn_sched_barrier(0);                   // (the prefetch is issued in front of the arithmetic, not sunk behind it)
        block_mfma(wc, cur);
        __builtin_amdgcn_sched_barrier(0);                   // (nor is the wait for the next x hoisted in front of it)
      }
      store_x(nxt, xv);
      __syncthreads();                                       // the next block of x is complete; this block's buffer is free
      unsigned char* t = cur; cur = nxt; nxt = t;
    };
    // two steps per trip so that the register sets swap without moves, and an odd last block BEHIND the loop: the loop then has
    // one entry state, one back edge and one exit, all with the next block pending into `wa` alone.  (A second step skipped
    // inside the loop, or a second exit, leaves an edge on which the loop head sees loads pending into either set and drains
    // them all: s_waitcnt vmcnt(0) every second block.)
    int b = b0;
    for (; b + 1 < b1; b += 2) {                             // (uniform over the workgroup)
      step(b, wa, wb);
      step(b + 1, wb, wa);
    }
    if (b < b1) step(b, wa, wb);
  };
  if (valid) slice(std::true_type{}); else slice(std::false_type{});

  // ================= K split over workgroups, as gemm_mx4.hip: write-through partial tiles, every wave drains its stores, one
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

struct Mx8Plan { int mt, nslab, ntiles, ntu, ngroups, nblk, ksplit; size_t ws_bytes; };

// K slices: enough workgroups for two per CU, at least two blocks per slice, at most 8 slices (gemm_mx4.hip's rule)
Mx8Plan mx8_plan(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) {
  Mx8Plan pl{};
  const bool sw = c.epi == EPI_SWIGLU;
  pl.ntiles = (sw ? c.pair_offset : W.N) / 16;
  pl.ntu = sw ? pl.ntiles : (pl.ntiles + 1) / 2;
  pl.ngroups = (pl.ntu + M8_NW - 1) / M8_NW;
  pl.nblk = W.K / 128;
  const int mt_all = (int)((rows + 15) / 16);
  pl.mt = std::min(mt_all, 2);
  pl.nslab = (mt_all + pl.mt - 1) / pl.mt;
  if (ksplit > 0) pl.ksplit = std::min(ksplit, pl.nblk);
  else {
    const int wgs = pl.ngroups * pl.nslab, want = 2 * gemv_cu_count();
    pl.ksplit = std::max(1, std::min({(want + wgs - 1) / wgs, 8, pl.nblk / 2}));
  }
  pl.ws_bytes = pl.ksplit > 1 ? (size_t)pl.nslab * pl.ksplit * pl.ntu * M8_TN * pl.mt * 1024 : 0;
  return pl;
}

}  // namespace

bool gemm_mx8_supported(const LinearW& W, const GemvCall& c, size_t rows) {
  if (c.force_v1 || W.layout != 1 || c.rnd != RND_NONE || W.wk != WK_MX8_BF16 || W.group != 32 || W.K % 128 != 0) return false;
  if (c.act != MI_BF16) return false;
  if (rows < 1 || rows > 128 || c.ldx % 8 != 0 || c.kx != 0) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID && c.epi != EPI_SWIGLU) return false;
  if (c.lora_t != nullptr) return false;                     // (adapters ride beside the linear: lora_rows.hip)
  const int n = c.epi == EPI_SWIGLU ? c.pair_offset : W.N;
  return n % 16 == 0 && W.N % 16 == 0 && (c.epi != EPI_SWIGLU || W.N == 2 * c.pair_offset);
}

int gemm_mx8_ksplit(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return mx8_plan(W, c, rows, ksplit).ksplit; }
size_t gemm_mx8_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows, int ksplit) { return mx8_plan(W, c, rows, ksplit).ws_bytes; }
int gemm_mx8_groups(const LinearW& W, const GemvCall& c, size_t rows) {
  const Mx8Plan pl = mx8_plan(W, c, rows, 0);
  return pl.ngroups * pl.nslab;
}

int launch_gemm_mx8(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr, int ksplit) {
  if (!gemm_mx8_supported(W, c, rows)) return fail(MI_ERR_INVALID, "gemm_mx8: unsupported call");
  if (c.pro != PRO_NONE) return fail(MI_ERR_INVALID, "gemm_mx8: normalise the activations first");
  const Mx8Plan pl = mx8_plan(W, c, rows, ksplit);
  if (pl.ksplit > 1 && (ws == nullptr || ctr == nullptr)) return fail(MI_ERR_INVALID, "gemm_mx8: workspace missing");
  // the over-read rule (include/mi355_ops.h): every block a wave addresses is a block of the matrix -- tiles below N / 16,
  // blocks inside a slice's own [b0, b1), prefetches clamped to b1 - 1; that the buffer holds tiled_bytes is the caller's contract
  Mx8Params p{};
  p.x = c.x; p.ldx = c.ldx; p.M = (int)rows;
  p.w = (const uint8_t*)W.w; p.N = W.N; p.K = W.K; p.nblk = pl.nblk;
  p.epi = c.epi; p.out = c.out; p.ldo = c.ldo; p.resid = c.resid; p.pair_offset = c.epi == EPI_SWIGLU ? c.pair_offset : 0;
  p.ntu = pl.ntu; p.ntiles = pl.ntiles; p.ksplit = pl.ksplit;
  p.ws = (float*)ws; p.ctr = ctr; p.bias = W.bias;
  const dim3 grid(pl.ngroups * pl.ksplit, pl.nslab), block(M8_NW * 64);
  if (pl.mt == 1) hipLaunchKernelGGL((mx8_kernel<1, true>), grid, block, 0, st, p);
  else if (pl.nslab == 1) hipLaunchKernelGGL((mx8_kernel<2, true>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((mx8_kernel<2, false>), grid, block, 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
