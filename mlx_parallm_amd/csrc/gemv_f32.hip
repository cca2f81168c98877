// gemv_f32.hip -- one-pass weight-streaming GEMV for FLOAT32 activations, <= 8 rows, on dense bf16 weights in the
// tile-major layout (repack.hip): the wide linears (gate|up, lm_head) of a decode step in the float32-KV
// ("PagedKVCache") mode of a bf16 model.
//
// Same operator and the same arithmetic contract as skinny_kernel<.., X32> (gemm_skinny.hip): x = hi + mid + lo exactly
// (three bf16 terms), every product exact in the float32 accumulator -- a float32 dot product in another summation
// order; outputs float32, no logical rounding.  What differs is the shape of the launch, which is that of gemv_mfma.hip:
//
//   * One 8-wave workgroup per CU, 16-row tiles of W dealt round-robin (tile = w + i G), NO K split over workgroups:
//     no workspace, no arrival counter, no partial tiles, nothing that another workgroup of the launch reads.
//   * Chunk-outer, tile-inner.  A workgroup walks K in chunks of 1024 and, inside a chunk, all the tiles of a "pass"
//     (up to 8), with one float32 accumulator per tile held in registers for the whole pass.  A workgroup with more
//     than 8 tiles runs several passes.
//   * The eight waves split the 32 k-blocks (of 32) of a chunk round-robin, wave v owns blocks v, v + 8, v + 16, v + 24
//     -- of EVERY tile.  So a wave only ever multiplies by the x of its own four blocks, and it needs no other wave's
//     activations: each lane fetches the 8 floats of its own MFMA A-fragment position straight from x (L2), splits them
//     in registers and keeps the fragments for all the tiles of the chunk.  There is no staging through LDS, no barrier
//     inside the stream and nothing to double-buffer: a block's fragments are replaced by the next chunk's right after
//     their last use (the chunk's last tile), from registers fetched two load positions earlier, so at most two blocks'
//     raw x are live.  A workgroup reads x once per pass (32 KiB per chunk, L2 traffic).
//   * No padded rows.  An MFMA A operand has 16 rows and the call at most 8: fragment rows 0..7 of the first image hold
//     `hi`, rows 8..15 hold `mid`; the second image holds `lo` in rows 0..7 and zeros (a lane select) in rows 8..15.
//     Two v_mfma_f32_16x16x32_bf16 per 1-KiB weight block; accumulator rows m and m + 8 are added once per tile in the
//     epilogue.
//   * Every wave keeps D 16-byte non-temporal loads in flight, rolling across tile and chunk ends (and into the next pass
//     when both are full), straight-line (no load under a branch; slots past the end re-load a cached block and are
//     ignored).  D = 16 (128 KiB per CU) when a pass has 4 or 8 tiles; otherwise the largest of 14 / 12 / 10 that divides
//     the 4 NT loads of a chunk, so that the slot of every load is static.
//     Inside a chunk the waits are the counted vmcnt(D - 1) and the stream does not drain.  AT EVERY CHUNK END IT DOES, in
//     this kernel: a wave's loads return in issue order, and split_x of the next chunk needs x that was requested two
//     positions earlier, behind all but one or two of the wave's weight loads -- the compiler's wait there is vmcnt(8), with
//     12 x / norm-weight loads younger than the weights it lets through.  The wave stands for about a memory round trip with
//     its ring nearly empty, and all waves of all workgroups reach their chunk ends together (the wait sequences: DESIGN §8d).
//     The resident form at the end of this file takes x out of the vector-memory queue of the loop; it is what the wide
//     linears of K <= 4096 run on.  This kernel stays for every other K and as the bit-for-bit yardstick.
//   * RMSNorm (PRO_NORM) is deferred and local: x is multiplied by the norm weight while it is split, the squares of the
//     raw x are summed on the way (first pass only: each element once per launch), and rs[m] = rsqrt(mean + eps) scales
//     the dot product in the epilogue.  Every workgroup sees all of x, so it owns the complete row sums.  In float32
//     this differs from w * (x * rs) by one rounding per element (~6e-8), as `defer_norm` in gemm_skinny.hip.
//
// Every load is addressed as a wave-uniform 64-bit base plus a 32-bit lane offset: with one 64-bit address pair per load
// position the loop spilled, and a spill reload drains the prefetch queue.
//
// Resources: 512 threads, 254 VGPRs (one workgroup per CU), no scratch.  LDS: 32.5 KiB static -- the cross-wave
// reduction of a pass ([8 tiles][8 waves][32 lanes] float4 = 32 KiB, written once per pass after the last chunk) and
// the waves' row sums of squares (8 x 8 floats).
//
// A second kernel of this file, gemv_f32_whole_kernel, is the same operator for the one NARROW linear of that step whose
// whole tile fits a workgroup's load queue (o_proj: one tile per CU, K <= 4096): no ring, no chunks, every load up front,
// bit-identical outputs.  Its notes are in front of it.  q|k|v and down_proj stay on the split-K kernel (gemm_skinny.hip).
// A third, gemv_f32_resident{,_gu8}_kernel, is this kernel's stream with x and the norm weights kept in LDS (K <= 4096): the
// form gate|up and lm_head of Mistral-7B run on, bit-identical again; its notes are in front of it, too.
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>

#include "gemv_phase.h"

namespace mi {

namespace {

using namespace gemv;

constexpr int F32_NW = 8;                       // waves per workgroup
constexpr int F32_TP = 8;                       // tiles per pass (one accumulator each)
constexpr int F32_KB = 32;                      // k-blocks (of 32) per chunk: chunks of 1024
constexpr int F32_UB = F32_KB / F32_NW;         // blocks per wave, tile and chunk

struct F32Params {
  const float* x; int ldx; int M;
  int pro; const float* norm_w; float eps;
  const void* w; int N, K;
  int epi; float* out; int ldo; float* resid;
};

// loads per wave in flight for a pass of NT tiles (see the header)
__host__ __device__ constexpr int f32_depth(int nt) {
  const int l = nt * F32_UB;
  return l < 16 ? l : l % 16 == 0 ? 16 : l % 14 == 0 ? 14 : l % 12 == 0 ? 12 : 10;
}

// base + off as a pointer the compiler keeps in scalar registers (both are wave-uniform): the loads below then take the
// "scalar base + 32-bit lane offset" form, and no load of the stream carries a 64-bit address register pair of its own
// (global address space spelled out: an integer turned pointer would otherwise be loaded through the flat path)
typedef const __attribute__((address_space(1))) char* gptr;
typedef const __attribute__((address_space(1))) u32x4* gptr16;
__device__ __forceinline__ gptr uniform_ptr(const void* base, size_t off) {
  const uint64_t a = (uint64_t)base + off;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (gptr)(((uint64_t)hi << 32) | lo);
}

// Two floats -> hi + mid + lo exactly (three bf16 terms each) -> one dword of a lane's two A-fragment images: `low` lanes
// (fragment rows 0..7) hold hi and lo, the others mid and zeros.  Every kernel of this file splits x here, which is why
// their outputs agree bit for bit.
__device__ __forceinline__ void split3(f32x2 f, bool low, uint32_t& a0, uint32_t& a1) {
  const uint32_t hi = pack2<bf16>(f);
  const f32x2 r1 = f - unpack2<bf16>(hi);
  const uint32_t mid = pack2<bf16>(r1);
  const uint32_t lo = pack2<bf16>(r1 - unpack2<bf16>(mid));
  a0 = low ? hi : mid;
  a1 = low ? lo : 0u;
}

template <bool GU8>
struct F32Body {
  const F32Params& p;
  float* red; float* sq_sh;
  int tid, lane, wave, c16, g;
  int G, w, ntiles_all, ntiles, nkb, nchunks;
  uint32_t xoff;                // bytes from x to this lane's A-fragment position: row min(c16 & 7, M - 1), column 8 g
  uint32_t noff;                // ... in the norm weights: column 8 g (without PRO_NORM x is loaded there and ignored)
  bool norm;

  u32x4 ring[16];
  f32x4 acc[F32_TP];
  u32x4 af[F32_UB][2];          // this lane's A fragments of the wave's four blocks of a chunk: [block][image]
  u32x4 xr[F32_UB][2], nr[F32_UB][2];   // raw x / norm weights of a block on their way to af (at most two blocks are live)
  float ss = 0.f;               // sum of squares of the raw x this lane has split (first pass)
  float rs = 1.f;               // threads of the epilogue: the row scale of their row

  __device__ __forceinline__ F32Body(const F32Params& pp, float* red_, float* sq_) : p(pp), red(red_), sq_sh(sq_) {
    tid = threadIdx.x; lane = tid & 63; wave = __builtin_amdgcn_readfirstlane(tid >> 6); c16 = lane & 15; g = lane >> 4;
    G = gridDim.x; w = blockIdx.x;
    ntiles_all = p.N / 16;
    ntiles = w < ntiles_all ? (ntiles_all - w + G - 1) / G : 0;
    nkb = p.K / 32;
    nchunks = (nkb + F32_KB - 1) / F32_KB;
    norm = p.pro == PRO_NORM;
    xoff = ((uint32_t)min(c16 & 7, p.M - 1) * (uint32_t)p.ldx + 8u * g) * 4u;      // (<= 8 rows: far below 4 GiB)
    noff = 32u * g;
  }

  __device__ __forceinline__ int tile_of(int i) const { return min(w + i * G, ntiles_all - 1); }

  // STRAIGHT-LINE (gemv_phase.h issue_u): an invalid slot re-loads block 0 of this workgroup's first tile
  __device__ __forceinline__ void issue(int slot, int i, int kb, bool valid) {
    const int t = valid ? tile_of(i) : w, b = valid ? kb : 0;
    // a uniform 64-bit tile base plus a 32-bit lane offset (a tile is K * 32 bytes): no per-position address registers
    const gptr tb = uniform_ptr(p.w, ((size_t)t * nkb + b) * 1024);
    ring[slot] = __builtin_nontemporal_load((gptr16)(tb + (uint32_t)lane * 16u));
  }

  // the x (and norm weights) of this wave's block u of chunk c, into registers
  __device__ __forceinline__ void load_x(int c, int u) {
    const int kb = c * F32_KB + u * F32_NW + wave;
    const int k = kb < nkb ? kb * 32 : 0;
    const gptr xb = uniform_ptr(p.x, (size_t)k * 4);
    const gptr nb = uniform_ptr(norm ? p.norm_w : p.x, (size_t)k * 4);
    xr[u][0] = *(gptr16)(xb + xoff);
    xr[u][1] = *(gptr16)(xb + xoff + 16u);
    nr[u][0] = *(gptr16)(nb + noff);
    nr[u][1] = *(gptr16)(nb + noff + 16u);
  }

  // registers -> (x * w_norm) -> hi / mid / lo -> the two A-fragment images of this lane for block u of chunk c.
  // `count`: the squares of the raw x go to the row sums
  __device__ __forceinline__ void split_x(int c, int u, bool count) {
    const bool low = c16 < 8;
    const int kb = c * F32_KB + u * F32_NW + wave;
    const uint32_t xd[8] = {xr[u][0].x, xr[u][0].y, xr[u][0].z, xr[u][0].w, xr[u][1].x, xr[u][1].y, xr[u][1].z, xr[u][1].w};
    const uint32_t nd[8] = {nr[u][0].x, nr[u][0].y, nr[u][0].z, nr[u][0].w, nr[u][1].x, nr[u][1].y, nr[u][1].z, nr[u][1].w};
    uint32_t a0[4], a1[4];
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x2 f = {__uint_as_float(xd[2 * j]), __uint_as_float(xd[2 * j + 1])};
      if (norm) {
        const f32x2 wf = {__uint_as_float(nd[2 * j]), __uint_as_float(nd[2 * j + 1])};
        sq = fmaf(f.x, f.x, sq); sq = fmaf(f.y, f.y, sq);
        f = f * wf;
      }
      split3(f, low, a0[j], a1[j]);
    }
    af[u][0] = u32x4{a0[0], a0[1], a0[2], a0[3]};
    af[u][1] = u32x4{a1[0], a1[1], a1[2], a1[3]};
    if (count && kb < nkb) ss += sq;
  }

  // One pass: tiles i0 .. i0 + NT - 1 of this workgroup over all of K.  `preloaded`: the previous pass has issued this
  // pass's first D loads and split its first chunk's x; `roll`: this pass does so for the next one (both have 8 tiles).
  template <int NT>
  __device__ __forceinline__ void pass(int i0, bool preloaded, bool roll, bool first) {
    constexpr int L = NT * F32_UB, D = f32_depth(NT);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!preloaded) {
#pragma unroll
      for (int s = 0; s < D; ++s) {
        const int kb = (s % F32_UB) * F32_NW + wave;
        issue(s, i0 + s / F32_UB, kb, kb < nkb);
      }
#pragma unroll
      for (int u = 0; u < F32_UB; ++u) load_x(0, u);
#pragma unroll
      for (int u = 0; u < F32_UB; ++u) split_x(0, u, first);
    }
    for (int c = 0; c < nchunks; ++c) {
      const bool last = c + 1 == nchunks;
      const int nc = last ? 0 : c + 1;
      const bool have_next = !last || roll;
      // The next chunk's x.  Block u's fragments are last used at position L - 4 + u: they are replaced right there, from
      // registers fetched XD positions earlier (an L2 round trip), so at most two blocks' raw x are live at a time.
      // In the last chunk of a pass that does not roll (`last && !roll`) chunk 0's x is fetched and split all the same, unused:
      // deliberate straight-line filler like the invalid weight slots (8 cached loads and 4 splits per wave at the tail of
      // the pass; `count` is false, so the row sums are not touched) -- a branch around the loads would drain the queue.
      constexpr int XD = 2;
#pragma unroll
      for (int u = 0; u < F32_UB; ++u)
        if (L - F32_UB + u - XD < 0) load_x(nc, u);           // (a pass of one tile: no earlier position)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int u = 0; u < F32_UB; ++u) {
          const int pos = t * F32_UB + u, slot = pos % D;
          if (c * F32_KB + u * F32_NW + wave < nkb) {       // (wave-uniform; no load inside)
            acc[t] = mfma16<bf16>(af[u][0], ring[slot], acc[t]);
            acc[t] = mfma16<bf16>(af[u][1], ring[slot], acc[t]);
          }
          __builtin_amdgcn_sched_barrier(0);
          // the same registers are re-loaded with the load D positions ahead in this workgroup's sequence
          const int q = pos + D;
          if (q < L) {
            const int kb = c * F32_KB + (q % F32_UB) * F32_NW + wave;
            issue(slot, i0 + q / F32_UB, kb, kb < nkb);
          } else {
            const int q2 = q - L;
            const int kb = nc * F32_KB + (q2 % F32_UB) * F32_NW + wave;
            issue(slot, (last ? i0 + NT : i0) + q2 / F32_UB, kb, have_next && kb < nkb);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (pos >= L - F32_UB) split_x(nc, pos - (L - F32_UB), first && !last);
          if (pos + XD >= L - F32_UB && pos + XD < L) load_x(nc, pos + XD - (L - F32_UB));
        }
      }
    }

    // ---- cross-wave reduction.  Lane (c16, g) holds D rows 4 g + r: rows 0..7 (hi and lo products) in g < 2, rows
    // 8..15 (mid products) in g >= 2 -- added here, lanes 0..31 publish y[m = 4 (lane >> 4) + r][n = lane & 15]
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 v = acc[t];
      v.x += __shfl_xor(v.x, 32); v.y += __shfl_xor(v.y, 32); v.z += __shfl_xor(v.z, 32); v.w += __shfl_xor(v.w, 32);
      if (lane < 32) *(f32x4*)&red[((t * F32_NW + wave) * 32 + lane) * 4] = v;
    }
    if (first && norm) {
      float v = ss;                               // lanes c16 < 8: row c16, the four k-groups of the wave's blocks
      v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
      if (lane < 8) sq_sh[wave * 8 + lane] = v;
    }
    __syncthreads();
    // thread (t, m, c): columns c and c + 8 of row m of tile t
    const int t = tid >> 6, m = (tid >> 3) & 7, cc = tid & 7;
    if (first && norm) {
      float tot = 0.f;
#pragma unroll
      for (int ww = 0; ww < F32_NW; ++ww) tot += sq_sh[ww * 8 + m];
      rs = 1.0f / sqrtf(tot / (float)p.K + p.eps);
    }
    if (t < NT && m < p.M) {
      const int el = (m >> 2) * 16 + cc, r = m & 3;
      float y0 = 0.f, y1 = 0.f;
#pragma unroll
      for (int ww = 0; ww < F32_NW; ++ww) {
        y0 += red[((t * F32_NW + ww) * 32 + el) * 4 + r];
        y1 += red[((t * F32_NW + ww) * 32 + el + 8) * 4 + r];
      }
      y0 *= rs; y1 *= rs;
      const int tile = w + (i0 + t) * G;          // (t < NT: one of this workgroup's tiles)
      if constexpr (GU8) {
        // row-interleaved gate|up tile: columns 0..7 are gate rows 8 tile .. + 7, columns 8..15 the matching up rows
        const float sig = 1.0f / (1.0f + expf(-y0));
        const float sl = y0 * sig;
        p.out[(size_t)m * p.ldo + tile * 8 + cc] = sl * y1;
      } else {
        const size_t o = (size_t)m * p.ldo + tile * 16 + cc;
        if (p.epi == EPI_RESID) {
          const float h0 = p.resid[o], h1 = p.resid[o + 8];
          p.resid[o] = h0 + y0; p.resid[o + 8] = h1 + y1;
        } else {                                  // EPI_STORE and EPI_STORE_F32 coincide
          p.out[o] = y0; p.out[o + 8] = y1;
        }
      }
    }
  }

  __device__ __forceinline__ void run() {
    int done = 0;
    bool pre = false;
    while (done < ntiles) {
      const int nt = min(F32_TP, ntiles - done);
      const bool roll = nt == F32_TP && ntiles - done - nt >= F32_TP;
      const bool first = done == 0;
      if (done > 0) __syncthreads();              // `red` is reused
      switch (nt) {
        case 8: pass<8>(done, pre, roll, first); break;
        case 7: pass<7>(done, false, false, first); break;
        case 6: pass<6>(done, false, false, first); break;
        case 5: pass<5>(done, false, false, first); break;
        case 4: pass<4>(done, false, false, first); break;
        case 3: pass<3>(done, false, false, first); break;
        case 2: pass<2>(done, false, false, first); break;
        default: pass<1>(done, false, false, first); break;
      }
      pre = roll;
      done += nt;
    }
  }
};

__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_kernel(F32Params p) {
  __shared__ __attribute__((aligned(16))) float red[F32_TP * F32_NW * 32 * 4];
  __shared__ float sq_sh[F32_NW * 8];
  F32Body<false> b(p, red, sq_sh);
  b.run();
}

// The same stream under its own symbol for the launches on a row-interleaved gate|up copy (EPI_SWIGLU_GU8, float32
// SwiGLU in the epilogue): the dominant kernel of a float32-KV decode step keeps a name of its own in traces.
__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_gu8_kernel(F32Params p) {
  __shared__ __attribute__((aligned(16))) float red[F32_TP * F32_NW * 32 * 4];
  __shared__ float sq_sh[F32_NW * 8];
  F32Body<true> b(p, red, sq_sh);
  b.run();
}

// ---- The whole-K form: one 16-row tile per workgroup, K <= 4096, every byte of the launch requested up front --------------
// A narrow linear (N / 16 <= CUs: o_proj) has one tile per CU, and at K <= 4096 a wave's share of it is at most 16 k-blocks
// -- the 16 loads a wave of the kernel above keeps in flight.  So there is no ring and no chunk: wave v issues the loads of
// ALL its blocks v, v + 8, v + 16, ... at once (128 KiB per CU at K = 4096), multiplies them in ascending order as they
// land, and the workgroup ends in the reduction and epilogue of F32Body::pass<1>.  Same splits (split3), same MFMAs in the
// same order, same sums: every output is bit-identical to gemv_f32_kernel on the same call.
//
// Program order, straight-line (no load under a branch; a slot past the wave's last block re-loads a valid block and is
// ignored).  A CU returns loads in issue order, so what a block's MFMAs need is asked for in the order they need it:
//   * EPI_RESID: the two h values of each epilogue thread (only this workgroup writes them in this launch), first -- two
//     4-byte loads, out of the way before the stream.
//   * then PER BLOCK, x and right behind it the block's weights: x0 w0 x1 w1 ... x15 w15.
//     x: M rows x K floats, once per workgroup, 16 bytes per thread and load.  Lane l of wave v takes row l & 7, piece
//     l >> 3 (4 floats) of the block: a wave-load covers one 128-byte line of each of the 8 rows, and wave v stages
//     exactly the blocks it multiplies -- x crosses lanes (through LDS), never waves, so there is no workgroup barrier
//     between x and the MFMAs.  (Fewer than 8 rows: the lanes of the missing rows re-load the last row into an image row
//     that is never read.)
//     weights: non-temporal, uniform 64-bit base + 32-bit lane offset (uniform_ptr).
//     All of x in front of all the weights (the first form built) was measured and is slower in the step: 11.17 against
//     10.58 us per launch (traces of two boxes), 0.051-0.058 against 0.082 ms per step in the A/B.  The
//     reasoning behind the interleaved order, an estimate that no stamp backs: 128 x-loads per CU at 16 cycles each on
//     the CU's address path are ~0.85 us before the first weight request leaves, and HBM idles meanwhile; interleaved,
//     the first weight request leaves behind ONE x load, x (an L2 hit) is back long before the weights in front of it,
//     and the in-order return hands every block its x just ahead of its weights.  Back to back, with the matrix
//     resident in the Infinity Cache, the order is the other way round (9.7 against 10.0 us), and the step is what counts.
// Then per block, as its loads land (counted vmcnt: 31, 30, ... 0): x -> LDS -> the lane's fragment position -> split ->
// two MFMAs.  The LDS round trip and the split of block u run while block u's weights are still on their way.
//
// LDS image of x, float32, in fragment order: k-block kb is one KiB, [half h of the 8 floats][lane group g][row m] x 16
// bytes.  A store (8 consecutive lanes = the 8 rows of one piece) fills 128 contiguous bytes; a fragment read
// (ds_read_b128: 16-lane groups that span two g and all rows; lanes c16 and c16 + 8 share an address) covers 256
// contiguous bytes: neither has a bank conflict.  The raw x of all 16 blocks is in registers as loaded (64 VGPRs, next to
// the 64 of the weights: everything is in flight at once); a block's pieces leave for LDS as they land, and only ONE block's
// fragment position is read back and split at a time: never 16 blocks of split fragments.
//
// Resources: 512 threads, 155 VGPRs, one workgroup per CU, no scratch.  LDS (dynamic, above 64 KiB -> function attribute):
// the 4-KiB reduction + K / 32 KiB of x (at least one block per wave, so that the ignored slots stay inside it): 132 KiB
// at K = 4096.
constexpr int F32W_UB = 16;                      // k-blocks per wave: K <= 8 * 16 * 32
constexpr int F32W_RED = F32_NW * 32 * 16;       // bytes of the cross-wave reduction, in front of the x image
constexpr size_t f32_whole_lds_bytes(int K) { return F32W_RED + (size_t)(K / 32 > F32_NW ? K / 32 : F32_NW) * 1024; }

__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_whole_kernel(F32Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char whole_lds[];
  float* red = (float*)whole_lds;
  unsigned char* ximg = whole_lds + F32W_RED;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c16 = lane & 15, g = lane >> 4;
  const int w = blockIdx.x, nkb = p.K / 32;

  // (b) thread (m, c) of wave 0 finishes columns c and c + 8 of row m (F32Body::pass): its h now, not as a dependent load
  // at the very end.  Straight-line: the pointer is selected, the load is not under a branch.
  const int em = (tid >> 3) & 7, ecc = tid & 7;
  const bool ep = tid < 64 && em < p.M;
  const bool res = ep && p.epi == EPI_RESID;
  const size_t eo = (size_t)em * p.ldo + w * 16 + ecc;
  const float* hp = res ? p.resid + eo : p.x;
  const float h0 = hp[0], h1 = hp[res ? 8 : 0];
  __builtin_amdgcn_sched_barrier(0);
  // (a), (c) per block: its x -- row lane & 7 (clamped), 16-byte piece lane >> 3 of the block's 128 bytes per row -- then its weights
  u32x4 xs[F32W_UB], ring[F32W_UB];
  const uint32_t xlane = ((uint32_t)min(lane & 7, p.M - 1) * (uint32_t)p.ldx + 4u * (lane >> 3)) * 4u;   // (<= 8 rows: far below 4 GiB)
#pragma unroll
  for (int u = 0; u < F32W_UB; ++u) {
    const int kb = u * F32_NW + wave, b = kb < nkb ? kb : 0;
    const gptr xb = uniform_ptr(p.x, (size_t)b * 128);
    xs[u] = *(gptr16)(xb + xlane);
    __builtin_amdgcn_sched_barrier(0);
    const gptr tb = uniform_ptr(p.w, ((size_t)w * nkb + b) * 1024);
    ring[u] = __builtin_nontemporal_load((gptr16)(tb + (uint32_t)lane * 16u));
    __builtin_amdgcn_sched_barrier(0);
  }

  // Per block, as its loads land: x -> LDS image (wave-uniform branch, no load inside) -> this lane's fragment position ->
  // split -> two MFMAs.  The image rows a wave reads are the ones it wrote, and the LDS operations of a wave complete in order.
  const uint32_t wofs = (uint32_t)(((lane >> 3) & 1) * 512 + ((lane >> 4) * 8 + (lane & 7)) * 16);
  const uint32_t rofs = (uint32_t)((g * 8 + min(c16 & 7, p.M - 1)) * 16);
  const bool low = c16 < 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < F32W_UB; ++u) {
    const int kb = u * F32_NW + wave;
    const bool valid = kb < nkb;                    // (wave-uniform)
    // a slot past the end reads the wave's own first image block (inside the allocation, written by no other wave)
    unsigned char* blk = ximg + (valid ? kb : wave) * 1024;
    if (valid) *(u32x4*)(blk + wofs) = xs[u];
    __builtin_amdgcn_wave_barrier();
    const u32x4 r0 = *(const u32x4*)(blk + rofs), r1 = *(const u32x4*)(blk + rofs + 512);
    const uint32_t xd[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    uint32_t a0[4], a1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(f32x2{__uint_as_float(xd[2 * j]), __uint_as_float(xd[2 * j + 1])}, low, a0[j], a1[j]);
    if (valid) {
      acc = mfma16<bf16>(u32x4{a0[0], a0[1], a0[2], a0[3]}, ring[u], acc);
      acc = mfma16<bf16>(u32x4{a1[0], a1[1], a1[2], a1[3]}, ring[u], acc);
    }
  }

  // ---- cross-wave reduction and epilogue: F32Body::pass<1>, tile 0
  f32x4 v = acc;
  v.x += __shfl_xor(v.x, 32); v.y += __shfl_xor(v.y, 32); v.z += __shfl_xor(v.z, 32); v.w += __shfl_xor(v.w, 32);
  if (lane < 32) *(f32x4*)&red[(wave * 32 + lane) * 4] = v;
  __syncthreads();
  if (ep) {
    const int el = (em >> 2) * 16 + ecc, r = em & 3;
    float y0 = 0.f, y1 = 0.f;
#pragma unroll
    for (int ww = 0; ww < F32_NW; ++ww) {
      y0 += red[(ww * 32 + el) * 4 + r];
      y1 += red[(ww * 32 + el + 8) * 4 + r];
    }
    if (p.epi == EPI_RESID) {
      p.resid[eo] = h0 + y0; p.resid[eo + 8] = h1 + y1;
    } else {                                        // EPI_STORE and EPI_STORE_F32 coincide
      p.out[eo] = y0; p.out[eo + 8] = y1;
    }
  }
}

// ---- The resident form: the stream of F32Body with x and the norm weights kept in LDS for the whole launch -----------------
// The chunked kernel above fetches a chunk's x from L2 while the weights stream, and a wave's loads return in issue order:
// the wait for the next chunk's x (vmcnt(8) where the steady state is vmcnt(D - 1)) is also a wait for all but one or two
// of the wave's weight loads.  All eight waves of all workgroups reach their chunk ends together, so the chip's request
// queue runs dry once per chunk.  Here the head stages x ONCE -- wave v exactly the k-blocks v, v + 8, ... that it multiplies,
// through the float32 fragment-order image of gemv_f32_whole_kernel (1 KiB per k-block; x crosses lanes, never waves: no
// workgroup barrier between x and the MFMAs) -- and, under PRO_NORM, the norm weights of the same blocks (128 bytes per
// k-block, read back as a broadcast).  From then on the only vector-memory loads of the stream are the non-temporal weight
// loads, and every wait in it is the counted vmcnt(D - 1) or higher.  A chunk's four fragment pairs are rebuilt from the
// images (four ds_read_b128 and the split of split_x per block) where split_x stands in the chunked kernel; the reads are
// issued in front of the position's MFMAs, which cover their latency.
//
// Same tile deal, passes, block ownership, split3 on x * w_norm, MFMAs in the same order, the same fmaf chain for the squares
// added in the same (chunk, block) order, the same cross-wave sums and epilogues: every output is bit-identical to
// gemv_f32_kernel / gemv_f32_gu8_kernel on the same call.
//
// Head (first pass), straight-line, nothing under a branch, neither a load nor a staging store: the norm weights (two
// 16-byte loads per lane cover the wave's 16 blocks; without PRO_NORM they read x and are ignored), x0 w0 x1 w1 x2 w2 x3 w3,
// x4 .. x15, then w4 .. w(D-1); slots past the end re-load block 0.  The first D weight loads with ALL the remaining x behind
// them (the first order built) make the wait for the last x load a wait for every weight load of the head: each wave, and
// so the chip, started the stream with an empty ring, and that form gained 0.014 / 0.020 ms per step in two A/B jobs where
// this one gains 0.059.  In this order the staging waits for w0 .. w3 only (vmcnt(D - 4)).  The first pass is
// an instantiation of its own in front of the loop over the later ones (see pass()).  Later passes never stage again: x
// survives in LDS.
//
// LDS (dynamic, one workgroup per CU): [row sums 256 B][reduction 8 KiB][x image K / 32 KiB][norm image K / 256 KiB], the
// images at least 8 blocks (one per wave, so that ignored slots stay inside them), and below K = 4096 one KiB per wave that
// takes the staging stores of blocks past the end: 152.25 KiB at K = 4096.  The 32-KiB reduction buffer of the chunked
// kernel does not fit next to the images, so a full pass (8 tiles) with another pass behind it reduces 2 tiles per round
// through the 8-KiB buffer.  After the workgroup's LAST pass -- every pass of fewer than 8 tiles is one (run(): nt < 8 only
// when nothing is left), and so is a full pass with nothing behind it -- nobody reads the images: behind a barrier its
// reduction takes 4 KiB per tile from the start of the buffer on into the x image, in one round as in the chunked kernel
// (the allocation is at least 32 KiB + 256 B).  Either way the sums are taken wave 0 .. 7 in order.
constexpr int F32R_UB = 16;                      // k-blocks per wave: K <= 8 * 16 * 32
constexpr int F32R_SQ = F32_NW * 8 * 4;          // bytes of the waves' row sums, at the start
constexpr int F32R_RED = 2 * F32_NW * 32 * 16;   // bytes of the 2-tile reduction buffer
constexpr size_t F32R_LDS_MAX = 160 * 1024;      // gfx950: LDS per CU
constexpr int f32_res_blocks(int K) { return K / 32 > F32_NW ? K / 32 : F32_NW; }
constexpr size_t f32_res_dump_bytes(int K) { return K / 32 < F32_NW * F32R_UB ? F32_NW * 1024 : 0; }   // (see stage())
constexpr size_t f32_res_lds_bytes(int K) {
  const size_t img = (size_t)F32R_RED + (size_t)f32_res_blocks(K) * (1024 + 128) + f32_res_dump_bytes(K);
  return F32R_SQ + (img > 32 * 1024 ? img : 32 * 1024);
}

template <bool GU8>
struct F32Resident : F32Body<GU8> {
  using B = F32Body<GU8>;
  using B::p; using B::red; using B::sq_sh; using B::tid; using B::lane; using B::wave; using B::c16; using B::g;
  using B::G; using B::w; using B::ntiles; using B::nkb; using B::nchunks; using B::norm;
  using B::ring; using B::acc; using B::af; using B::ss; using B::rs;
  unsigned char* ximg; unsigned char* nimg;
  uint32_t rofs;                // bytes from a block of the x image to this lane's fragment position (second half: + 512)

  __device__ __forceinline__ F32Resident(const F32Params& pp, unsigned char* lds)
      : B(pp, (float*)(lds + F32R_SQ), (float*)lds) {
    ximg = lds + F32R_SQ + F32R_RED;
    nimg = ximg + (size_t)f32_res_blocks(p.K) * 1024;
    rofs = (uint32_t)((g * 8 + min(c16 & 7, p.M - 1)) * 16);
  }

  // The head of the first pass: the norm weights, the first four weight loads with the x of their blocks in front of each,
  // the rest of x, the rest of the first D weight loads; then x and the norm weights into their images.  STRAIGHT-LINE.
  // A wave's loads return in issue order, so the wait for the last x load is a wait for w0 .. w3 only: the other D - 4
  // weight loads stay in flight across the staging, and the stream does not start with an empty ring.
  template <int D>
  __device__ __forceinline__ void stage(int i0) {
    u32x4 xs[F32R_UB], ns[2];
    const uint32_t xlane = ((uint32_t)min(lane & 7, p.M - 1) * (uint32_t)p.ldx + 4u * (lane >> 3)) * 4u;   // (<= 8 rows: far below 4 GiB)
    auto load_xs = [&](int u) {
      const int kb = u * F32_NW + wave, b = kb < nkb ? kb : 0;
      const gptr xb = uniform_ptr(p.x, (size_t)b * 128);
      xs[u] = *(gptr16)(xb + xlane);
    };
    auto issue_w = [&](int s) {
      const int kb = (s % F32_UB) * F32_NW + wave;
      B::issue(s, i0 + s / F32_UB, kb, kb < nkb);
    };
    // lane l: 32 bytes (piece l & 3) of the norm weights of the wave's block l >> 2
    const int nkbl = (lane >> 2) * F32_NW + wave;
    const bool nvalid = nkbl < nkb;
    const gptr nb = uniform_ptr(norm ? p.norm_w : p.x, 0);
    const uint32_t nlane = (uint32_t)(nvalid ? nkbl : 0) * 128u + (uint32_t)(lane & 3) * 32u;
    ns[0] = *(gptr16)(nb + nlane);
    ns[1] = *(gptr16)(nb + nlane + 16u);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < F32_UB; ++s) {            // (D >= 4 for every pass size)
      load_xs(s);
      __builtin_amdgcn_sched_barrier(0);
      issue_w(s);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = F32_UB; u < F32R_UB; ++u) load_xs(u);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = F32_UB; s < D; ++s) issue_w(s);
    __builtin_amdgcn_sched_barrier(0);
    // No store under a branch either: at the join behind a skipped store the compiler's wait for the skipped load's registers
    // came out as vmcnt(1) / vmcnt(0) in front of the first image reads -- the drain this form exists to remove.  A block past
    // the end (and the norm weights of one) goes to a KiB of the wave's own behind the images, which nobody reads; it is there
    // whenever a wave can have such a block (K < 4096).
    const uint32_t wofs = (uint32_t)(((lane >> 3) & 1) * 512 + ((lane >> 4) * 8 + (lane & 7)) * 16);
    unsigned char* dump = nimg + f32_res_blocks(p.K) * 128 + wave * 1024;
#pragma unroll
    for (int u = 0; u < F32R_UB; ++u) {
      const int kb = u * F32_NW + wave;
      *(u32x4*)((kb < nkb ? ximg + kb * 1024 : dump) + wofs) = xs[u];
    }
    unsigned char* d = nvalid ? nimg + nkbl * 128 + (lane & 3) * 32 : dump + (lane & 31) * 32;
    *(u32x4*)d = ns[0];
    *(u32x4*)(d + 16) = ns[1];
    __builtin_amdgcn_wave_barrier();              // the image blocks a wave reads are the ones it wrote, and its LDS operations complete in order
  }

  // this lane's raw x and norm weights of the wave's block u of chunk c, from the images (a block past the end reads the
  // wave's own first image block: inside the allocation, written by no other wave, never multiplied)
  __device__ __forceinline__ void read_img(int c, int u, u32x4 (&xr)[2], u32x4 (&nr)[2]) {
    const int kb = c * F32_KB + u * F32_NW + wave;
    const int b = kb < nkb ? kb : wave;
    const unsigned char* xb = ximg + b * 1024 + rofs;
    const unsigned char* nb = nimg + b * 128 + g * 32;
    xr[0] = *(const u32x4*)xb; xr[1] = *(const u32x4*)(xb + 512);
    nr[0] = *(const u32x4*)nb; nr[1] = *(const u32x4*)(nb + 16);
  }

  // F32Body::split_x on registers read from the images
  __device__ __forceinline__ void split_img(int c, int u, bool count, const u32x4 (&xr)[2], const u32x4 (&nr)[2]) {
    const bool low = c16 < 8;
    const int kb = c * F32_KB + u * F32_NW + wave;
    const uint32_t xd[8] = {xr[0].x, xr[0].y, xr[0].z, xr[0].w, xr[1].x, xr[1].y, xr[1].z, xr[1].w};
    const uint32_t nd[8] = {nr[0].x, nr[0].y, nr[0].z, nr[0].w, nr[1].x, nr[1].y, nr[1].z, nr[1].w};
    uint32_t a0[4], a1[4];
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x2 f = {__uint_as_float(xd[2 * j]), __uint_as_float(xd[2 * j + 1])};
      if (norm) {
        const f32x2 wf = {__uint_as_float(nd[2 * j]), __uint_as_float(nd[2 * j + 1])};
        sq = fmaf(f.x, f.x, sq); sq = fmaf(f.y, f.y, sq);
        f = f * wf;
      }
      split3(f, low, a0[j], a1[j]);
    }
    af[u][0] = u32x4{a0[0], a0[1], a0[2], a0[3]};
    af[u][1] = u32x4{a1[0], a1[1], a1[2], a1[3]};
    if (count && kb < nkb) ss += sq;
  }

  // the fragments of chunk 0
  __device__ __forceinline__ void rebuild0(bool count) {
#pragma unroll
    for (int u = 0; u < F32_UB; ++u) {
      u32x4 xr[2], nr[2];
      read_img(0, u, xr, nr);
      split_img(0, u, count, xr, nr);
    }
  }

  // F32Body::pass with the fragments rebuilt from LDS.  FIRST: this pass stages x and counts the squares (an instantiation of
  // its own, run in front of the loop over the later passes: inside that loop the compiler carries the previous pass's
  // ignored filler loads along as outstanding, and the waits it then put behind the staging -- vmcnt(1), vmcnt(0) -- drained
  // the ring that the head had just filled); `final`: it is the workgroup's last.
  template <int NT, bool FIRST>
  __device__ __forceinline__ void pass(int i0, bool preloaded, bool roll, bool final) {
    constexpr bool first = FIRST;
    constexpr int L = NT * F32_UB, D = f32_depth(NT);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!preloaded) {
      if constexpr (FIRST) {
        stage<D>(i0);
        rebuild0(true);
      } else {
#pragma unroll
        for (int s = 0; s < D; ++s) {
          const int kb = (s % F32_UB) * F32_NW + wave;
          B::issue(s, i0 + s / F32_UB, kb, kb < nkb);
        }
        rebuild0(false);
      }
    }
    for (int c = 0; c < nchunks; ++c) {
      const bool last = c + 1 == nchunks;
      const int nc = last ? 0 : c + 1;
      const bool have_next = !last || roll;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int u = 0; u < F32_UB; ++u) {
          const int pos = t * F32_UB + u, slot = pos % D;
          // Block u's fragments are last used at position L - 4 + u and replaced right there by the next chunk's, read from
          // the images in front of the MFMAs.  In the last chunk of a pass that does not roll, chunk 0's are rebuilt, unused
          // (straight-line filler as in F32Body::pass; `count` is false).
          u32x4 xr[2], nr[2];
          if (pos >= L - F32_UB) read_img(nc, pos - (L - F32_UB), xr, nr);
          if (c * F32_KB + u * F32_NW + wave < nkb) {       // (wave-uniform; no load inside)
            acc[t] = mfma16<bf16>(af[u][0], ring[slot], acc[t]);
            acc[t] = mfma16<bf16>(af[u][1], ring[slot], acc[t]);
          }
          __builtin_amdgcn_sched_barrier(0);
          // the same registers are re-loaded with the load D positions ahead in this workgroup's sequence
          const int q = pos + D;
          if (q < L) {
            const int kb = c * F32_KB + (q % F32_UB) * F32_NW + wave;
            B::issue(slot, i0 + q / F32_UB, kb, kb < nkb);
          } else {
            const int q2 = q - L;
            const int kb = nc * F32_KB + (q2 % F32_UB) * F32_NW + wave;
            B::issue(slot, (last ? i0 + NT : i0) + q2 / F32_UB, kb, have_next && kb < nkb);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (pos >= L - F32_UB) split_img(nc, pos - (L - F32_UB), first && !last, xr, nr);
        }
      }
    }

    // ---- cross-wave reduction and epilogue (see the notes above): the workgroup's last pass in one round over the images
    if constexpr (NT < F32_TP) {
      finish<NT, NT, true>(i0, first);
    } else {
      if (final) finish<NT, NT, true>(i0, first);
      else finish<NT, 2, false>(i0, first);
    }
  }

  // the cross-wave reduction and epilogue of F32Body::pass, TR tiles per round; OVER: `red` runs on into the images
  template <int NT, int TR, bool OVER>
  __device__ __forceinline__ void finish(int i0, bool first) {
    if (first && norm) {
      float v = ss;                               // lanes c16 < 8: row c16, the four k-groups of the wave's blocks
      v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
      if (lane < 8) sq_sh[wave * 8 + lane] = v;
    }
    // thread (t, m, c): columns c and c + 8 of row m of tile t of the round
    const int t = tid >> 6, m = (tid >> 3) & 7, cc = tid & 7;
#pragma unroll
    for (int r0 = 0; r0 < NT; r0 += TR) {
      if (OVER || r0 > 0) __syncthreads();        // the last pass: every wave is done with the images; a later round: with `red`
#pragma unroll
      for (int tl = 0; tl < TR; ++tl) {
        f32x4 v = acc[r0 + tl];
        v.x += __shfl_xor(v.x, 32); v.y += __shfl_xor(v.y, 32); v.z += __shfl_xor(v.z, 32); v.w += __shfl_xor(v.w, 32);
        if (lane < 32) *(f32x4*)&red[((tl * F32_NW + wave) * 32 + lane) * 4] = v;
      }
      __syncthreads();
      if (r0 == 0 && first && norm) {
        float tot = 0.f;
#pragma unroll
        for (int ww = 0; ww < F32_NW; ++ww) tot += sq_sh[ww * 8 + m];
        rs = 1.0f / sqrtf(tot / (float)p.K + p.eps);
      }
      if (t < TR && m < p.M) {
        const int el = (m >> 2) * 16 + cc, r = m & 3;
        float y0 = 0.f, y1 = 0.f;
#pragma unroll
        for (int ww = 0; ww < F32_NW; ++ww) {
          y0 += red[((t * F32_NW + ww) * 32 + el) * 4 + r];
          y1 += red[((t * F32_NW + ww) * 32 + el + 8) * 4 + r];
        }
        y0 *= rs; y1 *= rs;
        const int tile = w + (i0 + r0 + t) * G;     // (t < TR, r0 + t < NT: one of this workgroup's tiles)
        if constexpr (GU8) {
          // row-interleaved gate|up tile: columns 0..7 are gate rows 8 tile .. + 7, columns 8..15 the matching up rows
          const float sig = 1.0f / (1.0f + expf(-y0));
          const float sl = y0 * sig;
          p.out[(size_t)m * p.ldo + tile * 8 + cc] = sl * y1;
        } else {
          const size_t o = (size_t)m * p.ldo + tile * 16 + cc;
          if (p.epi == EPI_RESID) {
            const float h0 = p.resid[o], h1 = p.resid[o + 8];
            p.resid[o] = h0 + y0; p.resid[o + 8] = h1 + y1;
          } else {                                  // EPI_STORE and EPI_STORE_F32 coincide
            p.out[o] = y0; p.out[o + 8] = y1;
          }
        }
      }
    }
  }

  template <bool FIRST>
  __device__ __forceinline__ void pass_of(int nt, int i0, bool preloaded, bool roll, bool final) {
    switch (nt) {
      case 8: pass<8, FIRST>(i0, preloaded, roll, final); break;
      case 7: pass<7, FIRST>(i0, false, false, true); break;
      case 6: pass<6, FIRST>(i0, false, false, true); break;
      case 5: pass<5, FIRST>(i0, false, false, true); break;
      case 4: pass<4, FIRST>(i0, false, false, true); break;
      case 3: pass<3, FIRST>(i0, false, false, true); break;
      case 2: pass<2, FIRST>(i0, false, false, true); break;
      default: pass<1, FIRST>(i0, false, false, true); break;
    }
  }

  __device__ __forceinline__ void run() {
    if (ntiles <= 0) return;
    int done = min(F32_TP, ntiles);
    bool pre = done == F32_TP && ntiles - done >= F32_TP;
    pass_of<true>(done, 0, false, pre, done == ntiles);
    while (done < ntiles) {
      const int nt = min(F32_TP, ntiles - done);
      const bool roll = nt == F32_TP && ntiles - done - nt >= F32_TP;
      __syncthreads();                            // `red` is reused
      pass_of<false>(nt, done, pre, roll, done + nt == ntiles);
      pre = roll;
      done += nt;
    }
  }
};

__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_resident_kernel(F32Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_lds[];
  F32Resident<false> b(p, resident_lds);
  b.run();
}

// ... and under its own symbol for the gate|up launches, as gemv_f32_gu8_kernel
__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_resident_gu8_kernel(F32Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_lds[];
  F32Resident<true> b(p, resident_lds);
  b.run();
}

}  // namespace

// float32 activations without logical rounding, <= 8 rows, dense bf16 tile-major weights, no LoRA, no [hi | lo] walk;
// plain / residual stores and SwiGLU on the row-interleaved gate|up copy (EPI_SWIGLU_GU8: W is that copy, out has
// W.N / 2 columns).  EPI_SWIGLU on a plain gate|up matrix is NOT taken: the caller passes the interleaved copy.
bool gemv_f32_supported(const LinearW& W, const GemvCall& c) {
  if (c.force_v1 || W.layout != 1 || W.wk != WK_BF16) return false;
  if (c.act != MI_F32 || c.rnd != RND_NONE || c.kx != 0) return false;
  if (c.M < 1 || c.M > 8) return false;
  if (W.lora_b[0] != nullptr || W.lora_b[1] != nullptr || c.lora_t != nullptr) return false;
  if (W.bias != nullptr) return false;            // a biased linear runs on the split-K kernel (gemm_skinny.hip)
  if (W.K < 32 || W.K % 32 != 0 || W.N < 16 || W.N % 16 != 0 || c.ldx % 4 != 0) return false;
  if (c.pro != PRO_NONE && (c.pro != PRO_NORM || c.norm_w == nullptr)) return false;
  return c.epi == EPI_STORE || c.epi == EPI_STORE_F32 || c.epi == EPI_RESID || c.epi == EPI_SWIGLU_GU8;
}

int launch_gemv_f32(const LinearW& W, const GemvCall& c, hipStream_t st) {
  if (!gemv_f32_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "gemv_f32: call not supported by this kernel");
  F32Params p{};
  p.x = (const float*)c.x; p.ldx = c.ldx; p.M = c.M;
  p.pro = c.pro; p.norm_w = (const float*)c.norm_w; p.eps = c.eps;
  p.w = W.w; p.N = W.N; p.K = W.K;
  p.epi = c.epi; p.out = (float*)c.out; p.ldo = c.ldo; p.resid = (float*)c.resid;
  if (c.epi == EPI_RESID ? p.resid == nullptr : p.out == nullptr) return fail(MI_ERR_INVALID, "gemv_f32: output buffer missing");
  const int nwg = std::min(W.N / 16, gemv_cu_count());     // one workgroup per CU; tiles are dealt in-kernel
  if (c.epi == EPI_SWIGLU_GU8) hipLaunchKernelGGL(gemv_f32_gu8_kernel, dim3(nwg), dim3(F32_NW * 64), 0, st, p);
  else hipLaunchKernelGGL(gemv_f32_kernel, dim3(nwg), dim3(F32_NW * 64), 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// The whole-K form: what gemv_f32_supported takes, without a prologue, K <= 4096 (16 k-blocks per wave) and at most one
// tile per CU (the tile is the workgroup's only work: more tiles than CUs would queue whole workgroups behind one another)
bool gemv_f32_whole_supported(const LinearW& W, const GemvCall& c) {
  if (!gemv_f32_supported(W, c)) return false;
  if (c.pro != PRO_NONE) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID) return false;
  if (W.K > F32_NW * F32W_UB * 32) return false;
  return W.N / 16 <= gemv_cu_count();
}

int launch_gemv_f32_whole(const LinearW& W, const GemvCall& c, hipStream_t st) {
  if (!gemv_f32_whole_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "gemv_f32_whole: call not supported by this kernel");
  F32Params p{};
  p.x = (const float*)c.x; p.ldx = c.ldx; p.M = c.M;
  p.pro = PRO_NONE; p.norm_w = nullptr; p.eps = 0.f;
  p.w = W.w; p.N = W.N; p.K = W.K;
  p.epi = c.epi; p.out = (float*)c.out; p.ldo = c.ldo; p.resid = (float*)c.resid;
  if (c.epi == EPI_RESID ? p.resid == nullptr : p.out == nullptr) return fail(MI_ERR_INVALID, "gemv_f32_whole: output buffer missing");
  // the opt-in for LDS above 64 KiB belongs to the kernel object of the CURRENT device: one flag per device, set after the call
  static std::atomic<bool> attr_done[64];
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_done[dev].load(std::memory_order_acquire)) {
    MI_HIP(hipFuncSetAttribute((const void*)gemv_f32_whole_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)f32_whole_lds_bytes(F32_NW * F32W_UB * 32)));
    if (dev >= 0 && dev < 64) attr_done[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(gemv_f32_whole_kernel, dim3(W.N / 16), dim3(F32_NW * 64), f32_whole_lds_bytes(W.K), st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// The resident form: what gemv_f32_supported takes, with at most 16 k-blocks per wave (K <= 4096: the head holds a wave's
// raw x in registers at once) and the images and the reduction buffer inside a CU's LDS
bool gemv_f32_resident_supported(const LinearW& W, const GemvCall& c) {
  if (!gemv_f32_supported(W, c)) return false;
  if (W.K > F32_NW * F32R_UB * 32) return false;
  return f32_res_lds_bytes(W.K) <= F32R_LDS_MAX;
}

int launch_gemv_f32_resident(const LinearW& W, const GemvCall& c, hipStream_t st) {
  if (!gemv_f32_resident_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "gemv_f32_resident: call not supported by this kernel");
  F32Params p{};
  p.x = (const float*)c.x; p.ldx = c.ldx; p.M = c.M;
  p.pro = c.pro; p.norm_w = (const float*)c.norm_w; p.eps = c.eps;
  p.w = W.w; p.N = W.N; p.K = W.K;
  p.epi = c.epi; p.out = (float*)c.out; p.ldo = c.ldo; p.resid = (float*)c.resid;
  if (c.epi == EPI_RESID ? p.resid == nullptr : p.out == nullptr) return fail(MI_ERR_INVALID, "gemv_f32_resident: output buffer missing");
  // the opt-in for LDS above 64 KiB belongs to the kernel objects of the CURRENT device: one flag per device, set after the calls
  static std::atomic<bool> attr_done[64];
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_done[dev].load(std::memory_order_acquire)) {
    const int most = (int)f32_res_lds_bytes(F32_NW * F32R_UB * 32);
    MI_HIP(hipFuncSetAttribute((const void*)gemv_f32_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most));
    MI_HIP(hipFuncSetAttribute((const void*)gemv_f32_resident_gu8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most));
    if (dev >= 0 && dev < 64) attr_done[dev].store(true, std::memory_order_release);
  }
  const int nwg = std::min(W.N / 16, gemv_cu_count());     // one workgroup per CU; tiles are dealt in-kernel
  const size_t lds = f32_res_lds_bytes(W.K);
  if (c.epi == EPI_SWIGLU_GU8) hipLaunchKernelGGL(gemv_f32_resident_gu8_kernel, dim3(nwg), dim3(F32_NW * 64), lds, st, p);
  else hipLaunchKernelGGL(gemv_f32_resident_kernel, dim3(nwg), dim3(F32_NW * 64), lds, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
