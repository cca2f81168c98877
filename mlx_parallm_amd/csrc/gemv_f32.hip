// gemv_f32.hip -- one-pass weight-streaming GEMV for FLOAT32 activations, <= 8 rows, on dense bf16 weights in the
// tile-major layout (repack.hip): gate|up, lm_head and o_proj of a decode step in the float32-KV ("PagedKVCache") mode of
// a bf16 model.  q|k|v and down_proj stay on the split-K kernel (gemm_skinny.hip).
//
// Same operator and the same arithmetic contract as skinny_kernel<.., X32> (gemm_skinny.hip): x = hi + mid + lo exactly
// (three bf16 terms), every product exact in the float32 accumulator -- a float32 dot product in another summation
// order; outputs float32, no logical rounding.  The launch has the shape of gemv_mfma.hip.  Three forms, ONE set of parts:
//
//   chunked   gemv_f32{,_gu8}_kernel            any K; a chunk's x comes from L2 through registers (F32Body).  The yardstick.
//   whole-K   gemv_f32_whole_kernel             K <= 4096, one tile per CU (o_proj): no ring, every load up front
//   resident  gemv_f32_resident{,_gu8}_kernel   K <= 4096; x and the norm weights stay in LDS (F32Resident): what gate|up
//                                               and lm_head of Mistral-7B run on
//
// All three split x in split8, fetch weights in load_w, sum the waves in publish / sum_waves and address outputs in out_ofs;
// the chunked and the resident stream share F32Body's position (step), reduction and epilogue (finish, store_out) and pass
// dispatch (with_pass_size); the two LDS forms share the x image (ximg_*).  So they split, multiply and sum alike by
// construction, and every output of every form is bit-identical to gemv_f32_kernel on the same call.  What follows is the
// stream of F32Body; the notes of the other two forms are in front of them.
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
//     the chunked form: a wave's loads return in issue order, and split_x of the next chunk needs x that was requested two
//     positions earlier, behind all but one or two of the wave's weight loads -- the compiler's wait there is vmcnt(8), with
//     12 x / norm-weight loads younger than the weights it lets through.  The wave stands for about a memory round trip with
//     its ring nearly empty, and all waves of all workgroups reach their chunk ends together (the wait sequences: DESIGN §8d).
//     The resident form takes x out of the vector-memory queue of the loop.
//   * RMSNorm (PRO_NORM) is deferred and local: x is multiplied by the norm weight while it is split, the squares of the
//     raw x are summed on the way (first pass only: each element once per launch), and rs[m] = rsqrt(mean + eps) scales
//     the dot product in the epilogue.  Every workgroup sees all of x, so it owns the complete row sums.  In float32
//     this differs from w * (x * rs) by one rounding per element (~6e-8), as `defer_norm` in gemm_skinny.hip.
//
// Every load is addressed as a wave-uniform 64-bit base plus a 32-bit lane offset: with one 64-bit address pair per load
// position the loop spilled, and a spill reload drains the prefetch queue.
//
// Resources of the chunked form: 512 threads, 255 VGPRs (one workgroup per CU), no scratch.  LDS: 32.5 KiB static -- the
// cross-wave reduction of a pass ([8 tiles][8 waves][32 lanes] float4 = 32 KiB, written once per pass after the last chunk)
// and the waves' row sums of squares (8 x 8 floats).
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
constexpr int F32_LB = 16;                      // k-blocks per wave of the forms that hold a wave's x at once: K <= 8 * 16 * 32

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

// this lane's 16 bytes of the 1-KiB block (tile t, k-block kb) of W, non-temporal (a tile is K * 32 bytes)
__device__ __forceinline__ u32x4 load_w(const void* w, int t, int kb, int nkb, int lane) {
  const gptr tb = uniform_ptr(w, ((size_t)t * nkb + kb) * 1024);
  return __builtin_nontemporal_load((gptr16)(tb + (uint32_t)lane * 16u));
}

// Two floats -> hi + mid + lo exactly (three bf16 terms each) -> one dword of a lane's two A-fragment images: `low` lanes
// (fragment rows 0..7) hold hi and lo, the others mid and zeros.
__device__ __forceinline__ void split3(f32x2 f, bool low, uint32_t& a0, uint32_t& a1) {
  const uint32_t hi = pack2<bf16>(f);
  const f32x2 r1 = f - unpack2<bf16>(hi);
  const uint32_t mid = pack2<bf16>(r1);
  const uint32_t lo = pack2<bf16>(r1 - unpack2<bf16>(mid));
  a0 = low ? hi : mid;
  a1 = low ? lo : 0u;
}

// THE split of this file.  The 8 floats of a lane's A-fragment position of one k-block (two registers of raw x and, under
// `norm`, two of the norm weights of its columns) -> (x * w_norm) -> hi / mid / lo -> the lane's two fragment images `a`.
// `add`: the fmaf chain of the squares of the raw x goes to ss.  (The sum stays in here: handed back to the caller for the
// add, the same arithmetic compiled to another schedule of the chunked kernels, with spills.)
__device__ __forceinline__ void split8(const u32x4 (&x)[2], const u32x4 (&n)[2], bool norm, bool low, u32x4 (&a)[2], bool add, float& ss) {
  const uint32_t xd[8] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w};
  const uint32_t nd[8] = {n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, n[1].z, n[1].w};
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
  a[0] = u32x4{a0[0], a0[1], a0[2], a0[3]};
  a[1] = u32x4{a1[0], a1[1], a1[2], a1[3]};
  if (add) ss += sq;
}

// ---- The LDS image of x, float32, in fragment order (the whole-K and the resident form) ------------------------------------
// k-block kb is one KiB: [half h of the 8 floats][lane group g][row m] x 16 bytes.  Wave v fetches and stores exactly the
// blocks it multiplies, so x crosses lanes (through LDS), never waves: no workgroup barrier between x and the MFMAs.
// Fetch: M rows x K floats once per workgroup, 16 bytes per lane and load; lane l takes row l & 7, piece l >> 3 (4 floats)
// of the block: a wave-load covers one 128-byte line of each of the 8 rows.  (Fewer than 8 rows: the lanes of the missing
// rows re-load the last row into an image row that is never read.)  A store (8 consecutive lanes = the 8 rows of one
// piece) fills 128 contiguous bytes; a fragment read (ds_read_b128: 16-lane groups that span two g and all rows; lanes c16
// and c16 + 8 share an address) covers 256 contiguous bytes: neither has a bank conflict.
constexpr int XIMG_BLOCK = 1024, XIMG_HALF = 512;
__device__ __forceinline__ uint32_t ximg_fetch_ofs(int lane, int M, int ldx) {      // in x, from the block's first column of row 0
  return ((uint32_t)min(lane & 7, M - 1) * (uint32_t)ldx + 4u * (lane >> 3)) * 4u;   // (<= 8 rows: far below 4 GiB)
}
__device__ __forceinline__ uint32_t ximg_store_ofs(int lane) {                      // in an image block: the fetched piece
  return (uint32_t)(((lane >> 3) & 1) * XIMG_HALF + ((lane >> 4) * 8 + (lane & 7)) * 16);
}
__device__ __forceinline__ uint32_t ximg_read_ofs(int lane, int M) {                // in an image block: the fragment position
  return (uint32_t)(((lane >> 4) * 8 + min(lane & 7, M - 1)) * 16);
}
// STRAIGHT-LINE: a block past the end re-loads block 0
__device__ __forceinline__ u32x4 ximg_fetch(const float* x, uint32_t fetch_ofs, int kb, int nkb) {
  const gptr xb = uniform_ptr(x, (size_t)(kb < nkb ? kb : 0) * 128);
  return *(gptr16)(xb + fetch_ofs);
}
__device__ __forceinline__ void ximg_read(const unsigned char* blk, uint32_t read_ofs, u32x4 (&x)[2]) {
  x[0] = *(const u32x4*)(blk + read_ofs);
  x[1] = *(const u32x4*)(blk + read_ofs + XIMG_HALF);
}

// ---- The cross-wave reduction ------------------------------------------------------------------------------------------------
// Lane (c16, g) holds D rows 4 g + r: rows 0..7 (hi and lo products) in g < 2, rows 8..15 (mid products) in g >= 2 -- added
// here; lanes 0..31 publish y[m = 4 (lane >> 4) + r][n = lane & 15] of their wave into slot `tl` of `red` (4 KiB per slot)
__device__ __forceinline__ void publish(float* red, int tl, int wave, int lane, f32x4 v) {
  v.x += __shfl_xor(v.x, 32); v.y += __shfl_xor(v.y, 32); v.z += __shfl_xor(v.z, 32); v.w += __shfl_xor(v.w, 32);
  if (lane < 32) *(f32x4*)&red[((tl * F32_NW + wave) * 32 + lane) * 4] = v;
}
// columns cc and cc + 8 of row m of slot t: the waves' parts, wave 0 .. 7 in order
__device__ __forceinline__ void sum_waves(const float* red, int t, int m, int cc, float& y0, float& y1) {
  const int el = (m >> 2) * 16 + cc, r = m & 3;
  y0 = 0.f; y1 = 0.f;
#pragma unroll
  for (int ww = 0; ww < F32_NW; ++ww) {
    y0 += red[((t * F32_NW + ww) * 32 + el) * 4 + r];
    y1 += red[((t * F32_NW + ww) * 32 + el + 8) * 4 + r];
  }
}
// column cc of row m of a 16-column tile in out / resid (its partner of sum_waves: + 8)
__device__ __forceinline__ size_t out_ofs(int m, int ldo, int tile, int cc) { return (size_t)m * ldo + tile * 16 + cc; }

// f(NT) for a pass of nt tiles (1..8), NT = nt as a std::integral_constant: THE dispatch on the pass size
template <class F>
__device__ __forceinline__ void with_pass_size(int nt, F&& f) {
  switch (nt) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
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
    ring[slot] = load_w(p.w, valid ? tile_of(i) : w, valid ? kb : 0, nkb, lane);
  }
  __device__ __forceinline__ void issue_first(int s, int i0) {
    const int kb = (s % F32_UB) * F32_NW + wave;
    issue(s, i0 + s / F32_UB, kb, kb < nkb);
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
  __device__ __forceinline__ void split(int c, int u, bool count, const u32x4 (&x)[2], const u32x4 (&n)[2]) {
    split8(x, n, norm, c16 < 8, af[u], count && c * F32_KB + u * F32_NW + wave < nkb, ss);
  }
  __device__ __forceinline__ void split_x(int c, int u, bool count) { split(c, u, count, xr[u], nr[u]); }

  // One position of the stream: the MFMA pair of block u of tile t on ring[slot], then the same registers are re-loaded with
  // the load D positions ahead in this workgroup's sequence (`last`: into the next pass, if there is one: `have_next`)
  template <int NT>
  __device__ __forceinline__ void step(int i0, int c, int nc, int t, int u, bool last, bool have_next) {
    constexpr int L = NT * F32_UB, D = f32_depth(NT);
    const int pos = t * F32_UB + u, slot = pos % D;
    if (c * F32_KB + u * F32_NW + wave < nkb) {         // (wave-uniform; no load inside)
      acc[t] = mfma16<bf16>(af[u][0], ring[slot], acc[t]);
      acc[t] = mfma16<bf16>(af[u][1], ring[slot], acc[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
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
      for (int s = 0; s < D; ++s) issue_first(s, i0);
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
          const int pos = t * F32_UB + u;
          step<NT>(i0, c, nc, t, u, last, have_next);
          if (pos >= L - F32_UB) split_x(nc, pos - (L - F32_UB), first && !last);
          if (pos + XD >= L - F32_UB && pos + XD < L) load_x(nc, pos + XD - (L - F32_UB));
        }
      }
    }

    finish<NT, NT, false>(i0, first);
  }

  // row scale, GU8, residual and store tail of one output pair
  __device__ __forceinline__ void store_out(int m, int cc, int tile, float y0, float y1) {
    y0 *= rs; y1 *= rs;
    if constexpr (GU8) {
      // row-interleaved gate|up tile: columns 0..7 are gate rows 8 tile .. + 7, columns 8..15 the matching up rows
      p.out[(size_t)m * p.ldo + tile * 8 + cc] = swiglu_value<float>(y0, y1, RND_NONE);
    } else {
      const size_t o = out_ofs(m, p.ldo, tile, cc);
      if (p.epi == EPI_RESID) {
        const float h0 = p.resid[o], h1 = p.resid[o + 8];
        p.resid[o] = h0 + y0; p.resid[o + 8] = h1 + y1;
      } else {                                    // EPI_STORE and EPI_STORE_F32 coincide
        p.out[o] = y0; p.out[o + 8] = y1;
      }
    }
  }

  // the cross-wave reduction and epilogue of a pass, TR tiles per round; OVER: behind a barrier, `red` runs on into the images
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
      for (int tl = 0; tl < TR; ++tl) publish(red, tl, wave, lane, acc[r0 + tl]);
      __syncthreads();
      if (r0 == 0 && first && norm) {
        float tot = 0.f;
#pragma unroll
        for (int ww = 0; ww < F32_NW; ++ww) tot += sq_sh[ww * 8 + m];
        rs = 1.0f / sqrtf(tot / (float)p.K + p.eps);
      }
      if (t < TR && m < p.M) {
        float y0, y1;
        sum_waves(red, t, m, cc, y0, y1);
        store_out(m, cc, w + (i0 + r0 + t) * G, y0, y1);    // (t < TR, r0 + t < NT: one of this workgroup's tiles)
      }
    }
  }

  // the size of the pass that begins at this workgroup's tile `done`; `roll`: it is full and so is the one behind it
  __device__ __forceinline__ int pass_size(int done, bool& roll) const {
    const int nt = min(F32_TP, ntiles - done);
    roll = nt == F32_TP && ntiles - done - nt >= F32_TP;
    return nt;
  }

  __device__ __forceinline__ void run() {
    int done = 0;
    bool pre = false;
    while (done < ntiles) {
      bool roll;
      const int nt = pass_size(done, roll);
      const bool first = done == 0;
      if (done > 0) __syncthreads();              // `red` is reused
      // (only a full pass is ever preloaded or rolls)
      with_pass_size(nt, [&](auto n) __attribute__((always_inline)) {
        constexpr int NT = decltype(n)::value;
        pass<NT>(done, NT == F32_TP && pre, NT == F32_TP && roll, first);
      });
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
// -- the 16 loads a wave of the stream keeps in flight.  So there is no ring and no chunk: wave v issues the loads of ALL
// its blocks v, v + 8, v + 16, ... at once (128 KiB per CU at K = 4096), multiplies them in ascending order as they land,
// and the workgroup ends in the reduction of a pass of one tile (publish, sum_waves).
//
// Program order, straight-line (no load under a branch; a slot past the wave's last block re-loads a valid block and is
// ignored).  A CU returns loads in issue order, so what a block's MFMAs need is asked for in the order they need it:
//   * EPI_RESID: the two h values of each epilogue thread (only this workgroup writes them in this launch), first -- two
//     4-byte loads, out of the way before the stream, not dependent loads at the very end.
//   * then PER BLOCK, x and right behind it the block's weights: x0 w0 x1 w1 ... x15 w15.
//     All of x in front of all the weights (the first form built) was measured and is slower in the step: 11.17 against
//     10.58 us per launch (traces of two boxes), 0.051-0.058 against 0.082 ms per step in the A/B.  The
//     reasoning behind the interleaved order, an estimate that no stamp backs: 128 x-loads per CU at 16 cycles each on
//     the CU's address path are ~0.85 us before the first weight request leaves, and HBM idles meanwhile; interleaved,
//     the first weight request leaves behind ONE x load, x (an L2 hit) is back long before the weights in front of it,
//     and the in-order return hands every block its x just ahead of its weights.  Back to back, with the matrix
//     resident in the Infinity Cache, the order is the other way round (9.7 against 10.0 us), and the step is what counts.
// Then per block, as its loads land (counted vmcnt: 31, 30, ... 0): x -> the image -> the lane's fragment position -> split
// -> two MFMAs.  The LDS round trip and the split of block u run while block u's weights are still on their way.  The raw x
// of all 16 blocks is in registers as loaded (64 VGPRs, next to the 64 of the weights: everything is in flight at once), and
// only ONE block's fragment position is read back and split at a time: never 16 blocks of split fragments.
//
// Resources: 512 threads, 155 VGPRs, one workgroup per CU, no scratch.  LDS (dynamic, above 64 KiB -> function attribute):
// the 4-KiB reduction + K / 32 KiB of x (at least one block per wave, so that the ignored slots stay inside it): 132 KiB
// at K = 4096.
constexpr int F32W_RED = F32_NW * 32 * 16;       // bytes of the cross-wave reduction, in front of the x image
constexpr size_t f32_whole_lds_bytes(int K) { return F32W_RED + (size_t)(K / 32 > F32_NW ? K / 32 : F32_NW) * XIMG_BLOCK; }

__global__ __launch_bounds__(F32_NW * 64) void gemv_f32_whole_kernel(F32Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char whole_lds[];
  float* red = (float*)whole_lds;
  unsigned char* ximg = whole_lds + F32W_RED;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = blockIdx.x, nkb = p.K / 32;

  // thread (m, c) of wave 0 finishes columns c and c + 8 of row m (as F32Body::finish): its h now.  Straight-line: the
  // pointer is selected, the load is not under a branch.
  const int em = (tid >> 3) & 7, ecc = tid & 7;
  const bool ep = tid < 64 && em < p.M;
  const bool res = ep && p.epi == EPI_RESID;
  const size_t eo = out_ofs(em, p.ldo, w, ecc);
  const float* hp = res ? p.resid + eo : p.x;
  const float h0 = hp[0], h1 = hp[res ? 8 : 0];
  __builtin_amdgcn_sched_barrier(0);
  u32x4 xs[F32_LB], ring[F32_LB];
  const uint32_t xlane = ximg_fetch_ofs(lane, p.M, p.ldx);
#pragma unroll
  for (int u = 0; u < F32_LB; ++u) {
    const int kb = u * F32_NW + wave;
    xs[u] = ximg_fetch(p.x, xlane, kb, nkb);
    __builtin_amdgcn_sched_barrier(0);
    ring[u] = load_w(p.w, w, kb < nkb ? kb : 0, nkb, lane);
    __builtin_amdgcn_sched_barrier(0);
  }

  // Per block, as its loads land: x -> LDS image (wave-uniform branch, no load inside) -> this lane's fragment position ->
  // split -> two MFMAs.  The image rows a wave reads are the ones it wrote, and the LDS operations of a wave complete in order.
  const uint32_t wofs = ximg_store_ofs(lane), rofs = ximg_read_ofs(lane, p.M);
  const bool low = (lane & 15) < 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < F32_LB; ++u) {
    const int kb = u * F32_NW + wave;
    const bool valid = kb < nkb;                    // (wave-uniform)
    // a slot past the end reads the wave's own first image block (inside the allocation, written by no other wave)
    unsigned char* blk = ximg + (valid ? kb : wave) * XIMG_BLOCK;
    if (valid) *(u32x4*)(blk + wofs) = xs[u];
    __builtin_amdgcn_wave_barrier();
    u32x4 xr[2], a[2];
    ximg_read(blk, rofs, xr);
    float none = 0.f;
    split8(xr, xr, false, low, a, false, none);
    if (valid) {
      acc = mfma16<bf16>(a[0], ring[u], acc);
      acc = mfma16<bf16>(a[1], ring[u], acc);
    }
  }

  publish(red, 0, wave, lane, acc);
  __syncthreads();
  if (ep) {
    float y0, y1;
    sum_waves(red, 0, em, ecc, y0, y1);
    if (p.epi == EPI_RESID) {
      p.resid[eo] = h0 + y0; p.resid[eo + 8] = h1 + y1;
    } else {                                        // EPI_STORE and EPI_STORE_F32 coincide
      p.out[eo] = y0; p.out[eo + 8] = y1;
    }
  }
}

// ---- The resident form: the stream of F32Body with x and the norm weights kept in LDS for the whole launch -----------------
// The head stages x ONCE -- wave v exactly the k-blocks v, v + 8, ... that it multiplies, through the x image above -- and,
// under PRO_NORM, the norm weights of the same blocks into an image of their own (128 bytes per k-block, read back as a
// broadcast).  From then on the only vector-memory loads of the stream are the weight loads, and every wait in it is the
// counted vmcnt(D - 1) or higher.  A chunk's four fragment pairs are rebuilt from the images (four ds_read_b128 and the
// split per block) where split_x stands in the chunked form; the reads are issued in front of the position's MFMAs, which
// cover their latency.  Later passes never stage again.  Same tile deal, passes, block ownership, step(), split8 in the same
// (chunk, block) order, finish(): the outputs are those of gemv_f32_kernel / gemv_f32_gu8_kernel.
//
// LDS (dynamic, one workgroup per CU): [row sums 256 B][reduction 8 KiB][x image K / 32 KiB][norm image K / 256 KiB], the
// images at least 8 blocks (one per wave, so that ignored slots stay inside them), and below K = 4096 one KiB per wave that
// takes the staging stores of blocks past the end: 152.25 KiB at K = 4096.  The 32-KiB reduction buffer of the chunked
// form does not fit next to the images, so a full pass (8 tiles) with another pass behind it reduces 2 tiles per round
// through the 8-KiB buffer.  After the workgroup's LAST pass -- every pass of fewer than 8 tiles is one (run(): nt < 8 only
// when nothing is left), and so is a full pass with nothing behind it -- nobody reads the images: behind a barrier its
// reduction takes 4 KiB per tile from the start of the buffer on into the x image, in one round as in the chunked form
// (the allocation is at least 32 KiB + 256 B).  Either way the sums are taken wave 0 .. 7 in order.
constexpr int F32R_SQ = F32_NW * 8 * 4;          // bytes of the waves' row sums, at the start
constexpr int F32R_RED = 2 * F32_NW * 32 * 16;   // bytes of the 2-tile reduction buffer
constexpr size_t F32R_LDS_MAX = 160 * 1024;      // gfx950: LDS per CU
constexpr int f32_res_blocks(int K) { return K / 32 > F32_NW ? K / 32 : F32_NW; }
constexpr size_t f32_res_dump_bytes(int K) { return K / 32 < F32_NW * F32_LB ? F32_NW * 1024 : 0; }   // (see stage())
constexpr size_t f32_res_lds_bytes(int K) {
  const size_t img = (size_t)F32R_RED + (size_t)f32_res_blocks(K) * (XIMG_BLOCK + 128) + f32_res_dump_bytes(K);
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
    nimg = ximg + (size_t)f32_res_blocks(p.K) * XIMG_BLOCK;
    rofs = ximg_read_ofs(lane, p.M);
  }

  // The head of the first pass: the norm weights, the first four weight loads with the x of their blocks in front of each,
  // the rest of x, the rest of the first D weight loads; then x and the norm weights into their images.  STRAIGHT-LINE.
  // (Two 16-byte loads per lane cover the norm weights of the wave's 16 blocks; without PRO_NORM they read x and are ignored.)
  // A wave's loads return in issue order, so the wait for the last x load is a wait for w0 .. w3 only (vmcnt(D - 4)): the
  // other D - 4 weight loads stay in flight across the staging.  The first D weight loads with ALL the remaining x behind
  // them (the first order built) made it a wait for every weight load of the head: each wave, and so the chip, started the
  // stream with an empty ring, and that form gained 0.014 / 0.020 ms per step in two A/B jobs where this one gains 0.059
  // (DESIGN §5).
  template <int D>
  __device__ __forceinline__ void stage(int i0) {
    u32x4 xs[F32_LB], ns[2];
    const uint32_t xlane = ximg_fetch_ofs(lane, p.M, p.ldx);
    auto load_xs = [&](int u) { xs[u] = ximg_fetch(p.x, xlane, u * F32_NW + wave, nkb); };
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
      B::issue_first(s, i0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = F32_UB; u < F32_LB; ++u) load_xs(u);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = F32_UB; s < D; ++s) B::issue_first(s, i0);
    __builtin_amdgcn_sched_barrier(0);
    // No store under a branch either: at the join behind a skipped store the compiler's wait for the skipped load's registers
    // came out as vmcnt(1) / vmcnt(0) in front of the first image reads -- the drain this form exists to remove.  A block past
    // the end (and the norm weights of one) goes to a KiB of the wave's own behind the images, which nobody reads; it is there
    // whenever a wave can have such a block (K < 4096).
    const uint32_t wofs = ximg_store_ofs(lane);
    unsigned char* dump = nimg + f32_res_blocks(p.K) * 128 + wave * 1024;
#pragma unroll
    for (int u = 0; u < F32_LB; ++u) {
      const int kb = u * F32_NW + wave;
      *(u32x4*)((kb < nkb ? ximg + kb * XIMG_BLOCK : dump) + wofs) = xs[u];
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
    const unsigned char* nb = nimg + b * 128 + g * 32;
    ximg_read(ximg + b * XIMG_BLOCK, rofs, xr);
    nr[0] = *(const u32x4*)nb; nr[1] = *(const u32x4*)(nb + 16);
  }

  // the fragments of chunk 0
  __device__ __forceinline__ void rebuild0(bool count) {
#pragma unroll
    for (int u = 0; u < F32_UB; ++u) {
      u32x4 xr[2], nr[2];
      read_img(0, u, xr, nr);
      B::split(0, u, count, xr, nr);
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
        for (int s = 0; s < D; ++s) B::issue_first(s, i0);
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
          const int pos = t * F32_UB + u;
          // Block u's fragments are last used at position L - 4 + u and replaced right there by the next chunk's, read from
          // the images in front of the MFMAs.  In the last chunk of a pass that does not roll, chunk 0's are rebuilt, unused
          // (straight-line filler as in F32Body::pass; `count` is false).
          u32x4 xr[2], nr[2];
          if (pos >= L - F32_UB) read_img(nc, pos - (L - F32_UB), xr, nr);
          B::template step<NT>(i0, c, nc, t, u, last, have_next);
          if (pos >= L - F32_UB) B::split(nc, pos - (L - F32_UB), first && !last, xr, nr);
        }
      }
    }

    // ---- cross-wave reduction and epilogue (see the notes above): the workgroup's last pass in one round over the images
    if constexpr (NT < F32_TP) {
      B::template finish<NT, NT, true>(i0, first);
    } else {
      if (final) B::template finish<NT, NT, true>(i0, first);
      else B::template finish<NT, 2, false>(i0, first);
    }
  }

  template <bool FIRST>
  __device__ __forceinline__ void pass_of(int nt, int i0, bool preloaded, bool roll, bool final) {
    // (only a full pass is ever preloaded or rolls, and a shorter one is the workgroup's last)
    with_pass_size(nt, [&](auto n) __attribute__((always_inline)) {
      constexpr int NT = decltype(n)::value;
      pass<NT, FIRST>(i0, NT == F32_TP && preloaded, NT == F32_TP && roll, NT < F32_TP || final);
    });
  }

  __device__ __forceinline__ void run() {
    if (ntiles <= 0) return;
    bool pre;
    int done = B::pass_size(0, pre);
    pass_of<true>(done, 0, false, pre, done == ntiles);
    while (done < ntiles) {
      bool roll;
      const int nt = B::pass_size(done, roll);
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

// ---- host side -------------------------------------------------------------------------------------------------------------
// what every launcher of this file refuses
int f32_check(const char* name, bool supported, const GemvCall& c) {
  if (!supported) return fail(MI_ERR_UNSUPPORTED, std::string(name) + ": call not supported by this kernel");
  if (c.epi == EPI_RESID ? c.resid == nullptr : c.out == nullptr) return fail(MI_ERR_INVALID, std::string(name) + ": output buffer missing");
  return MI_OK;
}

F32Params make_params(const LinearW& W, const GemvCall& c) {
  F32Params p{};
  p.x = (const float*)c.x; p.ldx = c.ldx; p.M = c.M;
  p.pro = c.pro; p.norm_w = (const float*)c.norm_w; p.eps = c.eps;
  p.w = W.w; p.N = W.N; p.K = W.K;
  p.epi = c.epi; p.out = (float*)c.out; p.ldo = c.ldo; p.resid = (float*)c.resid;
  return p;
}

int f32_launch(void (*kern)(F32Params), int nwg, size_t lds, const LinearW& W, const GemvCall& c, hipStream_t st) {
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(F32_NW * 64), lds, st, make_params(W, c));
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// one workgroup per CU; tiles are dealt in-kernel
int f32_grid(const LinearW& W) { return std::min(W.N / 16, gemv_cu_count()); }

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
  MI_TRY(f32_check("gemv_f32", gemv_f32_supported(W, c), c));
  return f32_launch(c.epi == EPI_SWIGLU_GU8 ? gemv_f32_gu8_kernel : gemv_f32_kernel, f32_grid(W), 0, W, c, st);
}

// The whole-K form: what gemv_f32_supported takes, without a prologue, K <= 4096 (16 k-blocks per wave) and at most one
// tile per CU (the tile is the workgroup's only work: more tiles than CUs would queue whole workgroups behind one another)
bool gemv_f32_whole_supported(const LinearW& W, const GemvCall& c) {
  if (!gemv_f32_supported(W, c)) return false;
  if (c.pro != PRO_NONE) return false;
  if (c.epi != EPI_STORE && c.epi != EPI_STORE_F32 && c.epi != EPI_RESID) return false;
  if (W.K > F32_NW * F32_LB * 32) return false;
  return W.N / 16 <= gemv_cu_count();
}

int launch_gemv_f32_whole(const LinearW& W, const GemvCall& c, hipStream_t st) {
  MI_TRY(f32_check("gemv_f32_whole", gemv_f32_whole_supported(W, c), c));
  static std::atomic<bool> opted[64];
  MI_TRY(lds_opt_in(opted, {(const void*)gemv_f32_whole_kernel}, (int)f32_whole_lds_bytes(F32_NW * F32_LB * 32)));
  return f32_launch(gemv_f32_whole_kernel, W.N / 16, f32_whole_lds_bytes(W.K), W, c, st);
}

// The resident form: what gemv_f32_supported takes, with at most 16 k-blocks per wave (K <= 4096: the head holds a wave's
// raw x in registers at once) and the images and the reduction buffer inside a CU's LDS
bool gemv_f32_resident_supported(const LinearW& W, const GemvCall& c) {
  if (!gemv_f32_supported(W, c)) return false;
  if (W.K > F32_NW * F32_LB * 32) return false;
  return f32_res_lds_bytes(W.K) <= F32R_LDS_MAX;
}

int launch_gemv_f32_resident(const LinearW& W, const GemvCall& c, hipStream_t st) {
  MI_TRY(f32_check("gemv_f32_resident", gemv_f32_resident_supported(W, c), c));
  static std::atomic<bool> opted[64];
  MI_TRY(lds_opt_in(opted, {(const void*)gemv_f32_resident_kernel, (const void*)gemv_f32_resident_gu8_kernel},
                    (int)f32_res_lds_bytes(F32_NW * F32_LB * 32)));
  return f32_launch(c.epi == EPI_SWIGLU_GU8 ? gemv_f32_resident_gu8_kernel : gemv_f32_resident_kernel, f32_grid(W),
                    f32_res_lds_bytes(W.K), W, c, st);
}

}  // namespace mi
