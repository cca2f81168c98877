// moe_q.hip -- the grouped expert linear of moe.hip over MLX-affine quantised experts (QuantizedSwitchLinear on mx.gather_qmm:
// switch_layers.py:7-70; mixtral.py:198-215 stacks weight, scales and biases of every expert), group 64, 4 and 8 bits.
// Same contract as launch_moe_linear: for every pair p on expert e's list out[p][n] = T(x[p >> x_shift] . W_hat_e[n]), with
// SwiGLU T(T(silu(g)) u) of the gate and the up result (linear_epilogue.h).  W_hat = scale * q + bias stays in float32 and is
// never materialised: per group of 64
//     y += s * sum((offs + q) x) + (b - offs s) * sum(x)
// with the (offs + q) x products on v_mfma_f32_16x16x32_{bf16,f16} (T = float: q widened exactly, v_mfma_f32_16x16x4_f32) and
// the (b - offs s) sum(x) term of a block's groups on ONE v_mfma_f32_16x16x4_f32 (gemm_q4.hip's arithmetic).
//
// Shape of the work ("Quantised experts"):
//   * weights: the stacked [E][N][K] tensor is ONE tall [E N][K] matrix in repack.hip's tile-major int4 / int8 layout; expert
//     e's tiles start at row tile e N / 16.  A wave streams consecutive 1152 / 1088-byte blocks, lane-linear dwordx4 loads.
//   * x: prepared ONCE per launch by moe_q_prep_kernel -- every row of x in the piece order in which the lanes of the MFMA A
//     fragments consume it (int4: the nibble order of unpack_q4) plus the per-(row, group) sums of x.  The linear kernel
//     gathers 16-byte pieces by list[i]; its inner loop carries no re-staging arithmetic, no LDS traffic and no barrier.
//   * grid (tile units, E); a workgroup of four waves = TW tile units x KW K lanes.  Wave (tw, kw) owns unit tw and every
//     KW-th block; the KW partial accumulators meet in LDS once, in K-lane order.  KW is a function of K alone (the number of
//     blocks), never of the row count: the order in which a row's products are added must not change with the rows that share
//     the step.  The row count selects only RT, the row tiles that share one unpack of a weight block (1: a decode step).
//   * SwiGLU: a tile unit is the gate tile and the up tile of the same columns: one A fragment feeds both.
//   * every weight load stays inside its expert's tiles: the prefetch past a wave's last block is clamped to that block.
#include <algorithm>

#include "gemv_phase.h"

namespace mi {
namespace {

using gemv::Magic;
using gemv::unpack_q4;

constexpr int NTHR = 256;

template <typename S>
__device__ __forceinline__ float s_to_f32(uint32_t bits16) {
  if constexpr (std::is_same<S, bf16>::value) return __uint_as_float(bits16 << 16);
  else return (float)__builtin_bit_cast(f16, (uint16_t)bits16);
}

// position of the piece x[k .. k + 8) (k % 8 == 0) in a prepared row: fragment-major, lane group inside
template <int BITS>
__device__ __forceinline__ int piece_of(int k) {
  if constexpr (BITS == 4) {
    // 128-k block kb, quantisation group sg, MFMA step t, lane group gg: packed dword d = {0, 4, 2, 6}[gg] + t of the group
    // (gemv_phase.h: frag_slot -- where v_permlane32_swap leaves the dwords of a tile-major int4 block)
    const int dd = (k >> 3) & 15, kb = k >> 7, sg = dd >> 3, d = dd & 7, t = d & 1, ee = d - t;
    const int gg = (ee == 0) ? 0 : (ee == 4) ? 1 : (ee == 2) ? 2 : 3;
    return (((kb * 2 + sg) * 2 + t) * 4 + gg);
  } else {
    // 64-k block kb: lane group g holds k 16 g .. 16 g + 15, its first 8 feed step 0, the other 8 step 1
    const int k8 = k >> 3, kb = k8 >> 3, g = (k8 & 7) >> 1, t = k8 & 1;
    return ((kb * 2 + t) * 4 + g);
  }
}

// ---- x -> piece order + group sums.  One workgroup per row of x; xq [rows][K] of T, sx [rows][K / 64] float32.
template <typename T, int BITS>
__global__ __launch_bounds__(NTHR) void moe_q_prep_kernel(const T* x, int ldx, int K, T* xq, float* sx) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* xr = x + (size_t)row * ldx;
  T* dst = xq + (size_t)row * K;
  for (int k = tid * 8; k < K; k += NTHR * 8) {
    T e[8];
    if constexpr (sizeof(T) == 4) { *(f32x4*)e = *(const f32x4*)(xr + k); *(f32x4*)(e + 4) = *(const f32x4*)(xr + k + 4); }
    else *(u32x4*)e = *(const u32x4*)(xr + k);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += (float)e[j];
    sum = lane8_sum(sum);                                      // the 8 pieces of a 64-group sit in 8 consecutive threads
    T o[8];
    if constexpr (BITS == 4 && sizeof(T) == 2) {               // nibble order of unpack_q4: 2 p <- k + p, 2 p + 1 <- k + p + 4
#pragma unroll
      for (int q = 0; q < 4; ++q) { o[2 * q] = e[q]; o[2 * q + 1] = e[q + 4]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = e[j];
    }
    T* d = dst + (size_t)piece_of<BITS>(k) * 8;
    if constexpr (sizeof(T) == 4) { *(f32x4*)d = *(const f32x4*)o; *(f32x4*)(d + 4) = *(const f32x4*)(o + 4); }
    else *(u32x4*)d = *(const u32x4*)o;
    if ((tid & 7) == 0) sx[(size_t)row * (K / 64) + (k >> 6)] = sum;
  }
}

struct MoeQParams {
  const void* xq; const float* sx; int x_shift;
  const void* w; const void* w2;         // tile-major stacks; SWIGLU: w = gate, w2 = up
  int N, K, E, TW, KW;
  const int32_t* meta; const int32_t* list;
  void* out; int ldo, rnd;
};

// the weights of one block of one tile as a lane holds them
struct WBlock { u32x4 q; uint32_t s, b; };

// T: activations; S: scale dtype (= T unless T is float); RT: row tiles of 16 pairs per pass over the weights
template <typename T, typename S, int BITS, bool SWIGLU, int RT>
__global__ __launch_bounds__(NTHR) void moe_q_linear_kernel(MoeQParams p) {
  constexpr int TN = SWIGLU ? 2 : 1;
  constexpr int BK = BITS == 4 ? 128 : 64, BB = BITS == 4 ? 1152 : 1088;
  constexpr int NF = BK / 32;                                  // A fragments (32 k each) per block
  constexpr int SOFF = 1024, BOFF = BITS == 4 ? 1088 : 1056;
  constexpr int XV = sizeof(T) / 2;                            // 16-byte loads per piece
  constexpr bool X32 = sizeof(T) == 4;
  constexpr float OFFS = (BITS == 4 && !X32) ? Magic<S>::offs : 0.f;
  constexpr bool XFIRST = RT == 1;                             // a block's pieces of x are loaded in front of the weight prefetch
  __shared__ f32x4 red[3 * TN * RT * 64];                      // (KW - 1) TW <= 3 partial units

  const int e = blockIdx.y;
  const int cnt = p.meta[e];
  if (cnt <= 0) return;
  const int32_t* list = p.list + p.meta[p.E + e];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int TW = p.TW, KW = p.KW, kw = wave / TW, tw = wave - kw * TW;
  const int ntiles = p.N >> 4, nblk = p.K / BK, K = p.K;
  const int tu_raw = blockIdx.x * TW + tw;
  const bool valid = tu_raw < ntiles;
  const int tu = valid ? tu_raw : ntiles - 1;                  // a spare wave re-streams the last unit and stores nothing
  const char* wb[TN];
  wb[0] = (const char*)p.w + ((size_t)e * ntiles + tu) * nblk * BB;
  if constexpr (SWIGLU) wb[1] = (const char*)p.w2 + ((size_t)e * ntiles + tu) * nblk * BB;

  // block b of the wave's tiles (clamped: the prefetch past the last block re-reads it)
  auto fetch = [&](int b, WBlock (&o)[TN]) {
    const size_t off = (size_t)min(b, nblk - 1) * BB;
#pragma unroll
    for (int a = 0; a < TN; ++a) {
      const char* blk = wb[a] + off;
      o[a].q = __builtin_nontemporal_load((const u32x4*)(blk + lane * 16));
      if constexpr (BITS == 4) {
        o[a].s = *(const uint32_t*)(blk + SOFF + c * 4);
        o[a].b = *(const uint32_t*)(blk + BOFF + c * 4);
      } else {
        o[a].s = *(const uint16_t*)(blk + SOFF + c * 2);
        o[a].b = *(const uint16_t*)(blk + BOFF + c * 2);
      }
    }
  };

  for (int base = 0; base < cnt; base += 16 * RT) {
    const char* xr[RT];
    const float* sr[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int i = min(base + t * 16 + c, cnt - 1);           // (rows past the list repeat its last pair; never stored)
      const size_t row = (size_t)(list[i] >> p.x_shift);
      xr[t] = (const char*)p.xq + (row * K) * sizeof(T) + g * 16 * XV;
      sr[t] = p.sx + row * (K / 64);
    }
    f32x4 acc[TN][RT];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto load_x = [&](int b, int f, int t, u32x4 (&o)[XV]) {
      const char* px = xr[t] + (size_t)(b * NF + f) * (64 * XV);
#pragma unroll
      for (int v = 0; v < XV; ++v) o[v] = *(const u32x4*)(px + 16 * v);
    };

    WBlock w0[TN], w1[TN], w2[TN];
    fetch(kw, w0);
    fetch(kw + KW, w1);
    for (int b = kw; b < nblk; b += KW) {
      u32x4 xa[XFIRST ? NF : 1][XV];
      float sxa[RT];
      if constexpr (XFIRST) {
#pragma unroll
        for (int f = 0; f < NF; ++f) load_x(b, f, 0, xa[f]);
      }
      // sum(x) of row c, group (g & 1) of the block (int8: its one group) -- the A operand of the bias MFMA
#pragma unroll
      for (int t = 0; t < RT; ++t) sxa[t] = sr[t][BITS == 4 ? 2 * b + (g & 1) : b];
      __builtin_amdgcn_sched_barrier(0);
      fetch(b + 2 * KW, w2);
      __builtin_amdgcn_sched_barrier(0);

      // ---- one block of the wave's tiles against the row tiles
      uint32_t dw[TN][4];
      float sc[TN][2], bbv[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const u32x4 v = w0[a].q;
        if constexpr (BITS == 4) {
          // lanes g < 2 hold group A's dwords, g >= 2 group B's: afterwards {0, 1} = group A, {2, 3} = group B in every lane
          auto r0 = __builtin_amdgcn_permlane32_swap(v.x, v.z, false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(v.y, v.w, false, false);
          dw[a][0] = r0[0]; dw[a][1] = r1[0]; dw[a][2] = r0[1]; dw[a][3] = r1[1];
          sc[a][0] = s_to_f32<S>(w0[a].s & 0xffffu); sc[a][1] = s_to_f32<S>(w0[a].s >> 16);
          const float bv = s_to_f32<S>((g & 1) ? (w0[a].b >> 16) : (w0[a].b & 0xffffu));
          bbv[a] = g < 2 ? fmaf(-OFFS, sc[a][g & 1], bv) : 0.f;
        } else {
          dw[a][0] = v.x; dw[a][1] = v.y; dw[a][2] = v.z; dw[a][3] = v.w;
          sc[a][0] = sc[a][1] = s_to_f32<S>(w0[a].s);
          bbv[a] = g == 0 ? s_to_f32<S>(w0[a].b) : 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
        if (RT == 1 || base + t * 16 < cnt) {
#pragma unroll
          for (int a = 0; a < TN; ++a) acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sxa[t], bbv[a], acc[a][t], 0, 0, 0);
        }
      constexpr int NG = BITS == 4 ? 2 : 1;                    // quantisation groups per block; NF / NG fragments each
#pragma unroll
      for (int sg = 0; sg < NG; ++sg) {
        // the codes of the group's two fragments, unpacked once for all row tiles
        u32x4 wq[TN][2];
        float wf[TN][2][X32 ? 8 : 1];
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if constexpr (BITS == 4) {
              const uint32_t d = dw[a][sg * 2 + s];
              if constexpr (X32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) wf[a][s][j] = (float)((d >> (4 * j)) & 15u);
              } else {
                wq[a][s] = unpack_q4<S>(d);
              }
            } else {
              const uint32_t lo = dw[a][2 * s], hi = dw[a][2 * s + 1];
              if constexpr (X32) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { wf[a][s][j] = (float)((lo >> (8 * j)) & 255u); wf[a][s][4 + j] = (float)((hi >> (8 * j)) & 255u); }
              } else {
                S q8[8];                                       // 0..255 are exact in bf16 and f16
#pragma unroll
                for (int j = 0; j < 4; ++j) { q8[j] = (S)(float)((lo >> (8 * j)) & 255u); q8[4 + j] = (S)(float)((hi >> (8 * j)) & 255u); }
                wq[a][s] = *(const u32x4*)q8;
              }
            }
          }
#pragma unroll
        for (int t = 0; t < RT; ++t)
          if (RT == 1 || base + t * 16 < cnt) {
            f32x4 d[TN];
#pragma unroll
            for (int a = 0; a < TN; ++a) d[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const int f = sg * 2 + s;
              u32x4 xl[XV];
              if constexpr (!XFIRST) load_x(b, f, t, xl);
              const u32x4 (&xp)[XV] = XFIRST ? xa[XFIRST ? f : 0] : xl;
#pragma unroll
              for (int a = 0; a < TN; ++a) {
                if constexpr (X32) {
#pragma unroll
                  for (int j = 0; j < 8; ++j)
                    d[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(xp[j >> 2][j & 3]), wf[a][s][j], d[a], 0, 0, 0);
                } else {
                  d[a] = mfma16<T>(xp[0], wq[a][s], d[a]);
                }
              }
            }
#pragma unroll
            for (int a = 0; a < TN; ++a) {
              const float s1 = sc[a][sg];
              acc[a][t].x = fmaf(s1, d[a].x, acc[a][t].x); acc[a][t].y = fmaf(s1, d[a].y, acc[a][t].y);
              acc[a][t].z = fmaf(s1, d[a].z, acc[a][t].z); acc[a][t].w = fmaf(s1, d[a].w, acc[a][t].w);
            }
          }
        if constexpr (X32) {                                   // (the float32 MFMAs' B operands stay reserved: gemm_q4.hip, block_mfma)
#pragma unroll
          for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
              for (int j = 0; j < 8; ++j) asm volatile("" :: "v"(wf[a][s][j]));
        }
      }
#pragma unroll
      for (int t = 0; t < RT; ++t) asm volatile("" :: "v"(sxa[t]));
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        asm volatile("" :: "v"(bbv[a]));
        w0[a] = w1[a]; w1[a] = w2[a];
      }
    }

    // ---- the KW partial accumulators of a unit meet in LDS, in K-lane order
    if (KW > 1) {
      if (kw > 0) {
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
          for (int t = 0; t < RT; ++t) red[(((kw - 1) * TW + tw) * (TN * RT) + a * RT + t) * 64 + lane] = acc[a][t];
      }
      __syncthreads();
      if (kw == 0) {
        for (int k2 = 1; k2 < KW; ++k2) {
#pragma unroll
          for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const f32x4 v = red[(((k2 - 1) * TW + tw) * (TN * RT) + a * RT + t) * 64 + lane];
              acc[a][t].x += v.x; acc[a][t].y += v.y; acc[a][t].z += v.z; acc[a][t].w += v.w;
            }
        }
      }
    }
    // C layout: column = lane & 15, row = 4 (lane >> 4) + register
    if (kw == 0 && valid) {
      const int n = tu * 16 + c;
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = base + t * 16 + g * 4 + r;
          if (i < cnt) {
            float v = linear_value<T>(acc[0][t][r], false, nullptr, 0, 0, p.rnd);
            if constexpr (SWIGLU) v = swiglu_value<T>(v, linear_value<T>(acc[1][t][r], false, nullptr, 0, 0, p.rnd), p.rnd);
            ((T*)p.out)[(size_t)list[i] * p.ldo + n] = store_act<T>(v, p.rnd);
          }
        }
    }
    if (KW > 1 && base + 16 * RT < cnt) __syncthreads();       // `red` is written again by the next pass
  }
}

// router [E][H] from its quantised triple: s * q + b in float32 (two roundings, the oracle's W_hat)
template <typename S>
__global__ __launch_bounds__(NTHR) void moe_q_router_kernel(const uint32_t* codes, const S* scales, const S* biases, int bits, int H,
                                                            size_t total, float* out) {
  const size_t i = (size_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= total) return;
  const size_t row = i / H;
  const int k = (int)(i - row * H), per = 32 / bits;
  const uint32_t q = (codes[row * (H / per) + k / per] >> (bits * (k % per))) & ((1u << bits) - 1u);
  const size_t gi = row * (H / 64) + (k >> 6);
  out[i] = mul_add_unfused((float)scales[gi], (float)q, (float)biases[gi]);
}

template <typename T, typename S, int BITS>
int launch_q(const MoeQParams& p, bool swiglu, int rt, dim3 grid, hipStream_t st) {
  if (swiglu) {
    if (rt == 1) hipLaunchKernelGGL((moe_q_linear_kernel<T, S, BITS, true, 1>), grid, dim3(NTHR), 0, st, p);
    else hipLaunchKernelGGL((moe_q_linear_kernel<T, S, BITS, true, 4>), grid, dim3(NTHR), 0, st, p);
  } else {
    if (rt == 1) hipLaunchKernelGGL((moe_q_linear_kernel<T, S, BITS, false, 1>), grid, dim3(NTHR), 0, st, p);
    else hipLaunchKernelGGL((moe_q_linear_kernel<T, S, BITS, false, 4>), grid, dim3(NTHR), 0, st, p);
  }
  return MI_OK;
}

template <typename T, typename S>
int launch_ts(const MoeLinearQCall& c, MoeQParams& p, int rt, dim3 grid, hipStream_t st) {
  T* xq = (T*)c.ws;
  float* sx = (float*)((char*)c.ws + moe_q_ws_bytes(c.x_rows, c.K, c.act) - (size_t)c.x_rows * (c.K / 64) * sizeof(float));
  p.xq = xq; p.sx = sx;
  if (c.bits == 4) hipLaunchKernelGGL((moe_q_prep_kernel<T, 4>), dim3(c.x_rows), dim3(NTHR), 0, st, (const T*)c.x, c.ldx, c.K, xq, sx);
  else hipLaunchKernelGGL((moe_q_prep_kernel<T, 8>), dim3(c.x_rows), dim3(NTHR), 0, st, (const T*)c.x, c.ldx, c.K, xq, sx);
  MI_HIP(hipGetLastError());
  return c.bits == 4 ? launch_q<T, S, 4>(p, c.swiglu != 0, rt, grid, st) : launch_q<T, S, 8>(p, c.swiglu != 0, rt, grid, st);
}

}  // namespace

// prepared rows [x_rows][K] of T, then the group sums [x_rows][K / 64] float32
size_t moe_q_ws_bytes(int x_rows, int K, int act) {
  const size_t xq = ((size_t)x_rows * K * dtype_size(act) + 255) & ~(size_t)255;
  return xq + (size_t)x_rows * (K / 64) * sizeof(float);
}

int moe_q_check_shape(int bits, int group, int N, int K, const std::string& who) {
  if (bits != 4 && bits != 8) return fail(MI_ERR_UNSUPPORTED, who + ": quantised experts are int4 or int8");
  if (group != 64) return fail(MI_ERR_UNSUPPORTED, who + ": quantised experts need groups of 64");
  if (N < 16 || N % 16 != 0) return fail(MI_ERR_UNSUPPORTED, who + ": the rows of an expert matrix must be a multiple of 16");
  if (K < (bits == 4 ? 128 : 64) || K % (bits == 4 ? 128 : 64) != 0)
    return fail(MI_ERR_UNSUPPORTED, who + (bits == 4 ? ": int4 experts need K to be a multiple of 128" : ": int8 experts need K to be a multiple of 64"));
  return MI_OK;
}

int launch_moe_linear_q(const MoeLinearQCall& c, hipStream_t st) {
  if (c.act != MI_F32 && c.act != MI_BF16 && c.act != MI_F16) return fail(MI_ERR_INVALID, "moe_linear_q: bad activation dtype");
  if (c.sdt != MI_BF16 && c.sdt != MI_F16) return fail(MI_ERR_UNSUPPORTED, "moe_linear_q: scales must be bf16 or f16");
  if (c.act != MI_F32 && c.act != c.sdt) return fail(MI_ERR_UNSUPPORTED, "moe_linear_q: 16-bit activations need scales of the same dtype");
  if (!c.x || !c.w || !c.meta || !c.list || !c.out || !c.ws || (c.swiglu && !c.w2)) return fail(MI_ERR_INVALID, "moe_linear_q: null argument");
  if (c.E < 1 || c.E > MOE_MAX_EXPERTS) return fail(MI_ERR_UNSUPPORTED, "moe_linear_q: 1 to 16 experts");
  MI_TRY(moe_q_check_shape(c.bits, 64, c.N, c.K, "moe_linear_q"));
  if (c.ldx < c.K || c.ldx % 8 != 0 || c.ldo < c.N || c.x_shift < 0 || c.x_shift > 1 || c.x_rows < 1 || c.pairs < 1)
    return fail(MI_ERR_INVALID, "moe_linear_q: bad row stride or row count");
  if ((uintptr_t)c.x % 16 != 0 || (uintptr_t)c.w % 16 != 0 || (uintptr_t)c.w2 % 16 != 0 || (uintptr_t)c.ws % 256 != 0)
    return fail(MI_ERR_INVALID, "moe_linear_q: misaligned buffer");
  const int nblk = c.K / (c.bits == 4 ? 128 : 64);
  MoeQParams p{};
  p.x_shift = c.x_shift; p.w = c.w; p.w2 = c.w2; p.N = c.N; p.K = c.K; p.E = c.E;
  p.KW = nblk >= 4 ? 4 : nblk >= 2 ? 2 : 1;                    // K alone decides the order of a row's sums
  p.TW = 4 / p.KW;
  p.meta = c.meta; p.list = c.list; p.out = c.out; p.ldo = c.ldo; p.rnd = c.rnd;
  const int rt = c.pairs <= 16 ? 1 : 4;                        // no expert of a decode step has more than one row tile
  const dim3 grid((c.N / 16 + p.TW - 1) / p.TW, c.E);
  int rc;
  if (c.act == MI_BF16) rc = launch_ts<bf16, bf16>(c, p, rt, grid, st);
  else if (c.act == MI_F16) rc = launch_ts<f16, f16>(c, p, rt, grid, st);
  else if (c.sdt == MI_BF16) rc = launch_ts<float, bf16>(c, p, rt, grid, st);
  else rc = launch_ts<float, f16>(c, p, rt, grid, st);
  MI_TRY(rc);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_moe_router_dequant(const void* codes, const void* scales, const void* biases, int sdt, int bits, int E, int H, float* out,
                              hipStream_t st) {
  if (!codes || !scales || !biases || !out || (bits != 4 && bits != 8) || E < 1 || H < 64 || H % 64 != 0 || (sdt != MI_BF16 && sdt != MI_F16))
    return fail(MI_ERR_INVALID, "moe_router_dequant: bad argument");
  const size_t total = (size_t)E * H;
  const dim3 grid((unsigned)((total + NTHR - 1) / NTHR));
  if (sdt == MI_BF16) hipLaunchKernelGGL(moe_q_router_kernel<bf16>, grid, dim3(NTHR), 0, st, (const uint32_t*)codes, (const bf16*)scales, (const bf16*)biases, bits, H, total, out);
  else hipLaunchKernelGGL(moe_q_router_kernel<f16>, grid, dim3(NTHR), 0, st, (const uint32_t*)codes, (const f16*)scales, (const f16*)biases, bits, H, total, out);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
