// moe.hip -- the sparse mixture-of-experts MLP of Mixtral (mixtral.py:95-119, switch_layers.py:73-140) on the device:
//   route     gate logits g = T(xn Wg^T), the k largest (a tie goes to the lower expert index), scores = T(softmax_f32 over the
//             selected), then the per-expert work lists (pair = row * k + j, ascending) built by a scan
//   linear    grouped linear over the lists: every (column tile, expert) workgroup gathers its expert's rows and multiplies them
//             by that expert's matrix on the matrix cores; the gate|up form ends in SwiGLU, the down form in a plain store
//   combine   r = T(T(y_a s_a) + T(y_b s_b)), h = T(h + r), row-wise
// Which matrix a row meets is decided here, per row, per layer; the host never reads it.  Every rounding point is one of
// linear_epilogue.h's.  T = the activations' storage type (float32 in the float32-KV mode, where the 16-bit weights are widened
// -- exactly -- and multiplied with v_mfma_f32_16x16x4_f32: one float32 form serves bf16 and f16 checkpoints alike).
#include <algorithm>

#include "linear_epilogue.h"

namespace mi {
namespace {

constexpr int NTHR = 256;          // linear, gate and combine kernels: four waves
constexpr int LIST_THR = 1024;     // the list kernel: one workgroup of sixteen waves
constexpr int RT = 4;              // row tiles (of 16 pairs) that ride on one pass over a workgroup's weight tile

template <typename W>
__device__ __forceinline__ float w_to_f32(uint32_t bits16) {
  if constexpr (std::is_same<W, bf16>::value) return __uint_as_float(bits16 << 16);
  else return (float)__builtin_bit_cast(f16, (uint16_t)bits16);
}

// eight consecutive 16-bit weights (one 16-byte piece) widened to float32, element j at k + j
template <typename W>
__device__ __forceinline__ void widen8(const u32x4& v, float (&o)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[2 * j] = w_to_f32<W>(v[j] & 0xffffu);
    o[2 * j + 1] = w_to_f32<W>(v[j] >> 16);
  }
}

// ---- route, part 1: one wave per token row -------------------------------------------------------------------------------
template <typename T, typename W>
__global__ __launch_bounds__(NTHR) void moe_gate_kernel(const T* xn, int ldx, int R, int H, int rnd, const W* wg, int E, int k,
                                                        int32_t* sel, T* score) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6);
  if (row >= R) return;
  float acc[MOE_MAX_EXPERTS];
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) acc[e] = 0.f;
  const T* xr = xn + (size_t)row * ldx;
  for (int k0 = lane * 8; k0 < H; k0 += 64 * 8) {
    float xv[8];
    if constexpr (sizeof(T) == 4) {
      const f32x4 a = *(const f32x4*)(xr + k0), b = *(const f32x4*)(xr + k0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { xv[j] = a[j]; xv[4 + j] = b[j]; }
    } else {
      widen8<T>(*(const u32x4*)(xr + k0), xv);
    }
#pragma unroll
    for (int e = 0; e < MOE_MAX_EXPERTS; ++e)
      if (e < E) {
        float wv[8];
        widen8<W>(*(const u32x4*)(wg + (size_t)e * H + k0), wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[e] = fmaf(xv[j], wv[j], acc[e]);
      }
  }
  // g = T(sum): float32 accumulation, one rounding.  Then the k largest; strict comparisons in ascending index order give a
  // tie to the lower expert index
  float best = 0.f, second = 0.f;
  int a = -1, b = -1;
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e)
    if (e < E) {
      acc[e] = rounded<T>(wave_sum(acc[e]), rnd);
      if (a < 0 || acc[e] > best) { best = acc[e]; a = e; }
    }
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e)
    if (e < E && e != a && (b < 0 || acc[e] > second)) { second = acc[e]; b = e; }
  if (lane != 0) return;
  if (k == 1) {
    sel[row] = a;
    score[row] = from_f32<T>(rounded<T>(1.0f, rnd));
  } else {
    // softmax over the two selected in float32 (precise=True: exp(g - max) / sum), rounded once to T.  The one exp of a row is
    // taken in float64 and rounded to float32 -- a correctly rounded float32 exp, on one lane, for nothing
    const float eb = (float)exp((double)(second - best)), den = 1.0f + eb;
    sel[2 * (size_t)row] = a; sel[2 * (size_t)row + 1] = b;
    score[2 * (size_t)row] = from_f32<T>(rounded<T>(1.0f / den, rnd));
    score[2 * (size_t)row + 1] = from_f32<T>(rounded<T>(eb / den, rnd));
  }
}

// ---- route, part 2: the work lists.  One workgroup walks the P = R k pairs in order: counts first, then every chunk of 1024
// pairs places its members behind the earlier ones of the same expert (ballot ranks inside a wave, the waves' counts through
// LDS).  No atomic decides a position, so the lists are in ascending pair order in every run.
// meta[e] = cnt[e], meta[E + e] = the first entry of expert e in `list`.
__global__ __launch_bounds__(LIST_THR) void moe_lists_kernel(const int32_t* sel, int P, int E, int32_t* meta, int32_t* list) {
  __shared__ int cnt[MOE_MAX_EXPERTS], base[MOE_MAX_EXPERTS], wcnt[LIST_THR / 64][MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < MOE_MAX_EXPERTS) cnt[tid] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += LIST_THR) {
    const int s = sel[p];
    if ((unsigned)s < (unsigned)E) atomicAdd(&cnt[s], 1);          // (a count: the order of the adds cannot show)
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int e = 0; e < E; ++e) { base[e] = o; meta[e] = cnt[e]; meta[E + e] = o; o += cnt[e]; }
  }
  __syncthreads();
  for (int p0 = 0; p0 < P; p0 += LIST_THR) {
    const int p = p0 + tid;
    int s = p < P ? sel[p] : -1;
    if ((unsigned)s >= (unsigned)E) s = -1;
    int rank = 0;
    for (int e = 0; e < E; ++e) {
      const unsigned long long m = __ballot(s == e);
      if (s == e) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[wave][e] = __popcll(m);
    }
    __syncthreads();
    if (s >= 0) {
      int o = base[s] + rank;
      for (int w = 0; w < wave; ++w) o += wcnt[w][s];
      if (o < P) list[o] = p;
    }
    __syncthreads();
    if (tid < E) {
      int t = 0;
      for (int w = 0; w < LIST_THR / 64; ++w) t += wcnt[w][tid];
      base[tid] += t;
    }
    __syncthreads();
  }
}

// ---- grouped linear ------------------------------------------------------------------------------------------------------
struct MoeLinearParams {
  const void* x; int ldx, x_shift;       // pair p reads row p >> x_shift of x
  const void* w; const void* w2;         // [E][N][K]; SWIGLU: w = gate_e, w2 = up_e
  int N, K, E;
  const int32_t* meta; const int32_t* list;
  void* out; int ldo, rnd;               // out[p][n]
};

// acc += A B for one 16 x 16 tile over 32 values of k: lane (c = lane & 15, q = lane >> 4) holds x[row c][k0 + 8 q + j] and
// W[col c][k0 + 8 q + j], j < 8 -- the operand layout of v_mfma_f32_16x16x32_{bf16,f16}.  float32 rows: eight steps of
// v_mfma_f32_16x16x4_f32, step j taking element j of both (any one-to-one pairing of k is the same sum)
template <typename T, typename W>
__device__ __forceinline__ f32x4 tile_step(const T* xp, const u32x4& wv, const float (&wf)[8], f32x4 acc) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 a = *(const f32x4*)xp, b = *(const f32x4*)(xp + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], wf[j], acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], wf[4 + j], acc, 0, 0, 0);
    return acc;
  } else {
    return mfma16<T>(*(const u32x4*)xp, wv, acc);
  }
}

// grid (N / 64, E): a workgroup owns 64 output columns of one expert, a wave 16 of them over the whole K.  The expert's pairs
// come through its list in row tiles of 16; RT of them share one pass over the weight tile (a decode step has at most one).
template <typename T, typename W, bool SWIGLU>
__global__ __launch_bounds__(NTHR) void moe_linear_kernel(MoeLinearParams p) {
  const int e = blockIdx.y;
  const int cnt = p.meta[e];
  if (cnt <= 0) return;
  const int32_t* list = p.list + p.meta[p.E + e];
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
  const int K = p.K;
  const W* wrow = (const W*)p.w + ((size_t)e * p.N + n0 + c) * K + 8 * q;
  const W* wrow2 = SWIGLU ? (const W*)p.w2 + ((size_t)e * p.N + n0 + c) * K + 8 * q : nullptr;
  for (int base = 0; base < cnt; base += 16 * RT) {
    const T* xr[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int i = min(base + t * 16 + c, cnt - 1);                 // (rows past the list repeat its last pair; never stored)
      xr[t] = (const T*)p.x + (size_t)(list[i] >> p.x_shift) * p.ldx + 8 * q;
    }
    f32x4 acc[RT], acc2[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) { acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int k0 = 0; k0 < K; k0 += 32) {
      const u32x4 wv = *(const u32x4*)(wrow + k0);
      u32x4 wv2 = wv;
      if constexpr (SWIGLU) wv2 = *(const u32x4*)(wrow2 + k0);
      float wf[8], wf2[8];
      if constexpr (sizeof(T) == 4) { widen8<W>(wv, wf); if constexpr (SWIGLU) widen8<W>(wv2, wf2); }
#pragma unroll
      for (int t = 0; t < RT; ++t)
        if (base + t * 16 < cnt) {
          acc[t] = tile_step<T, W>(xr[t] + k0, wv, wf, acc[t]);
          if constexpr (SWIGLU) acc2[t] = tile_step<T, W>(xr[t] + k0, wv2, wf2, acc2[t]);
        }
    }
    // C layout: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = base + t * 16 + q * 4 + r;
        if (i < cnt) {
          float v = linear_value<T>(acc[t][r], false, nullptr, 0, 0, p.rnd);
          if constexpr (SWIGLU) v = swiglu_value<T>(v, linear_value<T>(acc2[t][r], false, nullptr, 0, 0, p.rnd), p.rnd);
          ((T*)p.out)[(size_t)list[i] * p.ldo + n0 + c] = store_act<T>(v, p.rnd);
        }
      }
  }
}

// ---- combine -------------------------------------------------------------------------------------------------------------
// out[row] = resid ? T(resid[row] + r) : r with r = T(T(y_a s_a) + T(y_b s_b)) (k = 1: T(y_a s_a)); y[row k + j][H]
template <typename T>
__global__ __launch_bounds__(NTHR) void moe_combine_kernel(const T* y, const T* score, int k, const T* resid, int ldr, T* out, int ldo,
                                                           int R, int H, int rnd) {
#pragma clang fp contract(off)
  const size_t total = (size_t)R * H;
  for (size_t i = (size_t)blockIdx.x * NTHR + threadIdx.x; i < total; i += (size_t)gridDim.x * NTHR) {
    const size_t row = i / H;
    const int n = (int)(i - row * H);
    float r = rounded<T>(to_f32<T>(y[row * k * H + n]) * to_f32<T>(score[row * k]), rnd);
    if (k == 2) {
      const float r2 = rounded<T>(to_f32<T>(y[(row * k + 1) * H + n]) * to_f32<T>(score[row * k + 1]), rnd);
      r = rounded<T>(r + r2, rnd);
    }
    if (resid != nullptr) r = rounded<T>(to_f32<T>(resid[row * ldr + n]) + r, rnd);
    out[row * ldo + n] = store_act<T>(r, rnd);
  }
}

int check_types(int act, int wdt, const char* who) {
  if (act != MI_F32 && act != MI_BF16 && act != MI_F16) return fail(MI_ERR_INVALID, std::string(who) + ": bad activation dtype");
  if (wdt != MI_BF16 && wdt != MI_F16) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": expert weights must be bf16 or f16");
  if (act != MI_F32 && act != wdt) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": 16-bit activations need weights of the same dtype");
  return MI_OK;
}

// the four (activation, weight) pairs: f(Tag<T>, Tag<W>)
template <typename X> struct Tag { using type = X; };
template <class F>
void with_types(int act, int wdt, F f) {
  if (act == MI_BF16) f(Tag<bf16>{}, Tag<bf16>{});
  else if (act == MI_F16) f(Tag<f16>{}, Tag<f16>{});
  else if (wdt == MI_BF16) f(Tag<float>{}, Tag<bf16>{});
  else f(Tag<float>{}, Tag<f16>{});
}

}  // namespace

int launch_moe_route(const MoeRouteCall& c, hipStream_t st) {
  MI_TRY(check_types(c.act, c.wdt, "moe_route"));
  if (!c.xn || !c.wg || !c.sel || !c.score || !c.meta || !c.list || c.R < 1) return fail(MI_ERR_INVALID, "moe_route: bad argument");
  if (c.E < 1 || c.E > MOE_MAX_EXPERTS) return fail(MI_ERR_UNSUPPORTED, "moe_route: 1 to 16 experts");
  if (c.k < 1 || c.k > 2 || c.k > c.E) return fail(MI_ERR_UNSUPPORTED, "moe_route: 1 or 2 experts per token, at most the expert count");
  if (c.H < 64 || c.H % 64 != 0 || c.ldx < c.H || c.ldx % 8 != 0) return fail(MI_ERR_UNSUPPORTED, "moe_route: the hidden size must be a multiple of 64");
  if ((long long)c.R * c.k > (1LL << 30)) return fail(MI_ERR_UNSUPPORTED, "moe_route: too many rows");
  if ((uintptr_t)c.xn % 16 != 0 || (uintptr_t)c.wg % 16 != 0) return fail(MI_ERR_INVALID, "moe_route: misaligned buffer");
  const dim3 grid((c.R + NTHR / 64 - 1) / (NTHR / 64));
  with_types(c.act, c.wdt, [&](auto t, auto w) {
    using T = typename decltype(t)::type; using W = typename decltype(w)::type;
    hipLaunchKernelGGL((moe_gate_kernel<T, W>), grid, dim3(NTHR), 0, st, (const T*)c.xn, c.ldx, c.R, c.H, c.rnd, (const W*)c.wg, c.E, c.k,
                       c.sel, (T*)c.score);
  });
  MI_HIP(hipGetLastError());
  hipLaunchKernelGGL(moe_lists_kernel, dim3(1), dim3(LIST_THR), 0, st, (const int32_t*)c.sel, c.R * c.k, c.E, c.meta, c.list);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_moe_linear(const MoeLinearCall& c, hipStream_t st) {
  MI_TRY(check_types(c.act, c.wdt, "moe_linear"));
  if (!c.x || !c.w || !c.meta || !c.list || !c.out || (c.swiglu && !c.w2)) return fail(MI_ERR_INVALID, "moe_linear: null argument");
  if (c.E < 1 || c.E > MOE_MAX_EXPERTS) return fail(MI_ERR_UNSUPPORTED, "moe_linear: 1 to 16 experts");
  if (c.N < 64 || c.N % 64 != 0 || c.K < 64 || c.K % 64 != 0) return fail(MI_ERR_UNSUPPORTED, "moe_linear: N and K must be multiples of 64");
  if (c.ldx < c.K || c.ldx % 8 != 0 || c.ldo < c.N || c.x_shift < 0 || c.x_shift > 1) return fail(MI_ERR_INVALID, "moe_linear: bad row stride");
  if ((uintptr_t)c.x % 16 != 0 || (uintptr_t)c.w % 16 != 0 || (uintptr_t)c.w2 % 16 != 0) return fail(MI_ERR_INVALID, "moe_linear: misaligned buffer");
  MoeLinearParams p{};
  p.x = c.x; p.ldx = c.ldx; p.x_shift = c.x_shift; p.w = c.w; p.w2 = c.w2; p.N = c.N; p.K = c.K; p.E = c.E;
  p.meta = c.meta; p.list = c.list; p.out = c.out; p.ldo = c.ldo; p.rnd = c.rnd;
  const dim3 grid(c.N / 64, c.E);
  with_types(c.act, c.wdt, [&](auto t, auto w) {
    using T = typename decltype(t)::type; using W = typename decltype(w)::type;
    if (c.swiglu) hipLaunchKernelGGL((moe_linear_kernel<T, W, true>), grid, dim3(NTHR), 0, st, p);
    else hipLaunchKernelGGL((moe_linear_kernel<T, W, false>), grid, dim3(NTHR), 0, st, p);
  });
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_moe_combine(const void* y, const void* score, int k, const void* resid, int ldr, void* out, int ldo, int R, int H,
                       int act, int rnd, hipStream_t st) {
  if (!y || !score || !out || R < 1 || H < 1 || k < 1 || k > 2 || ldo < H || (resid && ldr < H)) return fail(MI_ERR_INVALID, "moe_combine: bad argument");
  if (act != MI_F32 && act != MI_BF16 && act != MI_F16) return fail(MI_ERR_INVALID, "moe_combine: bad activation dtype");
  const size_t total = (size_t)R * H;
  const dim3 grid((unsigned)std::min<size_t>((total + NTHR - 1) / NTHR, (size_t)1 << 16));
  switch (act) {
    case MI_F32: hipLaunchKernelGGL(moe_combine_kernel<float>, grid, dim3(NTHR), 0, st, (const float*)y, (const float*)score, k, (const float*)resid, ldr, (float*)out, ldo, R, H, rnd); break;
    case MI_BF16: hipLaunchKernelGGL(moe_combine_kernel<bf16>, grid, dim3(NTHR), 0, st, (const bf16*)y, (const bf16*)score, k, (const bf16*)resid, ldr, (bf16*)out, ldo, R, H, rnd); break;
    case MI_F16: hipLaunchKernelGGL(moe_combine_kernel<f16>, grid, dim3(NTHR), 0, st, (const f16*)y, (const f16*)score, k, (const f16*)resid, ldr, (f16*)out, ldo, R, H, rnd); break;
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
