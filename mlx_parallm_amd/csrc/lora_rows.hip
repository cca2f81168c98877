// lora_rows.hip -- the LoRA term of a step, each row with the adapter it names (lora_rows.h).  Unfused on purpose: the term
// lives outside the linear kernels' parameter blocks (a per-lane B pointer inside their epilogues would cost registers in
// kernels that sit at an occupancy edge), behind a plain-store launch of the base linear.
//   lora_down_by_row_kernel    t = x A of each row's own adapter, for every part of the fused matrix the adapter covers
//   lora_up_add_by_row_kernel  y += T(scale (t B)) with the row's own B, rank and scale; with a residual operand also h += y'
//                              <T, true> (launched only for a table that holds a DoRA entry): an entry with a gain then ends its
//                              row with y' = T(T(g[n]) y')
//   dora_gain_kernel           g[n] = m[n] / ||W[n] + scale (A B)^T[n]|| of one part, once when a DoRA entry is set
//   swiglu_rows_kernel         gate|up with an adapted range: the linear stores T(acc) to a [rows][2 I] buffer (EPI_STORE), the
//                              up-add puts the terms on it and this kernel writes act = silu(gate) * up with the rounding
//                              points of the fused epilogues (gemv_v1.hip EPI_SWIGLU: sig, g * sig, s * u, each rounded to
//                              the activation dtype)
#include <algorithm>
#include <atomic>

#include "linear_epilogue.h"
#include "lora_rows.h"

namespace mi {

namespace {

constexpr int NTHR = 256;
constexpr int UP_COLS = 4 * NTHR;      // output columns of one workgroup of the up-add

struct DownRowsParams {
  const void* x; int ldx; int K;
  int pro; const void* norm_w; float eps; int rnd;
  const AdapterPart* table; const int32_t* row_adapter; int n_parts;
  float* t;
};

// t[m][part][j] = sum_k xin[m][k] * A[k][j], A = the part's factor of row m's adapter; xin = the (normalised) row, staged once
// in LDS.  The sum of a column: thread tid adds k = tid, tid + 256, ... in ascending order, then the wave sum, then the four
// waves in order.  A row without an adapter leaves at once; a part its adapter does not cover is skipped (both are uniform
// over the workgroup).
template <typename AT>
__global__ __launch_bounds__(NTHR) void lora_down_by_row_kernel(DownRowsParams p) {
  extern __shared__ float xs[];      // [K]
  __shared__ float rs_sh;
  __shared__ float red[4];
  __shared__ float red16[4][16];
  const int m = blockIdx.x;
  const int ad = p.row_adapter[m];
  if (ad < 0 || ad >= LORA_TABLE_COLS) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AT* x = (const AT*)p.x + (size_t)m * p.ldx;
  for (int k = tid; k < p.K; k += NTHR) xs[k] = to_f32(x[k]);          // (each thread reads back only what it wrote)
  if (p.pro == PRO_NORM) {
    float ss = 0.f;
    for (int k = tid; k < p.K; k += NTHR) { const float v = xs[k]; ss += v * v; }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    if (tid == 0) rs_sh = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)p.K + p.eps);
    __syncthreads();
    const float rs = rs_sh;
    for (int k = tid; k < p.K; k += NTHR) {
      const AT xn = store_act<AT>(xs[k] * rs, p.rnd);
      xs[k] = to_f32(store_act<AT>(to_f32(xn) * to_f32(((const AT*)p.norm_w)[k]), p.rnd));
    }
  }
#pragma unroll 1
  for (int r = 0; r < p.n_parts; ++r) {
    const AdapterPart ap = p.table[r * LORA_TABLE_COLS + ad];
    const float* A = ap.a;
    const int rk = min(ap.rank, 64);
    if (A == nullptr) continue;
    float* tr = p.t + (size_t)m * LORA_ROWS_T_LD + r * 64;
    for (int j0 = 0; j0 < rk; j0 += 16) {
      float s[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) s[j] = 0.f;
      const bool vec = (rk % 4 == 0) && (j0 + 16 <= rk);
      if (vec) {
#pragma unroll 4
        for (int k = tid; k < p.K; k += NTHR) {
          const float vv = xs[k];
          const float4* ar = (const float4*)(A + (size_t)k * rk + j0);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 a4 = ar[q];
            s[4 * q + 0] = fmaf(vv, a4.x, s[4 * q + 0]);
            s[4 * q + 1] = fmaf(vv, a4.y, s[4 * q + 1]);
            s[4 * q + 2] = fmaf(vv, a4.z, s[4 * q + 2]);
            s[4 * q + 3] = fmaf(vv, a4.w, s[4 * q + 3]);
          }
        }
      } else {
        for (int k = tid; k < p.K; k += NTHR) {
          const float vv = xs[k];
          const float* ar = A + (size_t)k * rk + j0;
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (j0 + j < rk) s[j] = fmaf(vv, ar[j], s[j]);
        }
      }
      __syncthreads();                 // (red16 of the previous group has been read)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float w = wave_sum(s[j]);
        if (lane == 0) red16[wave][j] = w;
      }
      __syncthreads();
      if (tid < 16 && j0 + tid < rk) tr[j0 + tid] = red16[0][tid] + red16[1][tid] + red16[2][tid] + red16[3][tid];
    }
  }
}

struct UpRowsParams {
  const AdapterPart* table; const int32_t* row_adapter; const float* t;
  int row0[3], n[3];
  int rnd;
};

// Part blockIdx.y, columns [blockIdx.z * UP_COLS, + UP_COLS) of token row blockIdx.x, consecutive lanes on consecutive columns:
//   y[m][row0 + n] = T(y + T(scale * sum_j t[m][part][j] B[j][n]))      lora_dot and lora_add (linear_epilogue.h)
// with B, rank and scale of the row's own adapter.  resid != null: h[m][n] = T(h[m][n] + y') instead of the store to y (the
// residual add of EPI_RESID, kernels.h), for EVERY row -- a row whose adapter does not cover the part adds the stored y.
//
// GAIN (DoRA): an entry with a gain ends its row with y' = T(T(g[n]) * y') ahead of the residual add -- g rounded to the call's
// T here, because one entry serves calls of different T (layer 0's q|k|v of the float32-KV mode rounds to 16 bits, every later
// linear does not).  The product and the residual add stay two roundings (gain_mul: contract off).  Rows whose entry has no
// gain, and rows without an entry, take no multiplication: their bits are those of the plain instantiation.
template <typename AT>
__device__ __forceinline__ float gain_mul(float g, float v, int rnd) {
#pragma clang fp contract(off)
  const float gt = rounded<AT>(g, rnd);
  const float pr = gt * v;
  return rounded<AT>(pr, rnd);
}

template <typename AT, bool GAIN>
__global__ __launch_bounds__(NTHR) void lora_up_add_by_row_kernel(UpRowsParams p, AT* y, int ldy, AT* resid, int ldr) {
  const int m = blockIdx.x, r = blockIdx.y;
  const int ln = p.n[r];
  const int n0 = blockIdx.z * UP_COLS;
  if (n0 >= ln) return;
  const int ad = p.row_adapter[m];
  AdapterPart ap{};
  if (ad >= 0 && ad < LORA_TABLE_COLS) ap = p.table[r * LORA_TABLE_COLS + ad];
  const float* lb = ap.b;
  if (lb == nullptr && resid == nullptr) return;
  const int rk = min(ap.rank, 64);
  const float sc = ap.scale;
  const float* tt = p.t + (size_t)m * LORA_ROWS_T_LD + r * 64;
  const int n1 = min(ln, n0 + UP_COLS);
  for (int n = n0 + threadIdx.x; n < n1; n += NTHR) {
    AT* o = y + (size_t)m * ldy + p.row0[r] + n;
    float v = to_f32(*o);
    if (lb != nullptr) v = lora_add<AT>(v, sc, lora_dot(tt, lb + n, ln, rk), p.rnd, RND_NONE);
    if constexpr (GAIN) {
      if (lb != nullptr && ap.gain != nullptr) v = gain_mul<AT>(ap.gain[n], v, p.rnd);
    }
    if (resid != nullptr) {
      AT* h = resid + (size_t)m * ldr + p.row0[r] + n;
      *h = store_act<AT>(to_f32(*h) + v, p.rnd);
    } else {
      *o = from_f32<AT>(v);
    }
  }
}

// 16 bytes of activations; the alignment is the element's own, so any row stride is a legal address (global loads and
// stores of gfx950 take unaligned dwordx4)
template <typename AT>
struct Vec16 {
  static constexpr int N = 16 / (int)sizeof(AT);
  typedef AT type __attribute__((ext_vector_type(16 / sizeof(AT)), aligned(sizeof(AT))));
};

// out[m][n] = T(T(g * T(sigmoid(g))) * u), g = x[m][n], u = x[m][I + n]  (llama.py:165; g and u are already T-rounded)
template <typename AT>
__global__ __launch_bounds__(NTHR) void swiglu_rows_kernel(const AT* x, int ldx, AT* out, int ldo, int M, int I, int rnd) {
  constexpr int V = Vec16<AT>::N;
  typedef typename Vec16<AT>::type vec;
  const size_t per_row = (size_t)(I / V), total = (size_t)M * per_row;
  for (size_t i = (size_t)blockIdx.x * NTHR + threadIdx.x; i < total; i += (size_t)gridDim.x * NTHR) {
    const size_t m = i / per_row;
    const int n = (int)(i - m * per_row) * V;
    const AT* row = x + m * (size_t)ldx + n;
    const vec gv = *(const vec*)row;
    const vec uv = *(const vec*)(row + I);
    vec ov;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      ov[j] = from_f32<AT>(swiglu_value<AT, true>(to_f32<AT>(gv[j]), to_f32<AT>(uv[j]), rnd));      // (the float64 sigmoid)
    }
    *(vec*)(out + m * (size_t)ldo + n) = ov;
  }
}

struct GainParams {
  const void* w; int layout, K, row0, n;
  const float* a; const float* b; const float* m; int rank; float scale;
  float* gain;
};

// W[row][k] of a dense 16-bit matrix, row-major or tile-major (repack.hip)
template <typename WT>
__device__ __forceinline__ float dense16_at(const void* w, int layout, size_t row, int k, int K) {
  if (layout == 1) return to_f32(*(const WT*)((const char*)w + tiled_piece_dense16(row, k & ~7, K) + (size_t)(k & 7) * sizeof(WT)));
  return to_f32(((const WT*)w)[row * (size_t)K + k]);
}

// DoRA's gain of the 16 rows [16 blockIdx.x, + 16) of a part: gain[i] = m[i] / sqrt(sum_k d[i][k]^2),
//   d[i][k] = W[row0 + i][k] + sum_j A[k][j] . (scale . B[j][i]).
// scale . B of the tile waits in LDS (one rounding each).  Thread tid owns k = tid, tid + 256, ...: per k, d starts from W and
// takes the rank terms as fmaf in ascending j; d^2 joins the thread's running sum by fmaf, in ascending k.  Then the wave sum
// (wave_sum: four row rotations, (a + b) + (c + d)), then the four waves in order.  No atomics, nothing depends on the layout
// of W or on the grid: the same inputs give the same bits.  The longest chain of additions behind one norm is
// ceil(K / 256) + 9; the error bound that follows from it stands in DESIGN.md §5 ("DoRA").
// A norm of 0 (or one that is not finite) leaves NaN: the host refuses the adapter.
template <typename WT>
__global__ __launch_bounds__(NTHR) void dora_gain_kernel(GainParams p) {
  __shared__ float sb[64][16];
  __shared__ float red[4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int rows = min(16, p.n - n0);
  const int rk = min(p.rank, 64);
  for (int e = tid; e < rk * 16; e += NTHR) {
    const int j = e >> 4, i = e & 15;
    sb[j][i] = i < rows ? p.scale * p.b[(size_t)j * p.n + n0 + i] : 0.f;
  }
  __syncthreads();
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const size_t r0 = (size_t)p.row0 + n0;
  for (int k = tid; k < p.K; k += NTHR) {
    float d[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = dense16_at<WT>(p.w, p.layout, r0 + min(i, rows - 1), k, p.K);   // (a ragged tile repeats its last row)
    const float* ar = p.a + (size_t)k * rk;
#pragma unroll 4
    for (int j = 0; j < rk; ++j) {
      const float av = ar[j];
#pragma unroll
      for (int i = 0; i < 16; ++i) d[i] = fmaf(av, sb[j][i], d[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = fmaf(d[i], d[i], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float w = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = w;
  }
  __syncthreads();
  if (tid < rows) {
    const float tot = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    const float denom = sqrtf(tot);
    p.gain[n0 + tid] = (denom > 0.f && denom <= 3.0e38f) ? p.m[n0 + tid] / denom : __builtin_nanf("");
  }
}

int check_call(const LoraRowsCall& c, const char* who) {
  if (c.table == nullptr || c.row_adapter == nullptr || c.t == nullptr) return fail(MI_ERR_INVALID, std::string(who) + ": null argument");
  if (c.M < 1) return fail(MI_ERR_INVALID, std::string(who) + ": no rows");
  if (c.n_parts < 1 || c.n_parts > 3) return fail(MI_ERR_INVALID, std::string(who) + ": 1 to 3 parts");
  if (c.act != MI_F32 && c.act != MI_BF16 && c.act != MI_F16) return fail(MI_ERR_INVALID, std::string(who) + ": bad activation dtype");
  return MI_OK;
}

}  // namespace

int launch_lora_down_by_row(const LoraRowsCall& c, const void* x, int ldx, int pro, const void* norm_w, float eps,
                            hipStream_t st) {
  MI_TRY(check_call(c, "lora_down_by_row"));
  if (x == nullptr || c.K < 1 || ldx < c.K || (pro == PRO_NORM && norm_w == nullptr)) return fail(MI_ERR_INVALID, "lora_down_by_row: bad argument");
  const size_t lds = (size_t)c.K * sizeof(float);
  if (lds > 144 * 1024) return fail(MI_ERR_UNSUPPORTED, "lora_down_by_row: K above 36864");
  if (lds > 48 * 1024) {               // (the statics ride beside the row: opt in well below the 64 KiB line)
    static std::atomic<bool> opted[64];
    MI_TRY(lds_opt_in(opted, {(const void*)lora_down_by_row_kernel<float>, (const void*)lora_down_by_row_kernel<bf16>,
                              (const void*)lora_down_by_row_kernel<f16>}, 144 * 1024));
  }
  DownRowsParams p{};
  p.x = x; p.ldx = ldx; p.K = c.K; p.pro = pro; p.norm_w = norm_w; p.eps = eps; p.rnd = c.rnd;
  p.table = c.table; p.row_adapter = c.row_adapter; p.n_parts = c.n_parts; p.t = c.t;
  const dim3 grid(c.M), block(NTHR);
  switch (c.act) {
    case MI_F32: hipLaunchKernelGGL(lora_down_by_row_kernel<float>, grid, block, lds, st, p); break;
    case MI_BF16: hipLaunchKernelGGL(lora_down_by_row_kernel<bf16>, grid, block, lds, st, p); break;
    case MI_F16: hipLaunchKernelGGL(lora_down_by_row_kernel<f16>, grid, block, lds, st, p); break;
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_lora_up_add_by_row(const LoraRowsCall& c, void* y, int ldy, void* resid, int ldr, hipStream_t st) {
  MI_TRY(check_call(c, "lora_up_add_by_row"));
  if (y == nullptr) return fail(MI_ERR_INVALID, "lora_up_add_by_row: null output");
  if (resid != nullptr && (c.n_parts != 1 || c.row0[0] != 0 || ldr < c.n[0])) return fail(MI_ERR_INVALID, "lora_up_add_by_row: a residual goes with one part at column 0");
  int widest = 0;
  for (int i = 0; i < c.n_parts; ++i) {
    if (c.n[i] < 1 || c.row0[i] < 0 || (long long)c.row0[i] + c.n[i] > ldy) return fail(MI_ERR_INVALID, "lora_up_add_by_row: a part lies outside the row");
    widest = std::max(widest, c.n[i]);
  }
  UpRowsParams p{};
  p.table = c.table; p.row_adapter = c.row_adapter; p.t = c.t; p.rnd = c.rnd;
  for (int i = 0; i < c.n_parts; ++i) { p.row0[i] = c.row0[i]; p.n[i] = c.n[i]; }
  const dim3 grid(c.M, c.n_parts, (widest + UP_COLS - 1) / UP_COLS), block(NTHR);
  if (c.gain) {                        // a table that holds a DoRA entry; every other call launches the plain instantiation
    switch (c.act) {
      case MI_BF16: hipLaunchKernelGGL((lora_up_add_by_row_kernel<bf16, true>), grid, block, 0, st, p, (bf16*)y, ldy, (bf16*)resid, ldr); break;
      case MI_F16: hipLaunchKernelGGL((lora_up_add_by_row_kernel<f16, true>), grid, block, 0, st, p, (f16*)y, ldy, (f16*)resid, ldr); break;
      case MI_F32: hipLaunchKernelGGL((lora_up_add_by_row_kernel<float, true>), grid, block, 0, st, p, (float*)y, ldy, (float*)resid, ldr); break;
    }
  } else {
    switch (c.act) {
      case MI_BF16: hipLaunchKernelGGL((lora_up_add_by_row_kernel<bf16, false>), grid, block, 0, st, p, (bf16*)y, ldy, (bf16*)resid, ldr); break;
      case MI_F16: hipLaunchKernelGGL((lora_up_add_by_row_kernel<f16, false>), grid, block, 0, st, p, (f16*)y, ldy, (f16*)resid, ldr); break;
      case MI_F32: hipLaunchKernelGGL((lora_up_add_by_row_kernel<float, false>), grid, block, 0, st, p, (float*)y, ldy, (float*)resid, ldr); break;
    }
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_dora_gain(const LinearW& W, int row0, int n, const float* A, const float* B, const float* m, int rank, float scale,
                     float* gain, hipStream_t st) {
  if (W.w == nullptr || A == nullptr || B == nullptr || m == nullptr || gain == nullptr) return fail(MI_ERR_INVALID, "dora_gain: null argument");
  if (W.wk != WK_BF16 && W.wk != WK_F16) return fail(MI_ERR_UNSUPPORTED, "dora_gain: dense bf16 / f16 weights only");
  if (rank < 1 || rank > 64) return fail(MI_ERR_INVALID, "dora_gain: rank outside 1..64");
  if (W.K < 1 || W.N < 1 || n < 1 || row0 < 0 || (long long)row0 + n > W.N) return fail(MI_ERR_INVALID, "dora_gain: the rows lie outside the matrix");
  if (W.layout != 0 && W.layout != 1) return fail(MI_ERR_INVALID, "dora_gain: bad layout");
  if (W.layout == 1 && (W.K % 32 != 0 || W.N % 16 != 0)) return fail(MI_ERR_INVALID, "dora_gain: a tile-major matrix has N % 16 == 0 and K % 32 == 0");
  if ((uintptr_t)W.w % 16 != 0 || (uintptr_t)A % 4 != 0 || (uintptr_t)B % 4 != 0 || (uintptr_t)m % 4 != 0 || (uintptr_t)gain % 4 != 0)
    return fail(MI_ERR_INVALID, "dora_gain: misaligned buffer");
  GainParams p{W.w, W.layout, W.K, row0, n, A, B, m, rank, scale, gain};
  const dim3 grid((n + 15) / 16), block(NTHR);
  if (W.wk == WK_BF16) hipLaunchKernelGGL(dora_gain_kernel<bf16>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(dora_gain_kernel<f16>, grid, block, 0, st, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_swiglu_rows(const void* x, int ldx, void* out, int ldo, int M, int I, int act, int rnd, hipStream_t st) {
  if (x == nullptr || out == nullptr || M < 1 || I < 1 || (rnd != RND_NONE && rnd != RND_BF16 && rnd != RND_F16))
    return fail(MI_ERR_INVALID, "swiglu_rows: bad argument");
  if (act != MI_F32 && act != MI_BF16 && act != MI_F16) return fail(MI_ERR_INVALID, "swiglu_rows: bad activation dtype");
  if (I % 8 != 0) return fail(MI_ERR_UNSUPPORTED, "swiglu_rows: the intermediate size must be a multiple of 8");
  if ((long long)ldx < 2LL * I || ldo < I) return fail(MI_ERR_INVALID, "swiglu_rows: a row stride is shorter than its row");
  const size_t es = dtype_size(act);
  if ((uintptr_t)x % es != 0 || (uintptr_t)out % es != 0) return fail(MI_ERR_INVALID, "swiglu_rows: misaligned buffer");
  const size_t pieces = (size_t)M * (size_t)(I / (int)(16 / es));
  const unsigned grid = (unsigned)std::min<size_t>((pieces + NTHR - 1) / NTHR, (size_t)1 << 16);
  switch (act) {
    case MI_F32: hipLaunchKernelGGL(swiglu_rows_kernel<float>, dim3(grid), dim3(NTHR), 0, st, (const float*)x, ldx, (float*)out, ldo, M, I, rnd); break;
    case MI_BF16: hipLaunchKernelGGL(swiglu_rows_kernel<bf16>, dim3(grid), dim3(NTHR), 0, st, (const bf16*)x, ldx, (bf16*)out, ldo, M, I, rnd); break;
    case MI_F16: hipLaunchKernelGGL(swiglu_rows_kernel<f16>, dim3(grid), dim3(NTHR), 0, st, (const f16*)x, ldx, (f16*)out, ldo, M, I, rnd); break;
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
