// lora.hip -- the kernels that carry LoRA to every projection of a block (mlx-lm LoRALinear on whatever
// lora_parameters.keys names: rl_training/lora_init.py:72,95-96).
//
// The streaming kernels add up to TWO adapted row ranges of a fused matrix in their plain-store epilogues (LinearW::lora_*[2]).
// What they do not cover lives here, outside their parameter blocks, so that none of them changes:
//   swiglu_rows_kernel   gate|up with an adapted range: the linear stores T(acc) + the LoRA terms to a [rows][2 I] buffer
//                        (EPI_STORE), this kernel writes act = silu(gate) * up with the rounding points of the fused epilogues
//                        (gemv_v1.hip EPI_SWIGLU: sig, g * sig, s * u, each rounded to the activation dtype)
//   lora_down3_kernel    q|k|v with all three projections adapted: t = x A for the three ranges in one launch, x and its
//                        RMSNorm read once per row
//   lora_up_add3_kernel  y += T(scale (t B)) on up to three ranges of a stored output: the third range behind a streaming
//                        launch, all three behind the prefill tile GEMM
#include <algorithm>

#include "linear_epilogue.h"

namespace mi {

namespace {

constexpr int NTHR = 256;

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

struct Down3Params {
  const void* x; int ldx; int K;
  int pro; const void* norm_w; float eps; int rnd;
  const float* a[3]; int rank[3];
  float* t[3]; int t_ld[3];          // t[r][m * t_ld[r] + j]
};

// t_r[m][j] = sum_k xin[m][k] * A_r[k][j] for the three ranges; xin = the (normalised) row, staged once in LDS.  The sum of a
// column is lora_down_kernel's (gemv_v1.hip): thread tid adds k = tid, tid + 256, ... in ascending order, then the wave sum,
// then the four waves in order -- t is the same bits whichever of the two kernels made it.
template <typename AT>
__global__ __launch_bounds__(NTHR) void lora_down3_kernel(Down3Params p) {
  extern __shared__ float xs[];      // [K]
  __shared__ float rs_sh;
  __shared__ float red[4];
  __shared__ float red16[4][16];
  const int m = blockIdx.x;
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
  for (int r = 0; r < 3; ++r) {
    const float* A = p.a[r];
    const int rk = p.rank[r];
    if (A == nullptr) continue;
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
      if (tid < 16 && j0 + tid < rk)
        p.t[r][(size_t)m * p.t_ld[r] + j0 + tid] = red16[0][tid] + red16[1][tid] + red16[2][tid] + red16[3][tid];
    }
  }
}

struct Up3Params {
  const float* b[3]; const float* t[3]; int t_ld[3];
  int row0[3], n[3], rank[3]; float scale[3];
  int rnd;
};

// y[m][row0 + n] = T(y + T(scale * sum_j t[m][j] B[j][n])) for range blockIdx.y: lora_up_add_kernel's arithmetic (gemv_v1.hip)
template <typename AT>
__global__ __launch_bounds__(NTHR) void lora_up_add3_kernel(Up3Params p, AT* y, int ldy) {
  const int m = blockIdx.x, r = blockIdx.y;
  const float* lb = p.b[r];
  if (lb == nullptr) return;
  const int ln = p.n[r], rk = p.rank[r];
  const float sc = p.scale[r];
  const float* tt = p.t[r] + (size_t)m * p.t_ld[r];
  for (int n = threadIdx.x; n < ln; n += NTHR) {
    const float z = lora_dot(tt, lb + n, ln, rk);
    AT* o = y + (size_t)m * ldy + p.row0[r] + n;
    *o = from_f32<AT>(lora_add<AT>(to_f32(*o), sc, z, p.rnd, RND_NONE));
  }
}

}  // namespace

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

int launch_lora_down3(const LinearW& W, const LoraRange& r3, const GemvCall& c, float* t, int t_ld, float* t3, int t3_ld,
                      hipStream_t st) {
  if (c.M < 1) return fail(MI_ERR_INVALID, "lora_down3: no rows");
  const size_t lds = (size_t)W.K * sizeof(float);
  if (lds > 60 * 1024) return fail(MI_ERR_UNSUPPORTED, "lora_down3: K above 15360");
  Down3Params p{};
  p.x = c.x; p.ldx = c.ldx; p.K = W.K; p.pro = c.pro; p.norm_w = c.norm_w; p.eps = c.eps; p.rnd = c.rnd;
  for (int i = 0; i < 2; ++i) { p.a[i] = W.lora_a[i]; p.rank[i] = W.lora_rank[i]; p.t[i] = t + i * (t_ld / 2); p.t_ld[i] = t_ld; }
  p.a[2] = r3.a; p.rank[2] = r3.rank; p.t[2] = t3; p.t_ld[2] = t3_ld;
  const dim3 grid(c.M), block(NTHR);
  switch (c.act) {
    case MI_F32: hipLaunchKernelGGL(lora_down3_kernel<float>, grid, block, lds, st, p); break;
    case MI_BF16: hipLaunchKernelGGL(lora_down3_kernel<bf16>, grid, block, lds, st, p); break;
    case MI_F16: hipLaunchKernelGGL(lora_down3_kernel<f16>, grid, block, lds, st, p); break;
    default: return fail(MI_ERR_INVALID, "lora_down3: bad activation dtype");
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_lora_up_add3(const LinearW* W, const LoraRange& r3, const GemvCall& c, const float* t, int t_ld, const float* t3,
                        int t3_ld, hipStream_t st) {
  if (c.epi != EPI_STORE) return fail(MI_ERR_UNSUPPORTED, "lora_up_add3: plain store epilogue only");
  if (c.M < 1) return fail(MI_ERR_INVALID, "lora_up_add3: no rows");
  Up3Params p{};
  if (W != nullptr)
    for (int i = 0; i < 2; ++i) {
      p.b[i] = W->lora_b[i]; p.t[i] = t + i * (t_ld / 2); p.t_ld[i] = t_ld;
      p.row0[i] = W->lora_row0[i]; p.n[i] = W->lora_n[i]; p.rank[i] = W->lora_rank[i]; p.scale[i] = W->lora_scale[i];
    }
  p.b[2] = r3.b; p.t[2] = t3; p.t_ld[2] = t3_ld;
  p.row0[2] = r3.row0; p.n[2] = r3.n; p.rank[2] = r3.rank; p.scale[2] = r3.scale;
  p.rnd = c.rnd;
  const dim3 grid(c.M, 3), block(NTHR);
  switch (c.act) {
    case MI_BF16: hipLaunchKernelGGL(lora_up_add3_kernel<bf16>, grid, block, 0, st, p, (bf16*)c.out, c.ldo); break;
    case MI_F16: hipLaunchKernelGGL(lora_up_add3_kernel<f16>, grid, block, 0, st, p, (f16*)c.out, c.ldo); break;
    case MI_F32: hipLaunchKernelGGL(lora_up_add3_kernel<float>, grid, block, 0, st, p, (float*)c.out, c.ldo); break;
    default: return fail(MI_ERR_UNSUPPORTED, "lora_up_add3: bad activation dtype");
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
