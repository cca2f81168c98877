// lora_merge.hip -- a LoRA / DoRA adapter added into the base weights once, in checkpoint layout (mi_lora_merge), and MLX's
// affine quantiser on its own (mi_quantize_mlx).  No engine is involved: row-major tensors of a checkpoint go in and come out.
//
// The arithmetic restates three pieces of mlx-lm's PUBLISHED code; mlx-lm is not among this project's sources and could not be
// run, so every rounding point below is restated and unchecked against it:
//   LoRALinear.fuse           Wd = T(scale q + bias) of a quantised base (one float32 multiply-add, one rounding), else W;
//                             b' = T(s B^T), a' = T(A^T);  delta = T(b' a') (float32 sums);  Wm = T(Wd + delta)
//   DoRALinear.fuse           norm[n] = ||Wm[n, :]||_2 in float32;  W' = T((m[n] / norm[n]) Wm[n][k])
//   QuantizedLinear.from_linear   mx.quantize(W', 64, bits), as oracle/ref_quant.quantize restates it
// Kernels:
//   lora_merge_kernel     one workgroup per output row n: Wm[n][:] and, for DoRA, the row's gain
//   dora_scale_kernel     W'[n][k] = T(g[n] Wm[n][k])
//   quantize_mlx_kernel   one wave per (row, group of 64), one lane per element: scale, bias, codes, packed words
// Every sum has a fixed order (a thread's k ascending in strides of 256, wave_sum, the four waves in order; the rank terms in
// ascending j); there are no atomics and nothing depends on the grid: the same inputs give the same bits.
#include <cmath>
#include <vector>

#include "common.h"

using namespace mi;

namespace {

constexpr int NTHR = 256;
constexpr int GROUP = 64;

struct MergeParams {
  const void* w; const void* scales; const void* biases;      // W (N, K) of T, or the packed triple
  int N, K, rank;
  const float* a; const float* b; float s;                    // A (K, r), B (r, N)
  const float* m;                                             // (N,) or null
  void* out;                                                  // Wm (N, K) of T
  float* gain;                                                // (N,), written when m is given
};

// Every rounding to T below takes a float32 value that exists as such.  Left alone, hipcc fuses a float32 operation and the
// conversion to f16 behind it into one v_fma_mixlo_f16, which rounds once; bf16 has no such instruction, so the two dtypes
// would round differently and neither as the steps are written (a float32 operation, then the rounding to T).
template <typename T>
__device__ __forceinline__ T round_T(float v) {
  asm volatile("" : "+v"(v));
  return from_f32<T>(v);
}

// step 1: the base value in T.  Quantised: element k of a row sits in word k / (32 / BITS) at bit BITS (k % (32 / BITS)).
template <typename T, int BITS>
__device__ __forceinline__ float base_value(const MergeParams& p, size_t n, int k) {
  if constexpr (BITS == 0) {
    return to_f32(((const T*)p.w)[n * p.K + k]);
  } else {
    constexpr int PER = 32 / BITS;
    const uint32_t word = ((const uint32_t*)p.w)[n * (size_t)(p.K / PER) + k / PER];
    const float q = (float)((word >> ((k % PER) * BITS)) & ((1u << BITS) - 1u));
    const size_t g = n * (size_t)(p.K / GROUP) + k / GROUP;
    return to_f32(round_T<T>(fmaf(to_f32(((const T*)p.scales)[g]), q, to_f32(((const T*)p.biases)[g]))));
  }
}

// steps 2-5a for row n = blockIdx.x.  b'[j] waits in LDS; thread tid owns k = tid, tid + 256, ...
template <typename T, int BITS>
__global__ __launch_bounds__(NTHR) void lora_merge_kernel(MergeParams p) {
  __shared__ float sb[64];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = blockIdx.x;
  if (tid < p.rank) sb[tid] = to_f32(round_T<T>(p.s * p.b[(size_t)tid * p.N + n]));
  __syncthreads();
  T* out = (T*)p.out + n * p.K;
  float ss = 0.f;
  for (int k = tid; k < p.K; k += NTHR) {
    const float wd = base_value<T, BITS>(p, n, k);
    const float* ar = p.a + (size_t)k * p.rank;
    float d = 0.f;
    for (int j = 0; j < p.rank; ++j) d = fmaf(sb[j], to_f32(from_f32<T>(ar[j])), d);
    const float delta = to_f32(round_T<T>(d));
    const T wm = round_T<T>(wd + delta);
    out[k] = wm;
    ss = fmaf(to_f32(wm), to_f32(wm), ss);
  }
  if (p.m == nullptr) return;
  const float w = wave_sum(ss);
  if (lane == 0) red[wave] = w;
  __syncthreads();
  if (tid == 0) {
    const float norm = sqrtf(((red[0] + red[1]) + red[2]) + red[3]);
    p.gain[n] = (norm > 0.f && norm <= 3.0e38f) ? p.m[n] / norm : __builtin_nanf("");
  }
}

// step 5b
template <typename T>
__global__ __launch_bounds__(NTHR) void dora_scale_kernel(const T* wm, const float* gain, T* out, int K) {
#pragma clang fp contract(off)
  const size_t n = blockIdx.x;
  const float g = gain[n];
  for (int k = threadIdx.x; k < K; k += NTHR) out[n * K + k] = round_T<T>(g * to_f32(wm[n * K + k]));
}

__device__ __forceinline__ uint32_t or_down(uint32_t v, int lanes) {
  for (int o = 1; o < lanes; o <<= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// step 6: oracle/ref_quant.quantize(w, 64, BITS, T), operation for operation in float32 (IEEE division, rintf).  The codes come
// from the unrounded scale and bias; the stored scale and bias are rounded to T.
template <typename T, int BITS>
__global__ __launch_bounds__(NTHR) void quantize_mlx_kernel(const T* w, size_t groups, int K, uint32_t* packed, T* scales, T* biases) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const size_t gid = (size_t)blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6);
  if (gid >= groups) return;                                  // (the whole wave leaves)
  constexpr int PER = 32 / BITS;
  const float n_bins = (float)((1 << BITS) - 1);
  const float v = to_f32(w[gid * GROUP + lane]);              // (K % 64 == 0: the groups of all rows lie back to back)
  const float w_max = wave_max(v), w_min = -wave_max(-v);
  const bool mask = fabsf(w_min) > fabsf(w_max);
  float scale = fmaxf((w_max - w_min) / n_bins, 1e-7f);
  scale = mask ? scale : -scale;
  const float edge = mask ? w_min : w_max;
  const float q0 = rintf(edge / scale);
  if (q0 != 0.f) scale = edge / q0;
  const float bias = q0 == 0.f ? 0.f : edge;
  const float q = fminf(fmaxf(rintf((v - bias) / scale), 0.f), n_bins);
  const uint32_t word = or_down((uint32_t)q << ((lane % PER) * BITS), PER);
  if (lane % PER == 0) packed[gid * (GROUP / PER) + lane / PER] = word;
  if (lane == 0) {
    scales[gid] = from_f32<T>(scale);
    biases[gid] = from_f32<T>(bias);
  }
}

struct DeviceScope {                                          // the calls are stateless: the caller's current device comes back
  int prev = -1;
  int enter(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(MI_ERR_RUNTIME, "no HIP device available (this library has no CPU backend)");
    if (device < 0 || device >= ndev) return fail(MI_ERR_INVALID, "device index outside the visible devices");
    MI_HIP(hipGetDevice(&prev));
    MI_HIP(hipSetDevice(device));
    return MI_OK;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

template <typename T>
int launch_quantize(const T* w, int N, int K, int bits, uint32_t* packed, T* scales, T* biases) {
  const size_t groups = (size_t)N * (K / GROUP);
  const dim3 grid((unsigned)((groups + NTHR / 64 - 1) / (NTHR / 64))), block(NTHR);
  if (bits == 4) hipLaunchKernelGGL((quantize_mlx_kernel<T, 4>), grid, block, 0, nullptr, w, groups, K, packed, scales, biases);
  else hipLaunchKernelGGL((quantize_mlx_kernel<T, 8>), grid, block, 0, nullptr, w, groups, K, packed, scales, biases);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

template <typename T>
int launch_merge(const MergeParams& p, int bits) {
  const dim3 grid(p.N), block(NTHR);
  if (bits == 0) hipLaunchKernelGGL((lora_merge_kernel<T, 0>), grid, block, 0, nullptr, p);
  else if (bits == 4) hipLaunchKernelGGL((lora_merge_kernel<T, 4>), grid, block, 0, nullptr, p);
  else hipLaunchKernelGGL((lora_merge_kernel<T, 8>), grid, block, 0, nullptr, p);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int check_quant_shape(const char* who, int N, int K, int dtype, int bits, int group) {
  if (dtype == MI_F32) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": float32 models are not supported (bf16 / f16 only)");
  if (dtype != MI_BF16 && dtype != MI_F16) return fail(MI_ERR_INVALID, std::string(who) + ": bad dtype");
  if (N < 1 || K < 1) return fail(MI_ERR_INVALID, std::string(who) + ": N and K must be positive");
  if (bits != 4 && bits != 8) return fail(MI_ERR_INVALID, std::string(who) + ": quant_bits must be 4 or 8");
  if (group == 32 || group == 128) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": quantisation groups of 64 only");
  if (group != GROUP) return fail(MI_ERR_INVALID, std::string(who) + ": bad quantisation group");
  if (K % GROUP != 0) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": K must be a multiple of 64 when quantised");
  if ((size_t)N * (K / GROUP) / (NTHR / 64) >= 0x7fffffffull) return fail(MI_ERR_UNSUPPORTED, std::string(who) + ": too many groups");
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_quantize_mlx(int device, int N, int K, int dtype, int bits, int group, const void* w, void* out_w, void* out_scales,
                    void* out_biases) {
  MI_TRY(check_quant_shape("mi_quantize_mlx", N, K, dtype, bits, group));
  if (!w || !out_w || !out_scales || !out_biases) return fail(MI_ERR_INVALID, "mi_quantize_mlx: null argument");
  if (!aligned(w, 2) || !aligned(out_w, 4) || !aligned(out_scales, 2) || !aligned(out_biases, 2))
    return fail(MI_ERR_INVALID, "mi_quantize_mlx: misaligned buffer");
  DeviceScope scope;
  MI_TRY(scope.enter(device));
  if (dtype == MI_BF16) MI_TRY(launch_quantize<bf16>((const bf16*)w, N, K, bits, (uint32_t*)out_w, (bf16*)out_scales, (bf16*)out_biases));
  else MI_TRY(launch_quantize<f16>((const f16*)w, N, K, bits, (uint32_t*)out_w, (f16*)out_scales, (f16*)out_biases));
  MI_HIP(hipStreamSynchronize(nullptr));
  return MI_OK;
}

int mi_lora_merge(int device, int N, int K, int rank, int dtype, int quant_bits, int quant_group, const void* w,
                  const void* scales, const void* biases, const float* A, const float* B, const float* m, float s,
                  int requantize, void* out_w, void* out_scales, void* out_biases) {
  if (dtype == MI_F32) return fail(MI_ERR_UNSUPPORTED, "mi_lora_merge: float32 models are not supported (bf16 / f16 only)");
  if (dtype != MI_BF16 && dtype != MI_F16) return fail(MI_ERR_INVALID, "mi_lora_merge: bad dtype");
  if (N < 1 || K < 1) return fail(MI_ERR_INVALID, "mi_lora_merge: N and K must be positive");
  if (rank < 1 || rank > 64) return fail(MI_ERR_INVALID, "mi_lora_merge: rank outside 1..64");
  if (quant_bits != 0) {
    MI_TRY(check_quant_shape("mi_lora_merge", N, K, dtype, quant_bits, quant_group));
    if (m != nullptr)
      return fail(MI_ERR_UNSUPPORTED, "mi_lora_merge: DoRA on a quantised base is not supported (as mi_engine_set_dora refuses it)");
    if (!scales || !biases) return fail(MI_ERR_INVALID, "mi_lora_merge: a quantised base needs scales and biases");
  } else if (requantize) {
    return fail(MI_ERR_INVALID, "mi_lora_merge: a re-quantised output needs a quantised input (its bits and group)");
  }
  if (!w || !A || !B || !out_w || (requantize && (!out_scales || !out_biases))) return fail(MI_ERR_INVALID, "mi_lora_merge: null argument");
  if (!std::isfinite(s)) return fail(MI_ERR_INVALID, "mi_lora_merge: the scale is not finite");
  if (!aligned(w, quant_bits ? 4 : 2) || !aligned(A, 4) || !aligned(B, 4) || !aligned(m, 4) || !aligned(out_w, requantize ? 4 : 2) ||
      !aligned(scales, 2) || !aligned(biases, 2) || !aligned(out_scales, 2) || !aligned(out_biases, 2))
    return fail(MI_ERR_INVALID, "mi_lora_merge: misaligned buffer");
  DeviceScope scope;
  MI_TRY(scope.enter(device));

  // Wm goes straight to the output only when nothing can refuse or transform it afterwards
  const bool staged = m != nullptr || requantize;
  DevBuf wm, gain;
  if (staged) MI_HIP(hipMalloc(&wm.p, (size_t)N * K * 2));
  if (m) MI_HIP(hipMalloc(&gain.p, (size_t)N * sizeof(float)));
  MergeParams p{w, scales, biases, N, K, rank, A, B, s, m, staged ? wm.p : out_w, (float*)gain.p};
  if (dtype == MI_BF16) MI_TRY(launch_merge<bf16>(p, quant_bits));
  else MI_TRY(launch_merge<f16>(p, quant_bits));
  if (m) {
    std::vector<float> g(N);
    MI_HIP(hipMemcpy(g.data(), gain.p, (size_t)N * sizeof(float), hipMemcpyDeviceToHost));    // (waits for the launch)
    for (int n = 0; n < N; ++n)
      if (!std::isfinite(g[n]))
        return fail(MI_ERR_INVALID, "mi_lora_merge: row " + std::to_string(n) + ": m is not finite, or the merged row's norm is 0 or not finite");
    const dim3 grid(N), block(NTHR);
    if (dtype == MI_BF16) hipLaunchKernelGGL(dora_scale_kernel<bf16>, grid, block, 0, nullptr, (const bf16*)wm.p, (const float*)gain.p, (bf16*)out_w, K);
    else hipLaunchKernelGGL(dora_scale_kernel<f16>, grid, block, 0, nullptr, (const f16*)wm.p, (const float*)gain.p, (f16*)out_w, K);
    MI_HIP(hipGetLastError());
  } else if (requantize) {
    if (dtype == MI_BF16) MI_TRY(launch_quantize<bf16>((const bf16*)wm.p, N, K, quant_bits, (uint32_t*)out_w, (bf16*)out_scales, (bf16*)out_biases));
    else MI_TRY(launch_quantize<f16>((const f16*)wm.p, N, K, quant_bits, (uint32_t*)out_w, (f16*)out_scales, (f16*)out_biases));
  }
  MI_HIP(hipStreamSynchronize(nullptr));
  return MI_OK;
}

}  // extern "C"
