// attn_mfma.h -- device helpers the matrix-core attention kernels share (attn_decode.hip, attn_prefill.hip).
#pragma once

#include "kernels.h"
#include "mfma16.h"

namespace mi {

typedef short s16x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  T v[2] = {(T)a, (T)b};
  return __builtin_bit_cast(uint32_t, v);
}

// P as TWO 16-bit operands (round 4): hi = T(p), lo = T(p - hi).  The reference's attention keeps the softmax numerators in
// float32 (App. A.4); feeding them to the matrix core as ONE 16-bit value was a rounding the oracle does not have -- the
// CPU variant with that rounding (oracle/numerics.py SDPA_P16) reproduces the 1.05 - 1.33 x excess of the device's mean
// |logprob - exact| over the float32-accumulating variants.  hi + lo carries 16+ mantissa bits; the second
// MFMA per V tile costs ~0.2 us per launch.
template <typename T>
__device__ __forceinline__ void pack2_split(float a, float b, uint32_t& hi, uint32_t& lo) {
  const T ha = (T)a, hb = (T)b;
  T h[2] = {ha, hb};
  T l[2] = {(T)(a - (float)ha), (T)(b - (float)hb)};
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}

// v_mfma_f32_16x16x4_f32: exact float32 products, one float per lane and operand (the float32 caches)
__device__ __forceinline__ f32x4 mfma_f32(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// A piece of a cached K / V row in the matrix-core kernel: one CU reads it once per step, and gigabytes of weights and other
// rows pass before the next step reads it again, so it goes past the caches like the weight streams (gemv_f32.hip: load_w).
// The KV append and the prologue's loads keep the default policy.
template <typename V>
__device__ __forceinline__ V load_kv(const void* p) { return __builtin_nontemporal_load((const V*)p); }

// The last split's combine: (max, sum, O[d]) of every split for one (head, d).  The loads of four splits are issued
// together (a loop over a run-time split count with the loads inside waits one L2 round trip per load: ~8 in a row
// for 4 splits), then merged in split order -- deterministic whoever arrived last.
template <int D>
__device__ __forceinline__ float combine_splits(const float* pp, int nsplit, int d) {
  float mn = -1e30f, L = 0.f, O[1] = {0.f};
  for (int i0 = 0; i0 < nsplit; i0 += 4) {
    float mv[4], lv[4], ov[4][1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* q = pp + (size_t)min(i0 + j, nsplit - 1) * (D + 2);
      mv[j] = __hip_atomic_load(&q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lv[j] = __hip_atomic_load(&q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ov[j][0] = __hip_atomic_load(&q[2 + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    merge_splits4<1>(mn, L, O, mv, lv, ov, nsplit - i0);
  }
  return merged_out(O[0], L);
}

}  // namespace mi
