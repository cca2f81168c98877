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

}  // namespace mi
