// mx4_cvt.h -- the conversions of MX codes to bf16 that the Microscaling kernels share: FP4 (E2M1) for gemm_mx4.hip (1..128 rows)
// and gemm_qtile.hip (prefill), FP8 (E4M3) for gemm_mx8.hip.
#pragma once

#include "mfma16.h"

namespace mi {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// the B operand of one MFMA step: the eight codes of `dw` (code e at nibble e) times `scale`, as bf16 -- four
// v_cvt_scalef32_pk_bf16_fp4, one per byte of the dword
__device__ __forceinline__ u32x4 mx_operand(uint32_t dw, float scale) {
  u32x4 r;
  r.x = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 0));
  r.y = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 1));
  r.z = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 2));
  r.w = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 3));
  return r;
}

// the same operand from E4M3 codes: the eight code bytes of `lo` (e = 0..3) and `hi` (e = 4..7), code e at byte e % 4 -- four
// v_cvt_scalef32_pk_bf16_fp8, the low and the high word of each dword
__device__ __forceinline__ u32x4 mx8_operand(uint32_t lo, uint32_t hi, float scale) {
  u32x4 r;
  r.x = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, false));
  r.y = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, true));
  r.z = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, false));
  r.w = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, true));
  return r;
}

// MX group T (0..3) of a block: its E8M0 scale byte in the row's dword, as float32 bits (byte 0 and 255: include/mi355_ops.h)
__device__ __forceinline__ float mx_scale(uint32_t sc, int T) { return __uint_as_float(((sc >> (8 * T)) & 0xffu) << 23); }

}  // namespace mi
