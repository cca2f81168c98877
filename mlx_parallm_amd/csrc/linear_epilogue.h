// linear_epilogue.h -- what ends a linear layer, once: the rounding points of its output value (kernels.h EPI_*)
// and the terms that come from outside the matrix (bias, LoRA).  Every kernel family that ends a linear calls these, so a
// rounding point or an activation is changed in ONE place and all routes keep giving the same bits.
//
//   R(v) = rounded<T>(v, rnd): T(v) for a 16-bit storage type T; for T = float the run-time logical rounding `rnd` (RND_NONE:
//   the identity), exactly store_act<T>.
//
//   linear_value   R(acc), or with a bias R(acc + b) (dense) / R(R(acc) + b) (quantised)
//   swiglu_value   R(R(g . R(sigmoid(g))) . u) from already rounded g and u
//   lora_add       R(y + R(scale . z)), one adapted range (lora_rows.hip); lora_term: both ranges of EpiTerms on one output
//                  element -- dead, EpiTerms::lora_t is always null (kernels.h, LinearW)
//   quant_accumulate  acc += scale . d + bias . sum(x) on the four rows a lane holds (the quantised kernels' inner step)
//
// Not here: the residual add h <- R(h0 + y).  It is one expression and is tied to each kernel's own prefetch of h.
//
// Contraction (hipcc fuses a product into an add of its result unless told otherwise) -- what each helper pins:
//   linear_value   the add of the bias is never fused with a product that made acc (add_bias, common.h: contract off)
//   swiglu_value   products only, each followed by R or by another product: nothing to fuse
//   lora_add       scale . z and y + (.) stay two float32 roundings (contract off): with T = float and rnd = RND_NONE nothing
//                  else stands between them.  That is what every site compiled to before this header existed -- the run-time
//                  select of R sat between the product and the add -- so the pragma changes no instruction.
//   quant_accumulate  explicit fmaf, inner term first
// Two sites that look alike and are NOT: the sigmoid.  The fused epilogues take expf in float32 and round the float32
// (sigmoid_rounded); swiglu_rows_kernel (lora_rows.hip) takes exp in float64 and rounds once (sigmoid_rounded_f64, the reason is
// written there).  They differ on the few g whose float32 sigmoid lands on a midpoint of T's grid; both are kept, by name.
#pragma once

#include "kernels.h"
#include "mfma16.h"

namespace mi {

// The epilogue's terms from outside the matrix, as a kernel sees them (a member of every linear kernel's parameter struct).
struct EpiTerms {
  const float* lora_t; int lora_t_ld;     // [M][2][lora_t_ld / 2] = round(x A) for the two adapted ranges; null: no LoRA term
  const float* lora_b[2];                 // B [rank][n] of range 0 / 1; null: no such range
  struct Range { int row0, n, rank; float scale; } r[2];    // output columns [row0, row0 + n)
  const float* bias; int bias2;           // LinearW::bias ([N] float32 or null); bias2 = quantised weights (two roundings)
};

inline EpiTerms epi_terms(const LinearW& W, const GemvCall& c) {
  EpiTerms e{};
  e.lora_t = c.lora_t; e.lora_t_ld = c.lora_t_ld;
  for (int i = 0; i < 2; ++i) {
    e.lora_b[i] = W.lora_b[i];
    e.r[i] = {W.lora_row0[i], W.lora_n[i], W.lora_rank[i], W.lora_scale[i]};
  }
  e.bias = W.bias; e.bias2 = wk_is_quant(W.wk) ? 1 : 0;
  return e;
}

template <typename T>
__device__ __forceinline__ float rounded(float v, int rnd) { return to_f32(store_act<T>(v, rnd)); }

// The plain value of output column n.  has_bias: a compile-time constant where the biased form is an instantiation of its
// own (skinny_kernel, Phase), `bias != nullptr` where it is not (gemv_v1, gemm_prefill).
template <typename T>
__device__ __forceinline__ float linear_value(float acc, bool has_bias, const float* bias, int n, int bias2, int rnd) {
  if (has_bias) return add_bias<T>(acc, bias[n], bias2 != 0, rnd);
  return rounded<T>(acc, rnd);
}

template <typename T>
__device__ __forceinline__ float sigmoid_rounded(float g, int rnd) { return rounded<T>(1.0f / (1.0f + expf(-g)), rnd); }

// sig = T(sigmoid(g)) with the exp taken in float64 and ONE rounding, float64 -> T.  Through float32 (sigmoid_rounded) the
// value is rounded twice, and for the few g whose sigmoid lies within a float32 ulp of a midpoint of T's grid
// (g = 11 x 2^-10: 0.5 + 5.5 ulps of f16 less 2.6e-8) the float32 lands ON the midpoint and the tie goes the wrong way: sig one ulp
// off, which g * sig can carry to two ulps of the product -- measured: nine elements of 129 x 14336 in f16.  For a kernel
// bound by its memory traffic (swiglu_rows_kernel), where the float64 exp is free.
template <typename T>
__device__ __forceinline__ float sigmoid_rounded_f64(float g, int rnd) {
  const double sg = 1.0 / (1.0 + exp(-(double)g));
  if constexpr (sizeof(T) == 4) {
    if (rnd == RND_BF16) return (float)(bf16)sg;
    if (rnd == RND_F16) return (float)(f16)sg;
    return (float)sg;
  } else {
    return (float)(T)sg;
  }
}

// nn.silu(gate) * up with every op rounded to the activation dtype (llama.py:165); g and u are linear_value's
template <typename T, bool SIG64 = false>
__device__ __forceinline__ float swiglu_value(float g, float u, int rnd) {
  float sig;
  if constexpr (SIG64) sig = sigmoid_rounded_f64<T>(g, rnd);
  else sig = sigmoid_rounded<T>(g, rnd);
  const float s = rounded<T>(g * sig, rnd);
  return rounded<T>(s * u, rnd);
}

// LoRALinear: y + (scale * ((x A) B)).astype(x.dtype), z = (x A) B of this element.  lora_rnd rounds z and scale * z once more
// ahead of R (gemv_v1's generic kernel carries the mode; everybody else passes the constant RND_NONE, which folds away).
template <typename T>
__device__ __forceinline__ float lora_add(float y, float scale, float z, int rnd, int lora_rnd) {
#pragma clang fp contract(off)
  z = round_rt(z, lora_rnd);
  z = round_rt(scale * z, lora_rnd);
  const float s = y + rounded<T>(z, rnd);
  return rounded<T>(s, rnd);
}

// both ranges of `e` on output element (m, n), range 0 first
template <typename T>
__device__ __forceinline__ float lora_term(float y, const EpiTerms& e, int m, int n, int rnd, int lora_rnd) {
  if (e.lora_t == nullptr) return y;
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const float* lb = e.lora_b[sl];
    const int r0 = e.r[sl].row0, ln = e.r[sl].n;
    if (lb != nullptr && n >= r0 && n < r0 + ln) {
      const float* tt = e.lora_t + (size_t)m * e.lora_t_ld + sl * (e.lora_t_ld / 2);
      y = lora_add<T>(y, e.r[sl].scale, lora_dot(tt, lb + (n - r0), ln, e.r[sl].rank), rnd, lora_rnd);
    }
  }
  return y;
}

// y += scale * sum((OFFS + q) x) + (bias - OFFS * scale) * sum(x) on the four output rows of a lane: d = the codes' dot
// products, sx = the rows' sums of x over the quantisation group
__device__ __forceinline__ void quant_accumulate(f32x4& acc, float sc, float bb, const f32x4& d, const f32x4& sx) {
  acc.x = fmaf(sc, d.x, fmaf(bb, sx.x, acc.x));
  acc.y = fmaf(sc, d.y, fmaf(bb, sx.y, acc.y));
  acc.z = fmaf(sc, d.z, fmaf(bb, sx.z, acc.z));
  acc.w = fmaf(sc, d.w, fmaf(bb, sx.w, acc.w));
}

}  // namespace mi
