// misc.hip -- embedding gather, row gather, KV copy, head permutation, offsets, RoPE tables, converters.
#include <type_traits>

#include "kernels.h"

namespace mi {

namespace {

// ------------------------------------------------------------------------------------------
// nn.Embedding / nn.QuantizedEmbedding row gather (llama.py:212, qwen3.py:166).
// Quantised rows are dequantised as round_T(scale*q + bias).
template <typename AT, int WK>
__global__ __launch_bounds__(256) void embed_kernel(LinearW W, EmbedCall c) {
  const int row = blockIdx.x;
  int tok = c.tokens[row];
  tok = min(max(tok, 0), W.N - 1);
  AT* out = (AT*)c.out + (size_t)row * W.K;
  if constexpr (WK == WK_BF16 || WK == WK_F16) {
    // 16-bit tables: 16-byte pieces (8 elements) per thread instead of one element per trip (10 -> ~4 us at the head of every
    // decode step); same values, store_act is applied element by element as below
    if (W.K % 8 == 0) {
      using WT = typename std::conditional<WK == WK_BF16, bf16, f16>::type;
      for (int p8 = threadIdx.x; p8 < W.K / 8; p8 += 256) {
        const char* src = W.layout ? (const char*)W.w + tiled_piece_dense16(tok, p8 * 8, W.K)
                                   : (const char*)W.w + ((size_t)tok * W.K + (size_t)p8 * 8) * 2;
        const uint4 raw = *(const uint4*)src;
        const WT* e = (const WT*)&raw;
        AT o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = store_act<AT>((float)e[i], c.rnd);
        if constexpr (sizeof(AT) == 2) {
          *(uint4*)(out + (size_t)p8 * 8) = *(const uint4*)o;
        } else {
          *(uint4*)(out + (size_t)p8 * 8) = *(const uint4*)o;
          *(uint4*)(out + (size_t)p8 * 8 + 4) = *(const uint4*)(o + 4);
        }
      }
      return;
    }
  }
  for (int k = threadIdx.x; k < W.K; k += 256) {
    float v;
    const int k8 = k & ~7;
    if constexpr (WK == WK_F32) v = ((const float*)W.w)[(size_t)tok * W.K + k];
    else if constexpr (WK == WK_BF16)
      v = W.layout ? (float)((const bf16*)((const char*)W.w + tiled_piece_dense16(tok, k8, W.K)))[k & 7]
                   : (float)((const bf16*)W.w)[(size_t)tok * W.K + k];
    else if constexpr (WK == WK_F16)
      v = W.layout ? (float)((const f16*)((const char*)W.w + tiled_piece_dense16(tok, k8, W.K)))[k & 7]
                   : (float)((const f16*)W.w)[(size_t)tok * W.K + k];
    else {
      constexpr int BITS = (WK >= WK_Q8_F32) ? 8 : 4;
      constexpr int SDT = (WK - 3) % 3;
      constexpr int PER = 32 / BITS;
      const size_t gi = (size_t)tok * (W.K / W.group) + k / W.group;
      float s, b;
      uint32_t word;
      if (BITS == 4 && SDT != 0 && W.layout) {     // tile-major int4 (repack.hip)
        const char* blk = (const char*)W.w + tiled_block_q4(tok, k, W.K);
        const int so = tiled_q4_scale_off(tok, k);
        if constexpr (SDT == 1) { s = (float)*(const bf16*)(blk + so); b = (float)*(const bf16*)(blk + so + 64); }
        else { s = (float)*(const f16*)(blk + so); b = (float)*(const f16*)(blk + so + 64); }
        word = *(const uint32_t*)(blk + tiled_q4_code_off(tok, k8));
      } else if (BITS == 8 && SDT != 0 && W.layout) {   // tile-major int8
        const char* blk = (const char*)W.w + tiled_block_q8(tok, k, W.K);
        const int so = tiled_q8_scale_off(tok);
        if constexpr (SDT == 1) { s = (float)*(const bf16*)(blk + so); b = (float)*(const bf16*)(blk + so + 32); }
        else { s = (float)*(const f16*)(blk + so); b = (float)*(const f16*)(blk + so + 32); }
        word = *(const uint32_t*)(blk + tiled_q8_code_off(tok, k & ~3));
      } else {
      if constexpr (SDT == 0) { s = ((const float*)W.scales)[gi]; b = ((const float*)W.biases)[gi]; }
      else if constexpr (SDT == 1) { s = (float)((const bf16*)W.scales)[gi]; b = (float)((const bf16*)W.biases)[gi]; }
      else { s = (float)((const f16*)W.scales)[gi]; b = (float)((const f16*)W.biases)[gi]; }
      word = ((const uint32_t*)W.w)[(size_t)tok * (W.K / PER) + k / PER];
      }
      const float q = (float)((word >> (BITS * (k % PER))) & ((1u << BITS) - 1u));
      v = mul_add_unfused(q, s, b);
    }
    out[k] = store_act<AT>(v, c.rnd);
  }
}

template <typename AT>
int launch_embed_wk(const LinearW& W, const EmbedCall& c, hipStream_t st) {
  const dim3 grid(c.rows), block(256);
#define EK(WKV) hipLaunchKernelGGL((embed_kernel<AT, WKV>), grid, block, 0, st, W, c); break
  switch (W.wk) {
    case WK_F32: EK(WK_F32);
    case WK_BF16: EK(WK_BF16);
    case WK_F16: EK(WK_F16);
    case WK_Q4_F32: EK(WK_Q4_F32);
    case WK_Q4_BF16: EK(WK_Q4_BF16);
    case WK_Q4_F16: EK(WK_Q4_F16);
    case WK_Q8_F32: EK(WK_Q8_F32);
    case WK_Q8_BF16: EK(WK_Q8_BF16);
    case WK_Q8_F16: EK(WK_Q8_F16);
    default: return fail(MI_ERR_UNSUPPORTED, "embed: bad weight kind");
  }
#undef EK
  MI_HIP(hipGetLastError());
  return MI_OK;
}

__global__ void advance_offsets_kernel(int32_t* offsets, const int32_t* rows, int B, int L) {
  const int i = threadIdx.x;
  if (i < B) offsets[rows ? rows[i] : i] += L;
}

__global__ void rope_tables_kernel(float* cos_tab, float* sin_tab, int max_pos, int D2, double base, double scale) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= max_pos * D2) return;
  const int pos = idx / D2, i = idx % D2;
  const double inv = pow(base, -2.0 * (double)i / (double)(2 * D2));
  const double ang = (double)pos * scale * inv;
  cos_tab[idx] = (float)cos(ang);
  sin_tab[idx] = (float)sin(ang);
}

template <typename S, typename T>
__global__ void convert_kernel(const S* src, T* dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = (T)(float)src[i];
}

}  // namespace

int launch_embed(const LinearW& W, const EmbedCall& c, hipStream_t st) {
  switch (c.act) {
    case MI_F32: return launch_embed_wk<float>(W, c, st);
    case MI_BF16: return launch_embed_wk<bf16>(W, c, st);
    case MI_F16: return launch_embed_wk<f16>(W, c, st);
  }
  return fail(MI_ERR_INVALID, "embed: bad activation dtype");
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const u128* src, size_t row_vecs, const int32_t* idx, u128* dst) {
  const u128* s = src + (size_t)idx[blockIdx.x] * row_vecs;
  u128* d = dst + (size_t)blockIdx.x * row_vecs;
  for (size_t i = threadIdx.x; i < row_vecs; i += 256) d[i] = s[i];
}

int launch_gather_rows(const void* src, size_t row_bytes, const int32_t* idx, int n, void* dst, hipStream_t st) {
  if (row_bytes % 16 != 0) return fail(MI_ERR_UNSUPPORTED, "gather_rows: rows must be multiples of 16 bytes");
  if (n <= 0) return MI_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, st, (const u128*)src, row_bytes / 16, idx, (u128*)dst);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// mi_kv_fork_row's copy: for every (layer, kv head, K | V) -- blockIdx.y -- the span of span_vecs 16-byte pieces at src_vec
// goes to dst_vec, both counted from the head's start in the K or V array (layer stride layer_vecs, head stride head_vecs).
// blockIdx.x strides over the pieces, one piece per lane and round.  The spans of one launch never overlap (two blocks of an
// arena, two rows of a cache).
__global__ __launch_bounds__(256) void kv_copy_tokens_kernel(u128* kc, u128* vc, size_t layer_vecs, int Hkv, size_t head_vecs,
                                                             size_t src_vec, size_t dst_vec, unsigned span_vecs) {
  const unsigned unit = blockIdx.y, lh = unit >> 1, layer = lh / (unsigned)Hkv, head = lh - layer * (unsigned)Hkv;
  u128* base = ((unit & 1) ? vc : kc) + (size_t)layer * layer_vecs + (size_t)head * head_vecs;
  const u128* s = base + src_vec;
  u128* d = base + dst_vec;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < span_vecs; i += gridDim.x * 256) d[i] = s[i];
}

int launch_kv_copy_tokens(void* kcache, void* vcache, int kv_dtype, int layers, size_t layer_elems, int Hkv, int D,
                          size_t head_stride, size_t src_off, size_t dst_off, int n_tokens, hipStream_t st) {
  if (kv_dtype != MI_F32 && kv_dtype != MI_BF16 && kv_dtype != MI_F16) return fail(MI_ERR_INVALID, "kv_copy_tokens: bad element type");
  if (!kcache || !vcache || layers < 1 || Hkv < 1 || D < 1 || n_tokens < 1) return fail(MI_ERR_INVALID, "kv_copy_tokens: bad argument");
  const size_t es = dtype_size(kv_dtype), span = (size_t)n_tokens * D;
  if (((uintptr_t)kcache | (uintptr_t)vcache) % 16 != 0 || (layer_elems * es) % 16 != 0 || (head_stride * es) % 16 != 0 ||
      (src_off * es) % 16 != 0 || (dst_off * es) % 16 != 0 || (span * es) % 16 != 0)
    return fail(MI_ERR_UNSUPPORTED, "kv_copy_tokens: every span, stride and offset must be a multiple of 16 bytes");
  // the spans lie inside their heads and the heads inside a layer; no head's destination touches any head's source: the two
  // sets of heads lie apart (two blocks, two rows), or they interleave with room for a span on either side
  const size_t delta = src_off < dst_off ? dst_off - src_off : src_off - dst_off, r = head_stride ? delta % head_stride : 0;
  if (span > head_stride || std::max(src_off, dst_off) + (size_t)(Hkv - 1) * head_stride + span > layer_elems ||
      !(delta >= (size_t)Hkv * head_stride || (r >= span && head_stride - r >= span)))
    return fail(MI_ERR_INVALID, "kv_copy_tokens: the spans overlap or leave the layer");
  const size_t units = (size_t)layers * Hkv * 2, span_vecs = span * es / 16;
  if (units > 65535 || span_vecs > 0xffffffffu - 32 * 256) return fail(MI_ERR_UNSUPPORTED, "kv_copy_tokens: too many layers x heads, or a span too long");
  const unsigned gx = (unsigned)std::min<size_t>((span_vecs + 255) / 256, 32);
  hipLaunchKernelGGL(kv_copy_tokens_kernel, dim3(gx, (unsigned)units), dim3(256), 0, st, (u128*)kcache, (u128*)vcache,
                     layer_elems * es / 16, Hkv, head_stride * es / 16, src_off * es / 16, dst_off * es / 16, (unsigned)span_vecs);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// rope_traditional: rows of a [nrows][row_u16 x 2 bytes] array regrouped inside every run of D rows (one head), new row j <-
// old row 2 j, new row D/2 + j <- old row 2 j + 1: the interleaved pairs (2 i, 2 i + 1) become the half-split pairs
// (i, i + D/2) that the RoPE kernels rotate.  One thread per 16-bit unit of the destination (load time only).
__global__ __launch_bounds__(256) void head_perm_rows_kernel(const uint16_t* src, uint16_t* dst, size_t nrows, int D, size_t row_u16) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows * row_u16) return;
  const size_t row = i / row_u16, col = i - row * row_u16;
  const int j = (int)(row % (size_t)D), half = D / 2;
  const size_t srow = row - j + (j < half ? 2 * j : 2 * (j - half) + 1);
  dst[i] = src[srow * row_u16 + col];
}

int launch_head_perm_rows(const void* src, void* dst, size_t nrows, int D, size_t row_bytes, hipStream_t st) {
  if (D < 2 || D % 2 != 0 || nrows % (size_t)D != 0 || row_bytes % 2 != 0)
    return fail(MI_ERR_INVALID, "head_perm_rows: whole heads of an even head_dim, rows of whole 16-bit units");
  const size_t total = nrows * (row_bytes / 2);
  if (total == 0) return MI_OK;
  hipLaunchKernelGGL(head_perm_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint16_t*)src,
                     (uint16_t*)dst, nrows, D, row_bytes / 2);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_advance_offsets(int32_t* offsets, const int32_t* rows, int B, int L, hipStream_t st) {
  hipLaunchKernelGGL(advance_offsets_kernel, dim3(1), dim3(64 * ((B + 63) / 64)), 0, st, offsets, rows, B, L);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_rope_tables(float* cos_tab, float* sin_tab, int max_pos, int D, float base, float scale, hipStream_t st) {
  const int n = max_pos * (D / 2);
  hipLaunchKernelGGL(rope_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cos_tab, sin_tab, max_pos, D / 2,
                     (double)base, (double)scale);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_convert(const void* src, int sdt, void* dst, int ddt, size_t n, hipStream_t st) {
  const dim3 grid((unsigned)std::min<size_t>((n + 255) / 256, 4096)), block(256);
#define CV(S, T) hipLaunchKernelGGL((convert_kernel<S, T>), grid, block, 0, st, (const S*)src, (T*)dst, n)
  if (sdt == MI_F32 && ddt == MI_F32) CV(float, float);
  else if (sdt == MI_BF16 && ddt == MI_F32) CV(bf16, float);
  else if (sdt == MI_F16 && ddt == MI_F32) CV(f16, float);
  else if (sdt == MI_F32 && ddt == MI_BF16) CV(float, bf16);
  else if (sdt == MI_F32 && ddt == MI_F16) CV(float, f16);
  else if (sdt == MI_BF16 && ddt == MI_BF16) CV(bf16, bf16);
  else if (sdt == MI_F16 && ddt == MI_F16) CV(f16, f16);
  else return fail(MI_ERR_UNSUPPORTED, "convert: dtype pair not supported");
#undef CV
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
