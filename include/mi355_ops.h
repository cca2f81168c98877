/*
 * mi355_ops.h -- kernel-level entry points of libmi355_decode.so.
 *
 * These expose the individual HIP kernels behind mi355_decode.h on caller-owned DEVICE
 * buffers (e.g. torch tensors) so that each fused stage can be checked against the oracle at
 * its own scale and timed on its own (bench.py roofline leg).  They are not needed to use the
 * engine.  Every call runs on the HIP null stream of the current device and synchronises
 * before returning.  Error convention as in mi355_decode.h.
 *
 * Reference op each one replaces (MLX call sites in the reference):
 *   mi_op_gemv        nn.Linear / nn.QuantizedLinear (+ fused RMSNorm / residual / SwiGLU):
 *                     llama.py:64-67,93,143,160-165,175-177,188-190,250-252; qwen3.py:37-40,63,115
 *   mi_op_gemv_gu8    nn.silu(gate_proj(x)) * up_proj(x) on the row-interleaved gate|up copy: llama.py:160-165
 *   mi_op_embed       nn.Embedding / QuantizedEmbedding: llama.py:212; qwen3.py:166
 *   mi_op_rope_append q_norm/k_norm + nn.RoPE + cache.update_and_fetch:
 *                     qwen3.py:65-70; llama.py:107-125; base.py:66-85,119-140
 *   mi_op_attention   mx.fast.scaled_dot_product_attention + causal mask: llama.py:139-141; base.py:17-40
 *   mi_op_sample      sample closure + top_p_sampling: utils.py:345-364; sample_utils.py:3-38
 *   mi_op_sample_ex   the same kernel with top_k / min_p and per-row random streams (no counterpart in the reference)
 *   mi_op_sample_rowbias  ... and a call-wide logit_bias list (utils.py:346-349) + the per-row table (no counterpart)
 *   mi_op_lora_rows   LoRALinear's term y + (scale * ((x A) B)).astype(x.dtype), each row with its own adapter (the per-request
 *                     table has no counterpart in the reference)
 *   mi_op_dora_gain / mi_op_dora_rows   mlx-lm DoRALinear's m / ||W + scale (A B)^T|| per output column, and the LoRA term followed
 *                     by that factor (restated from the published formula; mlx-lm is not among the reference's sources)
 *   mi_op_kv_copy_tokens  the tail copy of mi_kv_fork_row (no counterpart in the reference)
 *   mi_op_sample_rowlp    ... and the per-row logprobs settings of mi_kv_set_row_logprobs (no counterpart)
 *   mi_op_moe_route / mi_op_moe_linear / mi_op_moe_mlp   MixtralSparseMoeBlock: mixtral.py:108-119 (gate, argpartition, softmax,
 *                     SwitchGLU, weighted sum)
 */
#ifndef MI355_OPS_H
#define MI355_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weight kinds */
#define MI_WK_F32 0
#define MI_WK_BF16 1
#define MI_WK_F16 2
#define MI_WK_Q4_F32 3
#define MI_WK_Q4_BF16 4
#define MI_WK_Q4_F16 5
#define MI_WK_Q8_F32 6
#define MI_WK_Q8_BF16 7
#define MI_WK_Q8_F16 8

/* run-time logical rounding on top of the storage dtype */
#define MI_RND_NONE 0
#define MI_RND_BF16 1
#define MI_RND_F16 2

#define MI_PRO_NONE 0
#define MI_PRO_NORM 1

#define MI_EPI_STORE 0
#define MI_EPI_STORE_F32 1
#define MI_EPI_RESID 2
#define MI_EPI_SWIGLU 3

typedef struct mi_op_linear {
  int32_t wk;            /* MI_WK_* */
  int32_t N, K, group;
  const void* w;         /* [N][K] dense, or MLX-packed [N][K*bits/32] */
  const void* scales;    /* [N][K/group] */
  const void* biases;
  int32_t layout;        /* 0 = row-major (checkpoint order), 1 = tile-major (mi_op_repack_tiled; then w is
                            the tiled buffer and scales/biases are unused) */
  const float* bias;     /* [N] float32 bias of nn.Linear / nn.QuantizedLinear (llama.py:59-67,155-162), or NULL.  Dense
                            weights: y = T(acc + b); quantised: y = T(T(acc) + b).  mi_op_gemv, mi_op_gemm_skinny,
                            mi_op_gemm_prefill(_f32) apply it; mi_op_gemv_f32 and a forced gemm_q4 plan refuse it */
} mi_op_linear;

typedef struct mi_op_gemv_args {
  const void* x;         /* [M][ldx] */
  int32_t ldx, M;
  int32_t act, rnd;      /* MI_F32/BF16/F16 storage, MI_RND_* */
  int32_t pro;           /* MI_PRO_* */
  int32_t epi;           /* MI_EPI_* */
  const void* norm_w;    /* [K] */
  float eps;
  int32_t ldo;
  void* out;
  void* resid;
  int32_t pair_offset;
  int32_t force_generic; /* 1 = never take the MFMA path */
} mi_op_gemv_args;

typedef struct mi_op_attn_shape {
  int32_t B, L, Hq, Hkv, D;
  int32_t act, kv, rnd, cap;
} mi_op_attn_shape;

int mi_op_gemv(const mi_op_linear* w, const mi_op_gemv_args* a);
int mi_op_gemv_uses_mfma(const mi_op_linear* w, const mi_op_gemv_args* a);
/* the SwiGLU launch of the decode GEMV on the row-interleaved gate|up copy (gemv_mfma.hip: gemv_mfma_gu8_kernel, what the
 * engine runs for a dense 16-bit mlp.gate_proj | mlp.up_proj at 1..16 rows) on its own.  w: a tile-major dense bf16 / f16
 * gate|up matrix of 2 x a->pair_offset rows, a->epi = MI_EPI_SWIGLU, the other fields of a as for mi_op_gemv; the
 * row-interleaved copy (tile t = gate rows 8t..8t+7, then up rows 8t..8t+7) is made inside the call, as mi_op_gemv_f32 does.
 * mi_op_gemv with MI_EPI_SWIGLU runs the paired-tile form instead.  MI_ERR_UNSUPPORTED, nothing launched: a bias, quantised
 * or row-major weights, activations of another type than the weights, a->rnd != MI_RND_NONE, a->M outside 1..16,
 * a->pair_offset % 16 != 0, w->N != 2 * a->pair_offset, a->ldx % 8 != 0, w->K % 32 != 0, another epilogue. */
int mi_op_gemv_gu8(const mi_op_linear* w, const mi_op_gemv_args* a);
/* launches the same call `iters` times back to back and returns the mean launch time (HIP events) */
int mi_op_gemv_bench(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms);
/* the split-K weight-streaming GEMM the engine uses for decode steps of 9..128 rows (int4 / int8 weights: 1..128), on its own:
 * a->M in that range, a->pro = MI_PRO_NONE, tile-major 16-bit, int4 or int8 (group 64) weights.  ksplit 0 = the library's
 * cost model (returned in *ksplit_used); iters >= 1 also times that many back-to-back launches into *avg_ms.
 * int4 weights above 16 rows with ksplit <= 0 run the round-4 kernel (gemm_q4.hip: x prepared once per launch, K split
 * over the waves of a workgroup; a->pro may then be MI_PRO_NORM); ksplit < 0 forces its plan for tests and A/B runs:
 * -(row_tiles | tile_units << 3 | k_lanes << 7 | ksplit << 11 | staging_waves << 15), any field 0 = the cost model's choice. */
int mi_op_gemm_skinny(const mi_op_linear* w, const mi_op_gemv_args* a, int ksplit, int* ksplit_used, int iters,
                      float* avg_ms);
/* the one-pass weight-streaming GEMV of the float32-KV decode step (gemv_f32.hip) on its own: float32 activations, outputs
 * and norm weights, a->rnd = MI_RND_NONE, a->M in 1..8, tile-major dense bf16 weights, K % 32 == 0, N % 16 == 0.  Epilogues:
 * MI_EPI_STORE / MI_EPI_STORE_F32 / MI_EPI_RESID, and MI_EPI_SWIGLU on a gate|up matrix of 2 x a->pair_offset rows (the
 * row-interleaved copy the engine keeps is made inside the call).  a->pro may be MI_PRO_NORM: the row scale is applied in
 * the epilogue.  iters >= 1 also times that many back-to-back launches into *avg_ms. */
int mi_op_gemv_f32(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms);
/* the whole-K form of that kernel (the o_proj launch of the float32-KV decode step) on its own: the same operator and, output
 * for output, the same bits, for a narrow linear -- N / 16 at most the device's compute units (one 16-row tile per workgroup),
 * K <= 4096, a->pro = MI_PRO_NONE, MI_EPI_STORE / MI_EPI_STORE_F32 / MI_EPI_RESID.  Anything else is MI_ERR_UNSUPPORTED.
 * iters >= 1 also times that many back-to-back launches into *avg_ms. */
int mi_op_gemv_f32_whole(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms);
/* the resident form of that kernel (the gate|up and lm_head launches of the float32-KV decode step) on its own: the calls,
 * prologue and epilogues of mi_op_gemv_f32 and, output for output, the same bits, with x and the norm weights kept in LDS for
 * the whole launch -- K <= 4096.  Anything else is MI_ERR_UNSUPPORTED.  mi_op_gemv_f32 itself always runs the chunked kernel.
 * iters >= 1 also times that many back-to-back launches into *avg_ms. */
int mi_op_gemv_f32_resident(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms);
/* gemm_prefill.hip on its own: the tile GEMM of the prefill call (generate_step's first model call, utils.py:243-262: every
 * nn.Linear over B x L rows at once).  a->M rows of 16-bit activations, tile-major dense 16-bit weights, a->pro =
 * MI_PRO_NONE; plain / residual / SwiGLU epilogues.  iters >= 1 also times that many back-to-back launches into *avg_ms.
 * Tile-major int4 / int8 (group 64) weights (nn.QuantizedLinear, llama.py:64-67) are taken too: their [hi | lo] 16-bit copy is
 * made in a scratch buffer inside the call, as the engine does.  Float32 activations are refused: mi_op_gemm_prefill_f32. */
int mi_op_gemm_prefill(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms);
/* the same tile GEMM on float32 activations, the PagedKVCache mode (base.py:111-112 promotes every activation behind layer 0
 * to float32; the linears are llama.py:64-67,93,143,160-165 again): a->x float32 rows, a->act = MI_F32, a->rnd = MI_RND_NONE,
 * float32 outputs and residual; a->pro may be MI_PRO_NORM with float32 norm weights (llama.py:187,189), applied inside the
 * split.  The call splits x exactly into x_terms bf16 terms (mi_op_split_rows) and runs the tile GEMM over that image, as the
 * engine's prefill does.  w is tile-major: dense bf16 (x_terms 2 or 3), int4-bf16 group 64 (x_terms 3; the [hi | lo] copy is
 * made inside), or dense f16 with K % 64 == 0 (x_terms 3; its exact [hi | lo] bf16 copy is made inside).  Anything the tile
 * GEMM does not take returns MI_ERR_UNSUPPORTED -- no other kernel runs.  iters >= 1 also times that many back-to-back
 * launches of the GEMM (without the split) into *avg_ms. */
int mi_op_gemm_prefill_f32(const mi_op_linear* w, const mi_op_gemv_args* a, int x_terms, int iters, float* avg_ms);
/* the split in front of it on its own: rows x K float32 (row stride ldx; K % 4 == 0, ldx % 4 == 0), RMS-normalised first when
 * norm_w (float32 [K], nn.RMSNorm: llama.py:187,189) is not NULL -> out[rows][terms x K] bf16 = [hi | mid | lo] (terms 3) or
 * [hi | mid] (terms 2) with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): hi + mid + lo == x exactly. */
int mi_op_split_rows(const float* x, int ldx, const float* norm_w, float eps, int rows, int K, int terms, void* out);
/* SwiGLU over stored rows (lora_rows.hip): x[M][ldx] holds gate at column n and up at column I + n (the plain-store output of a
 * gate|up linear -- what the engine runs when mlp.gate_proj / mlp.up_proj carry a LoRA adapter, whose term must be added before
 * the activation); out[m][n] = T(T(g * T(sigmoid(g))) * u), the rounding points of nn.silu(gate) * up in the activation dtype
 * (llama.py:165), as MI_EPI_SWIGLU (the exp of the sigmoid is taken in float64).  act = MI_F32 / MI_BF16 / MI_F16 storage of x and out, rnd = MI_RND_* on top of float32
 * storage.  M >= 1, I a positive multiple of 8 (else MI_ERR_UNSUPPORTED), ldx >= 2 I, ldo >= I, buffers aligned to their
 * element (else MI_ERR_INVALID); nothing is launched on a refused call. */
int mi_op_swiglu_rows(const void* x, int ldx, void* out, int ldo, int M, int I, int act, int rnd);
/* the LoRA term of a step, each row with the adapter it names (lora_rows.hip), on its own: the two launches that stand around
 * every adapted linear of the engine, on caller-owned DEVICE buffers.
 *   MI_LORA_STAGE_DOWN  t[m][part][0..rank) = xs_m A, A [K][rank] float32 = the part's factor of row m's adapter, xs_m = row m
 *                       of x [M][ldx] (act storage, rnd on top of float32), with pro = MI_PRO_NORM after the RMSNorm of the
 *                       linear's prologue: xs = T(T(x rs) norm_w), norm_w [K] in act.  K <= 36864 (else MI_ERR_UNSUPPORTED).
 *   MI_LORA_STAGE_UP    y[m][row0[p] + c] = T(y + T(scale (t[m][p] B)[c])), c in [0, n[p]), B [rank][n[p]] float32, reading the
 *                       caller's t; with resid != NULL ([M][ldr], one part at column 0) EVERY row, adapted or not, ends with
 *                       resid[m][c] = T(resid + y') and y stays as it was.
 *   both (1 | 2)        the down launch, then the up-add, as the engine runs them.
 * t [M][3 * 64] float32 is the caller's.  row_adapter: device int32 [M], the table column of every row; a value outside
 * [0, MI_MAX_ADAPTERS] (mi355_decode.h) means "no adapter" and is not refused.  The adapter table is four HOST arrays
 * [n_parts][MI_MAX_ADAPTERS + 1] (tab_a / tab_b: device pointers; tab_rank; tab_scale), column MI_MAX_ADAPTERS being the
 * engine-wide adapter's; A = B = NULL: the adapter does not cover the part.  The call uploads it to a device table of its own
 * and frees that before it returns.  n_parts in 1..3 with HOST arrays row0[] / n[] (read by the up stage only).
 * MI_ERR_INVALID, nothing launched and no output touched: a null x, y, t, row_adapter or table array that a stage needs; M < 1;
 * n_parts outside 1..3; stages outside 1..3; a bad act, rnd or pro; a norm without norm_w; ldx < K; a part outside [0, ldy); a
 * residual with more than one part, a row0 other than 0 or ldr < n[0]; an entry with only one of A / B; a covered entry whose rank
 * is outside 1..64; A or B not 16-byte aligned; x, norm_w, y or resid not aligned to their element. */
#define MI_LORA_STAGE_DOWN 1
#define MI_LORA_STAGE_UP 2
int mi_op_lora_rows(const void* x, int ldx, int M, int K, int act, int rnd, int pro, const void* norm_w, float eps,
                    const int32_t* row_adapter, int n_parts, const int32_t* row0, const int32_t* n,
                    const float* const* tab_a, const float* const* tab_b, const int32_t* tab_rank, const float* tab_scale,
                    float* t, void* y, int ldy, void* resid, int ldr, int stages);
/* DoRA's gain kernel (lora_rows.hip) on its own, what mi_engine_set_dora runs once per adapted part:
 *   gain[i] = m[i] / || W[row0 + i, :] + scale sum_j B[j][i] A[:, j] ||_2,  i in [0, n)
 * w: a dense MI_WK_BF16 / MI_WK_F16 matrix, row-major or tile-major (mi_op_repack_tiled); rows [row0, row0 + n) are one part of
 * it.  A [K][rank], B [rank][n], m [n] and gain [n]: DEVICE float32.  float32 accumulation in a fixed order, no atomics: run to
 * run, and row-major against tile-major, the bits are the same.  A row whose norm is 0 gets NaN (the engine refuses such an
 * adapter).  MI_ERR_INVALID, nothing launched: a null pointer, rank outside 1..64, rows outside the matrix, a misaligned
 * buffer, a tile-major matrix with N % 16 != 0 or K % 32 != 0; MI_ERR_UNSUPPORTED: any other weight kind. */
int mi_op_dora_gain(const mi_op_linear* w, const float* A, const float* B, const float* m, int rank, float scale, int row0, int n,
                    float* gain);
/* mi_op_lora_rows with one more HOST table, tab_gain [n_parts][MI_MAX_ADAPTERS + 1] of DEVICE pointers (float32 [n[p]], as
 * mi_op_dora_gain writes them; NULL: a plain LoRA entry): the up stage ends a row whose entry has a gain with
 * y' = T(T(gain[c]) * y') ahead of the residual add.  The gain-aware instantiation of the up-add kernel runs exactly when some
 * entry has a gain; rows whose entry has none, and rows without an adapter, then take no multiplication -- their outputs are
 * mi_op_lora_rows', bit for bit.  Refusals as mi_op_lora_rows, and MI_ERR_INVALID, nothing launched: a null tab_gain, a gain on
 * an entry without A / B, a gain that is not 4-byte aligned. */
int mi_op_dora_rows(const void* x, int ldx, int M, int K, int act, int rnd, int pro, const void* norm_w, float eps,
                    const int32_t* row_adapter, int n_parts, const int32_t* row0, const int32_t* n,
                    const float* const* tab_a, const float* const* tab_b, const int32_t* tab_rank, const float* tab_scale,
                    const float* const* tab_gain, float* t, void* y, int ldy, void* resid, int ldr, int stages);
/* the copy of mi_kv_fork_row (mi355_decode.h) on its own, one launch: in each of `layers` layers (layer_elems elements apart),
 * for each of Hkv heads (head_stride elements apart) and in kcache and vcache alike, the n_tokens x D elements at element
 * offset src_off (of head 0, inside the layer) are copied to dst_off, in 16-byte pieces.  kv_dtype = MI_F32 / MI_BF16 /
 * MI_F16 elements.  Paged arena [block][Hkv][block_tokens][D]: head_stride = block_tokens x D, the offsets those of the
 * first tail token in the two blocks; contiguous cache [row][Hkv][cap][D]: head_stride = cap x D, the offsets those of the
 * two rows.  MI_ERR_UNSUPPORTED: a span, stride, offset or pointer that is no multiple of 16 bytes (head widths 32, 64, 96
 * and 128 always are); MI_ERR_INVALID: spans that leave the layer or where a destination touches a source.  Nothing is
 * launched on a refused call. */
int mi_op_kv_copy_tokens(void* kcache, void* vcache, int kv_dtype, int layers, int64_t layer_elems, int Hkv, int D,
                         int64_t head_stride, int64_t src_off, int64_t dst_off, int n_tokens);
/* tile-major weight layout of the streaming kernels (what mi_engine_finalize applies to eligible
 * matrices): returns the size of the tiled buffer (0 if the matrix is not eligible) / fills `dst`. */
uint64_t mi_op_tiled_bytes(const mi_op_linear* row_major);
int mi_op_repack_tiled(const mi_op_linear* row_major, void* dst);
int mi_op_embed(const mi_op_linear* w, const int32_t* tokens, int rows, int act, int rnd, void* out);
int mi_op_rope_tables(float* cos_tab, float* sin_tab, int max_pos, int head_dim, float base, float scale);
int mi_op_rope_append(const mi_op_attn_shape* s, const void* qkv, void* q_out, void* kcache, void* vcache,
                      const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                      const float* cos_tab, const float* sin_tab, int max_pos);
int mi_op_attention(const mi_op_attn_shape* s, const void* q, const void* kcache, const void* vcache,
                    const int32_t* offsets, void* out, float scale, int nsplit, float* partial);
/* fused decode attention (L == 1): q/k norm + RoPE + append + split-KV attention + combine.
 * counters: [B*Hkv] zero-initialised ints.  variant 0: MFMA kernel where it applies (16-bit caches,
 * head_dim % 32 == 0; float32 caches, head_dim 64 / 128), 1: VALU kernel.  iters > 1 repeats the launch (timing; avg_ms
 * may be NULL). */
int mi_op_attention_decode(const mi_op_attn_shape* s, const void* qkv, void* kcache, void* vcache,
                           const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                           const float* cos_tab, const float* sin_tab, void* out, float scale, int rnd_out,
                           int nsplit, float* partial, int32_t* counters, int variant, int iters, float* avg_ms);
/* the same launch with the cache row and the KV length of every sequence chosen by the caller.  rows: device [B] or NULL
 * (identity) -- sequence b lives in cache row rows[b], offsets[] is indexed by cache row (a step over a subset of the cache's
 * rows).  host_row / host_off: HOST arrays [B] or both NULL; when given (B <= 32) they travel in the kernel arguments as in
 * the engine's decode step -- host_row[b] = the cache row of b, host_off[b] = offsets[that row] -- and the kernel reads
 * neither rows nor offsets. */
int mi_op_attention_decode_host(const mi_op_attn_shape* s, const void* qkv, void* kcache, void* vcache,
                                const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                                const float* cos_tab, const float* sin_tab, void* out, float scale, int rnd_out,
                                int nsplit, float* partial, int32_t* counters, int variant, int iters, float* avg_ms,
                                const int32_t* rows, const int32_t* host_row, const int32_t* host_off);
int mi_op_sample(float* logits, int B, int V, float temperature, float top_p, const float* uniforms,
                 int top_logprobs, int32_t* tokens_out, float* logprob_out, float* prob_row0_out,
                 int32_t* topk_ids, float* topk_logprobs, float* row_stats);
/* the same kernel with every sampling control of mi_sample_params (mi355_decode.h, where the semantics are written down)
 * exposed: scalar top_k / min_p; DEVICE arrays [B] or NULL row_temperature + row_top_p (both or neither), row_top_k, row_min_p
 * (each on its own), row_seed + row_position (both or neither); the call-wide Philox key `seed` and counter `step`; `uniforms`
 * (device [B] or NULL) take precedence over every stream.  With all of them off / NULL and seed = step = 0 the call is
 * mi_op_sample, bit for bit.  top_k < 0, min_p outside [0, 1] or NaN, or half a pair: MI_ERR_INVALID, nothing is launched.
 * Per-row values are not read by the host: a row_top_k <= 0 or >= V and a row_min_p outside (0, 1] leave that control off. */
int mi_op_sample_ex(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                    const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                    const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                    const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                    float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats);
/* mi_op_sample_ex + both logit_bias inputs of the engine's sampler, all DEVICE arrays: the call-wide list (n_bias entries
 * bias_ids / bias_values, added to every row: mi_sample_params.logit_bias_*) and then the per-row table of
 * mi_kv_set_row_logit_bias (mi355_decode.h): sampled row b adds the row_bias_counts[t] entries (row_bias_ids[t][i],
 * row_bias_values[t][i]) of table row t = row_map ? row_map[b] : b; the table has table_rows rows of `cap` entries each.
 * logits change in place, logits[b][id] = float32(l + v), an id in both lists gets both, the call-wide one first.  Nothing is
 * validated on the host beyond the shapes: an id outside [0, V), a t outside [0, table_rows) and entries past `cap` are skipped
 * by the kernel; duplicate ids within ONE list are a data race (the engine refuses them).  row_bias_counts == NULL (then the
 * other table arguments are ignored) and n_bias = 0: mi_op_sample_ex, bit for bit, on the same instantiation of the kernel. */
int mi_op_sample_rowbias(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                         const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                         const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                         const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                         float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats,
                         int n_bias, const int32_t* bias_ids, const float* bias_values,
                         const int32_t* row_bias_counts, const int32_t* row_bias_ids, const float* row_bias_values,
                         int table_rows, int cap, const int32_t* row_map);
/* mi_op_sample_rowbias + the per-row logprobs settings of mi_kv_set_row_logprobs (mi355_decode.h), DEVICE arrays
 * [table_rows] indexed like the bias table (t = row_map ? row_map[b] : b; row_bias_counts may be NULL: settings without a
 * table): row_top_logprobs[t] >= 0 is sampled row b's own count of top entries (capped at MI_MAX_TOP_LOGPROBS) and
 * row_at_temperature[t] != 0 reports its logprob_out and top entries under softmax(logits / T_b) when T_b > 0;
 * row_top_logprobs[t] < 0, or a t outside the table: the row keeps the call's top_logprobs and logprobs_at_temperature.
 * n_row_settings = the number of table rows with a setting, which the host knows (the kernel does not count them):
 *   > 0: topk_ids / topk_logprobs are [B][MI_MAX_TOP_LOGPROBS]: a row's first k_b entries as mi_op_sample_ex writes them at
 *        top_logprobs = k_b (bit for bit; past the row's last comparable logit: id 0 and the logprob of -inf), then (-1, -inf);
 *   0:   the launch, the arguments and the [B][top_logprobs] layout of mi_op_sample_rowbias, whatever the arrays hold.
 * method: how a row with k_b > 0 finds its entries.  1: k rounds of arg-max, one walk of the row each (the form of every
 * other entry point); 2: the selection -- a count descent to the k_b-th key, one gather walk, at most five walks whatever
 * k_b; 0: per row, the selection from the measured crossover k_b >= 4 on (what the engine launches).  All three write the
 * same bits.  logprobs_at_temperature is the call-wide flag of mi_sample_params, which mi_op_sample_ex leaves off. */
int mi_op_sample_rowlp(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                       const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                       const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                       const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                       float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats,
                       int n_bias, const int32_t* bias_ids, const float* bias_values,
                       const int32_t* row_bias_counts, const int32_t* row_bias_ids, const float* row_bias_values,
                       int table_rows, int cap, const int32_t* row_map, const int32_t* row_top_logprobs,
                       const int32_t* row_at_temperature, int n_row_settings, int logprobs_at_temperature, int method);

/* ---- the sparse mixture-of-experts MLP of MI_ARCH_MIXTRAL (moe.hip), stage by stage.  T = `act` (MI_F32 / MI_BF16 / MI_F16
 * storage, `rnd` on top of float32); router and expert weights are dense, row-major, `wdt` = MI_BF16 / MI_F16 and equal to act
 * unless act is MI_F32 (then widened exactly).  E in 1..16, k in {1, 2}, k <= E; a pair is p = row * k + j.  iters >= 1 also
 * times that many back-to-back launches into *avg_ms.
 * mi_op_moe_route: xn [R][ldx] (H % 64 == 0, ldx % 8 == 0), wg [E][H] -> sel [R][k] int32 = the k largest g = T(xn wg^T) in
 * descending order, a tie going to the lower expert index; score [R][k] in T = T(softmax_float32(g[sel])); meta [2 E] int32 =
 * the pairs per expert, then where each expert's run starts in list; list [R k] int32 = the pairs grouped by expert, ascending
 * inside a run (built by a scan: the same in every run). */
int mi_op_moe_route(const void* xn, int ldx, int R, int H, int act, int rnd, const void* wg, int wdt, int E, int k,
                    int32_t* sel, void* score, int32_t* meta, int32_t* list, int iters, float* avg_ms);
/* the grouped linear with a plain store: out[p][n] = T(x[p >> x_shift] . w[e][n]) for every pair p on expert e's list; w
 * [E][N][K], N % 64 == 0, K % 64 == 0, x [x_rows][ldx], out [pairs][ldo]; pairs on no list are not written.  meta / list as
 * mi_op_moe_route writes them (DEVICE); the call reads them back first and refuses (MI_ERR_INVALID, nothing launched) runs that
 * leave list [pairs], an entry outside [0, pairs) or one whose row p >> x_shift is outside x. */
int mi_op_moe_linear(const void* x, int ldx, int x_rows, int x_shift, int act, int rnd, const void* w, int wdt, int E, int N,
                     int K, const int32_t* meta, const int32_t* list, int pairs, void* out, int ldo, int iters, float* avg_ms);
/* the route's outputs through the rest of the block: act[p] = T(T(silu(gate_e xn)) up_e xn), y[p] = down_e act[p] (workspace
 * of the call's own), out[row] = T(resid[row] + r) or, resid == NULL, r = T(T(y_a s_a) + T(y_b s_b)).  w_gate, w_up [E][I][H],
 * w_down [E][H][I]; H % 64 == 0, I % 64 == 0; the lists are checked as in mi_op_moe_linear.  stage_ms: NULL or float[3] =
 * the mean launch time of gate|up, down and combine over iters launches each. */
int mi_op_moe_mlp(const void* xn, int ldx, int R, int H, int I, int act, int rnd, int wdt, int E, int k, const void* w_gate,
                  const void* w_up, const void* w_down, const int32_t* meta, const int32_t* list, const void* score,
                  const void* resid, int ldr, void* out, int ldo, int iters, float* stage_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI355_OPS_H */
