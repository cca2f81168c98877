/*
 * mi355_decode.h -- C ABI of libmi355_decode.so, the MI355X (gfx950) batched-decode engine.
 *
 * The reference (misanthropic-ai/mlx_parallm) has NO FFI / plugin interface: its boundary is
 * the Python API in mlx_parallm/utils.py and everything below it is the third-party MLX
 * runtime.  This ABI sits where MLX sits today; each entry point names the reference
 * interface it replaces (file:line in the reference checkout).  The Python side that binds
 * it is mlx_parallm_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - return 0 = OK, <0 = error class; message via mi_last_error() (thread local).
 *       MI_ERR_INVALID  (-1)  -> Python ValueError
 *       MI_ERR_NOTFOUND (-2)  -> Python FileNotFoundError / KeyError
 *       MI_ERR_UNSUPPORTED(-3)-> Python NotImplementedError
 *       MI_ERR_RUNTIME  (-4)  -> Python RuntimeError (HIP failure, out of memory, no device)
 *   - the caller owns every host buffer it passes, for the duration of the call only;
 *     the library owns all device memory behind its handles; every *_create has a *_destroy.
 *   - one mi_engine per device; calls on one engine are NOT re-entrant (the reference is
 *     single-flight too: utils.py:1345, server/main.py:1076-1107).  Different engines may be
 *     driven from different host threads / processes concurrently.
 *   - there is NO CPU backend: without a HIP device mi_engine_create fails with
 *     MI_ERR_RUNTIME.
 */
#ifndef MI355_DECODE_H
#define MI355_DECODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI guard.  mi_abi_version() returns MI_ABI_VERSION of the library that was loaded; both parameter structs begin with
 * `struct_size`, which the caller sets to sizeof() of ITS definition -- a binding generated from another version of this
 * header (a shorter mi_sample_params would make the library read pointers past its end) is refused with MI_ERR_INVALID
 * by mi_engine_create / mi_decode_sample / mi_step_enqueue(_rows) / mi_score_tokens instead of being read. */
#define MI_ABI_VERSION 4

#define MI_OK 0
#define MI_ERR_INVALID (-1)
#define MI_ERR_NOTFOUND (-2)
#define MI_ERR_UNSUPPORTED (-3)
#define MI_ERR_RUNTIME (-4)

/* element types of tensors handed to mi_engine_set_tensor / activation + KV storage */
#define MI_F32 0
#define MI_BF16 1
#define MI_F16 2
#define MI_U32 3 /* MLX-packed quantised weights: 32/bits codes per word, little-endian */

#define MI_ARCH_LLAMA 0 /* mlx_parallm/models/llama.py (also model_type "mistral": utils.py:33-36) */
#define MI_ARCH_QWEN3 1 /* mlx_parallm/models/qwen3.py: + per-head q_norm/k_norm (qwen3.py:65-70) */
#define MI_ARCH_PHI3 2 /* mlx_parallm/models/phi3.py */
#define MI_ARCH_MIXTRAL 3 /* mlx_parallm/models/mixtral.py: Mistral's attention, a sparse mixture-of-experts MLP (see below) */

/* KV-cache element type selector for mi_kv_create */
#define MI_KV_MODEL (-1) /* BatchedKVCache semantics: KV in the model dtype (models/base.py:66-85) */
/* MI_F32 on a 16-bit model = PagedKVCache semantics: float32 KV and everything after the
 * layer-0 attention promoted to float32 (models/base.py:104-117). */

typedef struct mi_engine mi_engine; /* opaque; replaces the nn.Module returned by utils.load (utils.py:711-747) */
typedef struct mi_kv mi_kv;         /* opaque; replaces List[PagedKVCache] from _KVPool.get (utils.py:199-223) */

/* ModelArgs (llama.py:15-46 / mlx-lm qwen3 ModelArgs) + config.json["quantization"] (utils.py:679-690) */
typedef struct mi_model_desc {
  uint32_t struct_size;      /* = sizeof(mi_model_desc) of the caller's header (ABI guard) */
  int32_t arch;              /* MI_ARCH_* */
  int32_t hidden_size;
  int32_t num_layers;
  int32_t num_heads;
  int32_t num_kv_heads;
  int32_t head_dim;
  int32_t intermediate_size;
  int32_t vocab_size;
  float rms_norm_eps;
  float rope_theta;
  float rope_scale;          /* 1/factor for linear rope_scaling, else 1 (llama.py:69-76) */
  int32_t tie_word_embeddings;
  int32_t act_dtype;         /* MI_F32 | MI_BF16 | MI_F16: dtype of the weights (dense) or scales (quantised) */
  int32_t quant_bits;        /* 0 = no quantised tensors; else 4 or 8 */
  int32_t quant_group_size;  /* 64 (32 / 128 also accepted) */
  int32_t max_positions;     /* RoPE table length = largest KV capacity a mi_kv may have */
  /* ABI 3 (llama.py:59-67,155-162,77-82); MI_ARCH_LLAMA */
  int32_t attention_bias;    /* q/k/v/o_proj carry a `.bias` tensor ([N], model dtype or float32) */
  int32_t mlp_bias;          /* gate/up/down_proj carry a `.bias` tensor */
  int32_t rope_traditional;  /* nn.RoPE(traditional=True): pairs (2 i, 2 i + 1) of a head rotate.  mi_engine_finalize regroups
                              * the q / k rows (and biases; mi_engine_set_lora: the columns of B) into the half-split order
                              * of the kernels -- q.k is unchanged, V / O / the caches are untouched.  MI_ARCH_QWEN3 with the
                              * flag: MI_ERR_UNSUPPORTED (q_norm / k_norm would need the same regrouping) */
  /* MI_ARCH_MIXTRAL (mixtral.py:20,22); ignored by every other arch.  The struct grew without a new MI_ABI_VERSION: struct_size
   * refuses a binding built against the shorter layout. */
  int32_t num_local_experts;   /* E in 1..16 */
  int32_t num_experts_per_tok; /* k in {1, 2}, k <= E */
} mi_model_desc;

/* arguments of the `sample` closure (utils.py:345-364) + top_p_sampling (sample_utils.py:3-38) */
typedef struct mi_sample_params {
  uint32_t struct_size;      /* = sizeof(mi_sample_params) of the caller's header (ABI guard) */
  float temperature;         /* 0 -> greedy argmax (utils.py:352-353) */
  float top_p;               /* 0<top_p<1 -> nucleus (utils.py:355-356), else plain categorical */
  int32_t n_logit_bias;      /* logit_bias dict (utils.py:346-349) */
  const int32_t* logit_bias_ids;
  const float* logit_bias_values;
  const float* uniforms;     /* [B] caller-supplied U[0,1) noise, or NULL -> library Philox stream */
  uint64_t seed;             /* Philox key when uniforms == NULL */
  int32_t top_logprobs;      /* 0..MI_MAX_TOP_LOGPROBS: also return the k most likely tokens */
  int32_t logprobs_at_temperature; /* 0: logprob / top-k logprobs are log_softmax(logits) (generate_step);
                                    * 1 and temperature > 0: log_softmax(logits / temperature), the distribution
                                    * the server's logprobs path reports (server/main.py:571-584) */
  const float* row_temperature;    /* both NULL: `temperature` / `top_p` apply to every row.  Both [B]: per-row */
  const float* row_top_p;          /* values (continuous batching, where requests with different settings share a step) */
  int64_t stream_position;         /* Philox counter of this step when uniforms == NULL: >= 0 = the caller's own step index
                                    * (generate_step passes 0, 1, 2, ...: the same seed then reproduces the same tokens,
                                    * like re-seeding mx.random before a call); < 0 = the engine's running step counter */
  /* ABI 4: per-request sampling controls.  Candidates are ordered by descending logit, ties by ascending id; a row with
   * temperature > 0 keeps the SHORTEST (by count) of three prefixes of that order and draws from it with u * mass(kept);
   * greedy rows ignore all of them, and the reported logprobs stay those of the unfiltered distribution. */
  int32_t top_k;                   /* 0 < top_k < V: keep the first top_k candidates (a cut inside a tie group keeps its lowest
                                    * ids); the nucleus is then taken over them, against top_p * (their mass).  Else off */
  float min_p;                     /* 0 < min_p <= 1: keep the candidates with p >= min_p * p_max, tested on the device as
                                    * (logit - max) * (1 / temperature) >= logf(min_p) in float32.  0 = off */
  const int32_t* row_top_k;        /* [B] or NULL, each on its own: per-row values instead of the scalar (rows as for */
  const float* row_min_p;          /* row_temperature; mi_step_enqueue_mixed: one entry per wanted segment) */
  const uint64_t* row_seed;        /* [B], both or neither.  A row with row_position[b] >= 0 draws from the Philox stream */
  const int64_t* row_position;     /* (row_seed[b], row_position[b], 0): what the call-wide stream (seed, stream_position)
                                    * gives row 0, whichever index the row has and whoever shares the step.  < 0: the row
                                    * keeps the call-wide stream (seed, step, b).  `uniforms` take precedence over both.
                                    * Violations (top_k < 0, min_p outside [0, 1] or NaN, a per-row value out of range,
                                    * row_seed without row_position or the reverse) are MI_ERR_INVALID naming the field,
                                    * before anything is enqueued */
} mi_sample_params;

#define MI_MAX_TOP_LOGPROBS 20

/* ---- engine life cycle: replaces utils.load_model (utils.py:630-708) ------------------- */
int mi_engine_create(const mi_model_desc* desc, int device, mi_engine** out);
void mi_engine_destroy(mi_engine* e);

/* One call per checkpoint tensor, named as in the safetensors file (e.g.
 * "model.layers.3.self_attn.q_proj.weight" / ".scales" / ".biases", "model.norm.weight",
 * "lm_head.weight"); replaces model.load_weights (utils.py:693-702).  "<proj>.bias" (1-D, N elements, float32 / bf16 / f16;
 * not the quantisation ".biases") is taken for q/k/v/o_proj when desc.attention_bias is set and for gate/up/down_proj when
 * desc.mlp_bias is set; with the flag off the name is unknown (MI_ERR_NOTFOUND), as the reference filters it.  `data` is a host
 * pointer (on_device = 0) or a device pointer on the engine's device (on_device = 1, e.g. a
 * torch tensor that was just filled by an RCCL broadcast); the bytes are COPIED.
 * Unknown names -> MI_ERR_NOTFOUND (the reference filters them, utils.py:693-698).
 * MI_ARCH_PHI3 (phi3.py:48-49,116): "self_attn.qkv_proj" holds q, then k, then v along the rows and "mlp.gate_up_proj" gate,
 * then up; each is one tensor per ".weight" / ".scales" / ".biases" with all the rows (any other row count: MI_ERR_INVALID
 * naming it), and the split names (q_proj, ..., up_proj) are unknown.  phi3.py has no linear biases and no tied head:
 * desc.attention_bias, mlp_bias or tie_word_embeddings set is MI_ERR_INVALID at mi_engine_create; rope_traditional and
 * rope_scale are those of MI_ARCH_LLAMA (phi3.py:73-81).
 * MI_ARCH_MIXTRAL (mixtral.py:95-119,198-215): dense 16-bit checkpoints only -- act_dtype MI_F32 or quant_bits != 0 is
 * MI_ERR_UNSUPPORTED at mi_engine_create naming the field, as are num_local_experts outside 1..16, num_experts_per_tok outside
 * {1, 2} (or above the expert count) and a hidden_size or intermediate_size that is no multiple of 64; tie_word_embeddings,
 * attention_bias or mlp_bias set is MI_ERR_INVALID.  The MLP of a block is "block_sparse_moe.gate.weight" [E][H] and either the
 * stacked tensors "block_sparse_moe.switch_mlp.{gate_proj,up_proj,down_proj}.weight" ([E][I][H], [E][I][H], [E][H][I]) or, per
 * expert e, "block_sparse_moe.experts.<e>.{w1,w3,w2}.weight" (gate [I][H], up [I][H], down [H][I]; copied into slot e), in any
 * mix; a wrong shape is MI_ERR_INVALID naming the tensor, ".scales" / ".biases" of these names MI_ERR_UNSUPPORTED, and the
 * dense "mlp.*" names are unknown.  mi_engine_finalize names the first expert slot that was not set.  The block computes, in
 * the activations' dtype T: g = T(xn Wg^T); the k largest g, a tie going to the lower expert index; s = T(softmax_float32 over
 * the selected); y_e = down_e(T(T(silu(gate_e xn)) up_e xn)); h = T(h + T(T(y_a s_a) + T(y_b s_b))).  LoRA: q/k/v/o_proj as
 * on MI_ARCH_LLAMA, any "block_sparse_moe.*" name MI_ERR_UNSUPPORTED. */
int mi_engine_set_tensor(mi_engine* e, const char* name, const void* data, const int64_t* shape,
                         int ndim, int dtype, int on_device);

/* LoRALinear for one projection (mlx-lm load_adapters, utils.py:742-744; file layout
 * rl_training/lora_init.py:140-153; whatever lora_parameters.keys names, lora_init.py:72,95-96).  proj: any of the seven
 * linears of a block -- "self_attn.q_proj" / "k_proj" / "v_proj" / "o_proj", "mlp.gate_proj" / "up_proj" / "down_proj" --
 * in any combination (q, k and v together; gate and up: their terms are added BEFORE silu(gate) * up); any other name,
 * lm_head and the embedding included, is MI_ERR_UNSUPPORTED.  A is (K, r), B is (r, N), row-major, float32 (16-bit factors
 * and ranks outside 1..64: MI_ERR_UNSUPPORTED).  y += (scale * ((x A) B)).astype(x.dtype), on top of the projection's bias
 * when it has one.  With desc.rope_traditional the columns of B of q_proj / k_proj are regrouped like the rows of the matrix
 * (the caller passes them in checkpoint order, also on a hot-swap).  May be called on a finalized, live engine: a projection
 * that is already adapted is hot-swapped, a new one is added; the outputs do not depend on the order in which the
 * projections arrived.  A refused call changes nothing.
 * The engine-wide adapter is a private entry of the per-request adapters' table (below) that every token row of every step
 * runs, whatever mi_kv_set_row_adapter says: the same launches, the same bits as a batch whose rows all name one slot that
 * holds these factors.  No slot number reaches it (mi_engine_clear_adapter, mi_kv_set_row_adapter), and the cache rows stay
 * on "no adapter": prefix keys and forks are those of an engine without adapters.
 * MI_ARCH_PHI3: proj is "self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj" or "mlp.down_proj", the names an
 * adapter file of that family carries.  For the two fused ones A (K, r) is shared and B (r, N) is cut by columns into the
 * parts: bit for bit what one call per part with its column slice gives on an engine with split projections. */
int mi_engine_set_lora(mi_engine* e, int layer, const char* proj, const void* A, const void* B,
                       int rank, float scale, int dtype, int on_device);

/* Per-request adapters: up to MI_MAX_ADAPTERS LoRA adapters are resident on one engine, every KV row names one of them or
 * none (mi_kv_set_row_adapter), and every step -- decode, prefill, mixed, mi_score_tokens -- applies to each token row the
 * adapter of its sequence.  Several fine-tunes of one base model then share its weights and its batch.
 * mi_engine_set_adapter_lora: one projection of adapter slot `adapter` in [0, MI_MAX_ADAPTERS); projections, layouts, dtypes,
 * the rank range [1,64], the column cut of a MI_ARCH_PHI3 fused projection and the rope_traditional regrouping of B are those
 * of mi_engine_set_lora.  Adapters may cover different (layer, projection) subsets and have different ranks.  Works on a
 * finalized, live engine: an entry that exists is hot-swapped (the stream is drained first).  A refused call changes nothing.
 * mi_engine_clear_adapter: frees every entry of the slot; the slot is empty again.
 * Arithmetic of an adapted row: y = T(T(acc [+ b]) + T(scale (x A) B)), then the residual h + y where the projection has one --
 * the value, and the code, of mi_engine_set_lora.  The term runs as two small launches around the base linear ("Per-request
 * adapters"); a step in which no row names an adapter runs exactly the launches of an engine without adapters.
 * The table and the engine-wide adapter of mi_engine_set_lora exclude each other: whichever comes second is
 * MI_ERR_UNSUPPORTED.  A step one of whose rows names an empty slot is MI_ERR_INVALID before anything is launched.
 * Prefix reuse: the hash chain of a row starts from its adapter slot and the slot's generation (every set / clear bumps it),
 * so blocks published under one adapter are never attached under another or after the adapter changed; rows without an
 * adapter keep the keys they always had. */
#define MI_MAX_ADAPTERS 16
int mi_engine_set_adapter_lora(mi_engine* e, int adapter, int layer, const char* proj, const void* A, const void* B,
                               int rank, float scale, int dtype, int on_device);
int mi_engine_clear_adapter(mi_engine* e, int adapter);

/* DoRA (mlx-lm DoRALinear; adapter_config.json "fine_tune_type": "dora"): a LoRA entry with one more factor, the magnitude
 * m (N,) float32, N = the rows of the named projection.  mi_engine_set_dora is mi_engine_set_lora and
 * mi_engine_set_adapter_dora is mi_engine_set_adapter_lora with that argument: the same projection names, ranks 1..64, float32
 * factors, MI_ARCH_PHI3 fused projections (m is cut by parts, as B is cut by columns), rope_traditional regrouping (the m of
 * q_proj / k_proj follows the columns of B), exclusion of the engine-wide adapter and the slots, slot generation bump and
 * "a refused call changes nothing".  Arithmetic of an adapted row, T = the dtype of x in that call, W (N, K) the base matrix:
 *   y   = T(x W^T);  out = T(y + T(scale (x A) B))                      -- the LoRA entry, bit for bit
 *   g[n] = float32(m[n] / || float32(W)[n, :] + (scale B^T A^T)[n, :] ||_2)
 *   out = T(T(g[n]) * out), then the residual add / silu(gate) * up as always.
 * g is computed ONCE per call of these functions, by a kernel of fixed summation order (the same inputs give the same bits),
 * and kept as unrounded float32; the up-add launch rounds it to the T of each call.  It needs the final weights: before
 * mi_engine_finalize the call is MI_ERR_INVALID.  LoRA and DoRA entries may sit in different slots and in different projections
 * of one slot; setting LoRA over a DoRA entry drops its gain and the reverse adds one; mi_engine_clear_adapter frees it.  While
 * no resident entry of a matrix carries a gain its steps launch exactly the kernels of a LoRA-only engine; where one does,
 * rows whose adapter has no gain (and rows without an adapter) take no multiplication and keep their bits.
 * Refused, nothing changed: a projection whose base weights are quantised (mlx-lm multiplies x by the dtype-rounded
 * dequantised matrix there -- another product than QuantizedLinear's, which no kernel here computes) and a projection that
 * carries a linear bias (the reference adds the bias after the gain, the base kernels add it before): MI_ERR_UNSUPPORTED; a float32 model
 * (desc.act_dtype MI_F32: the gain kernel reads bf16 / f16 matrices): MI_ERR_UNSUPPORTED; an
 * m[n] that is not finite, or a row of W + scale (A B)^T whose norm is 0: MI_ERR_INVALID naming the projection.
 * The arithmetic restates mlx-lm's DoRALinear from its published formula; it could not be run against mlx-lm. */
int mi_engine_set_dora(mi_engine* e, int layer, const char* proj, const void* A, const void* B, const void* m, int rank,
                       float scale, int dtype, int on_device);
int mi_engine_set_adapter_dora(mi_engine* e, int adapter, int layer, const char* proj, const void* A, const void* B,
                               const void* m, int rank, float scale, int dtype, int on_device);

/* checks that every tensor was set (a missing `.bias` of a set bias flag: MI_ERR_NOTFOUND with its name), fuses q|k|v and
 * gate|up buffers, regroups q / k for rope_traditional, builds RoPE tables */
int mi_engine_finalize(mi_engine* e);

/* ---- KV cache: replaces _KVPool.get / PagedKVCache (utils.py:199-223, base.py:93-150) -- */
int mi_kv_create(mi_engine* e, int batch, int capacity_tokens, int kv_dtype, mi_kv** out);
/* Block-paged form for serving (the reference's continuous scheduler rebuilds its caches per batch and keeps a
 * process-global prefix cache, server/main.py:1404-1726, utils.py:231-287): `slots` rows share an arena of `n_blocks`
 * blocks of `block_tokens` tokens (a power of two >= 16; block 0 is reserved); a row's tokens live in the blocks its
 * table names, so a row grows without copying, costs memory only for what it holds, and rows with a common prompt
 * prefix can share blocks (mi_kv_prefix_*).  A row holds at most max_tokens_per_row tokens.  Every entry point that
 * takes a mi_kv accepts either form; mi_kv_reserve is a no-op up to that limit.  MI_ERR_RUNTIME when a step needs a
 * block and every block is held by a live sequence. */
int mi_kv_create_paged(mi_engine* e, int slots, int block_tokens, int n_blocks, int max_tokens_per_row, int kv_dtype,
                       mi_kv** out);
/* Prefix reuse on a paged cache.  attach: `row` is empty; the longest run of FULL blocks at the start of tokens[0..n)
 * that an earlier prompt has published is mapped into the row (shared, read-only), the row's length becomes
 * *n_reused (a multiple of block_tokens, < n: at least one token is left to run) and the caller prefills
 * tokens[*n_reused..n).  Identical tokens at identical positions give identical K / V, so this is exact up to the
 * summation-order noise between prefill shapes; hits are verified token by token, never by hash alone.
 * publish: the full blocks of tokens[0..n) (already in the row's cache, i.e. after its prefill was enqueued) become
 * reusable; they stay alive after the row is reset, until evicted (least recently used first) when a step needs a
 * block.  Eviction takes the deepest block of a chain before its parents (a chain is only reachable from its root).
 * clear: forget everything (after a weight or adapter update).
 * stats: out[0..n) = free blocks, usable blocks, cached (published) blocks, reused tokens, looked-up tokens, evictions,
 * evictable blocks (published blocks no live row maps: only these can be given back to a step that needs a block). */
int mi_kv_prefix_attach(mi_kv* kv, int row, const int32_t* tokens, int n, int* n_reused);
int mi_kv_prefix_publish(mi_kv* kv, int row, const int32_t* tokens, int n);
int mi_kv_prefix_clear(mi_kv* kv);
int mi_kv_stats(const mi_kv* kv, int64_t* out, int n);
void mi_kv_destroy(mi_kv* kv);
int mi_kv_reset(mi_kv* kv, int batch);               /* base.py:146-149 */
int mi_kv_reserve(mi_kv* kv, int capacity_tokens);   /* base.py:104-117 growth, contents kept */
int mi_kv_offsets(const mi_kv* kv, int32_t* out);    /* base.py:142-144: per-row lengths [B] */
int mi_kv_capacity(const mi_kv* kv);

/* ---- forward: replaces `model(y, cache=cache)` (utils.py:403; llama.py:243-253) --------- */
/* tokens [B,L] row-major.  L>1 = prefill with the additive causal mask of base.py:17-40
 * (left pads ARE attended, quirk Q1); L==1 = decode.  logits_out: NULL, or [B,V] floats of
 * the last position (utils.py:404), or [B,L,V] if all_pos.  Synchronous. */
int mi_forward(mi_engine* e, mi_kv* kv, const int32_t* tokens, int B, int L, float* logits_out,
               int all_pos);

/* ---- one generate_step iteration: `_step` (utils.py:401-418), synchronous -------------- */
/* tokens_in [B,L].  Outputs (any may be NULL): tokens_out [B]; logprob_out [B] =
 * log_softmax(logits)[b, token_b]; prob_row0_out [B] = softmax(logits)[0, token_b] (the
 * `probs` the reference yields, quirk Q6); topk_ids/topk_logprobs [B,top_logprobs]. */
int mi_decode_sample(mi_engine* e, mi_kv* kv, const int32_t* tokens_in, int B, int L,
                     const mi_sample_params* sp, int32_t* tokens_out, float* logprob_out,
                     float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs);

/* Teacher-forced scoring: the all-position logits + log-softmax gather of the server's echo /
 * perplexity paths (server/main.py:530-557, 646-654), through the KV cache instead of a re-run per
 * step.  Feeds tokens [B,L] (they are appended to `kv`), then for every position (b,i) reports
 * log softmax(logits[b,i] (+ logit_bias) (/ temperature if sp->logprobs_at_temperature))[targets[b,i]]
 * into logprob_out [B*L] (targets < 0: position skipped, 0.0 reported) and, if sp->top_logprobs = k > 0,
 * the k most likely ids / logprobs of that position into topk_ids / topk_logprobs [B*L,k].
 * Nothing is sampled; sp->top_p, uniforms, seed and the ABI 4 controls (top_k, min_p, row streams) are ignored. */
int mi_score_tokens(mi_engine* e, mi_kv* kv, const int32_t* tokens, const int32_t* targets, int B, int L,
                    const mi_sample_params* sp, float* logprob_out, int32_t* topk_ids, float* topk_logprobs);

/* ---- pipelined form of the same step: the reference's one-step-ahead
 *      mx.async_eval(next_y); mx.eval(y) (utils.py:420-427) ----------------------------- */
/* Enqueue one step on the engine's stream and return a ticket.  tokens_in == NULL feeds the
 * tokens sampled by the previous enqueued step (they never leave the device). */
int mi_step_enqueue(mi_engine* e, mi_kv* kv, const int32_t* tokens_in, int B, int L,
                    const mi_sample_params* sp, int64_t* ticket);
/* Continuous batching (server/main.py:1404-1726 admits requests between steps): the same step on a SUBSET of
 * the cache's rows.  rows[n] are distinct row indices of `kv` (its batch = the number of slots); tokens_in is
 * [n, L] in that order, or NULL to feed the tokens the previous step sampled -- then the previous step must have
 * had the same n (and, for meaningful results, the same rows in the same order).  Rows not named are untouched,
 * so a finished sequence's slot can be reset (mi_kv_reset_row) and prefilled with a new prompt (n = 1, L = its
 * length) while the other slots keep decoding in their own steps.  Results come back in `rows` order. */
int mi_step_enqueue_rows(mi_engine* e, mi_kv* kv, const int32_t* rows, int n, const int32_t* tokens_in, int L,
                         const mi_sample_params* sp, int64_t* ticket);
/* Chunked prefill co-scheduled with the live decode rows (the reference admits a request only between batches and
 * prefills it alone, server/main.py:1404-1726): ONE pass over the weights for n segments that advance by different
 * numbers of tokens.  Segment i appends lens[i] >= 1 tokens to cache row rows[i] (distinct rows); the one-token
 * segments (decode rows) must come first; `tokens` is the concatenation (sum of lens).  want[i] != 0: sample a token
 * from the logits after the segment's last position (every decode row, and the LAST chunk of a prompt); want[i] == 0:
 * an inner chunk, no logits.  mi_step_wait then returns the results of the wanted segments, in segment order (the
 * ticket's batch = their count; row_temperature / row_top_p and the other per-row arrays, if given, have one entry per wanted
 * segment).  Explicit
 * tokens only: the device-resident token feed of mi_step_enqueue(_rows) restarts after a mixed step. */
int mi_step_enqueue_mixed(mi_engine* e, mi_kv* kv, const int32_t* rows, const int32_t* lens, const int32_t* want, int n,
                          const int32_t* tokens, const mi_sample_params* sp, int64_t* ticket);
/* Forget the contents of one row (its length becomes 0); ordered behind the steps already enqueued. */
int mi_kv_reset_row(mi_kv* kv, int row);
/* Row `dst` (empty: mi_kv_reset_row first) becomes a copy of the first n_tokens tokens of row `src`, 1 <= n_tokens <= length
 * of src: the n choices of one request share one prompt prefill.  Paged cache: the full blocks are shared read-only (a block
 * that is not full is never shared) and the partly filled tail is copied into a block of dst's own, which costs one block --
 * none when n_tokens is a multiple of block_tokens.  Contiguous cache: all n_tokens are copied.  One launch either way, for
 * every layer, KV head, K and V.  dst's length becomes n_tokens; its logit_bias and logprobs setting are NOT forked: it starts
 * as an empty row does.  src keeps running untouched, and either row may be reset first.
 * Ordered on the engine's stream like mi_kv_reset_row: behind every step already enqueued (the pending appends of src are
 * in), ahead of every later one.
 * MI_ERR_INVALID, naming the argument, with nothing changed: a null kv; src or dst outside the cache; src == dst; a dst that is
 * not empty; n_tokens outside [1, length of src].  MI_ERR_RUNTIME when the arena has no block for the tail: nothing changed.
 * MI_ERR_RUNTIME when the launch or the length update fails: dst is empty again and its blocks are back in the arena, but a
 * prefix-cache block that was evicted to make room for the tail stays evicted. */
int mi_kv_fork_row(mi_kv* kv, int src, int dst, int n_tokens);
/* logit_bias of the REQUEST that occupies cache row `row` (the reference's logit_bias dict, utils.py:346-349, is one per call;
 * under continuous batching requests with different dicts share a step): n entries (ids[i], values[i]) replace the row's
 * bias, n == 0 clears it (ids / values may then be NULL).  Set once at admission, it travels with the row -- nothing is
 * uploaded per step: the device table [batch][MI_MAX_ROW_LOGIT_BIAS] belongs to the mi_kv (either form) and is allocated by
 * the first call that sets a bias, never inside a step.  mi_kv_reset_row clears the row's bias, mi_kv_reset every row's;
 * mi_kv_reserve and mi_kv_prefix_attach / _publish leave it alone.
 * Every entry point that samples through the mi_kv applies it: sampled row b of mi_decode_sample / mi_step_enqueue is cache
 * row b, sampled row i of mi_step_enqueue_rows is rows[i], wanted segment i of mi_step_enqueue_mixed is its segment's row.
 * The row's logits become float32(l + v) for its entries, in place and AFTER the call-wide list of mi_sample_params has been
 * added (an id in both lists gets both, in that order); the arg-max, the nucleus, top_k, min_p, the reported logprob, the
 * top-k logprobs and prob_row0_out all see the biased row.  mi_forward and mi_score_tokens ignore it.  A step on a cache
 * without a biased row is the step of a cache that never had one (the same kernel, bit-identical outputs).
 * Ordered on the engine's stream like mi_kv_reset_row: behind every step already enqueued, ahead of every later one.  The
 * arrays are copied into library-owned pinned staging before the call returns.
 * MI_ERR_INVALID, naming the argument, with nothing changed and the previous bias still in force: row outside the cache;
 * n < 0 or n > MI_MAX_ROW_LOGIT_BIAS; an id outside [0, vocab_size); an id that occurs twice; a value that is not finite. */
#define MI_MAX_ROW_LOGIT_BIAS 1024   /* entries per row (OpenAI allows 300) */
int mi_kv_set_row_logit_bias(mi_kv* kv, int row, const int32_t* ids, const float* values, int n);
/* logprobs of the REQUEST that occupies cache row `row` (the reference reports them for one request at a time,
 * server/main.py:571-584; under continuous batching requests that want them share a step with requests that do not):
 * top_logprobs in 0..MI_MAX_TOP_LOGPROBS is the row's own count of top entries, at_temperature != 0 reports the row's
 * logprob_out and top entries under softmax(logits / T_b), T_b the row's sampling temperature, when T_b > 0 (else the plain
 * log-softmax).  (0, 0) clears the row: it keeps the call's top_logprobs / logprobs_at_temperature again, as every row without
 * a setting does.  Like the bias it is set once at admission and travels with the row -- nothing is uploaded per step; the
 * device table [batch] belongs to the mi_kv (either form) and is allocated by the first call that sets a row, never inside a
 * step.  mi_kv_reset_row clears the row's setting, mi_kv_reset every row's; mi_kv_reserve and mi_kv_prefix_attach / _publish
 * leave it alone.  Every entry point that samples through the mi_kv obeys it, with the row mapping of the bias (sampled row b
 * of mi_decode_sample / mi_step_enqueue is cache row b, of mi_step_enqueue_rows rows[b], of mi_step_enqueue_mixed its wanted
 * segment's row); mi_score_tokens ignores it.  Ordered on the engine's stream like mi_kv_reset_row.
 * Layout: a step enqueued while at least one row of its cache has a setting returns topk_ids / topk_logprobs as
 * [B][MI_MAX_TOP_LOGPROBS] (mi_step_wait / mi_decode_sample copy B x MI_MAX_TOP_LOGPROBS entries: size the buffers for it):
 * a row's first k_b entries are its top list, the entries behind them hold id -1 and logprob -inf.  A row whose list runs past
 * its last comparable logit (k_b > the number of logits that are not NaN) gets id 0 and the logprob of -inf there, as the
 * call-wide count does.  A row with k_b = 0 costs no walk of its logits; from k_b = 4 on the list is selected in at most five
 * walks, whatever k_b, and is bit for bit the list that k_b rounds of arg-max give.  A step on a cache without a setting is
 * the step of a cache that never had one (the same kernel and arguments, the [B][top_logprobs] layout).
 * MI_ERR_INVALID, naming the argument, with nothing changed and the previous setting in force: row outside the cache;
 * top_logprobs outside [0, MI_MAX_TOP_LOGPROBS]; at_temperature other than 0 or 1. */
int mi_kv_set_row_logprobs(mi_kv* kv, int row, int top_logprobs, int at_temperature);
/* The adapter of the REQUEST that occupies cache row `row`: a slot of mi_engine_set_adapter_lora, or -1 = none (the default).
 * The row must be empty (length 0): its K / V depend on the adapter.  Like the other row settings it is set once at admission
 * and travels with the row; mi_kv_reset_row sets it back to -1, mi_kv_reset every row's.  mi_kv_fork_row wants dst to name
 * src's adapter already (MI_ERR_INVALID naming dst otherwise, nothing changed).  The slot may be filled later, but a step on
 * the row while the slot is empty is refused.  MI_ERR_INVALID, nothing changed: row outside the cache; adapter outside
 * [-1, MI_MAX_ADAPTERS); a row that is not empty. */
int mi_kv_set_row_adapter(mi_kv* kv, int row, int adapter);
/* Block until `ticket` has finished; copy out its results (same meaning as mi_decode_sample). */
int mi_step_wait(mi_engine* e, int64_t ticket, int32_t* tokens_out, float* logprob_out,
                 float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs);

/* ---- measurement hooks (bench.py) ------------------------------------------------------- */
/* Bracket every launch of the kernel family `name` ("gemv_gate_up", "gemv_qkv", "gemv_o",
 * "gemv_down", "gemv_head", "attn_decode", ...; NULL or "" = off) with HIP events on the
 * engine's own stream. */
int mi_profile_select(mi_engine* e, const char* name);
/* Drains the recorded events: number of launches and their summed duration in ms. */
int mi_profile_read(mi_engine* e, int64_t* n_launches, double* total_ms);
/* Engine switches (A/B measurement and tests); unknown key -> MI_ERR_NOTFOUND.
 *   "force_generic_gemv"      1: every linear layer on the generic VALU kernel (default 0)
 *   "fused_decode_attention"  0: decode attention as rope/append + attention + combine launches (default 1)
 *   "prefill_gemm"            0: prefill through the chunked <= 16-row kernels instead of the tile GEMM (default 1)
 *   "decode_attention_mfma"   0: the VALU form of the fused decode attention also for 16-bit caches (default 1)
 *   "skinny_gemm"             0: decode steps of 9..128 rows (int4 / int8 weights: of any size) through <= 16-row
 *                             launches of the M <= 16 kernels instead of the split-K streaming GEMM (default 1)
 *   "norm_handover"           0: decode steps of <= 16 rows through the split-K kernel run the RMSNorm as its own launch
 *                             instead of handing its row statistics from the residual epilogue of one launch to the
 *                             staging of the next (default 1)
 *   "defer_norm"              0: float32-activation (PagedKVCache mode) decode steps run the RMSNorm as its own launch
 *                             instead of applying its row scale in the epilogue of the linear behind it (default 1)
 *   "consumer_combine"        0 / 1, for float32-KV decode steps of one group of <= 8 rows on dense bf16 weights without LoRA
 *                             (everything else runs as with 0; outputs are bit-identical):
 *                             1: the q|k|v linear publishes its K slices' partial rows and ends; the decode attention's
 *                                prologue adds them (slice order) and applies the RMSNorm row scale (default);
 *                             0: the last workgroup to arrive combines inside the linear's launch.
 *                             Any other value: MI_ERR_INVALID, the option keeps its value.
 *   "consumer_combine_guard"  (a check, the value is ignored) MI_OK when the sentinels around the buffer of the q|k|v seam are
 *                             intact, MI_ERR_NOTFOUND when that seam has not run yet, MI_ERR_RUNTIME when one was overwritten
 *   "resident_x"              0 / 1, for the wide linears (gate|up, lm_head: at least 4 tiles per CU, K <= 4096) of float32-KV
 *                             decode steps of <= 8 rows on dense bf16 weights (outputs are bit-identical):
 *                             1: the one-pass GEMV keeps x and the norm weights in LDS for the whole launch (default);
 *                             0: it fetches them from L2 chunk by chunk (the form every other K runs on).
 *                             Any other value: MI_ERR_INVALID, the option keeps its value.
 *   "prefill_x_terms"         3: float32-activation (PagedKVCache mode) prefill multiplies an EXACT three-term 16-bit split of x
 *                             by dense bf16 weights (three walks of W); default 2: hi + lo, 16+ mantissa bits of x, two walks
 *                             (the CPU float32-accumulating variants do not move under it: DESIGN 8d); int4 always 3
 *   "short_prefill_skinny"    0: prefill calls of <= 128 rows in all through the tile GEMM like longer ones (default 1: the
 *                             weight-streaming split-K kernel of the decode steps, ~2x faster at that size)
 *   "tile_weights"            0: keep weights row-major (before mi_engine_finalize only; default 1)
 * Environment switches read per call by the library (reference paths for tests and A/B runs): MI_GEMM_DMA=0 (prefill:
 * the register-staged 256 x 256 tile instead of the LDS-DMA one), MI_GEMM_DMA_SPLITK=0 (no K split of the LDS-DMA tile),
 * MI_ATTN_PREFILL_DMA=0 (the register-staged prefill attention), MI_ATTN_PREFILL_F32_EXACT=1 (float32-KV prefill
 * attention with exact float32 products instead of two-term bf16 operands). */
int mi_engine_set_option(mi_engine* e, const char* key, int64_t value);
/* Blocks until the engine's stream is idle. */
int mi_engine_sync(mi_engine* e);

/* ---- merging an adapter into the base weights (the reference's tools/merge_lora.py is a stub) ------------------------
 * Stateless and synchronous: device pointers on device `device`, row-major tensors in checkpoint layout, no engine needed
 * (the caller's current device is restored).  T = dtype (MI_BF16 / MI_F16), W (N, K), A (K, rank) float32, B (rank, N) float32,
 * m (N,) float32 or NULL for LoRA, s the adapter's scale.  quant_bits 0: w is W in T and scales / biases are ignored;
 * 4 / 8: w is the MLX-packed uint32 (N, K bits / 32) with scales / biases (N, K / 64) in T, quant_group must be 64.
 * Arithmetic, every sum float32, in a fixed order (the same inputs give the same bits):
 *   Wd[n][k] = W[n][k], or T(scale q + bias) as ONE float32 multiply-add and one rounding
 *   b'[n][j] = T(s B[j][n]);  a'[j][k] = T(A[k][j])
 *   delta[n][k] = T(sum_j b'[n][j] a'[j][k])         an fmaf chain in ascending j from 0, one rounding at the end
 *   Wm = T(Wd + delta)
 *   with m: norm[n] = sqrt(sum_k Wm[n][k]^2) (a thread's k ascending in strides of 256, the wave sum, the four waves in
 *           order), g[n] = m[n] / norm[n] in float32, W' = T(g[n] Wm[n][k]);  without m: W' = Wm
 * requantize 0: out_w is W' in T (N, K), out_scales / out_biases are ignored -- also from a quantised input (a de-quantised
 * merge).  requantize 1 (quantised input only): W' is quantised again with the input's bits and group by mi_quantize_mlx's
 * kernel into out_w (packed) / out_scales / out_biases.  A linear bias is not an argument: merging leaves it as it is.
 * These steps restate mlx-lm's LoRALinear.fuse, DoRALinear.fuse and QuantizedLinear.from_linear from their published code;
 * they could not be run against mlx-lm.
 * MI_ERR_UNSUPPORTED: dtype MI_F32; m together with a quantised input (mi_engine_set_dora refuses DoRA on quantised weights
 * for the same reason); quant_group 32 or 128; K % 64 != 0 when quantised.  MI_ERR_INVALID: rank outside 1..64, a null or
 * misaligned buffer, requantize with a dense input, an s or an m[n] that is not finite, a merged row whose norm is 0 or not
 * finite (the message names the row).  A refused call writes nothing to the outputs. */
int mi_lora_merge(int device, int N, int K, int rank, int dtype, int quant_bits, int quant_group, const void* w,
                  const void* scales, const void* biases, const float* A, const float* B, const float* m, float s,
                  int requantize, void* out_w, void* out_scales, void* out_biases);
/* The quantiser alone: w (N, K) in T -> out_w uint32 (N, K bits / 32), out_scales / out_biases (N, K / 64) in T; bits 4 or 8,
 * group 64 (32 / 128: MI_ERR_UNSUPPORTED, as K % 64 != 0 and dtype MI_F32).  mx.quantize as published: per group of 64,
 * scale = max((max - min) / (2^bits - 1), 1e-7) signed towards the edge of larger magnitude, the edge snapped to a code, the
 * codes from the unrounded float32 scale and bias (IEEE division, round half to even), then scale and bias rounded to T. */
int mi_quantize_mlx(int device, int N, int K, int dtype, int bits, int group, const void* w, void* out_w, void* out_scales,
                    void* out_biases);

const char* mi_last_error(void);
const char* mi_version(void);
int mi_abi_version(void);                  /* MI_ABI_VERSION of the loaded library */

#ifdef __cplusplus
}
#endif
#endif /* MI355_DECODE_H */
