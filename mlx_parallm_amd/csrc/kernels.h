// kernels.h -- host-side launch interface of the HIP kernels (internal to the library).
#pragma once
#include "common.h"

namespace mi {

// One (possibly fused) weight matrix W[N][K] as the kernels see it.
struct LinearW {
  int wk = WK_F32;             // weight kind (common.h)
  const void* w = nullptr;     // dense [N][K] or MLX-packed [N][K*bits/32] uint32
  const void* scales = nullptr;  // [N][K/group] in the scale dtype
  const void* biases = nullptr;
  int N = 0, K = 0, group = 64;
  int layout = 0;              // 0 = row-major (checkpoint order); 1 = tile-major (repack.hip); then
                               // `w` is the single tiled buffer (int4: scales/biases live inside it)
  // LoRA (mlx-lm LoRALinear): rows [lora_row0, lora_row0+lora_n) of this (fused) matrix get
  // + scale * ((x A) B); A [K][r], B [r][lora_n] stored as float32.  DEAD since the engine-wide adapter runs through
  // lora_rows.hip: nothing sets these members or GemvCall::lora_t, the epilogues' lora_term always returns at once (DESIGN §5,
  // "One LoRA path": why they are still here).
  const float* lora_a[2] = {nullptr, nullptr};
  const float* lora_b[2] = {nullptr, nullptr};
  int lora_row0[2] = {0, 0}, lora_n[2] = {0, 0}, lora_rank[2] = {0, 0};
  float lora_scale[2] = {0.f, 0.f};
  // nn.Linear(bias=True) / nn.QuantizedLinear(bias=True) (llama.py:59-67,155-162): [N] float32, the checkpoint's values,
  // concatenated across the parts of a fused matrix; null = no bias.  Dense weights: y = T(acc + b) (mx.addmm, one
  // rounding); quantised weights: y = T(T(acc) + b) (quantized_matmul, then + bias) -- add_bias() in common.h.
  const float* bias = nullptr;
};

enum : int { PRO_NONE = 0, PRO_NORM = 1 };
enum : int {
  EPI_STORE = 0,      // out[m][n] = T(acc)
  EPI_STORE_F32 = 1,  // out_f32[m][n] = float(T(acc))            (logits for the sampler)
  EPI_RESID = 2,      // resid[m][n] = T(resid[m][n] + T(acc))     (h = x + r, llama.py:188,190)
  EPI_SWIGLU = 3,     // out[m][n] = T(T(silu(g)) * u), g/u = rows n, n+pair_offset (llama.py:165)
  EPI_SWIGLU_GU8 = 4, // the same on the row-interleaved copy of a gate|up matrix (tile t = gate rows 8t..8t+7, then up rows
                      // 8t..8t+7; launch_gate_up_interleave): a PLAIN one-stream GEMV over 2 x pair_offset rows whose
                      // epilogue pairs columns j and j + 8 of every tile -- gemv_mfma only (decode steps of <= 16 rows)
};

struct GemvCall {
  const void* x = nullptr;  // [M][ldx] activations (storage type `act`)
  int ldx = 0;
  int M = 0;
  int act = MI_F32;         // storage type of x / out / resid / norm_w
  int rnd = RND_NONE;       // logical rounding applied on top of the storage type
  int pro = PRO_NONE;
  const void* norm_w = nullptr;  // [K] RMSNorm weight (PRO_NORM)
  float eps = 0.f;
  int epi = EPI_STORE;
  void* out = nullptr;
  int ldo = 0;
  void* resid = nullptr;
  int pair_offset = 0;
  const float* lora_t = nullptr;  // [M][2][max_rank] = round(x A) for the (up to 2) adapted row ranges
  int lora_t_ld = 0;
  int force_v1 = 0;
  int kx = 0;                     // > 0: W is a [hi | lo] matrix of 2 kx columns (an f16 model in the float32-activation mode): the
                                  // activations have kx columns and are walked twice (k mod kx); 0: W.K columns
  // RMSNorm hand-over between two launches of gemm_skinny.hip's 16-row instantiation: a residual epilogue leaves
  // sum(h^2) per (tile group, row) in sq_out; the next linear (pro = PRO_NORM) reads them as sq_in[sq_parts][16]
  float* sq_out = nullptr;
  const float* sq_in = nullptr;
  int sq_parts = 0;
  // consumer_combine (gemm_skinny.hip, the bf16_publish form; a decode step of <= 8 float32 rows on a dense bf16 linear without
  // LoRA -- launch_gemm_skinny refuses anything else): publish only -- the K slices' partial tiles go row-major to cc_pub
  // [ksplit][8][N] and their row sums of squares to cc_pub_sq [ksplit][8]; nothing is combined and c.out is not written (the
  // decode attention adds them).  The engine's router (gemv_rows_on) takes the pointers as an OFFER: it clears them on every
  // route but that one.
  float* cc_pub = nullptr; float* cc_pub_sq = nullptr;
  void* ev_start = nullptr;       // measurement: hipEvent_t pair stamped with this kernel's own begin / end
  void* ev_stop = nullptr;        // (hipExtLaunchKernelGGL); MFMA path only
};

int launch_gemv(const LinearW& W, const GemvCall& c, hipStream_t st);

// prefill (many rows): MFMA tile GEMM + row-wise RMSNorm (gemm_prefill.hip)
bool gemm_prefill_supported(const LinearW& W, const GemvCall& c, size_t rows);
// splitk_ws / splitk_cap: float32 workspace for the K-split form of the 128 x 128 tile (few hundred rows against a narrow
// matrix); null = never split
int launch_gemm_prefill(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* scratch = nullptr,
                        void* splitk_ws = nullptr, size_t splitk_cap = 0);
// float32 activations (PagedKVCache mode) in front of launch_gemm_prefill: rows of [hi | mid | lo] bf16, 3 K wide, with the
// RMSNorm (norm_w = float32 weights, or null) applied first; then call launch_gemm_prefill with c.x = out, c.ldx = 3 K
size_t split3_bytes(size_t rows, int K);
int launch_split3_rows(const void* x, int ldx, const void* norm_w, float eps, void* out, int rows, int K, hipStream_t st,
                       int terms = 3);
// int4 (tile-major) -> 16-bit tile-major [hi | lo], K' = 2K: the operand of the prefill GEMM for quantised weights
size_t dequant_hilo_bytes(int N, int K);
int launch_dequant_q4_hilo(const LinearW& src, void* dst, hipStream_t st);
// block_per_row: one workgroup per row, row in registers -- for the few rows of a decode step (default: one wave
// per row, the prefill's kernel; the two add the squares in different orders)
// act = MI_F32: float32 rows and weights with the run-time logical rounding `rnd` (PagedKVCache mode)
int launch_rmsnorm_rows(const void* x, int ldx, const void* w, void* out, int ldo, int rows, int H, float eps, int act,
                        hipStream_t st, bool block_per_row = false, int rnd = 0);

// 9..64 rows, int8 weights 1..64 (decode steps of larger batches): weight-streaming split-K GEMM (gemm_skinny.hip).
// c.pro must be PRO_NONE; `ws` >= gemm_skinny_ws_bytes(), `ctr` >= gemm_skinny_groups() words that are zero between
// launches (the kernel leaves them zero); ksplit = 0 lets the cost model choose.
bool gemm_skinny_supported(const LinearW& W, const GemvCall& c, size_t rows);
size_t gemm_skinny_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows);
int gemm_skinny_groups(const LinearW& W, const GemvCall& c, size_t rows);
int gemm_skinny_ksplit(const LinearW& W, const GemvCall& c, size_t rows);
int gemm_skinny_handover_ld(const LinearW& W, const GemvCall& c, size_t rows);     // > 0: the call can leave / take the RMSNorm hand-over
int gemm_skinny_tile_groups(const LinearW& W, const GemvCall& c, size_t rows);
int launch_gemm_skinny(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr,
                       int ksplit = 0);

// float32 activations (no logical rounding), <= 8 rows, dense bf16 tile-major weights (gemv_f32.hip): one pass over W, one
// workgroup per CU, no K split, no workspace; RMSNorm (c.pro = PRO_NORM) deferred to the epilogue.  Epilogues: EPI_STORE /
// EPI_STORE_F32 / EPI_RESID in float32, EPI_SWIGLU_GU8 on the row-interleaved gate|up copy (W = the copy).
bool gemv_f32_supported(const LinearW& W, const GemvCall& c);
int launch_gemv_f32(const LinearW& W, const GemvCall& c, hipStream_t st);
// the same operator, bit for bit, for a NARROW linear of K <= 4096 (o_proj): one 16-row tile per workgroup over the whole K,
// at most one tile per CU, c.pro = PRO_NONE, EPI_STORE / EPI_STORE_F32 / EPI_RESID; every load of the launch issued up front
bool gemv_f32_whole_supported(const LinearW& W, const GemvCall& c);
int launch_gemv_f32_whole(const LinearW& W, const GemvCall& c, hipStream_t st);
// the same operator, bit for bit, for the WIDE linears of K <= 4096 (gate|up, lm_head): the stream of launch_gemv_f32 with
// x and the norm weights staged once per workgroup and kept in LDS (152.25 KiB at K = 4096), so that the stream loop waits
// for weight loads only; everything gemv_f32_supported takes at such a K
bool gemv_f32_resident_supported(const LinearW& W, const GemvCall& c);
int launch_gemv_f32_resident(const LinearW& W, const GemvCall& c, hipStream_t st);
int gemv_cu_count();            // compute units of the current device (gemv_mfma.hip)

// int4 (group 64) weights, 17..128 rows of 16-bit activations (gemm_q4.hip): x prepared once per launch (fragment-major,
// with the RMSNorm of c.pro = PRO_NORM applied there), K split over the waves of a workgroup.  launch_gemm_skinny routes
// to it; `ws` >= gemm_q4_ws_bytes() (preparation buffers + partial tiles), `ctr` >= gemm_q4_groups() zeroed words.
bool gemm_q4_supported(const LinearW& W, const GemvCall& c, size_t rows);
size_t gemm_q4_ws_bytes(const LinearW& W, const GemvCall& c, size_t rows);
int gemm_q4_groups(const LinearW& W, const GemvCall& c, size_t rows);
int gemm_q4_ksplit(const LinearW& W, const GemvCall& c, size_t rows);
void gemm_q4_force(int code);     // test / A-B hook: mt | TW << 3 | KW << 7 | ksplit << 11 | NS << 15 for this thread's next plans; 0 clears
int launch_gemm_q4(const LinearW& W, const GemvCall& c, size_t rows, hipStream_t st, void* ws, unsigned* ctr);

// tile-major weight layout (repack.hip)
bool tiled_supported(int wk, int N, int K, int group);
size_t tiled_bytes(int wk, int N, int K);
int launch_repack_tiled(const LinearW& src_row_major, void* dst, hipStream_t st);
// tile-major f16 (N x K) -> tile-major bf16 [hi | lo] (N x 2K), hi + lo == w exactly (repack.hip); dst: 2 x the source's bytes
int launch_f16_to_hilo(const LinearW& tiled_f16, void* dst, hipStream_t st);
// tile-major gate|up (rows [0, I) gate, [I, 2 I) up) -> tile-major with tile t = {gate rows 8t..8t+7, up rows 8t..8t+7}
int launch_gate_up_interleave(const LinearW& tiled, int pair_offset, void* dst, hipStream_t st);

// byte offset of the 16-byte piece holding W[row][k .. k+8) (k % 8 == 0) of a tile-major dense matrix
__host__ __device__ inline size_t tiled_piece_dense16(size_t row, int k, int K) {
  return (((row >> 4) * (size_t)(K / 32) + (size_t)(k >> 5)) * 64 + (size_t)(((k >> 3) & 3) * 16 + (int)(row & 15))) * 16;
}
// tile-major int4: byte offset of the block of (row, k), of the dword holding codes k..k+8, and of the scale / bias
__host__ __device__ inline size_t tiled_block_q4(size_t row, int k, int K) {
  return ((row >> 4) * (size_t)(K / 128) + (size_t)(k >> 7)) * 1152;
}
__host__ __device__ inline int tiled_q4_code_off(size_t row, int k) {   // within the block, bytes
  const int dd = (k >> 3) & 15;
  return (((dd >> 2) * 16 + (int)(row & 15)) * 4 + (dd & 3)) * 4;
}
__host__ __device__ inline int tiled_q4_scale_off(size_t row, int k) {  // + 64 for the bias
  return 1024 + (int)(row & 15) * 4 + ((k >> 6) & 1) * 2;
}
// tile-major int8 (group 64): block (row tile, k / 64) of 1088 bytes = [1024 codes: lane l = g*16 + r owns the 16
// codes W[16i + r][64j + 16g .. +16)] [32 B scales: row r -> one 16-bit value] [32 B biases]
__host__ __device__ inline size_t tiled_block_q8(size_t row, int k, int K) {
  return ((row >> 4) * (size_t)(K / 64) + (size_t)(k >> 6)) * 1088;
}
__host__ __device__ inline int tiled_q8_code_off(size_t row, int k) {   // within the block, bytes
  return (((k >> 4) & 3) * 16 + (int)(row & 15)) * 16 + (k & 15);
}
__host__ __device__ inline int tiled_q8_scale_off(size_t row) { return 1024 + (int)(row & 15) * 2; }   // + 32 for the bias

// ---- lora_rows.hip (the LoRA launches themselves: lora_rows.h)
// out[m][n] = T(T(g * T(sigmoid(g))) * u) with g = x[m][n], u = x[m][I + n]: the SwiGLU of a gate|up output stored by an
// EPI_STORE launch (an adapted gate|up), rounding points of EPI_SWIGLU.  I % 8 == 0, ldx >= 2 I, ldo >= I, any M, one launch.
int launch_swiglu_rows(const void* x, int ldx, void* out, int ldo, int M, int I, int act, int rnd, hipStream_t st);

// ---- moe.hip: the sparse mixture-of-experts MLP (mixtral.py:95-119).  T = the storage type `act` of the activations (with
// the logical rounding `rnd` on top of float32); expert weights are dense 16-bit (`wdt` = MI_BF16 / MI_F16, = act unless act
// is MI_F32, where they are widened exactly), row-major as in the checkpoint.  A pair is p = row * k + j.
constexpr int MOE_MAX_EXPERTS = 16;
// g = T(xn Wg^T) in float32 accumulation; sel[row][j] = the k largest in descending order, a tie to the lower expert index;
// score = T(softmax_float32(g[sel])); then the work lists by a scan (reproducible, ascending pairs): meta[e] = the number of
// pairs of expert e, meta[E + e] = where its run starts in list[R k].  Two kernels, no host round trip.  H % 64 == 0.
struct MoeRouteCall {
  const void* xn; int ldx, R, H, act, rnd;
  const void* wg; int wdt, E, k;         // Wg [E][H]
  int32_t* sel; void* score;             // [R][k] each (score in T)
  int32_t* meta; int32_t* list;          // [2 E], [R k]
};
int launch_moe_route(const MoeRouteCall& c, hipStream_t st);
// out[p][n] = T(x[p >> x_shift] . w_e[n]) for every pair p on the list of expert e (plain store), or with swiglu
// T(T(silu(g)) u) of g = T(x . w_e[n]), u = T(x . w2_e[n]) (linear_epilogue.h).  w, w2: [E][N][K].  N % 64 == 0, K % 64 == 0.
// Pairs on no list are not written; an expert without pairs costs a workgroup's launch and nothing else.
struct MoeLinearCall {
  const void* x; int ldx, x_shift, act, rnd;
  const void* w; const void* w2; int wdt, E, N, K, swiglu;
  const int32_t* meta; const int32_t* list;
  void* out; int ldo;
};
int launch_moe_linear(const MoeLinearCall& c, hipStream_t st);
// r = T(T(y[row k] s[row k]) + T(y[row k + 1] s[row k + 1])) (k = 1: the first term), out[row] = resid ? T(resid[row] + r) : r
int launch_moe_combine(const void* y, const void* score, int k, const void* resid, int ldr, void* out, int ldo, int R, int H,
                       int act, int rnd, hipStream_t st);

struct EmbedCall {
  const int32_t* tokens;  // device [rows]
  int rows;
  int act, rnd;
  void* out;  // [rows][H]
};
int launch_embed(const LinearW& W, const EmbedCall& c, hipStream_t st);

struct AttnShape {
  int B, L, Hq, Hkv, D;
  int act;      // storage type of qkv / q / out
  int kv;       // storage type of the caches
  int rnd;      // logical rounding of q, k (after norm / rope) and of the attention output
  int cap;      // cache capacity (tokens)
  const int32_t* rows;  // device [B] or null: batch entry b lives in cache row rows[b] (continuous batching:
                        // the call covers a subset of the cache's rows); offsets[] is indexed by cache row
  // Block-paged cache (mi_kv_create_paged): the cache arrays are arenas [block][Hkv][1 << bs_shift][D] and token `key` of
  // cache row r lives in block btab[r * bt_stride + (key >> bs_shift)].  btab == null: contiguous [row][Hkv][cap][D].
  const int32_t* btab;
  int bt_stride;
  int bs_shift;
};

// element index of (cache row kb, kv head kh, token key, d = 0) in a K or V array
template <bool PAGED>
__device__ __forceinline__ size_t kv_elem(const AttnShape& s, int kb, int kh, int key) {
  if constexpr (PAGED) {
    const int blk = s.btab[(size_t)kb * s.bt_stride + (key >> s.bs_shift)];
    return ((((size_t)blk * s.Hkv + kh) << s.bs_shift) + (size_t)(key & ((1 << s.bs_shift) - 1))) * s.D;
  } else {
    return (((size_t)kb * s.Hkv + kh) * s.cap + key) * s.D;
  }
}
struct RopeAppendCall {
  AttnShape s;
  const void* qkv;       // [B*L][(Hq+2Hkv)*D]
  void* q_out;           // [B*L][Hq*D]
  void* kcache;          // [B][Hkv][cap][D]
  void* vcache;
  const int32_t* offsets;  // device [B]: tokens already in the cache
  const void* q_norm_w;  // [D] or null (qwen3.py:65-70)
  const void* k_norm_w;
  float eps;
  const float* cos_tab;  // [max_pos][D/2]
  const float* sin_tab;
  int max_pos;
};
int launch_rope_append(const RopeAppendCall& c, hipStream_t st);

struct AttnCall {
  AttnShape s;
  const void* q;         // [B*L][Hq*D] (normed + roped)
  const void* kcache;
  const void* vcache;
  const int32_t* offsets;  // device [B]: tokens in the cache BEFORE this call's L were appended
  void* out;             // [B*L][Hq*D]
  float scale;
  int nsplit;            // >1 only for L == 1
  float* partial;        // [B*L*Hq][nsplit][D+2] when nsplit > 1
  int variant;           // 0: L > 1 goes to the MFMA prefill kernel where it applies; 1: always the VALU kernel
};
int launch_attention(const AttnCall& c, hipStream_t st);
// causal prefill attention on the matrix cores (attn_prefill.hip); launch_attention dispatches to it
bool attention_prefill_supported(const AttnShape& s);
int launch_attention_prefill(const AttnCall& c, hipStream_t st);

// fused decode step (L == 1): q/k norm + RoPE + KV append + split-KV attention + combine
struct AttnDecodeCall {
  AttnShape s;             // s.rnd = logical rounding of q / k after norm and RoPE
  const void* qkv;         // [B][(Hq+2Hkv)*D] raw projections
  void* kcache;
  void* vcache;
  const int32_t* offsets;  // device [B]: tokens already in the cache
  const void* q_norm_w;
  const void* k_norm_w;
  float eps;
  const float* cos_tab;
  const float* sin_tab;
  void* out;               // [B][Hq*D]
  float scale;
  int rnd_out;             // logical rounding of the attention output
  int nsplit;
  float* partial;          // [B*Hq][nsplit][D+2]
  int* counters;           // [B*Hkv] zero-initialised arrival tickets
  int variant;             // 0: MFMA kernel where it applies (16-bit caches, D % 32 == 0; float32, D 64 / 128); 1: VALU kernel
  int n_host_off;          // > 0: host_off[b] = offsets[cache row of b], host_row[b] = that cache row (B <= 32)
  int host_off[32];
  int host_row[32];
  // consumer_combine (float32 MFMA kernel, B <= 8): qkv is not read -- row b of it is the sum of the qkv_ksplit
  // partial rows qkv_pub[s][b][:] (slice order, from zero) times the RMSNorm row scale from qkv_pub_sq[s][b] (sums of squares
  // of the hidden_k inputs).  qkv_pub == null: the ordinary launch.
  const float* qkv_pub = nullptr; const float* qkv_pub_sq = nullptr;
  int qkv_ksplit = 0, hidden_k = 0;
  float qkv_eps = 0.f;
};
int launch_attention_decode(const AttnDecodeCall& c, hipStream_t st);
bool attention_decode_supported(const AttnShape& s);
bool gemv_mfma_supported(const LinearW& W, const GemvCall& c);

struct SampleCall {
  float* logits;         // [B][V] float32 (modified in place by logit_bias)
  int B, V;
  int rnd;
  float temperature, top_p;
  int n_bias;
  const int32_t* bias_ids;   // device
  const float* bias_vals;    // device
  const float* uniforms;     // device [B] or null
  uint64_t seed, step;       // Philox key/counter when uniforms == null
  int top_logprobs;
  int lp_temp;               // report logprobs under softmax(logits / temperature) (temperature > 0)
  const int32_t* forced;     // device [B] or null: teacher forcing -- score these ids instead of sampling (< 0: skip row)
  const float* row_temp;     // device [B] or null: per-row temperature / top_p instead of the scalars
  const float* row_top_p;
  int32_t* tokens_out;       // device [B]
  float* logprob_out;        // device [B]
  float* prob_row0_out;      // device [B]
  int32_t* topk_ids;         // device [B][top_logprobs]
  float* topk_logprobs;
  float* row_stats;          // device [B][2] scratch: (max, logsumexp)
  // top-k / min-p / per-row streams (sample_kernel<true>).  Behind the older fields, whose offsets the kernel without them keeps
  int top_k = 0;             // 0 < top_k < V: keep the first top_k candidates of the order (else off)
  float min_p = 0.f;         // 0 < min_p <= 1: keep p >= min_p * p_max, as (l - max) * (1/T) >= logf(min_p) in float32 (0: off)
  const int32_t* row_top_k = nullptr;    // device [B] or null: per-row top_k / min_p instead of the scalars (each on its own)
  const float* row_min_p = nullptr;
  const uint64_t* row_seed = nullptr;    // device [B], both or neither: row b with row_position[b] >= 0 draws
  const int64_t* row_position = nullptr; // philox(row_seed[b], row_position[b], 0); < 0: the call-wide (seed, step, b)
  // per-row logit_bias table (sample_kernel<*, true>; rb_cnt == null: the kernels without it).  Sampled row b adds the
  // rb_cnt[t] entries (rb_ids[t][i], rb_vals[t][i]) of table row t = rb_map ? rb_map[b] : b, after the call-wide list;
  // a t outside [0, rb_rows) and entries past rb_cap or with an id outside [0, V) are skipped
  const int32_t* rb_cnt = nullptr;       // device [rb_rows]
  const int32_t* rb_ids = nullptr;       // device [rb_rows][rb_cap]
  const float* rb_vals = nullptr;        // device [rb_rows][rb_cap]
  const int32_t* rb_map = nullptr;       // device [B] or null: the identity
  int rb_rows = 0, rb_cap = 0;
  // per-row logprobs settings (sample_kernel<*, true, true>; lp_k == null: the kernels without them).  Sampled row b on table
  // row t = rb_map ? rb_map[b] : b (t in [0, rb_rows)) with lp_k[t] >= 0 reports lp_k[t] top entries and, with lp_flag[t] != 0
  // and a row temperature > 0, logprobs under softmax(logits / T_b); lp_k[t] < 0 (or t outside the table): the call's
  // top_logprobs / lp_temp.  topk_ids / topk_logprobs are then [B][topk_stride]; entries past a row's count hold (-1, -inf).
  // rb_cnt may be null with lp_k set (settings without a bias table)
  const int32_t* lp_k = nullptr;         // device [rb_rows]
  const int32_t* lp_flag = nullptr;      // device [rb_rows]
  int topk_stride = 0;                   // >= every count (MI_MAX_TOP_LOGPROBS)
  int lp_method = 0;                     // 0: per row by LP_SELECT_MIN_K; 1: the k-round form on every row; 2: the selection
};
int launch_sample(const SampleCall& c, hipStream_t st);

int launch_advance_offsets(int32_t* offsets, const int32_t* rows, int B, int L, hipStream_t st);
// dst[i][:] = src[idx[i]][:] for n rows of row_bytes (a multiple of 16) each; idx on the device
int launch_gather_rows(const void* src, size_t row_bytes, const int32_t* idx, int n, void* dst, hipStream_t st);
// the first tokens of a cache row given to another row (mi_kv_fork_row): for every layer, kv head and for K and V alike, the
// n_tokens x D elements at src_off go to dst_off -- element offsets of head 0 inside a layer of layer_elems elements, head h
// at + h x head_stride.  One launch, 16-byte pieces; everything must be a multiple of 16 bytes and the spans apart.
int launch_kv_copy_tokens(void* kcache, void* vcache, int kv_dtype, int layers, size_t layer_elems, int Hkv, int D,
                          size_t head_stride, size_t src_off, size_t dst_off, int n_tokens, hipStream_t st);
// rope_traditional (llama.py:77-82) at load time: dst row (h D + j) = src row (h D + 2 j), dst row (h D + D/2 + j) = src row
// (h D + 2 j + 1) for j < D/2, over nrows = heads x D rows of row_bytes each (src != dst).  Applied alike to the q and k rows of
// a q|k|v matrix (codes, scales, quantisation biases), to their linear biases and to the columns of a LoRA B (as rows of
// 4 bytes, nrows = rank x n), it turns the interleaved rotation into the half-split one of the kernels; q.k is unchanged.
int launch_head_perm_rows(const void* src, void* dst, size_t nrows, int D, size_t row_bytes, hipStream_t st);
int launch_rope_tables(float* cos_tab, float* sin_tab, int max_pos, int D, float base, float scale,
                       hipStream_t st);
int launch_convert(const void* src, int src_dt, void* dst, int dst_dt, size_t n, hipStream_t st);

}  // namespace mi
