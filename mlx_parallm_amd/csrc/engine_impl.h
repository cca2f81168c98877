// engine_impl.h -- what the engine*.hip files share (included by nothing else): the host runtime behind the C ABI of
// include/mi355_decode.h.
//   engine.hip         create / destroy, workspace, the forward pass, sampling and steps, options, profiling, errors
//   engine_load.hip    checkpoint tensors and LoRA factors in, finalize (repacking, persistent second copies)
//   engine_linear.hip  gemv_rows: which kernel family a linear runs on, route by route
//   engine_kv.hip      the mi_kv_* entry points (the paged cache's host state: kv_blocks.h)
//
// One mi_engine = one model replica on one MI355X: device-resident weights (q|k|v and gate|up
// fused into single matrices), RoPE tables, an activation workspace, a private HIP stream and
// a small ring of pinned result slots for the one-step-ahead pipelining of generate_step
// (utils.py:420-427).  One mi_kv = the per-layer KV buffers of one batch, laid out
// [layer][B][Hkv][capacity][D], plus per-row lengths that live ON THE DEVICE so that a decode
// step needs no host data at all.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "kernels.h"
#include "kv_blocks.h"
#include "lora_rows.h"

namespace mi {

// The adapters of one fused matrix: the device table [part][LORA_TABLE_COLS] that lora_rows.hip reads, its host mirror (which
// owns the factors) and the number of entries that hold factors.  Columns 0 .. MI_MAX_ADAPTERS - 1 are the per-request slots
// (mi_engine_set_adapter_lora); column LORA_ENGINE_COL is the engine-wide adapter (mi_engine_set_lora), which no public slot
// number reaches.  Allocated by the first adapter that covers the matrix; a matrix without one keeps its fused launches in
// every step.
struct AdapterTable {
  AdapterPart h[3][LORA_TABLE_COLS];
  AdapterPart* d = nullptr;
  int set = 0;
  int gains = 0;                 // entries that carry a DoRA gain (> 0: the up-add's gain-aware instantiation, lora_rows.h)
  bool engine_wide() const { return h[0][LORA_ENGINE_COL].a || h[1][LORA_ENGINE_COL].a || h[2][LORA_ENGINE_COL].a; }
};

struct FusedLinear {
  LinearW W;
  int parts = 0;                 // bit mask of sub-tensors seen (weight / scales / biases per part)
  int n_parts = 1;
  int part_rows[3] = {0, 0, 0};
  bool quant = false;
  int dense_dtype = -1, scale_dtype = -1;
  size_t w_bytes = 0, s_bytes = 0;
  void* w = nullptr; void* scales = nullptr; void* biases = nullptr;
  // Persistent second copies of a matrix (made by mi_engine_finalize, i.e. BEFORE a scheduler sizes its KV arena from the
  // free device memory; a pointer is published only after its repack launch succeeded; when the allocation fails the
  // copy is marked unavailable and the linear keeps its plain path -- ensure_hilo / ensure_gu8)
  void* w_hilo = nullptr;        // f16 dense weights in the float32-activation (PagedKVCache) mode: [hi | lo] bf16 copy
  void* w_gu8 = nullptr;         // dense 16-bit gate|up: row-interleaved copy for the decode GEMV (EPI_SWIGLU_GU8)
  bool hilo_failed = false, gu8_failed = false;
  AdapterTable* adapters = nullptr;      // (a pointer: the [hi | lo] view of gemv_rows copies this struct)
  int seen_w[3] = {0, 0, 0}, seen_s[3] = {0, 0, 0}, seen_b[3] = {0, 0, 0};
  float* bias = nullptr;         // [rows of all parts] float32: the parts' `.bias` tensors (attention_bias / mlp_bias), as loaded
  int seen_bias[3] = {0, 0, 0};
  bool qk_regrouped = false;     // rope_traditional: permute_qk_heads has run (a finalize that failed later is not repeated on it)
};

struct LayerW {
  FusedLinear qkv, o, gate_up, down;
  void* in_norm = nullptr; void* post_norm = nullptr; void* q_norm = nullptr; void* k_norm = nullptr;
  // float32 copies for the float32-activation ("PagedKVCache quirk") mode
  void* in_norm32 = nullptr; void* post_norm32 = nullptr; void* q_norm32 = nullptr; void* k_norm32 = nullptr;
  // MI_ARCH_MIXTRAL (gate_up and down stay empty): the router [E][H] and the experts' matrices stacked by expert, dense in the
  // model dtype, row-major as loaded -- gate [E][I][H], up [E][I][H], down [E][H][I].  moe_seen[t][e]: slot e of tensor t
  // (0 gate, 1 up, 2 down) was set, by the stacked tensor or by the expert's own
  void* moe_router = nullptr; void* moe_w[3] = {nullptr, nullptr, nullptr};
  std::vector<char> moe_seen[3];
};

constexpr int NSLOT = 4;
struct Slot {
  hipEvent_t ev = nullptr;
  int32_t* tokens = nullptr; float* logprob = nullptr; float* prob0 = nullptr;
  int32_t* topk_ids = nullptr; float* topk_lp = nullptr;   // pinned host
  int B = 0, topk = 0; int64_t ticket = -1;
};

// RMSNorm hand-over between gemm_skinny launches (GemvCall::sq_out / sq_in): the residual linear in front of a norm
// leaves the rows' sums of squares in mi_engine::d_sq, the normalised linear behind it uses them instead of an rmsnorm launch
struct NormHandover {
  bool valid = false;
  const void* src = nullptr;     // the rows that were summed (the producer's resid)
  int parts = 0, K = 0, ld = 0;  // tile groups that left a sum each | columns summed | row stride of the table
  // does the producer's leftover describe x [rows][K] for a consumer whose plan reads a table of stride `take_ld`?
  bool matches(const void* x, int K_, int take_ld) const { return valid && take_ld == ld && src == x && K == K_; }
  void record(const void* src_, int parts_, int K_, int ld_) { valid = true; src = src_; parts = parts_; K = K_; ld = ld_; }
};

// A device buffer grown on demand.  need > *cap: the stream drains, the old buffer goes and *p = null, *cap = 0 until the new
// allocation succeeded -- a failed growth never leaves a freed pointer behind a capacity that passes the next check.
template <class T>
int grow(hipStream_t st, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return MI_OK;
  MI_HIP(hipStreamSynchronize(st));
  hipFree(*p); *p = nullptr; *cap = 0;
  MI_HIP(hipMalloc(p, need));
  *cap = need;
  return MI_OK;
}

}  // namespace mi

struct mi_engine {
  mi_model_desc d{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<mi::LayerW> layers;
  mi::FusedLinear embed, lm_head;
  void* final_norm = nullptr; void* final_norm32 = nullptr;
  bool finalized = false;
  float* cos_tab = nullptr; float* sin_tab = nullptr;
  // workspace (the *_cap of a buffer that mi::grow manages: bytes)
  size_t ws_rows = 0;
  void* h = nullptr; void* qkv = nullptr; void* q = nullptr; void* attn = nullptr; void* act = nullptr;
  float* logits = nullptr; size_t logits_cap = 0;
  void* gu = nullptr; size_t gu_cap = 0;                  // [rows][2 I]: the stored output of an ADAPTED gate|up (swiglu_rows_kernel reads it)
  // ---- adapters: per-request slot s is resident while adapter_parts[s] > 0 ((layer, projection part) entries that hold
  // factors); adapter_gen[s] counts the changes of the slot (the prefix cache's hash seed: K/V depend on the adapter).
  // engine_lora: mi_engine_set_lora has adapted this engine -- every token row of every step runs column LORA_ENGINE_COL of
  // the tables, whatever kv->row_adapter says; the two forms exclude each other.
  int adapter_parts[MI_MAX_ADAPTERS] = {};
  uint32_t adapter_gen[MI_MAX_ADAPTERS] = {};
  bool engine_lora = false;
  int32_t* d_row_adapter = nullptr; size_t d_row_adapter_cap = 0;   // [token rows] of the current step
  float* lora_rt = nullptr; size_t lora_rt_cap = 0;                 // [token rows][LORA_ROWS_T_LD]: t of the by-row kernels
  void* ys = nullptr; size_t ys_cap = 0;                            // [token rows][H]: stored o_proj / down_proj output ahead of the by-row up-add
  // MI_ARCH_MIXTRAL: sel | score | meta | list | act [R k][I] | y [R k][H] of the current layer, one block (moe_workspace)
  char* moe_ws = nullptr; size_t moe_ws_cap = 0;
  int32_t* d_tokens = nullptr; size_t d_tokens_cap = 0;
  const int32_t* tok_src = nullptr;                       // device-fed step: the embedding reads the sampler's output in place
  int32_t* d_forced = nullptr; size_t d_forced_cap = 0;   // mi_score_tokens targets
  int32_t* d_gather = nullptr;                            // token positions whose hidden state feeds the head (mixed steps)
  float* d_rowpar = nullptr; size_t d_rowpar_cap = 0;     // per-row temperature | top_p of the current step
  char* d_rowext = nullptr; size_t d_rowext_cap = 0;      // per-row seed | position (8 bytes each) | top_k | min_p
  void* deq_scratch = nullptr; size_t deq_cap = 0;        // [hi | lo] 16-bit copy of one int4 matrix (prefill GEMM)
  void* sk_ws = nullptr; size_t sk_ws_cap = 0;            // split-K partial tiles of gemm_skinny.hip
  unsigned* sk_ctr = nullptr; size_t sk_ctr_cap = 0;      // its per-tile-group arrival counters (zero between launches)
  int32_t* d_next = nullptr;      // tokens sampled by the last step [maxB]
  float* d_logprob = nullptr; float* d_prob0 = nullptr; float* d_rowstats = nullptr; float* d_uniforms = nullptr;
  int32_t* d_topk_ids = nullptr; float* d_topk_lp = nullptr;
  int32_t* d_bias_ids = nullptr; float* d_bias_vals = nullptr;
  int maxB = 0;
  mi::Slot slots[mi::NSLOT];
  int64_t next_ticket = 0;
  uint64_t step_counter = 0;
  // profiling
  std::string prof_name;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  int opt_force_v1 = 0;
  int opt_fused_attn = 1;
  int opt_attn_mfma = 1;                 // decode attention on the matrix cores where the shape allows
  int opt_tile_weights = 1;
  int opt_prefill_gemm = 1;
  int opt_skinny_gemm = 1;      // decode steps of 9..128 rows (int4 / int8: 1..128): the split-K weight-streaming GEMM (gemm_skinny.hip)
  int cur_L = 0;                // tokens per sequence of the forward pass being enqueued
  int opt_norm_handover = 1;    // round 2 (partial sums read in ONE round trip): Mistral-7B int4 +3.2 %, int8 +2.9 %, bf16 B = 16 +3.7 %, Qwen3-14B int4 +0.6 %
  int opt_prefill_x_terms = 2;  // float32 activations, prefill tile GEMM on dense bf16 weights: 16-bit terms of x (2 or 3 = exact)
  int opt_defer_norm = 1;       // float32 activations: RMSNorm row scale applied in the split-K kernel's epilogue (no norm launch)
  int opt_short_prefill_skinny = 1;   // short prefill / mixed calls on the weight-streaming kernel instead of the tile GEMM (gemv_rows)
  // the q|k|v linear of a float32-KV decode step publishes its K slices' partial rows and the decode attention's prologue
  // adds them (0: the linear's last arriver combines).  Bit-identical outputs; measurements and history: DESIGN §8e
  int opt_consumer_combine = 1;
  // the wide linears of a float32-KV decode step (gate|up, lm_head) at K <= 4096 on the resident form of gemv_f32.hip (x kept in
  // LDS; 0: the chunked kernel).  Bit-identical outputs; measurements: DESIGN §5, §8d
  int opt_resident_x = 1;
  float* cc_pub = nullptr; size_t cc_pub_cap = 0;      // the q|k|v seam: [guard][8 slices][8 rows][nqkv][guard][8 slices][8 rows][guard]
  float* d_sq = nullptr;        // [4096 tile groups][16 rows]
  mi::NormHandover handover;
  bool opt_gu8 = true;                   // decode GEMV of a dense gate|up matrix on its row-interleaved copy: 7 one-tile items per CU instead of 3.5 pairs (twice the matrix's bytes)
  bool opt_f16_hilo = true;              // f16 dense weights in the float32-activation mode through an exact [hi | lo] bf16 copy (matrix cores)
  int last_n = 0;                        // rows of the last enqueued step (device-resident token feed)
  void* xn = nullptr;            // [rows][max(H, I)] normalised activations of the prefill GEMMs
  void* xs = nullptr; size_t xs_cap = 0;   // [rows][3 K] bf16: float32 activations split three ways (float32-KV prefill)
  void* gk_ws = nullptr; size_t gk_cap = 0;   // float32 partial tiles of the K-split 128 x 128 tile GEMM
};

struct mi_kv {
  mi_engine* e = nullptr;
  int B = 0, cap = 0, dtype = MI_F32;
  bool quirk = false;            // float32 "PagedKVCache" semantics on a 16-bit model
  void* k = nullptr; void* v = nullptr;
  int32_t* d_off = nullptr;
  std::vector<int32_t> h_off;
  int32_t* d_rows = nullptr;     // [B] scratch: cache rows of the current call (continuous batching)
  std::vector<int32_t> row_adapter;      // [B]: adapter slot of the request that occupies the row, -1 = none (mi_kv_set_row_adapter)
  float* partial = nullptr; size_t partial_cap = 0;      // split-KV partials, sized for 16 splits (mi::grow: bytes)
  int* counters = nullptr;       // [B*Hkv] split-arrival tickets of the fused decode attention
  // ---- per-row logit_bias (mi_kv_set_row_logit_bias): one block [B counts | B map | B x MI_MAX_ROW_LOGIT_BIAS ids | as many
  // values], allocated by the first call that sets a bias.  rb_host_cnt mirrors the counts in enqueue order and rb_biased
  // counts the rows with entries: a step enqueued while it is 0 launches the sampler without the table.  Uploads go through
  // RB_STAGE pinned slots [ids | values], each reusable once its event (recorded behind its copies) has passed.
  static constexpr int RB_STAGE = 4;
  int32_t* rb_block = nullptr;
  std::vector<int32_t> rb_host_cnt;
  int rb_biased = 0;
  char* rb_stage = nullptr; hipEvent_t rb_ev[RB_STAGE] = {}; int rb_next = 0;
  int32_t* rb_cnt() const { return rb_block; }
  int32_t* rb_map() const { return rb_block + B; }                 // the sampled row -> cache row map of a mixed step
  int32_t* rb_ids() const { return rb_block + 2 * (size_t)B; }
  float* rb_vals() const { return (float*)(rb_block + 2 * (size_t)B + (size_t)B * MI_MAX_ROW_LOGIT_BIAS); }
  // ---- per-row logprobs settings (mi_kv_set_row_logprobs): one block [B counts (-1: no setting) | B flags | B map], allocated
  // by the first call that sets a row.  lp_host_k mirrors the counts in enqueue order and lp_set counts the rows with a
  // setting: a step enqueued while it is 0 launches the sampler without the settings and returns the [B][top_logprobs] layout.
  int32_t* lp_block = nullptr;
  std::vector<int32_t> lp_host_k;
  int lp_set = 0;
  int32_t* lp_k() const { return lp_block; }
  int32_t* lp_flag() const { return lp_block + B; }
  int32_t* lp_map() const { return lp_block + 2 * (size_t)B; }     // (mixed steps of a cache without a bias table)
  // ---- block-paged form (mi_kv_create_paged): k / v are arenas [layer][block][Hkv][1 << bs_shift][D], blocks.h_btab names
  // every row's blocks and d_btab is its copy on the device; cap = bt_stride << bs_shift is the longest sequence a row can hold
  bool paged = false;
  mi::KvBlocks blocks;
  int32_t* d_btab = nullptr;
};

namespace mi {

struct Prof {
  mi_engine* e; bool on; hipEvent_t a = nullptr, b = nullptr;
  Prof(mi_engine* e_, const char* name) : e(e_), on(!e_->prof_name.empty() && e_->prof_name == name) {
    if (on) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, e->stream); }
  }
  ~Prof() { if (on) { hipEventRecord(b, e->stream); e->prof_events.emplace_back(a, b); } }
};

// engine_load.hip
void free_linear(FusedLinear& f);
inline int adapters_resident(const mi_engine* e) { int n = 0; for (int s : e->adapter_parts) n += s > 0; return n; }
// engine_linear.hip.  gemv_rows: y = W x for `rows` rows on the kernel family its route picks.  consumer_combine: `published` !=
// null is an OFFER of the caller's -- "the next launch can add K slices published in the seam buffer instead of reading
// c.out".  The router takes it on the one route whose kernel has the publish-only form, and *published = the number of K
// slices it left there (0: declined, the ordinary launch wrote c.out).
int gemv_rows(mi_engine* e, const FusedLinear& f0, GemvCall c, size_t rows, size_t es_in, size_t es_out, const char* prof,
              int* published = nullptr);
bool ensure_hilo(mi_engine* e, FusedLinear& f);
bool ensure_gu8(mi_engine* e, FusedLinear& f, int pair_offset);
int check_cc_guards(mi_engine* e, int nqkv);
float* cc_pub_tiles(mi_engine* e);                   // [8 slices][8 rows][nqkv]
float* cc_pub_sumsq(mi_engine* e, int nqkv);         // [8 slices][8 rows]
// engine_kv.hip
int kv_ensure_blocks(mi_kv* kv, int row, int tokens);
int kv_upload_table(mi_kv* kv, hipStream_t st);
void kv_shape(const mi_kv* kv, AttnShape& s);
size_t kv_layer_elems(const mi_kv* kv, const mi_model_desc& d);

}  // namespace mi
