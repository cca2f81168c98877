// engine_kv.hip -- the mi_kv_* entry points: contiguous and block-paged caches, prefix reuse, forked rows, per-row logit_bias.  The paged
// cache's host state (block pool, tables, prefix cache) is mi::KvBlocks (kv_blocks.h); here are the argument checks and
// whatever a call enqueues on the engine's stream.
#include <cmath>
#include <cstring>

#include "engine_impl.h"

using namespace mi;

namespace mi {

// the row's table covers `tokens` positions after this
int kv_ensure_blocks(mi_kv* kv, int row, int tokens) {
  if (!kv->paged) return MI_OK;
  switch (kv->blocks.ensure(row, tokens)) {
    case KvBlocks::Ensure::TOO_LONG: return fail(MI_ERR_INVALID, "paged KV: sequence longer than the row's block table");
    case KvBlocks::Ensure::EXHAUSTED: return fail(MI_ERR_RUNTIME, "paged KV: the block arena is exhausted (every block is held by a live sequence)");
    case KvBlocks::Ensure::OK: break;
  }
  return MI_OK;
}

int kv_upload_table(mi_kv* kv, hipStream_t st) {
  if (kv->paged && kv->blocks.btab_dirty) {
    // (pageable host memory: the copy is staged by the runtime before the call returns, so h_btab may change afterwards)
    const std::vector<int32_t>& tab = kv->blocks.h_btab;
    MI_HIP(hipMemcpyAsync(kv->d_btab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    kv->blocks.btab_dirty = false;
  }
  return MI_OK;
}

void kv_shape(const mi_kv* kv, AttnShape& s) {
  if (kv->paged) { s.btab = kv->d_btab; s.bt_stride = kv->blocks.bt_stride; s.bs_shift = kv->blocks.bs_shift; }
}

size_t kv_layer_elems(const mi_kv* kv, const mi_model_desc& d) {
  return kv->paged ? ((size_t)kv->blocks.nblocks * d.num_kv_heads << kv->blocks.bs_shift) * d.head_dim
                   : (size_t)kv->B * d.num_kv_heads * kv->cap * d.head_dim;
}

}  // namespace mi

namespace {

void kv_release_row(mi_kv* kv, int row) {
  if (kv->paged) kv->blocks.release_row(row);
}

// the element type of the caches for the caller's kv_dtype: the model's, or float32 ("PagedKVCache" semantics)
int set_kv_dtype(mi_kv* kv, int kv_dtype) {
  const int act = kv->e->d.act_dtype;
  if (kv_dtype == MI_KV_MODEL || kv_dtype == act) { kv->dtype = act; kv->quirk = false; }
  else if (kv_dtype == MI_F32) { kv->dtype = MI_F32; kv->quirk = true; }
  else return fail(MI_ERR_UNSUPPORTED, "kv dtype must be the model dtype or float32");
  return MI_OK;
}

// every buffer allocated, zeroed on the stream (like the reference's mx.zeros, base.py:71-72,111-112) and the stream drained --
// or none of them left behind
struct Buf { void** p; size_t bytes; };
int zero_all(hipStream_t st, std::initializer_list<Buf> bufs) {
  for (const Buf& b : bufs) MI_HIP(hipMemsetAsync(*b.p, 0, b.bytes, st));
  MI_HIP(hipStreamSynchronize(st));
  return MI_OK;
}
int alloc_zeroed(hipStream_t st, std::initializer_list<Buf> bufs, const char* oom) {
  int rc = MI_OK;
  for (const Buf& b : bufs)
    if (rc == MI_OK && hipMalloc(b.p, b.bytes) != hipSuccess) rc = fail(MI_ERR_RUNTIME, oom);
  if (rc == MI_OK) rc = zero_all(st, bufs);
  if (rc != MI_OK) for (const Buf& b : bufs) { hipFree(*b.p); *b.p = nullptr; }
  return rc;
}

// the row's logit_bias count -> 0, behind the steps already enqueued (a row without entries: nothing to do)
int rb_clear_row(mi_kv* kv, int row) {
  if (kv->rb_biased > 0 && kv->rb_host_cnt[row] > 0) {
    MI_HIP(hipMemsetAsync(kv->rb_cnt() + row, 0, sizeof(int32_t), kv->e->stream));
    kv->rb_host_cnt[row] = 0;
    --kv->rb_biased;
  }
  return MI_OK;
}

// the row's logprobs setting -> none, behind the steps already enqueued
int lp_clear_row(mi_kv* kv, int row) {
  if (kv->lp_set > 0 && kv->lp_host_k[row] >= 0) {
    MI_HIP(hipMemsetD32Async((hipDeviceptr_t)(kv->lp_k() + row), -1, 1, kv->e->stream));
    kv->lp_host_k[row] = -1;
    --kv->lp_set;
  }
  return MI_OK;
}

// where the row's prefix hash chains start: K / V depend on the adapter (0 for a row without one: the keys of always)
uint64_t prefix_seed(const mi_kv* kv, int row) {
  const int a = kv->row_adapter[row];
  return a < 0 ? 0 : KvBlocks::adapter_seed(a, kv->e->adapter_gen[a]);
}

}  // namespace

extern "C" {

int mi_kv_create(mi_engine* e, int batch, int capacity_tokens, int kv_dtype, mi_kv** out) {
  if (!e || !out) return fail(MI_ERR_INVALID, "null argument");
  if (batch < 1 || capacity_tokens < 1) return fail(MI_ERR_INVALID, "batch and capacity must be positive");
  if (capacity_tokens > e->d.max_positions) return fail(MI_ERR_INVALID, "capacity exceeds desc.max_positions");
  MI_HIP(hipSetDevice(e->device));
  mi_kv* kv = new mi_kv();
  kv->e = e; kv->B = batch; kv->cap = capacity_tokens;
  int rc = set_kv_dtype(kv, kv_dtype);
  const size_t bytes = (size_t)e->d.num_layers * batch * e->d.num_kv_heads * capacity_tokens * e->d.head_dim * dtype_size(kv->dtype);
  if (rc == MI_OK)
    rc = alloc_zeroed(e->stream, {{(void**)&kv->counters, (size_t)batch * e->d.num_kv_heads * sizeof(int)}, {&kv->k, bytes}, {&kv->v, bytes},
                                  {(void**)&kv->d_off, batch * sizeof(int32_t)}}, "out of device memory allocating the KV cache");
  if (rc != MI_OK) { delete kv; return rc; }
  kv->h_off.assign(batch, 0);
  kv->row_adapter.assign(batch, -1);
  *out = kv;
  return MI_OK;
}

int mi_kv_create_paged(mi_engine* e, int slots, int block_tokens, int n_blocks, int max_tokens_per_row, int kv_dtype, mi_kv** out) {
  if (!e || !out) return fail(MI_ERR_INVALID, "null argument");
  if (slots < 1 || n_blocks < 2 || max_tokens_per_row < 1) return fail(MI_ERR_INVALID, "slots, blocks and tokens per row must be positive (block 0 is reserved)");
  if (block_tokens < 16 || (block_tokens & (block_tokens - 1)) != 0) return fail(MI_ERR_INVALID, "block_tokens must be a power of two >= 16");
  if (max_tokens_per_row > e->d.max_positions) return fail(MI_ERR_INVALID, "max_tokens_per_row exceeds desc.max_positions");
  MI_HIP(hipSetDevice(e->device));
  mi_kv* kv = new mi_kv();
  kv->e = e; kv->B = slots; kv->paged = true;
  kv->blocks.init(slots, block_tokens, n_blocks, max_tokens_per_row);
  kv->cap = std::min(kv->blocks.bt_stride * block_tokens, e->d.max_positions);
  int rc = set_kv_dtype(kv, kv_dtype);
  const size_t bytes = (size_t)e->d.num_layers * n_blocks * e->d.num_kv_heads * block_tokens * e->d.head_dim * dtype_size(kv->dtype);
  if (rc == MI_OK)
    rc = alloc_zeroed(e->stream, {{(void**)&kv->counters, (size_t)slots * e->d.num_kv_heads * sizeof(int)}, {&kv->k, bytes}, {&kv->v, bytes},
                                  {(void**)&kv->d_off, slots * sizeof(int32_t)}, {(void**)&kv->d_btab, kv->blocks.h_btab.size() * sizeof(int32_t)}},
                      "out of device memory allocating the paged KV arena");
  if (rc != MI_OK) { delete kv; return rc; }
  kv->h_off.assign(slots, 0);
  kv->row_adapter.assign(slots, -1);
  *out = kv;
  return MI_OK;
}

int mi_kv_prefix_attach(mi_kv* kv, int row, const int32_t* tokens, int n, int* n_reused) {
  if (!kv || !tokens || !n_reused) return fail(MI_ERR_INVALID, "null argument");
  if (!kv->paged) return fail(MI_ERR_INVALID, "prefix reuse needs a paged KV (mi_kv_create_paged)");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "row out of range");
  if (kv->h_off[row] != 0 || kv->blocks.row_blocks[row] != 0) return fail(MI_ERR_INVALID, "prefix attach: the row must be empty (mi_kv_reset_row first)");
  const int reused = kv->blocks.attach(row, tokens, n, prefix_seed(kv, row));
  if (reused > 0) {
    kv->h_off[row] = reused;
    MI_HIP(hipSetDevice(kv->e->device));
    MI_HIP(hipMemsetD32Async((hipDeviceptr_t)(kv->d_off + row), reused, 1, kv->e->stream));
  }
  *n_reused = reused;
  return MI_OK;
}

int mi_kv_prefix_publish(mi_kv* kv, int row, const int32_t* tokens, int n) {
  if (!kv || !tokens) return fail(MI_ERR_INVALID, "null argument");
  if (!kv->paged) return fail(MI_ERR_INVALID, "prefix reuse needs a paged KV (mi_kv_create_paged)");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "row out of range");
  if (n > kv->h_off[row]) return fail(MI_ERR_INVALID, "prefix publish: those tokens are not in the row's cache yet");
  kv->blocks.publish(row, tokens, n, prefix_seed(kv, row));
  return MI_OK;
}

int mi_kv_prefix_clear(mi_kv* kv) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  kv->blocks.clear_prefix();
  return MI_OK;
}

int mi_kv_stats(const mi_kv* kv, int64_t* out, int n) {
  if (!kv || !out) return fail(MI_ERR_INVALID, "null argument");
  kv->blocks.stats(out, n);
  return MI_OK;
}

void mi_kv_destroy(mi_kv* kv) {
  if (!kv) return;
  hipSetDevice(kv->e->device);
  hipStreamSynchronize(kv->e->stream);
  hipFree(kv->k); hipFree(kv->v); hipFree(kv->d_off); hipFree(kv->partial); hipFree(kv->counters); hipFree(kv->d_rows);
  hipFree(kv->d_btab);
  hipFree(kv->rb_block); hipFree(kv->lp_block);
  if (kv->rb_stage) hipHostFree(kv->rb_stage);
  for (hipEvent_t ev : kv->rb_ev) if (ev) hipEventDestroy(ev);
  delete kv;
}

int mi_kv_reset(mi_kv* kv, int batch) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (batch != kv->B) return fail(MI_ERR_INVALID, "mi_kv_reset: batch differs from the allocated batch (create a new kv)");
  MI_HIP(hipSetDevice(kv->e->device));
  MI_HIP(hipMemsetAsync(kv->d_off, 0, kv->B * sizeof(int32_t), kv->e->stream));
  for (int r = 0; r < kv->B; ++r) MI_TRY(rb_clear_row(kv, r));     // every row's logit_bias goes with its contents
  for (int r = 0; r < kv->B; ++r) MI_TRY(lp_clear_row(kv, r));     // and its logprobs setting
  MI_HIP(hipStreamSynchronize(kv->e->stream));
  std::fill(kv->h_off.begin(), kv->h_off.end(), 0);
  std::fill(kv->row_adapter.begin(), kv->row_adapter.end(), -1);
  for (int r = 0; r < kv->B; ++r) kv_release_row(kv, r);
  return MI_OK;
}

int mi_kv_reset_row(mi_kv* kv, int row) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_reset_row: row out of range");
  MI_HIP(hipSetDevice(kv->e->device));
  MI_HIP(hipMemsetAsync(kv->d_off + row, 0, sizeof(int32_t), kv->e->stream));   // ordered behind the steps already enqueued
  kv->h_off[row] = 0;
  kv->row_adapter[row] = -1;                                // the next occupant of the row names its own adapter
  kv_release_row(kv, row);      // (paged: the blocks go back to the pool; whoever gets them next writes behind the steps in flight)
  MI_TRY(rb_clear_row(kv, row));                            // the next occupant of the row samples unbiased
  return lp_clear_row(kv, row);                             // and reports what its own request asks for
}

int mi_kv_fork_row(mi_kv* kv, int src, int dst, int n_tokens) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (src < 0 || src >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_fork_row: src out of range");
  if (dst < 0 || dst >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_fork_row: dst out of range");
  if (src == dst) return fail(MI_ERR_INVALID, "mi_kv_fork_row: src and dst are the same row");
  if (kv->h_off[dst] != 0 || (kv->paged && kv->blocks.row_blocks[dst] != 0))
    return fail(MI_ERR_INVALID, "mi_kv_fork_row: dst must be empty (mi_kv_reset_row first)");
  if (n_tokens < 1 || n_tokens > kv->h_off[src])
    return fail(MI_ERR_INVALID, "mi_kv_fork_row: n_tokens must be in [1, " + std::to_string(kv->h_off[src]) + "], the length of src");
  if (kv->row_adapter[dst] != kv->row_adapter[src])
    return fail(MI_ERR_INVALID, "mi_kv_fork_row: dst names adapter " + std::to_string(kv->row_adapter[dst]) + ", src adapter " +
                                    std::to_string(kv->row_adapter[src]) + " (mi_kv_set_row_adapter on dst first: K / V depend on the adapter)");
  MI_HIP(hipSetDevice(kv->e->device));
  const mi_model_desc& d = kv->e->d;
  hipStream_t st = kv->e->stream;
  // on the engine's stream: behind every step already enqueued (the appends of src are in), ahead of every later one
  int rc = MI_OK;
  if (kv->paged) {
    int src_blk = 0, dst_blk = 0;
    switch (kv->blocks.fork(src, dst, n_tokens, &src_blk, &dst_blk)) {
      case KvBlocks::Ensure::TOO_LONG: return fail(MI_ERR_INVALID, "mi_kv_fork_row: n_tokens is longer than the row's block table");
      case KvBlocks::Ensure::EXHAUSTED: return fail(MI_ERR_RUNTIME, "mi_kv_fork_row: the block arena has no block for the tail (every block is held by a live sequence)");
      case KvBlocks::Ensure::OK: break;
    }
    const int bs = 1 << kv->blocks.bs_shift, tail = n_tokens & (bs - 1);
    if (tail > 0) {       // the full blocks are shared; the tail starts at the same token of both blocks
      const size_t head = (size_t)bs * d.head_dim, blk = (size_t)d.num_kv_heads * head;
      rc = launch_kv_copy_tokens(kv->k, kv->v, kv->dtype, d.num_layers, kv_layer_elems(kv, d), d.num_kv_heads, d.head_dim, head,
                                 (size_t)src_blk * blk, (size_t)dst_blk * blk, tail, st);
    }
  } else {
    const size_t head = (size_t)kv->cap * d.head_dim, row = (size_t)d.num_kv_heads * head;
    rc = launch_kv_copy_tokens(kv->k, kv->v, kv->dtype, d.num_layers, kv_layer_elems(kv, d), d.num_kv_heads, d.head_dim, head,
                               (size_t)src * row, (size_t)dst * row, n_tokens, st);
  }
  if (rc == MI_OK && hipMemsetD32Async((hipDeviceptr_t)(kv->d_off + dst), n_tokens, 1, st) != hipSuccess)
    rc = fail(MI_ERR_RUNTIME, "mi_kv_fork_row: hipMemsetD32Async failed");
  if (rc != MI_OK) { kv_release_row(kv, dst); return rc; }     // dst stays empty
  kv->h_off[dst] = n_tokens;
  return MI_OK;
}

int mi_kv_set_row_adapter(mi_kv* kv, int row, int adapter) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_set_row_adapter: row out of range");
  if (adapter < -1 || adapter >= MI_MAX_ADAPTERS)
    return fail(MI_ERR_INVALID, "mi_kv_set_row_adapter: adapter " + std::to_string(adapter) + " is outside [-1, " + std::to_string(MI_MAX_ADAPTERS) + ")");
  if (kv->h_off[row] != 0 || (kv->paged && kv->blocks.row_blocks[row] != 0))
    return fail(MI_ERR_INVALID, "mi_kv_set_row_adapter: the row must be empty (mi_kv_reset_row first): its K / V depend on the adapter");
  kv->row_adapter[row] = adapter;
  return MI_OK;
}

int mi_kv_set_row_logprobs(mi_kv* kv, int row, int top_logprobs, int at_temperature) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_set_row_logprobs: row out of range");
  if (top_logprobs < 0 || top_logprobs > MI_MAX_TOP_LOGPROBS)
    return fail(MI_ERR_INVALID, "mi_kv_set_row_logprobs: top_logprobs must be in [0, " + std::to_string(MI_MAX_TOP_LOGPROBS) + "]");
  if (at_temperature != 0 && at_temperature != 1) return fail(MI_ERR_INVALID, "mi_kv_set_row_logprobs: at_temperature must be 0 or 1");
  MI_HIP(hipSetDevice(kv->e->device));
  hipStream_t st = kv->e->stream;
  if (top_logprobs == 0 && at_temperature == 0) return lp_clear_row(kv, row);   // (a cache that never had a setting: nothing to clear)
  if (!kv->lp_block) {                                      // first use: the table, every row without a setting
    int32_t* blk = nullptr;
    if (hipMalloc(&blk, 3 * (size_t)kv->B * sizeof(int32_t)) != hipSuccess) return fail(MI_ERR_RUNTIME, "out of device memory allocating the logprobs settings");
    if (hipMemsetAsync(blk, 0xff, 3 * (size_t)kv->B * sizeof(int32_t), st) != hipSuccess) {
      hipFree(blk);
      return fail(MI_ERR_RUNTIME, "hipMemsetAsync failed (logprobs settings)");
    }
    kv->lp_block = blk;
    kv->lp_host_k.assign(kv->B, -1);
  }
  // the flag, then the count that makes it a setting: behind every step already enqueued, ahead of every later one
  MI_HIP(hipMemsetD32Async((hipDeviceptr_t)(kv->lp_flag() + row), at_temperature, 1, st));
  MI_HIP(hipMemsetD32Async((hipDeviceptr_t)(kv->lp_k() + row), top_logprobs, 1, st));
  if (kv->lp_host_k[row] < 0) ++kv->lp_set;
  kv->lp_host_k[row] = top_logprobs;
  return MI_OK;
}

int mi_kv_set_row_logit_bias(mi_kv* kv, int row, const int32_t* ids, const float* values, int n) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (row < 0 || row >= kv->B) return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: row out of range");
  if (n < 0 || n > MI_MAX_ROW_LOGIT_BIAS)
    return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: n must be in [0, " + std::to_string(MI_MAX_ROW_LOGIT_BIAS) + "]");
  if (n > 0 && (!ids || !values)) return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: null ids / values");
  const int V = kv->e->d.vocab_size;
  if (n > 0) {
    std::vector<int32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < n; ++i) {
      if (ids[i] < 0 || ids[i] >= V)
        return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) +
                                        " is outside the vocabulary [0, " + std::to_string(V) + ")");
      if (!std::isfinite(values[i]))
        return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: values[" + std::to_string(i) + "] is not finite");
      if (i > 0 && sorted[i] == sorted[i - 1])
        return fail(MI_ERR_INVALID, "mi_kv_set_row_logit_bias: ids names token " + std::to_string(sorted[i]) + " twice");
    }
  }
  MI_HIP(hipSetDevice(kv->e->device));
  hipStream_t st = kv->e->stream;
  if (n == 0) return rb_clear_row(kv, row);                 // clear; a cache that never had a bias has nothing to clear
  const size_t cap = MI_MAX_ROW_LOGIT_BIAS;
  if (!kv->rb_block) {                                      // first use: the table, its staging and their events
    const size_t words = 2 * (size_t)kv->B + 2 * (size_t)kv->B * cap;
    int32_t* blk = nullptr; char* stage = nullptr;
    if (hipMalloc(&blk, words * sizeof(int32_t)) != hipSuccess) return fail(MI_ERR_RUNTIME, "out of device memory allocating the logit_bias table");
    if (hipHostMalloc(&stage, (size_t)mi_kv::RB_STAGE * cap * 8) != hipSuccess) {
      hipFree(blk);
      return fail(MI_ERR_RUNTIME, "out of pinned host memory allocating the logit_bias staging");
    }
    for (hipEvent_t& ev : kv->rb_ev)
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        for (hipEvent_t& x : kv->rb_ev) { if (x) hipEventDestroy(x); x = nullptr; }
        hipFree(blk); hipHostFree(stage);
        return fail(MI_ERR_RUNTIME, "hipEventCreate failed (logit_bias staging)");
      }
    if (hipMemsetAsync(blk, 0, 2 * (size_t)kv->B * sizeof(int32_t), st) != hipSuccess) {
      for (hipEvent_t& x : kv->rb_ev) { hipEventDestroy(x); x = nullptr; }
      hipFree(blk); hipHostFree(stage);
      return fail(MI_ERR_RUNTIME, "hipMemsetAsync failed (logit_bias table)");
    }
    kv->rb_block = blk; kv->rb_stage = stage;
    kv->rb_host_cnt.assign(kv->B, 0);
  }
  // the caller's arrays -> a pinned slot of ours (they are the caller's again when this returns) -> the row's entries and
  // then its count, on the engine's stream: behind every step already enqueued, ahead of every later one
  const int slot = kv->rb_next;
  MI_HIP(hipEventSynchronize(kv->rb_ev[slot]));             // (a never-recorded event is complete)
  char* stage = kv->rb_stage + (size_t)slot * cap * 8;
  memcpy(stage, ids, (size_t)n * sizeof(int32_t));
  memcpy(stage + cap * 4, values, (size_t)n * sizeof(float));
  MI_HIP(hipMemcpyAsync(kv->rb_ids() + (size_t)row * cap, stage, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  MI_HIP(hipMemcpyAsync(kv->rb_vals() + (size_t)row * cap, stage + cap * 4, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  MI_HIP(hipMemsetD32Async((hipDeviceptr_t)(kv->rb_cnt() + row), n, 1, st));
  MI_HIP(hipEventRecord(kv->rb_ev[slot], st));
  kv->rb_next = (slot + 1) % mi_kv::RB_STAGE;
  if (kv->rb_host_cnt[row] == 0) ++kv->rb_biased;
  kv->rb_host_cnt[row] = n;
  return MI_OK;
}

int mi_kv_reserve(mi_kv* kv, int capacity_tokens) {
  if (!kv) return fail(MI_ERR_INVALID, "null kv");
  if (capacity_tokens <= kv->cap) return MI_OK;
  mi_engine* e = kv->e;
  if (kv->paged) return fail(MI_ERR_INVALID, "paged KV: a row holds at most block_tokens x table length tokens (create a larger table)");
  if (capacity_tokens > e->d.max_positions) return fail(MI_ERR_INVALID, "capacity exceeds desc.max_positions");
  MI_HIP(hipSetDevice(e->device));
  const size_t es = dtype_size(kv->dtype);
  const size_t slabs = (size_t)e->d.num_layers * kv->B * e->d.num_kv_heads;
  const size_t old_pitch = (size_t)kv->cap * e->d.head_dim * es, new_pitch = (size_t)capacity_tokens * e->d.head_dim * es;
  void* nk = nullptr; void* nv = nullptr;
  if (hipMalloc(&nk, slabs * new_pitch) != hipSuccess || hipMalloc(&nv, slabs * new_pitch) != hipSuccess) {
    hipFree(nk); hipFree(nv);
    return fail(MI_ERR_RUNTIME, "out of device memory growing the KV cache");
  }
  MI_HIP(hipMemsetAsync(nk, 0, slabs * new_pitch, e->stream));
  MI_HIP(hipMemsetAsync(nv, 0, slabs * new_pitch, e->stream));
  MI_HIP(hipMemcpy2DAsync(nk, new_pitch, kv->k, old_pitch, old_pitch, slabs, hipMemcpyDeviceToDevice, e->stream));
  MI_HIP(hipMemcpy2DAsync(nv, new_pitch, kv->v, old_pitch, old_pitch, slabs, hipMemcpyDeviceToDevice, e->stream));
  MI_HIP(hipStreamSynchronize(e->stream));
  hipFree(kv->k); hipFree(kv->v);
  kv->k = nk; kv->v = nv; kv->cap = capacity_tokens;
  return MI_OK;
}

int mi_kv_offsets(const mi_kv* kv, int32_t* out) {
  if (!kv || !out) return fail(MI_ERR_INVALID, "null argument");
  for (int b = 0; b < kv->B; ++b) out[b] = kv->h_off[b];
  return MI_OK;
}

int mi_kv_capacity(const mi_kv* kv) { return kv ? kv->cap : 0; }

}  // extern "C"
