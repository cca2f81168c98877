// ops_api.hip -- kernel-level C entry points (include/mi355_ops.h) on caller-owned device buffers.
#include <algorithm>
#include <vector>

#include "../../include/mi355_ops.h"
#include "kernels.h"
#include "lora_rows.h"

namespace mi {
int launch_gemv(const LinearW& W, const GemvCall& c, hipStream_t st);
bool gemv_mfma_supported(const LinearW& W, const GemvCall& c);
int launch_gemv_mfma(const LinearW& W, const GemvCall& c, hipStream_t st);
}  // namespace mi

using namespace mi;

namespace {

int ready() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MI_ERR_RUNTIME, "no HIP device available (this library has no CPU backend)");
  return MI_OK;
}

int finish() {
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(nullptr));
  return MI_OK;
}

// One launch; with iters >= 1 and avg_ms, `iters` more behind that warm one, timed by events into *avg_ms.  Returns the
// first failing launch's code, else finish()'s.
template <class Launch>
int run_timed(Launch launch, int iters, float* avg_ms) {
  int rc = launch();
  if (rc == MI_OK && iters >= 1 && avg_ms) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && rc == MI_OK; ++i) rc = launch();
    hipEventRecord(e1, nullptr);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *avg_ms = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  const int rc2 = finish();
  return rc != MI_OK ? rc : rc2;
}

// The benchmark entry points' form: a warm launch, then `iters` timed ones; any failing call returns at once, its code unchanged.
template <class Launch>
int run_timed_strict(Launch launch, int iters, float* avg_ms) {
  hipEvent_t e0, e1;
  MI_HIP(hipEventCreate(&e0)); MI_HIP(hipEventCreate(&e1));
  MI_TRY(launch());
  MI_HIP(hipEventRecord(e0, nullptr));
  for (int i = 0; i < iters; ++i) MI_TRY(launch());
  MI_HIP(hipEventRecord(e1, nullptr));
  MI_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MI_HIP(hipEventElapsedTime(&ms, e0, e1));
  if (avg_ms) *avg_ms = ms / iters;
  hipEventDestroy(e0); hipEventDestroy(e1);
  return finish();
}

struct FreeGuard { void*& p; ~FreeGuard() { if (p) hipFree(p); } };

// MI_EPI_SWIGLU on a gate|up matrix of 2 x pair_offset rows: its row-interleaved copy is made here, as mi_engine_finalize
// does, into gu8 (the caller frees it), and W and c are turned to it.  `taken`: the kernel takes the call on that copy.
int gate_up_interleaved(LinearW& W, GemvCall& c, void*& gu8, bool taken, const char* refusal) {
  if (c.epi != EPI_SWIGLU) return MI_OK;
  if (!taken) return fail(MI_ERR_UNSUPPORTED, refusal);
  MI_HIP(hipMalloc(&gu8, (size_t)W.N * W.K * sizeof(uint16_t)));
  MI_TRY(launch_gate_up_interleave(W, c.pair_offset, gu8, nullptr));
  W.w = gu8; c.epi = EPI_SWIGLU_GU8;
  return MI_OK;
}

LinearW to_linear(const mi_op_linear* w) {
  LinearW W;
  W.wk = w->wk; W.w = w->w; W.scales = w->scales; W.biases = w->biases; W.N = w->N; W.K = w->K;
  W.group = w->group > 0 ? w->group : 64;
  W.layout = w->layout;
  W.bias = w->bias;
  return W;
}

GemvCall to_call(const mi_op_gemv_args* a) {
  GemvCall c;
  c.x = a->x; c.ldx = a->ldx; c.M = a->M; c.act = a->act; c.rnd = a->rnd; c.pro = a->pro; c.norm_w = a->norm_w;
  c.eps = a->eps; c.epi = a->epi; c.out = a->out; c.ldo = a->ldo; c.resid = a->resid; c.pair_offset = a->pair_offset;
  c.force_v1 = a->force_generic;
  return c;
}

AttnShape to_shape(const mi_op_attn_shape* s) {
  return AttnShape{s->B, s->L, s->Hq, s->Hkv, s->D, s->act, s->kv, s->rnd, s->cap};
}

}  // namespace

extern "C" {

int mi_op_gemv(const mi_op_linear* w, const mi_op_gemv_args* a) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  const LinearW W = to_linear(w);
  const GemvCall c = to_call(a);
  const int maxm = gemv_mfma_supported(W, c) ? 16 : 8;
  if (c.M < 1 || c.M > maxm) return fail(MI_ERR_INVALID, "mi_op_gemv: M out of range for this kernel");
  MI_TRY(launch_gemv(W, c, nullptr));
  return finish();
}

int mi_op_gemv_bench(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms) {
  if (!w || !a || !avg_ms || iters < 1) return fail(MI_ERR_INVALID, "bad argument");
  MI_TRY(ready());
  const LinearW W = to_linear(w);
  const GemvCall c = to_call(a);
  return run_timed_strict([&] { return launch_gemv(W, c, nullptr); }, iters, avg_ms);
}

// gemv_mfma.hip's launch on the row-interleaved gate|up copy (gemv_mfma_gu8_kernel) on its own: a->epi = MI_EPI_SWIGLU, w a
// tile-major dense 16-bit gate|up matrix of 2 x a->pair_offset rows.  The copy is made here, as mi_engine_finalize does; what
// the engine's gu8_wanted + gemv_mfma_supported would not take is refused, nothing launched.
int mi_op_gemv_gu8(const mi_op_linear* w, const mi_op_gemv_args* a) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  LinearW W = to_linear(w);
  GemvCall c = to_call(a);
  const char* refusal = "mi_op_gemv_gu8: call not supported by this kernel";
  GemvCall probe = c; probe.epi = EPI_SWIGLU_GU8;
  const bool taken = c.epi == EPI_SWIGLU && W.bias == nullptr && W.layout == 1 && (W.wk == WK_BF16 || W.wk == WK_F16) &&
                     c.pair_offset > 0 && c.pair_offset % 16 == 0 && W.N == 2 * c.pair_offset && gemv_mfma_supported(W, probe);
  if (!taken) return fail(MI_ERR_UNSUPPORTED, refusal);
  void* gu8 = nullptr;
  FreeGuard guard{gu8};
  MI_TRY(gate_up_interleaved(W, c, gu8, taken, refusal));
  MI_TRY(launch_gemv_mfma(W, c, nullptr));
  return finish();
}

// gemv_f32.hip on its own: float32 activations (a->rnd = MI_RND_NONE), a->M in 1..8, dense bf16 tile-major weights; plain,
// float32 and residual stores; a->pro may be MI_PRO_NORM (float32 norm weights).  MI_EPI_SWIGLU: w is a gate|up matrix of
// 2 x a->pair_offset rows -- its row-interleaved copy is made here, as mi_engine_finalize does, and the launch runs on it.
// iters >= 1 additionally times `iters` back-to-back launches.
int mi_op_gemv_f32(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  LinearW W = to_linear(w);
  GemvCall c = to_call(a);
  void* gu8 = nullptr;
  FreeGuard guard{gu8};
  MI_TRY(gate_up_interleaved(W, c, gu8, W.wk == WK_BF16 && W.layout == 1, "mi_op_gemv_f32: call not supported by this kernel"));
  if (!gemv_f32_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "mi_op_gemv_f32: call not supported by this kernel");
  return run_timed([&] { return launch_gemv_f32(W, c, nullptr); }, iters, avg_ms);
}

// the whole-K form of gemv_f32.hip on its own (one tile per workgroup: N / 16 <= CUs, K <= 4096, a->pro = MI_PRO_NONE; plain,
// float32 and residual stores), with the refusals of its launch.  iters >= 1 additionally times `iters` back-to-back launches.
int mi_op_gemv_f32_whole(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  const LinearW W = to_linear(w);
  const GemvCall c = to_call(a);
  if (!gemv_f32_whole_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "mi_op_gemv_f32_whole: call not supported by this kernel");
  return run_timed([&] { return launch_gemv_f32_whole(W, c, nullptr); }, iters, avg_ms);
}

// the resident form of gemv_f32.hip on its own (x and the norm weights kept in LDS: K <= 4096): mi_op_gemv_f32's calls,
// epilogues and prologue, with the refusals of its launch.  iters >= 1 additionally times `iters` back-to-back launches.
int mi_op_gemv_f32_resident(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  LinearW W = to_linear(w);
  GemvCall c = to_call(a);
  void* gu8 = nullptr;
  FreeGuard guard{gu8};
  GemvCall probe = c; probe.epi = EPI_SWIGLU_GU8;
  MI_TRY(gate_up_interleaved(W, c, gu8, gemv_f32_resident_supported(W, probe), "mi_op_gemv_f32_resident: call not supported by this kernel"));
  if (!gemv_f32_resident_supported(W, c)) return fail(MI_ERR_UNSUPPORTED, "mi_op_gemv_f32_resident: call not supported by this kernel");
  return run_timed([&] { return launch_gemv_f32_resident(W, c, nullptr); }, iters, avg_ms);
}

// gemm_skinny.hip on its own: a->M in 9..128 (int4 / int8: 1..128), a->pro must be MI_PRO_NONE; ksplit 0 = the cost model's choice
// (*ksplit_used returns it); iters >= 1 additionally times `iters` back-to-back launches.  int4 weights above 16 rows with
// ksplit <= 0 run gemm_q4.hip (a->pro may then be MI_PRO_NORM); ksplit < 0 forces its plan: -(mt | TW << 3 | KW << 7 | ksplit << 11 | NS << 15).
int mi_op_gemm_skinny(const mi_op_linear* w, const mi_op_gemv_args* a, int ksplit, int* ksplit_used, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  const LinearW W = to_linear(w);
  const GemvCall c = to_call(a);
  struct ForceGuard { bool on; ~ForceGuard() { if (on) gemm_q4_force(0); } } guard{ksplit < 0};
  if (ksplit < 0) {
    gemm_q4_force(-ksplit);
    if (!gemm_q4_supported(W, c, (size_t)c.M)) return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_skinny: ksplit < 0 forces gemm_q4, which does not take this call");
  }
  if (!gemm_skinny_supported(W, c, (size_t)c.M) && !gemm_q4_supported(W, c, (size_t)c.M))
    return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_skinny: call not supported by this kernel");
  const int groups = std::max(1, gemm_skinny_groups(W, c, (size_t)c.M));
  void* ws = nullptr; unsigned* ctr = nullptr;
  // 16 slices x N x 128 rows x 4 B: any ksplit of gemm_skinny; gemm_q4: its preparation buffers + partial tiles
  MI_HIP(hipMalloc(&ws, std::max((size_t)W.N * 8192 + 1024, gemm_skinny_ws_bytes(W, c, (size_t)c.M))));
  MI_HIP(hipMalloc(&ctr, (size_t)groups * sizeof(unsigned)));
  MI_HIP(hipMemset(ctr, 0, (size_t)groups * sizeof(unsigned)));
  if (ksplit_used) *ksplit_used = ksplit > 0 ? ksplit : gemm_skinny_ksplit(W, c, (size_t)c.M);
  if (ksplit < 0) ksplit = 0;
  const int rc = run_timed([&] { return launch_gemm_skinny(W, c, (size_t)c.M, nullptr, ws, ctr, ksplit); }, iters, avg_ms);
  hipFree(ws); hipFree(ctr);
  return rc;
}

// gemm_prefill.hip on its own, 16-bit activations: dense 16-bit weights, or int4 / int8 (group 64) weights through the [hi | lo]
// 16-bit copy that the launch makes in a scratch buffer allocated here (the engine's deq_scratch).
int mi_op_gemm_prefill(const mi_op_linear* w, const mi_op_gemv_args* a, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  const LinearW W = to_linear(w);
  const GemvCall c = to_call(a);
  if (c.act == MI_F32)
    return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_prefill: 16-bit activations only (float32 activations: mi_op_gemm_prefill_f32)");
  if (c.M < 1 || c.pro != PRO_NONE || W.layout != 1 || (wk_is_quant(W.wk) && !gemm_prefill_supported(W, c, (size_t)c.M)))
    return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_prefill: tile-major dense 16-bit, int4 or int8 (group 64) weights, 16-bit activations, no prologue");
  void* ws = nullptr; void* scratch = nullptr; size_t cap = 0;
  FreeGuard g_ws{ws}, g_scratch{scratch};
  if (wk_is_quant(W.wk)) MI_HIP(hipMalloc(&scratch, dequant_hilo_bytes(W.N, W.K)));
  // K-split workspace as the engine holds it (float32 partial tiles; prompts below 4096 rows)
  if (c.M < 4096) { cap = (size_t)128 << 20; MI_HIP(hipMalloc(&ws, cap)); }
  return run_timed([&] { return launch_gemm_prefill(W, c, (size_t)c.M, nullptr, scratch, ws, cap); }, iters, avg_ms);
}

// gemm_prefill.hip on float32 activations, as gemv_rows_on (engine.hip) runs it: (norm +) launch_split3_rows into a buffer of
// split3_bytes, then launch_gemm_prefill on that image with c.ldx = x_terms x K.  An f16 matrix is multiplied through its
// [hi | lo] bf16 copy (launch_f16_to_hilo), presented as gemv_rows does: wk = WK_BF16, K = 2 K, c.kx = K.  Every buffer
// is made here; the timed launches are the GEMM's alone.
int mi_op_gemm_prefill_f32(const mi_op_linear* w, const mi_op_gemv_args* a, int x_terms, int iters, float* avg_ms) {
  if (!w || !a) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  LinearW W = to_linear(w);
  GemvCall c = to_call(a);
  const int KT = W.K;                                         // the true K: everything that is about x keeps it
  if (c.M < 1 || c.act != MI_F32 || (x_terms != 2 && x_terms != 3) || (x_terms == 2 && W.wk != WK_BF16))
    return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_prefill_f32: float32 activations in two (dense bf16 weights) or three terms");
  void* hilo = nullptr; void* xs = nullptr; void* scratch = nullptr; void* ws = nullptr; size_t cap = 0;
  FreeGuard g_hilo{hilo}, g_xs{xs}, g_scratch{scratch}, g_ws{ws};
  if (W.wk == WK_F16 && W.layout == 1) {
    MI_HIP(hipMalloc(&hilo, 2 * (size_t)W.N * W.K * sizeof(uint16_t)));
    MI_TRY(launch_f16_to_hilo(W, hilo, nullptr));
    W.wk = WK_BF16; W.w = hilo; W.K = 2 * KT;
    c.kx = KT;
  }
  if (!gemm_prefill_supported(W, c, (size_t)c.M))
    return fail(MI_ERR_UNSUPPORTED, "mi_op_gemm_prefill_f32: call not supported by the tile GEMM");
  MI_HIP(hipMalloc(&xs, split3_bytes((size_t)c.M, KT)));
  MI_TRY(launch_split3_rows(c.x, c.ldx, c.pro == PRO_NORM ? c.norm_w : nullptr, c.eps, xs, c.M, KT, nullptr, x_terms));
  c.x = xs; c.ldx = x_terms * KT; c.pro = PRO_NONE;
  if (wk_is_quant(W.wk)) MI_HIP(hipMalloc(&scratch, dequant_hilo_bytes(W.N, KT)));
  if (c.M < 4096) { cap = (size_t)128 << 20; MI_HIP(hipMalloc(&ws, cap)); }
  return run_timed([&] { return launch_gemm_prefill(W, c, (size_t)c.M, nullptr, scratch, ws, cap); }, iters, avg_ms);
}

// launch_split3_rows on its own: rows x K float32 (row stride ldx; RMS-normalised first when norm_w is not null) ->
// out[rows][terms x K] bf16, [hi | mid | lo] or [hi | mid]
int mi_op_split_rows(const float* x, int ldx, const float* norm_w, float eps, int rows, int K, int terms, void* out) {
  if (!x || !out || rows < 1 || K < 1) return fail(MI_ERR_INVALID, "bad argument");
  MI_TRY(ready());
  MI_TRY(launch_split3_rows(x, ldx, norm_w, eps, out, rows, K, nullptr, terms));
  return finish();
}

// swiglu_rows_kernel (lora_rows.hip) on its own; the launch validates its arguments
int mi_op_swiglu_rows(const void* x, int ldx, void* out, int ldo, int M, int I, int act, int rnd) {
  MI_TRY(ready());
  MI_TRY(launch_swiglu_rows(x, ldx, out, ldo, M, I, act, rnd, nullptr));
  return finish();
}

// lora_down_by_row_kernel and lora_up_add_by_row_kernel (lora_rows.hip) on their own: the two launches of lora_rows.h on the
// caller's buffers, the adapter table uploaded from the host arrays for the length of the call.  Everything is validated
// before the first launch -- the launchers' own refusals included, so that a call of both stages never runs half.
// tab_gain: null for mi_op_lora_rows (no entry has a gain), the table of mi_op_dora_rows otherwise
static int lora_rows_op(const void* x, int ldx, int M, int K, int act, int rnd, int pro, const void* norm_w, float eps,
                        const int32_t* row_adapter, int n_parts, const int32_t* row0, const int32_t* n,
                        const float* const* tab_a, const float* const* tab_b, const int32_t* tab_rank, const float* tab_scale,
                        const float* const* tab_gain, float* t, void* y, int ldy, void* resid, int ldr, int stages) {
  MI_TRY(ready());
  const bool down = (stages & MI_LORA_STAGE_DOWN) != 0, up = (stages & MI_LORA_STAGE_UP) != 0;
  if (stages < 1 || stages > (MI_LORA_STAGE_DOWN | MI_LORA_STAGE_UP)) return fail(MI_ERR_INVALID, "mi_op_lora_rows: stages is MI_LORA_STAGE_DOWN, _UP or both");
  if (!row_adapter || !t || !tab_a || !tab_b || !tab_rank || !tab_scale) return fail(MI_ERR_INVALID, "mi_op_lora_rows: null argument");
  if (M < 1) return fail(MI_ERR_INVALID, "mi_op_lora_rows: no rows");
  if (n_parts < 1 || n_parts > 3) return fail(MI_ERR_INVALID, "mi_op_lora_rows: 1 to 3 parts");
  if (act != MI_F32 && act != MI_BF16 && act != MI_F16) return fail(MI_ERR_INVALID, "mi_op_lora_rows: bad activation dtype");
  if (rnd != RND_NONE && rnd != RND_BF16 && rnd != RND_F16) return fail(MI_ERR_INVALID, "mi_op_lora_rows: bad rounding mode");
  if (pro != PRO_NONE && pro != PRO_NORM) return fail(MI_ERR_INVALID, "mi_op_lora_rows: bad prologue");
  const size_t es = dtype_size(act);
  if ((uintptr_t)t % sizeof(float) != 0 || (uintptr_t)row_adapter % sizeof(int32_t) != 0) return fail(MI_ERR_INVALID, "mi_op_lora_rows: misaligned buffer");
  if (down) {
    if (!x) return fail(MI_ERR_INVALID, "mi_op_lora_rows: null x");
    if (K < 1 || ldx < K) return fail(MI_ERR_INVALID, "mi_op_lora_rows: a row of x is shorter than K");
    if (pro == PRO_NORM && !norm_w) return fail(MI_ERR_INVALID, "mi_op_lora_rows: a norm without its weights");
    if (K > 36864) return fail(MI_ERR_UNSUPPORTED, "mi_op_lora_rows: K above 36864");
    if ((uintptr_t)x % es != 0 || (uintptr_t)norm_w % es != 0) return fail(MI_ERR_INVALID, "mi_op_lora_rows: misaligned buffer");
  }
  if (up) {
    if (!y || !row0 || !n) return fail(MI_ERR_INVALID, "mi_op_lora_rows: null output");
    for (int r = 0; r < n_parts; ++r)
      if (n[r] < 1 || row0[r] < 0 || (long long)row0[r] + n[r] > ldy) return fail(MI_ERR_INVALID, "mi_op_lora_rows: a part lies outside the row");
    if (resid && (n_parts != 1 || row0[0] != 0 || ldr < n[0])) return fail(MI_ERR_INVALID, "mi_op_lora_rows: a residual goes with one part at column 0");
    if ((uintptr_t)y % es != 0 || (uintptr_t)resid % es != 0) return fail(MI_ERR_INVALID, "mi_op_lora_rows: misaligned buffer");
  }
  std::vector<AdapterPart> table((size_t)n_parts * LORA_TABLE_COLS);
  for (size_t i = 0; i < table.size(); ++i) {
    if ((tab_a[i] == nullptr) != (tab_b[i] == nullptr)) return fail(MI_ERR_INVALID, "mi_op_lora_rows: a table entry with only one of A and B");
    if (tab_a[i] == nullptr) continue;
    if (tab_rank[i] < 1 || tab_rank[i] > 64) return fail(MI_ERR_INVALID, "mi_op_lora_rows: rank outside 1..64");
    if ((uintptr_t)tab_a[i] % 16 != 0 || (uintptr_t)tab_b[i] % 16 != 0) return fail(MI_ERR_INVALID, "mi_op_lora_rows: A and B must be 16-byte aligned");
    table[i].a = tab_a[i]; table[i].b = tab_b[i]; table[i].rank = tab_rank[i]; table[i].scale = tab_scale[i];
  }
  bool any_gain = false;
  for (size_t i = 0; tab_gain != nullptr && i < table.size(); ++i) {
    if (tab_gain[i] == nullptr) continue;
    if (tab_a[i] == nullptr) return fail(MI_ERR_INVALID, "mi_op_dora_rows: a gain on an entry without A and B");
    if ((uintptr_t)tab_gain[i] % sizeof(float) != 0) return fail(MI_ERR_INVALID, "mi_op_dora_rows: a gain must be 4-byte aligned");
    table[i].gain = tab_gain[i];
    any_gain = true;
  }
  void* dtab = nullptr;
  FreeGuard guard{dtab};
  MI_HIP(hipMalloc(&dtab, table.size() * sizeof(AdapterPart)));
  MI_HIP(hipMemcpy(dtab, table.data(), table.size() * sizeof(AdapterPart), hipMemcpyHostToDevice));
  LoraRowsCall c;
  c.table = (const AdapterPart*)dtab; c.row_adapter = row_adapter; c.n_parts = n_parts; c.M = M; c.K = K; c.act = act; c.rnd = rnd;
  c.t = t; c.gain = any_gain;
  if (up) for (int r = 0; r < n_parts; ++r) { c.row0[r] = row0[r]; c.n[r] = n[r]; }
  if (down) MI_TRY(launch_lora_down_by_row(c, x, ldx, pro, norm_w, eps, nullptr));
  if (up) MI_TRY(launch_lora_up_add_by_row(c, y, ldy, resid, ldr, nullptr));
  return finish();
}

int mi_op_lora_rows(const void* x, int ldx, int M, int K, int act, int rnd, int pro, const void* norm_w, float eps,
                    const int32_t* row_adapter, int n_parts, const int32_t* row0, const int32_t* n,
                    const float* const* tab_a, const float* const* tab_b, const int32_t* tab_rank, const float* tab_scale,
                    float* t, void* y, int ldy, void* resid, int ldr, int stages) {
  return lora_rows_op(x, ldx, M, K, act, rnd, pro, norm_w, eps, row_adapter, n_parts, row0, n, tab_a, tab_b, tab_rank, tab_scale,
                      nullptr, t, y, ldy, resid, ldr, stages);
}

// ... with the gains of DoRA entries in the table (the gain-aware instantiation of the up-add when one is set)
int mi_op_dora_rows(const void* x, int ldx, int M, int K, int act, int rnd, int pro, const void* norm_w, float eps,
                    const int32_t* row_adapter, int n_parts, const int32_t* row0, const int32_t* n,
                    const float* const* tab_a, const float* const* tab_b, const int32_t* tab_rank, const float* tab_scale,
                    const float* const* tab_gain, float* t, void* y, int ldy, void* resid, int ldr, int stages) {
  if (!tab_gain) return fail(MI_ERR_INVALID, "mi_op_dora_rows: null argument");
  return lora_rows_op(x, ldx, M, K, act, rnd, pro, norm_w, eps, row_adapter, n_parts, row0, n, tab_a, tab_b, tab_rank, tab_scale,
                      tab_gain, t, y, ldy, resid, ldr, stages);
}

// dora_gain_kernel (lora_rows.hip) on its own; the launch validates its arguments
int mi_op_dora_gain(const mi_op_linear* w, const float* A, const float* B, const float* m, int rank, float scale, int row0, int n,
                    float* gain) {
  if (!w) return fail(MI_ERR_INVALID, "mi_op_dora_gain: null argument");
  MI_TRY(ready());
  MI_TRY(launch_dora_gain(to_linear(w), row0, n, A, B, m, rank, scale, gain, nullptr));
  return finish();
}

// kv_copy_tokens_kernel (misc.hip) on its own; the launch validates its arguments
int mi_op_kv_copy_tokens(void* kcache, void* vcache, int kv_dtype, int layers, int64_t layer_elems, int Hkv, int D,
                         int64_t head_stride, int64_t src_off, int64_t dst_off, int n_tokens) {
  if (layer_elems < 1 || head_stride < 1 || src_off < 0 || dst_off < 0) return fail(MI_ERR_INVALID, "kv_copy_tokens: bad argument");
  MI_TRY(ready());
  MI_TRY(launch_kv_copy_tokens(kcache, vcache, kv_dtype, layers, (size_t)layer_elems, Hkv, D, (size_t)head_stride, (size_t)src_off,
                               (size_t)dst_off, n_tokens, nullptr));
  return finish();
}

int mi_op_gemv_uses_mfma(const mi_op_linear* w, const mi_op_gemv_args* a) {
  if (!w || !a) return 0;
  return gemv_mfma_supported(to_linear(w), to_call(a)) ? 1 : 0;
}

uint64_t mi_op_tiled_bytes(const mi_op_linear* w) {
  if (!w || !tiled_supported(w->wk, w->N, w->K, w->group > 0 ? w->group : 64)) return 0;
  return (uint64_t)tiled_bytes(w->wk, w->N, w->K);
}

int mi_op_repack_tiled(const mi_op_linear* w, void* dst) {
  if (!w || !dst) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  MI_TRY(launch_repack_tiled(to_linear(w), dst, nullptr));
  return finish();
}

int mi_op_embed(const mi_op_linear* w, const int32_t* tokens, int rows, int act, int rnd, void* out) {
  if (!w || !tokens || !out) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  EmbedCall ec{tokens, rows, act, rnd, out};
  MI_TRY(launch_embed(to_linear(w), ec, nullptr));
  return finish();
}

int mi_op_rope_tables(float* cos_tab, float* sin_tab, int max_pos, int head_dim, float base, float scale) {
  MI_TRY(ready());
  MI_TRY(launch_rope_tables(cos_tab, sin_tab, max_pos, head_dim, base, scale, nullptr));
  return finish();
}

int mi_op_rope_append(const mi_op_attn_shape* s, const void* qkv, void* q_out, void* kcache, void* vcache,
                      const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                      const float* cos_tab, const float* sin_tab, int max_pos) {
  if (!s) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  RopeAppendCall rc{to_shape(s), qkv, q_out, kcache, vcache, offsets, q_norm_w, k_norm_w, eps, cos_tab, sin_tab, max_pos};
  MI_TRY(launch_rope_append(rc, nullptr));
  return finish();
}

int mi_op_attention(const mi_op_attn_shape* s, const void* q, const void* kcache, const void* vcache,
                    const int32_t* offsets, void* out, float scale, int nsplit, float* partial) {
  if (!s) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  AttnCall ac{to_shape(s), q, kcache, vcache, offsets, out, scale, nsplit, partial};
  MI_TRY(launch_attention(ac, nullptr));
  return finish();
}

// one launch, or iters back-to-back launches behind a warm-up one, timed into *avg_ms
static int run_attention_decode(const AttnDecodeCall& ac, int iters, float* avg_ms) {
  if (iters <= 1) {
    MI_TRY(launch_attention_decode(ac, nullptr));
    return finish();
  }
  return run_timed_strict([&] { return launch_attention_decode(ac, nullptr); }, iters, avg_ms);
}

int mi_op_attention_decode(const mi_op_attn_shape* s, const void* qkv, void* kcache, void* vcache,
                           const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                           const float* cos_tab, const float* sin_tab, void* out, float scale, int rnd_out,
                           int nsplit, float* partial, int32_t* counters, int variant, int iters, float* avg_ms) {
  if (!s) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  AttnDecodeCall ac{to_shape(s), qkv, kcache, vcache, offsets, q_norm_w, k_norm_w, eps, cos_tab, sin_tab,
                    out, scale, rnd_out, nsplit, partial, (int*)counters, variant};
  return run_attention_decode(ac, iters, avg_ms);
}

int mi_op_attention_decode_host(const mi_op_attn_shape* s, const void* qkv, void* kcache, void* vcache,
                                const int32_t* offsets, const void* q_norm_w, const void* k_norm_w, float eps,
                                const float* cos_tab, const float* sin_tab, void* out, float scale, int rnd_out,
                                int nsplit, float* partial, int32_t* counters, int variant, int iters, float* avg_ms,
                                const int32_t* rows, const int32_t* host_row, const int32_t* host_off) {
  if (!s) return fail(MI_ERR_INVALID, "null argument");
  if ((host_row != nullptr) != (host_off != nullptr)) return fail(MI_ERR_INVALID, "attention_decode_host: host_row and host_off come together");
  if (host_row && (s->B < 1 || s->B > 32)) return fail(MI_ERR_INVALID, "attention_decode_host: host arrays take 1..32 sequences");
  MI_TRY(ready());
  AttnDecodeCall ac{to_shape(s), qkv, kcache, vcache, offsets, q_norm_w, k_norm_w, eps, cos_tab, sin_tab,
                    out, scale, rnd_out, nsplit, partial, (int*)counters, variant};
  ac.s.rows = rows;
  if (host_row) {                                  // as the engine's decode step fills them
    ac.n_host_off = s->B;
    for (int b = 0; b < s->B; ++b) { ac.host_row[b] = host_row[b]; ac.host_off[b] = host_off[b]; }
  }
  return run_attention_decode(ac, iters, avg_ms);
}

int mi_op_sample(float* logits, int B, int V, float temperature, float top_p, const float* uniforms,
                 int top_logprobs, int32_t* tokens_out, float* logprob_out, float* prob_row0_out,
                 int32_t* topk_ids, float* topk_logprobs, float* row_stats) {
  if (!logits || !tokens_out || !row_stats) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(ready());
  SampleCall sc{};
  sc.logits = logits; sc.B = B; sc.V = V; sc.rnd = RND_NONE; sc.temperature = temperature; sc.top_p = top_p;
  sc.uniforms = uniforms; sc.seed = 0; sc.step = 0; sc.top_logprobs = top_logprobs; sc.lp_temp = 0;
  sc.tokens_out = tokens_out; sc.logprob_out = logprob_out; sc.prob_row0_out = prob_row0_out;
  sc.topk_ids = topk_ids; sc.topk_logprobs = topk_logprobs; sc.row_stats = row_stats;
  MI_TRY(launch_sample(sc, nullptr));
  return finish();
}

// mi_op_sample_ex and mi_op_sample_rowbias: one launch of the sampler with every control; `who` prefixes the refusals
static int sample_op(const std::string& who, float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                     const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                     const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                     const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                     float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats,
                     int n_bias, const int32_t* bias_ids, const float* bias_values,
                     const int32_t* row_bias_counts, const int32_t* row_bias_ids, const float* row_bias_values,
                     int table_rows, int cap, const int32_t* row_map, const int32_t* row_lp_k = nullptr,
                     const int32_t* row_lp_flag = nullptr, int n_row_settings = 0, int lp_at_temperature = 0, int method = 0) {
  if (!logits || !tokens_out || !row_stats) return fail(MI_ERR_INVALID, "null argument");
  if (n_row_settings < 0 || (n_row_settings > 0 && (!row_lp_k || !row_lp_flag || table_rows < 1 || !topk_ids || !topk_logprobs)))
    return fail(MI_ERR_INVALID, who + ": row settings need row_lp_k, row_lp_flag, table_rows >= 1 and the top-k outputs");
  if (method < 0 || method > 2) return fail(MI_ERR_INVALID, who + ": method must be 0, 1 or 2");
  if (B < 1 || V < 1) return fail(MI_ERR_INVALID, who + ": B and V must be positive");
  if (top_k < 0) return fail(MI_ERR_INVALID, who + ": top_k must be >= 0 (0 = off)");
  if (!(min_p >= 0.f && min_p <= 1.f)) return fail(MI_ERR_INVALID, who + ": min_p must be in [0, 1] (0 = off)");
  if ((row_temperature != nullptr) != (row_top_p != nullptr)) return fail(MI_ERR_INVALID, who + ": row_temperature and row_top_p come together");
  if ((row_seed != nullptr) != (row_position != nullptr)) return fail(MI_ERR_INVALID, who + ": row_seed and row_position come together");
  if (n_bias < 0 || (n_bias > 0 && (!bias_ids || !bias_values))) return fail(MI_ERR_INVALID, who + ": n_bias entries need bias_ids and bias_values");
  if (row_bias_counts && (!row_bias_ids || !row_bias_values || table_rows < 1 || cap < 1))
    return fail(MI_ERR_INVALID, who + ": a table needs row_bias_ids, row_bias_values, table_rows >= 1 and cap >= 1");
  MI_TRY(ready());
  SampleCall sc{};
  sc.logits = logits; sc.B = B; sc.V = V; sc.rnd = RND_NONE; sc.temperature = temperature; sc.top_p = top_p;
  sc.n_bias = n_bias; sc.bias_ids = bias_ids; sc.bias_vals = bias_values;
  sc.uniforms = uniforms; sc.seed = seed; sc.step = step; sc.top_logprobs = top_logprobs; sc.lp_temp = lp_at_temperature ? 1 : 0;
  sc.row_temp = row_temperature; sc.row_top_p = row_top_p;
  sc.top_k = top_k; sc.min_p = min_p; sc.row_top_k = row_top_k; sc.row_min_p = row_min_p;
  sc.row_seed = row_seed; sc.row_position = row_position;
  sc.tokens_out = tokens_out; sc.logprob_out = logprob_out; sc.prob_row0_out = prob_row0_out;
  sc.topk_ids = topk_ids; sc.topk_logprobs = topk_logprobs; sc.row_stats = row_stats;
  if (row_bias_counts) {                           // (null: launch_sample picks the instantiations without the table)
    sc.rb_cnt = row_bias_counts; sc.rb_ids = row_bias_ids; sc.rb_vals = row_bias_values;
    sc.rb_rows = table_rows; sc.rb_cap = cap; sc.rb_map = row_map;
  }
  if (n_row_settings > 0) {                        // (0: the launch of a call without the arrays, whatever they hold)
    sc.lp_k = row_lp_k; sc.lp_flag = row_lp_flag; sc.topk_stride = MI_MAX_TOP_LOGPROBS; sc.lp_method = method;
    sc.rb_rows = table_rows; sc.rb_map = row_map;
  }
  MI_TRY(launch_sample(sc, nullptr));
  return finish();
}

int mi_op_sample_ex(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                    const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                    const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                    const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                    float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats) {
  return sample_op("sample_ex", logits, B, V, temperature, top_p, top_k, min_p, row_temperature, row_top_p, row_top_k, row_min_p,
                   row_seed, row_position, seed, step, uniforms, top_logprobs, tokens_out, logprob_out, prob_row0_out, topk_ids,
                   topk_logprobs, row_stats, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr);
}

int mi_op_sample_rowbias(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                         const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                         const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                         const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                         float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats,
                         int n_bias, const int32_t* bias_ids, const float* bias_values,
                         const int32_t* row_bias_counts, const int32_t* row_bias_ids, const float* row_bias_values,
                         int table_rows, int cap, const int32_t* row_map) {
  return sample_op("sample_rowbias", logits, B, V, temperature, top_p, top_k, min_p, row_temperature, row_top_p, row_top_k,
                   row_min_p, row_seed, row_position, seed, step, uniforms, top_logprobs, tokens_out, logprob_out, prob_row0_out,
                   topk_ids, topk_logprobs, row_stats, n_bias, bias_ids, bias_values, row_bias_counts, row_bias_ids,
                   row_bias_values, table_rows, cap, row_map);
}

int mi_op_sample_rowlp(float* logits, int B, int V, float temperature, float top_p, int top_k, float min_p,
                       const float* row_temperature, const float* row_top_p, const int32_t* row_top_k, const float* row_min_p,
                       const uint64_t* row_seed, const int64_t* row_position, uint64_t seed, uint64_t step,
                       const float* uniforms, int top_logprobs, int32_t* tokens_out, float* logprob_out,
                       float* prob_row0_out, int32_t* topk_ids, float* topk_logprobs, float* row_stats,
                       int n_bias, const int32_t* bias_ids, const float* bias_values,
                       const int32_t* row_bias_counts, const int32_t* row_bias_ids, const float* row_bias_values,
                       int table_rows, int cap, const int32_t* row_map, const int32_t* row_top_logprobs,
                       const int32_t* row_at_temperature, int n_row_settings, int logprobs_at_temperature, int method) {
  return sample_op("sample_rowlp", logits, B, V, temperature, top_p, top_k, min_p, row_temperature, row_top_p, row_top_k,
                   row_min_p, row_seed, row_position, seed, step, uniforms, top_logprobs, tokens_out, logprob_out, prob_row0_out,
                   topk_ids, topk_logprobs, row_stats, n_bias, bias_ids, bias_values, row_bias_counts, row_bias_ids,
                   row_bias_values, table_rows, cap, row_map, row_top_logprobs, row_at_temperature, n_row_settings,
                   logprobs_at_temperature, method);
}

}  // extern "C"

// ---- moe.hip on its own ---------------------------------------------------------------------------------------------------
namespace {
// the lists of a route, read back: every run inside list[pairs], every entry a pair whose row of x exists
int check_moe_lists(const int32_t* meta, const int32_t* list, int E, int pairs, int x_rows, int x_shift, const char* who) {
  if (!meta || !list || E < 1 || E > MOE_MAX_EXPERTS || pairs < 1) return fail(MI_ERR_INVALID, std::string(who) + ": bad lists");
  std::vector<int32_t> hm(2 * (size_t)E), hl((size_t)pairs);
  MI_HIP(hipMemcpy(hm.data(), meta, hm.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  MI_HIP(hipMemcpy(hl.data(), list, hl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int e = 0; e < E; ++e) {
    const long long cnt = hm[e], off = hm[E + e];
    if (cnt < 0 || off < 0 || off + cnt > pairs) return fail(MI_ERR_INVALID, std::string(who) + ": the list of expert " + std::to_string(e) + " leaves the list array");
    for (long long i = off; i < off + cnt; ++i)
      if (hl[i] < 0 || hl[i] >= pairs || (hl[i] >> x_shift) >= x_rows)
        return fail(MI_ERR_INVALID, std::string(who) + ": list entry " + std::to_string(i) + " is no pair of this call");
  }
  return MI_OK;
}
}  // namespace

extern "C" {

int mi_op_moe_route(const void* xn, int ldx, int R, int H, int act, int rnd, const void* wg, int wdt, int E, int k,
                    int32_t* sel, void* score, int32_t* meta, int32_t* list, int iters, float* avg_ms) {
  MI_TRY(ready());
  if (rnd != RND_NONE && rnd != RND_BF16 && rnd != RND_F16) return fail(MI_ERR_INVALID, "mi_op_moe_route: bad rounding mode");
  const MoeRouteCall c{xn, ldx, R, H, act, rnd, wg, wdt, E, k, sel, score, meta, list};
  return run_timed([&] { return launch_moe_route(c, nullptr); }, iters, avg_ms);
}

int mi_op_moe_linear(const void* x, int ldx, int x_rows, int x_shift, int act, int rnd, const void* w, int wdt, int E, int N,
                     int K, const int32_t* meta, const int32_t* list, int pairs, void* out, int ldo, int iters, float* avg_ms) {
  MI_TRY(ready());
  if (rnd != RND_NONE && rnd != RND_BF16 && rnd != RND_F16) return fail(MI_ERR_INVALID, "mi_op_moe_linear: bad rounding mode");
  if (x_shift < 0 || x_shift > 1 || x_rows < 1) return fail(MI_ERR_INVALID, "mi_op_moe_linear: bad x_rows / x_shift");
  MI_TRY(check_moe_lists(meta, list, E, pairs, x_rows, x_shift, "mi_op_moe_linear"));
  const MoeLinearCall c{x, ldx, x_shift, act, rnd, w, nullptr, wdt, E, N, K, 0, meta, list, out, ldo};
  return run_timed([&] { return launch_moe_linear(c, nullptr); }, iters, avg_ms);
}

int mi_op_moe_mlp(const void* xn, int ldx, int R, int H, int I, int act, int rnd, int wdt, int E, int k, const void* w_gate,
                  const void* w_up, const void* w_down, const int32_t* meta, const int32_t* list, const void* score,
                  const void* resid, int ldr, void* out, int ldo, int iters, float* stage_ms) {
  MI_TRY(ready());
  if (rnd != RND_NONE && rnd != RND_BF16 && rnd != RND_F16) return fail(MI_ERR_INVALID, "mi_op_moe_mlp: bad rounding mode");
  if (R < 1 || k < 1 || k > 2 || H < 64 || I < 64 || (long long)R * k > (1LL << 30)) return fail(MI_ERR_INVALID, "mi_op_moe_mlp: bad shape");
  if (act != MI_F32 && act != MI_BF16 && act != MI_F16) return fail(MI_ERR_INVALID, "mi_op_moe_mlp: bad activation dtype");
  const int P = R * k;
  MI_TRY(check_moe_lists(meta, list, E, P, R, k - 1, "mi_op_moe_mlp"));
  const size_t es = dtype_size(act);
  void* acts = nullptr; void* y = nullptr;
  FreeGuard g1{acts}, g2{y};
  MI_HIP(hipMalloc(&acts, (size_t)P * I * es));
  MI_HIP(hipMalloc(&y, (size_t)P * H * es));
  const MoeLinearCall gu{xn, ldx, k - 1, act, rnd, w_gate, w_up, wdt, E, I, H, 1, meta, list, acts, I};
  const MoeLinearCall dn{acts, I, 0, act, rnd, w_down, nullptr, wdt, E, H, I, 0, meta, list, y, H};
  int rc = run_timed([&] { return launch_moe_linear(gu, nullptr); }, iters, stage_ms);
  if (rc == MI_OK) rc = run_timed([&] { return launch_moe_linear(dn, nullptr); }, iters, stage_ms ? stage_ms + 1 : nullptr);
  if (rc == MI_OK && resid == out && resid != nullptr && iters >= 1 && stage_ms) rc = fail(MI_ERR_INVALID, "mi_op_moe_mlp: a timed call cannot add into its own residual");
  if (rc == MI_OK)
    rc = run_timed([&] { return launch_moe_combine(y, score, k, resid, ldr, out, ldo, R, H, act, rnd, nullptr); }, iters, stage_ms ? stage_ms + 2 : nullptr);
  return rc;
}

}  // extern "C"
