// engine_linear.hip -- gemv_rows: which kernel family a linear of the forward pass runs on.  gemv_rows_on is the ordered list
// of routes; every route is one function that declines (NOT_TAKEN) or runs the call, with the measurements that justify it.
#include "engine_impl.h"

namespace mi {

int launch_gemv_v1(const LinearW& W, const GemvCall& c, hipStream_t st);
int launch_gemv_mfma(const LinearW& W, const GemvCall& c, hipStream_t st);

int launch_gemv(const LinearW& W, const GemvCall& c, hipStream_t st) {
  if (gemv_mfma_supported(W, c)) return launch_gemv_mfma(W, c, st);
  return launch_gemv_v1(W, c, st);
}

// ---- persistent weight copies.  Both return true when the copy exists afterwards.  A failed allocation is not an error of
// the call: the runtime's error state is cleared, the copy is marked unavailable for this linear and the caller uses the
// path that reads the matrix as loaded.  The pointer is published only once the repack kernel has been enqueued successfully
// (same stream as every consumer).
static bool hilo_wanted(const mi_engine* e, const FusedLinear& f) {
  return f.W.wk == WK_F16 && f.W.layout == 1 && e->opt_f16_hilo && !e->opt_force_v1 && f.W.K % 256 == 0;
}
bool ensure_hilo(mi_engine* e, FusedLinear& f) {
  if (f.w_hilo != nullptr) return true;
  if (f.hilo_failed || !hilo_wanted(e, f)) return false;
  void* p = nullptr;
  if (hipMalloc(&p, 2 * (size_t)f.W.N * f.W.K * sizeof(uint16_t)) != hipSuccess) { (void)hipGetLastError(); f.hilo_failed = true; return false; }
  if (launch_f16_to_hilo(f.W, p, e->stream) != MI_OK) { hipFree(p); f.hilo_failed = true; return false; }
  f.w_hilo = p;
  return true;
}
static bool gu8_wanted(const mi_engine* e, const FusedLinear& f, int pair_offset) {
  if (f.W.bias != nullptr) return false;        // the interleaved copy's epilogues carry no bias: the paired-tile SwiGLU kernels run
  if (f.adapters != nullptr && f.adapters->engine_wide()) return false;     // every step stores gate|up for the LoRA term: the copy would never be read
  return e->opt_gu8 && !e->opt_force_v1 && f.W.layout == 1 && (f.W.wk == WK_BF16 || f.W.wk == WK_F16) &&
         f.W.N == 2 * pair_offset && pair_offset % 16 == 0;
}
bool ensure_gu8(mi_engine* e, FusedLinear& f, int pair_offset) {
  if (f.w_gu8 != nullptr) return true;
  if (f.gu8_failed || !gu8_wanted(e, f, pair_offset)) return false;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)f.W.N * f.W.K * sizeof(uint16_t)) != hipSuccess) { (void)hipGetLastError(); f.gu8_failed = true; return false; }
  if (launch_gate_up_interleave(f.W, pair_offset, p, e->stream) != MI_OK) { hipFree(p); f.gu8_failed = true; return false; }
  f.w_gu8 = p;
  return true;
}

constexpr size_t CC_GUARD = 64;                  // floats of sentinel around each part of the seam's buffer
constexpr uint32_t CC_SENTINEL = 0x7fc0c0c0u;    // (a NaN: a read of it would not go unnoticed either)
static int ensure_cc_pub(mi_engine* e, int nqkv) {
  const size_t need = (3 * CC_GUARD + (size_t)8 * 8 * nqkv + 8 * 8) * sizeof(float);
  if (need <= e->cc_pub_cap) return MI_OK;
  MI_TRY(grow(e->stream, &e->cc_pub, &e->cc_pub_cap, need));
  e->cc_pub_cap = 0;                             // (the buffer counts once its sentinels are in)
  std::vector<uint32_t> fill(need / sizeof(float), CC_SENTINEL);
  MI_HIP(hipMemcpy(e->cc_pub, fill.data(), need, hipMemcpyHostToDevice));
  e->cc_pub_cap = need;
  return MI_OK;
}
// the three sentinel runs of the seam's buffer (option "consumer_combine_guard"): intact -> MI_OK
int check_cc_guards(mi_engine* e, int nqkv) {
  if (e->cc_pub == nullptr) return fail(MI_ERR_NOTFOUND, "consumer_combine_guard: the q|k|v seam has not run");
  MI_HIP(hipStreamSynchronize(e->stream));
  const size_t body = (size_t)8 * 8 * nqkv, at[3] = {0, CC_GUARD + body, 2 * CC_GUARD + body + 64};
  uint32_t g[CC_GUARD];
  for (int i = 0; i < 3; ++i) {
    MI_HIP(hipMemcpy(g, e->cc_pub + at[i], sizeof(g), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < CC_GUARD; ++j)
      if (g[j] != CC_SENTINEL) return fail(MI_ERR_RUNTIME, "consumer_combine_guard: sentinel run " + std::to_string(i) + " was overwritten");
  }
  return MI_OK;
}
float* cc_pub_tiles(mi_engine* e) { return e->cc_pub + CC_GUARD; }
float* cc_pub_sumsq(mi_engine* e, int nqkv) { return e->cc_pub + 2 * CC_GUARD + (size_t)8 * 8 * nqkv; }

namespace {

// the split-K workspace of gemm_skinny.hip: at least `need` bytes of partial tiles and `groups` arrival counters (zeroed)
int ensure_skinny_ws(mi_engine* e, size_t need, int groups) {
  MI_TRY(grow(e->stream, &e->sk_ws, &e->sk_ws_cap, need));
  const size_t ctr = (size_t)std::max(groups, 4096) * sizeof(unsigned);
  if (ctr <= e->sk_ctr_cap) return MI_OK;
  MI_TRY(grow(e->stream, &e->sk_ctr, &e->sk_ctr_cap, ctr));
  e->sk_ctr_cap = 0;                             // (the counters count once they are zero)
  MI_HIP(hipMemsetAsync(e->sk_ctr, 0, ctr, e->stream));
  e->sk_ctr_cap = ctr;
  return MI_OK;
}
// ... sized for the call c at `rows` rows
int skinny_ws_for(mi_engine* e, const LinearW& W, const GemvCall& c, size_t rows) {
  return ensure_skinny_ws(e, gemm_skinny_ws_bytes(W, c, rows), gemm_skinny_groups(W, c, rows));
}
// ... and the call launched on it
int run_skinny(mi_engine* e, const LinearW& W, const GemvCall& c, size_t rows) {
  MI_TRY(skinny_ws_for(e, W, c, rows));
  return launch_gemm_skinny(W, c, rows, e->stream, e->sk_ws, e->sk_ctr);
}

// the call on rows [r, r + M) of its x / out / resid
GemvCall row_slab(const GemvCall& c, size_t r, size_t M, size_t es_in, size_t es_out) {
  GemvCall cc = c;
  cc.M = (int)M;
  cc.x = (const char*)c.x + r * (size_t)c.ldx * es_in;
  if (c.out) cc.out = (char*)c.out + r * (size_t)c.ldo * es_out;
  if (c.resid) cc.resid = (char*)c.resid + r * (size_t)c.ldo * es_in;
  return cc;
}

// RMSNorm of the call's x into e->xn (one workgroup per row); the call then reads e->xn with no prologue
int norm_into_xn(mi_engine* e, GemvCall& c, size_t rows, int K, int rnd) {
  MI_TRY(launch_rmsnorm_rows(c.x, c.ldx, c.norm_w, e->xn, K, (int)rows, K, c.eps, c.act, e->stream, true, rnd));
  c.x = e->xn; c.ldx = K; c.pro = PRO_NONE;
  return MI_OK;
}

// One call of gemv_rows as its routes see it.  f: the matrix the matmul kernels stream (f0 itself, or its [hi | lo] view);
// f0: the linear as loaded (true K); c: a route works on a copy; left: the hand-over the launch before this one left
struct Lin {
  mi_engine* e; const FusedLinear& f; const FusedLinear& f0; const GemvCall& c; size_t rows, es_in, es_out;
  const char* prof; const NormHandover& left; int* published;
  int KT() const { return f0.W.K; }            // the true K: columns of x
  bool quant() const { return wk_is_quant(f.W.wk); }
};
constexpr int NOT_TAKEN = 1;                   // a route's answer beside MI_OK / MI_ERR_*: the next route is asked

// Which kernel for a call that is not a pure decode step (prefill, mixed step)?  Measured on Mistral-7B shapes, one prompt
// of L tokens (ms for the whole call): dense 16-bit weights -- streaming kernel 4.2 / 5.1 /
// 6.1 / 6.9 at L = 32 / 64 / 96 / 128 against 5.2 / 5.5 / 5.6 / 5.8 on the K-split 128 x 128 tile: the hand-over is at ~80 rows;
// int4 -- 3.0 / 5.0 / 6.9 (L <= 96) against 15.5 on the tile path, which first writes a [hi | lo] 16-bit copy of every
// matrix (4 x 54 us per layer): the streaming kernel keeps the call, in two row slabs up to twice its row limit.
size_t short_rows(const Lin& a) { return a.e->opt_short_prefill_skinny ? (a.quant() ? 128 : 64) : 0; }

// 1. quantised weights, a call just above the streaming kernel's row limit: two slabs of rows, two reads of W
int route_two_slabs(const Lin& a) {
  mi_engine* e = a.e; const FusedLinear& f = a.f; const size_t rows = a.rows;
  if (!(e->opt_skinny_gemm && e->cur_L != 1 && a.quant() && e->opt_short_prefill_skinny && rows > 64 && rows <= 256 &&
        !gemm_skinny_supported(f.W, a.c, rows))) return NOT_TAKEN;
  const size_t half = (rows + 1) / 2;
  GemvCall probe = a.c; probe.pro = PRO_NONE;
  if (!gemm_skinny_supported(f.W, probe, half)) return NOT_TAKEN;
  Prof pr(e, a.prof);
  GemvCall c = a.c;
  if (c.pro == PRO_NORM) MI_TRY(norm_into_xn(e, c, rows, a.KT(), c.rnd));
  for (size_t r = 0; r < rows; r += half) {
    const GemvCall cc = row_slab(c, r, std::min(half, rows - r), a.es_in, a.es_out);
    MI_TRY(run_skinny(e, f.W, cc, (size_t)cc.M));
  }
  return MI_OK;
}

// float32-KV decode step of <= 8 sequences: what routes 2 and 3 share
bool f32_decode(const Lin& a) {
  return a.e->opt_skinny_gemm && a.e->cur_L == 1 && a.rows <= 8 && a.c.act == MI_F32 && a.c.rnd == RND_NONE && a.c.kx == 0;
}

// 2. float32-KV decode step of <= 8 sequences, the WIDE linears (at least 4 tiles per CU: gate|up on its row-interleaved copy,
// lm_head): one pass over W with one workgroup per CU and no K split (gemv_f32.hip) instead of the 9..128-row kernel below,
// whose tile groups x K slices leave CUs idle at this shape and meet through a workspace.  RMSNorm is deferred to the
// epilogue there.  Narrow linears (q|k|v, down: 1-1.5 tiles per CU) stay below -- measured, DESIGN §8d.
int route_f32_wide(const Lin& a) {
  if (!f32_decode(a)) return NOT_TAKEN;
  mi_engine* e = a.e;
  GemvCall cw = a.c;
  cw.M = (int)a.rows;
  LinearW wv = a.f.W;                          // (a view: the interleaved copy stays owned by f0)
  if (cw.epi == EPI_SWIGLU) {
    if (!(gu8_wanted(e, a.f0, cw.pair_offset) && ensure_gu8(e, const_cast<FusedLinear&>(a.f0), cw.pair_offset))) return NOT_TAKEN;
    wv.w = a.f0.w_gu8; cw.epi = EPI_SWIGLU_GU8;
  }
  if (!(wv.N / 16 >= 4 * gemv_cu_count() && gemv_f32_supported(wv, cw))) return NOT_TAKEN;
  Prof pr(e, a.prof);
  if (cw.pro == PRO_NORM && !e->opt_defer_norm) MI_TRY(norm_into_xn(e, cw, a.rows, a.KT(), cw.rnd));
  // K <= 4096: x and the norm weights stay in LDS, the stream loop waits for weight loads only (same bits)
  if (e->opt_resident_x && gemv_f32_resident_supported(wv, cw)) return launch_gemv_f32_resident(wv, cw, e->stream);
  return launch_gemv_f32(wv, cw, e->stream);
}

// 3. ... and the one NARROW linear whose whole tile a workgroup can request at once (K <= 4096, at most one tile per CU,
// no prologue: o_proj of Mistral-7B): one tile per workgroup over the whole K, no K split, no partial tiles, no arrival
// counter (gemv_f32.hip, the whole-K form).  Below half the CUs the K split is what fills the chip.
int route_f32_whole(const Lin& a) {
  if (!f32_decode(a)) return NOT_TAKEN;
  GemvCall cw = a.c;
  cw.M = (int)a.rows;
  if (!(a.f.W.N / 16 > gemv_cu_count() / 2 && gemv_f32_whole_supported(a.f.W, cw))) return NOT_TAKEN;
  Prof pr(a.e, a.prof);
  return launch_gemv_f32_whole(a.f.W, cw, a.e->stream);
}

// 4. the decode step of a batch of 9..128 sequences (int4 / int8 weights: any batch up to 128): W is streamed once, K split
// over workgroups (gemm_skinny.hip) -- up to 96 rows for dense weights: above that the K-split tile GEMM is ahead
// (Mistral-7B bf16, KV 512: 96 rows 7.18 vs 7.14 ms / step, 128 rows 8.71 vs 7.96).
// Also a prefill of up to 128 rows in all (a short prompt, a few short prompts): at that size the op is a weight
// stream, not a GEMM -- measured on Mistral-7B bf16, one prompt of 64 tokens: 13.0 ms through the 128 x 128 tile GEMM
// (32 workgroups for N = 4096) against ~6 ms here.  The price: a sequence's prefill arithmetic (summation order) now
// depends on whether the whole call is above or below 128 rows; inside one regime rows stay bit-independent of
// their neighbours (tests/test_gpu_fullsize.py).
int route_skinny(const Lin& a) {
  mi_engine* e = a.e; const FusedLinear& f = a.f; const FusedLinear& f0 = a.f0; const size_t rows = a.rows; const int KT = a.KT();
  const size_t decode_max = a.quant() ? 128 : 96;
  if (!(e->opt_skinny_gemm && ((e->cur_L == 1 && rows <= decode_max) || rows <= short_rows(a)) && gemm_skinny_supported(f.W, a.c, rows)))
    return NOT_TAKEN;
  Prof pr(e, a.prof);
  GemvCall c = a.c;
  c.M = (int)rows;
  // (float32 activations: the split-K kernel neither leaves nor takes the row statistics -- always the norm launch)
  const int take_ld = (c.act != MI_F32 && c.pro == PRO_NORM) ? gemm_skinny_handover_ld(f.W, c, rows) : 0;
  const bool handed = e->opt_norm_handover && take_ld > 0 && c.ldx == KT && a.left.matches(c.x, KT, take_ld);
  // float32 activations without logical rounding (PagedKVCache mode after layer 0): the kernel applies the row scale
  // of the RMSNorm in its epilogue (gemm_skinny.hip "defer_norm") -- no norm launch, nothing waits for row statistics
  const bool defer = e->opt_defer_norm && c.pro == PRO_NORM && c.act == MI_F32 && c.rnd == RND_NONE && !handed;
  const bool q4_prep = gemm_q4_supported(f.W, c, rows);      // gemm_q4.hip: its preparation pass over x applies the RMSNorm
  if (handed) { c.sq_in = e->d_sq; c.sq_parts = a.left.parts; }
  else if (c.pro == PRO_NORM && !defer && !q4_prep) MI_TRY(norm_into_xn(e, c, rows, KT, c.rnd));
  // consumer_combine: the offer is taken by the call that the publish-only instantiation covers (gemm_skinny.hip, CC) --
  // <= 8 unrounded float32 rows with the RMSNorm deferred, a dense bf16 matrix as loaded, 2..8 K slices
  if (a.published != nullptr && f.W.wk == WK_BF16 && c.kx == 0 && f0.W.bias == nullptr && c.rnd == RND_NONE && defer && rows <= 8) {      // (a bias is added where slices are combined: the last arriver)
    const int ks = gemm_skinny_ksplit(f.W, c, rows);
    if (ks >= 2 && ks <= 8) {
      MI_TRY(ensure_cc_pub(e, f.W.N));
      c.cc_pub = cc_pub_tiles(e); c.cc_pub_sq = cc_pub_sumsq(e, f.W.N);
      *a.published = ks;
    }
  }
  const int tgroups = gemm_skinny_tile_groups(f.W, c, rows);
  const int leave_ld = (c.act != MI_F32 && c.epi == EPI_RESID) ? gemm_skinny_handover_ld(f.W, c, rows) : 0;
  const bool produce = e->opt_norm_handover && leave_ld > 0 && tgroups <= 64 && c.ldo == f.W.N;
  if (produce) {
    if (!e->d_sq) MI_HIP(hipMalloc(&e->d_sq, (size_t)4096 * 16 * sizeof(float)));     // (64 tile groups x <= 128 rows fit eight times)
    c.sq_out = e->d_sq;
  }
  MI_TRY(run_skinny(e, f.W, c, rows));
  if (produce) e->handover.record(c.resid, tgroups, f.W.N, leave_ld);
  return MI_OK;
}

// 5. prefill: one MFMA tile GEMM over all rows (the RMSNorm runs as its own row-wise kernel)
int route_prefill_gemm(const Lin& a) {
  mi_engine* e = a.e; const FusedLinear& f = a.f; const size_t rows = a.rows; const int KT = a.KT();
  if (!(e->opt_prefill_gemm && gemm_prefill_supported(f.W, a.c, rows))) return NOT_TAKEN;
  Prof pr(e, a.prof);
  GemvCall c = a.c;
  if (c.act == MI_F32) {      // PagedKVCache mode: (norm +) exact three-way split of x, then the same tile GEMM over 3 K
    MI_TRY(grow(e->stream, &e->xs, &e->xs_cap, split3_bytes(rows, KT)));
    // dense bf16 weights: two terms (16+ mantissa bits of x, two walks of W; option "prefill_x_terms"); int4 / [hi | lo]
    // matrices keep the exact three (their own pair needs the 3 : 2 walk)
    const int terms = (e->opt_prefill_x_terms == 2 && f.W.wk == WK_BF16 && c.kx == 0 && c.rnd == RND_NONE) ? 2 : 3;
    MI_TRY(launch_split3_rows(c.x, c.ldx, c.pro == PRO_NORM ? c.norm_w : nullptr, c.eps, e->xs, (int)rows, KT, e->stream, terms));
    c.x = e->xs; c.ldx = terms * KT; c.pro = PRO_NONE;
  } else if (c.pro == PRO_NORM) {    // (one workgroup per row also here: one L2 round trip per row instead of a wave's 16)
    MI_TRY(norm_into_xn(e, c, rows, KT, RND_NONE));
  }
  void* scratch = nullptr;
  if (a.quant()) {                             // int4: the GEMM multiplies by a [hi | lo] 16-bit copy made on the fly
    MI_TRY(grow(e->stream, &e->deq_scratch, &e->deq_cap, dequant_hilo_bytes(f.W.N, KT)));
    scratch = e->deq_scratch;
  }
  if (rows < 4096 && e->gk_ws == nullptr) {     // K-split partial tiles of the tile GEMMs (one prompt of a few hundred to a few thousand rows)
    e->gk_cap = (size_t)128 << 20;
    if (hipMalloc(&e->gk_ws, e->gk_cap) != hipSuccess) { e->gk_ws = nullptr; e->gk_cap = 0; }
  }
  return launch_gemm_prefill(f.W, c, rows, e->stream, scratch, rows < 4096 ? e->gk_ws : nullptr, e->gk_cap);
}

// 6. PagedKVCache mode, more than 32 rows (its prefill): 32 rows per launch of the float32-activation streaming kernel
// (each row's arithmetic is that of a decode step, whatever the batch); the generic kernel took 8 rows per pass
// over W.  A tile GEMM with the three-way split of x is the next step for this mode.
int route_f32_chunks(const Lin& a) {
  mi_engine* e = a.e; const FusedLinear& f = a.f; const size_t rows = a.rows;
  if (!(e->opt_skinny_gemm && a.c.act == MI_F32 && rows > 32 && gemm_skinny_supported(f.W, a.c, 32))) return NOT_TAKEN;
  Prof pr(e, a.prof);
  GemvCall c = a.c;
  if (c.pro == PRO_NORM) MI_TRY(norm_into_xn(e, c, rows, a.KT(), c.rnd));
  // workspace for every chunk size that is launched below, before the first launch: full 32-row chunks and the tail, whose
  // plan (tile rows, K split) is made for ITS row count and can need more partial-tile space than the 32-row plan
  GemvCall c32 = c; c32.M = 32;
  MI_TRY(skinny_ws_for(e, f.W, c32, 32));
  if (const size_t tail = rows % 32) { GemvCall ct = c; ct.M = (int)tail; MI_TRY(skinny_ws_for(e, f.W, ct, tail)); }
  for (size_t r = 0; r < rows; r += 32) {
    GemvCall cc = row_slab(c, r, std::min<size_t>(32, rows - r), a.es_in, a.es_out);
    MI_TRY(launch_gemm_skinny(f.W, cc, (size_t)cc.M, e->stream, e->sk_ws, e->sk_ctr));
  }
  return MI_OK;
}

// 7. the generic per-8 / per-16-row kernels read the matrix as loaded (an f16 model falls back to its f16 weights, exact VALU)
int route_generic(const Lin& a) {
  mi_engine* e = a.e; const FusedLinear& f0 = a.f0; const size_t rows = a.rows;
  GemvCall c = a.c;
  c.kx = 0;
  GemvCall probe = c; probe.M = (int)std::min<size_t>(rows, 16);
  const bool mfma = gemv_mfma_supported(f0.W, probe);
  const size_t step = mfma ? 16 : 8;
  // measurement: the MFMA kernel is stamped with its own dispatch begin/end (hipExtLaunchKernelGGL);
  // other paths are bracketed with events on the stream
  const bool selected = !e->prof_name.empty() && e->prof_name == a.prof;
  const bool stamp = selected && mfma && rows <= step;
  Prof pr(e, stamp ? "" : a.prof);
  if (stamp) {
    hipEvent_t ea = nullptr, eb = nullptr;
    hipEventCreate(&ea); hipEventCreate(&eb);
    c.ev_start = ea; c.ev_stop = eb;
    e->prof_events.emplace_back(ea, eb);
  }
  // SwiGLU on the matrix-core GEMV: the row-interleaved copy of the gate|up matrix (repack.hip; made by mi_engine_finalize,
  // here only if the option was switched on later; without it the paired-tile form below)
  const bool gu8 = mfma && c.epi == EPI_SWIGLU && gu8_wanted(e, f0, c.pair_offset) &&
                   ensure_gu8(e, const_cast<FusedLinear&>(f0), c.pair_offset);
  for (size_t r = 0; r < rows; r += step) {
    GemvCall cc = row_slab(c, r, std::min(step, rows - r), a.es_in, a.es_out);
    if (gu8) {
      LinearW wv = f0.W;                       // (a view: the copy stays owned by f0)
      wv.w = f0.w_gu8;
      cc.epi = EPI_SWIGLU_GU8;
      MI_TRY(launch_gemv_mfma(wv, cc, e->stream));
      continue;
    }
    MI_TRY(launch_gemv(f0.W, cc, e->stream));
  }
  return MI_OK;
}

// the routes in the order they are asked; the first that does not decline runs the call
int gemv_rows_on(const Lin& a) {
  int rc;
  if ((rc = route_two_slabs(a)) != NOT_TAKEN) return rc;
  if ((rc = route_f32_wide(a)) != NOT_TAKEN) return rc;
  if ((rc = route_f32_whole(a)) != NOT_TAKEN) return rc;
  if ((rc = route_skinny(a)) != NOT_TAKEN) return rc;
  if ((rc = route_prefill_gemm(a)) != NOT_TAKEN) return rc;
  if ((rc = route_f32_chunks(a)) != NOT_TAKEN) return rc;
  return route_generic(a);
}

}  // namespace

int gemv_rows(mi_engine* e, const FusedLinear& f0, GemvCall c, size_t rows, size_t es_in, size_t es_out, const char* prof,
              int* published) {
  if (published != nullptr) *published = 0;
  c.force_v1 = e->opt_force_v1;
  c.cc_pub = nullptr; c.cc_pub_sq = nullptr;     // (set by the split-K route alone, when it takes the offer)
  const NormHandover left = e->handover;      // whatever runs now consumes or invalidates the hand-over
  e->handover.valid = false;
  // An f16 model in the PagedKVCache mode (float32 activations): the matrix-core kernels of that mode multiply an exact
  // three-way bf16 split of x by bf16 weights, so an f16 matrix is used through its exact [hi | lo] bf16 copy (2 K
  // columns, x walked twice: GemvCall::kx) -- made by mi_engine_finalize (here only if the option was switched on later),
  // twice the matrix's bytes; without it (allocation failed) the exact VALU kernel reads the f16 matrix.  Everything that is
  // about x (norms, the split) keeps the true K of f0.
  if (c.act == MI_F32 && hilo_wanted(e, f0) && ensure_hilo(e, const_cast<FusedLinear&>(f0))) {
    FusedLinear fh = f0;                       // (a view: the pointers stay owned by f0)
    fh.W.wk = WK_BF16; fh.W.w = f0.w_hilo; fh.W.K = 2 * f0.W.K;
    c.kx = f0.W.K;
    return gemv_rows_on(Lin{e, fh, f0, c, rows, es_in, es_out, prof, left, published});
  }
  return gemv_rows_on(Lin{e, f0, f0, c, rows, es_in, es_out, prof, left, published});
}

}  // namespace mi
