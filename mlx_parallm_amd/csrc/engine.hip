// engine.hip -- the engine itself: create / destroy, the activation workspace, the forward pass, sampling and the step
// functions, options, profiling and the library's error state (the other parts: engine_impl.h).
#include <cmath>
#include <cstring>

#include "engine_impl.h"

namespace mi {

static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
int fail(int code, const std::string& m) { g_err = m; return code; }

}  // namespace mi

using namespace mi;

namespace {

// The activation workspace for `rows` token rows, `logit_rows` rows of logits and a batch of B sampled rows.  A group of buffers
// that grows together counts (ws_rows, maxB) only while all of it is there: a failed growth leaves the count 0 and every
// pointer of the group null or valid, so the next call allocates again instead of passing the size check.
int ensure_workspace(mi_engine* e, size_t rows, size_t logit_rows, int B) {
  const mi_model_desc& d = e->d;
  if (rows > e->ws_rows) {
    MI_HIP(hipStreamSynchronize(e->stream));
    const size_t es = 4;  // sized for float32 activations (the widest mode)
    const size_t nqkv = (size_t)(d.num_heads + 2 * d.num_kv_heads) * d.head_dim, qd = (size_t)d.num_heads * d.head_dim;
    const struct { void** p; size_t bytes; } bufs[5] = {
        {&e->h, rows * d.hidden_size * es}, {&e->qkv, rows * nqkv * es}, {&e->q, rows * qd * es}, {&e->attn, rows * qd * es},
        {&e->act, rows * (size_t)d.intermediate_size * es}};
    e->ws_rows = 0;
    for (const auto& b : bufs) { hipFree(*b.p); *b.p = nullptr; }
    for (const auto& b : bufs) MI_HIP(hipMalloc(b.p, b.bytes));
    hipFree(e->xn); e->xn = nullptr;
    MI_HIP(hipMalloc(&e->xn, rows * (size_t)d.hidden_size * es));
    e->ws_rows = rows;
  }
  MI_TRY(grow(e->stream, &e->logits, &e->logits_cap, logit_rows * (size_t)d.vocab_size * sizeof(float)));
  MI_TRY(grow(e->stream, &e->d_tokens, &e->d_tokens_cap, rows * sizeof(int32_t)));
  if (B > e->maxB) {
    MI_HIP(hipStreamSynchronize(e->stream));
    e->maxB = 0;
    hipFree(e->d_next); hipFree(e->d_rowstats); hipFree(e->d_uniforms);      // (d_logprob / d_prob0 live in d_next's block)
    hipFree(e->d_topk_ids); hipFree(e->d_topk_lp);
    e->d_next = e->d_topk_ids = nullptr;
    e->d_logprob = e->d_prob0 = e->d_rowstats = e->d_uniforms = e->d_topk_lp = nullptr;
    // tokens | logprobs | row-0 probabilities of a step in ONE block: one device-to-host copy per step instead of three
    MI_HIP(hipMalloc(&e->d_next, (size_t)3 * B * sizeof(int32_t)));
    e->d_logprob = (float*)(e->d_next + B);
    e->d_prob0 = (float*)(e->d_next + 2 * B);
    MI_HIP(hipMalloc(&e->d_rowstats, 2 * B * sizeof(float)));
    MI_HIP(hipMalloc(&e->d_uniforms, B * sizeof(float)));
    MI_HIP(hipMalloc(&e->d_topk_ids, (size_t)B * MI_MAX_TOP_LOGPROBS * sizeof(int32_t)));
    MI_HIP(hipMalloc(&e->d_topk_lp, (size_t)B * MI_MAX_TOP_LOGPROBS * sizeof(float)));
    for (auto& s : e->slots) {
      hipHostFree(s.tokens); hipHostFree(s.topk_ids); hipHostFree(s.topk_lp);       // (logprob / prob0 live in tokens' block)
      s.tokens = s.topk_ids = nullptr;
      s.logprob = s.prob0 = s.topk_lp = nullptr;
      MI_HIP(hipHostMalloc(&s.tokens, (size_t)3 * B * sizeof(int32_t)));
      s.logprob = (float*)(s.tokens + B);
      s.prob0 = (float*)(s.tokens + 2 * B);
      MI_HIP(hipHostMalloc(&s.topk_ids, (size_t)B * MI_MAX_TOP_LOGPROBS * sizeof(int32_t)));
      MI_HIP(hipHostMalloc(&s.topk_lp, (size_t)B * MI_MAX_TOP_LOGPROBS * sizeof(float)));
      if (!s.ev) MI_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    e->maxB = B;
  }
  return MI_OK;
}

int choose_nsplit(const mi_kv* kv, int B, int Hkv, int L, const int32_t* rows = nullptr) {
  if (L != 1) return 1;
  int mx = 0;
  for (int b = 0; b < B; ++b) mx = std::max(mx, kv->h_off[rows ? rows[b] : b] + 1);
  // float32 caches, at most one (sequence, kv head) pair per CU: the largest split count whose workgroups fit the CUs in one
  // wave, with at least 64 keys per split up to 8 splits and at least 128 beyond, and no step-down.  From tools/bench_attn.py
  // --kv float32 (Mistral-7B heads, B = 1 .. 6, 8, 16, 32, KV 256 .. 4096, 1 .. 16 splits): a launch of more
  // workgroups than CUs falls off a cliff (B = 8, KV 1060: 4 splits 17.4 us, 5 splits 24.3; B = 3: 10 splits 12.2, 11 splits
  // = 264 workgroups 15.8; B = 8, KV 4097: 4 splits 45.4, the 5 that the 1024-key limit below asks for 59.0); up to the CU
  // count the stepped-down count is nowhere faster and 0.5 - 1.0 us slower at KV 256 .. 1060 (the waves walk their own
  // keys and the splits are cut in whole tiles -- attn_decode.hip -- so a short last round costs two or three waves a tile
  // each, not all eight a round); sixteen 69-key splits are 1.2 us slower than eight (B = 2, KV 1060: the merge).
  const int cus = gemv_cu_count();
  if (kv->dtype == MI_F32 && B * Hkv <= cus)
    return std::max(1, std::min({cus / (B * Hkv), std::max(std::min(mx / 64, 8), mx / 128), 16}));
  int ns = (256 + B * Hkv - 1) / (B * Hkv);
  ns = std::min(ns, std::max(1, mx / 64));
  // long contexts: at most four 256-key rounds per workgroup -- eight when the batch alone fills the CUs (every extra
  // workgroup then costs a prologue and a merge on a CU that is already busy)
  const int per_wg = B * Hkv >= 256 ? 2048 : 1024;
  ns = std::max(ns, (mx + per_wg - 1) / per_wg);
  ns = std::max(1, std::min(ns, 16));
  // a workgroup walks its keys in rounds of 256 (float32 caches: 128): the smallest split count with the SAME number of
  // rounds has fewer workgroups to start and fewer partials to merge (KV length 1100, B = 8, bf16: 4 -> 3 splits, 2238 ->
  // 2252 tok/s; more splits are slower: 5 / 6 / 8 splits 2175 / 2173 / 2155)
  const int rk = kv->dtype == MI_F32 ? 128 : 256;
  auto rounds = [&](int n) { return ((mx - 1 + n - 1) / n + rk - 1) / rk; };     // (the cached keys; the new one is merged from registers)
  const int r0 = rounds(ns);
  while (ns > 1 && rounds(ns - 1) == r0) --ns;
  return std::max(1, std::min(ns, 16));
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// MI_ARCH_MIXTRAL, the MLP half of a block (mixtral.py:108-119,143-144): xn = post_attention_layernorm(h) once, then route,
// grouped gate|up + SwiGLU, grouped down, combine + residual -- six kernels on the stream, nothing read back.  T is `act`
// without a logical rounding (the activations behind the first attention: float32 in the float32-KV mode).
int moe_block(mi_engine* e, LayerW& lw, size_t R, int act, bool w32) {
  const mi_model_desc& d = e->d;
  const int H = d.hidden_size, I = d.intermediate_size, E = d.num_local_experts, k = d.num_experts_per_tok;
  const size_t es = dtype_size(act), P = R * k;
  hipStream_t st = e->stream;
  e->handover.valid = false;      // (o_proj's row sums describe h before this block adds to it: nothing here takes them)
  const size_t o_sel = 0, o_score = o_sel + align256(P * 4), o_meta = o_score + align256(P * es),
               o_list = o_meta + align256(2 * (size_t)E * 4), o_act = o_list + align256(P * 4), o_y = o_act + align256(P * I * es),
               total = o_y + align256(P * H * es);
  MI_TRY(grow(st, &e->moe_ws, &e->moe_ws_cap, total));
  char* ws = e->moe_ws;
  int32_t* sel = (int32_t*)(ws + o_sel); void* score = ws + o_score; int32_t* meta = (int32_t*)(ws + o_meta); int32_t* list = (int32_t*)(ws + o_list);
  void* acts = ws + o_act; void* y = ws + o_y;
  { Prof pr(e, "moe_route");
    MI_TRY(launch_rmsnorm_rows(e->h, H, w32 ? lw.post_norm32 : lw.post_norm, e->xn, H, (int)R, H, d.rms_norm_eps, act, st, true, RND_NONE));
    MoeRouteCall rc{e->xn, H, (int)R, H, act, RND_NONE, lw.moe_router, d.act_dtype, E, k, sel, score, meta, list};
    MI_TRY(launch_moe_route(rc, st)); }
  { Prof pr(e, "moe_gate_up");
    MoeLinearCall c{e->xn, H, k == 2 ? 1 : 0, act, RND_NONE, lw.moe_w[0], lw.moe_w[1], d.act_dtype, E, I, H, 1, meta, list, acts, I};
    MI_TRY(launch_moe_linear(c, st)); }
  { Prof pr(e, "moe_down");
    MoeLinearCall c{acts, I, 0, act, RND_NONE, lw.moe_w[2], nullptr, d.act_dtype, E, H, I, 0, meta, list, y, H};
    MI_TRY(launch_moe_linear(c, st)); }
  Prof pr(e, "moe_combine");
  return launch_moe_combine(y, score, k, e->h, H, e->h, H, (int)R, H, act, RND_NONE, st);
}

// A group of cache rows that advance by the same number of tokens in one forward pass: entries [r0, r0 + B) of the
// call's row list, L tokens each, the group's first token at position tok0 of the token buffer.
struct AttnGroup { int r0, B, L; size_t tok0; };

// Which hidden states feed the head: none; the last position of every row or every position (a call of ONE group);
// the token positions listed in `gather` (mixed steps).
enum class Head { NONE, LAST, ALL, GATHER };

// The model forward for the tokens already in e->d_tokens (or at e->tok_src); logits of the head's rows end up in
// e->logits (float32, [rows][V]).  `rows` (host) = the cache row of every entry of the call, in group order; null =
// entry b is row b.  All linear layers run ONCE over the concatenated tokens of every group (a chunked prefill next to
// the live decode rows reads the weights of a layer once for both); every group runs attention of its own.
// cur_L: tokens per row as gemv_rows sees it (1 = the decode step's kernels).  `what` prefixes the error messages.
int forward(mi_engine* e, mi_kv* kv, const int32_t* rows, const std::vector<AttnGroup>& groups, int cur_L, Head head,
            const std::vector<int32_t>& gather = {}, const char* what = "forward") {
  const mi_model_desc& d = e->d;
  const bool quirk = kv->quirk;
  const int act = quirk ? MI_F32 : d.act_dtype;
  const size_t es = dtype_size(act);
  const int rndT = quirk ? (d.act_dtype == MI_BF16 ? RND_BF16 : RND_F16) : RND_NONE;
  const int H = d.hidden_size, D = d.head_dim, Hq = d.num_heads, Hkv = d.num_kv_heads, I = d.intermediate_size;
  const int nqkv = (Hq + 2 * Hkv) * D;
  hipStream_t st = e->stream;
  auto row_of = [&](const AttnGroup& g, int b) { return rows ? rows[g.r0 + b] : g.r0 + b; };
  int n = 0; size_t R = 0;
  for (const AttnGroup& g : groups) {
    for (int b = 0; b < g.B; ++b)
      if (kv->h_off[row_of(g, b)] + g.L > kv->cap || kv->h_off[row_of(g, b)] + g.L > d.max_positions)
        return fail(MI_ERR_INVALID, std::string(what) + ": KV capacity / max_positions exceeded (call mi_kv_reserve)");
    n += g.B; R += (size_t)g.B * g.L;
  }
  // adapters: the table column of every token row.  The engine-wide adapter: its private column for every row (the cache rows
  // name nothing and keep -1, so prefix chains and forks are those of an engine without adapters).  Per-request adapters:
  // the slot of the row's cache row.  A step none of whose rows names an adapter (by_row stays false) runs the launches of
  // an engine without adapters, whatever is resident.
  bool by_row = e->engine_lora;
  std::vector<int32_t> tok_adapter;
  if (by_row) tok_adapter.assign(R, LORA_ENGINE_COL);
  for (const AttnGroup& g : groups)
    for (int b = 0; b < g.B; ++b) {
      const int a = kv->row_adapter[row_of(g, b)];
      if (a < 0) continue;
      if (e->adapter_parts[a] == 0)
        return fail(MI_ERR_INVALID, std::string(what) + ": cache row " + std::to_string(row_of(g, b)) + " names adapter " + std::to_string(a) +
                                        ", an empty slot (mi_engine_set_adapter_lora)");
      if (!by_row) { tok_adapter.assign(R, -1); by_row = true; }
      std::fill_n(tok_adapter.begin() + g.tok0 + (size_t)b * g.L, g.L, a);
    }
  e->cur_L = cur_L;
  e->handover.valid = false;
  if (by_row) {
    MI_TRY(grow(st, &e->d_row_adapter, &e->d_row_adapter_cap, R * sizeof(int32_t)));
    MI_TRY(grow(st, &e->lora_rt, &e->lora_rt_cap, R * LORA_ROWS_T_LD * sizeof(float)));
    MI_HIP(hipMemcpyAsync(e->d_row_adapter, tok_adapter.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  // the adapted form of linear f in this step: some row runs an adapter and some resident adapter covers f
  auto rows_adapt = [&](const FusedLinear& f) { return by_row && f.adapters != nullptr && f.adapters->set > 0; };
  auto rows_call = [&](const FusedLinear& f, int K, int rnd_) {
    LoraRowsCall rc;
    rc.table = f.adapters->d; rc.row_adapter = e->d_row_adapter; rc.n_parts = f.n_parts;
    for (int i = 0, r0 = 0; i < f.n_parts; ++i) { rc.row0[i] = r0; rc.n[i] = f.part_rows[i]; r0 += f.part_rows[i]; }
    rc.M = (int)R; rc.K = K; rc.act = act; rc.rnd = rnd_; rc.t = e->lora_rt;
    rc.gain = f.adapters->gains > 0;
    return rc;
  };
  // o_proj / down_proj (c: the EPI_RESID call): an adapted one stores y = T(acc [+ b]) to a scratch buffer and ONE launch
  // adds the rows' terms and then the residual -- y' = T(y + T(scale z)) first, h = T(h + y') second (the
  // reference's order; adding the term onto an already summed residual would round differently)
  auto resid_linear = [&](const FusedLinear& f, GemvCall c, int K, const char* prof) -> int {
    if (!rows_adapt(f)) return gemv_rows(e, f, c, R, es, es, prof);
    const LoraRowsCall rc = rows_call(f, K, c.rnd);
    MI_TRY(grow(st, &e->ys, &e->ys_cap, R * (size_t)H * 4));                // (sized for float32 activations)
    { Prof pr(e, "lora_rows"); MI_TRY(launch_lora_down_by_row(rc, c.x, c.ldx, PRO_NONE, nullptr, 0.f, st)); }
    c.epi = EPI_STORE; c.out = e->ys; c.resid = nullptr;
    MI_TRY(gemv_rows(e, f, c, R, es, es, prof));
    Prof pr(e, "lora_rows");
    return launch_lora_up_add_by_row(rc, e->ys, c.ldo, e->h, c.ldo, st);
  };
  if (rows) {
    if (!kv->d_rows) MI_HIP(hipMalloc(&kv->d_rows, kv->B * sizeof(int32_t)));
    MI_HIP(hipMemcpyAsync(kv->d_rows, rows, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  auto d_rows_of = [&](const AttnGroup& g) -> const int32_t* { return rows ? kv->d_rows + g.r0 : nullptr; };
  for (const AttnGroup& g : groups)
    for (int b = 0; b < g.B; ++b) MI_TRY(kv_ensure_blocks(kv, row_of(g, b), kv->h_off[row_of(g, b)] + g.L));
  MI_TRY(kv_upload_table(kv, st));

  { Prof pr(e, "embed");
    EmbedCall ec{e->tok_src ? e->tok_src : e->d_tokens, (int)R, act, rndT, e->h};
    MI_TRY(launch_embed(e->embed.W, ec, st)); }

  const size_t layer_elems = kv_layer_elems(kv, d);
  const size_t kes = dtype_size(kv->dtype);
  std::vector<int> nsplit(groups.size());
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const AttnGroup& g = groups[gi];
    nsplit[gi] = choose_nsplit(kv, g.B, Hkv, g.L, rows ? rows + g.r0 : nullptr);
    // (sized once for 16 splits, the most choose_nsplit returns)
    if (nsplit[gi] > 1) MI_TRY(grow(st, &kv->partial, &kv->partial_cap, (size_t)kv->B * Hq * 16 * (D + 2) * sizeof(float)));
  }

  for (int li = 0; li < d.num_layers; ++li) {
    LayerW& lw = e->layers[li];
    const bool w32 = quirk && d.act_dtype != MI_F32;     // norm weights must match the activation storage type
    const void* q_norm = w32 ? lw.q_norm32 : lw.q_norm;
    const void* k_norm = w32 ? lw.k_norm32 : lw.k_norm;
    // everything up to the layer-0 attention still rounds to the model dtype in quirk mode
    const int rnd = (quirk && li == 0) ? rndT : RND_NONE;
    // consumer_combine: a decode step of one group of at most 8 rows (every cache row, in order: not a row-subset step)
    // whose attention runs on the float32 MFMA kernel can add published K slices of q|k|v in its prologue
    bool cc_attn = false;
    int qkv_ks = 0;                              // > 0: this layer's q|k|v ran publish-only with that many K slices
    if (e->opt_consumer_combine && e->opt_defer_norm && cur_L == 1 && rows == nullptr && groups.size() == 1 && groups[0].L == 1 && R <= 8 && act == MI_F32 &&
        kv->dtype == MI_F32 && e->opt_fused_attn && e->opt_attn_mfma && D % 64 == 0 && D <= 128) {
      AttnShape s{groups[0].B, 1, Hq, Hkv, D, act, kv->dtype, rnd, kv->cap, nullptr};
      cc_attn = attention_decode_supported(s);
    }
    { // input_layernorm + q|k|v projections (llama.py:187,93)
      GemvCall c; c.x = e->h; c.ldx = H; c.act = act; c.rnd = rnd; c.pro = PRO_NORM;
      c.norm_w = w32 ? lw.in_norm32 : lw.in_norm; c.eps = d.rms_norm_eps; c.epi = EPI_STORE; c.out = e->qkv; c.ldo = nqkv;
      if (rows_adapt(lw.qkv)) {
        // adapted: t = x A by row, the base linear stores q|k|v, the rows' terms are added to the stored output
        const LoraRowsCall rc = rows_call(lw.qkv, H, rnd);
        { Prof pr(e, "lora_rows"); MI_TRY(launch_lora_down_by_row(rc, c.x, c.ldx, c.pro, c.norm_w, c.eps, st)); }
        MI_TRY(gemv_rows(e, lw.qkv, c, R, es, es, "gemv_qkv"));
        Prof pr(e, "lora_rows");
        MI_TRY(launch_lora_up_add_by_row(rc, e->qkv, nqkv, nullptr, 0, st));
      } else {
        // (the offer: gemv_rows takes it -- qkv_ks K slices published -- or runs the ordinary launch)
        MI_TRY(gemv_rows(e, lw.qkv, c, R, es, es, "gemv_qkv", cc_attn ? &qkv_ks : nullptr));
      } }
    void* kc = (char*)kv->k + (size_t)li * layer_elems * kes;
    void* vc = (char*)kv->v + (size_t)li * layer_elems * kes;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const AttnGroup& g = groups[gi];
      AttnShape s{g.B, g.L, Hq, Hkv, D, act, kv->dtype, rnd, kv->cap, d_rows_of(g)};
      kv_shape(kv, s);
      const void* qkv_g = (const char*)e->qkv + g.tok0 * (size_t)nqkv * es;
      void* q_g = (char*)e->q + g.tok0 * (size_t)Hq * D * es;
      void* o_g = (char*)e->attn + g.tok0 * (size_t)Hq * D * es;
      if (g.L == 1 && e->opt_fused_attn && attention_decode_supported(s)) {
        // decode: norm + RoPE + append + attention + split combine in one launch
        AttnDecodeCall ac{s, qkv_g, kc, vc, kv->d_off, q_norm, k_norm, d.rms_norm_eps, e->cos_tab, e->sin_tab,
                          o_g, 1.0f / sqrtf((float)D), RND_NONE, nsplit[gi], kv->partial, kv->counters,
                          e->opt_attn_mfma ? 0 : 1};
        if (g.B <= 32) {
          ac.n_host_off = g.B;
          for (int b = 0; b < g.B; ++b) { ac.host_row[b] = row_of(g, b); ac.host_off[b] = kv->h_off[row_of(g, b)]; }
        }
        if (qkv_ks > 0) {
          ac.qkv_pub = cc_pub_tiles(e); ac.qkv_pub_sq = cc_pub_sumsq(e, nqkv);
          ac.qkv_ksplit = qkv_ks; ac.hidden_k = H; ac.qkv_eps = d.rms_norm_eps;
        }
        Prof pr(e, "attn");
        MI_TRY(launch_attention_decode(ac, st));
      } else {
        if (qkv_ks > 0) return fail(MI_ERR_RUNTIME, "consumer_combine: the attention left the fused kernel");
        { Prof pr(e, "rope_append");
          RopeAppendCall rc{s, qkv_g, q_g, kc, vc, kv->d_off, q_norm, k_norm, d.rms_norm_eps,
                            e->cos_tab, e->sin_tab, d.max_positions};
          MI_TRY(launch_rope_append(rc, st)); }
        { Prof pr(e, "attn");
          AttnShape sa = s; sa.rnd = RND_NONE;  // SDPA output dtype = promote(q, kv): float32 in quirk mode
          AttnCall ac{sa, q_g, kc, vc, kv->d_off, o_g, 1.0f / sqrtf((float)D), nsplit[gi], kv->partial,
                      e->opt_attn_mfma ? 0 : 1};
          MI_TRY(launch_attention(ac, st)); }
      }
    }
    { // o_proj + residual (llama.py:143,188)
      GemvCall c; c.x = e->attn; c.ldx = Hq * D; c.act = act; c.rnd = RND_NONE; c.epi = EPI_RESID; c.resid = e->h; c.ldo = H;
      MI_TRY(resid_linear(lw.o, c, Hq * D, "gemv_o")); }
    if (d.arch == MI_ARCH_MIXTRAL) {
      MI_TRY(moe_block(e, lw, R, act, w32));
      continue;
    }
    { // post_attention_layernorm + gate|up + SwiGLU (llama.py:189,165)
      GemvCall c; c.x = e->h; c.ldx = H; c.act = act; c.rnd = RND_NONE; c.pro = PRO_NORM; c.norm_w = w32 ? lw.post_norm32 : lw.post_norm;
      c.eps = d.rms_norm_eps; c.epi = EPI_SWIGLU; c.out = e->act; c.ldo = I; c.pair_offset = I;
      if (rows_adapt(lw.gate_up)) {
        // adapted gate and / or up: no SwiGLU epilogue carries the LoRA term, so the linear stores gate|up, the rows' terms
        // are added to the stored rows and a row-wise kernel applies SwiGLU to them
        const LoraRowsCall rc = rows_call(lw.gate_up, H, c.rnd);
        MI_TRY(grow(st, &e->gu, &e->gu_cap, R * 2 * (size_t)I * 4));      // (sized for float32 activations)
        { Prof pr(e, "lora_rows"); MI_TRY(launch_lora_down_by_row(rc, c.x, c.ldx, c.pro, c.norm_w, c.eps, st)); }
        c.epi = EPI_STORE; c.out = e->gu; c.ldo = 2 * I; c.pair_offset = 0;
        MI_TRY(gemv_rows(e, lw.gate_up, c, R, es, es, "gemv_gate_up"));
        { Prof pr(e, "lora_rows"); MI_TRY(launch_lora_up_add_by_row(rc, e->gu, 2 * I, nullptr, 0, st)); }
        Prof pr(e, "swiglu_rows");
        MI_TRY(launch_swiglu_rows(e->gu, 2 * I, e->act, I, (int)R, I, act, c.rnd, st));
      } else {
        MI_TRY(gemv_rows(e, lw.gate_up, c, R, es, es, "gemv_gate_up"));
      } }
    { // down_proj + residual (llama.py:165,190)
      GemvCall c; c.x = e->act; c.ldx = I; c.act = act; c.rnd = RND_NONE; c.epi = EPI_RESID; c.resid = e->h; c.ldo = H;
      MI_TRY(resid_linear(lw.down, c, I, "gemv_down")); }
  }
  if (head != Head::NONE) {  // final norm + lm_head / tied embedding (llama.py:231,249-252)
    const FusedLinear& hw = d.tie_word_embeddings ? e->embed : e->lm_head;
    GemvCall c; c.act = act; c.rnd = RND_NONE; c.pro = PRO_NORM; c.norm_w = (quirk && d.act_dtype != MI_F32) ? e->final_norm32 : e->final_norm; c.eps = d.rms_norm_eps;
    c.epi = EPI_STORE_F32; c.out = e->logits; c.ldo = d.vocab_size; c.x = e->h; c.ldx = H;
    if (head == Head::ALL) {
      MI_TRY(gemv_rows(e, hw, c, R, es, sizeof(float), "gemv_head"));
    } else if (head == Head::LAST) {      // the last position of every row, read in place
      const int L = groups[0].L;
      c.x = (char*)e->h + (size_t)(L - 1) * H * es; c.ldx = L * H;
      MI_TRY(gemv_rows(e, hw, c, groups[0].B, es, sizeof(float), "gemv_head"));
    } else {                              // the wanted positions -> compact rows -> head
      if (!e->d_gather) MI_HIP(hipMalloc(&e->d_gather, 4096 * sizeof(int32_t)));
      if (gather.size() > 4096) return fail(MI_ERR_INVALID, std::string(what) + ": too many sampled rows");
      MI_HIP(hipMemcpyAsync(e->d_gather, gather.data(), gather.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      MI_TRY(launch_gather_rows(e->h, (size_t)H * es, e->d_gather, (int)gather.size(), e->xn, st));
      c.x = e->xn;
      e->cur_L = 1;                       // the few sampled rows go through the decode step's head kernel
      const int rc_head = gemv_rows(e, hw, c, gather.size(), es, sizeof(float), "gemv_head");
      e->cur_L = cur_L;
      MI_TRY(rc_head);
    }
  }
  for (const AttnGroup& g : groups) MI_TRY(launch_advance_offsets(kv->d_off, d_rows_of(g), g.B, g.L, st));
  for (const AttnGroup& g : groups)
    for (int b = 0; b < g.B; ++b) kv->h_off[row_of(g, b)] += g.L;
  return MI_OK;
}

int check_call(mi_engine* e, mi_kv* kv, int B, int L) {
  if (!e || !kv) return fail(MI_ERR_INVALID, "null handle");
  if (!e->finalized) return fail(MI_ERR_INVALID, "engine not finalized");
  if (kv->e != e) return fail(MI_ERR_INVALID, "kv belongs to another engine");
  if (B != kv->B) return fail(MI_ERR_INVALID, "batch size mismatch (PagedKVCache batch size mismatch, base.py:125)");
  if (L < 1) return fail(MI_ERR_INVALID, "L must be >= 1");
  MI_HIP(hipSetDevice(e->device));
  return MI_OK;
}

int upload_tokens(mi_engine* e, const int32_t* tokens, int B, int L) {
  const size_t R = (size_t)B * L;
  for (size_t i = 0; i < R; ++i)
    if (tokens[i] < 0 || tokens[i] >= e->d.vocab_size) return fail(MI_ERR_INVALID, "token id out of range");
  MI_HIP(hipMemcpyAsync(e->d_tokens, tokens, R * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  return MI_OK;
}

// ABI guard (mi355_decode.h): a binding built against another layout of the struct is refused, never read
int check_params(const mi_sample_params* sp) {
  if (sp != nullptr && sp->struct_size != sizeof(mi_sample_params))
    return fail(MI_ERR_INVALID, "mi_sample_params.struct_size = " + std::to_string(sp->struct_size) + ", this library (ABI " +
                                    std::to_string(MI_ABI_VERSION) + ") expects " + std::to_string(sizeof(mi_sample_params)) +
                                    ": the binding was generated from another version of mi355_decode.h");
  return MI_OK;
}

// The ABI 4 controls of a sampling call over B rows, checked before anything is enqueued (mi_score_tokens ignores them)
int check_controls(const mi_sample_params* sp, int B) {
  if (!sp) return MI_OK;
  if (sp->top_k < 0) return fail(MI_ERR_INVALID, "mi_sample_params.top_k must be >= 0 (0 = off)");
  if (!(sp->min_p >= 0.f && sp->min_p <= 1.f)) return fail(MI_ERR_INVALID, "mi_sample_params.min_p must be in [0, 1] (0 = off)");
  if ((sp->row_seed != nullptr) != (sp->row_position != nullptr))
    return fail(MI_ERR_INVALID, "mi_sample_params.row_seed and row_position come together");
  for (int b = 0; b < B; ++b) {
    if (sp->row_top_k && sp->row_top_k[b] < 0)
      return fail(MI_ERR_INVALID, "mi_sample_params.row_top_k[" + std::to_string(b) + "] must be >= 0 (0 = off)");
    if (sp->row_min_p && !(sp->row_min_p[b] >= 0.f && sp->row_min_p[b] <= 1.f))
      return fail(MI_ERR_INVALID, "mi_sample_params.row_min_p[" + std::to_string(b) + "] must be in [0, 1] (0 = off)");
  }
  return MI_OK;
}

// kv: the cache whose per-row logit_bias table the sampled rows obey (null: none, mi_score_tokens); rb_map: device [B], the
// cache row of every sampled row, or null when sampled row b is cache row b
int run_sample(mi_engine* e, int B, const mi_sample_params* sp, const int32_t* forced = nullptr, const mi_kv* kv = nullptr,
               const int32_t* rb_map = nullptr) {
  mi_sample_params def{}; def.struct_size = sizeof(def); def.temperature = 0.f; def.top_p = 1.f; def.stream_position = -1;
  if (!sp) sp = &def;
  hipStream_t st = e->stream;
  if (sp->n_logit_bias > 0) {
    if (sp->n_logit_bias > 4096) return fail(MI_ERR_INVALID, "too many logit_bias entries");
    if (!e->d_bias_ids) { MI_HIP(hipMalloc(&e->d_bias_ids, 4096 * sizeof(int32_t))); MI_HIP(hipMalloc(&e->d_bias_vals, 4096 * sizeof(float))); }
    MI_HIP(hipMemcpyAsync(e->d_bias_ids, sp->logit_bias_ids, sp->n_logit_bias * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MI_HIP(hipMemcpyAsync(e->d_bias_vals, sp->logit_bias_values, sp->n_logit_bias * sizeof(float), hipMemcpyHostToDevice, st));
  }
  if (sp->uniforms && !forced) MI_HIP(hipMemcpyAsync(e->d_uniforms, sp->uniforms, B * sizeof(float), hipMemcpyHostToDevice, st));
  const bool per_row = sp->row_temperature != nullptr && sp->row_top_p != nullptr && !forced;
  if (per_row) {
    MI_TRY(grow(st, &e->d_rowpar, &e->d_rowpar_cap, 2 * (size_t)B * sizeof(float)));
    MI_HIP(hipMemcpyAsync(e->d_rowpar, sp->row_temperature, B * sizeof(float), hipMemcpyHostToDevice, st));
    MI_HIP(hipMemcpyAsync(e->d_rowpar + B, sp->row_top_p, B * sizeof(float), hipMemcpyHostToDevice, st));
  }
  const bool ext_rows = !forced && (sp->row_top_k || sp->row_min_p || sp->row_position);
  if (ext_rows) {                                           // like d_rowpar: [seed B | position B | top_k B | min_p B]
    MI_TRY(grow(st, &e->d_rowext, &e->d_rowext_cap, 24 * (size_t)B));
    char* base = e->d_rowext;
    if (sp->row_position) {
      MI_HIP(hipMemcpyAsync(base, sp->row_seed, B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      MI_HIP(hipMemcpyAsync(base + 8 * (size_t)B, sp->row_position, B * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    if (sp->row_top_k) MI_HIP(hipMemcpyAsync(base + 16 * (size_t)B, sp->row_top_k, B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (sp->row_min_p) MI_HIP(hipMemcpyAsync(base + 20 * (size_t)B, sp->row_min_p, B * sizeof(float), hipMemcpyHostToDevice, st));
  }
  Prof pr(e, "sample");
  SampleCall sc{};
  sc.logits = e->logits; sc.B = B; sc.V = e->d.vocab_size; sc.rnd = RND_NONE;
  sc.temperature = sp->temperature; sc.top_p = sp->top_p;
  sc.n_bias = sp->n_logit_bias; sc.bias_ids = e->d_bias_ids; sc.bias_vals = e->d_bias_vals;
  sc.forced = forced;
  sc.uniforms = (sp->uniforms && !forced) ? e->d_uniforms : nullptr; sc.seed = sp->seed; sc.step = sp->stream_position >= 0 ? (uint64_t)sp->stream_position : e->step_counter++;
  sc.top_logprobs = sp->top_logprobs;
  sc.lp_temp = sp->logprobs_at_temperature;
  sc.row_temp = per_row ? e->d_rowpar : nullptr;
  sc.row_top_p = per_row ? e->d_rowpar + B : nullptr;
  if (!forced) {                                            // teacher forcing samples nothing: the controls stay off
    sc.top_k = sp->top_k; sc.min_p = sp->min_p;
    if (sp->row_position) { sc.row_seed = (const uint64_t*)e->d_rowext; sc.row_position = (const int64_t*)(e->d_rowext + 8 * (size_t)B); }
    if (sp->row_top_k) sc.row_top_k = (const int32_t*)(e->d_rowext + 16 * (size_t)B);
    if (sp->row_min_p) sc.row_min_p = (const float*)(e->d_rowext + 20 * (size_t)B);
  }
  sc.tokens_out = e->d_next; sc.logprob_out = e->d_logprob; sc.prob_row0_out = forced ? nullptr : e->d_prob0;
  sc.topk_ids = e->d_topk_ids; sc.topk_logprobs = e->d_topk_lp; sc.row_stats = e->d_rowstats;
  if (kv && kv->rb_biased > 0 && !forced) {                 // (no biased row: the launch and the arguments of a cache without a table)
    sc.rb_cnt = kv->rb_cnt(); sc.rb_ids = kv->rb_ids(); sc.rb_vals = kv->rb_vals(); sc.rb_map = rb_map;
    sc.rb_rows = kv->B; sc.rb_cap = MI_MAX_ROW_LOGIT_BIAS;
  }
  if (kv && kv->lp_set > 0 && !forced) {                    // (no row setting: the launch, the arguments and the layout of before)
    sc.lp_k = kv->lp_k(); sc.lp_flag = kv->lp_flag(); sc.topk_stride = MI_MAX_TOP_LOGPROBS;
    sc.rb_map = rb_map; sc.rb_rows = kv->B;
  }
  return launch_sample(sc, st);
}

// The step's results -> a pinned slot (tokens | logprobs | row-0 probabilities: one copy, d_next and the slot's block
// share the layout), then the event mi_step_wait waits for.
// kv with a row logprobs setting: the top-k arrays have the fixed stride MI_MAX_TOP_LOGPROBS (mi_kv_set_row_logprobs)
int finish_step(mi_engine* e, int B, const mi_sample_params* sp, int64_t* ticket, const mi_kv* kv) {
  hipStream_t st = e->stream;
  const int64_t t = e->next_ticket++;
  Slot& s = e->slots[t % NSLOT];
  s.B = B; s.topk = (kv && kv->lp_set > 0) ? MI_MAX_TOP_LOGPROBS : sp ? sp->top_logprobs : 0; s.ticket = t;
  if (B > 0) {
    MI_HIP(hipMemcpyAsync(s.tokens, e->d_next, ((size_t)2 * e->maxB + B) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (s.topk > 0) {
      MI_HIP(hipMemcpyAsync(s.topk_ids, e->d_topk_ids, (size_t)B * s.topk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      MI_HIP(hipMemcpyAsync(s.topk_lp, e->d_topk_lp, (size_t)B * s.topk * sizeof(float), hipMemcpyDeviceToHost, st));
    }
  }
  MI_HIP(hipEventRecord(s.ev, st));
  *ticket = t;
  return MI_OK;
}

// mi_step_enqueue / mi_step_enqueue_rows once their arguments are checked: n rows x L tokens (rows null = rows 0..n-1),
// tokens_in null = the device-resident feed (the previous step's samples)
int step_enqueue(mi_engine* e, mi_kv* kv, const int32_t* rows, int n, const int32_t* tokens_in, int L,
                 const mi_sample_params* sp, int64_t* ticket) {
  MI_TRY(ensure_workspace(e, (size_t)n * L, (size_t)n, std::max(n, kv->B)));
  if (tokens_in) MI_TRY(upload_tokens(e, tokens_in, n, L));
  e->tok_src = tokens_in ? nullptr : e->d_next;            // (no copy: the sampler overwrites d_next only at the end of this step)
  const int frc = forward(e, kv, rows, {{0, n, L, 0}}, L, Head::LAST);
  e->tok_src = nullptr;
  MI_TRY(frc);
  MI_TRY(run_sample(e, n, sp, nullptr, kv, rows ? kv->d_rows : nullptr));   // (forward left the call's rows in d_rows)
  e->last_n = n;
  return finish_step(e, n, sp, ticket, kv);
}

}  // namespace

// =========================================================================================
extern "C" {

const char* mi_last_error(void) { return g_err.c_str(); }
const char* mi_version(void) { return "mi355_decode 0.2 (gfx950)"; }
int mi_abi_version(void) { return MI_ABI_VERSION; }

int mi_engine_create(const mi_model_desc* desc, int device, mi_engine** out) {
  if (!desc || !out) return fail(MI_ERR_INVALID, "null argument");
  if (desc->struct_size != sizeof(mi_model_desc))
    return fail(MI_ERR_INVALID, "mi_model_desc.struct_size = " + std::to_string(desc->struct_size) + ", this library (ABI " +
                                    std::to_string(MI_ABI_VERSION) + ") expects " + std::to_string(sizeof(mi_model_desc)));
  const mi_model_desc& d = *desc;
  if (d.arch != MI_ARCH_LLAMA && d.arch != MI_ARCH_QWEN3 && d.arch != MI_ARCH_PHI3 && d.arch != MI_ARCH_MIXTRAL)
    return fail(MI_ERR_UNSUPPORTED, "unsupported arch");
  if (d.arch == MI_ARCH_PHI3 && (d.attention_bias || d.mlp_bias || d.tie_word_embeddings))
    return fail(MI_ERR_INVALID, "arch phi3 has neither linear biases nor a tied lm_head (attention_bias, mlp_bias, tie_word_embeddings must be 0)");
  if (d.hidden_size <= 0 || d.num_layers <= 0 || d.num_heads <= 0 || d.num_kv_heads <= 0 || d.head_dim <= 0 ||
      d.intermediate_size <= 0 || d.vocab_size <= 0 || d.max_positions <= 0)
    return fail(MI_ERR_INVALID, "model dimensions must be positive");
  if (d.num_heads % d.num_kv_heads != 0) return fail(MI_ERR_INVALID, "num_heads must be a multiple of num_kv_heads");
  if (d.act_dtype != MI_F32 && d.act_dtype != MI_BF16 && d.act_dtype != MI_F16) return fail(MI_ERR_INVALID, "bad act_dtype");
  if (d.quant_bits != 0 && d.quant_bits != 4 && d.quant_bits != 8) return fail(MI_ERR_UNSUPPORTED, "quant_bits must be 0, 4 or 8");
  if (d.hidden_size % 8 || d.intermediate_size % 8 || (d.num_heads * d.head_dim) % 8)
    return fail(MI_ERR_UNSUPPORTED, "hidden / intermediate sizes must be multiples of 8");
  if (d.rope_traditional && d.arch == MI_ARCH_QWEN3)
    return fail(MI_ERR_UNSUPPORTED, "rope_traditional with arch qwen3 is not supported (q_norm / k_norm would need the same regrouping)");
  if (d.rope_traditional && d.head_dim % 2 != 0) return fail(MI_ERR_INVALID, "rope_traditional needs an even head_dim");
  if (d.arch == MI_ARCH_MIXTRAL) {      // mixtral.py: dense 16-bit checkpoints, E <= 16 experts, the best 1 or 2 per token
    if (d.attention_bias || d.mlp_bias || d.tie_word_embeddings)
      return fail(MI_ERR_INVALID, "arch mixtral has neither linear biases nor a tied lm_head (attention_bias, mlp_bias, tie_word_embeddings must be 0)");
    if (d.act_dtype == MI_F32) return fail(MI_ERR_UNSUPPORTED, "arch mixtral: act_dtype must be MI_BF16 or MI_F16 (float32 weights are not supported)");
    if (d.quant_bits != 0) return fail(MI_ERR_UNSUPPORTED, "arch mixtral: quant_bits must be 0 (quantised experts are not supported yet)");
    if (d.num_local_experts < 1 || d.num_local_experts > MOE_MAX_EXPERTS)
      return fail(MI_ERR_UNSUPPORTED, "arch mixtral: num_local_experts must be in [1, " + std::to_string(MOE_MAX_EXPERTS) + "]");
    if (d.num_experts_per_tok < 1 || d.num_experts_per_tok > 2 || d.num_experts_per_tok > d.num_local_experts)
      return fail(MI_ERR_UNSUPPORTED, "arch mixtral: num_experts_per_tok must be 1 or 2 and at most num_local_experts");
    if (d.hidden_size % 64 || d.intermediate_size % 64)
      return fail(MI_ERR_UNSUPPORTED, "arch mixtral: hidden_size and intermediate_size must be multiples of 64");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MI_ERR_RUNTIME, "no HIP device available (this library has no CPU backend)");
  if (device < 0 || device >= ndev) return fail(MI_ERR_INVALID, "bad device index");
  MI_HIP(hipSetDevice(device));
  mi_engine* e = new mi_engine();
  e->d = d; e->device = device;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return fail(MI_ERR_RUNTIME, "hipStreamCreate failed"); }
  e->layers.resize(d.num_layers);
  const int D = d.head_dim;
  for (auto& l : e->layers) {
    l.qkv.n_parts = 3; l.qkv.part_rows[0] = d.num_heads * D; l.qkv.part_rows[1] = d.num_kv_heads * D; l.qkv.part_rows[2] = d.num_kv_heads * D;
    l.o.n_parts = 1; l.o.part_rows[0] = d.hidden_size;
    l.gate_up.n_parts = 2; l.gate_up.part_rows[0] = d.intermediate_size; l.gate_up.part_rows[1] = d.intermediate_size;
    l.down.n_parts = 1; l.down.part_rows[0] = d.hidden_size;
    if (d.arch == MI_ARCH_MIXTRAL) for (auto& seen : l.moe_seen) seen.assign(d.num_local_experts, 0);
  }
  e->embed.n_parts = 1; e->embed.part_rows[0] = d.vocab_size;
  e->lm_head.n_parts = 1; e->lm_head.part_rows[0] = d.vocab_size;
  *out = e;
  return MI_OK;
}

void mi_engine_destroy(mi_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  for (auto& l : e->layers) {
    free_linear(l.qkv); free_linear(l.o); free_linear(l.gate_up); free_linear(l.down);
    hipFree(l.in_norm); hipFree(l.post_norm); hipFree(l.q_norm); hipFree(l.k_norm);
    hipFree(l.in_norm32); hipFree(l.post_norm32); hipFree(l.q_norm32); hipFree(l.k_norm32);
    hipFree(l.moe_router); for (void* w : l.moe_w) hipFree(w);
  }
  hipFree(e->final_norm32); hipFree(e->xn); hipFree(e->xs); hipFree(e->gk_ws);
  free_linear(e->embed); free_linear(e->lm_head);
  hipFree(e->final_norm); hipFree(e->cos_tab); hipFree(e->sin_tab);
  hipFree(e->h); hipFree(e->qkv); hipFree(e->q); hipFree(e->attn); hipFree(e->act); hipFree(e->logits); hipFree(e->gu); hipFree(e->d_forced); hipFree(e->d_gather);
  hipFree(e->d_rowpar); hipFree(e->d_rowext); hipFree(e->deq_scratch);
  hipFree(e->d_row_adapter); hipFree(e->lora_rt); hipFree(e->ys); hipFree(e->moe_ws);
  hipFree(e->sk_ws); hipFree(e->sk_ctr); hipFree(e->d_sq); hipFree(e->cc_pub);
  hipFree(e->d_tokens); hipFree(e->d_next); hipFree(e->d_rowstats);
  hipFree(e->d_uniforms); hipFree(e->d_topk_ids); hipFree(e->d_topk_lp); hipFree(e->d_bias_ids); hipFree(e->d_bias_vals);
  for (auto& s : e->slots) {
    hipHostFree(s.tokens); hipHostFree(s.topk_ids); hipHostFree(s.topk_lp);
    if (s.ev) hipEventDestroy(s.ev);
  }
  for (auto& p : e->prof_events) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
  hipStreamDestroy(e->stream);
  delete e;
}

// ---- forward / sampling --------------------------------------------------------------------
int mi_forward(mi_engine* e, mi_kv* kv, const int32_t* tokens, int B, int L, float* logits_out, int all_pos) {
  MI_TRY(check_call(e, kv, B, L));
  if (!tokens) return fail(MI_ERR_INVALID, "null tokens");
  const size_t R = (size_t)B * L;
  MI_TRY(ensure_workspace(e, R, all_pos ? R : (size_t)B, B));
  MI_TRY(upload_tokens(e, tokens, B, L));
  MI_TRY(forward(e, kv, nullptr, {{0, B, L, 0}}, L, !logits_out ? Head::NONE : all_pos ? Head::ALL : Head::LAST));
  if (logits_out)
    MI_HIP(hipMemcpyAsync(logits_out, e->logits, (all_pos ? R : (size_t)B) * e->d.vocab_size * sizeof(float),
                          hipMemcpyDeviceToHost, e->stream));
  MI_HIP(hipStreamSynchronize(e->stream));
  return MI_OK;
}

int mi_score_tokens(mi_engine* e, mi_kv* kv, const int32_t* tokens, const int32_t* targets, int B, int L,
                    const mi_sample_params* sp, float* logprob_out, int32_t* topk_ids, float* topk_logprobs) {
  MI_TRY(check_params(sp));
  MI_TRY(check_call(e, kv, B, L));
  if (!tokens || !targets || !logprob_out) return fail(MI_ERR_INVALID, "null argument");
  const size_t R = (size_t)B * L;
  if (R > (size_t)(1 << 20)) return fail(MI_ERR_INVALID, "score: too many positions in one call");
  const int k = sp ? sp->top_logprobs : 0;
  if (k > 0 && (!topk_ids || !topk_logprobs)) return fail(MI_ERR_INVALID, "score: top_logprobs > 0 needs output buffers");
  MI_TRY(ensure_workspace(e, R, R, (int)R));
  hipStream_t st = e->stream;
  MI_TRY(grow(st, &e->d_forced, &e->d_forced_cap, R * sizeof(int32_t)));
  MI_TRY(upload_tokens(e, tokens, B, L));
  MI_HIP(hipMemcpyAsync(e->d_forced, targets, R * sizeof(int32_t), hipMemcpyHostToDevice, st));
  MI_TRY(forward(e, kv, nullptr, {{0, B, L, 0}}, L, Head::ALL));
  MI_TRY(run_sample(e, (int)R, sp, e->d_forced));
  MI_HIP(hipMemcpyAsync(logprob_out, e->d_logprob, R * sizeof(float), hipMemcpyDeviceToHost, st));
  if (k > 0) {
    MI_HIP(hipMemcpyAsync(topk_ids, e->d_topk_ids, R * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MI_HIP(hipMemcpyAsync(topk_logprobs, e->d_topk_lp, R * k * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  MI_HIP(hipStreamSynchronize(st));
  return MI_OK;
}

int mi_step_enqueue(mi_engine* e, mi_kv* kv, const int32_t* tokens_in, int B, int L, const mi_sample_params* sp,
                    int64_t* ticket) {
  MI_TRY(check_params(sp));
  MI_TRY(check_call(e, kv, B, L));
  if (!ticket) return fail(MI_ERR_INVALID, "null ticket");
  if (!tokens_in && L != 1) return fail(MI_ERR_INVALID, "device-resident token feed needs L == 1");
  if (!tokens_in && e->maxB < B) return fail(MI_ERR_INVALID, "no previous step to take tokens from");
  MI_TRY(check_controls(sp, B));
  return step_enqueue(e, kv, nullptr, B, tokens_in, L, sp, ticket);
}

int mi_step_enqueue_rows(mi_engine* e, mi_kv* kv, const int32_t* rows, int n, const int32_t* tokens_in, int L,
                         const mi_sample_params* sp, int64_t* ticket) {
  if (!e || !kv || !rows) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(check_params(sp));
  if (n < 1 || n > kv->B) return fail(MI_ERR_INVALID, "mi_step_enqueue_rows: n must be in [1, batch of the kv]");
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= kv->B) return fail(MI_ERR_INVALID, "mi_step_enqueue_rows: row out of range");
    for (int j = 0; j < i; ++j) if (rows[j] == rows[i]) return fail(MI_ERR_INVALID, "mi_step_enqueue_rows: duplicate row");
  }
  MI_TRY(check_call(e, kv, kv->B, L));
  if (!ticket) return fail(MI_ERR_INVALID, "null ticket");
  if (!tokens_in && L != 1) return fail(MI_ERR_INVALID, "device-resident token feed needs L == 1");
  if (!tokens_in && e->last_n != n) return fail(MI_ERR_INVALID, "device-resident token feed needs the row set of the previous step");
  MI_TRY(check_controls(sp, n));
  return step_enqueue(e, kv, rows, n, tokens_in, L, sp, ticket);
}

// One pass over the weights for rows that advance by DIFFERENT numbers of tokens (chunked prefill co-scheduled with the
// live decode rows): segment i = lens[i] tokens of cache row rows[i].  The decode rows (lens == 1) come first in the
// token buffer and form one attention group; every longer segment is a group of its own.  Logits are produced for the
// last token of the segments with want[i] != 0, in segment order.
int mi_step_enqueue_mixed(mi_engine* e, mi_kv* kv, const int32_t* rows, const int32_t* lens, const int32_t* want, int n,
                          const int32_t* tokens, const mi_sample_params* sp, int64_t* ticket) {
  if (!e || !kv || !rows || !lens || !want || !tokens) return fail(MI_ERR_INVALID, "null argument");
  MI_TRY(check_params(sp));
  if (n < 1 || n > kv->B) return fail(MI_ERR_INVALID, "mi_step_enqueue_mixed: n must be in [1, batch of the kv]");
  size_t R = 0; int n_out = 0;
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= kv->B) return fail(MI_ERR_INVALID, "mi_step_enqueue_mixed: row out of range");
    for (int j = 0; j < i; ++j) if (rows[j] == rows[i]) return fail(MI_ERR_INVALID, "mi_step_enqueue_mixed: duplicate row");
    if (lens[i] < 1) return fail(MI_ERR_INVALID, "mi_step_enqueue_mixed: every segment needs at least one token");
    R += (size_t)lens[i]; n_out += want[i] ? 1 : 0;
  }
  MI_TRY(check_call(e, kv, kv->B, 1));
  if (!ticket) return fail(MI_ERR_INVALID, "null ticket");
  if (sp && (sp->row_temperature != nullptr) != (sp->row_top_p != nullptr)) return fail(MI_ERR_INVALID, "row_temperature and row_top_p come together");
  MI_TRY(check_controls(sp, n_out));
  MI_TRY(ensure_workspace(e, R, (size_t)std::max(n_out, 1), std::max(n, kv->B)));
  for (size_t i = 0; i < R; ++i)
    if (tokens[i] < 0 || tokens[i] >= e->d.vocab_size) return fail(MI_ERR_INVALID, "token id out of range");
  MI_HIP(hipMemcpyAsync(e->d_tokens, tokens, R * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  int nd = 0;                                    // decode rows: the leading segments of length 1
  while (nd < n && lens[nd] == 1) ++nd;
  std::vector<AttnGroup> groups;
  std::vector<int32_t> gather;                   // token positions whose hidden state feeds the head
  if (nd > 0) groups.push_back({0, nd, 1, 0});
  size_t tok0 = 0;
  for (int i = 0; i < n; ++i) {
    if (i >= nd) {
      if (lens[i] == 1) return fail(MI_ERR_INVALID, "mixed step: one-token segments must come first");
      groups.push_back({i, 1, lens[i], tok0});
    }
    if (want[i]) gather.push_back((int32_t)(tok0 + lens[i] - 1));
    tok0 += (size_t)lens[i];
  }
  // Only decode rows: the decode step's kernels.  Otherwise the call is routed like a prefill of R rows (gemv_rows: the
  // weight-streaming kernel for short calls, the K-split 128 x 128 tile for a few hundred rows, plain tiles above).
  MI_TRY(forward(e, kv, rows, groups, R == (size_t)nd ? 1 : 2, n_out > 0 ? Head::GATHER : Head::NONE, gather, "mixed step"));
  if (n_out > 0) {
    const int32_t* rb_map = nullptr;
    if (kv->rb_biased > 0 || kv->lp_set > 0) {   // sampled row i = the i-th wanted segment: its cache row
      std::vector<int32_t> wanted;
      for (int i = 0; i < n; ++i) if (want[i]) wanted.push_back(rows[i]);
      rb_map = kv->rb_biased > 0 ? kv->rb_map() : kv->lp_map();
      MI_HIP(hipMemcpyAsync((void*)rb_map, wanted.data(), wanted.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    }
    MI_TRY(run_sample(e, n_out, sp, nullptr, kv, rb_map));
  }
  e->last_n = -1;                                // the device-resident token feed does not survive a mixed step
  return finish_step(e, n_out, sp, ticket, n_out > 0 ? kv : nullptr);
}

int mi_step_wait(mi_engine* e, int64_t ticket, int32_t* tokens_out, float* logprob_out, float* prob_row0_out,
                 int32_t* topk_ids, float* topk_logprobs) {
  if (!e) return fail(MI_ERR_INVALID, "null engine");
  if (ticket < 0 || ticket >= e->next_ticket) return fail(MI_ERR_INVALID, "unknown ticket");
  Slot& s = e->slots[ticket % NSLOT];
  if (s.ticket != ticket) return fail(MI_ERR_INVALID, "ticket expired (more than 4 steps in flight)");
  MI_HIP(hipSetDevice(e->device));
  MI_HIP(hipEventSynchronize(s.ev));
  if (tokens_out) memcpy(tokens_out, s.tokens, s.B * sizeof(int32_t));
  if (logprob_out) memcpy(logprob_out, s.logprob, s.B * sizeof(float));
  if (prob_row0_out) memcpy(prob_row0_out, s.prob0, s.B * sizeof(float));
  if (topk_ids && s.topk > 0) memcpy(topk_ids, s.topk_ids, (size_t)s.B * s.topk * sizeof(int32_t));
  if (topk_logprobs && s.topk > 0) memcpy(topk_logprobs, s.topk_lp, (size_t)s.B * s.topk * sizeof(float));
  return MI_OK;
}

int mi_decode_sample(mi_engine* e, mi_kv* kv, const int32_t* tokens_in, int B, int L, const mi_sample_params* sp,
                     int32_t* tokens_out, float* logprob_out, float* prob_row0_out, int32_t* topk_ids,
                     float* topk_logprobs) {
  int64_t t = -1;
  MI_TRY(mi_step_enqueue(e, kv, tokens_in, B, L, sp, &t));
  return mi_step_wait(e, t, tokens_out, logprob_out, prob_row0_out, topk_ids, topk_logprobs);
}

// ---- measurement hooks ----------------------------------------------------------------------
int mi_profile_select(mi_engine* e, const char* name) {
  if (!e) return fail(MI_ERR_INVALID, "null engine");
  hipStreamSynchronize(e->stream);
  for (auto& p : e->prof_events) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
  e->prof_events.clear();
  e->prof_name = name ? name : "";
  return MI_OK;
}

int mi_profile_read(mi_engine* e, int64_t* n_launches, double* total_ms) {
  if (!e || !n_launches || !total_ms) return fail(MI_ERR_INVALID, "null argument");
  MI_HIP(hipStreamSynchronize(e->stream));
  double tot = 0.0;
  for (auto& p : e->prof_events) {
    float ms = 0.f;
    MI_HIP(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
    hipEventDestroy(p.first); hipEventDestroy(p.second);
  }
  *n_launches = (int64_t)e->prof_events.size();
  *total_ms = tot;
  e->prof_events.clear();
  return MI_OK;
}

int mi_engine_set_option(mi_engine* e, const char* key, int64_t value) {
  if (!e || !key) return fail(MI_ERR_INVALID, "null argument");
  const std::string k(key);
  if (k == "force_generic_gemv") { e->opt_force_v1 = value != 0; return MI_OK; }
  if (k == "fused_decode_attention") { e->opt_fused_attn = value != 0; return MI_OK; }
  if (k == "prefill_gemm") { e->opt_prefill_gemm = value != 0; return MI_OK; }
  if (k == "skinny_gemm") { e->opt_skinny_gemm = value != 0; return MI_OK; }
  if (k == "norm_handover") { e->opt_norm_handover = value != 0; return MI_OK; }
  if (k == "consumer_combine") { if (value != 0 && value != 1) return fail(MI_ERR_INVALID, "consumer_combine: 0 or 1"); e->opt_consumer_combine = (int)value; return MI_OK; }
  if (k == "resident_x") { if (value != 0 && value != 1) return fail(MI_ERR_INVALID, "resident_x: 0 or 1"); e->opt_resident_x = (int)value; return MI_OK; }
  if (k == "consumer_combine_guard") return check_cc_guards(e, (e->d.num_heads + 2 * e->d.num_kv_heads) * e->d.head_dim);   // (a check, not a setting)
  if (k == "defer_norm") { e->opt_defer_norm = value != 0; return MI_OK; }
  if (k == "prefill_x_terms") { if (value != 2 && value != 3) return fail(MI_ERR_INVALID, "prefill_x_terms: 2 or 3"); e->opt_prefill_x_terms = (int)value; return MI_OK; }
  if (k == "short_prefill_skinny") { e->opt_short_prefill_skinny = value != 0; return MI_OK; }
  if (k == "decode_attention_mfma") { e->opt_attn_mfma = value != 0; return MI_OK; }
  if (k == "f16_hilo") { e->opt_f16_hilo = value != 0; return MI_OK; }
  if (k == "gate_up_interleave") { e->opt_gu8 = value != 0; return MI_OK; }
  if (k == "tile_weights") {
    if (e->finalized) return fail(MI_ERR_INVALID, "tile_weights must be set before mi_engine_finalize");
    e->opt_tile_weights = value != 0; return MI_OK;
  }
  return fail(MI_ERR_NOTFOUND, "unknown option: " + k);
}

int mi_engine_sync(mi_engine* e) {
  if (!e) return fail(MI_ERR_INVALID, "null engine");
  MI_HIP(hipSetDevice(e->device));
  MI_HIP(hipStreamSynchronize(e->stream));
  return MI_OK;
}

}  // extern "C"
