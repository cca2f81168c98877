// engine_load.hip -- a checkpoint's tensors and LoRA factors into an engine, and mi_engine_finalize: the fused matrices are
// checked, regrouped (rope_traditional), repacked tile-major and given their persistent second copies.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine_impl.h"

using namespace mi;

namespace {

int kind_of(const FusedLinear& f, int bits) {
  if (!f.quant) return f.dense_dtype == MI_F32 ? WK_F32 : (f.dense_dtype == MI_BF16 ? WK_BF16 : WK_F16);
  const int base = bits == 8 ? WK_Q8_F32 : WK_Q4_F32;
  return base + (f.scale_dtype == MI_F32 ? 0 : (f.scale_dtype == MI_BF16 ? 1 : 2));
}

int copy_in(void* dst, const void* src, size_t bytes, int on_device, hipStream_t st) {
  MI_HIP(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  MI_HIP(hipStreamSynchronize(st));
  return MI_OK;
}

// sub-tensor `part` of a fused linear: kind 0 = weight, 1 = scales, 2 = biases
int set_linear(mi_engine* e, FusedLinear& f, int part, int K, int kind, const void* data, const int64_t* shape,
               int ndim, int dtype, int on_device, const std::string& name) {
  const mi_model_desc& d = e->d;
  if (ndim != 2) return fail(MI_ERR_INVALID, name + ": expected a 2-D tensor");
  const int rows = f.part_rows[part];
  int total = 0, row0 = 0;
  for (int i = 0; i < f.n_parts; ++i) { if (i < part) row0 += f.part_rows[i]; total += f.part_rows[i]; }
  if (shape[0] != rows) return fail(MI_ERR_INVALID, name + ": wrong number of rows");
  if (kind == 0) {
    const bool packed = dtype == MI_U32;
    if (packed && d.quant_bits == 0) return fail(MI_ERR_INVALID, name + ": packed weights but desc.quant_bits == 0");
    const int64_t cols = packed ? (int64_t)K * d.quant_bits / 32 : K;
    if (shape[1] != cols) return fail(MI_ERR_INVALID, name + ": wrong number of columns");
    if (!packed && dtype != d.act_dtype)
      return fail(MI_ERR_UNSUPPORTED, name + ": dense weight dtype differs from the model dtype");
    if (f.w != nullptr && f.quant != packed) return fail(MI_ERR_UNSUPPORTED, name + ": fused parts mix dense and quantised weights");
    const size_t row_bytes = (size_t)cols * dtype_size(dtype);
    if (f.w == nullptr) {
      f.quant = packed; f.dense_dtype = packed ? -1 : dtype; f.w_bytes = row_bytes * total;
      MI_HIP(hipMalloc(&f.w, f.w_bytes));
    }
    MI_TRY(copy_in((char*)f.w + (size_t)row0 * row_bytes, data, row_bytes * rows, on_device, e->stream));
    f.seen_w[part] = 1;
  } else {
    if (d.quant_bits == 0) return fail(MI_ERR_INVALID, name + ": scales/biases but desc.quant_bits == 0");
    if (K % d.quant_group_size != 0) return fail(MI_ERR_INVALID, name + ": K not divisible by the group size");
    const int64_t cols = K / d.quant_group_size;
    if (shape[1] != cols) return fail(MI_ERR_INVALID, name + ": wrong number of groups");
    if (dtype != MI_F32 && dtype != MI_BF16 && dtype != MI_F16) return fail(MI_ERR_INVALID, name + ": bad dtype");
    if (f.scale_dtype >= 0 && f.scale_dtype != dtype) return fail(MI_ERR_UNSUPPORTED, name + ": mixed scale dtypes");
    f.scale_dtype = dtype;
    const size_t row_bytes = (size_t)cols * dtype_size(dtype);
    void*& dst = kind == 1 ? f.scales : f.biases;
    if (dst == nullptr) { f.s_bytes = row_bytes * total; MI_HIP(hipMalloc(&dst, f.s_bytes)); }
    MI_TRY(copy_in((char*)dst + (size_t)row0 * row_bytes, data, row_bytes * rows, on_device, e->stream));
    (kind == 1 ? f.seen_s : f.seen_b)[part] = 1;
  }
  return MI_OK;
}

// MI_ARCH_PHI3: a checkpoint's fused matrix (phi3.py: qkv_proj = q, then k, then v along the rows; gate_up_proj = gate, then
// up) stored as the parts of f.  Dense rows, or the rows of codes / scales / quantisation biases: groups run along K, so
// whole rows move.
int set_linear_fused(mi_engine* e, FusedLinear& f, int K, int kind, const void* data, const int64_t* shape,
                     int ndim, int dtype, int on_device, const std::string& name) {
  if (ndim != 2) return fail(MI_ERR_INVALID, name + ": expected a 2-D tensor");
  int total = 0;
  for (int i = 0; i < f.n_parts; ++i) total += f.part_rows[i];
  if (shape[0] != total) return fail(MI_ERR_INVALID, name + ": wrong number of rows (the fused matrix has " + std::to_string(total) + ")");
  if (shape[1] <= 0 || dtype_size(dtype) == 0) return fail(MI_ERR_INVALID, name + ": bad shape or dtype");
  const size_t row_bytes = (size_t)shape[1] * dtype_size(dtype);
  size_t row0 = 0;
  for (int i = 0; i < f.n_parts; ++i) {
    const int64_t sub[2] = {f.part_rows[i], shape[1]};
    MI_TRY(set_linear(e, f, i, K, kind, (const char*)data + row0 * row_bytes, sub, 2, dtype, on_device, name));
    row0 += f.part_rows[i];
  }
  return MI_OK;
}

int set_vector(mi_engine* e, void*& dst, int n, const void* data, const int64_t* shape, int ndim, int dtype,
               int on_device, const std::string& name) {
  if (ndim != 1 || shape[0] != n) return fail(MI_ERR_INVALID, name + ": wrong shape");
  if (dtype != e->d.act_dtype) return fail(MI_ERR_UNSUPPORTED, name + ": norm weight dtype differs from the model dtype");
  if (dst == nullptr) MI_HIP(hipMalloc(&dst, (size_t)n * dtype_size(dtype)));
  return copy_in(dst, data, (size_t)n * dtype_size(dtype), on_device, e->stream);
}

// `<proj>.bias` of part `part` (1-D, the part's rows; float32 or a 16-bit float) -> float32 at the part's rows of f.bias
int set_bias(mi_engine* e, FusedLinear& f, int part, const void* data, const int64_t* shape, int ndim, int dtype,
             int on_device, const std::string& name) {
  const int rows = f.part_rows[part];
  int total = 0, row0 = 0;
  for (int i = 0; i < f.n_parts; ++i) { if (i < part) row0 += f.part_rows[i]; total += f.part_rows[i]; }
  if (ndim != 1 || shape[0] != rows) return fail(MI_ERR_INVALID, name + ": wrong shape");
  if (dtype != MI_F32 && dtype != MI_BF16 && dtype != MI_F16) return fail(MI_ERR_INVALID, name + ": bad dtype");
  if (f.bias == nullptr) MI_HIP(hipMalloc(&f.bias, (size_t)total * sizeof(float)));
  if (dtype == MI_F32) {
    MI_TRY(copy_in(f.bias + row0, data, (size_t)rows * sizeof(float), on_device, e->stream));
  } else {
    void* tmp = nullptr;
    MI_HIP(hipMalloc(&tmp, (size_t)rows * dtype_size(dtype)));
    int rc = copy_in(tmp, data, (size_t)rows * dtype_size(dtype), on_device, e->stream);
    if (rc == MI_OK) rc = launch_convert(tmp, dtype, f.bias + row0, MI_F32, (size_t)rows, e->stream);
    if (rc == MI_OK && hipStreamSynchronize(e->stream) != hipSuccess) rc = fail(MI_ERR_RUNTIME, name + ": converting the bias failed");
    hipFree(tmp);
    MI_TRY(rc);
  }
  f.seen_bias[part] = 1;
  return MI_OK;
}

// rope_traditional: the first `nrows` rows (whole heads of D) of a row-major device array regrouped in place (kernels.h)
int head_perm_inplace(mi_engine* e, void* buf, size_t nrows, int D, size_t row_bytes) {
  if (buf == nullptr || nrows == 0 || row_bytes == 0) return MI_OK;
  void* tmp = nullptr;
  MI_HIP(hipMalloc(&tmp, nrows * row_bytes));
  int rc = launch_head_perm_rows(buf, tmp, nrows, D, row_bytes, e->stream);
  if (rc == MI_OK && (hipMemcpyAsync(buf, tmp, nrows * row_bytes, hipMemcpyDeviceToDevice, e->stream) != hipSuccess ||
                      hipStreamSynchronize(e->stream) != hipSuccess))
    rc = fail(MI_ERR_RUNTIME, "regrouping the q / k rows for rope_traditional failed");
  hipFree(tmp);
  return rc;
}

// the q and k parts of a q|k|v matrix as loaded (row-major, before the tile-major repack): codes, scales, quantisation
// biases and linear biases.  Quantisation groups run along K, so whole rows move.
int permute_qk_heads(mi_engine* e, FusedLinear& f) {
  int total = 0;
  if (f.qk_regrouped || f.W.layout == 1) return MI_OK;
  for (int i = 0; i < f.n_parts; ++i) { total += f.part_rows[i]; if (!f.seen_w[i]) return MI_OK; }   // (finalize_linear reports it)
  const size_t nrows = (size_t)f.part_rows[0] + f.part_rows[1];
  const int D = e->d.head_dim;
  MI_TRY(head_perm_inplace(e, f.w, nrows, D, f.w_bytes / total));
  if (f.quant && f.scales != nullptr && f.biases != nullptr) {
    MI_TRY(head_perm_inplace(e, f.scales, nrows, D, f.s_bytes / total));
    MI_TRY(head_perm_inplace(e, f.biases, nrows, D, f.s_bytes / total));
  }
  if (f.bias != nullptr && f.seen_bias[0] && f.seen_bias[1]) MI_TRY(head_perm_inplace(e, f.bias, nrows, D, sizeof(float)));
  f.qk_regrouped = true;
  return MI_OK;
}

int finalize_linear(mi_engine* e, FusedLinear& f, int K, const std::string& name) {
  int total = 0;
  for (int i = 0; i < f.n_parts; ++i) {
    total += f.part_rows[i];
    if (!f.seen_w[i]) return fail(MI_ERR_NOTFOUND, name + ": weight not set");
    if (f.quant && (!f.seen_s[i] || !f.seen_b[i])) return fail(MI_ERR_NOTFOUND, name + ": scales/biases not set");
  }
  if (f.quant && f.scale_dtype != e->d.act_dtype)
    return fail(MI_ERR_UNSUPPORTED, name + ": scale dtype differs from the model dtype");
  f.W.wk = kind_of(f, e->d.quant_bits);
  f.W.w = f.w; f.W.scales = f.scales; f.W.biases = f.biases;
  f.W.N = total; f.W.K = K; f.W.group = e->d.quant_group_size > 0 ? e->d.quant_group_size : 64;
  f.W.bias = f.bias;
  // "repack weights": tile-major layout for the matrices the streaming kernels read (repack.hip)
  if (e->opt_tile_weights && tiled_supported(f.W.wk, f.W.N, f.W.K, f.W.group)) {
    void* dst = nullptr;
    if (hipMalloc(&dst, tiled_bytes(f.W.wk, f.W.N, f.W.K)) != hipSuccess)
      return fail(MI_ERR_RUNTIME, name + ": out of device memory repacking weights");
    MI_TRY(launch_repack_tiled(f.W, dst, e->stream));
    MI_HIP(hipStreamSynchronize(e->stream));
    hipFree(f.w); hipFree(f.scales); hipFree(f.biases);
    f.w = dst; f.scales = nullptr; f.biases = nullptr;
    f.W.w = dst; f.W.scales = nullptr; f.W.biases = nullptr; f.W.layout = 1;
  }
  return MI_OK;
}

int make_f32_copy(mi_engine* e, const void* src, int n, void** dst) {
  if (src == nullptr) { *dst = nullptr; return MI_OK; }
  if (e->d.act_dtype == MI_F32) { *dst = nullptr; return MI_OK; }
  MI_HIP(hipMalloc(dst, (size_t)n * sizeof(float)));
  return launch_convert(src, e->d.act_dtype, *dst, MI_F32, (size_t)n, e->stream);
}

// one of the seven linears of a block by its checkpoint name: the fused matrix, the part of it, its K, attention or MLP.
// MI_ARCH_PHI3 names q|k|v and gate|up as one linear each (part -1: every part of f); the split names are unknown there.
struct Proj { FusedLinear* f; int part, K; bool attn; };
bool find_proj(const mi_model_desc& d, LayerW& l, const std::string& sub, Proj* p) {
  const int H = d.hidden_size, QD = d.num_heads * d.head_dim;
  if (d.arch == MI_ARCH_PHI3) {
    if (sub == "self_attn.qkv_proj") *p = {&l.qkv, -1, H, true};
    else if (sub == "mlp.gate_up_proj") *p = {&l.gate_up, -1, H, false};
    else if (sub == "self_attn.o_proj") *p = {&l.o, 0, QD, true};
    else if (sub == "mlp.down_proj") *p = {&l.down, 0, d.intermediate_size, false};
    else return false;
    return true;
  }
  if (d.arch == MI_ARCH_MIXTRAL && sub.compare(0, 4, "mlp.") == 0) return false;        // (its MLP is block_sparse_moe: set_moe_tensor)
  if (sub == "self_attn.q_proj") *p = {&l.qkv, 0, H, true};
  else if (sub == "self_attn.k_proj") *p = {&l.qkv, 1, H, true};
  else if (sub == "self_attn.v_proj") *p = {&l.qkv, 2, H, true};
  else if (sub == "self_attn.o_proj") *p = {&l.o, 0, QD, true};
  else if (sub == "mlp.gate_proj") *p = {&l.gate_up, 0, H, false};
  else if (sub == "mlp.up_proj") *p = {&l.gate_up, 1, H, false};
  else if (sub == "mlp.down_proj") *p = {&l.down, 0, d.intermediate_size, false};
  else return false;
  return true;
}

// MI_ARCH_MIXTRAL: `sub` = "block_sparse_moe.<rest>" of block l.  gate: the router [E][H]; switch_mlp.{gate,up,down}_proj: all
// experts stacked, 3-D; experts.<e>.{w1,w3,w2}: one expert, 2-D, into slot e (w1 = gate, w3 = up, w2 = down: mixtral.py:203).
int set_moe_tensor(mi_engine* e, LayerW& l, const std::string& rest, int kind, const void* data, const int64_t* shape, int ndim,
                   int dtype, int on_device, const std::string& name) {
  const mi_model_desc& d = e->d;
  const int64_t E = d.num_local_experts, H = d.hidden_size, I = d.intermediate_size;
  if (kind == 1 || kind == 2) return fail(MI_ERR_UNSUPPORTED, name + ": quantised experts are not supported");
  if (kind != 0) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
  if (dtype != d.act_dtype) return fail(MI_ERR_UNSUPPORTED, name + ": dense weight dtype differs from the model dtype");
  const size_t es = dtype_size(dtype);
  if (rest == "gate") {
    if (ndim != 2 || shape[0] != E || shape[1] != H) return fail(MI_ERR_INVALID, name + ": expected shape [num_local_experts][hidden_size]");
    if (l.moe_router == nullptr) MI_HIP(hipMalloc(&l.moe_router, (size_t)(E * H) * es));
    return copy_in(l.moe_router, data, (size_t)(E * H) * es, on_device, e->stream);
  }
  int t = -1; int64_t slot = -1;                  // tensor (0 gate, 1 up, 2 down); expert slot, -1 = the stacked form
  if (rest == "switch_mlp.gate_proj") t = 0;
  else if (rest == "switch_mlp.up_proj") t = 1;
  else if (rest == "switch_mlp.down_proj") t = 2;
  else if (rest.compare(0, 8, "experts.") == 0) {
    const size_t dot = rest.find('.', 8);
    if (dot == std::string::npos) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
    const std::string idx = rest.substr(8, dot - 8), w = rest.substr(dot + 1);
    if (idx.empty() || idx.size() > 4 || idx.find_first_not_of("0123456789") != std::string::npos) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
    slot = std::stoi(idx);
    t = w == "w1" ? 0 : w == "w3" ? 1 : w == "w2" ? 2 : -1;
    if (t >= 0 && slot >= E) return fail(MI_ERR_NOTFOUND, "expert index out of range: " + name);
  }
  if (t < 0) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
  const int64_t rows = t == 2 ? H : I, cols = t == 2 ? I : H;
  const size_t one = (size_t)(rows * cols) * es;
  if (slot < 0) {
    if (ndim != 3 || shape[0] != E || shape[1] != rows || shape[2] != cols)
      return fail(MI_ERR_INVALID, name + ": expected shape [" + std::to_string(E) + "][" + std::to_string(rows) + "][" + std::to_string(cols) + "]");
  } else if (ndim != 2 || shape[0] != rows || shape[1] != cols) {
    return fail(MI_ERR_INVALID, name + ": expected shape [" + std::to_string(rows) + "][" + std::to_string(cols) + "]");
  }
  if (l.moe_w[t] == nullptr) MI_HIP(hipMalloc(&l.moe_w[t], one * (size_t)E));
  if (slot < 0) {
    MI_TRY(copy_in(l.moe_w[t], data, one * (size_t)E, on_device, e->stream));
    std::fill(l.moe_seen[t].begin(), l.moe_seen[t].end(), 1);
  } else {
    MI_TRY(copy_in((char*)l.moe_w[t] + one * (size_t)slot, data, one, on_device, e->stream));
    l.moe_seen[t][slot] = 1;
  }
  return MI_OK;
}

}  // namespace

void mi::free_linear(FusedLinear& f) {
  hipFree(f.w); hipFree(f.scales); hipFree(f.biases); hipFree(f.w_hilo); hipFree(f.w_gu8); hipFree(f.bias);
  if (f.adapters != nullptr) {
    for (auto& part : f.adapters->h)
      for (AdapterPart& ap : part) { hipFree(const_cast<float*>(ap.a)); hipFree(const_cast<float*>(ap.b)); hipFree(const_cast<float*>(ap.gain)); }
    hipFree(f.adapters->d);
    delete f.adapters;
    f.adapters = nullptr;
  }
}

extern "C" {

int mi_engine_set_tensor(mi_engine* e, const char* name_c, const void* data, const int64_t* shape, int ndim,
                         int dtype, int on_device) {
  if (!e || !name_c || !data || !shape) return fail(MI_ERR_INVALID, "null argument");
  if (e->finalized) return fail(MI_ERR_INVALID, "engine already finalized");
  MI_HIP(hipSetDevice(e->device));
  const mi_model_desc& d = e->d;
  std::string name(name_c);
  int kind = -1;
  std::string base;
  auto strip = [&](const char* suf, int k) {
    const size_t n = strlen(suf);
    if (name.size() > n && name.compare(name.size() - n, n, suf) == 0) { base = name.substr(0, name.size() - n); kind = k; }
  };
  strip(".weight", 0); strip(".scales", 1); strip(".biases", 2); strip(".bias", 3);    // (".biases" does not end in ".bias")
  if (kind < 0) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
  const int H = d.hidden_size;
  if (kind != 3) {
    if (base == "model.embed_tokens") return set_linear(e, e->embed, 0, H, kind, data, shape, ndim, dtype, on_device, name);
    if (base == "lm_head") {
      if (d.tie_word_embeddings) return fail(MI_ERR_NOTFOUND, "lm_head given but tie_word_embeddings is set: " + name);
      return set_linear(e, e->lm_head, 0, H, kind, data, shape, ndim, dtype, on_device, name);
    }
    if (base == "model.norm" && kind == 0) return set_vector(e, e->final_norm, H, data, shape, ndim, dtype, on_device, name);
  }
  const std::string pre = "model.layers.";          // model.layers.<li>.<sub>
  const size_t dot = base.compare(0, pre.size(), pre) == 0 ? base.find('.', pre.size()) : std::string::npos;
  if (dot == std::string::npos) return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
  int li = -1;
  try { li = std::stoi(base.substr(pre.size(), dot - pre.size())); } catch (...) { li = -1; }
  if (li < 0 || li >= d.num_layers) return fail(MI_ERR_NOTFOUND, (kind == 3 ? "unknown tensor: " : "layer index out of range: ") + name);
  const std::string sub = base.substr(dot + 1);
  LayerW& l = e->layers[li];
  Proj p;
  if (d.arch == MI_ARCH_MIXTRAL && sub.compare(0, 17, "block_sparse_moe.") == 0)
    return set_moe_tensor(e, l, sub.substr(17), kind, data, shape, ndim, dtype, on_device, name);
  if (find_proj(d, l, sub, &p)) {
    if (kind != 3 && p.part < 0) return set_linear_fused(e, *p.f, p.K, kind, data, shape, ndim, dtype, on_device, name);
    if (kind != 3) return set_linear(e, *p.f, p.part, p.K, kind, data, shape, ndim, dtype, on_device, name);
    // nn.Linear(bias=True): only where the model has one -- anything else is an unmatched tensor
    if (p.attn ? d.attention_bias : d.mlp_bias) return set_bias(e, *p.f, p.part, data, shape, ndim, dtype, on_device, name);
  } else if (kind == 0) {
    if (sub == "input_layernorm") return set_vector(e, l.in_norm, H, data, shape, ndim, dtype, on_device, name);
    if (sub == "post_attention_layernorm") return set_vector(e, l.post_norm, H, data, shape, ndim, dtype, on_device, name);
    if (d.arch == MI_ARCH_QWEN3 && sub == "self_attn.q_norm") return set_vector(e, l.q_norm, d.head_dim, data, shape, ndim, dtype, on_device, name);
    if (d.arch == MI_ARCH_QWEN3 && sub == "self_attn.k_norm") return set_vector(e, l.k_norm, d.head_dim, data, shape, ndim, dtype, on_device, name);
  }
  return fail(MI_ERR_NOTFOUND, "unknown tensor: " + name);
}

// one adapted range of table column `col` (a per-request slot, or LORA_ENGINE_COL: the engine-wide adapter): entry
// [pj.part][col] of the matrix's table (lora_rows.h), hot-swapped when it exists.  The stream is drained first and the table
// entry is written with a blocking copy: no step is in flight.
//
// Two steps, so that a call that covers several parts (a MI_ARCH_PHI3 fused projection) changes nothing when one of them is
// refused: make_adapter_part builds the device buffers of an entry -- with m (HOST, the part's n values; null: plain LoRA) also
// the DoRA gain, one launch of launch_dora_gain on the finalized matrix, read back and checked -- and set_adapter_part
// publishes it.
static void free_adapter_part(AdapterPart& ap) {
  hipFree(const_cast<float*>(ap.a)); hipFree(const_cast<float*>(ap.b)); hipFree(const_cast<float*>(ap.gain));
  ap = AdapterPart{};
}

static int make_adapter_part(mi_engine* e, LayerW& l, const Proj& pj, const void* A, const void* B, const float* m, int rank, float scale,
                             int on_device, const std::string& name, AdapterPart* out) {
  const mi_model_desc& d = e->d;
  FusedLinear* f = pj.f;
  const int QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim, K = pj.K, n = f->part_rows[pj.part];
  int row0 = 0;
  for (int i = 0; i < pj.part; ++i) row0 += f->part_rows[i];
  // rope_traditional: the output columns of an adapted q / k projection follow the regrouped rows of the matrix
  const bool regroup = d.rope_traditional && f == &l.qkv && row0 < QD + KD;
  MI_HIP(hipStreamSynchronize(e->stream));
  if (f->adapters == nullptr) {
    AdapterPart* dt = nullptr;
    MI_HIP(hipMalloc(&dt, sizeof(AdapterTable::h)));
    if (hipMemset(dt, 0, sizeof(AdapterTable::h)) != hipSuccess) { hipFree(dt); return fail(MI_ERR_RUNTIME, "adapter table: hipMemset failed"); }
    f->adapters = new AdapterTable();
    f->adapters->d = dt;
  }
  float* na = nullptr; float* nb = nullptr; float* dm = nullptr; float* ng = nullptr;
  auto drop = [&](int rc) { hipFree(na); hipFree(nb); hipFree(dm); hipFree(ng); return rc; };
  if (hipMalloc(&na, (size_t)K * rank * sizeof(float)) != hipSuccess || hipMalloc(&nb, (size_t)rank * n * sizeof(float)) != hipSuccess ||
      (m != nullptr && (hipMalloc(&dm, (size_t)n * sizeof(float)) != hipSuccess || hipMalloc(&ng, (size_t)n * sizeof(float)) != hipSuccess))) {
    (void)hipGetLastError();
    return drop(fail(MI_ERR_RUNTIME, name + (m != nullptr ? ": DoRA: out of device memory" : ": LoRA: out of device memory")));
  }
  int rc = copy_in(na, A, (size_t)K * rank * sizeof(float), on_device, e->stream);
  if (rc == MI_OK) rc = copy_in(nb, B, (size_t)rank * n * sizeof(float), on_device, e->stream);
  if (rc == MI_OK && regroup) rc = head_perm_inplace(e, nb, (size_t)rank * n, d.head_dim, sizeof(float));
  if (rc == MI_OK && m != nullptr) {
    // DoRA: m follows the rows like B's columns; the gain of the part from the matrix as the linears read it
    std::vector<float> hg((size_t)n);
    rc = copy_in(dm, m, (size_t)n * sizeof(float), 0, e->stream);
    if (rc == MI_OK && regroup) rc = head_perm_inplace(e, dm, (size_t)n, d.head_dim, sizeof(float));
    if (rc == MI_OK) rc = launch_dora_gain(f->W, row0, n, na, nb, dm, rank, scale, ng, e->stream);
    if (rc == MI_OK && (hipMemcpyAsync(hg.data(), ng, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                        hipStreamSynchronize(e->stream) != hipSuccess))
      rc = fail(MI_ERR_RUNTIME, name + ": computing the DoRA gain failed");
    for (int i = 0; rc == MI_OK && i < n; ++i)
      if (!std::isfinite(hg[i]))
        rc = fail(MI_ERR_INVALID, name + ": DoRA: a row of W + scale (A B)^T has norm 0 (or m / norm is not finite); nothing was changed");
  }
  if (rc != MI_OK) return drop(rc);
  hipFree(dm);
  *out = AdapterPart{na, nb, rank, scale, ng};
  return MI_OK;
}

static int set_adapter_part(mi_engine* e, int col, LayerW& l, const Proj& pj, AdapterPart& fresh) {
  FusedLinear* f = pj.f;
  AdapterPart& slot = f->adapters->h[pj.part][col];
  if (hipMemcpy(f->adapters->d + pj.part * LORA_TABLE_COLS + col, &fresh, sizeof(fresh), hipMemcpyHostToDevice) != hipSuccess) {
    free_adapter_part(fresh);
    return fail(MI_ERR_RUNTIME, "adapter table: hipMemcpy failed");
  }
  const bool was_empty = slot.a == nullptr;
  f->adapters->gains += (fresh.gain != nullptr) - (slot.gain != nullptr);
  free_adapter_part(slot);
  slot = fresh;
  f->adapters->set += was_empty;
  if (col == LORA_ENGINE_COL) {
    e->engine_lora = true;
    // an adapted gate|up never runs a SwiGLU epilogue again: its row-interleaved copy (ensure_gu8) is dead weight
    if (f == &l.gate_up && f->w_gu8 != nullptr) { hipFree(f->w_gu8); f->w_gu8 = nullptr; }
  } else {
    e->adapter_parts[col] += was_empty;
    ++e->adapter_gen[col];              // K / V made with the slot's earlier contents are unreachable from now on (kv_blocks.h)
  }
  return MI_OK;
}

// mi_engine_set_lora (adapter < 0: the engine-wide adapter, the table's private column) and mi_engine_set_adapter_lora (a slot)
// dora: mi_engine_set_dora / mi_engine_set_adapter_dora -- m (N,) float32 rides with the factors and every part gets a gain
static int set_lora_any(mi_engine* e, int adapter, int layer, const char* proj, const void* A, const void* B, const void* m, bool dora,
                        int rank, float scale, int dtype, int on_device) {
  if (!e || !proj || !A || !B || (dora && !m)) return fail(MI_ERR_INVALID, "null argument");
  if (adapter >= MI_MAX_ADAPTERS) return fail(MI_ERR_INVALID, "adapter slot must be in [0, " + std::to_string(MI_MAX_ADAPTERS) + ")");
  if (adapter >= 0 && e->engine_lora)
    return fail(MI_ERR_UNSUPPORTED, "mi_engine_set_adapter_lora: this engine carries the engine-wide adapter of mi_engine_set_lora; the two exclude each other");
  if (adapter < 0 && adapters_resident(e) > 0)
    return fail(MI_ERR_UNSUPPORTED, "mi_engine_set_lora: this engine carries per-request adapters (mi_engine_set_adapter_lora); the two exclude each other");
  if (layer < 0 || layer >= e->d.num_layers) return fail(MI_ERR_INVALID, "layer out of range");
  if (rank < 1 || rank > 64) return fail(MI_ERR_UNSUPPORTED, "LoRA rank must be in [1,64]");
  if (dtype != MI_F32 && dtype != MI_BF16 && dtype != MI_F16) return fail(MI_ERR_INVALID, "bad LoRA dtype");
  if (dtype != MI_F32 && dtype != e->d.act_dtype) return fail(MI_ERR_UNSUPPORTED, "LoRA dtype must be float32 or the model dtype");
  if (dtype != MI_F32) return fail(MI_ERR_UNSUPPORTED, "16-bit LoRA factors are not supported yet (float32 only)");
  MI_HIP(hipSetDevice(e->device));
  const mi_model_desc& d = e->d;
  LayerW& l = e->layers[layer];
  const std::string p(proj);
  Proj pj;
  if (d.arch == MI_ARCH_MIXTRAL && p.compare(0, 17, "block_sparse_moe.") == 0)
    return fail(MI_ERR_UNSUPPORTED, "LoRA on " + p + " is not supported (arch mixtral: the attention projections only)");
  if (!find_proj(d, l, p, &pj)) return fail(MI_ERR_UNSUPPORTED, "LoRA on " + p + " is not supported (the linears of a block only)");
  const std::string name = "model.layers." + std::to_string(layer) + "." + p;
  int N = 0;                                       // rows of the named projection
  if (pj.part >= 0) N = pj.f->part_rows[pj.part];
  else for (int i = 0; i < pj.f->n_parts; ++i) N += pj.f->part_rows[i];
  std::vector<float> hm;                           // DoRA: m on the host, checked before anything is made
  if (dora) {
    if (!e->finalized)
      return fail(MI_ERR_INVALID, name + ": DoRA needs the final weights (the gain is computed from them): call mi_engine_finalize first");
    if (pj.f->quant)
      return fail(MI_ERR_UNSUPPORTED, name + ": DoRA on a projection whose base weights are quantised is not supported");
    if (pj.f->bias != nullptr)
      return fail(MI_ERR_UNSUPPORTED, name + ": DoRA on a projection that carries a linear bias is not supported");
    if (pj.f->W.wk != WK_BF16 && pj.f->W.wk != WK_F16)
      return fail(MI_ERR_UNSUPPORTED, name + ": DoRA needs dense bf16 / f16 base weights");
    hm.resize((size_t)N);
    MI_HIP(hipMemcpy(hm.data(), m, hm.size() * sizeof(float), on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    for (int i = 0; i < N; ++i)
      if (!std::isfinite(hm[i])) return fail(MI_ERR_INVALID, name + ": DoRA: m[" + std::to_string(i) + "] is not finite; nothing was changed");
  }
  const int col = adapter >= 0 ? adapter : LORA_ENGINE_COL;
  if (pj.part >= 0) {
    AdapterPart fresh;
    MI_TRY(make_adapter_part(e, l, pj, A, B, dora ? hm.data() : nullptr, rank, scale, on_device, name, &fresh));
    return set_adapter_part(e, col, l, pj, fresh);
  }
  // MI_ARCH_PHI3, qkv_proj / gate_up_proj: A is shared, B (rank, N) is cut by columns into the parts (and m by parts) -- what
  // one call per part with the column slice does on an engine with split projections.  Every part is made before the first is
  // published.
  std::vector<float> hb((size_t)rank * N), slice;
  MI_HIP(hipMemcpy(hb.data(), B, hb.size() * sizeof(float), on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  AdapterPart made[3];
  int col0 = 0;
  for (int i = 0; i < pj.f->n_parts; ++i) {
    const int n = pj.f->part_rows[i];
    slice.resize((size_t)rank * n);
    for (int r = 0; r < rank; ++r) memcpy(&slice[(size_t)r * n], &hb[(size_t)r * N + col0], (size_t)n * sizeof(float));
    float* sb = slice.data();
    void* db = nullptr;
    int rc = MI_OK;
    if (on_device) {                               // (A stays where it is: the slice goes where A is)
      if (hipMalloc(&db, slice.size() * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); db = nullptr; rc = fail(MI_ERR_RUNTIME, name + ": out of device memory for a column slice"); }
      else if (hipMemcpy(db, sb, slice.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = fail(MI_ERR_RUNTIME, name + ": copying a column slice failed");
    }
    const Proj part{pj.f, i, pj.K, pj.attn};
    if (rc == MI_OK)
      rc = make_adapter_part(e, l, part, A, on_device ? db : (const void*)sb, dora ? hm.data() + col0 : nullptr, rank, scale,
                             on_device, name, &made[i]);
    hipFree(db);
    if (rc != MI_OK) {
      for (int j = 0; j < i; ++j) free_adapter_part(made[j]);
      return rc;
    }
    col0 += n;
  }
  for (int i = 0; i < pj.f->n_parts; ++i) {
    const Proj part{pj.f, i, pj.K, pj.attn};
    const int rc = set_adapter_part(e, col, l, part, made[i]);
    if (rc != MI_OK) {
      for (int j = i + 1; j < pj.f->n_parts; ++j) free_adapter_part(made[j]);
      return rc;
    }
  }
  return MI_OK;
}

int mi_engine_set_lora(mi_engine* e, int layer, const char* proj, const void* A, const void* B, int rank, float scale,
                       int dtype, int on_device) {
  return set_lora_any(e, -1, layer, proj, A, B, nullptr, false, rank, scale, dtype, on_device);
}

int mi_engine_set_adapter_lora(mi_engine* e, int adapter, int layer, const char* proj, const void* A, const void* B, int rank,
                               float scale, int dtype, int on_device) {
  if (adapter < 0 || adapter >= MI_MAX_ADAPTERS)
    return fail(MI_ERR_INVALID, "mi_engine_set_adapter_lora: adapter " + std::to_string(adapter) + " is outside [0, " + std::to_string(MI_MAX_ADAPTERS) + ")");
  return set_lora_any(e, adapter, layer, proj, A, B, nullptr, false, rank, scale, dtype, on_device);
}

int mi_engine_set_dora(mi_engine* e, int layer, const char* proj, const void* A, const void* B, const void* m, int rank, float scale,
                       int dtype, int on_device) {
  return set_lora_any(e, -1, layer, proj, A, B, m, true, rank, scale, dtype, on_device);
}

int mi_engine_set_adapter_dora(mi_engine* e, int adapter, int layer, const char* proj, const void* A, const void* B, const void* m,
                               int rank, float scale, int dtype, int on_device) {
  if (adapter < 0 || adapter >= MI_MAX_ADAPTERS)
    return fail(MI_ERR_INVALID, "mi_engine_set_adapter_dora: adapter " + std::to_string(adapter) + " is outside [0, " + std::to_string(MI_MAX_ADAPTERS) + ")");
  return set_lora_any(e, adapter, layer, proj, A, B, m, true, rank, scale, dtype, on_device);
}

int mi_engine_clear_adapter(mi_engine* e, int adapter) {
  if (!e) return fail(MI_ERR_INVALID, "null engine");
  if (adapter < 0 || adapter >= MI_MAX_ADAPTERS)
    return fail(MI_ERR_INVALID, "mi_engine_clear_adapter: adapter " + std::to_string(adapter) + " is outside [0, " + std::to_string(MI_MAX_ADAPTERS) + ")");
  MI_HIP(hipSetDevice(e->device));
  MI_HIP(hipStreamSynchronize(e->stream));          // no step reads the factors any more
  for (LayerW& l : e->layers)
    for (FusedLinear* f : {&l.qkv, &l.o, &l.gate_up, &l.down}) {
      if (f->adapters == nullptr) continue;
      bool changed = false;
      for (auto& part : f->adapters->h) {
        AdapterPart& ap = part[adapter];
        if (ap.a == nullptr) continue;
        f->adapters->gains -= ap.gain != nullptr;
        free_adapter_part(ap);
        --f->adapters->set;
        changed = true;
      }
      if (changed) MI_HIP(hipMemcpy(f->adapters->d, f->adapters->h, sizeof(AdapterTable::h), hipMemcpyHostToDevice));
    }
  e->adapter_parts[adapter] = 0;
  ++e->adapter_gen[adapter];
  return MI_OK;
}

int mi_engine_finalize(mi_engine* e) {
  if (!e) return fail(MI_ERR_INVALID, "null engine");
  if (e->finalized) return MI_OK;
  MI_HIP(hipSetDevice(e->device));
  const mi_model_desc& d = e->d;
  const int H = d.hidden_size, QD = d.num_heads * d.head_dim;
  // MI_ARCH_MIXTRAL: the router and every expert slot of every block, before anything is repacked (a call that stops here
  // can be repeated once the missing tensor is set)
  for (int i = 0; d.arch == MI_ARCH_MIXTRAL && i < d.num_layers; ++i) {
    const LayerW& l = e->layers[i];
    const std::string p = "model.layers." + std::to_string(i);
    if (l.moe_router == nullptr) return fail(MI_ERR_NOTFOUND, p + ".block_sparse_moe.gate.weight not set");
    static const char* const stacked[3] = {"gate_proj", "up_proj", "down_proj"};
    static const char* const single[3] = {"w1", "w3", "w2"};
    for (int t = 0; t < 3; ++t)
      for (int x = 0; x < d.num_local_experts; ++x)
        if (!l.moe_seen[t][x])
          return fail(MI_ERR_NOTFOUND, p + ".block_sparse_moe: expert " + std::to_string(x) + " of switch_mlp." + stacked[t] + ".weight (experts." +
                                           std::to_string(x) + "." + single[t] + ".weight) not set");
  }
  for (int i = 0; i < d.num_layers; ++i) {
    LayerW& l = e->layers[i];
    const std::string p = "model.layers." + std::to_string(i);
    {   // a set bias flag makes the `.bias` of each of its projections a required tensor
      const struct { const FusedLinear* f; int part; const char* sub; int32_t want; } req[7] = {
          {&l.qkv, 0, ".self_attn.q_proj.bias", d.attention_bias}, {&l.qkv, 1, ".self_attn.k_proj.bias", d.attention_bias},
          {&l.qkv, 2, ".self_attn.v_proj.bias", d.attention_bias}, {&l.o, 0, ".self_attn.o_proj.bias", d.attention_bias},
          {&l.gate_up, 0, ".mlp.gate_proj.bias", d.mlp_bias}, {&l.gate_up, 1, ".mlp.up_proj.bias", d.mlp_bias},
          {&l.down, 0, ".mlp.down_proj.bias", d.mlp_bias}};
      for (const auto& r : req)
        if (r.want && !r.f->seen_bias[r.part]) return fail(MI_ERR_NOTFOUND, p + r.sub + " not set");
    }
    if (d.rope_traditional) MI_TRY(permute_qk_heads(e, l.qkv));      // in front of the tile-major repack
    MI_TRY(finalize_linear(e, l.qkv, H, p + (d.arch == MI_ARCH_PHI3 ? ".self_attn.qkv_proj" : ".self_attn.{q,k,v}_proj")));
    MI_TRY(finalize_linear(e, l.o, QD, p + ".self_attn.o_proj"));
    if (d.arch != MI_ARCH_MIXTRAL) {
      MI_TRY(finalize_linear(e, l.gate_up, H, p + (d.arch == MI_ARCH_PHI3 ? ".mlp.gate_up_proj" : ".mlp.{gate,up}_proj")));
      MI_TRY(finalize_linear(e, l.down, d.intermediate_size, p + ".mlp.down_proj"));
    }
    if (!l.in_norm || !l.post_norm) return fail(MI_ERR_NOTFOUND, p + ": layernorm weights not set");
    if (d.arch == MI_ARCH_QWEN3 && (!l.q_norm || !l.k_norm)) return fail(MI_ERR_NOTFOUND, p + ": q_norm/k_norm not set");
    MI_TRY(make_f32_copy(e, l.in_norm, H, &l.in_norm32));
    MI_TRY(make_f32_copy(e, l.post_norm, H, &l.post_norm32));
    MI_TRY(make_f32_copy(e, l.q_norm, d.head_dim, &l.q_norm32));
    MI_TRY(make_f32_copy(e, l.k_norm, d.head_dim, &l.k_norm32));
    // persistent second copies, while mem_get_info still tells a scheduler the truth about what is left for its KV arena
    if (d.arch != MI_ARCH_MIXTRAL) (void)ensure_gu8(e, l.gate_up, d.intermediate_size);
    if (d.act_dtype == MI_F16) {
      (void)ensure_hilo(e, l.qkv); (void)ensure_hilo(e, l.o);
      if (d.arch != MI_ARCH_MIXTRAL) { (void)ensure_hilo(e, l.gate_up); (void)ensure_hilo(e, l.down); }
    }
  }
  MI_TRY(finalize_linear(e, e->embed, H, "model.embed_tokens"));
  if (!d.tie_word_embeddings) MI_TRY(finalize_linear(e, e->lm_head, H, "lm_head"));
  if (d.act_dtype == MI_F16) (void)ensure_hilo(e, d.tie_word_embeddings ? e->embed : e->lm_head);
  if (!e->final_norm) return fail(MI_ERR_NOTFOUND, "model.norm.weight not set");
  MI_TRY(make_f32_copy(e, e->final_norm, H, &e->final_norm32));
  const size_t n = (size_t)d.max_positions * (d.head_dim / 2);
  MI_HIP(hipMalloc(&e->cos_tab, n * sizeof(float)));
  MI_HIP(hipMalloc(&e->sin_tab, n * sizeof(float)));
  MI_TRY(launch_rope_tables(e->cos_tab, e->sin_tab, d.max_positions, d.head_dim, d.rope_theta, d.rope_scale, e->stream));
  MI_HIP(hipStreamSynchronize(e->stream));
  e->finalized = true;
  return MI_OK;
}

}  // extern "C"
