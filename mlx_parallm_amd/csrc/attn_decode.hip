// attn_decode.hip -- fused decode step of one attention block (L == 1), ONE launch:
//   q/k RMSNorm (qwen3.py:65-70) + RoPE (llama.py:107-117) + KV append (base.py:66-85 / 119-140)
//   + scaled_dot_product_attention over the cache (llama.py:139-141) + split-KV combine.
//
// Grid (nsplit, B*Hkv), 512 threads = 8 waves.  A lane group of 16 lanes (one DPP row) owns one
// key at a time and D/16 elements of it: a wave reads four consecutive KV rows (1 KiB for
// bf16 D = 128) per instruction, and every (wave, lane group) issues U K-rows and U V-rows before
// touching any of them, so a 256-key split is entirely in flight at once.
//   * the GQA group (G = Hq/Hkv query heads) shares every K/V row;
//   * q.k on 16-bit caches uses v_dot2c_f32_{bf16,f16}; the 16-lane reductions are DPP row
//     rotations (no LDS traffic); softmax runs in the exp2 domain, one rescale per U-key block;
//   * the RoPE partner (i <-> i + D/2) is the lane 8 positions away in the row;
//   * the split that owns the new position appends K/V and takes the new key from registers;
//   * splits publish (max, sum, O) partials and take a ticket; the last arriver of a
//     (sequence, kv-head) combines them (agent-scope release -> ticket -> acquire; nobody waits).
#include <type_traits>

#include "attn_dispatch.h"
#include "attn_mfma.h"
#include "gemv_phase.h"

namespace mi {

// Debug build (tools/debug/build_trace_lib.sh): wall-clock stamps of the MFMA decode attention, one 16-slot row per workgroup in
// a buffer of their own (gemm_skinny.hip owns it): 0 entry, 1 every load of the prologue has landed (16-bit caches: the first
// round's K / V were issued in front of them and return in order; float32 caches: the prologue's loads go first and the wait
// leaves the K / V loads behind them in flight), 2 prologue barrier, 3 last MFMA, 4 partial stored, 5 end;
// 6 + r: wave 0 enters round r of a float32 cache (r <= 8); 15: the first round's K / V and the prologue's loads have all been
// issued (the clock is read there and stored with stamp 1: a store in between would count in vmcnt).
#ifdef MI_SK_TRACE
unsigned long long* dbg_trace_slot(int N, int K, int grid, int epi, int M, int kind, int pro, int act);   // gemm_skinny.hip
#define AT_TRACE_PARAM , unsigned long long* trace
#define AT_TRACE_ARG , trace
#define AT_STAMP_AT(i, t) do { if (trace != nullptr && threadIdx.x == 0) trace[(size_t)((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * 16 + (i)] = (t); } while (0)
#define AT_STAMP(i) AT_STAMP_AT(i, wall_clock64())
#define AT_CLOCK(t) const unsigned long long t = wall_clock64()
#define AT_LANDED(n) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n) : "memory")   // n loads issued behind the prologue's stay in flight
#define AT_STAMP_ROUND(r) AT_STAMP(6 + min((int)(r), 8))       // float32 caches: wave 0 enters round r (slots 6..14)
#else
#define AT_TRACE_PARAM
#define AT_TRACE_ARG
#define AT_STAMP_AT(i, t) do { } while (0)
#define AT_STAMP(i) do { } while (0)
#define AT_CLOCK(t) do { } while (0)
#define AT_LANDED(n) do { } while (0)
#define AT_STAMP_ROUND(r) do { } while (0)
#endif

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float row16_ror8(float v) { return __builtin_amdgcn_update_dpp(0.f, v, 0x128, 0xf, 0xf, false); }

template <typename T>
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
  if constexpr (std::is_same<T, bf16>::value)
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
  else
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c, false);
}

// one lane's piece of a row: NW32 dwords of raw bits
template <int NW32>
__device__ __forceinline__ void load_raw(const void* p, uint32_t (&o)[NW32]) {
  if constexpr (NW32 % 4 == 0) {
#pragma unroll
    for (int i = 0; i < NW32 / 4; ++i) {
      const u32x4 v = *((const u32x4*)p + i);
      o[4 * i] = v.x; o[4 * i + 1] = v.y; o[4 * i + 2] = v.z; o[4 * i + 3] = v.w;
    }
  } else if constexpr (NW32 == 2) {
    const u32x2 v = *(const u32x2*)p;
    o[0] = v.x; o[1] = v.y;
  } else if constexpr (NW32 == 6) {               // head_dim 96, float32: 24 bytes, 8-byte aligned
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const u32x2 v = *((const u32x2*)p + i);
      o[2 * i] = v.x; o[2 * i + 1] = v.y;
    }
  } else if constexpr (NW32 == 3) {               // head_dim 96, 16-bit: 12 bytes, 4-byte aligned (one global_load_dwordx3)
    struct W3 { uint32_t a, b, c; };
    const W3 v = *(const W3*)p;
    o[0] = v.a; o[1] = v.b; o[2] = v.c;
  } else {
#pragma unroll
    for (int i = 0; i < NW32; ++i) o[i] = ((const uint32_t*)p)[i];
  }
}

template <typename T, int EPL, int NW32>
__device__ __forceinline__ void raw_to_f32(const uint32_t (&r)[NW32], float (&o)[EPL]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[e] = __uint_as_float(r[e]);
  } else if constexpr (std::is_same<T, bf16>::value) {
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) { o[2 * e] = __uint_as_float(r[e] << 16); o[2 * e + 1] = __uint_as_float(r[e] & 0xffff0000u); }
  } else {
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) {
      const f16x2 h = __builtin_bit_cast(f16x2, r[e]);
      o[2 * e] = (float)h.x; o[2 * e + 1] = (float)h.y;
    }
  }
}


// The last split's combine: (max, sum, O[d]) of every split for one (head, d).  The loads of four splits are issued
// together (a loop over a run-time split count with the loads inside waits one L2 round trip per load: ~8 in a row
// for 4 splits), then merged in split order -- deterministic whoever arrived last.
template <int D>
__device__ __forceinline__ float combine_splits(const float* pp, int nsplit, int d) {
  float mn = -1e30f, L = 0.f, O[1] = {0.f};
  for (int i0 = 0; i0 < nsplit; i0 += 4) {
    float mv[4], lv[4], ov[4][1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* q = pp + (size_t)min(i0 + j, nsplit - 1) * (D + 2);
      mv[j] = __hip_atomic_load(&q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lv[j] = __hip_atomic_load(&q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ov[j][0] = __hip_atomic_load(&q[2 + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    merge_splits4<1>(mn, L, O, mv, lv, ov, nsplit - i0);
  }
  return merged_out(O[0], L);
}

// Cache row and KV length of batch entry b (wave-uniform).  The host knows both (it advances the lengths itself) and passes
// them in the kernel arguments: n_host_off > 0.  On that path nothing may touch vector memory -- the first K/V load waits for
// these two values.  Written as `cond ? c.host_row[b] : rows[b]`, hipcc selects between the two ADDRESSES and emits one
// flat_load_dword per value, one waiting for the other.  So the argument arrays are read unconditionally (index clamped: B
// may exceed 32 on the other path) and each value goes through readfirstlane before the select: the two sources stay two
// values, and the kernel-argument one stays a scalar load.  Device path (op-level calls, row-subset steps): rows[b], then offsets[row].
struct RowLen { int kb, pos; };
__device__ __forceinline__ RowLen row_and_length(const AttnDecodeCall& c, int b) {
  const int bi = min(b, 31);
  const int hrow = __builtin_amdgcn_readfirstlane(c.host_row[bi]);
  const int hoff = __builtin_amdgcn_readfirstlane(c.host_off[bi]);
  if (c.n_host_off > 0) return RowLen{hrow, hoff};
  const int kb = c.s.rows ? c.s.rows[b] : b;
  return RowLen{kb, c.offsets[kb]};
}

// D must be a multiple of 32 for 16-bit caches (two elements per dword per lane); float caches any D % 16 == 0
template <typename T, int D, int G, bool NORM, bool PAGED>
__global__ __launch_bounds__(512) void attn_decode_kernel(AttnDecodeCall c) {
  constexpr int EPL = D / 16, NWV = 8, U = 8;
  constexpr int NW32 = EPL * (int)sizeof(T) / 4;
  constexpr bool PACKED = sizeof(T) == 2;
  constexpr float LOG2E = 1.4426950408889634f;
  const AttnShape& s = c.s;
  const int split = blockIdx.x, bh = blockIdx.y;
  const int b = bh / s.Hkv, kh = bh % s.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, gq = lane >> 4;
  const RowLen rl = row_and_length(c, b);
  const int kb = rl.kb, pos = rl.pos;            // cache row of batch entry b, tokens already in it
  const int n_keys = pos + 1;
  const int chunk = (n_keys + c.nsplit - 1) / c.nsplit;
  const int s0 = split * chunk, s1 = min(n_keys, s0 + chunk);
  const bool owner = pos >= s0 && pos < s1;
  const int nq = s.Hq * D;
  const T* row = (const T*)c.qkv + (size_t)b * (nq + 2 * s.Hkv * D);

  __shared__ float st_m[NWV][G], st_l[NWV][G];
  __shared__ float st_o[NWV][G][D];
  __shared__ int is_last_sh;

  // ---- the K/V rows of the first block go out before anything else: they depend on nothing
  // but the offsets, and their latency then hides the q / k_new prologue
  T* kc = (T*)c.kcache;                          // + kv_elem(row, head, key): contiguous slabs or the block arena
  T* vc = (T*)c.vcache;
  const int send = min(s1, pos);                 // cached keys of this split: [s0, send)
  const T* kbase = kc + li * EPL;
  const T* vbase = vc + li * EPL;
  uint32_t kr[U][NW32], vr[U][NW32];
  bool ok[U];
  auto issue_kv = [&](int base) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sp = base + 4 * wave + gq + 4 * NWV * u;
      ok[u] = sp < send;
      const int spc = ok[u] ? sp : s0;
      const size_t ro = kv_elem<PAGED>(s, kb, kh, spc);
      load_raw<NW32>(kbase + ro, kr[u]);
      load_raw<NW32>(vbase + ro, vr[u]);
    }
  };
  if (s0 < send) issue_kv(s0);

  // ---- prologue: this lane's pieces of q (G heads), k_new, v_new; norm + RoPE in registers.
  // Every load is issued before the first use (straight-line code: a load under a branch costs a
  // vmcnt(0) drain of the K/V rows already in flight and a serialized L2 round trip each).
  const bool hi = li >= 8;                       // this lane holds the second half of a RoPE pair
  uint32_t qraw[G][NW32], kraw[NW32], vnr[NW32];
#pragma unroll
  for (int g = 0; g < G; ++g) load_raw<NW32>(row + (size_t)(kh * G + g) * D + li * EPL, qraw[g]);
  load_raw<NW32>(row + nq + (size_t)kh * D + li * EPL, kraw);
  load_raw<NW32>(row + nq + (size_t)(s.Hkv + kh) * D + li * EPL, vnr);
  float cs[EPL], sn[EPL];
  {
    const float* cp = c.cos_tab + (size_t)pos * (D / 2) + (li & 7) * EPL;
    const float* sp = c.sin_tab + (size_t)pos * (D / 2) + (li & 7) * EPL;
#pragma unroll
    for (int e = 0; e < EPL; ++e) { cs[e] = cp[e]; sn[e] = sp[e]; }
  }
  float qnw[EPL], knw[EPL];
  if constexpr (NORM) {
    uint32_t r0[NW32], r1[NW32];
    load_raw<NW32>((const T*)c.q_norm_w + li * EPL, r0);
    load_raw<NW32>((const T*)c.k_norm_w + li * EPL, r1);
    raw_to_f32<T, EPL, NW32>(r0, qnw);
    raw_to_f32<T, EPL, NW32>(r1, knw);
  }
  auto norm_rope = [&](float (&x)[EPL], const float (&nw)[EPL]) {
    if constexpr (NORM) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) ss = fmaf(x[e], x[e], ss);
      ss = row16_sum(ss);
      const float rs = 1.0f / sqrtf(ss / (float)D + c.eps);
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        x[e] = to_f32(store_act<T>(to_f32(store_act<T>(x[e] * rs, s.rnd)) * nw[e], s.rnd));
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const float p = row16_ror8(x[e]);          // the partner lane (li ^ 8) of the same row
      const float o = hi ? (p * sn[e] + x[e] * cs[e]) : (x[e] * cs[e] - p * sn[e]);
      x[e] = to_f32(store_act<T>(o, s.rnd));
    }
  };
  auto pack = [&](const float (&x)[EPL], uint32_t (&r)[NW32]) {
    if constexpr (PACKED) {
#pragma unroll
      for (int e = 0; e < EPL / 2; ++e) {
        T a[2] = {(T)x[2 * e], (T)x[2 * e + 1]};
        r[e] = __builtin_bit_cast(uint32_t, a);
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = __float_as_uint(x[e]);
    }
  };

  uint32_t qr[G][NW32];                          // q after norm + RoPE, in the cache's element type
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float x[EPL];
    raw_to_f32<T, EPL, NW32>(qraw[g], x);
    norm_rope(x, qnw);
    pack(x, qr[g]);
  }
  uint32_t knr[NW32];
  {
    float x[EPL];
    raw_to_f32<T, EPL, NW32>(kraw, x);
    norm_rope(x, knw);
    pack(x, knr);
  }
  if (owner && wave == 0 && gq == 0 && pos < s.cap) {
    const size_t ro = kv_elem<PAGED>(s, kb, kh, pos) + li * EPL;
#pragma unroll
    for (int i = 0; i < NW32; ++i) {
      ((uint32_t*)(kc + ro))[i] = knr[i];
      ((uint32_t*)(vc + ro))[i] = vnr[i];
    }
  }

  // ---- streaming softmax state (exp2 domain; finite "minus infinity" keeps every exp2 argument finite)
  const float sc2 = c.scale * LOG2E;
  float m[G], l[G], o[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -1e30f; l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }
  auto score = [&](const uint32_t (&kr)[NW32], int g) -> float {
    float d = 0.f;
    if constexpr (PACKED) {
#pragma unroll
      for (int i = 0; i < NW32; ++i) d = dot2<T>(kr[i], qr[g][i], d);
    } else {
#pragma unroll
      for (int i = 0; i < NW32; ++i) d = fmaf(__uint_as_float(kr[i]), __uint_as_float(qr[g][i]), d);
    }
    return d;
  };
  // NK keys held by this lane group: scores -> one rescale -> P.V
  auto block = [&](auto& kr, auto& vr, const bool* ok, auto nk_tag) {
    constexpr int NK = decltype(nk_tag)::value;
    float d[NK][G];
#pragma unroll
    for (int u = 0; u < NK; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) d[u][g] = score(kr[u], g);
#pragma unroll
    for (int u = 0; u < NK; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float v = row16_sum(d[u][g]) * sc2;
        d[u][g] = ok[u] ? v : -INFINITY;
      }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < NK; ++u) mn = fmaxf(mn, d[u][g]);
      const float corr = __builtin_amdgcn_exp2f(m[g] - mn);
      l[g] *= corr;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[g][e] *= corr;
#pragma unroll
      for (int u = 0; u < NK; ++u) { d[u][g] = __builtin_amdgcn_exp2f(d[u][g] - mn); l[g] += d[u][g]; }
      m[g] = mn;
    }
#pragma unroll
    for (int u = 0; u < NK; ++u) {
      float vf[EPL];
      raw_to_f32<T, EPL, NW32>(vr[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] = fmaf(d[u][g], vf[e], o[g][e]);
    }
  };

  for (int base = s0; base < send; base += 4 * NWV * U) {     // uniform trip count
    if (base != s0) issue_kv(base);
    block(kr, vr, ok, std::integral_constant<int, U>{});
  }
  if (owner && wave == 0) {                      // the new key, from registers (wave-uniform branch)
    uint32_t k1[1][NW32], v1[1][NW32];
#pragma unroll
    for (int i = 0; i < NW32; ++i) { k1[0][i] = knr[i]; v1[0][i] = vnr[i]; }
    const bool ok1[1] = {gq == 0};
    block(k1, v1, ok1, std::integral_constant<int, 1>{});
  }

  // ---- merge the four lane groups of the wave (lanes li, li+16, li+32, li+48), then the waves
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float mo = __shfl_xor(m[g], off, 64);
      const float lo = __shfl_xor(l[g], off, 64);
      const float mn = fmaxf(m[g], mo);
      const float ca = __builtin_amdgcn_exp2f(m[g] - mn), cb = __builtin_amdgcn_exp2f(mo - mn);
      l[g] = l[g] * ca + lo * cb;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float oo = __shfl_xor(o[g][e], off, 64);
        o[g][e] = o[g][e] * ca + oo * cb;
      }
      m[g] = mn;
    }
    if (gq == 0) {
      if (li == 0) { st_m[wave][g] = m[g]; st_l[wave][g] = l[g]; }
#pragma unroll
      for (int e = 0; e < EPL; ++e) st_o[wave][g][li * EPL + e] = o[g][e];
    }
  }
  __syncthreads();
  T* out = (T*)c.out + (size_t)b * nq;
  for (int idx = tid; idx < G * D; idx += 512) {
    const int g = idx / D, d = idx % D;
    float mn = -1e30f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) mn = fmaxf(mn, st_m[w][g]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const float cw = __builtin_amdgcn_exp2f(st_m[w][g] - mn);
      L = fmaf(st_l[w][g], cw, L);
      O = fmaf(st_o[w][g][d], cw, O);
    }
    const int h = kh * G + g;
    if (c.nsplit == 1) {
      out[(size_t)h * D + d] = store_act<T>(O / L, c.rnd_out);
    } else {
      // partials are published with write-through (sc1) stores and read back with sc1 loads: no
      // release / acquire fence is needed (an agent release fence here writes back the whole XCD
      // L2 and was measured at ~8 us per launch with the previous kernel's output still dirty)
      float* pp = c.partial + (((size_t)b * s.Hq + h) * c.nsplit + split) * (D + 2);
      __hip_atomic_store(&pp[2 + d], O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == 0) {
        __hip_atomic_store(&pp[0], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&pp[1], L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (c.nsplit == 1 || c.counters == nullptr) return;    // (counters == nullptr: timing experiments only)

  // ---- every storing wave drains its stores, the workgroup meets, ONE lane takes a ticket; the
  // workgroup that draws the last ticket of this (b, kv-head) combines (it waits for nobody)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int ticket = __hip_atomic_fetch_add(&c.counters[bh], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == c.nsplit - 1;
    if (last) __hip_atomic_store(&c.counters[bh], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    is_last_sh = last;
  }
  __syncthreads();
  if (!is_last_sh) return;
  for (int idx = tid; idx < G * D; idx += 512) {
    const int g = idx / D, d = idx % D, h = kh * G + g;
    const float* pp = c.partial + ((size_t)b * s.Hq + h) * c.nsplit * (D + 2);
    out[(size_t)h * D + d] = store_act<T>(combine_splits<D>(pp, c.nsplit, d), c.rnd_out);
  }
}

// ---------------------------------------------------------------------------------------------
// MFMA form of the same launch for 16-bit caches (D a multiple of 32).  Same grid and split
// publication.  The prologue (q / k_new RMSNorm + RoPE, K/V append) is spread over the lane groups,
// one vector each, and meets in LDS; the new key is scored from there and merged as a ninth partial;
// the cached keys -- cut evenly over the splits, 256 per workgroup per round -- go through the
// matrix cores.  Measured (Mistral-7B geometry, B = 8, 1024 keys, 4 splits): 14.1 us against 17.8 us
// for the VALU kernel; a workgroup's own timeline is ~8 us, of which ~3 us are the first global loads.
//   * a wave owns 32 consecutive keys per round (8 waves: 256 keys per workgroup per round) and has
//     their K fragments (16 B per lane, straight from the cache rows: lane (c16, g) of tile t reads
//     K[key 16t + c16][32kk + 8g ..]) and their V rows in flight before the prologue starts;
//   * S^T = K Q^T: v_mfma_16x16x32 with A = K tile, B = Q^T (the G query heads in columns 0..G-1,
//     the other columns zero) -> lane (c16 = head, g) holds the scores of keys 4g + r of each tile;
//   * after exp2 those eight values ARE the B fragment of the next product: the MFMA k index is a
//     free labelling, slot j of lane group g = key 4g + j (tile 0) / 16 + 4g + j - 4 (tile 1);
//   * O^T = V^T P: V rows are written to a per-wave LDS image [16-d tile][key][16 d] (32-B rows) and
//     read back transposed with ds_read_b64_tr_b16 (lane group g: the 4 keys 4g..4g+3 of a tile, lane
//     i of the group receives column i) -- conflict-free, and exactly the key order of P above;
//   * lane (c16 = head, g) ends up with O[head][16 dt + 4g + r]; the online-softmax rescale is a per-
//     lane scalar.  Waves, the new key and the splits are merged as in the VALU kernel.
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int NWV = 8;                           // waves per workgroup of the MFMA kernel

template <int G, int D, int ES>
__host__ __device__ constexpr size_t attn_mfma_vimg_bytes() {     // float32 caches (ES 4): no V image
  return ES == 2 ? (size_t)NWV * 32 * D * 2 : 0;
}

template <int G, int D, int ES>
__host__ __device__ constexpr size_t attn_mfma_lds_bytes() {
  // [V images: NWV waves x 32 keys x D x 2 B (16-bit caches only)][q + new key: (G + 1) x D x ES B]
  // [st_o: (NWV + 1) x G x D floats][st_m, st_l: (NWV + 1) x G floats each]
  return attn_mfma_vimg_bytes<G, D, ES>() + (size_t)(G + 1) * D * ES + (size_t)(NWV + 1) * G * D * 4 + (size_t)2 * (NWV + 1) * G * 4 + 16;
}

// float32 caches, G <= 4 (the 16-block MFMA loop): behind the above, 16-byte aligned, per wave [4 heads][16 keys] softmax
// numerators of the current tile + the 4 heads' correction factors (+ padding: 80 floats)
constexpr int PBLK_FLOATS = 80;
template <int G, int D, int ES>
__host__ __device__ constexpr size_t attn_mfma_pblk_offset() { return (attn_mfma_lds_bytes<G, D, ES>() + 15) / 16 * 16; }
template <int G, int D, int ES>
__host__ __device__ constexpr size_t attn_mfma_lds_total() {
  return ES == 4 && G <= 4 ? attn_mfma_pblk_offset<G, D, ES>() + (size_t)NWV * PBLK_FLOATS * 4 : attn_mfma_lds_bytes<G, D, ES>();
}

// float32 caches (the PagedKVCache mode, base.py:104-140): v_mfma_f32_16x16x4_f32 -- exact float32 products, one float per
// lane and operand.  The MFMA k index and the row index of the A operand are free labellings, which lets every operand
// come straight from 16-byte global loads with no LDS image and no transpose:
//   * S^T = K Q^T: lane (c16 = key, g4) loads K[key][16 i + 4 g4 .. + 3] (i < D/16: per instruction a row gives 64
//     contiguous bytes, as in the 16-bit kernel); step (i, e) multiplies element e of piece i, i.e. lane group g4
//     supplies d = 16 i + 4 g4 + e, and lane (c16 = head, g4) holds the same d of q.  Scores land as in the 16-bit
//     kernel: lane (head, g4) has keys 4 g4 + r.
//   * O^T = V^T P: step r of a 16-key tile takes key 4 g4 + r from lane group g4 -- exactly the P value that lane holds
//     in register r.  Lane (c16, g4) loads V[key 4 g4 + r][64 h + 4 c16 .. + 3]: per instruction 256 contiguous bytes of
//     each of 4 rows; element e of that load is row c16 of the A tile (h, e), so output tile (h, e) row c16' = 4 g4 + reg
//     is d = 64 h + 4 c16' + e.  D/4 MFMAs per key tile for each product (32 + 32 at D = 128, 32 cycles each).
__device__ __forceinline__ f32x4 mfma_f32(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// v_mfma_f32_4x4x1_16b_f32: 16 independent 4 x 4 x 1 blocks, block = lane >> 2; acc[i] of lane 4 blk + j += a(lane 4 blk + i) * b(lane 4 blk + j)
__device__ __forceinline__ f32x4 mfma_blk(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));   // row_ror:8
  v = fmaxf(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));   // row_ror:4
  v = fmaxf(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));   // row_ror:2
  v = fmaxf(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));   // row_ror:1
  return v;
}

// A piece of a cached K / V row in the matrix-core kernel: one CU reads it once per step, and gigabytes of weights and other
// rows pass before the next step reads it again, so it goes past the caches like the weight streams (gemv_f32.hip: load_w).
// The KV append and the prologue's loads keep the default policy.
template <typename V>
__device__ __forceinline__ V load_kv(const void* p) { return __builtin_nontemporal_load((const V*)p); }

// (a call, not an assignment: the address is computed before the value, which the epilogue's schedule depends on)
template <typename T>
__device__ __forceinline__ void store_out(T* p, T v) { *p = v; }

// The launch as a device function.  o_proj + residual hosted behind the attention in the same launch was built,
// bit-identical, and measured SLOWER than two launches (36.7 / 33.7 us against 19.6 + 12.1 us): dropped, DESIGN 4.
// A twelve-wave form (1536 keys in one round of four splits) measured 2251 vs 2257 tok/s (bf16) and 1928 vs 1962 (float32
// caches) against eight waves: removed in this commit; see git history.
// float32 caches on two-term bf16 operands (three v_mfma_f32_16x16x32_bf16 per product) measured 1913 / 1907 against
// 1998 / 1987 tok/s for the exact form below: removed in this commit; see git history.
// QS (consumer_combine, float32 only): the q / k_new / v_new vectors are not read from c.qkv -- the q|k|v linear ran
// publish-only (gemm_skinny.hip, skinny_kernel<bf16_publish, ..>) and each lane group adds the K slices' partial rows of ITS vector here,
// at the place of its one load, with the arithmetic of that linear's last arriver (common.h: add_slice, rs_from_sumsq,
// scale_row).  QSN = 2, 4 or 8 slices (the class of the launch's count: 2, 3..4, 5..8; inside a class a slice past the last
// re-loads the last), all fetched in one round trip in front of the first round's K/V loads.
// Owners only: the prologue -- its global loads and its arithmetic -- runs in the lane groups that own a vector and nowhere
// else.  A split that does not own the new position has the G query heads only (the new key and value are neither loaded,
// summed, rotated nor scored there; its ninth merge slot is written neutral by wave NWV - 1); the new value loads neither
// cos / sin nor norm weights; a wave without an owner (wave * 4 >= vectors) goes from row and length straight to
// issue_k / issue_v.  The vectors stay PACKED from wave 0 up (4 per wave): a wave's instruction issue costs the same with
// 16 or with 64 live lanes, so one vector per wave would put the prologue's ~300 instructions and its wait in front of round
// 0 in G + 2 waves instead of (G + 5) / 4, for the same bytes on the CU's address path; at G = 4 six waves of eight (seven
// in the splits without the new position) now issue round 0 at entry.  In the disassembly of
// attn_decode_mfma_qs_kernel<128,4,false,false,4> an owner wave issues 12 prologue loads (8 slice, 4 cos / sin; the slices'
// row sums are scalar loads), then the 16 K / V loads, and its arithmetic waits vmcnt(23) .. vmcnt(16); the parent issued
// 28 + 16 in every wave.  Measured ("owners only"): 17.58 -> 16.6-16.9 us per launch under the profiler, barrier
// at 5.5 us of the workgroup instead of 7.0.
template <typename T, int D, int G, bool NORM, bool PAGED, int QSN = 0>
__device__ __forceinline__ void attn_decode_mfma_body(const AttnDecodeCall& c, unsigned char* smem AT_TRACE_PARAM) {
  AT_STAMP(0);
  constexpr bool QS = QSN > 0;
  static_assert(!QS || sizeof(T) == 4, "partial q|k|v rows: float32 activations");
  static_assert(QSN == 0 || QSN == 2 || QSN == 4 || QSN == 8, "K slices fetched: the classes 2, 3..4, 5..8");
  constexpr bool F32 = sizeof(T) == 4;           // float32 q / caches / outputs, multiplied exactly on v_mfma_f32_16x16x4_f32
  constexpr bool BLK = sizeof(T) == 4 && G <= 4; // float32, at most 4 query heads per kv head: the 16-block MFMA loop
  static_assert(D % 32 == 0 && D <= 128 && G <= 8 && (!F32 || D % 64 == 0 || (D == 96 && BLK && !QS)),
                "16-bit caches: head_dim 32/64/96/128; float32: 64/128, and 96 in the 16-block form");
  constexpr int EPL = D / 16, NW32 = EPL * (int)sizeof(T) / 4, NTH = NWV * 64;
  constexpr int KK = D / 32, DT = D / 16, NV = (32 * D * 2) / (64 * 16);   // K steps, 16-d tiles, 16-B V loads per lane
  constexpr int KPW = F32 ? 16 : 32;             // keys per wave and round
  constexpr int NP = D / 16, NH = D / 64 > 0 ? D / 64 : 1;   // float32: 16-byte K pieces per lane and tile, 64-d halves of a V row
  // float32, head_dim 96: behind the one 64-d half a row has 32 more floats, 8 bytes per lane: lane (c16, g4) loads
  // V[key 4 g4 + r][64 + 2 c16 .. + 1], two more A tiles (e < 2) whose row c16 is d = 64 + 2 c16 + e -- accO[4], accO[5]
  constexpr bool VT = F32 && D % 64 == 32;
  constexpr float LOG2E = 1.4426950408889634f;
  const AttnShape& s = c.s;
  const int split = blockIdx.x, bh = blockIdx.y;
  const int b = bh / s.Hkv, kh = bh % s.Hkv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, gq = lane >> 4;      // VALU prologue view: lane li of a row owns D/16 elements
  const int c16 = li, g4 = gq;                   // MFMA view: column / lane group
  const RowLen rl = row_and_length(c, b);
  const int kb = rl.kb, pos = rl.pos;            // cache row of batch entry b, tokens already in it
  // the pos cached keys are cut evenly over the splits (a 1024-key context = 4 x 256 = one round each); the
  // new key is merged by the last split from registers / LDS
  // (float32: in whole 16-key tiles -- a wave's unit of work -- so that at most one split ends in a ragged tile)
  const int chunk = F32 ? ((pos + 16 * c.nsplit - 1) / (16 * c.nsplit)) * 16 : (pos + c.nsplit - 1) / c.nsplit;
  const int s0 = split * chunk;
  const bool owner = split == c.nsplit - 1;
  const int nq = s.Hq * D;
  const T* row = (const T*)c.qkv + (size_t)b * (nq + 2 * s.Hkv * D);

  constexpr size_t VIMG = attn_mfma_vimg_bytes<G, D, (int)sizeof(T)>();
  unsigned char* vimg = smem + (size_t)wave * (32 * D * 2);           // this wave's V image (16-bit caches)
  T* q_sh = (T*)(smem + VIMG);                                        // [G + 1][D]: q heads, then the new key
  float* st_o = (float*)(smem + VIMG + (size_t)(G + 1) * D * sizeof(T));   // [NWV + 1][G][D]
  float* st_m = st_o + (NWV + 1) * G * D;                             // [NWV + 1][G]
  float* st_l = st_m + (NWV + 1) * G;
  int& is_last_sh = *(int*)(st_l + (NWV + 1) * G);       // (no static __shared__ in front of the dynamic region)

  T* kc = (T*)c.kcache;                          // + kv_elem(row, head, key): contiguous slabs or the block arena
  T* vc = (T*)c.vcache;
  const int send = min(s0 + chunk, pos);         // cached keys of this split: [s0, send)

  // ---- the K fragments and V rows of the first round go out before anything else
  u32x4 kf[F32 ? 1 : 2][F32 ? 1 : KK], vrow[F32 ? 1 : NV];
  f32x4 kf32[F32 ? NP : 1], vv32[F32 ? 4 : 1][F32 ? NH : 1];
  f32x2 vt32[VT ? 4 : 1];
  const int klast = max(send - 1, 0);            // every address is clamped to a valid row: no load sits under a branch
  auto issue_k = [&](int base) {                 // keys base + KPW wave + [0, KPW)
    const int k0 = base + KPW * wave;
    if constexpr (F32) {
      const int key = min(k0 + c16, klast);
      const size_t ro = kv_elem<PAGED>(s, kb, kh, key);
#pragma unroll
      for (int i = 0; i < NP; ++i) kf32[i] = load_kv<f32x4>(kc + ro + 16 * i + 4 * g4);
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int key = min(k0 + 16 * t + c16, klast);
        const size_t ro = kv_elem<PAGED>(s, kb, kh, key);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kf[t][kk] = load_kv<u32x4>(kc + ro + 32 * kk + 8 * g4);
      }
    }
  };
  auto issue_v = [&](int base) {
    const int k0 = base + KPW * wave;
    if constexpr (F32) {                         // key 4 g4 + r of the tile, 256 contiguous bytes per row and instruction
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = min(k0 + 4 * g4 + r, klast);
        const size_t ro = kv_elem<PAGED>(s, kb, kh, key);
#pragma unroll
        for (int h = 0; h < NH; ++h) vv32[r][h] = load_kv<f32x4>(vc + ro + 64 * h + 4 * c16);
        if constexpr (VT) vt32[r] = load_kv<f32x2>(vc + ro + 64 * NH + 2 * c16);
      }
    } else {                                     // 32 keys x (D/8) 16-byte pieces, lane-linear: piece = i * 64 + lane
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int piece = i * 64 + lane, kl = piece / (D / 8), dc = piece % (D / 8);
        const int key = min(k0 + kl, klast);
        vrow[i] = load_kv<u32x4>(vc + kv_elem<PAGED>(s, kb, kh, key) + 8 * dc);
      }
    }
  };
  // 16-bit caches: the first round's K / V go out before anything else.  float32 caches: behind the prologue's loads -- a
  // CU returns loads in the order of issue, and a round of float32 K / V is 128 KiB per CU: in front, it held the
  // prologue (and with it the barrier, the q fragments and the first product) back until the whole round had landed.
  // (Block-paged float32 caches keep the old order: their K / V addresses wait for a block-table load, which would
  // queue behind the prologue's loads; not measured.)
  constexpr bool PRO_FIRST = F32 && !PAGED;
  if constexpr (!PRO_FIRST) {
    issue_k(s0);
    issue_v(s0);
  }

  // ---- prologue, spread over the workgroup: lane group (wave, gq) = vector vi owns ONE of the G query heads (vi < G), the
  // new key (vi == G) or the new value (vi == G + 1): raw load, RMSNorm, RoPE, result to LDS.  Owners only (see the header):
  //   * a split that does not own the new position has G vectors, not G + 2 -- the new key and the new value are neither
  //     loaded, summed, rotated nor scored there;
  //   * a lane group without a vector is masked out of every load and every instruction of the prologue;
  //   * a wave without any owner (wv * 4 >= nvec: waves 2..7 at G = 4 in the owning split, 1..7 in the others) branches
  //     round it -- a scalar branch: from row and length straight to issue_k / issue_v.
  // Inside an owner wave the lane groups run one path side by side, so the wave spends the time of one vector.
  const int vi = wave * 4 + gq;
  const int nvec = owner ? G + 2 : G;
  const bool is_q = vi < G, is_k = owner && vi == G, is_v = owner && vi == G + 1;
  const bool has_vec = vi < nvec, rot = is_q || is_k;          // rot: the vectors that are normed and rotated
  const bool wave_owns = __builtin_amdgcn_readfirstlane(wave) * 4 < nvec;
  const bool hi = li >= 8;
  const T* src = row + (is_q ? (size_t)(kh * G + vi) * D : is_k ? (size_t)nq + (size_t)kh * D
                                                               : (size_t)nq + (size_t)(s.Hkv + kh) * D) + li * EPL;
  uint32_t raw[NW32];
  // K slices fetched per lane group: the launch picks the class of c.qkv_ksplit (2, 3..4, 5..8 -> QSN 2, 4, 8)
  f32x4 qs_p[QS ? QSN : 1][QS ? EPL / 4 : 1];
  float qs_sq[QS ? QSN : 1];
  float cs[EPL], sn[EPL];
  uint32_t r0[NW32];
  constexpr int KV_BEHIND = PRO_FIRST ? NP + 4 * NH + (VT ? 4 : 0) : 0;   // K / V loads per lane of a float32 round, in the queue behind the prologue's
  auto pro_loads = [&]() {                       // (runs under both tests below, in the lane groups that own a vector)
    {
      if constexpr (QS) {                        // straight-line: inside a class, a slice past the last re-loads the last
        const size_t ld = (size_t)nq + 2 * (size_t)s.Hkv * D, col = (size_t)(src - row);
#pragma unroll
        for (int j = 0; j < QSN; ++j) {
          const int sl = min(j, c.qkv_ksplit - 1);
          const float* pp = c.qkv_pub + ((size_t)sl * 8 + b) * ld + col;
#pragma unroll
          for (int i = 0; i < EPL / 4; ++i) qs_p[j][i] = *(const f32x4*)(pp + 4 * i);
          qs_sq[j] = c.qkv_pub_sq[sl * 8 + b];
        }
      } else {
        load_raw<NW32>(src, raw);
      }
      if (rot) {                                 // the new value is neither normed nor rotated: no tables, no weights
        const float* cp = c.cos_tab + (size_t)pos * (D / 2) + (li & 7) * EPL;
        const float* sp = c.sin_tab + (size_t)pos * (D / 2) + (li & 7) * EPL;
#pragma unroll
        for (int e = 0; e < EPL; ++e) { cs[e] = cp[e]; sn[e] = sp[e]; }
        if constexpr (NORM) load_raw<NW32>((const T*)(is_k ? c.k_norm_w : c.q_norm_w) + li * EPL, r0);
      }
    }
  };
  auto pro_math = [&]() {
    // (thread 0, which writes the stamps, always owns query head 0)
    AT_CLOCK(t_issued);
    AT_LANDED(KV_BEHIND);
    AT_STAMP_AT(15, t_issued);
    AT_STAMP(1);
    {
      if constexpr (QS) {                        // the q|k|v linear's combine and epilogue: slices in order from zero, then x rs
        float tot = 0.f;
#pragma unroll
        for (int j = 0; j < QSN; ++j) if (j < c.qkv_ksplit) tot = add_slice(tot, qs_sq[j]);
        const float rs = rs_from_sumsq(tot, c.hidden_k, c.qkv_eps);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          float a = 0.f;
#pragma unroll
          for (int j = 0; j < QSN; ++j) if (j < c.qkv_ksplit) a = add_slice(a, qs_p[j][e >> 2][e & 3]);
          raw[e] = __float_as_uint(scale_row(a, rs));
        }
      }
      uint32_t pk[NW32];
      if (rot) {
        float x[EPL];
        raw_to_f32<T, EPL, NW32>(raw, x);
        if constexpr (NORM) {
          float nw[EPL];
          raw_to_f32<T, EPL, NW32>(r0, nw);
          float ss = 0.f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) ss = fmaf(x[e], x[e], ss);
          ss = row16_sum(ss);
          const float rs = 1.0f / sqrtf(ss / (float)D + c.eps);
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            x[e] = to_f32(store_act<T>(to_f32(store_act<T>(x[e] * rs, s.rnd)) * nw[e], s.rnd));
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const float p = row16_ror8(x[e]);
          const float o = hi ? (p * sn[e] + x[e] * cs[e]) : (x[e] * cs[e] - p * sn[e]);
          x[e] = to_f32(store_act<T>(o, s.rnd));
        }
        if constexpr (F32) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) pk[e] = __float_as_uint(x[e]);
        } else {
#pragma unroll
          for (int e = 0; e < EPL / 2; ++e) pk[e] = pack2<T>(x[2 * e], x[2 * e + 1]);
        }
        // q heads at rows 0..G-1 of q_sh, the new key at row G (a split without the new position leaves row G
        // unwritten, and does not read it: the new key's scores are not computed there)
#pragma unroll
        for (int i = 0; i < NW32; ++i) ((uint32_t*)(q_sh + (size_t)vi * D + li * EPL))[i] = pk[i];
      } else {                                   // v: untouched bits
#pragma unroll
        for (int i = 0; i < NW32; ++i) pk[i] = raw[i];
      }
      if (!is_q && pos < s.cap) {                // KV append (base.py:66-85); is_k / is_v: only in the split that owns pos
        T* dst = (is_k ? kc : vc) + kv_elem<PAGED>(s, kb, kh, pos) + li * EPL;
#pragma unroll
        for (int i = 0; i < NW32; ++i) ((uint32_t*)dst)[i] = pk[i];
      }
      if (is_v) {                                // merge slot 8 = the new key: O = v_new (for every head)
        float vf[EPL];
        raw_to_f32<T, EPL, NW32>(raw, vf);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < EPL; ++e) st_o[(NWV * G + g) * D + li * EPL + e] = vf[e];
      }
    }
  };
  if constexpr (PRO_FIRST) {
    // float32, contiguous: the owners' loads, then ONE copy of round 0's issue for every wave, then the owners' arithmetic.
    // It waits for vmcnt(KV_BEHIND), not for an empty queue: at the join behind the first branch the owners' loads are
    // pending on one path and unknown on the other, which keeps their distance to the end of the queue exact.  (With a
    // copy of the issue in each arm of `if (wave_owns) .. else ..` hipcc lets the arm without the prologue fall into the
    // other under an empty exec mask, counts that arm's K / V loads as pending on the owners' path and puts vmcnt(7) ..
    // vmcnt(1) in front of the owners' K / V issue: a round trip of the prologue's loads before round 0 leaves.)
    if (wave_owns) if (has_vec) pro_loads();
    __builtin_amdgcn_sched_barrier(0);
    issue_k(s0);
    issue_v(s0);
    // (Two barriers: where a hook used to sit between them; with one, hipcc allocates the body's registers differently.)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_sched_barrier(0);
    if (wave_owns) if (has_vec) pro_math();
  } else {
    // round 0 is out already: loads and arithmetic under ONE branch.  (Under two, hipcc counts the loads as pending on the
    // path that skips the arithmetic, and every wave meets vmcnt(0) -- the whole of round 0 -- behind the barrier.)
    if (wave_owns) if (has_vec) {
      pro_loads();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_sched_barrier(0);
      pro_math();
    }
  }
  const float sc2 = c.scale * LOG2E;
  __syncthreads();
  AT_STAMP(2);
  if (wave == NWV - 1 && !owner) {
    // A split without the new position: merge slot 8 is neutral -- zeros under the maximum -1e30 and the sum 0, the words
    // the parent wrote there from a loaded and rotated new key -- and nothing of the new key or value is read for it.  Such
    // a split leaves q_sh row G unwritten (nothing reads it); every word the merge below reads is written.
    for (int i = lane; i < G * D / 4; i += 64) *(f32x4*)(st_o + NWV * G * D + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (lane < G) { st_m[NWV * G + lane] = -1e30f; st_l[NWV * G + lane] = 0.f; }
  }
  if (wave == NWV - 1 && owner) {                // scores of the new key: q_sh rows 0..G-1 against row G
    uint32_t kn[NW32];
#pragma unroll
    for (int i = 0; i < NW32; ++i) kn[i] = ((const uint32_t*)(q_sh + (size_t)G * D + li * EPL))[i];
#pragma unroll
    for (int j = 0; j < (G + 3) / 4; ++j) {
      const int g = min(gq + 4 * j, G - 1);
      float d = 0.f;
      if constexpr (F32) {
#pragma unroll
        for (int i = 0; i < NW32; ++i)
          d = fmaf(__uint_as_float(kn[i]), __uint_as_float(((const uint32_t*)(q_sh + (size_t)g * D + li * EPL))[i]), d);
      } else {
#pragma unroll
        for (int i = 0; i < NW32; ++i) d = dot2<T>(kn[i], ((const uint32_t*)(q_sh + (size_t)g * D + li * EPL))[i], d);
      }
      d = row16_sum(d) * sc2;
      if (li == 0 && gq + 4 * j < G) { st_m[NWV * G + g] = d; st_l[NWV * G + g] = 1.f; }
    }
  }
  u32x4 qf[F32 ? 1 : KK];
  f32x4 qf32[F32 ? NP : 1];
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int hq = BLK ? (c16 & 3) : c16;      // (16-block form: lane j of a block supplies head j)
      qf32[i] = *(const f32x4*)(q_sh + (size_t)(hq < G ? hq : 0) * D + 16 * i + 4 * g4);
      if (hq >= G) qf32[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[kk] = *(const u32x4*)(q_sh + (size_t)(c16 < G ? c16 : 0) * D + 32 * kk + 8 * g4);
      if (c16 >= G) qf[kk] = u32x4{0u, 0u, 0u, 0u};
    }
  }

  // ---- rounds of 256 keys per workgroup (float32 caches: 128)
  // m_run / l_run: of head c16 (lanes c16 < G) over this lane group's keys; in the 16-block float32 loop (BLK) of head g4
  // over the keys of this lane (key c16 of every tile)
  float m_run = -1e30f, l_run = 0.f;
  f32x4 accO[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) accO[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BLK) {
    // v_mfma_f32_4x4x1_16b_f32: the G <= 4 heads fill the 4 rows of each of the 16 blocks, where the 16x16x4 form gives them 4 of
    // its 16 columns -- a quarter of the matrix time per key tile, from the same loads (lane (c16, g4), block = lane >> 2):
    //   * S = Q K^T: b = kf32[i][e] = K[key c16][16 i + 4 g4 + e], a = q[head c16 & 3][same d]: register h accumulates
    //     (head h, key c16) over the quarter of d that lane group g4 owns.  The four groups then add their quarters so
    //     that group g4 is left with head g4 (a reduce-scatter: 3 exchanges), and runs that head's online softmax over
    //     the 16 keys of its row (DPP); m_run / l_run are head g4's (l_run: this lane's keys, summed over the row at the end).
    //   * O = P V: b = vv32[r][h][e] = V[key 4 g4 + r][64 h + 4 c16 + e], a = P[head c16 & 3][key 4 g4 + r].  P[head g4][key c16]
    //     is in lane (c16, g4), so it goes through 256 B of LDS of the wave's own, with the four correction factors behind
    //     it: one 4-byte write and two 16-byte reads per lane and tile.  Only this wave touches them (DS operations of a
    //     wave execute in order): no workgroup barrier.  Register i of accO[4 h + e] = O[head i][64 h + 4 c16 + e] over
    //     the keys of group g4; the groups are added once behind the loop.
    // The trip count is the wave's own, as below.
    float* p_sh = (float*)(smem + attn_mfma_pblk_offset<G, D, 4>()) + wave * PBLK_FLOATS;
    const bool gb0 = (g4 & 1) != 0, gb1 = (g4 & 2) != 0;
    for (int base = s0; base + KPW * wave < send; base += KPW * NWV) {
      const bool more = base + KPW * NWV + KPW * wave < send;
      AT_STAMP_ROUND((base - s0) / (KPW * NWV));
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};          // two chains: the dependent latency is hidden
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        sa = mfma_blk(qf32[i][0], kf32[i][0], sa);
        sb = mfma_blk(qf32[i][1], kf32[i][1], sb);
        sa = mfma_blk(qf32[i][2], kf32[i][2], sa);
        sb = mfma_blk(qf32[i][3], kf32[i][3], sb);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_k(base + KPW * NWV);
      __builtin_amdgcn_sched_barrier(0);
      const f32x4 sc = sa + sb;
      // groups {0, 1} keep heads {0, 1} and receive them from groups {2, 3}, and vice versa; then the same inside each pair
      float k0v = gb1 ? sc[2] : sc[0], k1v = gb1 ? sc[3] : sc[1];
      k0v += __shfl_xor(gb1 ? sc[0] : sc[2], 32, 64);
      k1v += __shfl_xor(gb1 ? sc[1] : sc[3], 32, 64);
      float sv = (gb0 ? k1v : k0v) + __shfl_xor(gb0 ? k0v : k1v, 16, 64);   // (head g4, key c16), all of d
      sv = (base + KPW * wave + c16) < send ? sv * sc2 : -INFINITY;
      const float mn = fmaxf(m_run, row16_max(sv));
      const float corr = __builtin_amdgcn_exp2f(m_run - mn);
      const float pv = __builtin_amdgcn_exp2f(sv - mn);
      m_run = mn;
      l_run = l_run * corr + pv;
      p_sh[16 * g4 + c16] = pv;
      if (c16 == 0) p_sh[64 + g4] = corr;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const f32x4 pa = *(const f32x4*)(p_sh + 16 * (c16 & 3) + 4 * g4);
      const f32x4 cr = *(const f32x4*)(p_sh + 64);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) accO[dt] *= cr;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) accO[h * 4 + e] = mfma_blk(pa[r], vv32[r][h][e], accO[h * 4 + e]);
      if constexpr (VT) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 2; ++e) accO[NH * 4 + e] = mfma_blk(pa[r], vt32[r][e], accO[NH * 4 + e]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_v(base + KPW * NWV);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else if constexpr (F32) {
    // 16 keys per wave and round.  The trip count is the wave's own: nothing in the loop crosses waves, and a wave whose
    // keys are exhausted neither loads nor multiplies for the others' last round (it would add p = 0 under a correction
    // of 1: skipping is bit-identical; a wave with no keys at all merges as (-1e30, 0, 0)).
    for (int base = s0; base + KPW * wave < send; base += KPW * NWV) {
      const bool more = base + KPW * NWV + KPW * wave < send;   // wave-uniform: no prefetch of a round that is not computed
      AT_STAMP_ROUND((base - s0) / (KPW * NWV));
      f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = mfma_f32(kf32[i][e], qf32[i][e], sc);
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_k(base + KPW * NWV);       // rolling prefetch: the next round's K into the registers just consumed
      __builtin_amdgcn_sched_barrier(0);
      const int k0 = base + KPW * wave;
      float mx = -1e30f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = (k0 + 4 * g4 + r) < send;
        sc[r] = ok ? sc[r] * sc2 : -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));    // max over the wave's 16 keys, per head
      const float mn = fmaxf(m_run, mx);
      const float corr = __builtin_amdgcn_exp2f(m_run - mn);
      m_run = mn;
      l_run *= corr;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) accO[dt] *= corr;
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[r] = __builtin_amdgcn_exp2f(sc[r] - mn); l_run += p[r]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) accO[h * 4 + e] = mfma_f32(vv32[r][h][e], p[r], accO[h * 4 + e]);
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_v(base + KPW * NWV);       // ... and the next round's V rows
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
  for (int base = s0; base < send; base += 32 * NWV) {        // uniform trip count
    // S^T tiles: rows = keys, columns = heads
    f32x4 sc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) sc[t] = mfma16<T>(kf[t][kk], qf[kk], sc[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
    issue_k(base + 32 * NWV);                    // rolling prefetch: the next round's K into the registers just consumed
    __builtin_amdgcn_sched_barrier(0);
    const int k0 = base + 32 * wave;
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = (k0 + 16 * t + 4 * g4 + r) < send;
        sc[t][r] = ok ? sc[t][r] * sc2 : -INFINITY;
        mx = fmaxf(mx, sc[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // max over the wave's 32 keys, per head
    const float mn = fmaxf(m_run, mx);
    const float corr = __builtin_amdgcn_exp2f(m_run - mn);
    m_run = mn;
    l_run *= corr;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accO[dt] *= corr;
    float p[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[t][r] = __builtin_amdgcn_exp2f(sc[t][r] - mn); l_run += p[t][r]; }
    uint32_t ph[4], pw[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      pack2_split<T>(p[t][0], p[t][1], ph[2 * t], pw[2 * t]);
      pack2_split<T>(p[t][2], p[t][3], ph[2 * t + 1], pw[2 * t + 1]);
    }
    const u32x4 pf = {ph[0], ph[1], ph[2], ph[3]}, pl = {pw[0], pw[1], pw[2], pw[3]};
    // V rows -> this wave's image [16-d tile][key][16 d]
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int piece = i * 64 + lane, kl = piece / (D / 8), dc = piece % (D / 8);
      *(u32x4*)(vimg + (size_t)(dc >> 1) * 1024 + kl * 32 + (dc & 1) * 16) = vrow[i];
    }
    __builtin_amdgcn_sched_barrier(0);
    issue_v(base + 32 * NWV);                    // ... and the next round's V rows
    __builtin_amdgcn_sched_barrier(0);
    // O^T tiles: A = V^T (transposed reads), B = P
    const int tq = c16 >> 2, tp = c16 & 3;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const unsigned char* a0 = vimg + (size_t)dt * 1024 + (4 * g4 + tq) * 32 + tp * 8;
      const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
      const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 16 * 32));
      const uint32_t* w0 = (const uint32_t*)&v0;
      const uint32_t* w1 = (const uint32_t*)&v1;
      const u32x4 vf = {w0[0], w0[1], w1[0], w1[1]};
      accO[dt] = mfma16<T>(vf, pf, accO[dt]);
      accO[dt] = mfma16<T>(vf, pl, accO[dt]);
    }
  }
  }
  AT_STAMP(3);
  // ---- this wave's (m, l, O) for the heads in columns c16 < G
  if constexpr (BLK) {
    // the same reduce-scatter over the lane groups for O: group g4 is left with O[head g4][64 h + 4 c16 + e], 16 bytes per h
    const bool gb0 = (g4 & 1) != 0, gb1 = (g4 & 2) != 0;
    l_run = row16_sum(l_run);
    f32x4 oh[NH + (VT ? 1 : 0)];                  // (head_dim 96: the 8-byte tail in oh[NH][0], oh[NH][1])
#pragma unroll
    for (int h = 0; h < NH + (VT ? 1 : 0); ++h)
#pragma unroll
      for (int e = 0; e < (h < NH ? 4 : 2); ++e) {
        const f32x4 a = accO[h * 4 + e];
        float k0v = gb1 ? a[2] : a[0], k1v = gb1 ? a[3] : a[1];
        k0v += __shfl_xor(gb1 ? a[0] : a[2], 32, 64);
        k1v += __shfl_xor(gb1 ? a[1] : a[3], 32, 64);
        oh[h][e] = (gb0 ? k1v : k0v) + __shfl_xor(gb0 ? k0v : k1v, 16, 64);
      }
    if (g4 < G) {
      if (c16 == 0) { st_m[wave * G + g4] = m_run; st_l[wave * G + g4] = l_run; }
#pragma unroll
      for (int h = 0; h < NH; ++h) *(f32x4*)(st_o + (size_t)(wave * G + g4) * D + 64 * h + 4 * c16) = oh[h];
      if constexpr (VT) *(f32x2*)(st_o + (size_t)(wave * G + g4) * D + 64 * NH + 2 * c16) = f32x2{oh[NH][0], oh[NH][1]};
    }
  } else {
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (c16 < G) {
    if (g4 == 0) { st_m[wave * G + c16] = m_run; st_l[wave * G + c16] = l_run; }
    if constexpr (F32) {                         // tile (h, e), row 4 g4 + r  <->  d = 64 h + 4 (4 g4 + r) + e
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_o[(wave * G + c16) * D + 64 * (dt >> 2) + 16 * g4 + 4 * r + (dt & 3)] = accO[dt][r];
    } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_o[(wave * G + c16) * D + 16 * dt + 4 * g4 + r] = accO[dt][r];
    }
  }
  }
  __syncthreads();
  T* out = (T*)c.out + (size_t)b * nq;
  for (int idx = tid; idx < G * D; idx += NTH) {
    const int g = idx / D, d = idx % D;
    float mn = -1e30f;
#pragma unroll
    for (int w = 0; w < NWV + 1; ++w) mn = fmaxf(mn, st_m[w * G + g]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < NWV + 1; ++w) {
      const float cw = __builtin_amdgcn_exp2f(st_m[w * G + g] - mn);
      L = fmaf(st_l[w * G + g], cw, L);
      O = fmaf(st_o[(w * G + g) * D + d], cw, O);
    }
    const int h = kh * G + g;
    if (c.nsplit == 1) {
      store_out<T>(&out[(size_t)h * D + d], store_act<T>(O / L, c.rnd_out));
    } else {
      float* pp = c.partial + (((size_t)b * s.Hq + h) * c.nsplit + split) * (D + 2);
      __hip_atomic_store(&pp[2 + d], O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == 0) {
        __hip_atomic_store(&pp[0], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&pp[1], L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  AT_STAMP(4);
  if (c.nsplit == 1 || c.counters == nullptr) { AT_STAMP(5); return; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int ticket = __hip_atomic_fetch_add(&c.counters[bh], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == c.nsplit - 1;
    if (last) __hip_atomic_store(&c.counters[bh], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last_sh = last;
  }
  __syncthreads();
  if (!is_last_sh) { AT_STAMP(5); return; }
  for (int idx = tid; idx < G * D; idx += NTH) {
    const int g = idx / D, d = idx % D, h = kh * G + g;
    const float* pp = c.partial + ((size_t)b * s.Hq + h) * c.nsplit * (D + 2);
    store_out<T>(&out[(size_t)h * D + d], store_act<T>(combine_splits<D>(pp, c.nsplit, d), c.rnd_out));
  }
  AT_STAMP(5);
}

template <typename T, int D, int G, bool NORM, bool PAGED>
__global__ __launch_bounds__(NWV * 64) void attn_decode_mfma_kernel(AttnDecodeCall c AT_TRACE_PARAM) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn_decode_mfma_body<T, D, G, NORM, PAGED>(c, smem AT_TRACE_ARG);
}

// consumer_combine: the same launch with the q|k|v partial rows added in the prologue (a kernel of its own: the
// ordinary instantiations keep their code and registers).  QSN: the K slices each owner fetches -- 2, 4 or 8 for the
// q|k|v launch's 2, 3..4 or 5..8 (launch_mfma_qs_n), so the launch of the headline shape (4 slices) fetches 4, not 8
template <int D, int G, bool NORM, bool PAGED, int QSN>
__global__ __launch_bounds__(NWV * 64) void attn_decode_mfma_qs_kernel(AttnDecodeCall c AT_TRACE_PARAM) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn_decode_mfma_body<float, D, G, NORM, PAGED, QSN>(c, smem AT_TRACE_ARG);
}

template <int D, int G, bool NORM, bool PAGED, int QSN>
int launch_mfma_qs(const AttnDecodeCall& c, const dim3 grid, hipStream_t st AT_TRACE_PARAM) {
  constexpr size_t lds = attn_mfma_lds_total<G, D, 4>();
  auto kern = attn_decode_mfma_qs_kernel<D, G, NORM, PAGED, QSN>;
  MI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, dim3(NWV * 64), lds, st, c AT_TRACE_ARG);
  MI_HIP(hipGetLastError());
  return MI_OK;
}
template <int D, int G, bool NORM, bool PAGED>
int launch_mfma_qs_n(const AttnDecodeCall& c, const dim3 grid, hipStream_t st AT_TRACE_PARAM) {
  if (c.qkv_ksplit <= 2) return launch_mfma_qs<D, G, NORM, PAGED, 2>(c, grid, st AT_TRACE_ARG);
  if (c.qkv_ksplit <= 4) return launch_mfma_qs<D, G, NORM, PAGED, 4>(c, grid, st AT_TRACE_ARG);
  return launch_mfma_qs<D, G, NORM, PAGED, 8>(c, grid, st AT_TRACE_ARG);
}

template <typename T, int D, int G, bool NORM, bool PAGED>
int launch_mfma_g(const AttnDecodeCall& c, hipStream_t st) {
  const AttnShape& s = c.s;
  const dim3 grid(c.nsplit, s.B * s.Hkv);
#ifdef MI_SK_TRACE
  // record: N = Hq D, K = keys of row 0, epi = splits, kind -2 (-3: the q|k|v slices are added here), pro = 1 when a last arriver combines
  unsigned long long* trace = dbg_trace_slot(s.Hq * D, c.n_host_off > 0 ? c.host_off[0] : 0, c.nsplit * s.B * s.Hkv, c.nsplit, s.B,
                                             c.qkv_pub != nullptr ? -3 : -2, c.counters != nullptr ? 1 : 0, s.act);
#endif
  if (c.qkv_pub != nullptr) {
    if constexpr (sizeof(T) == 4 && D % 64 != 0) {     // head_dim 96: the engine makes no such offer (engine.hip, cc_attn)
      return fail(MI_ERR_UNSUPPORTED, "attention_decode: partial q|k|v rows need head_dim 64 or 128");
    } else if constexpr (sizeof(T) == 4) {
      if (c.qkv_pub_sq == nullptr || c.qkv_ksplit < 2 || c.qkv_ksplit > 8 || s.B > 8 || c.hidden_k <= 0)
        return fail(MI_ERR_INVALID, "attention_decode: partial q|k|v rows need 2..8 K slices and at most 8 sequences");
      return launch_mfma_qs_n<D, G, NORM, PAGED>(c, grid, st AT_TRACE_ARG);
    } else {
      return fail(MI_ERR_INVALID, "attention_decode: partial q|k|v rows need float32 activations");
    }
  }
  auto kern = attn_decode_mfma_kernel<T, D, G, NORM, PAGED>;
  constexpr size_t lds = attn_mfma_lds_total<G, D, (int)sizeof(T)>();
  MI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, dim3(NWV * 64), lds, st, c AT_TRACE_ARG);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// the widths of the matrix-core kernel; the float32 one has head_dim 96 in its 16-block form (G <= 4), which the three groups
// served at that width (attn_dispatch.h) all take
template <typename T, int D>
constexpr bool attn_mfma_ok() { return (sizeof(T) == 2 && D % 32 == 0) || (sizeof(T) == 4 && (D % 64 == 0 || D == 96)); }

template <typename T, int D, bool NORM>
int launch_gn(const AttnDecodeCall& c, hipStream_t st) {
  const AttnShape& s = c.s;
  if constexpr (attn_mfma_ok<T, D>()) {
    if (c.variant != 1)
      return attn_dispatch<D>("attention", s, [&](auto g, auto paged) { return launch_mfma_g<T, D, g(), NORM, paged()>(c, st); });
  }
  if (c.qkv_pub != nullptr) return fail(MI_ERR_INVALID, "attention_decode: partial q|k|v rows are read by the float32 MFMA kernel only");
  const dim3 grid(c.nsplit, s.B * s.Hkv), block(512);
  return attn_dispatch<D>("attention", s, [&](auto g, auto paged) {
    hipLaunchKernelGGL((attn_decode_kernel<T, D, g(), NORM, paged()>), grid, block, 0, st, c);
    MI_HIP(hipGetLastError());
    return MI_OK;
  });
}

template <typename T, int D>
int launch_g(const AttnDecodeCall& c, hipStream_t st) {
  const bool norm = c.q_norm_w != nullptr && c.k_norm_w != nullptr;
  if ((c.q_norm_w != nullptr) != (c.k_norm_w != nullptr)) return fail(MI_ERR_INVALID, "attention_decode: q_norm and k_norm must come together");
  return norm ? launch_gn<T, D, true>(c, st) : launch_gn<T, D, false>(c, st);
}

template <typename T>
int launch_d(const AttnDecodeCall& c, hipStream_t st) {
  switch (c.s.D) {
    case 16: if constexpr (sizeof(T) == 4) return launch_g<T, 16>(c, st); break;
    case 32: return launch_g<T, 32>(c, st);
    case 64: return launch_g<T, 64>(c, st);
    case 96: return launch_g<T, 96>(c, st);
    case 128: return launch_g<T, 128>(c, st);
  }
  return fail(MI_ERR_UNSUPPORTED, "attention_decode: head_dim not supported by the fused kernel");
}

}  // namespace

bool attention_decode_supported(const AttnShape& s) {
  if (s.L != 1 || s.act != s.kv) return false;
  if (!attn_group_ok(s.D, s.Hkv > 0 ? s.Hq / s.Hkv : 0)) return false;
  if (s.D == 16) return s.act == MI_F32;
  return s.D == 32 || s.D == 64 || s.D == 96 || s.D == 128;
}

int launch_attention_decode(const AttnDecodeCall& c, hipStream_t st) {
  const AttnShape& s = c.s;
  if (!attention_decode_supported(s)) return fail(MI_ERR_UNSUPPORTED, "attention_decode: shape / dtype not supported");
  if (c.nsplit < 1 || (c.nsplit > 1 && c.partial == nullptr))
    return fail(MI_ERR_INVALID, "attention_decode: bad split configuration");
  if (s.act == MI_F32) return launch_d<float>(c, st);
  if (s.act == MI_BF16) return launch_d<bf16>(c, st);
  return launch_d<f16>(c, st);
}

}  // namespace mi
