// attn_shared.hip -- decode attention (L == 1) over a block-paged cache in which rows SHARE leading blocks (forked choices of
// one prompt, rows attached to one published prefix): the shared run of a set of rows is read once per column group, not once
// per row.  q is normed and roped and rope_append has appended the new key and value: row b attends to offsets[b] + 1 keys.
//
// Work split, ONE launch, grid (items, Hkv), 512 threads = 8 waves:
//   * prefix items (set, column group, key chunk of the run): a column group is up to MPG = 16 / G members of the set; MFMA
//     column m * G + g is query head g of member m (columns past nm * G are zero and never stored).  The K / V addresses come
//     from the block table of the set's first member.  A set of more than MPG members is cut into several groups, each of which
//     reads the run again.
//   * tail items (row, key chunk of [run, offsets + 1)): the row's own keys, its G heads in columns 0..G-1.
// The key loop is the one of attn_decode.hip with sixteen live columns: S^T = K Q^T with the K fragments straight from 16-byte
// non-temporal loads of cache rows (A operand) and the column group's Q^T staged once in LDS (B operand), online softmax per
// column in the lane that holds it; 16-bit caches: v_mfma_f32_16x16x32, V through a per-wave LDS image read back with
// ds_read_b64_tr_b16, P as two 16-bit operands (pack2_split); float32 caches: v_mfma_f32_16x16x4_f32, exact products, P in
// float32, no image.
// Every item leaves one (m, l, O[D]) per (row, head) in slot `pc` (prefix chunk) or `prefix slots + tc` (tail chunk) of the
// row's 16 slots [D + 2]; then it takes a ticket of every row it served, and whoever draws a row's last ticket merges that
// row's slots in slot order -- prefix chunks ascending, then tail chunks ascending (combine_splits) -- and writes `out`.
// Nobody waits, no float atomics, the same inputs give the same bits, the tickets are back at zero when the launch ends.
//
// LDS of a workgroup at D = 128 (the CU has 160 KiB):
//   [0, 64 KiB)   16-bit caches: 8 waves x V image [D/16 tiles][32 keys][16 d] x 2 B = 8 KiB each.  Once a wave has left the
//                 key loop its image is dead and the SAME 8 KiB are its merge area [16 columns][D] floats (a wave's DS
//                 operations execute in order and its O depends on its last image reads: no barrier in between);
//                 float32 caches: the merge areas alone
//   + Q^T         16 columns x D x 2 B = 4 KiB (float32: 8 KiB)
//   + (m, l)      2 x 8 waves x 16 columns x 4 B = 1 KiB, + 16 batch indices + 16 last-arriver flags
//   = 69.1 KiB (float32: 73.1 KiB); D = 64: half of the first two.
// Residency: at D = 64 the kernels take 98 - 100 VGPRs and two workgroups share a CU; at D = 128 they take 156 - 162 (the
// 16-column accumulators and a round of K / V in flight), three waves per SIMD where a 512-thread workgroup needs two, so ONE
// workgroup is resident per CU and the aliasing saves LDS without buying residency there.
#include <algorithm>

#include "attn_dispatch.h"
#include "attn_mfma.h"

namespace mi {

namespace {

constexpr int NWV = 8;                           // waves per workgroup
constexpr int SLOTS = 16;                        // partial slots of a (row, head)

template <int D, int ES>
constexpr size_t shared_lds_bytes() { return (size_t)NWV * 64 * D + (size_t)16 * D * ES + (size_t)2 * NWV * 16 * 4 + 2 * 16 * 4; }

template <typename T, int D, int G>
__global__ __launch_bounds__(NWV * 64) void attn_shared_kernel(AttnSharedCall c, int PC, int TC, int CG) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int MPG = 16 / G;                    // members of a column group
  constexpr int KK = D / 32, DT = D / 16, NV = (32 * D * 2) / (64 * 16);   // K steps, 16-d tiles, 16-B V loads per lane
  constexpr int KPW = F32 ? 16 : 32;             // keys per wave and round
  constexpr int NP = D / 16, NH = D / 64;        // float32: 16-byte K pieces per lane and tile, 64-d halves of a V row
  constexpr int PPR = D * (int)sizeof(T) / 16;   // 16-byte pieces of a q row
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const AttnShape& s = c.s;
  const int item = blockIdx.x, kh = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g4 = lane >> 4;     // MFMA view: column / lane group
  const int B = s.B, nsets = c.n_sets;

  // ---- which item (everything here is workgroup-uniform)
  const int nP = c.n_shared * CG * PC;            // prefix items: over the sets that have a run, not over the sets of one
  int p0, nm, run, s0, send, slot, ptab;         // first member's place in set_members | members | shared run | keys | slot | place of the table's row
  if (item < nP) {
    const int si = item / (CG * PC), cg = (item / PC) % CG, pc = item % PC;
    const int a = min(max(c.set_ptr[si], 0), B), e = min(max(c.set_ptr[si + 1], 0), B);
    run = min(c.set_run[si], c.max_run);
    p0 = a + cg * MPG; nm = min(MPG, e - p0); ptab = a;
    if (run <= 0 || nm <= 0) return;             // a set without a run, or fewer column groups than the largest set
    const int chunk = ((run + 16 * PC - 1) / (16 * PC)) * 16;
    s0 = pc * chunk; send = min(s0 + chunk, run); slot = pc;
  } else {
    const int j = item - nP, tc = j % TC;
    p0 = j / TC; nm = 1; ptab = p0;
    int si = 0;
    while (si + 1 < nsets && c.set_ptr[si + 1] <= p0) ++si;
    run = si < c.n_shared ? max(min(c.set_run[si], c.max_run), 0) : 0;
    const int b = min(max(c.set_members[p0], 0), B - 1), row = s.rows ? s.rows[b] : b;
    const int n_keys = c.offsets[row] + 1, len = max(n_keys - run, 0);
    const int chunk = ((len + 16 * TC - 1) / (16 * TC)) * 16;
    s0 = run + tc * chunk; send = min(s0 + chunk, n_keys); slot = (run > 0 ? PC : 0) + tc;
  }
  p0 = __builtin_amdgcn_readfirstlane(p0); nm = __builtin_amdgcn_readfirstlane(nm);
  s0 = __builtin_amdgcn_readfirstlane(s0); send = __builtin_amdgcn_readfirstlane(send);
  slot = __builtin_amdgcn_readfirstlane(slot);
  const int nslots = (run > 0 ? PC : 0) + TC;    // of every row this item serves
  int kb;                                        // the cache row whose block table addresses this item's keys
  {
    const int b = min(max(c.set_members[ptab], 0), B - 1);
    kb = __builtin_amdgcn_readfirstlane(s.rows ? s.rows[b] : b);
  }

  unsigned char* vimg = smem + (size_t)wave * (64 * D);                // this wave's V image, later its merge area
  float* st_o = (float*)smem;                                          // [NWV][16][D]
  T* q_sh = (T*)(smem + (size_t)NWV * 64 * D);                         // [16][D]
  float* st_m = (float*)(smem + (size_t)NWV * 64 * D + (size_t)16 * D * sizeof(T));   // [NWV][16]
  float* st_l = st_m + NWV * 16;
  int* col_b = (int*)(st_l + NWV * 16);                                // [16]: batch index of member m
  int* last_sh = col_b + 16;                                           // [16]: member m's last ticket was drawn here

  const T* kc = (const T*)c.kcache;
  const T* vc = (const T*)c.vcache;

  // ---- the K fragments and V rows of the first round go out before anything else
  u32x4 kf[F32 ? 1 : 2][F32 ? 1 : KK], vrow[F32 ? 1 : NV];
  f32x4 kf32[F32 ? NP : 1], vv32[F32 ? 4 : 1][F32 ? NH : 1];
  const int klast = max(send - 1, 0);            // every address is clamped to a mapped row: no load sits under a branch
  auto issue_k = [&](int base) {                 // keys base + KPW wave + [0, KPW)
    const int k0 = base + KPW * wave;
    if constexpr (F32) {
      const size_t ro = kv_elem<true>(s, kb, kh, min(k0 + c16, klast));
#pragma unroll
      for (int i = 0; i < NP; ++i) kf32[i] = load_kv<f32x4>(kc + ro + 16 * i + 4 * g4);
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const size_t ro = kv_elem<true>(s, kb, kh, min(k0 + 16 * t + c16, klast));
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
        const size_t ro = kv_elem<true>(s, kb, kh, min(k0 + 4 * g4 + r, klast));
#pragma unroll
        for (int h = 0; h < NH; ++h) vv32[r][h] = load_kv<f32x4>(vc + ro + 64 * h + 4 * c16);
      }
    } else {                                     // 32 keys x (D/8) 16-byte pieces, lane-linear: piece = i * 64 + lane
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int piece = i * 64 + lane, kl = piece / (D / 8), dc = piece % (D / 8);
        vrow[i] = load_kv<u32x4>(vc + kv_elem<true>(s, kb, kh, min(k0 + kl, klast)) + 8 * dc);
      }
    }
  };
  issue_k(s0);
  issue_v(s0);

  // ---- Q^T of the column group -> LDS: column m * G + g = head g of member m; the columns past nm * G are zero
  for (int i = tid; i < 16 * PPR; i += NWV * 64) {
    const int col = i / PPR, piece = i % PPR, m = col / G, g = col % G;
    const int b = min(max(c.set_members[p0 + min(m, nm - 1)], 0), B - 1);
    u32x4 v = *(const u32x4*)((const T*)c.q + ((size_t)b * s.Hq + kh * G + g) * D + piece * (16 / (int)sizeof(T)));
    if (m >= nm) v = u32x4{0u, 0u, 0u, 0u};
    *(u32x4*)(q_sh + (size_t)col * D + piece * (16 / (int)sizeof(T))) = v;
    if (piece == 0 && g == 0 && m < MPG) col_b[m] = b;
  }
  const float sc2 = c.scale * LOG2E;
  __syncthreads();
  u32x4 qf[F32 ? 1 : KK];
  f32x4 qf32[F32 ? NP : 1];
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < NP; ++i) qf32[i] = *(const f32x4*)(q_sh + (size_t)c16 * D + 16 * i + 4 * g4);
  } else {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = *(const u32x4*)(q_sh + (size_t)c16 * D + 32 * kk + 8 * g4);
  }

  // ---- rounds of 256 keys per workgroup (float32 caches: 128); m_run / l_run: of column c16 over this lane group's keys
  float m_run = -1e30f, l_run = 0.f;
  f32x4 accO[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) accO[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (F32) {
    // the trip count is the wave's own: a wave whose keys are exhausted neither loads nor multiplies (it merges as (-1e30, 0, 0))
    for (int base = s0; base + KPW * wave < send; base += KPW * NWV) {
      const bool more = base + KPW * NWV + KPW * wave < send;
      f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = mfma_f32(kf32[i][e], qf32[i][e], sc);
      __builtin_amdgcn_sched_barrier(0);
      if (more) issue_k(base + KPW * NWV);
      __builtin_amdgcn_sched_barrier(0);
      const int k0 = base + KPW * wave;
      float mx = -1e30f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[r] = (k0 + 4 * g4 + r) < send ? sc[r] * sc2 : -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));    // max over the wave's 16 keys, per column
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
      if (more) issue_v(base + KPW * NWV);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    for (int base = s0; base < send; base += 32 * NWV) {      // uniform trip count; the prefetch past the end is clamped
      f32x4 sc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) sc[t] = mfma16<T>(kf[t][kk], qf[kk], sc[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
      issue_k(base + 32 * NWV);
      __builtin_amdgcn_sched_barrier(0);
      const int k0 = base + 32 * wave;
      float mx = -1e30f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc[t][r] = (k0 + 16 * t + 4 * g4 + r) < send ? sc[t][r] * sc2 : -INFINITY;
          mx = fmaxf(mx, sc[t][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));    // max over the wave's 32 keys, per column
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
      issue_v(base + 32 * NWV);
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

  // ---- this wave's (m, l, O) of every live column, over its dead V image
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  __builtin_amdgcn_sched_barrier(0);
  if (c16 < nm * G) {
    if (g4 == 0) { st_m[wave * 16 + c16] = m_run; st_l[wave * 16 + c16] = l_run; }
    if constexpr (F32) {                         // tile (h, e), row 4 g4 + r  <->  d = 64 h + 4 (4 g4 + r) + e
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_o[(wave * 16 + c16) * D + 64 * (dt >> 2) + 16 * g4 + 4 * r + (dt & 3)] = accO[dt][r];
    } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_o[(wave * 16 + c16) * D + 16 * dt + 4 * g4 + r] = accO[dt][r];
    }
  }
  __syncthreads();
  // the waves merged in wave order; an item without keys leaves the neutral partial (-inf, 0, 0)
  for (int idx = tid; idx < nm * G * D; idx += NWV * 64) {
    const int col = idx / D, d = idx % D, b = col_b[col / G], h = kh * G + col % G;
    float mn = -1e30f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) mn = fmaxf(mn, st_m[w * 16 + col]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const float cw = __builtin_amdgcn_exp2f(st_m[w * 16 + col] - mn);
      L = fmaf(st_l[w * 16 + col], cw, L);
      O = fmaf(st_o[(w * 16 + col) * D + d], cw, O);
    }
    // published with write-through stores and read back with sc1 loads, as in attn_decode.hip: no fence
    float* pp = c.partial + (((size_t)b * s.Hq + h) * SLOTS + slot) * (D + 2);
    __hip_atomic_store(&pp[2 + d], O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d == 0) {
      __hip_atomic_store(&pp[0], L > 0.f ? mn : -INFINITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&pp[1], L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // ---- every storing wave drains its stores, the workgroup meets, one lane per member takes that row's ticket; whoever
  // draws the last of a (row, kv head) merges the row's slots in slot order
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < nm) {
    int* ctr = c.counters + (size_t)col_b[tid] * s.Hkv + kh;
    const int ticket = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == nslots - 1;
    if (last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    last_sh[tid] = last;
  }
  __syncthreads();
  for (int m = 0; m < nm; ++m) {
    if (!last_sh[m]) continue;
    const int b = col_b[m];
    T* out = (T*)c.out + (size_t)b * s.Hq * D;
    for (int idx = tid; idx < G * D; idx += NWV * 64) {
      const int h = kh * G + idx / D, d = idx % D;
      const float* pp = c.partial + ((size_t)b * s.Hq + h) * SLOTS * (D + 2);
      out[(size_t)h * D + d] = store_act<T>(combine_splits<D>(pp, nslots, d), s.rnd);
    }
  }
}

template <typename T, int D, int G>
int launch_shared_g(const AttnSharedCall& c, hipStream_t st) {
  const AttnShape& s = c.s;
  constexpr int MPG = 16 / G, RK = sizeof(T) == 4 ? 128 : 256;      // members per column group | keys of a workgroup's round
  const int CG = (c.max_members + MPG - 1) / MPG;
  // chunks: one round of keys each, at most 4 for the tails and 12 for the run (16 slots per row), and no more prefix
  // chunks than the resident workgroups take in one wave -- two per CU at D = 64, one at D = 128 (the file comment) --
  // counting the column groups of the rows that share as at most ceil(B / MPG)
  const int TC = std::max(1, std::min((c.max_tail + RK - 1) / RK, 4));
  int PC = std::max(1, std::min((c.max_run + RK - 1) / RK, SLOTS - 4));
  const int cus = gemv_cu_count(), groups = (s.B + MPG - 1) / MPG;
  while (PC > 1 && (groups * PC + s.B * TC) * s.Hkv > (D == 64 ? 2 : 1) * cus) --PC;
  auto kern = attn_shared_kernel<T, D, G>;
  constexpr size_t lds = shared_lds_bytes<D, (int)sizeof(T)>();
  static_assert(lds <= 80 * 1024, "half a CU's LDS");
  MI_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid(c.n_shared * CG * PC + s.B * TC, s.Hkv);
  hipLaunchKernelGGL(kern, grid, dim3(NWV * 64), lds, st, c, PC, TC, CG);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

template <typename T>
int launch_shared_d(const AttnSharedCall& c, hipStream_t st) {
  auto go = [&](auto d) {
    return attn_dispatch<d()>("attention_shared", c.s, [&](auto g, auto) { return launch_shared_g<T, d(), g()>(c, st); });
  };
  return c.s.D == 64 ? go(std::integral_constant<int, 64>{}) : go(std::integral_constant<int, 128>{});
}

}  // namespace

bool attention_shared_supported(const AttnShape& s) {
  if (s.L != 1 || s.btab == nullptr || s.act != s.kv || s.Hkv < 1 || s.Hq % s.Hkv != 0) return false;
  if (s.act != MI_F32 && s.act != MI_BF16 && s.act != MI_F16) return false;
  return (s.D == 64 || s.D == 128) && attn_group_ok(s.D, s.Hq / s.Hkv);
}

int launch_attention_shared(const AttnSharedCall& c, hipStream_t st) {
  const AttnShape& s = c.s;
  if (!attention_shared_supported(s)) return fail(MI_ERR_UNSUPPORTED, "attention_shared: shape / dtype / cache layout not supported");
  if (!c.q || !c.kcache || !c.vcache || !c.offsets || !c.out || !c.partial || !c.counters || !c.set_ptr || !c.set_members || !c.set_run)
    return fail(MI_ERR_INVALID, "attention_shared: null argument");
  if (s.B < 1 || c.n_sets < 1 || c.n_sets > s.B || c.max_members < 1 || c.max_members > s.B || c.n_shared < 0 || c.n_shared > c.n_sets)
    return fail(MI_ERR_INVALID, "attention_shared: 1 <= sets <= rows, 1 <= members of a set <= rows, 0 <= sets with a run <= sets");
  if (c.max_run < 0 || c.max_run > s.cap || (c.max_run & ((1 << s.bs_shift) - 1)) != 0 || c.max_tail < 1 || c.max_tail > s.cap)
    return fail(MI_ERR_INVALID, "attention_shared: the shared run is a multiple of the block size within the row's capacity, a tail has at least the new key");
  if (s.act == MI_F32) return launch_shared_d<float>(c, st);
  if (s.act == MI_BF16) return launch_shared_d<bf16>(c, st);
  return launch_shared_d<f16>(c, st);
}

}  // namespace mi
