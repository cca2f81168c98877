// sampler.hip -- the device sampler: greedy / temperature / top-p / top-k / min-p draw, logit_bias, logprobs and their top entries.
#include <type_traits>

#include "kernels.h"

namespace mi {

namespace {

// ------------------------------------------------------------------------------------------
// Sampler: the `sample` closure of generate_step (utils.py:345-364) + top_p_sampling
// (sample_utils.py:3-38).  One 1024-thread workgroup per row; logits stay in L2.
//   greedy: argmax, lowest index among ties (mx.argmax).
//   temp>0: candidates in descending-probability order (ties: ascending id); nucleus keeps the
//           prefix whose INCLUSIVE cumulative probability is <= top_p (empty -> top-1, quirk Q5);
//           the draw is an inverse-CDF pick with one uniform per row.
//   top_k / min_p: two more prefixes of the same order.  top-k keeps the first k candidates (a cut inside
//           a tie group keeps its lowest ids); the nucleus is then cut against top_p * Z_k, Z_k = the mass of those k;
//           min-p keeps the candidates with (l - max) * (1/T) >= logf(min_p) in float32, i.e. p >= min_p * p_max.  The kept
//           set is the SHORTEST of the three, compared by COUNT (far-tail masses are 0 in fixed point, so a prefix
//           defined by mass can run past the k-th candidate); the draw is the same pick with u * mass(kept).
//   streams: a row with row_position[b] >= 0 draws philox(row_seed[b], row_position[b], 0) -- what the call-wide stream
//           gives row 0 -- whichever index it has in the step; the others keep (seed, step, b).
// Cumulative masses are integers (probability * 2^40 summed with integer atomics), so the
// result does not depend on the order in which threads add.
//
// What the layout of this file owes to measurements ("The default path costs what it did"): the kernel comes in
// six instantiations and the ones without the newer controls (EXT = false) call no part of the draw that the others call -- an
// instantiation that shared the descent with EXT = true measured 1.2 - 6 % slower.  So every helper below that both sides use is
// __forceinline__ or templated on EXT, and find_prefix stays a called function with one copy per EXT.
constexpr int ST = 1024;

// f(value, index) over one row of logits.  A pass is latency-bound if every thread walks it one dependent 4-byte load
// at a time (measured: ~9 us per pass over 32000 logits); 16-byte loads, two in flight per thread.  (Four in flight:
// measured in round 4, no change -- 55.7 us per top-p draw at V = 32000 either way.  What bounds the histogram passes is
// the same-address serialisation of their LDS atomics: a row's logits share a handful of exponents.)
template <class F>
__device__ __forceinline__ void for_row(const float* lg, int V, F f) {
  if ((V & 3) == 0 && (((uintptr_t)lg) & 15) == 0) {
    const float4* p4 = (const float4*)lg;
    const int n4 = V >> 2;
    int i = threadIdx.x;
    for (; i + ST < n4; i += 2 * ST) {
      const float4 a = p4[i], b = p4[i + ST];
      const int j = 4 * i, k = 4 * (i + ST);
      f(a.x, j); f(a.y, j + 1); f(a.z, j + 2); f(a.w, j + 3);
      f(b.x, k); f(b.y, k + 1); f(b.z, k + 2); f(b.w, k + 3);
    }
    if (i < n4) {
      const float4 a = p4[i];
      const int j = 4 * i;
      f(a.x, j); f(a.y, j + 1); f(a.z, j + 2); f(a.w, j + 3);
    }
  } else {
    for (int i = threadIdx.x; i < V; i += ST) f(lg[i], i);
  }
}

__device__ __forceinline__ uint32_t order_key(float f) {  // larger float -> larger key
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct ArgMax { float v; int i; };
__device__ __forceinline__ ArgMax am_better(ArgMax a, ArgMax b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

__device__ __forceinline__ ArgMax block_argmax(ArgMax a, ArgMax* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax b{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)};
    a = am_better(a, b);
  }
  __syncthreads();
  if (lane == 0) sh[wave] = a;
  __syncthreads();
  ArgMax r = sh[0];
  for (int w = 1; w < ST / 64; ++w) r = am_better(r, sh[w]);
  return r;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < ST / 64; ++w) r += sh[w];
  return r;
}

__device__ __forceinline__ unsigned long long mass_fx(float l, float mx, float inv_t) {
  // exp((l - max)/T) in (0, 1] as 2^40 fixed point
  return (unsigned long long)(__expf((l - mx) * inv_t) * 1099511627776.0f);
}

// Philox-4x32-10 (key = seed, counter = (step, row)) -> one uniform in [0,1)
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t step, uint32_t row) {
  uint32_t c0 = (uint32_t)step, c1 = (uint32_t)(step >> 32), c2 = row, c3 = 0x9E3779B9u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * (1.0f / 16777216.0f);
}

// ---- what the helpers pass around ------------------------------------------------------------------------------------------
// The row's invariants: its logits and, once known, their maximum and 1 / T.
struct Row { const float* lg; int V; float mx, inv_t; };

// A prefix of the candidate order: the key of the first element NOT wholly inside it (`kstar`), how many elements with
// key == kstar are inside it (`ntie`), its mass and its number of candidates.
struct Prefix { uint32_t kstar; int ntie; unsigned long long mass; int count; };

// (chunk, wave) entries of the index-ordered walk (tie_count below): 64 chunks of ST lanes, i.e. V <= 65536 ids one per lane
// or 262144 ids four per lane.
constexpr int TIE_TBL = 1024;

// The block's LDS scratch, one object in the kernel.  hist_*: one level of a radix descent; priv_*: the 8 private copies of a
// level-0 histogram; h0_*: the level-0 histogram of the draw's order, built once per row and shared by every descent.
struct Scratch {
  unsigned long long priv_m[256][8], hist_m[256], h0_m[256];
  int priv_c[256][8], hist_c[256], h0_c[256];
  int tie_tbl[TIE_TBL];
  Prefix p;
  ArgMax am[ST / 64];
  float f[ST / 64];
  int i[ST / 64], found;
};

// The two candidate orders, which every walk below is compiled for (DRAW).  The draw's: every value, by order_key, and the walks
// sum masses.  The top entries': the order of the k-round form's float comparisons, which differs from order_key in two places
// -- a NaN is never a candidate (key 0, never counted, never gathered) and -0.0 ties +0.0 by id (both get the key of +0.0; the
// gathered VALUE is kept, its sign reaches the logprob) -- and the walks only count.
__device__ __forceinline__ uint32_t lp_key(float f) {
  if (f != f) return 0u;
  return f == 0.f ? 0x80000000u : order_key(f);
}
template <bool DRAW> __device__ __forceinline__ uint32_t key_of(float f) { return DRAW ? order_key(f) : lp_key(f); }
template <bool DRAW> __device__ __forceinline__ bool is_candidate(uint32_t key) { return DRAW || key != 0u; }

// ---- histograms --------------------------------------------------------------------------------------------------------------
// Level-0 histogram (top 8 key bits) of the whole row into out_c (DRAW: and the masses into out_m).  The logits of one row
// share a few exponents, i.e. a few level-0 bins: the adds are spread over 8 private copies (by lane) to cut the same-address
// serialisation of the LDS atomics, then folded.  No barrier behind the fold: select_bin, which reads it, starts with one.
template <bool DRAW>
__device__ __forceinline__ void level0_hist(const Row& r, Scratch& s, unsigned long long* out_m, int* out_c) {
  // [bin][copy]: the 8 copies of a bin are neighbours, i.e. on different LDS banks ([copy][bin] would put them 2 KiB
  // apart -- all on one bank)
  for (int i = threadIdx.x; i < 8 * 256; i += ST) { if (DRAW) s.priv_m[i >> 3][i & 7] = 0; s.priv_c[i >> 3][i & 7] = 0; }
  __syncthreads();
  const int cp = threadIdx.x & 7;
  for_row(r.lg, r.V, [&](float l, int) {
    const uint32_t key = key_of<DRAW>(l);
    if (DRAW) atomicAdd(&s.priv_m[key >> 24][cp], mass_fx(l, r.mx, r.inv_t));
    if (is_candidate<DRAW>(key)) atomicAdd(&s.priv_c[key >> 24][cp], 1);
  });
  __syncthreads();
  if (threadIdx.x < 256) {
    unsigned long long m = 0; int n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { if (DRAW) m += s.priv_m[threadIdx.x][k]; n += s.priv_c[threadIdx.x][k]; }
    if (DRAW) out_m[threadIdx.x] = m;
    out_c[threadIdx.x] = n;
  }
}

// One lower level of a descent into s.hist_c (DRAW: and s.hist_m): the 8 key bits at `shift` of the candidates whose key has
// `bits` under `mask`.  No barrier behind the walk, as above.
template <bool DRAW>
__device__ __forceinline__ void level_hist(const Row& r, Scratch& s, uint32_t mask, uint32_t bits, int shift) {
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += ST) { if (DRAW) s.hist_m[i] = 0; s.hist_c[i] = 0; }
  __syncthreads();
  for_row(r.lg, r.V, [&](float l, int) {
    const uint32_t k = key_of<DRAW>(l);
    if (is_candidate<DRAW>(k) && (k & mask) == bits) {
      const int bin = (k >> shift) & 255;
      if (DRAW) atomicAdd(&s.hist_m[bin], mass_fx(l, r.mx, r.inv_t));
      atomicAdd(&s.hist_c[bin], 1);
    }
  });
}

// Which bin holds the element at which the descending cumulative mass (starting from `above`) first exceeds
// `target`?  One wave scans the 256 bins from 255 down (4 bins per lane + a wave scan: two block barriers instead of
// a block-wide scan); returns through out: mass / count of everything above that bin, and the bin in ntie (-1: all fits).
// BY_COUNT: `target` is a number of candidates instead -- the bin that holds the candidate with that 0-based position.
// MASS = false (with BY_COUNT): hist_m is not read and out->mass not written.
template <bool BY_COUNT, bool MASS = true>
__device__ __forceinline__ void select_bin(const unsigned long long* hist_m, const int* hist_c, unsigned long long above,
                                           int above_cnt, unsigned long long target, Prefix* out) {
  static_assert(MASS || BY_COUNT, "a mass target needs the masses");
  __syncthreads();
  if (threadIdx.x < 64) {
    const int L = threadIdx.x;
    unsigned long long m[4], tm = 0; int c[4], tc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { m[j] = MASS ? hist_m[255 - (4 * L + j)] : 0ull; c[j] = hist_c[255 - (4 * L + j)]; tm += m[j]; tc += c[j]; }
    unsigned long long im = tm; int ic = tc;                       // inclusive scan over lanes = descending bins
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long om = MASS ? __shfl_up(im, off, 64) : 0ull;
      const int oc = __shfl_up(ic, off, 64);
      if (L >= off) { im += om; ic += oc; }
    }
    unsigned long long cum = above + im - tm; int cnt = above_cnt + ic - tc;
    int pos = 256; unsigned long long pm = 0; int pc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (pos == 256) {
        if (c[j] > 0 && (BY_COUNT ? (unsigned long long)(cnt + c[j]) > target : cum + m[j] > target)) { pos = 4 * L + j; pm = cum; pc = cnt; }
        else { cum += m[j]; cnt += c[j]; }
      }
    }
    int best = pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if (best == 256) { if (L == 63) { if (MASS) out->mass = cum; out->count = cnt; out->ntie = -1; } }
    else if (pos == best) { if (MASS) out->mass = pm; out->count = pc; out->ntie = 255 - best; }
  }
  __syncthreads();
}

// Find the descending-order prefix whose cumulative mass is <= target (radix descent over the order key, 8 bits per
// level; level 0 comes from the cached histogram, the lower levels touch only the elements under the chosen prefix).
// BY_COUNT: the prefix of the first `target` candidates instead (target < V) -- kstar = the key of the candidate at that
// position, ntie = how many candidates of that key lie before it, mass = above + ntie * each like the mass descent.
// (EXT: one copy per instantiation of the kernel, so that the code of the one without the newer controls does not depend on
// what the other one calls.  The descent stays a called function, aligned like a kernel: where its loops fall in the
// instruction cache's lines then does not depend on what the file holds in front of it.)
template <bool EXT, bool BY_COUNT = false>
__device__ __attribute__((aligned(256))) Prefix find_prefix(Row r, unsigned long long target, Scratch* sp) {
  Scratch& s = *sp;
  uint32_t prefix_bits = 0;   // fixed high bits of kstar so far
  uint32_t prefix_mask = 0;
  unsigned long long above = 0;  // mass of keys strictly greater than the current candidate bin
  int above_cnt = 0;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    if (level == 0) {
      select_bin<BY_COUNT>(s.h0_m, s.h0_c, above, above_cnt, target, &s.p);
    } else {
      level_hist<true>(r, s, prefix_mask, prefix_bits, shift);
      select_bin<BY_COUNT>(s.hist_m, s.hist_c, above, above_cnt, target, &s.p);
    }
    above = s.p.mass;
    above_cnt = s.p.count;
    const int bin = s.p.ntie;
    if (bin < 0) {
      __syncthreads();
      Prefix all{0u, 0, above, above_cnt};
      return all;  // the whole (sub)set is inside the prefix
    }
    prefix_bits |= (uint32_t)bin << shift;
    prefix_mask |= 255u << shift;
  }
  // kstar = prefix_bits: all elements with this exact key have the same mass; count how many fit
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long each = mass_fx(__uint_as_float((prefix_bits & 0x80000000u) ? (prefix_bits & 0x7fffffffu) : ~prefix_bits), r.mx, r.inv_t);
    unsigned long long cum = above;
    int n = 0;
    if constexpr (BY_COUNT) { n = (int)target - above_cnt; cum += (unsigned long long)n * each; }
    else while (each > 0 && cum + each <= target) { cum += each; ++n; }
    s.p.mass = cum;
    s.p.ntie = n;
    s.p.count = above_cnt + n;
  }
  __syncthreads();
  Prefix res{prefix_bits, s.p.ntie, s.p.mass, s.p.count};
  __syncthreads();
  return res;
}

// ---- the index-ordered walk ------------------------------------------------------------------------------------------------
// 16-bit logits make big tie groups (hundreds of ids share one value), so "the n-th id of this key" cannot be found by
// trying ids one at a time.  The row is walked once in index order instead, in chunks of PER * ST ids (lane t of chunk j owns
// ids PER * (ST * j + t) .. + PER - 1; PER = 4 with 16-byte loads, else 1): tie_count notes per (chunk, wave) how many ids have
// the key, a single thread scans that small table, and in tie_ranks the wave that owns an entry ranks its ids by prefix ballots.
struct TieWalk {
  const float* lg; int V; bool vec; int nch;
  __device__ __forceinline__ TieWalk(const float* lg_, int V_)
      : lg(lg_), V(V_), vec((V_ & 3) == 0 && (((uintptr_t)lg_) & 15) == 0), nch((V_ + (vec ? 4 : 1) * ST - 1) / ((vec ? 4 : 1) * ST)) {}
  __device__ __forceinline__ int entries() const { return nch * (ST / 64); }
  __device__ __forceinline__ bool fits() const { return entries() <= TIE_TBL; }        // (uniform) the table's capacity rule
  // f(std::integral_constant<int, PER>), PER = the ids per lane: the loops over a chunk are compiled for each width (with the
  // width a run-time value a top-p launch measured 1 - 2.4 % slower: DESIGN.md §2)
  template <class F>
  __device__ __forceinline__ void with_width(F f) const {
    if (vec) f(std::integral_constant<int, 4>{}); else f(std::integral_constant<int, 1>{});
  }
  // this lane's PER ids of chunk j: the first id, whether they lie in the row, and the values
  template <int PER>
  __device__ __forceinline__ int load(int j, float (&v)[PER], bool& in) const {
    const int base = PER * (ST * j + (int)threadIdx.x);
    in = base < V;
    if constexpr (PER == 4) {
      float4 x = {0.f, 0.f, 0.f, 0.f};
      if (in) x = *(const float4*)(lg + base);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = in ? lg[base] : 0.f;
    }
    return base;
  }
};

// tbl[(chunk, wave)] = the number of ids there with the key kstar; other(key, value, id) sees every id of the row.
// Ends with a barrier: the table is complete.
template <bool DRAW, class F>
__device__ __forceinline__ void tie_count(const TieWalk& w, uint32_t kstar, int* tbl, F other) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  w.with_width([&](auto width) {
    constexpr int PER = decltype(width)::value;
    for (int j = 0; j < w.nch; ++j) {
      float v[PER]; bool in;
      const int base = w.template load<PER>(j, v, in);
      int n = 0;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const uint32_t key = key_of<DRAW>(v[e]);
        if (in) other(key, v[e], base + e);
        n += __popcll(__ballot(in && key == kstar));
      }
      if (lane == 0) tbl[j * (ST / 64) + wave] = n;
    }
  });
  __syncthreads();
}

// The wave that owns table entry `at`: hit(rank, value, id) for each of its ids with the key, rank = 0, 1, .. in id order.
template <bool DRAW, class F>
__device__ __forceinline__ void tie_ranks(const TieWalk& w, uint32_t kstar, int at, F hit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave != at % (ST / 64)) return;                         // (uniform over the wave)
  w.with_width([&](auto width) {
    constexpr int PER = decltype(width)::value;
    float v[PER]; bool in;
    const int base = w.template load<PER>(at / (ST / 64), v, in);
    const unsigned long long lt = (1ull << lane) - 1ull;
    bool is[PER];
    int rank = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) { is[e] = in && key_of<DRAW>(v[e]) == kstar; rank += __popcll(__ballot(is[e]) & lt); }
#pragma unroll
    for (int e = 0; e < PER; ++e)
      if (is[e]) { hit(rank, v[e], base + e); ++rank; }
  });
}

// index of the (rank)-th smallest token id among those whose key == kstar; -1: fewer than rank + 1 ties (the caller falls
// back to the arg-max).  A row too long for the tie table takes one walk per tie rank.
__device__ __forceinline__ int nth_tie(const Row& r, uint32_t kstar, int rank, Scratch& s) {
  const TieWalk w(r.lg, r.V);
  if (w.fits()) {
    if (threadIdx.x == 0) s.found = -1;
    tie_count<true>(w, kstar, s.tie_tbl, [](uint32_t, float, int) {});
    if (threadIdx.x == 0) {                       // (chunk, wave) that holds the rank-th tie, and the rank inside it
      int left = rank, at = -1;
      for (int i = 0; i < w.entries(); ++i) {
        const int n = s.tie_tbl[i];
        if (left < n) { at = i; break; }
        left -= n;
      }
      s.i[0] = at; s.i[1] = left;
    }
    __syncthreads();
    const int at = s.i[0], left = s.i[1];
    if (at >= 0) tie_ranks<true>(w, kstar, at, [&](int k, float, int id) { if (k == left) s.found = id; });
    __syncthreads();
    const int id = s.found;
    __syncthreads();
    return id;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int last = -1;
  for (int n = 0; n <= rank; ++n) {
    int best = 0x7fffffff;
    for_row(r.lg, r.V, [&](float l, int i) {
      if (i > last && i < best && order_key(l) == kstar) best = i;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    __syncthreads();
    if (lane == 0) s.i[wave] = best;
    __syncthreads();
    best = s.i[0];
    for (int w2 = 1; w2 < ST / 64; ++w2) best = min(best, s.i[w2]);
    last = best;
    __syncthreads();
  }
  return last;
}

// min-p: the candidates with (l - max) * (1/T) >= thr (thr = logf(min_p) <= 0: the arg-max always passes).  The predicate is
// monotone in l, so they are a prefix of the order, whole tie groups; one walk counts them and sums their masses.
__device__ __forceinline__ Prefix min_p_prefix(const Row& r, float thr, Scratch& s) {
  __syncthreads();
  if (threadIdx.x == 0) { s.p.mass = 0; s.p.count = 0; }
  __syncthreads();
  unsigned long long m = 0; int n = 0;
  for_row(r.lg, r.V, [&](float l, int) {
    if ((l - r.mx) * r.inv_t >= thr) { m += mass_fx(l, r.mx, r.inv_t); ++n; }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { m += __shfl_xor(m, o, 64); n += __shfl_xor(n, o, 64); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(&s.p.mass, m); atomicAdd(&s.p.count, n); }
  __syncthreads();
  Prefix res{0u, 0, s.p.mass, s.p.count};
  __syncthreads();
  return res;
}

// ---- top-k logprobs in a bounded number of walks (sample_kernel<*, *, true>) ----------------------------------------------
// The k-round form (top_rounds) walks the row once per entry.  This one finds the key of the k-th candidate by a radix descent
// over counts (8 bits per level, one walk each, at most four), stops descending as soon as everything from the chosen bin
// upwards fits LP_CAND slots, gathers in one more walk, and orders the few gathered candidates by (logit descending, id
// ascending): at most five walks, whatever k.  The order is lp_key's.
constexpr int LP_CAND = 64;
// Smallest per-row count that takes the selection instead of k rounds: the smallest k at which it measured faster in every
// cell of the launch-time table of DESIGN.md §5 (profiles/sampler_rowlp_launch_times.txt; B = 8, µs, rounds / selection --
// V = 32000: k = 3 22.2 / 23.1, k = 4 27.2 / 23.2, k = 20 106.1 / 24.9; V = 151936: k = 3 72.1 / 70.5, k = 4 90.1 / 70.7,
// k = 20 378.3 / 72.6.  A round costs one walk, the selection three on ordinary rows).
constexpr int LP_SELECT_MIN_K = 4;

// logprobs are reported as (lg - mx) * scale - lse: the plain log-softmax, or the one of logits / T
struct LpTerms { float scale, lse; };
__device__ __forceinline__ float lp_value(float v, float mx, LpTerms lp) { return (v - mx) * lp.scale - lp.lse; }

// Writes out_ids / out_lp [0, k) of one row; false (nothing written): the row is too long for the tie table and the caller
// runs the k-round form (V not a multiple of 4 above 65536 ids, or above 262144).
__device__ bool lp_select_topk(Row r, LpTerms lp, int k, int32_t* out_ids, float* out_lp, Scratch* sp) {
  __shared__ float cand_v[LP_CAND];
  __shared__ int cand_i[LP_CAND], cand_n;
  __shared__ int te_at[MI_MAX_TOP_LOGPROBS], te_first[MI_MAX_TOP_LOGPROBS], te_take[MI_MAX_TOP_LOGPROBS], te_n;
  Scratch& s = *sp;
  const int tid = threadIdx.x;
  const TieWalk w(r.lg, r.V);
  if (!w.fits()) return false;                                // (uniform)
  auto gather = [&](float v, int id) {
    const int at = atomicAdd(&cand_n, 1);
    if (at < LP_CAND) { cand_v[at] = v; cand_i[at] = id; }
  };
  __syncthreads();
  if (tid == 0) { cand_n = 0; te_n = 0; }
  level0_hist<false>(r, s, nullptr, s.hist_c);      // walk 1
  select_bin<true, false>(nullptr, s.hist_c, 0ull, 0, ~0ull, &s.p);   // target past the end: the number of candidates
  const int ke = min(k, s.p.count);                           // entries past the last comparable logit are filler
  uint32_t bits = 0, mask = 0;
  int above = 0, binc = 0;
  bool exact = true;
  if (ke > 0) {
    for (int level = 0; level < 4; ++level) {
      const int shift = 24 - 8 * level;
      if (level > 0) level_hist<false>(r, s, mask, bits, shift);
      select_bin<true, false>(nullptr, s.hist_c, 0ull, above, (unsigned long long)(ke - 1), &s.p);
      above = s.p.count;
      const int bin = max(s.p.ntie, 0);                       // (ke - 1 < the count: a bin is always found)
      binc = s.hist_c[bin];
      bits |= (uint32_t)bin << shift;
      mask |= 255u << shift;
      if (above + binc <= LP_CAND) { exact = false; break; }  // everything from this bin upwards fits the list
    }
    if (!exact) {                                             // gather walk: every candidate with key >= the bin's first key
      const uint32_t ge = max(bits, 1u);
      for_row(r.lg, r.V, [&](float l, int i) { if (lp_key(l) >= ge) gather(l, i); });
    } else {
      // gather walk in index order: the candidates above kstar = bits go to the list (above < ke of them), the ties of kstar
      // are counted per (chunk, wave); the first ke - above of them by id follow
      const uint32_t kstar = bits;
      tie_count<false>(w, kstar, s.tie_tbl, [&](uint32_t key, float v, int id) { if (key > kstar) gather(v, id); });
      if (tid == 0) {                                         // the (chunk, wave) entries that hold the first ke - above ties
        int left = ke - above, m = 0;
        for (int i = 0; i < w.entries() && left > 0 && m < MI_MAX_TOP_LOGPROBS; ++i) {
          const int n = s.tie_tbl[i];
          if (n > 0) { const int take = min(n, left); te_at[m] = i; te_first[m] = ke - above - left; te_take[m] = take; ++m; left -= take; }
        }
        te_n = m;
      }
      __syncthreads();
      const int m = te_n;
      for (int x = 0; x < m; ++x)
        tie_ranks<false>(w, kstar, te_at[x], [&](int rank, float v, int id) {
          if (rank < te_take[x]) {
            const int pos = above + te_first[x] + rank;       // < ke
            out_ids[pos] = id;
            out_lp[pos] = lp_value(v, r.mx, lp);
          }
        });
    }
    __syncthreads();
    const int n = min(cand_n, LP_CAND);
    if (tid < n) {                                            // rank among the gathered: (logit descending, id ascending)
      const float v = cand_v[tid]; const int id = cand_i[tid];
      int rank = 0;
      for (int u = 0; u < n; ++u) rank += (cand_v[u] > v || (cand_v[u] == v && cand_i[u] < id)) ? 1 : 0;
      if (rank < ke) { out_ids[rank] = id; out_lp[rank] = lp_value(v, r.mx, lp); }
    }
  }
  if (tid >= ke && tid < k) {                                 // what a k-round arg-max without candidates reports
    out_ids[tid] = 0;
    out_lp[tid] = lp_value(-INFINITY, r.mx, lp);
  }
  __syncthreads();
  return true;
}

// ---- the stages of sample_kernel, in its order -----------------------------------------------------------------------------
// lg[ids[i]] += vals[i] for the n entries of one list (utils.py:346-349).  The barrier also orders a second list behind this
// one: an id in both gets both, in this order.
__device__ __forceinline__ void add_bias(float* lg, int V, const int32_t* ids, const float* vals, int n, int rnd) {
  for (int i = threadIdx.x; i < n; i += ST) {
    const int id = ids[i];
    if (id >= 0 && id < V) lg[id] = round_rt(lg[id] + vals[i], rnd);
  }
  __syncthreads();
}

// The row of the per-row tables (SampleCall::rb_*, lp_*) that holds the settings of sampled row b; -1: none.
__device__ __forceinline__ int table_row(const SampleCall& c, int b) {
  const int t = c.rb_map ? c.rb_map[b] : b;
  return (t >= 0 && t < c.rb_rows) ? t : -1;
}

// 1. bias: the call-wide list, then the list of the request that holds this row's cache row (a row without one reads only
// its count)
template <bool ROWB, bool ROWLP>
__device__ __forceinline__ void stage_bias(const SampleCall& c, float* lg, int t) {
  if (c.n_bias > 0) add_bias(lg, c.V, c.bias_ids, c.bias_vals, c.n_bias, c.rnd);
  if constexpr (ROWB) {
    const int n = (t >= 0 && (!ROWLP || c.rb_cnt)) ? min(c.rb_cnt[t], c.rb_cap) : 0;
    if (n > 0)             // (uniform over the block)
      add_bias(lg, c.V, c.rb_ids + (size_t)t * c.rb_cap, c.rb_vals + (size_t)t * c.rb_cap, n, c.rnd);
  }
}

// 2. row statistics: max / argmax and the sum of exp(l - max)
struct RowStats { ArgMax a; float se; };
__device__ __forceinline__ RowStats stage_stats(const float* lg, int V, Scratch& s) {
  ArgMax a{-INFINITY, 0x7fffffff};
  for_row(lg, V, [&](float l, int i) { a = am_better(a, ArgMax{l, i}); });
  a = block_argmax(a, s.am);
  const float mx = a.v;
  float se = 0.f;
  for_row(lg, V, [&](float l, int) { se += __expf(l - mx); });
  se = block_sum(se, s.f);
  return RowStats{a, se};
}

// 3. the draw at temperature 1 / r.inv_t: the kept set (the shortest of the top-k, nucleus and min-p prefixes), the inverse-CDF
// pick inside it, and the id of the picked (key, tie rank).  -> the token, or an id outside [0, V) when there is none.
template <bool EXT>
__device__ __forceinline__ int stage_draw(const SampleCall& c, int b, const Row& r, float top_p, Scratch& s) {
  // total mass Z (integer) = sum of the level-0 histogram, which every descent below reuses
  level0_hist<true>(r, s, s.h0_m, s.h0_c);
  select_bin<false>(s.h0_m, s.h0_c, 0ull, 0, ~0ull, &s.p);       // target = +inf: everything fits
  Prefix all{0u, 0, s.p.mass, s.p.count};
  const unsigned long long Z = all.mass;
  Prefix kept = all;
  uint32_t keep_key = 0; int keep_tie = 0x7fffffff;
  bool by_count = false;     // kept was cut by top-k / min-p: its last candidate is known by position, not by (key, tie)
  if constexpr (EXT) {
    const int top_k = c.row_top_k ? c.row_top_k[b] : c.top_k;
    if (top_k > 0 && top_k < all.count) {     // the first top_k candidates: kept.count = top_k, kept.mass = Z_k
      kept = find_prefix<EXT, true>(r, (unsigned long long)top_k, &s);
      by_count = true;
    }
  }
  if (top_p > 0.f && top_p < 1.f) {
    // (EXT: against top_p * Z_k, the nucleus of the top-k survivors; kept.mass == Z without top-k)
    const unsigned long long tgt = (unsigned long long)((double)top_p * (double)(EXT ? kept.mass : Z));
    Prefix nuc = find_prefix<EXT>(r, tgt, &s);
    uint32_t nuc_key = nuc.kstar; int nuc_tie = nuc.ntie;
    if (nuc.count == 0) {  // top token alone exceeds top_p (reference: 0/0); keep top-1
      nuc.count = 1; nuc.mass = mass_fx(r.mx, r.mx, r.inv_t);
      nuc_key = order_key(r.mx); nuc_tie = 1;
    }
    if (!EXT || nuc.count < kept.count) { kept = nuc; keep_key = nuc_key; keep_tie = nuc_tie; by_count = false; }
  }
  if constexpr (EXT) {
    const float min_p = c.row_min_p ? c.row_min_p[b] : c.min_p;
    if (min_p > 0.f) {
      const Prefix mp = min_p_prefix(r, logf(min_p), s);
      // (a count of 0 is a threshold above the arg-max, min_p > 1: off)
      if (mp.count > 0 && mp.count < kept.count) { kept.count = mp.count; kept.mass = mp.mass; by_count = true; }
    }
  }
  float u;
  if (c.uniforms) u = c.uniforms[b];
  else if (EXT && c.row_position && c.row_position[b] >= 0) u = philox_uniform(c.row_seed[b], (uint64_t)c.row_position[b], 0u);
  else u = philox_uniform(c.seed, c.step, (uint32_t)b);
  // first candidate whose inclusive cumulative mass exceeds u * Z_kept
  unsigned long long y = (unsigned long long)((double)u * (double)kept.mass);
  if (y >= kept.mass) y = kept.mass - 1;
  Prefix pk = find_prefix<EXT>(r, y, &s);
  // pk.count candidates lie strictly before the pick; the pick is the next one in order
  int rank_in_key = pk.ntie;
  uint32_t key = pk.kstar;
  if (pk.count >= kept.count) {  // numerical corner: clamp to the last kept candidate
    key = keep_key; rank_in_key = max(keep_tie - 1, 0);
    if (keep_tie == 0x7fffffff) { key = pk.kstar; rank_in_key = max(pk.ntie - 1, 0); }
    if (EXT && by_count) {       // ... which is the candidate at position kept.count - 1
      const Prefix last = find_prefix<EXT, true>(r, (unsigned long long)(kept.count - 1), &s);
      key = last.kstar; rank_in_key = last.ntie;
    }
  }
  return nth_tie(r, key, rank_in_key, s);
}

// 4. the terms of the reported logprobs: the plain log-softmax, or the one of logits / T for a row that asks for it
__device__ __forceinline__ LpTerms stage_lp_terms(const Row& r, float se, float lse, float temperature, int lp_temp, Scratch& s) {
  LpTerms lp{1.0f, lse - r.mx};
  if (lp_temp && temperature > 0.f) {
    lp.scale = 1.0f / temperature;
    float st = se;                               // T = 1: the sum of the pass above, term for term (no second walk of the row)
    if (lp.scale != 1.0f) {                      // (uniform)
      st = 0.f;
      for_row(r.lg, r.V, [&](float l, int) { st += __expf((l - r.mx) * lp.scale); });
      st = block_sum(st, s.f);
    }
    lp.lse = __logf(st);
  }
  return lp;
}

// 5. the top entries, k rounds of arg-max with exclusion of already emitted ids
__device__ __forceinline__ void top_rounds(const Row& r, LpTerms lp, int k, int32_t* out_ids, float* out_lp, Scratch& s) {
  float prev_v = INFINITY; int prev_i = -1;
  for (int n = 0; n < k; ++n) {
    ArgMax t{-INFINITY, 0x7fffffff};
    for_row(r.lg, r.V, [&](float v, int i) {
      if (v < prev_v || (v == prev_v && i > prev_i)) t = am_better(t, ArgMax{v, i});
    });
    t = block_argmax(t, s.am);
    if (threadIdx.x == 0) {
      out_ids[n] = t.i < r.V ? t.i : 0;
      out_lp[n] = lp_value(t.v, r.mx, lp);
    }
    prev_v = t.v; prev_i = t.i;
  }
}

// EXT = false: temperature / top-p with the call-wide stream, the launch of every call that sets none of the newer controls
// (its code does not change when they do).  EXT = true: + top-k, min-p and per-row streams.  ROWB = true: + the per-row
// logit_bias table (SampleCall::rb_*), launched only when the call carries one.  ROWLP = true (with ROWB; the bias table may
// then be absent): + the per-row logprobs settings (SampleCall::lp_*): a row's own count of top entries and its own
// at-temperature flag, the top-k arrays at the fixed stride c.topk_stride, and lp_select_topk for the rows it pays for.
template <bool EXT, bool ROWB = false, bool ROWLP = false>
__global__ __launch_bounds__(ST) void sample_kernel(SampleCall c) {
  __shared__ Scratch s;
  const int b = blockIdx.x, V = c.V;
  float* lg = c.logits + (size_t)b * V;
  // per-row sampling parameters (continuous batching: every request keeps its own) or the call's scalars
  const float temperature = c.row_temp ? c.row_temp[b] : c.temperature;
  const float top_p = c.row_top_p ? c.row_top_p[b] : c.top_p;
  const int t = ROWB ? table_row(c, b) : -1;

  stage_bias<ROWB, ROWLP>(c, lg, t);
  const RowStats rs = stage_stats(lg, V, s);
  Row r{lg, V, rs.a.v, 0.f};
  const float lse = r.mx + __logf(rs.se);
  if (threadIdx.x == 0 && c.row_stats) { c.row_stats[2 * b] = r.mx; c.row_stats[2 * b + 1] = lse; }

  int token = rs.a.i;
  const int forced = c.forced ? c.forced[b] : 0;
  if (c.forced) {
    if (forced >= 0 && forced < V) token = forced;
  } else if (temperature != 0.f) {
    r.inv_t = 1.0f / temperature;
    token = stage_draw<EXT>(c, b, r, top_p, s);
    if (token < 0 || token >= V) token = rs.a.i;
  }
  int top_n = c.top_logprobs, lp_temp = c.lp_temp;   // this row's count of top entries and its at-temperature flag
  if constexpr (ROWLP)
    if (t >= 0 && c.lp_k[t] >= 0) { top_n = min(c.lp_k[t], c.topk_stride); lp_temp = c.lp_flag[t]; }
  const LpTerms lp = stage_lp_terms(r, rs.se, lse, temperature, lp_temp, s);
  // a row without a single comparable logit (all NaN / -inf: a broken checkpoint, an overflow upstream) has no
  // arg-max; it yields token 0 rather than an id that the next kernels would use as an address
  if (token < 0 || token >= V) token = 0;
  if (threadIdx.x == 0) {
    c.tokens_out[b] = token;
    if (c.logprob_out) c.logprob_out[b] = (c.forced && forced < 0) ? 0.f : lp_value(lg[token], r.mx, lp);
  }
  const int tk_stride = ROWLP ? c.topk_stride : c.top_logprobs;
  int32_t* top_ids = c.topk_ids + (size_t)b * tk_stride;
  float* top_lp = c.topk_logprobs + (size_t)b * tk_stride;
  if constexpr (ROWLP) {   // entries past the row's count: (-1, -inf); the row's own entries by the selection where it pays
    for (int n = top_n + (int)threadIdx.x; n < tk_stride; n += ST) { top_ids[n] = -1; top_lp[n] = -INFINITY; }
    if (top_n > 0 && (c.lp_method == 2 || (c.lp_method == 0 && top_n >= LP_SELECT_MIN_K)) &&
        lp_select_topk(r, lp, top_n, top_ids, top_lp, &s))
      top_n = 0;
  }
  if (top_n > 0) top_rounds(r, lp, top_n, top_ids, top_lp, s);
}

// probs = softmax(logits)[0, tokens] (utils.py:363, row-0 quirk Q6)
__global__ void prob_row0_kernel(const float* logits, const float* row_stats, const int32_t* tokens, float* out, int B) {
  const int b = threadIdx.x;
  if (b < B) out[b] = __expf(logits[tokens[b]] - row_stats[1]);
}

}  // namespace

int launch_sample(const SampleCall& c, hipStream_t st) {
  const bool rowlp = c.lp_k != nullptr, rowb = rowlp || c.rb_cnt != nullptr;
  if (c.top_logprobs < 0 || c.top_logprobs > MI_MAX_TOP_LOGPROBS) return fail(MI_ERR_INVALID, "sample: top_logprobs out of range");
  if (rowlp && (!c.lp_flag || c.rb_rows < 1 || c.topk_stride < 1 || c.topk_stride > MI_MAX_TOP_LOGPROBS || c.top_logprobs > c.topk_stride ||
                !c.topk_ids || !c.topk_logprobs || c.lp_method < 0 || c.lp_method > 2))
    return fail(MI_ERR_INVALID, "sample: incomplete row logprobs settings");
  if (c.rb_cnt && (!c.rb_ids || !c.rb_vals || c.rb_rows < 1 || c.rb_cap < 1)) return fail(MI_ERR_INVALID, "sample: incomplete row bias table");
  // one of the six instantiations: EXT on its own, and (ROWB, ROWLP) in {(0, 0), (1, 0), (1, 1)}
  const bool ext = c.top_k > 0 || c.min_p > 0.f || c.row_top_k || c.row_min_p || c.row_position;
  auto launch = [&](auto rb, auto rl) {
    if (ext) hipLaunchKernelGGL((sample_kernel<true, decltype(rb)::value, decltype(rl)::value>), dim3(c.B), dim3(ST), 0, st, c);
    else hipLaunchKernelGGL((sample_kernel<false, decltype(rb)::value, decltype(rl)::value>), dim3(c.B), dim3(ST), 0, st, c);
  };
  if (rowlp) launch(std::true_type{}, std::true_type{});
  else if (rowb) launch(std::true_type{}, std::false_type{});
  else launch(std::false_type{}, std::false_type{});
  MI_HIP(hipGetLastError());
  if (c.prob_row0_out) {
    hipLaunchKernelGGL(prob_row0_kernel, dim3(1), dim3(64 * ((c.B + 63) / 64)), 0, st, c.logits, c.row_stats,
                       c.tokens_out, c.prob_row0_out, c.B);
    MI_HIP(hipGetLastError());
  }
  return MI_OK;
}

}  // namespace mi
