// attn_dispatch.h -- the head shapes the attention kernels are built for, stated once, and the one dispatch from the
// run-time (Hq/Hkv, paged cache) to the compile-time (G, PAGED) of a kernel.  Host only.
//
// Which head_dim a kernel family serves is that family's own switch (launch_attn_d, launch_d, launch_pt, the float32
// prefill); which query-head groups G = Hq/Hkv exist at a head_dim is this table, for every family.
#pragma once

#include <string>
#include <type_traits>
#include <utility>

#include "kernels.h"

namespace mi {

// THE TABLE: the groups served at head_dim D, and what a caller is told about any other.
template <int D>
struct AttnGroups : std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8> {
  static constexpr const char* need = ": Hq/Hkv must be 1, 2, 3, 4, 5, 6 or 8";
};
template <>
struct AttnGroups<96> : std::integer_sequence<int, 1, 2, 4> {      // Phi-3's width
  static constexpr const char* need = ": head_dim 96 needs Hq/Hkv of 1, 2 or 4";
};

template <int... Gs>
constexpr bool attn_group_in(std::integer_sequence<int, Gs...>, int G) { return ((G == Gs) || ...); }

// the only predicate on groups (head_dim itself is checked by the caller)
constexpr bool attn_group_ok(int D, int G) {
  return D == 96 ? attn_group_in(AttnGroups<96>{}, G) : attn_group_in(AttnGroups<0>{}, G);
}

// f(std::bool_constant<PAGED>) for the cache of s
template <typename F>
int attn_dispatch_paged(const AttnShape& s, F&& f) {
  return s.btab ? f(std::true_type{}) : f(std::false_type{});
}

template <int D, typename F, int... Gs>
int attn_dispatch_groups(const char* who, const AttnShape& s, F&& f, std::integer_sequence<int, Gs...>) {
  const int G = s.Hq / s.Hkv;
  int rc = MI_OK;
  auto launch = [&](auto g) { rc = attn_dispatch_paged(s, [&](auto paged) { return f(g, paged); }); return true; };
  const bool served = ((G == Gs && launch(std::integral_constant<int, Gs>{})) || ...);   // the first (only) match, no further
  return served ? rc : fail(MI_ERR_UNSUPPORTED, std::string(who) + AttnGroups<D>::need);
}

// f(std::integral_constant<int, G>, std::bool_constant<PAGED>) -> int for the group and cache of s at head_dim D, or
// MI_ERR_UNSUPPORTED "<who>: ..." for a group the table does not have.
template <int D, typename F>
int attn_dispatch(const char* who, const AttnShape& s, F&& f) {
  return attn_dispatch_groups<D>(who, s, f, AttnGroups<D>{});
}

}  // namespace mi
