// kv_blocks_sets_test.cpp -- mi::KvBlocks::shared_sets (csrc/kv_blocks.h) under -fsanitize=address,undefined: which rows of a
// decode step form a set.  One "ok ..." line per check, "FAIL ..." and exit 1 at the first that fails (tests/test_kv_sets_host.py).
#include <cstdio>
#include <cstdlib>

#include "kv_blocks.h"

using mi::KvBlocks;
using Ints = std::vector<int32_t>;

static int n_checks = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); exit(1); } printf("ok %d: %s\n", __LINE__, #c); ++n_checks; } while (0)

constexpr int BS = 16, ROWS = 6, STRIDE = 8, NBLK = 40;
static KvBlocks fresh() { KvBlocks b; b.init(ROWS, BS, NBLK, BS * STRIDE); return b; }
static void fork(KvBlocks& b, int src, int dst, int n) { int s, d; if (b.fork(src, dst, n, &s, &d) != KvBlocks::Ensure::OK) exit(2); }

int main() {
  {  // a fork group of 4 (3 blocks + 5 tokens) and a fifth row that shares only the first block
    KvBlocks b = fresh();
    b.ensure(0, 53);
    for (int r = 1; r < 4; ++r) fork(b, 0, r, 53);
    fork(b, 0, 4, 16);
    b.ensure(4, 53);
    const Ints rows = {0, 1, 2, 3, 4}, lens = {53, 53, 53, 53, 53};
    const uint64_t v0 = b.tab_version;
    KvBlocks::SharedSets s = b.shared_sets(rows.data(), lens.data(), 5, 16);
    CHECK(s.ptr == (Ints{0, 4, 5}) && s.members == (Ints{0, 1, 2, 3, 4}) && s.run == (Ints{48, 0}) && s.max_members == 4 && s.max_run == 48 && s.n_shared == 1);
    // a run below the threshold: no set is formed
    s = b.shared_sets(rows.data(), lens.data(), 5, 49);
    CHECK(s.ptr == (Ints{0, 1, 2, 3, 4, 5}) && s.run == (Ints{0, 0, 0, 0, 0}) && s.max_members == 1 && s.max_run == 0 && s.n_shared == 0);
    // a member leaves: the set shrinks, and the table's version says so
    b.release_row(2);
    CHECK(b.tab_version != v0);
    b.ensure(0, 70);                            // a row's fresh block of its own is no change of what rows share
    CHECK(b.tab_version == v0 + 1 && b.btab_dirty);
    const Ints rows4 = {0, 1, 3, 4}, lens4 = {53, 53, 53, 53};
    s = b.shared_sets(rows4.data(), lens4.data(), 4, 16);
    CHECK(s.ptr == (Ints{0, 3, 4}) && s.members == (Ints{0, 1, 2, 3}) && s.run == (Ints{48, 0}));
  }
  {  // equal LATER blocks (mapped by hand) behind different first blocks share nothing
    KvBlocks b = fresh();
    b.ensure(0, 48);
    b.ensure(1, 16);
    for (int i = 1; i < 3; ++i) { b.h_btab[(size_t)1 * b.bt_stride + i] = b.h_btab[(size_t)0 * b.bt_stride + i]; ++b.refcnt[b.h_btab[i]]; }
    b.row_blocks[1] = 3;
    const Ints rows = {0, 1}, lens = {48, 48};
    const KvBlocks::SharedSets s = b.shared_sets(rows.data(), lens.data(), 2, 16);
    CHECK(s.ptr == (Ints{0, 1, 2}) && s.run == (Ints{0, 0}) && s.max_members == 1);
  }
  printf("checks %d\n", n_checks);
  return 0;
}
