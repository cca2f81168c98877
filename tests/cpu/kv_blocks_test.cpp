// kv_blocks_test.cpp -- mi::KvBlocks (csrc/kv_blocks.h) on the CPU, meant for -fsanitize=address,undefined: directed cases on
// a small pool, then a seeded random walk against a naive model.  One "ok ..." line per check; the first failed check
// prints "FAIL ..." and exits 1.  tests/test_kv_blocks_host.py builds and runs it.
//
// Not reachable from here: the branch of attach / publish where a key is found but its stored tokens or parent differ
// (two prefixes with one 64-bit hash).  It is covered by reading the code; there is no hook to inject a hash.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "kv_blocks.h"

using mi::KvBlocks;
using Toks = std::vector<int32_t>;

static int n_checks = 0;
static void check(bool ok, const char* what, int line) {
  if (!ok) { printf("FAIL line %d: %s\n", line, what); exit(1); }
  printf("ok %d: %s\n", line, what);
  ++n_checks;
}
#define CHECK(cond) check((cond), #cond, __LINE__)
// inside the walk: silent while it holds (the walk ends in a few CHECK lines of its own)
#define REQUIRE(cond) do { if (!(cond)) { printf("FAIL line %d, op %d: %s\n", __LINE__, op_no, #cond); exit(1); } } while (0)

constexpr int BS = 16, ROWS = 4, STRIDE = 4, NBLK = 12;
static KvBlocks fresh() { KvBlocks b; b.init(ROWS, BS, NBLK, BS * STRIDE); return b; }
static int tab(const KvBlocks& b, int row, int i) { return b.h_btab[(size_t)row * b.bt_stride + i]; }
static Toks seq(int k, int n) { Toks t(n); for (int i = 0; i < n; ++i) t[i] = 1000 * k + i; return t; }
static int64_t stat(const KvBlocks& b, int i) { int64_t s[7]; b.stats(s, 7); return s[i]; }
enum { FREE = 0, TOTAL, CACHED, HIT, LOOKUP, EVICTIONS, EVICTABLE };
// `row` publishes the first n tokens of t from blocks of its own and lets go of them: the cache alone holds them afterwards
static void publish_and_release(KvBlocks& b, int row, const Toks& t, int n) {
  b.ensure(row, n); b.publish(row, t.data(), n); b.release_row(row);
}

static void directed() {
  using E = KvBlocks::Ensure;
  {  // the pool as made; ensure
    KvBlocks b = fresh();
    CHECK(b.bs_shift == 4 && b.bt_stride == STRIDE && b.free_blocks.size() == NBLK - 1);
    CHECK(std::count(b.free_blocks.begin(), b.free_blocks.end(), 0) == 0);          // block 0 is never handed out
    CHECK(std::count(b.h_btab.begin(), b.h_btab.end(), 0) == ROWS * STRIDE);         // unassigned entries are 0
    CHECK(b.ensure(0, 1) == E::OK && b.row_blocks[0] == 1);
    CHECK(b.ensure(0, 16) == E::OK && b.row_blocks[0] == 1);
    CHECK(b.ensure(0, 17) == E::OK && b.row_blocks[0] == 2);
    CHECK(b.ensure(0, 64) == E::OK && b.row_blocks[0] == 4 && b.free_blocks.size() == NBLK - 5);
    const std::vector<int32_t> before = b.h_btab;
    CHECK(std::set<int32_t>(before.begin(), before.begin() + 4).size() == 4 && std::count(before.begin(), before.begin() + 4, 0) == 0);
    CHECK(b.ensure(0, 65) == E::TOO_LONG && b.h_btab == before && b.row_blocks[0] == 4);   // the 65th token
    CHECK(b.ensure(1, 64) == E::OK && b.ensure(2, 32) == E::OK && b.ensure(3, 16) == E::OK && b.free_blocks.empty());
    const std::vector<int32_t> full = b.h_btab;
    CHECK(b.ensure(3, 33) == E::EXHAUSTED && b.h_btab == full && b.row_blocks[3] == 1);   // every block held by a live row
    CHECK(stat(b, FREE) == 0 && stat(b, TOTAL) == NBLK - 1 && stat(b, EVICTABLE) == 0);
    b.release_row(0);
    CHECK(b.free_blocks.size() == 4 && b.row_blocks[0] == 0 && tab(b, 0, 0) == 0 && tab(b, 0, 3) == 0);
  }
  {  // attach, publish, clear
    KvBlocks b = fresh();
    const Toks P = seq(1, 49);
    b.ensure(0, 48); b.publish(0, P.data(), 48);
    const int c0 = tab(b, 0, 0), c1 = tab(b, 0, 1), c2 = tab(b, 0, 2);
    CHECK(stat(b, CACHED) == 3 && b.refcnt[c0] == 2 && b.refcnt[c1] == 2 && b.refcnt[c2] == 2);
    CHECK(b.attach(1, P.data(), 48) == 32);                 // not 48: the last token's logits are needed
    CHECK(tab(b, 1, 0) == c0 && tab(b, 1, 1) == c1 && b.row_blocks[1] == 2 && b.btab_dirty);
    CHECK(b.refcnt[c0] == 3 && b.refcnt[c1] == 3 && b.refcnt[c2] == 2);
    CHECK(stat(b, HIT) == 32 && stat(b, LOOKUP) == 48);
    b.release_row(1);
    CHECK(b.refcnt[c0] == 2 && b.refcnt[c1] == 2 && b.free_blocks.size() == NBLK - 4 && stat(b, CACHED) == 3);
    CHECK(b.attach(1, P.data(), 49) == 48 && tab(b, 1, 2) == c2);
    b.release_row(1);
    Toks Q = seq(1, 64); Q[20] = -7;                        // block 1 differs: blocks 2 and 3 hang off another parent
    CHECK(b.attach(1, Q.data(), 64) == 16 && b.row_blocks[1] == 1 && tab(b, 1, 0) == c0);
    b.release_row(1);
    CHECK(b.attach(1, P.data(), 16) == 0 && b.attach(1, P.data(), 17) == 16);   // at least one token is left to run
    b.release_row(1);
    b.release_row(0);                                       // the cache's reference keeps the blocks
    CHECK(b.refcnt[c0] == 1 && b.refcnt[c1] == 1 && b.refcnt[c2] == 1 && b.free_blocks.size() == NBLK - 4);
    b.ensure(2, 48); b.publish(2, P.data(), 48);            // an equal prefix owns the chain already
    CHECK(stat(b, CACHED) == 3 && b.refcnt[tab(b, 2, 0)] == 1 && b.refcnt[tab(b, 2, 2)] == 1 && b.refcnt[c0] == 1);
    b.publish(2, P.data(), 15);                             // no full block
    CHECK(stat(b, CACHED) == 3);
    CHECK(b.attach(3, P.data(), 33) == 32);                 // c0, c1 also a row's; c2 the cache's alone
    const size_t free_before = b.free_blocks.size();
    b.clear_prefix();
    CHECK(b.free_blocks.size() == free_before + 1 && b.free_blocks.back() == c2 && stat(b, CACHED) == 0);
    CHECK(b.refcnt[c0] == 1 && b.refcnt[c1] == 1 && b.refcnt[c2] == 0 && b.lru.empty());
    b.release_row(3);
    CHECK(b.refcnt[c0] == 0 && b.free_blocks.size() == free_before + 3);
  }
  {  // eviction: the deepest block of the least recently used chain first, never a parent before its child
    KvBlocks b = fresh();
    const Toks A = seq(1, 64), B = seq(2, 64);
    b.ensure(0, 48); b.publish(0, A.data(), 48);
    const int a0 = tab(b, 0, 0), a1 = tab(b, 0, 1), a2 = tab(b, 0, 2);
    b.release_row(0);
    b.ensure(0, 32); b.publish(0, B.data(), 32);
    const int b0 = tab(b, 0, 0), b1 = tab(b, 0, 1);
    b.release_row(0);
    CHECK(b.ensure(1, 64) == E::OK && b.ensure(2, 32) == E::OK && b.free_blocks.empty());
    CHECK(stat(b, EVICTABLE) == 5 && stat(b, CACHED) == 5 && stat(b, EVICTIONS) == 0);
    CHECK(b.ensure(2, 48) == E::OK && tab(b, 2, 2) == a2 && stat(b, EVICTIONS) == 1 && stat(b, CACHED) == 4);
    CHECK(b.attach(3, A.data(), 64) == 32 && tab(b, 3, 0) == a0 && tab(b, 3, 1) == a1);   // the parents are still there; A is recent now
    CHECK(stat(b, EVICTABLE) == 2);                         // b0, b1: a0 and a1 are a row's as well
    int took = 0;                                           // one block at a time until nothing can be taken
    std::vector<int> order;
    for (int row : {2, 0, 0, 0}) {
      if (b.ensure(row, (b.row_blocks[row] + 1) * BS) != E::OK) break;
      order.push_back(tab(b, row, b.row_blocks[row] - 1));
      ++took;
    }
    CHECK(took == 2 && order[0] == b1 && order[1] == b0);   // evictable == the takes that succeed with no free block
    CHECK(b.ensure(0, 32) == E::EXHAUSTED && b.refcnt[a0] == 2 && b.refcnt[a1] == 2 && stat(b, CACHED) == 2 && stat(b, EVICTIONS) == 3);
  }
  {  // a block that a row maps is passed over, however old
    KvBlocks b = fresh();
    const Toks A = seq(1, 64), B = seq(2, 64);
    b.ensure(0, 32); b.publish(0, A.data(), 32);            // row 0 keeps its chain (the oldest entries)
    publish_and_release(b, 1, B, 32);
    const int a0 = tab(b, 0, 0), a1 = tab(b, 0, 1);
    CHECK(b.ensure(1, 64) == E::OK && b.ensure(2, 48) == E::OK && b.free_blocks.empty() && stat(b, EVICTABLE) == 2);
    CHECK(b.ensure(2, 64) == E::OK && b.ensure(3, 16) == E::OK && b.ensure(3, 32) == E::EXHAUSTED);
    CHECK(stat(b, CACHED) == 2 && b.refcnt[a0] == 2 && b.refcnt[a1] == 2 && tab(b, 0, 0) == a0 && tab(b, 0, 1) == a1);
  }
}

// ---- the walk.  The model: token-prefix tuple -> block for the cache, one owner list per block, the rows' tables and
// lengths.  Where the struct is free to choose (which block ensure hands out) the model checks that the choice was legal
// (a free block while there is one; else a cached block nobody maps and no cached entry hangs off) and follows it.
static void walk(unsigned seed, int n_ops) {
  KvBlocks b = fresh();
  std::mt19937 rng(seed);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  std::map<Toks, int> cache;
  std::vector<std::vector<int>> owners(NBLK), rows(ROWS);
  std::vector<Toks> text(ROWS);                 // the row's tokens: its prompt, then whatever "ran"
  std::vector<int> len(ROWS, 0);                // tokens in the row's cache (the callers' h_off)
  std::vector<bool> orphan(NBLK, false);        // mapped by several rows when a clear took its cache entry: stays shared until they let go
  int64_t hit = 0, lookup = 0, evictions = 0, exhausted = 0, too_long = 0, multi_hit = 0, rejected_publish = 0, rejected_attach = 0;
  int op_no = 0;
  auto cached_block = [&](int blk) { for (auto& kv : cache) if (kv.second == blk) return true; return false; };
  auto model_free = [&] { int n = 0; for (int k = 1; k < NBLK; ++k) n += owners[k].empty() && !cached_block(k); return n; };
  auto drop_owner = [&](int blk, int row) { auto& o = owners[blk]; o.erase(std::find(o.begin(), o.end(), row)); };
  for (; op_no < n_ops; ++op_no) {
    const int row = rnd(0, ROWS - 1);
    switch (rnd(0, 10)) {
      case 0: case 1: {                                                        // reset_row
        b.release_row(row);
        for (int blk : rows[row]) drop_owner(blk, row);
        rows[row].clear(); text[row].clear(); len[row] = 0;
        break;
      }
      case 2: case 3: case 4: {                                                // attach (the caller's check first)
        if (len[row] != 0 || b.row_blocks[row] != 0) { ++rejected_attach; break; }
        const int n = rnd(1, 64), keep = std::max(0, n - rnd(0, 24));
        Toks t = seq(rnd(1, 3), n);
        for (int i = keep; i < n; ++i) t[i] = rnd(0, 3);                       // a random tail
        int want = 0;
        std::vector<int> blocks;
        while (want + BS <= n - 1 && (int)blocks.size() < STRIDE) {
          auto it = cache.find(Toks(t.begin(), t.begin() + want + BS));
          if (it == cache.end()) break;
          blocks.push_back(it->second); want += BS;
        }
        REQUIRE(b.attach(row, t.data(), n) == want);
        for (int blk : blocks) owners[blk].push_back(row);
        rows[row] = blocks; text[row] = t; len[row] = want;
        lookup += n; hit += want; multi_hit += want >= 2 * BS;
        break;
      }
      case 5: case 6: case 7: {                                                // ensure to a random length, then "run" to it
        const int target = rnd(len[row], 64 + 4 * (rnd(0, 7) == 0));
        const int free_before = model_free();
        const KvBlocks::Ensure rc = b.ensure(row, target);
        if (rc == KvBlocks::Ensure::TOO_LONG) { REQUIRE(target > 64 && b.row_blocks[row] == (int)rows[row].size()); ++too_long; break; }
        int fresh_blocks = 0;
        for (int i = (int)rows[row].size(); i < b.row_blocks[row]; ++i, ++fresh_blocks) {
          const int blk = tab(b, row, i);
          REQUIRE(blk >= 1 && blk < NBLK && owners[blk].empty());
          if (cached_block(blk)) {                                             // an eviction
            REQUIRE(fresh_blocks >= free_before);                              // only once nothing was free
            auto it = std::find_if(cache.begin(), cache.end(), [&](auto& kv) { return kv.second == blk; });
            for (auto& kv : cache)                                             // no entry hangs off the evicted one
              REQUIRE(!(kv.first.size() == it->first.size() + BS && std::equal(it->first.begin(), it->first.end(), kv.first.begin())));
            cache.erase(it);
            ++evictions;
          }
          owners[blk].push_back(row); rows[row].push_back(blk);
        }
        if (rc == KvBlocks::Ensure::EXHAUSTED) { REQUIRE(model_free() == 0); ++exhausted; break; }
        REQUIRE((int)rows[row].size() == std::max((target + BS - 1) / BS, (int)rows[row].size() - fresh_blocks));   // exactly what is needed
        while ((int)text[row].size() < target) text[row].push_back(rnd(0, 3));
        len[row] = std::max(len[row], target);
        break;
      }
      case 8: case 9: {                                                        // publish (the caller's check first)
        const int n = rnd(std::max(0, len[row] - 8), std::min(64, len[row] + 4));
        if (n > len[row]) { ++rejected_publish; break; }
        b.publish(row, text[row].data(), n);
        for (int i = 0; (i + 1) * BS <= n; ++i) cache.emplace(Toks(text[row].begin(), text[row].begin() + (i + 1) * BS), rows[row][i]);
        break;
      }
      default: {                                                               // clear, rarely
        if (rnd(0, 9) != 0) break;
        b.clear_prefix();
        cache.clear();
        for (int blk = 1; blk < NBLK; ++blk) orphan[blk] = owners[blk].size() > 1;
      }
    }
    // ---- invariants
    for (int blk = 1; blk < NBLK; ++blk) {
      const auto in_free = std::count(b.free_blocks.begin(), b.free_blocks.end(), blk);
      const int refs = (int)owners[blk].size() + (cached_block(blk) ? 1 : 0);
      REQUIRE((in_free == 1 && refs == 0 && b.refcnt[blk] == 0) || (in_free == 0 && refs > 0 && b.refcnt[blk] == refs));
      if (owners[blk].size() <= 1) orphan[blk] = false;
      REQUIRE(owners[blk].size() <= 1 || cached_block(blk) || orphan[blk]);    // shared by rows only through the cache
    }
    REQUIRE(std::count(b.free_blocks.begin(), b.free_blocks.end(), 0) == 0);
    for (int r = 0; r < ROWS; ++r) {
      REQUIRE(b.row_blocks[r] == (int)rows[r].size());
      for (int i = 0; i < STRIDE; ++i) REQUIRE(tab(b, r, i) == (i < (int)rows[r].size() ? rows[r][i] : 0));
    }
    int64_t evictable = 0;
    for (auto& kv : cache) evictable += owners[kv.second].empty();
    REQUIRE(stat(b, FREE) == model_free() && stat(b, CACHED) == (int64_t)cache.size() && stat(b, HIT) == hit &&
            stat(b, LOOKUP) == lookup && stat(b, EVICTIONS) == evictions && stat(b, EVICTABLE) == evictable);
  }
  CHECK(op_no >= 5000);
  printf("walk: %d ops, evictions %lld, exhausted %lld, too long %lld, multi-block hits %lld, rejected publishes %lld, rejected attaches %lld\n",
         op_no, (long long)evictions, (long long)exhausted, (long long)too_long, (long long)multi_hit, (long long)rejected_publish, (long long)rejected_attach);
  CHECK(evictions >= 1);
  CHECK(exhausted >= 1);
  CHECK(multi_hit >= 1);
  CHECK(rejected_publish >= 1);
}

int main() {
  directed();
  walk(20261019u, 6000);
  printf("checks %d\n", n_checks);
  return 0;
}
