// kv_blocks_adapter_test.cpp -- the seeded prefix chains of mi::KvBlocks (csrc/kv_blocks.h) on the CPU, meant for
// -fsanitize=address,undefined: K / V blocks depend on the adapter of the row that made them, so attach and publish start a
// row's hash chain from adapter_seed(slot, generation) and a row without an adapter from 0.  Directed cases on a 12-block pool
// of 16-token blocks, then a seeded random walk (ensure / release / attach / publish under changing seeds) against a naive
// model whose cache is keyed by (seed, token prefix).  One "ok ..." line per check; the first failed check prints "FAIL ..."
// and exits 1.  tests/test_kv_adapter_host.py builds and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "kv_blocks.h"

using mi::KvBlocks;
using Toks = std::vector<int32_t>;
using E = KvBlocks::Ensure;

static int n_checks = 0;
static void check(bool ok, const char* what, int line) {
  if (!ok) { printf("FAIL line %d: %s\n", line, what); exit(1); }
  printf("ok %d: %s\n", line, what);
  ++n_checks;
}
#define CHECK(cond) check((cond), #cond, __LINE__)
#define REQUIRE(cond) do { if (!(cond)) { printf("FAIL line %d, op %d: %s\n", __LINE__, op_no, #cond); exit(1); } } while (0)

constexpr int BS = 16, ROWS = 4, STRIDE = 4, NBLK = 12;
static KvBlocks fresh() { KvBlocks b; b.init(ROWS, BS, NBLK, BS * STRIDE); return b; }
static int tab(const KvBlocks& b, int row, int i) { return b.h_btab[(size_t)row * b.bt_stride + i]; }
static Toks seq(int k, int n) { Toks t(n); for (int i = 0; i < n; ++i) t[i] = 1000 * k + i; return t; }
static int64_t stat(const KvBlocks& b, int i) { int64_t s[7]; b.stats(s, 7); return s[i]; }
enum { FREE = 0, TOTAL, CACHED, HIT, LOOKUP, EVICTIONS, EVICTABLE };
static uint64_t S(int slot, uint32_t gen) { return KvBlocks::adapter_seed(slot, gen); }

static void directed() {
  {  // the seeds: never 0, one per (slot, generation)
    std::set<uint64_t> seen;
    bool nonzero = true;
    for (int slot = 0; slot < 16; ++slot)
      for (uint32_t gen : {0u, 1u, 2u, 1000u, 0xffffffffu}) { const uint64_t s = S(slot, gen); nonzero = nonzero && s != 0; seen.insert(s); }
    CHECK(nonzero && seen.size() == 16 * 5);
  }
  const Toks P = seq(1, 40);
  {  // published under adapter 0: found under (0, same generation) alone
    KvBlocks b = fresh();
    b.ensure(0, 40); b.publish(0, P.data(), 40, S(0, 0));
    CHECK(stat(b, CACHED) == 2);
    CHECK(b.attach(1, P.data(), 40, S(0, 0)) == 32 && tab(b, 1, 0) == tab(b, 0, 0) && tab(b, 1, 1) == tab(b, 0, 1));
    b.release_row(1);
    CHECK(b.attach(1, P.data(), 40, S(3, 0)) == 0 && b.row_blocks[1] == 0);       // another adapter
    CHECK(b.attach(1, P.data(), 40, 0) == 0 && b.row_blocks[1] == 0);             // no adapter
    CHECK(b.attach(1, P.data(), 40, S(0, 1)) == 0 && b.row_blocks[1] == 0);       // the slot after a set / clear
    CHECK(b.attach(1, P.data(), 40) == 0);                                       // (the default argument is seed 0)
    CHECK(stat(b, HIT) == 32 && stat(b, LOOKUP) == 5 * 40);
  }
  {  // seed 0 gives the keys of a cache that knows no adapters: a chain published without the argument is found with seed 0
    KvBlocks a = fresh(), b = fresh();
    a.ensure(0, 40); a.publish(0, P.data(), 40);
    b.ensure(0, 40); b.publish(0, P.data(), 40, 0);
    std::set<uint64_t> ka, kb;
    for (auto& e : a.prefix) ka.insert(e.first);
    for (auto& e : b.prefix) kb.insert(e.first);
    CHECK(ka == kb && ka.size() == 2);
    CHECK(a.attach(1, P.data(), 40, 0) == 32 && b.attach(1, P.data(), 40) == 32);
  }
  {  // the same prompt published under three seeds: three chains, three sets of blocks, each found under its own seed
    KvBlocks b = fresh();
    const uint64_t seeds[3] = {0, S(0, 0), S(3, 0)};
    for (int r = 0; r < 3; ++r) { b.ensure(r, 40); b.publish(r, P.data(), 40, seeds[r]); }
    CHECK(stat(b, CACHED) == 6);
    bool own = true;
    for (int r = 0; r < 3; ++r) {
      CHECK(b.attach(3, P.data(), 40, seeds[r]) == 32);
      own = own && tab(b, 3, 0) == tab(b, r, 0) && tab(b, 3, 1) == tab(b, r, 1);
      b.release_row(3);
    }
    CHECK(own);
    CHECK(tab(b, 0, 0) != tab(b, 1, 0) && tab(b, 1, 0) != tab(b, 2, 0) && tab(b, 0, 0) != tab(b, 2, 0));
  }
  {  // a replaced adapter: its chain is unreachable, nothing is cleared, and it leaves through the LRU when blocks run out
    KvBlocks b = fresh();
    b.ensure(0, 40); b.publish(0, P.data(), 40, S(0, 0)); b.release_row(0);
    CHECK(stat(b, CACHED) == 2 && stat(b, EVICTABLE) == 2 && stat(b, FREE) == NBLK - 1 - 2);
    CHECK(b.attach(0, P.data(), 40, S(0, 1)) == 0 && stat(b, CACHED) == 2);        // generation 1 sees nothing of generation 0
    b.ensure(0, 40); b.publish(0, P.data(), 40, S(0, 1));
    CHECK(stat(b, CACHED) == 4);
    b.ensure(1, 64); b.ensure(2, 64);                                           // 3 + 4 + 4 blocks live: the two old ones must go
    CHECK(stat(b, EVICTIONS) == 2 && stat(b, CACHED) == 2 && b.free_blocks.empty());
    b.release_row(1);
    CHECK(b.attach(1, P.data(), 40, S(0, 1)) == 32 && b.attach(3, P.data(), 40, S(0, 0)) == 0);   // the live chain survived
  }
  {  // a chain under one seed is not continued under another: the second block's parent is the first block's key
    KvBlocks b = fresh();
    b.ensure(0, 16); b.publish(0, P.data(), 16, S(0, 0));
    b.ensure(1, 40); b.publish(1, P.data(), 40, S(3, 0));
    CHECK(stat(b, CACHED) == 3);
    CHECK(b.attach(2, P.data(), 40, S(0, 0)) == 16 && tab(b, 2, 0) == tab(b, 0, 0));
    CHECK(b.attach(3, P.data(), 40, S(3, 0)) == 32 && tab(b, 3, 0) == tab(b, 1, 0));
  }
}

// ---- the walk.  Every row has a seed, changed only while the row is empty (mi_kv_set_row_adapter's rule).  The model's cache:
// (seed, token prefix) -> block.
static void walk(unsigned seed, int n_ops) {
  KvBlocks b = fresh();
  std::mt19937 rng(seed);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const uint64_t seeds[4] = {0, S(0, 0), S(0, 1), S(3, 0)};
  using Key = std::pair<uint64_t, Toks>;
  std::map<Key, int> cache;
  std::vector<std::vector<int>> owners(NBLK), rows(ROWS);
  std::vector<Toks> text(ROWS);
  std::vector<int> len(ROWS, 0);
  std::vector<uint64_t> row_seed(ROWS, 0);
  int64_t hit = 0, lookup = 0, evictions = 0, hits_seeded = 0, hits_plain = 0, misses_other_seed = 0;
  int op_no = 0;
  auto cached_block = [&](int blk) { for (auto& kv : cache) if (kv.second == blk) return true; return false; };
  auto model_free = [&] { int n = 0; for (int k = 1; k < NBLK; ++k) n += owners[k].empty() && !cached_block(k); return n; };
  auto model_evictable = [&] { int n = 0; for (auto& kv : cache) n += owners[kv.second].empty(); return n; };
  for (; op_no < n_ops; ++op_no) {
    const int row = rnd(0, ROWS - 1);
    switch (rnd(0, 9)) {
      case 0: case 1: {                                                        // release
        b.release_row(row);
        for (int blk : rows[row]) { auto& o = owners[blk]; o.erase(std::find(o.begin(), o.end(), row)); }
        rows[row].clear(); text[row].clear(); len[row] = 0;
        break;
      }
      case 2: case 3: case 4: {                                                // a new occupant: its seed, then attach
        if (len[row] != 0 || b.row_blocks[row] != 0) break;
        row_seed[row] = seeds[rnd(0, 3)];
        const int n = rnd(1, 64), keep = std::max(0, n - rnd(0, 24));
        Toks t = seq(rnd(1, 2), n);
        for (int i = keep; i < n; ++i) t[i] = rnd(0, 3);
        int want = 0;
        std::vector<int> blocks;
        while (want + BS <= n - 1 && (int)blocks.size() < STRIDE) {
          auto it = cache.find(Key(row_seed[row], Toks(t.begin(), t.begin() + want + BS)));
          if (it == cache.end()) break;
          blocks.push_back(it->second); want += BS;
        }
        if (want == 0 && n > BS)                                               // the prefix exists, under another seed only
          for (uint64_t s : seeds) misses_other_seed += s != row_seed[row] && cache.count(Key(s, Toks(t.begin(), t.begin() + BS)));
        REQUIRE(b.attach(row, t.data(), n, row_seed[row]) == want);
        for (int blk : blocks) owners[blk].push_back(row);
        rows[row] = blocks; text[row] = t; len[row] = want;
        lookup += n; hit += want;
        (row_seed[row] ? hits_seeded : hits_plain) += want > 0;
        break;
      }
      case 5: case 6: case 7: {                                                // ensure to a random length, then "run" to it
        const int target = rnd(len[row], 64);
        const int free_before = model_free();
        const E rc = b.ensure(row, target);
        int handed = 0;
        for (int i = (int)rows[row].size(); i < b.row_blocks[row]; ++i, ++handed) {
          const int blk = tab(b, row, i);
          REQUIRE(blk >= 1 && blk < NBLK && owners[blk].empty());
          if (cached_block(blk)) {                                             // taken from the cache: only once nothing was free
            REQUIRE(handed >= free_before);
            cache.erase(std::find_if(cache.begin(), cache.end(), [&](auto& kv) { return kv.second == blk; }));
            ++evictions;
          }
          owners[blk].push_back(row); rows[row].push_back(blk);
        }
        if (rc == E::EXHAUSTED) { REQUIRE(model_free() == 0 && model_evictable() == 0); break; }
        REQUIRE(rc == E::OK);
        while ((int)text[row].size() < target) text[row].push_back(rnd(0, 3));
        len[row] = std::max(len[row], target);
        break;
      }
      default: {                                                               // publish under the row's seed
        const int n = rnd(std::max(0, len[row] - 8), len[row]);
        b.publish(row, text[row].data(), n, row_seed[row]);
        for (int i = 0; (i + 1) * BS <= n; ++i)
          cache.emplace(Key(row_seed[row], Toks(text[row].begin(), text[row].begin() + (i + 1) * BS)), rows[row][i]);
      }
    }
    // ---- invariants
    for (int blk = 1; blk < NBLK; ++blk) {
      const auto in_free = std::count(b.free_blocks.begin(), b.free_blocks.end(), blk);
      const int refs = (int)owners[blk].size() + (cached_block(blk) ? 1 : 0);
      REQUIRE((in_free == 1 && refs == 0 && b.refcnt[blk] == 0) || (in_free == 0 && refs > 0 && b.refcnt[blk] == refs));
    }
    for (int r = 0; r < ROWS; ++r) {
      REQUIRE(b.row_blocks[r] == (int)rows[r].size());
      for (int i = 0; i < STRIDE; ++i) REQUIRE(tab(b, r, i) == (i < (int)rows[r].size() ? rows[r][i] : 0));
    }
    REQUIRE(stat(b, FREE) == model_free() && stat(b, CACHED) == (int64_t)cache.size() && stat(b, HIT) == hit &&
            stat(b, LOOKUP) == lookup && stat(b, EVICTIONS) == evictions && stat(b, EVICTABLE) == model_evictable());
  }
  CHECK(op_no >= 5000);
  printf("walk: %d ops, attaches that hit under an adapter seed %lld, under seed 0 %lld, misses of a prefix cached under another seed %lld, "
         "evictions %lld\n", op_no, (long long)hits_seeded, (long long)hits_plain, (long long)misses_other_seed, (long long)evictions);
  CHECK(hits_seeded >= 20 && hits_plain >= 5);
  CHECK(misses_other_seed >= 20);
  CHECK(evictions >= 1);
}

int main() {
  directed();
  walk(20261021u, 8000);
  printf("checks %d\n", n_checks);
  return 0;
}
