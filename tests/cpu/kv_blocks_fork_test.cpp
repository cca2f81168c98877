// kv_blocks_fork_test.cpp -- mi::KvBlocks::fork (csrc/kv_blocks.h) on the CPU, meant for -fsanitize=address,undefined: directed
// cases on a 12-block pool of 16-token blocks, then a seeded random walk (ensure / release / attach / publish / fork) against
// a naive model.  One "ok ..." line per check; the first failed check prints "FAIL ..." and exits 1.
// tests/test_kv_fork_host.py builds and runs it.
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
static std::vector<int> sorted_free(const KvBlocks& b) { std::vector<int> f = b.free_blocks; std::sort(f.begin(), f.end()); return f; }

// everything a failed fork must leave alone
struct Snapshot {
  std::vector<int32_t> btab; std::vector<int> row_blocks, refcnt, free_blocks; bool dirty; size_t cached; int64_t evictions;
  explicit Snapshot(const KvBlocks& b) : btab(b.h_btab), row_blocks(b.row_blocks), refcnt(b.refcnt), free_blocks(b.free_blocks),
                                         dirty(b.btab_dirty), cached(b.prefix.size()), evictions(b.stat_evictions) {}
  bool same(const KvBlocks& b) const {
    return btab == b.h_btab && row_blocks == b.row_blocks && refcnt == b.refcnt && free_blocks == b.free_blocks &&
           dirty == b.btab_dirty && cached == b.prefix.size() && evictions == b.stat_evictions;
  }
};

static void directed() {
  for (int n : {1, 15, 16, 17, 32, 33}) {      // a row of 40 tokens (3 blocks, the last one partly filled) gives its first n
    KvBlocks b = fresh();
    b.ensure(0, 40);
    b.btab_dirty = false;
    const int full = n / BS, tail = n % BS, free_before = (int)b.free_blocks.size();
    int sb = -1, db = -1;
    printf("fork n_tokens %d\n", n);
    CHECK(b.fork(0, 1, n, &sb, &db) == E::OK && b.btab_dirty);
    CHECK(b.row_blocks[1] == full + (tail ? 1 : 0) && b.row_blocks[0] == 3 && (int)b.free_blocks.size() == free_before - (tail ? 1 : 0));
    bool shared = true;
    for (int i = 0; i < full; ++i) shared = shared && tab(b, 1, i) == tab(b, 0, i) && b.refcnt[tab(b, 0, i)] == 2;
    CHECK(shared);
    if (tail) CHECK(sb == tab(b, 0, full) && db == tab(b, 1, full) && db != sb && db >= 1 && b.refcnt[db] == 1 && b.refcnt[sb] == 1);
    else CHECK(sb == 0 && db == 0);                        // a multiple of the block size: no block, no copy
    bool rest = true;
    for (int i = b.row_blocks[1]; i < STRIDE; ++i) rest = rest && tab(b, 1, i) == 0;
    for (int i = full; i < 3; ++i) rest = rest && b.refcnt[tab(b, 0, i)] == 1;      // what src keeps for itself
    CHECK(rest);
  }
  {  // a fork of a fork
    KvBlocks b = fresh();
    b.ensure(0, 40);
    int sb, db;
    CHECK(b.fork(0, 1, 33, &sb, &db) == E::OK && sb == tab(b, 0, 2) && db == tab(b, 1, 2));
    CHECK(b.fork(1, 2, 20, &sb, &db) == E::OK && sb == tab(b, 1, 1) && sb == tab(b, 0, 1) && db == tab(b, 2, 1));
    CHECK(tab(b, 2, 0) == tab(b, 0, 0) && b.refcnt[tab(b, 0, 0)] == 3 && b.refcnt[tab(b, 0, 1)] == 2 && b.refcnt[tab(b, 2, 1)] == 1);
    CHECK(b.row_blocks[2] == 2 && b.free_blocks.size() == NBLK - 1 - 3 - 1 - 1);
    b.release_row(1);                                      // the middle one goes: row 2 keeps block 0
    CHECK(b.refcnt[tab(b, 0, 0)] == 2 && b.refcnt[tab(b, 0, 1)] == 1 && tab(b, 2, 0) == tab(b, 0, 0));
    b.release_row(0);
    CHECK(b.refcnt[tab(b, 2, 0)] == 1 && b.free_blocks.size() == NBLK - 1 - 2);
    b.release_row(2);
    CHECK(b.free_blocks.size() == NBLK - 1);
  }
  {  // from a row whose full blocks are published
    KvBlocks b = fresh();
    const Toks P = seq(1, 40);
    b.ensure(0, 40); b.publish(0, P.data(), 40);
    const int c0 = tab(b, 0, 0), c1 = tab(b, 0, 1), t0 = tab(b, 0, 2);
    CHECK(stat(b, CACHED) == 2 && b.refcnt[c0] == 2 && b.refcnt[c1] == 2 && b.refcnt[t0] == 1);
    int sb, db;
    CHECK(b.fork(0, 1, 39, &sb, &db) == E::OK && sb == t0 && db != t0 && tab(b, 1, 0) == c0 && tab(b, 1, 1) == c1);
    CHECK(b.refcnt[c0] == 3 && b.refcnt[c1] == 3 && b.refcnt[db] == 1 && stat(b, CACHED) == 2 && stat(b, EVICTABLE) == 0);
    b.publish(1, P.data(), 39);                            // the same chain again: nothing new, the private tail is not full
    CHECK(stat(b, CACHED) == 2 && b.refcnt[c0] == 3 && b.refcnt[db] == 1);
    b.release_row(0); b.release_row(1);
    CHECK(b.refcnt[c0] == 1 && b.refcnt[c1] == 1 && b.free_blocks.size() == NBLK - 1 - 2 && stat(b, EVICTABLE) == 2);
  }
  for (int first : {0, 1}) {                               // either row may be reset first: the free list returns to its start
    KvBlocks b = fresh();
    const std::vector<int> start = sorted_free(b);
    b.ensure(0, 40);
    int sb, db;
    b.fork(0, 1, 39, &sb, &db);
    b.ensure(1, 64);                                       // dst grows on behind its private tail
    b.ensure(0, 50);
    CHECK(b.free_blocks.size() == NBLK - 1 - 4 - 2);
    b.release_row(first);
    bool alive = true;                                     // the other row still maps blocks with a reference each
    for (int i = 0; i < b.row_blocks[1 - first]; ++i) alive = alive && b.refcnt[tab(b, 1 - first, i)] == 1;
    CHECK(alive && b.row_blocks[first] == 0);
    b.release_row(1 - first);
    CHECK(sorted_free(b) == start && std::count(b.refcnt.begin(), b.refcnt.end(), 0) == NBLK);
  }
  {  // EXHAUSTED and TOO_LONG change nothing
    KvBlocks b = fresh();
    b.ensure(0, 64); b.ensure(1, 64); b.ensure(2, 40);
    CHECK(b.free_blocks.empty() && stat(b, EVICTABLE) == 0);
    b.btab_dirty = false;
    const Snapshot snap(b);
    int sb = -1, db = -1;
    CHECK(b.fork(2, 3, 17, &sb, &db) == E::EXHAUSTED && snap.same(b) && sb == 0 && db == 0);
    CHECK(b.fork(0, 3, 65, &sb, &db) == E::TOO_LONG && snap.same(b));      // (the entry point refuses n_tokens > length first)
    CHECK(b.fork(2, 3, 32, &sb, &db) == E::OK && b.row_blocks[3] == 2 && b.free_blocks.empty());    // full blocks need none
    CHECK(b.refcnt[tab(b, 2, 0)] == 2 && b.refcnt[tab(b, 2, 1)] == 2 && b.refcnt[tab(b, 2, 2)] == 1);
  }
  {  // the tail's block comes through take_block: a cache-only prefix block is evicted for it
    KvBlocks b = fresh();
    const Toks A = seq(1, 16);
    b.ensure(3, 16); b.publish(3, A.data(), 16); b.release_row(3);
    const int cached = b.prefix.begin()->second.block;
    b.ensure(0, 64); b.ensure(1, 64); b.ensure(2, 20);
    CHECK(b.free_blocks.empty() && stat(b, EVICTABLE) == 1);
    int sb, db;
    CHECK(b.fork(2, 3, 20, &sb, &db) == E::OK && db == cached && stat(b, EVICTIONS) == 1 && stat(b, CACHED) == 0 && b.refcnt[db] == 1);
  }
}

// ---- the walk.  The model: token-prefix tuple -> block for the cache, one owner list per block, the rows' tables, lengths
// and tokens.  Where the struct is free to choose (which block it hands out) the model checks that the choice was legal (a
// free block while there is one, else a cached block nobody maps) and follows it.
static void walk(unsigned seed, int n_ops) {
  KvBlocks b = fresh();
  std::mt19937 rng(seed);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  std::map<Toks, int> cache;
  std::vector<std::vector<int>> owners(NBLK), rows(ROWS);
  std::vector<Toks> text(ROWS);
  std::vector<int> len(ROWS, 0);
  int64_t hit = 0, lookup = 0, evictions = 0, exhausted = 0, forks = 0, fork_tails = 0, fork_exhausted = 0, fork_evictions = 0,
          forks_of_published = 0, forks_of_forks = 0, shared_now = 0;
  std::vector<bool> forked(ROWS, false);
  int op_no = 0;
  auto cached_block = [&](int blk) { for (auto& kv : cache) if (kv.second == blk) return true; return false; };
  auto model_free = [&] { int n = 0; for (int k = 1; k < NBLK; ++k) n += owners[k].empty() && !cached_block(k); return n; };
  auto model_evictable = [&] { int n = 0; for (auto& kv : cache) n += owners[kv.second].empty(); return n; };
  auto drop_owner = [&](int blk, int row) { auto& o = owners[blk]; o.erase(std::find(o.begin(), o.end(), row)); };
  // a block the struct handed out: nobody's, free while anything was free, else taken from the cache (an eviction)
  auto took = [&](int blk, int handed_before, int free_before) {
    REQUIRE(blk >= 1 && blk < NBLK && owners[blk].empty());
    if (cached_block(blk)) {
      REQUIRE(handed_before >= free_before);
      cache.erase(std::find_if(cache.begin(), cache.end(), [&](auto& kv) { return kv.second == blk; }));
      ++evictions;
      return true;
    }
    return false;
  };
  for (; op_no < n_ops; ++op_no) {
    const int row = rnd(0, ROWS - 1);
    switch (rnd(0, 12)) {
      case 0: case 1: {                                                        // release
        b.release_row(row);
        for (int blk : rows[row]) drop_owner(blk, row);
        rows[row].clear(); text[row].clear(); len[row] = 0; forked[row] = false;
        break;
      }
      case 2: case 3: {                                                        // attach (the caller's check first)
        if (len[row] != 0 || b.row_blocks[row] != 0) break;
        const int n = rnd(1, 64), keep = std::max(0, n - rnd(0, 24));
        Toks t = seq(rnd(1, 3), n);
        for (int i = keep; i < n; ++i) t[i] = rnd(0, 3);
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
        lookup += n; hit += want;
        break;
      }
      case 4: case 5: case 6: {                                                // ensure to a random length, then "run" to it
        const int target = rnd(len[row], 64);
        const int free_before = model_free();
        const E rc = b.ensure(row, target);
        int handed = 0;
        for (int i = (int)rows[row].size(); i < b.row_blocks[row]; ++i, ++handed) {
          const int blk = tab(b, row, i);
          took(blk, handed, free_before);
          owners[blk].push_back(row); rows[row].push_back(blk);
        }
        if (rc == E::EXHAUSTED) { REQUIRE(model_free() == 0 && model_evictable() == 0); ++exhausted; break; }
        REQUIRE(rc == E::OK);
        while ((int)text[row].size() < target) text[row].push_back(rnd(0, 3));
        len[row] = std::max(len[row], target);
        break;
      }
      case 7: case 8: {                                                        // publish (the caller's check first)
        const int n = rnd(std::max(0, len[row] - 8), len[row]);
        b.publish(row, text[row].data(), n);
        for (int i = 0; (i + 1) * BS <= n; ++i) cache.emplace(Toks(text[row].begin(), text[row].begin() + (i + 1) * BS), rows[row][i]);
        break;
      }
      case 9: case 10: case 11: {                                              // fork (the caller's checks first)
        const int dst = rnd(0, ROWS - 1);
        if (dst == row || len[dst] != 0 || b.row_blocks[dst] != 0 || len[row] < 1) break;
        const int n = rnd(1, len[row]), full = n / BS, tail = n % BS;
        const int free_before = model_free(), evictable_before = model_evictable();
        const Snapshot snap(b);
        int sb = -1, db = -1;
        const E rc = b.fork(row, dst, n, &sb, &db);
        if (tail && free_before == 0 && evictable_before == 0) {
          REQUIRE(rc == E::EXHAUSTED && snap.same(b));
          ++fork_exhausted;
          break;
        }
        REQUIRE(rc == E::OK && b.btab_dirty && b.row_blocks[dst] == full + (tail ? 1 : 0));
        for (int i = 0; i < full; ++i) {
          const int blk = rows[row][i];
          REQUIRE(tab(b, dst, i) == blk);
          owners[blk].push_back(dst); rows[dst].push_back(blk);
        }
        forks_of_published += full > 0 && cached_block(rows[row][0]);
        if (tail) {
          REQUIRE(sb == rows[row][full] && db == tab(b, dst, full) && db != sb);
          fork_evictions += took(db, 0, free_before);
          owners[db].push_back(dst); rows[dst].push_back(db);
          ++fork_tails;
        } else {
          REQUIRE(sb == 0 && db == 0 && (int)b.free_blocks.size() == (int)snap.free_blocks.size());
        }
        text[dst].assign(text[row].begin(), text[row].begin() + n);
        len[dst] = n;
        forks_of_forks += forked[row];
        forked[dst] = true;
        ++forks;
        break;
      }
      default: {                                                               // clear, rarely
        if (rnd(0, 9) != 0) break;
        b.clear_prefix();
        cache.clear();
      }
    }
    // ---- invariants
    for (int blk = 1; blk < NBLK; ++blk) {
      const auto in_free = std::count(b.free_blocks.begin(), b.free_blocks.end(), blk);
      const int refs = (int)owners[blk].size() + (cached_block(blk) ? 1 : 0);      // rows mapping it + (published ? 1 : 0)
      REQUIRE((in_free == 1 && refs == 0 && b.refcnt[blk] == 0) || (in_free == 0 && refs > 0 && b.refcnt[blk] == refs));
      shared_now += owners[blk].size() > 1;
    }
    REQUIRE(std::count(b.free_blocks.begin(), b.free_blocks.end(), 0) == 0);
    for (int r = 0; r < ROWS; ++r) {
      REQUIRE(b.row_blocks[r] == (int)rows[r].size() && (int)rows[r].size() * BS >= len[r]);
      for (int i = 0; i < STRIDE; ++i) REQUIRE(tab(b, r, i) == (i < (int)rows[r].size() ? rows[r][i] : 0));
      // a block that is not full -- the one behind the row's last full block, and any the row holds beyond -- is the row's alone
      for (int i = len[r] / BS; i < (int)rows[r].size(); ++i) REQUIRE(b.refcnt[rows[r][i]] == 1 && owners[rows[r][i]].size() == 1);
    }
    REQUIRE(stat(b, FREE) == model_free() && stat(b, CACHED) == (int64_t)cache.size() && stat(b, HIT) == hit &&
            stat(b, LOOKUP) == lookup && stat(b, EVICTIONS) == evictions && stat(b, EVICTABLE) == model_evictable());
  }
  CHECK(op_no >= 5000);
  printf("walk: %d ops, forks %lld (with a tail %lld, refused for blocks %lld, onto an evicted block %lld, of published rows %lld, of forks %lld), "
         "evictions %lld, exhausted ensures %lld, shared block sightings %lld\n", op_no, (long long)forks, (long long)fork_tails,
         (long long)fork_exhausted, (long long)fork_evictions, (long long)forks_of_published, (long long)forks_of_forks,
         (long long)evictions, (long long)exhausted, (long long)shared_now);
  CHECK(forks >= 100 && fork_tails >= 50);
  CHECK(fork_exhausted >= 1);
  CHECK(fork_evictions >= 1);
  CHECK(forks_of_published >= 1 && forks_of_forks >= 1);
  CHECK(evictions >= 1 && exhausted >= 1);
}

int main() {
  directed();
  walk(20261020u, 8000);
  printf("checks %d\n", n_checks);
  return 0;
}
