// kv_blocks.h -- the host side of a block-paged KV cache (mi_kv_create_paged): the block pool, the rows' block tables and the
// prefix cache.  Standard library only: the device sees nothing but the table that engine_kv.hip uploads, and
// tests/cpu/kv_blocks_test.cpp compiles this header alone, under the sanitizers.
//
// A row owns the blocks its table names, in order; block 0 is never handed out (unassigned table entries point at it, so a
// clamped address is always mapped memory).  refcnt[b] = rows that map block b + 1 if the prefix cache holds it.
//
// Sharing (attach, fork) is read-only and covers FULL blocks alone.  The invariant: a block that is not full is mapped by
// exactly one row and is never in the prefix cache.  No shared block is ever written, because the kernels append at a row's
// own length only -- behind its last full block, in a block of its own (ensure) or in the private copy that fork made.
#pragma once
#include <cstdint>
#include <cstring>
#include <list>
#include <unordered_map>
#include <vector>

namespace mi {

struct KvBlocks {
  enum class Ensure { OK, TOO_LONG, EXHAUSTED };
  int bs_shift = 0, nblocks = 0, bt_stride = 0;
  std::vector<int32_t> h_btab;   // [rows][bt_stride]: what the device's table is a copy of (btab_dirty: since the last upload)
  std::vector<int> row_blocks;   // blocks in use per row
  std::vector<int> refcnt;
  std::vector<int> free_blocks;
  bool btab_dirty = false;
  // prefix cache: full blocks of prompts, keyed by the hash of ALL tokens up to and including the block; an entry keeps
  // the block's own tokens and its parent's key, so a hit is verified token by token (no reliance on the hash alone)
  struct PrefixEntry { int block; uint64_t parent; std::vector<int32_t> tokens; std::list<uint64_t>::iterator lru_it; };
  std::unordered_map<uint64_t, PrefixEntry> prefix;
  std::list<uint64_t> lru;       // front = most recently used
  int64_t stat_hit_tokens = 0, stat_lookup_tokens = 0, stat_evictions = 0;

  // block_tokens: a power of two; the longest sequence of a row is bt_stride << bs_shift tokens
  void init(int slots, int block_tokens, int n_blocks, int max_tokens_per_row) {
    while ((1 << bs_shift) < block_tokens) ++bs_shift;
    nblocks = n_blocks;
    bt_stride = (max_tokens_per_row + block_tokens - 1) / block_tokens;
    h_btab.assign((size_t)slots * bt_stride, 0);
    row_blocks.assign(slots, 0);
    refcnt.assign(n_blocks, 0);
    for (int b = n_blocks - 1; b >= 1; --b) free_blocks.push_back(b);     // block 0 stays out of circulation
  }

  // the row's table covers `tokens` positions after this; a failure leaves the blocks the row already has
  Ensure ensure(int row, int tokens) {
    const int need = (tokens + (1 << bs_shift) - 1) >> bs_shift;
    if (need > bt_stride) return Ensure::TOO_LONG;
    while (row_blocks[row] < need) {
      const int blk = take_block();
      if (blk < 0) return Ensure::EXHAUSTED;
      h_btab[(size_t)row * bt_stride + row_blocks[row]++] = blk;
      btab_dirty = true;
    }
    return Ensure::OK;
  }

  void release_row(int row) {
    for (int i = 0; i < row_blocks[row]; ++i) {
      release_block(h_btab[(size_t)row * bt_stride + i]);
      h_btab[(size_t)row * bt_stride + i] = 0;
    }
    if (row_blocks[row] > 0) btab_dirty = true;
    row_blocks[row] = 0;
  }

  // Where the hash chains of a row that runs adapter `slot` start: K / V depend on the adapter, so chains published under
  // one (slot, generation) are found under no other -- the seed is the first block's parent, which same_prefix compares,
  // so this does not rest on the hash alone.  `generation` counts the changes of the slot: the chains of a replaced adapter
  // become unreachable and leave through the LRU.  Never 0, the seed of a row without an adapter (the keys of always).
  static uint64_t adapter_seed(int slot, uint32_t generation) {
    uint64_t z = (((uint64_t)(uint32_t)(slot + 1)) << 32 | generation) + 0x9E3779B97F4A7C15ull;     // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z ? z : 1;
  }

  // An EMPTY row (the caller checks) maps the published blocks that its prompt of n tokens starts with; returns the tokens they
  // hold.  Full blocks only, and at least one token of the prompt is left to run (its logits are needed).  seed: adapter_seed
  // of the row's adapter, 0 without one.
  int attach(int row, const int32_t* tokens, int n, uint64_t seed = 0) {
    const int bs = 1 << bs_shift;
    uint64_t parent = seed;
    int reused = 0;
    std::vector<uint64_t> chain;
    while (reused + bs <= n - 1 && row_blocks[row] < bt_stride) {
      const uint64_t h = prefix_hash(parent, tokens + reused, bs);
      auto it = prefix.find(h);
      if (it == prefix.end() || !same_prefix(it->second, parent, tokens + reused)) break;
      h_btab[(size_t)row * bt_stride + row_blocks[row]++] = it->second.block;
      ++refcnt[it->second.block];
      chain.push_back(h);
      parent = h;
      reused += bs;
    }
    lru_touch_chain(chain);
    stat_lookup_tokens += n;
    stat_hit_tokens += reused;
    if (reused > 0) btab_dirty = true;
    return reused;
  }

  // the full blocks of the row's first n tokens (all of them in its cache already: the caller checks) enter the prefix cache
  void publish(int row, const int32_t* tokens, int n, uint64_t seed = 0) {
    const int bs = 1 << bs_shift;
    uint64_t parent = seed;
    std::vector<uint64_t> chain;
    for (int i = 0; (i + 1) * bs <= n; ++i) {
      const uint64_t h = prefix_hash(parent, tokens + i * bs, bs);
      auto it = prefix.find(h);
      if (it == prefix.end()) {
        PrefixEntry pe;
        pe.block = h_btab[(size_t)row * bt_stride + i]; pe.parent = parent; pe.tokens.assign(tokens + i * bs, tokens + (i + 1) * bs);
        lru.push_front(h);
        pe.lru_it = lru.begin();
        ++refcnt[pe.block];                     // the cache's own reference: the block outlives the row
        prefix.emplace(h, std::move(pe));
      } else if (!same_prefix(it->second, parent, tokens + i * bs)) {
        break;                                  // a different prefix owns this key: leave it (and everything behind it) alone
      }
      chain.push_back(h);
      parent = h;
    }
    lru_touch_chain(chain);
  }

  // An EMPTY row `dst` (the caller checks) becomes a copy of the first n_tokens tokens of `src` (1 <= n_tokens <= the length
  // of src: the caller checks).  The n_tokens >> bs_shift full blocks are mapped, not copied (one more reference each); a
  // partly filled tail gets ONE block of dst's own (take_block: a cache-only prefix block may be evicted for it, as in
  // ensure), and the two tail block ids are reported for the caller's copy -- both 0 when n_tokens is a multiple of the
  // block size, which needs neither a block nor a copy.  A failure leaves both rows, refcnt and the free list as they were.
  Ensure fork(int src, int dst, int n_tokens, int* src_tail_blk, int* dst_tail_blk) {
    const int full = n_tokens >> bs_shift;
    const bool tail = (n_tokens & ((1 << bs_shift) - 1)) != 0;
    *src_tail_blk = *dst_tail_blk = 0;
    if (full + (tail ? 1 : 0) > bt_stride) return Ensure::TOO_LONG;
    int own = 0;
    if (tail && (own = take_block()) < 0) return Ensure::EXHAUSTED;      // first: nothing else has changed yet
    const int32_t* s = &h_btab[(size_t)src * bt_stride];
    int32_t* d = &h_btab[(size_t)dst * bt_stride];
    for (int i = 0; i < full; ++i) { d[i] = s[i]; ++refcnt[s[i]]; }
    if (tail) { d[full] = own; *src_tail_blk = s[full]; *dst_tail_blk = own; }
    row_blocks[dst] = full + (tail ? 1 : 0);
    btab_dirty = true;
    return Ensure::OK;
  }

  void clear_prefix() {
    for (auto& p : prefix) release_block(p.second.block);
    prefix.clear();
    lru.clear();
  }

  // free blocks | blocks in circulation (-1 each without a pool) | cached blocks | hit tokens | looked-up tokens | evictions |
  // evictable: published blocks that only the cache holds -- what evict_one can actually give back
  void stats(int64_t* out, int n) const {
    int64_t evictable = 0;
    for (const auto& pe : prefix) evictable += refcnt[pe.second.block] == 1 ? 1 : 0;
    const int64_t v[7] = {nblocks > 0 ? (int64_t)free_blocks.size() : -1, nblocks > 0 ? (int64_t)nblocks - 1 : -1,
                          (int64_t)prefix.size(), stat_hit_tokens, stat_lookup_tokens, stat_evictions, evictable};
    for (int i = 0; i < n && i < 7; ++i) out[i] = v[i];
  }

 private:
  static uint64_t prefix_hash(uint64_t parent, const int32_t* toks, int n) {
    uint64_t h = parent ^ 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) { h ^= (uint64_t)(uint32_t)toks[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xD6E8FEB86659FD93ull; }
    return h ? h : 1;
  }
  bool same_prefix(const PrefixEntry& pe, uint64_t parent, const int32_t* toks) const {
    return pe.parent == parent && memcmp(pe.tokens.data(), toks, sizeof(int32_t) << bs_shift) == 0;
  }

  void release_block(int blk) {
    if (blk <= 0) return;
    if (--refcnt[blk] == 0) free_blocks.push_back(blk);
  }

  // A prefix chain is only reachable from its first block (attach stops at the first miss), so a chain is made "recent"
  // leaf first: afterwards its root is the most recently used entry and its deepest block the oldest of the chain --
  // eviction (from the back) takes leaves before their parents and never strands children behind a missing parent.
  void lru_touch_chain(const std::vector<uint64_t>& chain) {
    for (auto h = chain.rbegin(); h != chain.rend(); ++h) {
      auto it = prefix.find(*h);
      if (it == prefix.end()) continue;
      lru.erase(it->second.lru_it);
      lru.push_front(*h);
      it->second.lru_it = lru.begin();
    }
  }

  // a block nobody but the prefix cache holds can be taken back (least recently used first)
  bool evict_one() {
    for (auto it = lru.rbegin(); it != lru.rend(); ++it) {
      auto pe = prefix.find(*it);
      if (pe == prefix.end() || refcnt[pe->second.block] != 1) continue;
      const int blk = pe->second.block;
      lru.erase(pe->second.lru_it);
      prefix.erase(pe);
      release_block(blk);
      ++stat_evictions;
      return true;
    }
    return false;
  }

  int take_block() {
    if (free_blocks.empty() && !evict_one()) return -1;
    const int blk = free_blocks.back();
    free_blocks.pop_back();
    refcnt[blk] = 1;
    return blk;
  }
};

}  // namespace mi
