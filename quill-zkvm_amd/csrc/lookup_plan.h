// The host-side decisions of the lookup multiplicities (lookup.hip): the table
// mode and the env switches, the global caps, and for the hash-partitioned
// sharded flow the owner of a tuple, the agreed record counts, the layout of a
// payload chunk, the owner's slot capacity and the scratch sizes.  Plain
// integers and small structs - no HIP - so tests/cpp/lookup_plan_check.cpp pins
// them on the CPU.  The functions the kernels call as well carry the device
// qualifier under hipcc only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>

#include "../../include/quill_gpu.h"
#include "error.h"

#ifdef __HIPCC__
#define LK_PLAN_HD __host__ __device__ __forceinline__
#else
#define LK_PLAN_HD inline
#endif

namespace qg {

static constexpr uint32_t LK_MAXCOLS = 16;
static constexpr uint32_t LK_EMPTY = 0xffffffffu;
static constexpr uint64_t LK_EMPTY64 = ~0ull;
// partitioned mode: the route kernels keep one LDS counter per destination rank
static constexpr uint32_t LK_MAX_WORLD = 1024;
static constexpr uint32_t LK_META_BYTES = 8;  // per record: two 32-bit words
static constexpr uint32_t LK_WORD_BYTES = 32;  // one Fr

// ---------------------------------------------------------------- switches
// QG_LOOKUP_HASH_BITS=<b> / QG_LOOKUP_OWNER_BITS=<b>, read per call: keep the
// low b bits of a 32-bit hash (unset or empty: all 32; b <= 0: none)
inline uint32_t lk_bits_mask(const char* text) {
  if (!text || !text[0]) return 0xffffffffu;
  const int b = atoi(text);
  if (b <= 0) return 0u;
  return b >= 32 ? 0xffffffffu : (1u << b) - 1u;
}
inline uint32_t lk_hash_mask_env() { return lk_bits_mask(getenv("QG_LOOKUP_HASH_BITS")); }
inline uint32_t lk_owner_mask_env() { return lk_bits_mask(getenv("QG_LOOKUP_OWNER_BITS")); }

inline bool lk_mode_known(uint32_t mode) {
  return mode == QG_LOOKUP_TABLE_REPLICATED || mode == QG_LOOKUP_TABLE_PARTITIONED;
}
inline void lk_check_mode(uint32_t mode) {
  QG_CHECK(lk_mode_known(mode), QG_ERR_INVALID,
           "lookup multiplicities: unknown table mode " + std::to_string(mode));
}

// ---------------------------------------------------------------- caps
// world x len >= limit, without overflow
inline bool lk_global_over(uint64_t world, uint64_t len, uint64_t limit) {
  return len >= (limit + world - 1) / world;
}
// the caps on the global lengths; every rank evaluates them on the agreed
// header values, so all ranks take the same branch
inline void lk_check_global(uint64_t world, uint32_t ncols, uint64_t src_len, uint64_t tab_len) {
  QG_CHECK(ncols <= LK_MAXCOLS, QG_ERR_UNSUPPORTED, "lookup multiplicities: more than 16 columns");
  QG_CHECK(!lk_global_over(world, tab_len, 1ull << 31), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: global table of 2^31 rows or more");
  // also what keeps a row's count inside 32 bits
  QG_CHECK(!lk_global_over(world, src_len, 1ull << 32), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: 2^32 global source rows or more");
}

// ---------------------------------------------------------------- owner
// murmur3's 32-bit finaliser: a bijection of the 32-bit words
LK_PLAN_HD uint32_t lk_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// The rank that matches a tuple, from the tuple's unmasked row hash: one more
// finaliser round, so the owner hangs on other bits than the slot index (the
// low bits of the hash itself) and not on QG_LOOKUP_HASH_BITS; then the range
// reduction of the top bits.  owner_mask = 0 sends every tuple to rank 0.
LK_PLAN_HD uint32_t lk_owner(uint32_t hash, uint32_t owner_mask, uint32_t world) {
  const uint32_t h = lk_fmix(hash) & owner_mask;
  return (uint32_t)(((uint64_t)h * world) >> 32);
}

// ---------------------------------------------------------------- sizes
// `counts` is the gathered W x 2W matrix: row s = rank s's records per
// destination, table first ([0, W)), then source ([W, 2W)).  The agreed chunk
// lengths are the maxima over all pairs, rounded up to even (a chunk's column
// regions then start on 16 bytes), at least 2.
struct LkMax {
  uint64_t t, s;
};
inline uint64_t lk_round_even(uint64_t v) { return v < 2 ? 2 : v + (v & 1); }
inline LkMax lk_pair_max(const uint32_t* counts, uint32_t world) {
  uint64_t t = 0, s = 0;
  for (uint32_t r = 0; r < world; r++)
    for (uint32_t d = 0; d < world; d++) {
      const uint32_t* row = counts + (size_t)r * 2 * world;
      if (row[d] > t) t = row[d];
      if (row[world + d] > s) s = row[world + d];
    }
  return {lk_round_even(t), lk_round_even(s)};
}

// One payload chunk (what one rank sends one rank) of `max` record slots:
//   [meta: max x 8 B][col 0: max x 32 B] ... [col ncols-1]
// meta = (global row, EMPTY) of a table record, (global source row, local
// count) of a source record, all ones in a padding slot.
struct LkChunk {
  uint64_t max;    // record slots, even
  uint32_t ncols;
  LK_PLAN_HD uint64_t meta_off() const { return 0; }
  LK_PLAN_HD uint64_t col_off(uint32_t c) const {
    return max * LK_META_BYTES + (uint64_t)c * max * LK_WORD_BYTES;
  }
  LK_PLAN_HD uint64_t bytes() const { return col_off(ncols); }
};

// open addressing over n records: the smallest power of two >= 2 n
inline uint64_t lk_slot_cap(uint64_t n) {
  uint64_t cap = 2;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

inline uint64_t lk_mul(uint64_t a, uint64_t b) {
  QG_CHECK(b == 0 || a <= UINT64_MAX / b, QG_ERR_UNSUPPORTED,
           "lookup multiplicities: scratch size overflows 64 bits");
  return a * b;
}

// everything the partitioned flow sizes from the agreed numbers
struct LkPartPlan {
  uint32_t world, ncols;
  LkChunk tab, src;
  uint64_t tab_records, src_records;  // world x max: what an owner receives
  uint64_t cap;                       // owner slots (64-bit words)
  uint64_t tab_buf_bytes, src_buf_bytes;  // one send or one receive buffer
  uint64_t return_bytes;                  // per pair, the counters going back
  uint64_t exchange_bytes;                // received in the three payload collectives
};
inline LkPartPlan lk_part_plan(uint64_t world, uint32_t ncols, uint64_t src_len, uint64_t tab_len,
                               LkMax mx) {
  QG_CHECK(world >= 1 && world <= LK_MAX_WORLD, QG_ERR_UNSUPPORTED,
           "lookup multiplicities: partitioned table on more than 1024 ranks");
  lk_check_global(world, ncols, src_len, tab_len);
  // a rank sends a destination at most its whole block
  QG_CHECK(mx.t >= 2 && mx.s >= 2 && !(mx.t & 1) && !(mx.s & 1) &&
               mx.t <= lk_round_even(tab_len) && mx.s <= lk_round_even(src_len),
           QG_ERR_INVALID, "lookup multiplicities: record counts outside the block lengths");
  LkPartPlan p;
  p.world = (uint32_t)world;
  p.ncols = ncols;
  p.tab = {mx.t, ncols};
  p.src = {mx.s, ncols};
  p.tab_records = lk_mul(world, mx.t);
  p.src_records = lk_mul(world, mx.s);
  // a record index shares a 64-bit slot with the global row: 32 bits each
  QG_CHECK(p.tab_records < (1ull << 32), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: 2^32 table records or more on one owner");
  QG_CHECK(p.src_records < (1ull << 32), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: 2^32 source records or more on one owner");
  p.cap = lk_slot_cap(p.tab_records);
  p.tab_buf_bytes = lk_mul(world, p.tab.bytes());
  p.src_buf_bytes = lk_mul(world, p.src.bytes());
  p.return_bytes = lk_mul(mx.t, sizeof(uint32_t));
  p.exchange_bytes = p.tab_buf_bytes + p.src_buf_bytes + lk_mul(world, p.return_bytes);
  return p;
}

// replicated mode: the gathered table columns and the counters' all-to-all
inline uint64_t lk_replicated_exchange_bytes(uint64_t world, uint32_t ncols, uint64_t tab_len) {
  return world * tab_len * ((uint64_t)LK_WORD_BYTES * ncols + sizeof(uint32_t));
}

}  // namespace qg
