// CPU check of the lookup multiplicities' host-side decisions
// (quill-zkvm_amd/csrc/lookup_plan.h): the owner reduction, the agreed chunk
// lengths, the chunk layout, the owner's slot capacity, the size arithmetic at
// the global caps and the mode / env parsers.  Prints "ok <name>" per check;
// exits non-zero when one fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quill-zkvm_amd/csrc/lookup_plan.h"

using namespace qg;

static int fails = 0;
static bool row_ok = true;
static void eq(const char* what, long long got, long long want) {
  if (got == want) return;
  printf("  %s = %lld, expected %lld\n", what, got, want);
  row_ok = false;
}
#define EQ(a, b) eq(#a, (long long)(a), (long long)(b))
#define TRUE(a) eq(#a, (a) ? 1 : 0, 1)
static void row(const char* name) {
  printf("%s %s\n", row_ok ? "ok" : "FAIL", name);
  if (!row_ok) fails++;
  row_ok = true;
}

template <class F>
static int code_of(F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code;
  }
  return 0;
}

// a cheap stream of 32-bit "row hashes"
static uint32_t next(uint32_t& x) {
  x = x * 1664525u + 1013904223u;
  return x ^ (x >> 15);
}

int main() {
  // owner < W for W = 1..8 and non-powers of two; every rank is hit
  for (uint32_t W : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 12u, 1000u, 1024u}) {
    std::vector<uint32_t> seen(W, 0);
    uint32_t x = W;
    for (int i = 0; i < 200000; i++) {
      const uint32_t d = lk_owner(next(x), 0xffffffffu, W);
      TRUE(d < W);
      if (d < W) seen[d]++;
    }
    for (uint32_t d = 0; d < W; d++) TRUE(seen[d] > 0);
    EQ(lk_owner(0xffffffffu, 0xffffffffu, W) < W, 1);
    EQ(lk_owner(0u, 0xffffffffu, W), 0);
  }
  // the extremes of the finalised hash map to the first and the last rank
  EQ((uint32_t)(((uint64_t)0xffffffffu * 7) >> 32), 6);
  row("owner_in_range");

  {  // uniform enough at W = 4: every rank within 2 % of a quarter
    uint32_t x = 99, seen[4] = {0, 0, 0, 0};
    for (int i = 0; i < 400000; i++) seen[lk_owner(next(x), 0xffffffffu, 4)]++;
    for (int d = 0; d < 4; d++) TRUE(seen[d] > 98000 && seen[d] < 102000);
  }
  row("owner_uniform");

  {  // owner bits 0: rank 0 owns everything; few bits: only low ranks
    uint32_t x = 5;
    for (int i = 0; i < 10000; i++) {
      const uint32_t h = next(x);
      EQ(lk_owner(h, lk_bits_mask("0"), 8), 0);
      EQ(lk_owner(h, lk_bits_mask("31"), 8) < 4, 1);
      // independent of the low bits the slot index uses: the owner is a
      // function of the whole hash, not of h & mask
    }
    // the same low 16 bits, different owners
    bool differ = false;
    for (uint32_t hi = 0; hi < 64 && !differ; hi++)
      differ = lk_owner(hi << 16 | 0x1234u, 0xffffffffu, 4) != lk_owner(0x1234u, 0xffffffffu, 4);
    TRUE(differ);
  }
  row("owner_bits");

  {  // maxima from a skewed matrix; odd rounds up; zero rows give 2
    const uint32_t W = 3;
    //                    table to 0,1,2   source to 0,1,2
    const uint32_t m[] = {1, 0, 0, /**/ 9, 0, 1,    // rank 0
                          0, 7, 2, /**/ 0, 0, 0,    // rank 1
                          3, 0, 0, /**/ 2, 40, 5};  // rank 2
    const LkMax mx = lk_pair_max(m, W);
    EQ(mx.t, 8);
    EQ(mx.s, 40);
    const uint32_t one[] = {1, 1};
    EQ(lk_pair_max(one, 1).t, 2);
    EQ(lk_pair_max(one, 1).s, 2);
    const uint32_t none[] = {0, 0, 0, 0, 0, 0, 0, 0};
    EQ(lk_pair_max(none, 2).t, 2);
    EQ(lk_round_even(0), 2);
    EQ(lk_round_even(2), 2);
    EQ(lk_round_even(3), 4);
    EQ(lk_round_even(4), 4);
    EQ(lk_round_even(1025), 1026);
  }
  row("pair_max");

  // chunk regions: 16-byte aligned, in order, no overlap, chunks tile the buffer
  for (uint32_t ncols : {1u, 2u, 3u, 16u})
    for (uint64_t max : {2ull, 6ull, 258ull, 1026ull, 1ull << 20}) {
      const LkChunk ch{max, ncols};
      EQ(ch.meta_off(), 0);
      EQ(ch.col_off(0), max * 8);
      uint64_t end = ch.meta_off() + max * LK_META_BYTES;
      for (uint32_t c = 0; c < ncols; c++) {
        EQ(ch.col_off(c) % 16, 0);
        EQ(ch.col_off(c), end);  // starts where the region before ends
        end = ch.col_off(c) + max * LK_WORD_BYTES;
      }
      EQ(ch.bytes(), end);
      EQ(ch.bytes(), max * (8 + 32ull * ncols));
      EQ(ch.bytes() % 16, 0);  // chunk d starts at d x bytes: aligned too
    }
  row("chunk_layout");

  {  // slot capacity: a power of two, at least twice the records
    for (uint64_t n : {1ull, 2ull, 3ull, 64ull, 65ull, 1000ull, (1ull << 20) + 1, 1ull << 31}) {
      const uint64_t cap = lk_slot_cap(n);
      TRUE(cap >= 2 * n);
      TRUE((cap & (cap - 1)) == 0);
      TRUE(cap < 4 * n || cap == 2);
    }
    const LkPartPlan p = lk_part_plan(4, 2, 4096, 4096, {1086, 1090});
    TRUE(p.cap >= 2 * 4 * 1086);
    TRUE((p.cap & (p.cap - 1)) == 0);
    EQ(p.cap, 16384);
    EQ(p.tab_records, 4 * 1086);
    EQ(p.src_records, 4 * 1090);
    EQ(p.tab_buf_bytes, 4 * 1086 * 72);
    EQ(p.src_buf_bytes, 4 * 1090 * 72);
    EQ(p.return_bytes, 1086 * 4);
    EQ(p.exchange_bytes, 4 * 1086 * 72 + 4 * 1090 * 72 + 4 * 1086 * 4);
    EQ(lk_replicated_exchange_bytes(4, 2, 4096), 4 * 4096 * 68);
    TRUE(p.exchange_bytes < lk_replicated_exchange_bytes(4, 2, 4096));
  }
  row("slot_capacity");

  {  // the global caps, and nothing overflows below them
    EQ(code_of([] { lk_check_global(2, 1, 8, 1ull << 30); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_check_global(2, 1, 1ull << 31, 8); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_check_global(2, 1, (1ull << 31) - 1, (1ull << 30) - 1); }), 0);
    EQ(code_of([] { lk_check_global(3, 17, 8, 8); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_check_global(1ull << 40, 1, 1ull << 40, 1); }), QG_ERR_UNSUPPORTED);
    EQ(lk_global_over(3, 0x55555555ull, 1ull << 32), 0);  // 3 x that = 2^32 - 1
    EQ(lk_global_over(3, 0x55555556ull, 1ull << 32), 1);
    EQ(code_of([] { lk_part_plan(2, 1, 8, 1ull << 30, {2, 2}); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_part_plan(2, 1, 1ull << 31, 8, {2, 2}); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_part_plan(1025, 1, 8, 8, {2, 2}); }), QG_ERR_UNSUPPORTED);
    EQ(code_of([] { lk_part_plan(4, 1, 8, 8, {10, 2}); }), QG_ERR_INVALID);  // more than a block
    EQ(code_of([] { lk_part_plan(4, 1, 8, 8, {3, 2}); }), QG_ERR_INVALID);   // odd
    EQ(code_of([] { lk_part_plan(4, 1, 7, 7, {8, 8}); }), 0);                // 7 rounds up to 8
    // the largest shape under the caps: exact 64-bit sizes
    const uint64_t tl = (1ull << 30) - 1, sl = (1ull << 31) - 3;
    const LkPartPlan p = lk_part_plan(2, 16, sl, tl, {lk_round_even(tl), lk_round_even(sl)});
    EQ(p.tab_records, 1ull << 31);
    EQ(p.cap, 1ull << 32);
    EQ(p.src_records, (1ull << 32) - 4);
    EQ(p.src_buf_bytes, ((1ull << 32) - 4) * (8 + 32 * 16));
    EQ(code_of([] { lk_mul(1ull << 40, 1ull << 30); }), QG_ERR_UNSUPPORTED);
    EQ(lk_mul(1ull << 40, 1ull << 20), 1ull << 60);
  }
  row("caps_and_overflow");

  {  // parsers
    EQ(lk_bits_mask(nullptr), 0xffffffffu);
    EQ(lk_bits_mask(""), 0xffffffffu);
    EQ(lk_bits_mask("0"), 0);
    EQ(lk_bits_mask("-3"), 0);
    EQ(lk_bits_mask("1"), 1);
    EQ(lk_bits_mask("8"), 255);
    EQ(lk_bits_mask("31"), 0x7fffffffu);
    EQ(lk_bits_mask("32"), 0xffffffffu);
    EQ(lk_bits_mask("99"), 0xffffffffu);
    unsetenv("QG_LOOKUP_HASH_BITS");
    unsetenv("QG_LOOKUP_OWNER_BITS");
    EQ(lk_hash_mask_env(), 0xffffffffu);
    EQ(lk_owner_mask_env(), 0xffffffffu);
    setenv("QG_LOOKUP_OWNER_BITS", "0", 1);
    EQ(lk_owner_mask_env(), 0);
    EQ(lk_hash_mask_env(), 0xffffffffu);  // the two switches are separate
    setenv("QG_LOOKUP_HASH_BITS", "4", 1);
    EQ(lk_hash_mask_env(), 15);
    unsetenv("QG_LOOKUP_HASH_BITS");
    unsetenv("QG_LOOKUP_OWNER_BITS");
    EQ(QG_LOOKUP_TABLE_REPLICATED, 0);
    EQ(QG_LOOKUP_TABLE_PARTITIONED, 1);
    EQ(code_of([] { lk_check_mode(QG_LOOKUP_TABLE_REPLICATED); }), 0);
    EQ(code_of([] { lk_check_mode(QG_LOOKUP_TABLE_PARTITIONED); }), 0);
    EQ(code_of([] { lk_check_mode(2); }), QG_ERR_INVALID);
    EQ(code_of([] { lk_check_mode(0xffffffffu); }), QG_ERR_INVALID);
  }
  row("parsers");

  return fails ? 1 : 0;
}
