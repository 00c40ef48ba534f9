// Multiplicities of a Logup lookup for gfx950 - the column the reference's
// callers build by hand (hyperplonk/src/piops/lookup.rs:186-193, a byte-table
// index trick in test code):
//     m[j] = #{ i : source row i == table row j }
// for a table of any content.  A row is the tuple of its ncols entries; the
// inputs are canonical Montgomery words, so equality of the 32-byte words is
// equality in Fr.  A tuple the table holds at several rows is counted at the
// LOWEST of them (the others get 0): a valid Logup assignment, and m is then a
// function of the inputs alone.
//
//  * k_lookup_build: an open-addressing table in HBM of cap = 2^ceil(log2(2 x
//    tab_len)) uint32 slots (filled with 0xffffffff every call).  One thread
//    per table row hashes its 8 x ncols limbs and probes linearly with
//    atomicCAS(slot, EMPTY, j); a slot that already holds an equal row gets
//    atomicMin(slot, j).  A slot's tuple never changes once set and no thread
//    walks past an empty slot, so every tuple ends in exactly one slot, which
//    holds its lowest row - whatever the order the threads ran in.
//  * k_lookup_count (a separate launch: the slots are complete and visible at
//    the kernel boundary): one thread per source row (grid stride) walks the
//    same probe sequence to the first slot whose row equals its tuple and
//    counts there; an empty slot first means the tuple is in no table row
//    (atomicMin into first_missing, one lane per wave).
//    Contention: a byte table under 2^22 source rows would put every atomic on
//    256 addresses.  Tables of up to LK_LDS_ROWS rows are counted in per-block
//    LDS counters, each nonzero one flushed to HBM once per block.  Above that
//    the lanes of a wave that hit the leading lane's row are merged into one
//    atomicAdd, for LK_MERGE_ROUNDS leaders (takes the heavy rows of a skewed
//    source); the rest add on their own.  Integer adds commute: the counts are
//    the same from run to run.
//  * k_lookup_finish: m[j] = Fr::from(count[j]).
//  * No thread waits on another: every probe loop is bounded by cap steps
//    (cap >= 2 x tab_len, so an empty slot always exists) and running out sets
//    an error word instead of running on.
//  * QG_LOOKUP_HASH_BITS=<b> (read per call) keeps only the low b bits of the
//    hash: b = 0 sends every row down one probe chain (tests).
//    QG_LOOKUP_BLOCKS=<k> caps the count kernel's grid.
//
// Sharded contexts (the _dev entries only; world W, rank r): every rank holds
// one block of each column, global row = rank x block length + local row, and
// receives its block of the global m.  Two explicit modes compute the same m
// (qg_lookup_multiplicities_dev_ex; the host decisions are in lookup_plan.h).
//
// QG_LOOKUP_TABLE_REPLICATED: the table is replicated, the source stays where
// it is (lookup_run_sharded):
//   1. header allgather (32 B per rank: status of the local argument checks,
//      ncols, src_len, tab_len, table mode) - a rank whose checks failed still
//      joins, so all ranks leave together and none waits in a later collective;
//   2. one allgather per table column into one global column (rank-major order
//      is global row order);
//   3. k_lookup_build over the gathered table (global length), k_lookup_count
//      over the local source rows into W x tab_len counters - both unchanged,
//      so the lowest GLOBAL row of a duplicated tuple takes the count;
//   4. one all-to-all of tab_len x 4 bytes (slice d of the counters to rank d),
//      k_lookup_finish_parts sums the W slices received into m;
//   5. one allgather of (lowest missing global row, error word): min and OR.
// ncols + 3 collectives per call ("lookup_collectives" of qg_ctx_counter).
// What bounds it: W x tab_len < 2^31 rows of table on every rank (32 x ncols
// bytes each, plus 12 bytes of slots and counters), received and built again
// by every rank: right for a small table under a big trace.
//
// QG_LOOKUP_TABLE_PARTITIONED: every tuple has one owner rank, chosen by a
// hash of the tuple; no rank holds more than its blocks, its share of the
// distinct tuples and padding (lookup_run_partitioned):
//   1. the header allgather, as above;
//   2. local dedup with the kernels above: k_lookup_build + k_lookup_count of
//      the source block against itself leave a counter > 0 exactly at the
//      lowest local row of each distinct tuple (its local count); the same for
//      the table block.  Only these representatives travel;
//   3. k_lookup_route_count: owner = (fmix(row hash) x W) >> 32 per
//      representative, counted per destination (LDS, then one global atomic
//      per block and destination).  QG_LOOKUP_OWNER_BITS=<b> (read per call)
//      keeps the low b bits of the finalised hash first: b = 0 makes rank 0
//      the owner of everything (tests);
//   4. one allgather of every rank's 2 W counts; all ranks take the maxima
//      over all pairs, rounded up to even: the fixed chunk lengths of 6.;
//   5. k_lookup_route_scatter: the representatives into W chunks
//      [meta: max x 8 B][col 0: max x 32 B]...; meta (filled with ones every
//      call) = (global row, EMPTY) or (global source row, local count);
//   6. two all-to-alls: table records, source records;
//   7. k_lookup_owner_build over the received table records: 64-bit slots
//      (global row << 32 | record index), atomicCAS to claim, atomicMin on an
//      equal tuple - the slot names the record with the lowest global row;
//   8. k_lookup_owner_count over the received source records: the local count
//      onto the winning record's counter; an empty slot first lowers
//      first_missing to the record's global row (a representative is its
//      tuple's lowest row on its rank, so the minimum over all is the lowest
//      missing global row);
//   9. one all-to-all takes the counters back in arrival positions;
//      k_lookup_finish_routed writes m through the meta the sender kept;
//  10. the allgather of (lowest missing global row, error word).
// 6 collectives per call whatever ncols.  What bounds it: the most records any
// rank sends any rank (a send and a receive buffer of W x max x (8 + 32 x
// ncols) bytes each for the table and for the source, plus 24 bytes of slots
// and counters per received table record); with distinct rows and an even
// hash W x max is about the rank's own block, whatever W.  Kernels of both
// flows: no thread waits on another, every loop has a bound, nothing depends
// on block order or placement.
#include <stdlib.h>

#include <string>
#include <vector>

#include "common.h"
#include "lookup_plan.h"

using namespace qg;

namespace qg {

static constexpr int LK_BLOCK = 256;        // build / finish
static constexpr int LK_CBLOCK = 1024;      // count: two blocks fill a CU's 32 wave slots
static constexpr uint32_t LK_LDS_ROWS = 16384;  // 64 KB of uint32 counters per block
static constexpr int LK_MERGE_ROUNDS = 4;

struct LkCols {
  const Fr* c[LK_MAXCOLS];
};

// device words of one call: [0..1] first missing source row (u64), [2] error
struct LkState {
  unsigned long long first_missing;
  uint32_t err;
  uint32_t pad;
};

struct LkWord {
  uint4 lo, hi;
};
QG_DEV LkWord lk_load(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  return {q[0], q[1]};
}
QG_DEV bool lk_same(const LkWord& a, const LkWord& b) {
  return ((a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) |
          (a.hi.x ^ b.hi.x) | (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w)) == 0;
}

QG_DEV uint32_t lk_mix(uint32_t h, uint32_t k) {  // murmur3 body
  k *= 0xcc9e2d51u;
  k = (k << 15) | (k >> 17);
  k *= 0x1b873593u;
  h ^= k;
  h = (h << 13) | (h >> 19);
  return h * 5u + 0xe6546b64u;
}

static constexpr uint32_t LK_SEED = 0x9747b28cu;
QG_DEV uint32_t lk_mix_word(uint32_t h, const LkWord& w) {
  h = lk_mix(h, w.lo.x);
  h = lk_mix(h, w.lo.y);
  h = lk_mix(h, w.lo.z);
  h = lk_mix(h, w.lo.w);
  h = lk_mix(h, w.hi.x);
  h = lk_mix(h, w.hi.y);
  h = lk_mix(h, w.hi.z);
  return lk_mix(h, w.hi.w);
}

// hash of row `row` of `cols` (all 8 limbs of every column), cut to hash_mask
QG_DEV uint32_t lk_hash(const LkCols& cols, uint32_t ncols, size_t row, uint32_t hash_mask) {
  uint32_t h = LK_SEED;
  for (uint32_t c = 0; c < ncols; c++) h = lk_mix_word(h, lk_load(cols.c[c] + row));
  return lk_fmix(h) & hash_mask;
}

// row a of A == row b of B, column by column
QG_DEV bool lk_rows_equal(const LkCols& A, size_t a, const LkCols& B, size_t b, uint32_t ncols) {
  for (uint32_t c = 0; c < ncols; c++)
    if (!lk_same(lk_load(A.c[c] + a), lk_load(B.c[c] + b))) return false;
  return true;
}

__global__ __launch_bounds__(LK_BLOCK) void k_lookup_build(LkCols tab, uint32_t ncols,
                                                           uint32_t tab_len,
                                                           uint32_t* __restrict__ slots,
                                                           uint64_t cap, uint32_t hash_mask,
                                                           LkState* __restrict__ st) {
  const uint64_t j64 = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (j64 >= tab_len) return;
  const uint32_t j = (uint32_t)j64;
  const uint64_t mask = cap - 1;
  uint64_t s = lk_hash(tab, ncols, j, hash_mask) & mask;
  for (uint64_t it = 0; it < cap; it++, s = (s + 1) & mask) {
    const uint32_t prev = atomicCAS(&slots[s], LK_EMPTY, j);
    if (prev == LK_EMPTY) return;
    // prev < tab_len: only build threads write slots, and only row indices
    if (prev < tab_len && lk_rows_equal(tab, prev, tab, j, ncols)) {
      atomicMin(&slots[s], j);
      return;
    }
  }
  atomicOr(&st->err, 1u);
}

// LDS = true: tab_len <= LK_LDS_ROWS, per-block counters in LDS
template <bool LDS>
__global__ __launch_bounds__(LK_CBLOCK) void k_lookup_count(LkCols src, LkCols tab, uint32_t ncols,
                                                            uint64_t src_len, uint32_t tab_len,
                                                            const uint32_t* __restrict__ slots,
                                                            uint64_t cap, uint32_t hash_mask,
                                                            uint32_t* __restrict__ count,
                                                            LkState* __restrict__ st) {
  __shared__ uint32_t lc[LDS ? LK_LDS_ROWS : 1];
  if (LDS) {
    for (uint32_t j = threadIdx.x; j < tab_len; j += LK_CBLOCK) lc[j] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const uint64_t mask = cap - 1;
  const uint64_t stride = (uint64_t)gridDim.x * LK_CBLOCK;
  // every lane of a wave runs the same number of rounds (the ballots below)
  const uint64_t rounds = (src_len + stride - 1) / stride;
  uint64_t i = (uint64_t)blockIdx.x * LK_CBLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    const bool live = i < src_len;
    uint32_t hit = LK_EMPTY;
    bool missing = false;
    if (live) {
      uint64_t s = lk_hash(src, ncols, i, hash_mask) & mask;
      bool done = false;
      for (uint64_t it = 0; it < cap; it++, s = (s + 1) & mask) {
        const uint32_t k = slots[s];
        if (k == LK_EMPTY) {
          missing = done = true;
          break;
        }
        if (k < tab_len && lk_rows_equal(tab, k, src, i, ncols)) {
          hit = k;
          done = true;
          break;
        }
      }
      if (!done) atomicOr(&st->err, 1u);
    }
    // lowest missing row: i grows with the lane, so the first lane that
    // missed holds this wave's lowest; skip what cannot lower the word
    const unsigned long long miss = __ballot(missing);
    if (miss && lane == __ffsll(miss) - 1 &&
        i < __hip_atomic_load(&st->first_missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&st->first_missing, (unsigned long long)i);
    if (LDS) {
      if (hit != LK_EMPTY) atomicAdd(&lc[hit], 1u);
    } else {
      unsigned long long todo = __ballot(hit != LK_EMPTY);
      for (int m = 0; m < LK_MERGE_ROUNDS && todo; m++) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t lr = __shfl(hit, leader, 64);
        const unsigned long long same = __ballot(hit == lr);  // lr != EMPTY: hits only
        if (lane == leader) atomicAdd(&count[lr], (uint32_t)__popcll(same));
        todo &= ~same;
      }
      if ((todo >> lane) & 1) atomicAdd(&count[hit], 1u);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tab_len; j += LK_CBLOCK) {
      const uint32_t c = lc[j];
      if (c) atomicAdd(&count[j], c);
    }
  }
}

// m[j] = Fr::from(count[j])
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_finish(const uint32_t* __restrict__ count,
                                                            uint32_t tab_len,
                                                            Fr* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (j >= tab_len) return;
  Fr x = Fr::zero();
  x.v[0] = count[j];
  out[j] = to_mont(x);
}

// sharded: m[j] = Fr::from(sum over source ranks s of recv[s * tab_len + j]),
// recv = the counters every rank held for this rank's block of the table.  The
// sum is at most the global number of source rows, W x src_len < 2^32
// (lookup_check_global), so it fits the 32-bit word.
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_finish_parts(
    const uint32_t* __restrict__ recv, uint32_t world, uint32_t tab_len, Fr* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (j >= tab_len) return;
  uint32_t c = 0;
  for (uint32_t s = 0; s < world; s++) c += recv[(uint64_t)s * tab_len + j];
  Fr x = Fr::zero();
  x.v[0] = c;
  out[j] = to_mont(x);
}

// QG_LOOKUP_BLOCKS=<k>, read per call: caps the count kernel's grid (default two
// blocks per CU), so a small input runs several grid-stride rounds
static size_t lookup_count_blocks(qg_ctx* ctx) {
  const char* lb = getenv("QG_LOOKUP_BLOCKS");
  const int k = lb ? atoi(lb) : 0;
  return k > 0 ? (size_t)k : 2 * (size_t)ctx->num_cus();
}

static void lookup_check_lengths(uint32_t ncols, size_t src_len, size_t tab_len) {
  QG_CHECK(ncols >= 1 && src_len >= 1 && tab_len >= 1, QG_ERR_INVALID,
           "lookup multiplicities need at least one column, source row and table row");
  QG_CHECK(ncols <= LK_MAXCOLS, QG_ERR_UNSUPPORTED, "lookup multiplicities: more than 16 columns");
  QG_CHECK((uint64_t)tab_len < (1ull << 31), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: table of 2^31 rows or more");
  QG_CHECK((uint64_t)src_len < (1ull << 32), QG_ERR_UNSUPPORTED,
           "lookup multiplicities: 2^32 source rows or more");
}

// Slots, counters and state words of one call, all filled here (nothing of an
// earlier call survives), then the build over `tab` (tab_len rows) and the count
// of the src_len rows of `src` into d_count[0 .. tab_len).
struct LkWork {
  uint32_t* d_count;
  LkState* d_st;
};
// the scratch a build-and-count keeps its slots, counters and state words in,
// and the timing groups its two launches are booked under
struct LkNames {
  const char *slots, *count, *state, *build_group, *count_group;
};
static constexpr LkNames LK_MAIN = {"lk_slots", "lk_count", "lk_state", "lookup_build",
                                    "lookup_count"};
static LkWork lookup_build_count(qg_ctx* ctx, uint32_t ncols, const LkCols& src, size_t src_len,
                                 const LkCols& tab, size_t tab_len, const LkNames& nm = LK_MAIN) {
  const uint64_t cap = lk_slot_cap(tab_len);
  const uint32_t hash_mask = lk_hash_mask_env();
  uint32_t* d_slots = ctx->scratch_as<uint32_t>(nm.slots, cap);
  uint32_t* d_count = ctx->scratch_as<uint32_t>(nm.count, tab_len);
  LkState* d_st = ctx->scratch_as<LkState>(nm.state, 1);
  const uint32_t tl = (uint32_t)tab_len;
  {
    QgTimed tm(ctx, nm.build_group);
    // nothing of an earlier call survives: slots, counters and the state words
    QG_HIP(hipMemsetAsync(d_slots, 0xff, cap * sizeof(uint32_t), ctx->stream));
    QG_HIP(hipMemsetAsync(&d_st->first_missing, 0xff, sizeof(unsigned long long), ctx->stream));
    QG_HIP(hipMemsetAsync(&d_st->err, 0, 2 * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_lookup_build, dim3(div_up(tab_len, LK_BLOCK)), dim3(LK_BLOCK), 0,
                       ctx->stream, tab, ncols, tl, d_slots, cap, hash_mask, d_st);
    QG_LAUNCH_CHECK();
  }
  {
    QgTimed tm(ctx, nm.count_group);
    QG_HIP(hipMemsetAsync(d_count, 0, tab_len * sizeof(uint32_t), ctx->stream));
    const size_t want = div_up(src_len, LK_CBLOCK);
    const unsigned grid = (unsigned)std::min<size_t>(want, lookup_count_blocks(ctx));
    if (tab_len <= LK_LDS_ROWS)
      hipLaunchKernelGGL(k_lookup_count<true>, dim3(grid), dim3(LK_CBLOCK), 0, ctx->stream, src,
                         tab, ncols, (uint64_t)src_len, tl, d_slots, cap, hash_mask, d_count, d_st);
    else
      hipLaunchKernelGGL(k_lookup_count<false>, dim3(grid), dim3(LK_CBLOCK), 0, ctx->stream, src,
                         tab, ncols, (uint64_t)src_len, tl, d_slots, cap, hash_mask, d_count, d_st);
    QG_LAUNCH_CHECK();
  }
  return {d_count, d_st};
}

// d_out[j] = multiplicity of table row j; returns the lowest source row that is
// in no table row, or -1
static int64_t lookup_run(qg_ctx* ctx, uint32_t ncols, const LkCols& src, size_t src_len,
                          const LkCols& tab, size_t tab_len, Fr* d_out) {
  const LkWork w = lookup_build_count(ctx, ncols, src, src_len, tab, tab_len);
  {
    QgTimed tm(ctx, "lookup_finish");
    hipLaunchKernelGGL(k_lookup_finish, dim3(div_up(tab_len, LK_BLOCK)), dim3(LK_BLOCK), 0,
                       ctx->stream, w.d_count, (uint32_t)tab_len, d_out);
    QG_LAUNCH_CHECK();
  }
  LkState h;
  QG_HIP(hipMemcpyAsync(&h, w.d_st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  QG_CHECK(!h.err, QG_ERR_DEVICE, "lookup multiplicities: probe sequence exhausted");
  return h.first_missing >= (unsigned long long)src_len ? -1 : (int64_t)h.first_missing;
}

// ---- sharded flow ----------------------------------------------------------
// what every rank tells the others before any other collective
struct LkHeader {
  int32_t status;  // of this rank's local argument checks
  uint32_t ncols;
  uint64_t src_len, tab_len;
  uint64_t mode;  // QG_LOOKUP_TABLE_*: 0 in the replicated mode
};
static_assert(sizeof(LkHeader) == 32, "lookup header is 32 bytes per rank");
// ... and after the count
struct LkResult {
  unsigned long long first_missing;  // global source row, ~0 when none
  uint32_t err, pad;
};

// every rank's `mine`, in rank order; one collective
template <class T>
static std::vector<T> lookup_exchange(qg_ctx* ctx, const T& mine) {
  const size_t W = (size_t)ctx->world;
  uint8_t* d = ctx->scratch_as<uint8_t>("lk_hdr", sizeof(LkHeader) * (W + 1));
  static_assert(sizeof(T) <= sizeof(LkHeader), "exchange slot");
  QG_HIP(hipMemcpyAsync(d, &mine, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  comm_allgather_bytes(ctx, d, d + sizeof(LkHeader), sizeof(T));
  ctx->lookup_collectives++;
  std::vector<T> all(W);
  QG_HIP(hipMemcpyAsync(all.data(), d + sizeof(LkHeader), sizeof(T) * W, hipMemcpyDeviceToHost,
                        ctx->stream));
  ctx->sync();
  return all;
}

// this rank's block of the global m into d_out; returns the lowest GLOBAL source
// row that is in no table row, or -1 (the same value on every rank)
static int64_t lookup_run_sharded(qg_ctx* ctx, uint32_t ncols, const LkCols& src, size_t src_len,
                                  const LkCols& tab_blocks, size_t tab_len, Fr* d_out) {
  const size_t W = (size_t)ctx->world, G = W * tab_len;
  Fr* d_gtab = ctx->scratch_as<Fr>("lk_gtab", (size_t)ncols * G);
  uint32_t* d_recv = ctx->scratch_as<uint32_t>("lk_recv", G);
  LkCols tab{};
  {
    QgTimed tm(ctx, "lookup_gather");
    for (uint32_t c = 0; c < ncols; c++) {
      Fr* g = d_gtab + (size_t)c * G;
      comm_allgather_bytes(ctx, tab_blocks.c[c], g, tab_len * sizeof(Fr));
      ctx->lookup_collectives++;
      tab.c[c] = g;
    }
  }
  const LkWork w = lookup_build_count(ctx, ncols, src, src_len, tab, G);
  {
    QgTimed tm(ctx, "lookup_exchange");
    comm_alltoall_bytes(ctx, w.d_count, d_recv, tab_len * sizeof(uint32_t));
    ctx->lookup_collectives++;
  }
  ctx->lookup_exchange_bytes += lk_replicated_exchange_bytes(W, ncols, tab_len);
  {
    QgTimed tm(ctx, "lookup_finish");
    hipLaunchKernelGGL(k_lookup_finish_parts, dim3(div_up(tab_len, LK_BLOCK)), dim3(LK_BLOCK), 0,
                       ctx->stream, d_recv, (uint32_t)W, (uint32_t)tab_len, d_out);
    QG_LAUNCH_CHECK();
  }
  LkState h;
  QG_HIP(hipMemcpyAsync(&h, w.d_st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  LkResult mine{~0ull, h.err, 0};
  if (h.first_missing < (unsigned long long)src_len)
    mine.first_missing = (unsigned long long)ctx->rank * src_len + h.first_missing;
  unsigned long long first = ~0ull;
  uint32_t err = 0;
  for (const LkResult& r : lookup_exchange(ctx, mine)) {
    first = std::min(first, r.first_missing);
    err |= r.err;
  }
  QG_CHECK(!err, QG_ERR_DEVICE, "lookup multiplicities: probe sequence exhausted");
  return first == ~0ull ? -1 : (int64_t)first;
}

// ---- sharded flow, hash-partitioned table -----------------------------------
// A payload buffer is W chunks of the LkChunk layout (lookup_plan.h); record
// `idx` of a buffer is slot idx % max of chunk idx / max.
struct LkRecs {
  const uint8_t* base;
  LkChunk ch;
  uint64_t chunk_bytes;
};
QG_DEV uint2 lk_rec_meta(const LkRecs& r, uint32_t idx) {
  const uint64_t s = idx / r.ch.max, k = idx % r.ch.max;
  return reinterpret_cast<const uint2*>(r.base + s * r.chunk_bytes)[k];
}
QG_DEV LkWord lk_rec_word(const LkRecs& r, uint32_t idx, uint32_t c) {
  const uint64_t s = idx / r.ch.max, k = idx % r.ch.max;
  return lk_load(reinterpret_cast<const Fr*>(r.base + s * r.chunk_bytes + r.ch.col_off(c)) + k);
}
// the unmasked row hash of a record: lk_hash of the row it was copied from
QG_DEV uint32_t lk_rec_hash(const LkRecs& r, uint32_t idx) {
  uint32_t h = LK_SEED;
  for (uint32_t c = 0; c < r.ch.ncols; c++) h = lk_mix_word(h, lk_rec_word(r, idx, c));
  return lk_fmix(h);
}
QG_DEV bool lk_recs_equal(const LkRecs& A, uint32_t a, const LkRecs& B, uint32_t b) {
  for (uint32_t c = 0; c < A.ch.ncols; c++)
    if (!lk_same(lk_rec_word(A, a, c), lk_rec_word(B, b, c))) return false;
  return true;
}

// Route, pass 1: one thread per row of a block of columns.  A row whose dedup
// counter is nonzero is its tuple's representative (the lowest local row); its
// owner goes to dest[row] (EMPTY for the other rows) and is counted, per block
// in LDS, then with one global atomic per block and destination.
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_route_count(
    LkCols cols, uint32_t ncols, uint64_t len, const uint32_t* __restrict__ dedup, uint32_t world,
    uint32_t owner_mask, uint32_t* __restrict__ dest, uint32_t* __restrict__ totals) {
  __shared__ uint32_t lc[LK_MAX_WORLD];
  for (uint32_t d = threadIdx.x; d < world; d += LK_BLOCK) lc[d] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (i < len) {
    uint32_t d = LK_EMPTY;
    if (dedup[i]) {
      d = lk_owner(lk_hash(cols, ncols, i, 0xffffffffu), owner_mask, world);
      atomicAdd(&lc[d], 1u);
    }
    dest[i] = d;
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < world; d += LK_BLOCK)
    if (lc[d]) atomicAdd(&totals[d], lc[d]);
}

// Route, pass 2: the representatives into the W chunks of `send` (`max` slots
// each, meta pre-filled with ones).  A block reserves its slots of a chunk with
// one atomicAdd on that chunk's cursor; a row's place inside the reservation is
// its LDS ticket.  Which slot a record lands in depends on the order the blocks
// ran in; nothing downstream does.  A slot index is checked against `max`
// before the store (it cannot pass it: pass 1 counted the same rows).
// SRC: meta = (global source row, local count); else (global table row, EMPTY).
template <bool SRC>
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_route_scatter(
    LkCols cols, uint32_t ncols, uint64_t len, const uint32_t* __restrict__ dedup,
    const uint32_t* __restrict__ dest, uint32_t world, uint64_t row_base,
    uint32_t* __restrict__ cursors, uint8_t* __restrict__ send, LkChunk ch,
    LkState* __restrict__ st) {
  __shared__ uint32_t lc[LK_MAX_WORLD];
  for (uint32_t d = threadIdx.x; d < world; d += LK_BLOCK) lc[d] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  const uint32_t d = i < len ? dest[i] : LK_EMPTY;
  uint32_t ticket = 0;
  if (d < world) ticket = atomicAdd(&lc[d], 1u);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < world; k += LK_BLOCK)
    if (lc[k]) lc[k] = atomicAdd(&cursors[k], lc[k]);  // count -> base of the reservation
  __syncthreads();
  if (d >= world) return;
  const uint64_t slot = (uint64_t)lc[d] + ticket;
  if (slot >= ch.max) {
    atomicOr(&st->err, 1u);
    return;
  }
  uint8_t* chunk = send + (uint64_t)d * ch.bytes();
  reinterpret_cast<uint2*>(chunk)[slot] =
      make_uint2((uint32_t)(row_base + i), SRC ? dedup[i] : LK_EMPTY);
  for (uint32_t c = 0; c < ncols; c++) {
    const LkWord w = lk_load(cols.c[c] + i);
    uint4* q = reinterpret_cast<uint4*>(chunk + ch.col_off(c)) + 2 * slot;
    q[0] = w.lo;
    q[1] = w.hi;
  }
}

// Owner build: one thread per received table record (padding slots leave at
// once).  Open addressing over 64-bit slots (global row << 32 | record index),
// filled with ones every call.  A claimed slot's tuple never changes; an equal
// tuple lowers the slot with atomicMin, so the slot names the record with the
// lowest global row whatever the thread order and the arrival order.
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_owner_build(
    LkRecs tab, uint32_t nrec, unsigned long long* __restrict__ slots, uint64_t cap,
    uint32_t hash_mask, LkState* __restrict__ st) {
  const uint64_t i64 = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (i64 >= nrec) return;
  const uint32_t idx = (uint32_t)i64;
  const uint2 meta = lk_rec_meta(tab, idx);
  if (meta.x == LK_EMPTY) return;
  const unsigned long long mine = ((unsigned long long)meta.x << 32) | idx;
  const uint64_t mask = cap - 1;
  uint64_t s = (lk_rec_hash(tab, idx) & hash_mask) & mask;
  for (uint64_t it = 0; it < cap; it++, s = (s + 1) & mask) {
    const unsigned long long prev = atomicCAS(&slots[s], LK_EMPTY64, mine);
    if (prev == LK_EMPTY64) return;
    const uint32_t pidx = (uint32_t)prev;  // only build threads write slots
    if (pidx < nrec && lk_recs_equal(tab, pidx, tab, idx)) {
      atomicMin(&slots[s], mine);
      return;
    }
  }
  atomicOr(&st->err, 1u);
}

// Owner count: one thread per received source record (a separate launch: the
// slots are complete).  The record's local count is added to the counter of
// the winning table record; an empty slot first means the tuple is in no table
// row, and the record's global row (the lowest of its tuple on its rank) goes
// into first_missing.  Equal hits in a wave are NOT merged: the records were
// deduplicated per rank, so a tuple arrives at most W times in all, spread
// over W chunks, and a ballot round would cost more than the adds it saves.
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_owner_count(
    LkRecs src, uint32_t nsrc, LkRecs tab, uint32_t nrec,
    const unsigned long long* __restrict__ slots, uint64_t cap, uint32_t hash_mask,
    uint32_t* __restrict__ count, LkState* __restrict__ st) {
  const uint64_t i64 = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (i64 >= nsrc) return;
  const uint32_t idx = (uint32_t)i64;
  const uint2 meta = lk_rec_meta(src, idx);
  if (meta.x == LK_EMPTY) return;
  const uint64_t mask = cap - 1;
  uint64_t s = (lk_rec_hash(src, idx) & hash_mask) & mask;
  for (uint64_t it = 0; it < cap; it++, s = (s + 1) & mask) {
    const unsigned long long k = slots[s];
    if (k == LK_EMPTY64) {
      if (meta.x < __hip_atomic_load(&st->first_missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&st->first_missing, (unsigned long long)meta.x);
      return;
    }
    const uint32_t widx = (uint32_t)k;
    if (widx < nrec && lk_recs_equal(tab, widx, src, idx)) {
      atomicAdd(&count[widx], meta.y);
      return;
    }
  }
  atomicOr(&st->err, 1u);
}

// Finish: the counters came back in the positions the records were sent in;
// the meta kept in the send buffer names each position's row.  out was zeroed:
// a row that was no representative, or whose tuple a lower row won, stays 0.
__global__ __launch_bounds__(LK_BLOCK) void k_lookup_finish_routed(
    LkRecs sent, const uint32_t* __restrict__ back, uint32_t nrec, uint64_t row_base,
    uint32_t tab_len, Fr* __restrict__ out) {
  const uint64_t i64 = (uint64_t)blockIdx.x * LK_BLOCK + threadIdx.x;
  if (i64 >= nrec) return;
  const uint2 meta = lk_rec_meta(sent, (uint32_t)i64);
  if (meta.x == LK_EMPTY) return;
  const uint64_t local = (uint64_t)meta.x - row_base;
  if (local >= tab_len) return;  // this rank wrote the meta: cannot happen
  Fr x = Fr::zero();
  x.v[0] = back[i64];
  out[local] = to_mont(x);
}

static constexpr LkNames LK_DEDUP_TAB = {"lkp_tslots", "lkp_tcount", "lkp_tstate", "lookup_dedup",
                                         "lookup_dedup"};
static constexpr LkNames LK_DEDUP_SRC = {"lkp_sslots", "lkp_scount", "lkp_sstate", "lookup_dedup",
                                         "lookup_dedup"};

// this rank's block of the global m into d_out; returns the lowest GLOBAL source
// row that is in no table row, or -1 (the same value on every rank)
static int64_t lookup_run_partitioned(qg_ctx* ctx, uint32_t ncols, const LkCols& src,
                                      size_t src_len, const LkCols& tab, size_t tab_len,
                                      Fr* d_out) {
  const uint32_t W = (uint32_t)ctx->world;
  QG_CHECK(W <= LK_MAX_WORLD, QG_ERR_UNSUPPORTED,
           "lookup multiplicities: partitioned table on more than 1024 ranks");
  const uint32_t hash_mask = lk_hash_mask_env(), owner_mask = lk_owner_mask_env();
  hipStream_t st = ctx->stream;
  // 2. local dedup: counter > 0 exactly at the lowest local row of each tuple
  const LkWork dt = lookup_build_count(ctx, ncols, tab, tab_len, tab, tab_len, LK_DEDUP_TAB);
  const LkWork ds = lookup_build_count(ctx, ncols, src, src_len, src, src_len, LK_DEDUP_SRC);
  // 3. owners and per-destination counts: [table W][source W]
  uint32_t* d_dest_t = ctx->scratch_as<uint32_t>("lkp_tdest", tab_len);
  uint32_t* d_dest_s = ctx->scratch_as<uint32_t>("lkp_sdest", src_len);
  uint32_t* d_totals = ctx->scratch_as<uint32_t>("lkp_totals", 4 * (size_t)W);  // + cursors
  uint32_t* d_cursors = d_totals + 2 * (size_t)W;
  uint32_t* d_sizes = ctx->scratch_as<uint32_t>("lkp_sizes", 2 * (size_t)W * W);
  const unsigned grid_t = div_up(tab_len, LK_BLOCK), grid_s = div_up(src_len, LK_BLOCK);
  {
    QgTimed tm(ctx, "lookup_route");
    QG_HIP(hipMemsetAsync(d_totals, 0, 4 * (size_t)W * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_lookup_route_count, dim3(grid_t), dim3(LK_BLOCK), 0, st, tab, ncols,
                       (uint64_t)tab_len, dt.d_count, W, owner_mask, d_dest_t, d_totals);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lookup_route_count, dim3(grid_s), dim3(LK_BLOCK), 0, st, src, ncols,
                       (uint64_t)src_len, ds.d_count, W, owner_mask, d_dest_s, d_totals + W);
    QG_LAUNCH_CHECK();
  }
  // 4. size agreement
  std::vector<uint32_t> sizes(2 * (size_t)W * W);
  {
    QgTimed tm(ctx, "lookup_exchange");
    comm_allgather_bytes(ctx, d_totals, d_sizes, 2 * (size_t)W * sizeof(uint32_t));
    ctx->lookup_collectives++;
  }
  QG_HIP(hipMemcpyAsync(sizes.data(), d_sizes, sizes.size() * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, st));
  ctx->sync();
  const LkPartPlan p = lk_part_plan(W, ncols, src_len, tab_len, lk_pair_max(sizes.data(), W));
  const uint32_t* own = sizes.data() + (size_t)ctx->rank * 2 * W;
  for (uint32_t d = 0; d < W; d++) {
    ctx->lookup_routed_tab += own[d];
    ctx->lookup_routed_src += own[W + d];
  }
  // 5. scatter into the send buffers (meta all ones: padding, and nothing of an
  //    earlier call)
  uint8_t* d_send_t = ctx->scratch_as<uint8_t>("lkp_tsend", p.tab_buf_bytes);
  uint8_t* d_recv_t = ctx->scratch_as<uint8_t>("lkp_trecv", p.tab_buf_bytes);
  uint8_t* d_send_s = ctx->scratch_as<uint8_t>("lkp_ssend", p.src_buf_bytes);
  uint8_t* d_recv_s = ctx->scratch_as<uint8_t>("lkp_srecv", p.src_buf_bytes);
  LkState* d_st = ctx->scratch_as<LkState>("lkp_state", 1);
  {
    QgTimed tm(ctx, "lookup_route");
    QG_HIP(hipMemsetAsync(&d_st->first_missing, 0xff, sizeof(unsigned long long), st));
    QG_HIP(hipMemsetAsync(&d_st->err, 0, 2 * sizeof(uint32_t), st));
    for (uint32_t d = 0; d < W; d++) {
      QG_HIP(hipMemsetAsync(d_send_t + d * p.tab.bytes(), 0xff, p.tab.max * LK_META_BYTES, st));
      QG_HIP(hipMemsetAsync(d_send_s + d * p.src.bytes(), 0xff, p.src.max * LK_META_BYTES, st));
    }
    hipLaunchKernelGGL(k_lookup_route_scatter<false>, dim3(grid_t), dim3(LK_BLOCK), 0, st, tab,
                       ncols, (uint64_t)tab_len, dt.d_count, d_dest_t, W,
                       (uint64_t)ctx->rank * tab_len, d_cursors, d_send_t, p.tab, d_st);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lookup_route_scatter<true>, dim3(grid_s), dim3(LK_BLOCK), 0, st, src,
                       ncols, (uint64_t)src_len, ds.d_count, d_dest_s, W,
                       (uint64_t)ctx->rank * src_len, d_cursors + W, d_send_s, p.src, d_st);
    QG_LAUNCH_CHECK();
  }
  // 6. payload
  {
    QgTimed tm(ctx, "lookup_exchange");
    comm_alltoall_bytes(ctx, d_send_t, d_recv_t, p.tab.bytes());
    comm_alltoall_bytes(ctx, d_send_s, d_recv_s, p.src.bytes());
    ctx->lookup_collectives += 2;
  }
  // 7, 8. the owner matches what it received
  unsigned long long* d_slots = ctx->scratch_as<unsigned long long>("lkp_oslots", p.cap);
  uint32_t* d_count = ctx->scratch_as<uint32_t>("lkp_ocount", p.tab_records);
  uint32_t* d_back = ctx->scratch_as<uint32_t>("lkp_back", p.tab_records);
  const LkRecs rt{d_recv_t, p.tab, p.tab.bytes()}, rs{d_recv_s, p.src, p.src.bytes()};
  const uint32_t nrec = (uint32_t)p.tab_records;
  const uint32_t nsrc = (uint32_t)p.src_records;
  {
    QgTimed tm(ctx, "lookup_owner");
    QG_HIP(hipMemsetAsync(d_slots, 0xff, p.cap * sizeof(unsigned long long), st));
    QG_HIP(hipMemsetAsync(d_count, 0, p.tab_records * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_lookup_owner_build, dim3(div_up(nrec, LK_BLOCK)), dim3(LK_BLOCK), 0, st,
                       rt, nrec, d_slots, p.cap, hash_mask, d_st);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lookup_owner_count, dim3(div_up(nsrc, LK_BLOCK)), dim3(LK_BLOCK), 0, st,
                       rs, nsrc, rt, nrec, d_slots, p.cap, hash_mask, d_count, d_st);
    QG_LAUNCH_CHECK();
  }
  // 9. the counters go back in arrival positions
  {
    QgTimed tm(ctx, "lookup_exchange");
    comm_alltoall_bytes(ctx, d_count, d_back, p.return_bytes);
    ctx->lookup_collectives++;
  }
  ctx->lookup_exchange_bytes += p.exchange_bytes;
  {
    QgTimed tm(ctx, "lookup_finish");
    QG_HIP(hipMemsetAsync(d_out, 0, tab_len * sizeof(Fr), st));
    const LkRecs sent{d_send_t, p.tab, p.tab.bytes()};
    hipLaunchKernelGGL(k_lookup_finish_routed, dim3(div_up(nrec, LK_BLOCK)), dim3(LK_BLOCK), 0, st,
                       sent, d_back, nrec, (uint64_t)ctx->rank * tab_len, (uint32_t)tab_len, d_out);
    QG_LAUNCH_CHECK();
  }
  // 10. lowest missing row and error words (the two dedups' and the owner's)
  LkState h, ht, hs;
  QG_HIP(hipMemcpyAsync(&h, d_st, sizeof(h), hipMemcpyDeviceToHost, st));
  QG_HIP(hipMemcpyAsync(&ht, dt.d_st, sizeof(ht), hipMemcpyDeviceToHost, st));
  QG_HIP(hipMemcpyAsync(&hs, ds.d_st, sizeof(hs), hipMemcpyDeviceToHost, st));
  ctx->sync();
  // first_missing holds a global row already (below 2^32) or all ones
  const LkResult mine{h.first_missing, h.err | ht.err | hs.err, 0};
  unsigned long long first = ~0ull;
  uint32_t err = 0;
  for (const LkResult& r : lookup_exchange(ctx, mine)) {
    first = std::min(first, r.first_missing);
    err |= r.err;
  }
  QG_CHECK(!err, QG_ERR_DEVICE, "lookup multiplicities: probe sequence exhausted");
  return first == ~0ull ? -1 : (int64_t)first;
}

static void lookup_report(int64_t miss, int64_t* first_missing) {
  if (first_missing) *first_missing = miss;
  QG_CHECK(miss < 0, QG_ERR_ASSERT,
           "lookup source row " + std::to_string(miss) + " is in no table row");
}

// the _dev entry's checks of this rank's own arguments; `check_buffers` is
// false when the lengths are over a cap (no buffer of such a length exists)
static void lookup_check_dev_args(uint32_t ncols, const qg_buf* const* src_cols, size_t src_len,
                                  const qg_buf* const* tab_cols, size_t tab_len,
                                  const qg_buf* out_m, bool check_buffers, LkCols& src,
                                  LkCols& tab) {
  QG_CHECK(src_cols && tab_cols && out_m, QG_ERR_INVALID, "null argument");
  QG_CHECK(ncols >= 1 && src_len >= 1 && tab_len >= 1, QG_ERR_INVALID,
           "lookup multiplicities need at least one column, source row and table row");
  if (!check_buffers) return;
  QG_CHECK(out_m->n >= tab_len, QG_ERR_INVALID, "output buffer too short");
  for (uint32_t c = 0; c < ncols; c++) {
    QG_CHECK(src_cols[c] && src_cols[c]->n >= src_len, QG_ERR_INVALID,
             "source column buffer missing or too short");
    QG_CHECK(tab_cols[c] && tab_cols[c]->n >= tab_len, QG_ERR_INVALID,
             "table column buffer missing or too short");
    QG_CHECK(!ranges_overlap(out_m->d, tab_len, src_cols[c]->d, src_len) &&
                 !ranges_overlap(out_m->d, tab_len, tab_cols[c]->d, tab_len),
             QG_ERR_INVALID, "output aliases an input column");
    src.c[c] = src_cols[c]->d;
    tab.c[c] = tab_cols[c]->d;
  }
}

}  // namespace qg

// ---------------------------------------------------------------- C-ABI
extern "C" {

int qg_lookup_multiplicities(qg_ctx* ctx, uint32_t ncols, const uint64_t* const* src_cols,
                             size_t src_len, const uint64_t* const* tab_cols, size_t tab_len,
                             uint64_t* out_m, int64_t* first_missing) {
  if (!ctx) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(src_cols && tab_cols && out_m, QG_ERR_INVALID, "null argument");
    lookup_check_lengths(ncols, src_len, tab_len);
    // a sharded caller holds device blocks: only the _dev entry has the sharded form
    QG_CHECK(!ctx->sharded, QG_ERR_UNSUPPORTED,
             "lookup multiplicities from host pointers are not supported on a sharded context "
             "(communicator attached): use qg_lookup_multiplicities_dev");
    for (uint32_t c = 0; c < ncols; c++) {
      QG_CHECK(src_cols[c] && tab_cols[c], QG_ERR_INVALID, "null column");
      QG_CHECK(!ranges_overlap(out_m, 4 * tab_len, src_cols[c], 4 * src_len) &&
                   !ranges_overlap(out_m, 4 * tab_len, tab_cols[c], 4 * tab_len),
               QG_ERR_INVALID, "output aliases an input column");
    }
    QG_HIP(hipSetDevice(ctx->device));
    Fr* d = ctx->scratch_as<Fr>("lk_in", (size_t)ncols * (src_len + tab_len) + tab_len);
    LkCols src{}, tab{};
    for (uint32_t c = 0; c < ncols; c++) {
      Fr* s = d + (size_t)c * src_len;
      Fr* t = d + (size_t)ncols * src_len + (size_t)c * tab_len;
      fr_upload(ctx, s, src_cols[c], src_len);
      fr_upload(ctx, t, tab_cols[c], tab_len);
      src.c[c] = s;
      tab.c[c] = t;
    }
    Fr* d_out = d + (size_t)ncols * (src_len + tab_len);
    if (first_missing) *first_missing = -1;
    const int64_t miss = lookup_run(ctx, ncols, src, src_len, tab, tab_len, d_out);
    lookup_report(miss, first_missing);
    fr_download(ctx, out_m, d_out, tab_len);
    ctx->sync();
  });
}

int qg_lookup_multiplicities_dev_ex(qg_ctx* ctx, uint32_t ncols, const qg_buf* const* src_cols,
                                    size_t src_len, const qg_buf* const* tab_cols, size_t tab_len,
                                    qg_buf* out_m, int64_t* first_missing, uint32_t table_mode) {
  if (!ctx) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    LkCols src{}, tab{};
    if (!ctx->sharded) {
      lk_check_mode(table_mode);
      QG_CHECK(src_cols && tab_cols && out_m, QG_ERR_INVALID, "null argument");
      lookup_check_lengths(ncols, src_len, tab_len);
      lookup_check_dev_args(ncols, src_cols, src_len, tab_cols, tab_len, out_m, true, src, tab);
      QG_HIP(hipSetDevice(ctx->device));
      if (first_missing) *first_missing = -1;
      // one context holds the whole table: both modes are the same flow
      const int64_t miss = lookup_run(ctx, ncols, src, src_len, tab, tab_len, out_m->d);
      lookup_report(miss, first_missing);
      return;
    }
    // sharded: lengths are this rank's block lengths.  The local checks never
    // end the call on their own: their status travels in the header, so that
    // every rank leaves here together or goes on together.
    QG_HIP(hipSetDevice(ctx->device));
    LkHeader mine{QG_OK, ncols, (uint64_t)src_len, (uint64_t)tab_len, (uint64_t)table_mode};
    std::string why;
    try {
      lk_check_mode(table_mode);
      const bool under = ncols <= LK_MAXCOLS && !lk_global_over(ctx->world, tab_len, 1ull << 31) &&
                         !lk_global_over(ctx->world, src_len, 1ull << 32);
      lookup_check_dev_args(ncols, src_cols, src_len, tab_cols, tab_len, out_m, under, src, tab);
    } catch (const Error& e) {
      mine.status = e.code;
      why = e.what();
    }
    const std::vector<LkHeader> all = lookup_exchange(ctx, mine);
    if (mine.status != QG_OK) throw Error(QG_ERR_INVALID, why);
    for (size_t r = 0; r < all.size(); r++) {
      QG_CHECK(all[r].status == QG_OK, QG_ERR_INVALID,
               "lookup multiplicities: rank " + std::to_string(r) + " failed its argument checks");
      QG_CHECK(all[r].ncols == ncols && all[r].src_len == src_len && all[r].tab_len == tab_len,
               QG_ERR_INVALID,
               "lookup multiplicities: rank " + std::to_string(r) +
                   " passed another ncols, src_len or tab_len (every rank passes the same)");
      QG_CHECK(all[r].mode == table_mode, QG_ERR_INVALID,
               "lookup multiplicities: rank " + std::to_string(r) +
                   " passed another table mode (every rank passes the same)");
    }
    lk_check_global(ctx->world, ncols, src_len, tab_len);
    if (first_missing) *first_missing = -1;
    const int64_t miss =
        table_mode == QG_LOOKUP_TABLE_PARTITIONED
            ? lookup_run_partitioned(ctx, ncols, src, src_len, tab, tab_len, out_m->d)
            : lookup_run_sharded(ctx, ncols, src, src_len, tab, tab_len, out_m->d);
    lookup_report(miss, first_missing);
  });
}

int qg_lookup_multiplicities_dev(qg_ctx* ctx, uint32_t ncols, const qg_buf* const* src_cols,
                                 size_t src_len, const qg_buf* const* tab_cols, size_t tab_len,
                                 qg_buf* out_m, int64_t* first_missing) {
  return qg_lookup_multiplicities_dev_ex(ctx, ncols, src_cols, src_len, tab_cols, tab_len, out_m,
                                         first_missing, QG_LOOKUP_TABLE_REPLICATED);
}

}  // extern "C"
