// The launch plan of one MSM's bucketing and accumulation (msm.hip): every
// size, geometry and kernel form msm_accumulate_phase launches with, from the
// MSM's shape and the tuning overrides alone.  Pure host integers - no HIP -
// so tests/cpp/msm_plan_check.cpp pins whole plans on the CPU.
#pragma once
#include <errno.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <optional>
#include <string>

#include "../../include/quill_gpu.h"
#include "error.h"

namespace qg {

static constexpr int SORT_BLOCK = 256;                      // k_sortA_hist, and the narrowest BLK
static constexpr int SORT_TILE_MAX = 1024;                  // scalars per block (pass A)
static constexpr size_t SORT_LDS_A = 72 * 1024;             // LDS budget for staged entries (2 blocks/CU)
static constexpr int SORT_CHUNK = 8192;                     // entries per block (pass B), 256-thread blocks
static constexpr int SORT_H_MAX = 1024, SORT_NL_MAX = 4096; // most groups / buckets per group

// exclusive scan of (count, ceil(count/E)) over nb buckets: k_scan_tiles
static constexpr int SCAN_PER_THREAD = 8;
static constexpr int SCAN_BLOCK = 256;
static constexpr int SCAN_TILE = SCAN_PER_THREAD * SCAN_BLOCK;

// resident waves per SIMD of k_msm_accumulate_coop
#ifndef QG_COOP_WPE
#define QG_COOP_WPE 3
#endif

// The tuning overrides of the bucketing and the accumulation (A/B runs and
// tuning experiments), by the name of their environment variable; unset: the
// rule of msm_plan decides.
struct MsmTuning {
  std::optional<int> sort_block_a, sort_block_b;  // QG_SORT_BLOCK_A / _B
  std::optional<int> sort_tile, sort_chunk;       // QG_SORT_TILE, QG_SORT_CHUNK
  std::optional<int> sort_grid_a, sort_grid_b;    // QG_SORT_GRID_A / _B
  std::optional<int> rounds;                      // QG_MSM_ROUNDS
  std::optional<int> cpb;                         // QG_MSM_CPB
  std::optional<int> elog;                        // QG_MSM_ELOG
  std::optional<int> pf, coop;                    // QG_MSM_PF, QG_MSM_COOP
  std::optional<int> eqsplit;                     // QG_MSM_EQSPLIT
};

static constexpr int SORT_GRID_MAX = 1 << 20;

// one override: unset, or a whole decimal number in [lo, hi]
inline std::optional<int> msm_env_int(const char* name, long lo, long hi) {
  const char* ov = getenv(name);
  if (!ov) return std::nullopt;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(ov, &end, 10);
  QG_CHECK(end != ov && *end == 0 && errno == 0 && v >= lo && v <= hi, QG_ERR_INVALID,
           std::string(name) + " must be a whole number in [" + std::to_string(lo) + ", " +
               std::to_string(hi) + "]");
  return (int)v;
}

// Read per MSM: tests and A/B harnesses toggle the variables in-process.
inline MsmTuning msm_tuning_from_env() {
  MsmTuning t;
  t.sort_block_a = msm_env_int("QG_SORT_BLOCK_A", 0, INT_MAX);
  t.sort_block_b = msm_env_int("QG_SORT_BLOCK_B", 0, INT_MAX);
  t.sort_tile = msm_env_int("QG_SORT_TILE", 0, INT_MAX);
  t.sort_chunk = msm_env_int("QG_SORT_CHUNK", 0, INT_MAX);
  t.sort_grid_a = msm_env_int("QG_SORT_GRID_A", 0, SORT_GRID_MAX);
  t.sort_grid_b = msm_env_int("QG_SORT_GRID_B", 0, SORT_GRID_MAX);
  t.rounds = msm_env_int("QG_MSM_ROUNDS", 1, 64);
  t.cpb = msm_env_int("QG_MSM_CPB", INT_MIN, INT_MAX);  // below 1 counts as 1
  t.elog = msm_env_int("QG_MSM_ELOG", 2, 16);
  t.pf = msm_env_int("QG_MSM_PF", INT_MIN, INT_MAX);
  t.coop = msm_env_int("QG_MSM_COOP", INT_MIN, INT_MAX);
  t.eqsplit = msm_env_int("QG_MSM_EQSPLIT", 0, INT_MAX);
  return t;
}

// Launch geometry of the sort kernels: pass A's scatter / rows kernels run
// blkA threads over a tile of `tile` scalars, pass B's kernels blkB threads
// over a chunk of `chunk` entries.  Only the instantiated pairs are valid:
//   pass A: 256 threads with any tile, 512 with tile 512 / 1024, 1024 with 1024
//   pass B: (256, 8192), (512, 8192), (512, 16384), (1024, 16384)
// wide: the class whose scatter blocks walk several tiles each by default
// (sort_scatter_grid)
struct SortGeom {
  uint32_t blkA, tile, blkB, chunk;
  bool wide;
};

// The default by the MSM's entries (profiles/r08_sort_block_ab.txt; bucketing
// ms with 256- / 512- / 1024-thread blocks, the last over tile 1024 and chunk
// 16384): 2^26 entries and more take 1024 threads (13 x 2^24: 2.41 / 2.20 /
// 2.02, 13 x 2^23: 1.26 / 1.13 / 1.06), 2^20 and more 512 threads over the same
// tile and chunk as before (13 x 2^22: 0.674 / 0.576 / 0.587, 15 x 2^20 at
// c = 17: 0.200 / 0.174 / 0.192, 17 x 2^16: 0.088 / 0.079 / 0.087), fewer keep
// 256 (24 x 2^12: 0.076 / 0.078).  QG_SORT_BLOCK_A / QG_SORT_TILE /
// QG_SORT_BLOCK_B / QG_SORT_CHUNK override (A/B runs); a combination without
// an instantiation is QG_ERR_INVALID.  QG_SORT_GRID_A / QG_SORT_GRID_B force
// the scatters' block counts (0 = one block per tile / chunk; any count up to
// SORT_GRID_MAX runs, a multiple of 8 keeps a block's tiles on one XCD; blocks
// beyond the tile count exit at once); out of range is QG_ERR_INVALID.
// side: an MSM of a batch on the side streams, whose bucketing runs beside the
// other stream's accumulation, keeps 256 threads: with the wider blocks
// HyperPlonk's side bucketing gained 1-4 ms per proof and the accumulation
// beside it lost 24-34 ms (proof 848-854 -> 870-872 ms).  The windows of
// one-shot bases (wsel >= 0) keep it too: 2^20 bases measured 1.93 -> 1.85 ms of
// bucketing with 512 threads, but the 2^24 bench leg 27.3 -> 27.4-27.6 ms.
static constexpr size_t SORT_WIDE_MIN = (size_t)1 << 26;
static constexpr size_t SORT_MID_MIN = (size_t)1 << 20;
inline SortGeom sort_geometry(size_t max_entries, int WE, bool narrow, const MsmTuning& tn) {
  SortGeom g;
  const bool wide = !narrow && max_entries >= SORT_WIDE_MIN;
  const bool mid = !narrow && max_entries >= SORT_MID_MIN;
  g.blkA = wide ? 1024 : mid ? 512 : SORT_BLOCK;
  g.blkB = wide ? 1024 : mid ? 512 : SORT_BLOCK;
  g.chunk = wide ? 16384 : SORT_CHUNK;
  g.wide = wide;
  // a block stages at least one scalar per thread: with many windows (small c)
  // the wide tile does not fit the CU's LDS, and the default steps down
  while (g.blkA > (uint32_t)SORT_BLOCK &&
         (size_t)g.blkA * WE * 8 + (3 * (size_t)SORT_H_MAX + 16) * 4 > 160 * 1024)
    g.blkA >>= 1;
  if (tn.sort_block_a) g.blkA = (uint32_t)*tn.sort_block_a;
  if (tn.sort_block_b) g.blkB = (uint32_t)*tn.sort_block_b;
  if (tn.sort_chunk) g.chunk = (uint32_t)*tn.sort_chunk;
  // pass-A tile: as many scalars as fit their WE digits (8 B each) in the LDS
  // budget of 256-thread blocks; a wider block takes at least its own width
  g.tile = SORT_TILE_MAX;
  while (g.tile > 64 && (size_t)g.tile * WE * 8 > SORT_LDS_A) g.tile >>= 1;
  if (g.blkA > SORT_BLOCK && g.blkA <= (uint32_t)SORT_TILE_MAX) g.tile = std::max(g.tile, g.blkA);
  if (tn.sort_tile) g.tile = (uint32_t)*tn.sort_tile;
  QG_CHECK(g.tile >= 64 && g.tile <= (uint32_t)SORT_TILE_MAX && (g.tile & (g.tile - 1)) == 0,
           QG_ERR_INVALID, "QG_SORT_TILE must be a power of two in [64, 1024]");
  QG_CHECK(g.blkA == 256 || ((g.blkA == 512 || g.blkA == 1024) && g.tile >= g.blkA),
           QG_ERR_INVALID, "no pass-A sort kernel for this QG_SORT_BLOCK_A / QG_SORT_TILE");
  QG_CHECK((g.blkB == 256 && g.chunk == 8192) || (g.blkB == 512 && g.chunk == 8192) ||
               (g.blkB == 512 && g.chunk == 16384) || (g.blkB == 1024 && g.chunk == 16384),
           QG_ERR_INVALID, "no pass-B sort kernel for this QG_SORT_BLOCK_B / QG_SORT_CHUNK");
  return g;
}

// Blocks of a scatter kernel.  forced > 0: that many; 0: one per tile.  The
// default (unset) is one per tile too, except where `multi` (the wide class with
// the prefetching instantiation): SORT_GRID_ROUNDS times the blocks the device
// holds at once (the kernel's occupancy at this LDS size x CUs), a multiple
// of 8 so that a block's tiles stay in one XCD's range, at most one per tile.
// Exactly the resident count measured no better than one block per tile
// (2^24 bucketing 2.02 ms both; the slowest CU sets the time), 4 and 8 rounds
// of blocks, which the dispatcher hands to whichever CU is free, 1.93 / 1.90
// (profiles/r09_sort_pipeline_ab.txt).
// occ(): the kernel's resident blocks per CU, asked only for that default.
static constexpr size_t SORT_GRID_ROUNDS = 8;
template <class Occ>
uint32_t sort_scatter_grid(std::optional<int> forced, bool multi, size_t count, int cus, Occ&& occ) {
  QG_CHECK(!forced || (*forced >= 0 && *forced <= SORT_GRID_MAX), QG_ERR_INVALID,
           "QG_SORT_GRID_A / QG_SORT_GRID_B must be a block count in [0, 2^20]");
  if (forced && *forced > 0) return (uint32_t)*forced;
  if (forced || !multi) return (uint32_t)count;
  const int per_cu = occ();
  QG_CHECK(per_cu >= 1, QG_ERR_DEVICE, "sort scatter kernel cannot be resident");
  const size_t blocks = (((size_t)per_cu * cus) & ~(size_t)7) * SORT_GRID_ROUNDS;
  return (uint32_t)(blocks >= 8 && blocks < count ? blocks : count);
}

// An MSM run as the plan sees it: n > 0 scalars over an SRS of W windows of c
// bits; wsel >= 0: the digits of window wsel only (one-shot bases), -1: every
// window; side: on a side stream of a batch; cus: the device's compute units.
struct MsmShape {
  size_t n;
  int c, W, wsel;
  bool side;
  int cus;
};

struct MsmPlan {
  int WE;              // digits per scalar this run bins
  uint32_t nb;         // buckets
  size_t max_entries;  // n * WE
  int LO, H, NL;       // bucket id b = (g << LO) | l: H groups of NL buckets
  SortGeom geo;
  uint32_t nblk;      // pass-A tiles
  size_t nghist;      // H * nblk
  size_t max_chunks;  // bound of pass B's chunks
  int ntiles;         // tiles of the bucket scan
  uint32_t L;         // entries per accumulation thread
  uint64_t Lm;        // msm_chunk_of's multiplier
  uint32_t T;         // partial slots the reduction adds in a row
  size_t max_threads, nslots;
  bool pf, coop;         // the accumulate form
  size_t smemA, smemB;   // dynamic LDS of the two scatters
  uint32_t gridA, gridB; // their blocks
  bool pfA, pfB;         // the prefetching instantiation (<1024, true>)
};

inline size_t msm_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// occ(pass, blk, smem): resident blocks per CU of the prefetching scatter of
// pass 'A' / 'B' with blk threads and smem bytes of dynamic LDS - the only
// thing the plan asks of the device.  Every error of an MSM's shape or its
// overrides is raised here, before anything is queued.
template <class Occ>
MsmPlan msm_plan(const MsmShape& s, const MsmTuning& tn, Occ&& occ) {
  MsmPlan p{};
  const int c = s.c, cus = s.cus;
  const bool side = s.side;
  const int WE = p.WE = s.wsel < 0 ? s.W : 1;
  const uint32_t nb = p.nb = 1u << (c - 1);
  const size_t max_entries = p.max_entries = s.n * (size_t)WE;
  QG_CHECK(max_entries < 0xffffffffull, QG_ERR_UNSUPPORTED, "too many MSM entries");
  // bucket id b = (g << LO) | l
  const int BB = c - 1, LO = (BB + 1) / 2, HI = BB - LO;
  const int H = 1 << HI, NL = 1 << LO;
  p.LO = LO, p.H = H, p.NL = NL;
  const SortGeom geo = p.geo = sort_geometry(max_entries, WE, side || s.wsel >= 0, tn);
  const uint32_t tile = geo.tile, chunk = geo.chunk;
  const uint32_t nblk = p.nblk = (uint32_t)msm_ceil_div(s.n, tile);
  p.nghist = (size_t)H * nblk;
  const size_t max_chunks = p.max_chunks = max_entries / chunk + H + 1;
  p.ntiles = (int)msm_ceil_div(nb, SCAN_TILE);
  // entries per accumulation thread (flat chunks, k_msm_accumulate): 64, or
  // 128 for the largest MSMs, fewer while that would leave < 3 waves of
  // threads per resident slot (256 CUs x 16 waves).  Measured against equal
  // splits into 1 / 2 / 3 whole waves of the chip (QG_MSM_ROUNDS, which also
  // leave fewer partials for the reduction): the accumulate loses 0.3-0.5 ms
  // at 2^24 with 1-2 waves, and 3 waves is no faster than 128 entries.
  uint32_t L;
  if (tn.rounds) {  // tuning experiments
    const int rounds = *tn.rounds;
    QG_CHECK(rounds >= 1 && rounds <= 64, QG_ERR_INVALID, "QG_MSM_ROUNDS out of range");
    const size_t resident = (size_t)cus * 16 * 64;
    L = 4;  // a power of two (k_msm_accumulate takes log2 L), rounded up
    while ((size_t)L * resident * rounds < max_entries) L <<= 1;
  } else {
    int elog = max_entries >= ((size_t)1 << 27) ? 7 : 6;
    while (elog > 2 && (max_entries >> elog) < (size_t)cus * 16 * 64 * 3) elog--;
    // but at most ~4 chunks per bucket: below that the reduction's slot
    // merges cost more than the accumulation gains from the extra threads
    // (own-SRS MSMs, profiles/r04_msm_small_elog.txt: 2^20 / 2^18 / 2^16 at
    // c = 17 / 16 / 15 take 1.73 / 1.09 / 0.73 ms with the thread rule alone,
    // 1.69 / 0.87 / 0.69 ms with 64 / 32 / 32 entries per chunk)
    // In a batch on the side streams (HyperPlonk's openings: 2^20-2^23-scalar
    // MSMs on the c = 20 tables, many buckets per MSM) at most ~2 chunks per
    // bucket: fewer partial slots to merge, HyperPlonk reduce 73.5 / 73.9 ->
    // 63.5 / 63.3 ms per proof, proof 879.7 / 878.3 -> 872.0 / 871.7 ms
    // (profiles/r06e_msm_cpb_ab.txt); a lone MSM keeps 4 (the 2^24 headline
    // measured no better with 2).  QG_MSM_CPB overrides (A/B runs).
    int emin = 0;
    size_t cpb = side ? 2 : 4;
    if (tn.cpb) cpb = (size_t)std::max(1, *tn.cpb);
    while (emin < 7 && ((size_t)1 << emin) * cpb * nb < max_entries) emin++;
    elog = std::max(elog, emin);
    L = 1u << elog;
  }
  if (tn.elog) {  // tuning experiments
    QG_CHECK(*tn.elog >= 2 && *tn.elog <= 16, QG_ERR_INVALID, "QG_MSM_ELOG out of range");
    L = 1u << *tn.elog;
  }
  // the accumulate form (msm_accumulate_launch) and its resident waves per SIMD
  bool pf = max_entries >= ((size_t)1 << 27);
  if (tn.pf) pf = *tn.pf != 0;
  bool coop = max_entries >= ((size_t)1 << 25);
  if (tn.coop) coop = *tn.coop != 0;
  p.pf = pf, p.coop = coop;
  // Equal chunks (any multiple of 4 entries) filling exactly k rounds of the
  // chip's resident waves: no partly-filled last round, and fewer, longer
  // chunks leave fewer partial slots per bucket for the reduction.  The MSMs
  // of a side-stream batch take k = 1: HyperPlonk 866.9 / 870.6 -> 847.1 /
  // 850.5 ms per proof, its reduce 63.3 -> 52.1 ms (the accumulate itself
  // slower, the other stream's bucketing beside it faster), 2^24 headline
  // unchanged (profiles/r06g_msm_eqsplit_ab.txt).  A lone MSM keeps the
  // power-of-two rule: with k = 1 / 2 / 3 the 2^24 accumulate is 1.4 / 0.7 /
  // 0.5 ms slower for a reduction 0.20 / 0.10 / 0.18 ms faster (the waves of
  // one round do not finish together; many rounds even them out).
  // QG_MSM_EQSPLIT=k overrides (0: the power-of-two rule; A/B runs).
  const int eqk = tn.eqsplit ? *tn.eqsplit : (side ? 1 : 0);
  QG_CHECK(eqk >= 0, QG_ERR_INVALID, "QG_MSM_EQSPLIT out of range");
  if (eqk > 0) {
    const size_t wpe = coop ? QG_COOP_WPE : (pf ? 3 : 4);
    const size_t resident = (size_t)cus * 4 * wpe * 64;
    const size_t lq = (msm_ceil_div(max_entries, resident * (size_t)eqk) + 3) & ~(size_t)3;
    L = (uint32_t)std::max<size_t>(4, lq);
  }
  // partial slots a bucket's sum adds in a row in the reduction: the typical
  // count + 1 (a bucket of c entries spans ceil(c / L) or one more slots);
  // skewed buckets beyond it are pre-summed by tree steps
  p.T = std::max<uint32_t>(4, (uint32_t)msm_ceil_div(msm_ceil_div(max_entries, nb), L) + 2);
  // k_msm_accumulate takes the group phase of entry e as e & 3: chunks start
  // at multiples of 4
  QG_CHECK(L >= 4 && L <= 65536 && (L & 3u) == 0, QG_ERR_INVALID, "MSM chunk length out of range");
  p.L = L;
  p.Lm = ~0ull / L + 1;  // msm_chunk_of's multiplier
  p.max_threads = msm_ceil_div(max_entries, L);
  p.nslots = p.max_threads + nb + 1;  // partial slot of (thread t, bucket b): t + b
  QG_CHECK(p.ntiles <= 1024 * 64 && H <= SORT_H_MAX && NL <= SORT_NL_MAX, QG_ERR_UNSUPPORTED,
           "bucket count too large");
  // dynamic LDS of the two scatters: staged entries, three count / offset
  // rows, the scan's wave totals
  p.smemA = (size_t)tile * WE * 8 + (3 * (size_t)H + geo.blkA / 64) * 4;
  p.smemB = (size_t)chunk * 6 + (3 * (size_t)NL + geo.blkB / 64) * 4;
  QG_CHECK(p.smemA <= 160 * 1024 && p.smemB <= 160 * 1024, QG_ERR_UNSUPPORTED,
           "sort tile / chunk exceeds LDS");
  // The scatters' grids.  Fewer blocks than tiles / chunks: the 1024-thread
  // kernels prefetch the next tile (a second row buffer in LDS, where it
  // fits); the narrower ones walk their tiles without (no measured case for
  // them).
  const size_t smemA2 = p.smemA + 3 * (size_t)H * 4, smemB2 = p.smemB + 3 * (size_t)NL * 4;
  const bool canA = geo.blkA == 1024 && smemA2 <= 160 * 1024;
  const bool canB = geo.blkB == 1024 && smemB2 <= 160 * 1024;
  p.gridA = sort_scatter_grid(tn.sort_grid_a, geo.wide && canA, nblk, cus,
                              [&] { return occ('A', 1024, smemA2); });
  p.gridB = sort_scatter_grid(tn.sort_grid_b, geo.wide && canB, max_chunks, cus,
                              [&] { return occ('B', 1024, smemB2); });
  p.pfA = canA && p.gridA < nblk;
  p.pfB = canB && p.gridB < max_chunks;
  if (p.pfA) p.smemA = smemA2;
  if (p.pfB) p.smemB = smemB2;
  QG_CHECK(p.nslots < 0xffffffffull && max_chunks < 0xffffffffull, QG_ERR_UNSUPPORTED,
           "MSM too large");
  QG_CHECK(msm_ceil_div(p.nghist, 2048) <= 1024u * 1024u, QG_ERR_UNSUPPORTED, "histogram too large");
  return p;
}

}  // namespace qg
