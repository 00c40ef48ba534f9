// CPU check of the MSM launch plan (quill-zkvm_amd/csrc/msm_plan.h): whole
// plans of the shapes the product runs, the geometry overrides that name no
// kernel instantiation, and the override parser.  256 CUs, one resident block
// per CU of the prefetching scatters.  Prints "ok <name>" per check; exits
// non-zero when one fails.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <utility>

#include "../../quill-zkvm_amd/csrc/msm_plan.h"

using namespace qg;

static int fails = 0;
static bool row_ok = true;
static void eq(const char* what, long long got, long long want) {
  if (got == want) return;
  printf("  %s = %lld, expected %lld\n", what, got, want);
  row_ok = false;
}
#define EQ(a, b) eq(#a, (long long)(a), (long long)(b))
static void row(const char* name) {
  printf("%s %s\n", row_ok ? "ok" : "FAIL", name);
  if (!row_ok) fails++;
  row_ok = true;
}

static const char* const VARS[] = {"QG_SORT_BLOCK_A", "QG_SORT_BLOCK_B", "QG_SORT_TILE",
                                   "QG_SORT_CHUNK",   "QG_SORT_GRID_A",  "QG_SORT_GRID_B",
                                   "QG_MSM_ROUNDS",   "QG_MSM_CPB",      "QG_MSM_ELOG",
                                   "QG_MSM_PF",       "QG_MSM_COOP",     "QG_MSM_EQSPLIT"};
using Env = std::initializer_list<std::pair<const char*, const char*>>;

static MsmShape shape(size_t n, int c, int W, int wsel, bool side) {
  MsmShape s;
  s.n = n, s.c = c, s.W = W, s.wsel = wsel, s.side = side, s.cus = 256;
  return s;
}

// the plan of shape s with exactly the overrides of `env` set in the environment
static MsmPlan plan(const MsmShape& s, Env env = {}) {
  for (const char* v : VARS) unsetenv(v);
  for (const auto& kv : env) setenv(kv.first, kv.second, 1);
  return msm_plan(s, msm_tuning_from_env(), [](char, int, size_t) { return 1; });
}

// the error code of that plan; 0: none
static int plan_error(const MsmShape& s, Env env) {
  try {
    plan(s, env);
  } catch (const Error& e) {
    return e.code;
  }
  return 0;
}

static void geom(const MsmPlan& p, uint32_t blkA, uint32_t tile, uint32_t blkB, uint32_t chunk,
                 bool wide) {
  EQ(p.geo.blkA, blkA);
  EQ(p.geo.tile, tile);
  EQ(p.geo.blkB, blkB);
  EQ(p.geo.chunk, chunk);
  EQ(p.geo.wide, wide);
}

int main() {
  const MsmShape headline = shape((size_t)1 << 24, 20, 13, -1, false);
  {  // the 2^24 headline: 13 x 2^24 entries
    const MsmPlan p = plan(headline);
    EQ(p.WE, 13), EQ(p.nb, 1u << 19), EQ(p.max_entries, (size_t)13 << 24);
    EQ(p.LO, 10), EQ(p.H, 512), EQ(p.NL, 1024);
    geom(p, 1024, 1024, 1024, 16384, true);
    EQ(p.nblk, 16384), EQ(p.nghist, (size_t)512 * 16384), EQ(p.max_chunks, 13825), EQ(p.ntiles, 256);
    EQ(p.smemA, 118848), EQ(p.smemB, 122944);  // both with the second row buffer
    EQ(p.gridA, 2048), EQ(p.gridB, 2048), EQ(p.pfA, true), EQ(p.pfB, true);
    EQ(p.L, 128), EQ(p.Lm, (~0ull >> 7) + 1), EQ(p.T, 6), EQ(p.pf, true), EQ(p.coop, true);
    EQ(p.max_threads, 1703936), EQ(p.nslots, 2228225);
    row("headline_2p24_c20");
  }
  {  // the same with one block per tile forced in pass A: no prefetch there
    const MsmPlan p = plan(headline, {{"QG_SORT_GRID_A", "0"}});
    EQ(p.gridA, 16384), EQ(p.pfA, false), EQ(p.smemA, 112704);
    EQ(p.gridB, 2048), EQ(p.pfB, true), EQ(p.smemB, 122944);
    row("headline_grid_a_0");
  }
  {  // a HyperPlonk opening: an MSM of a side-stream batch
    const MsmPlan p = plan(shape((size_t)1 << 20, 20, 13, -1, true));
    EQ(p.WE, 13), EQ(p.nb, 1u << 19), EQ(p.LO, 10), EQ(p.H, 512), EQ(p.NL, 1024);
    geom(p, 256, 512, 256, 8192, false);
    EQ(p.nblk, 2048), EQ(p.max_chunks, 2177), EQ(p.ntiles, 256);
    EQ(p.smemA, 59408), EQ(p.smemB, 61456);
    EQ(p.gridA, 2048), EQ(p.gridB, 2177), EQ(p.pfA, false), EQ(p.pfB, false);
    EQ(p.L, 52), EQ(p.T, 4), EQ(p.pf, false), EQ(p.coop, false);  // equal split, k = 1
    EQ(p.max_threads, 262144), EQ(p.nslots, 786433);
    row("side_2p20_c20");
  }
  {  // the same MSM alone on the context stream: the 512-thread class, L by the power-of-two rule
    const MsmPlan p = plan(shape((size_t)1 << 20, 20, 13, -1, false));
    geom(p, 512, 512, 512, 8192, false);
    EQ(p.smemA, 512 * 13 * 8 + (3 * 512 + 8) * 4), EQ(p.smemB, 8192 * 6 + (3 * 1024 + 8) * 4);
    EQ(p.gridA, 2048), EQ(p.gridB, 2177), EQ(p.pfA, false), EQ(p.pfB, false);
    EQ(p.L, 16), EQ(p.T, 4), EQ(p.coop, false);
    EQ(p.max_threads, 851968), EQ(p.nslots, 851968 + 524288 + 1);
    row("lone_2p20_c20");
  }
  const MsmShape small20 = shape((size_t)1 << 15, 13, 20, -1, false);
  {  // 20 windows: the tile steps down to the LDS budget
    const MsmPlan p = plan(small20);
    EQ(p.WE, 20), EQ(p.nb, 4096), EQ(p.LO, 6), EQ(p.H, 64), EQ(p.NL, 64);
    geom(p, 256, 256, 256, 8192, false);
    EQ(p.nblk, 128), EQ(p.max_chunks, 145), EQ(p.ntiles, 2);
    EQ(p.smemA, 41744), EQ(p.smemB, 49936);
    EQ(p.gridA, 128), EQ(p.gridB, 145), EQ(p.pfA, false), EQ(p.pfB, false);
    EQ(p.L, 64), EQ(p.T, 5), EQ(p.pf, false), EQ(p.coop, false);
    EQ(p.max_threads, 10240), EQ(p.nslots, 14337);
    row("lone_2p15_c13");
  }
  // ... where a tile of 1024 scalars cannot run at any block width
  EQ(plan_error(small20, {{"QG_SORT_TILE", "1024"}}), QG_ERR_UNSUPPORTED);
  row("lone_2p15_c13_tile_1024_unsupported");
  {  // wide by entries, but 1024 x 20 digits do not fit: pass A steps down to 512
    const MsmPlan p = plan(shape((size_t)1 << 22, 13, 20, -1, false));
    geom(p, 512, 512, 1024, 16384, true);
    EQ(p.nblk, 8192), EQ(p.max_chunks, 5185);
    EQ(p.gridA, 8192), EQ(p.pfA, false), EQ(p.smemA, 82720);  // one block per tile
    EQ(p.gridB, 2048), EQ(p.pfB, true), EQ(p.smemB, 99904);   // multi-tile
    EQ(p.L, 128), EQ(p.T, 162), EQ(p.pf, false), EQ(p.coop, true);
    EQ(p.max_threads, 655360), EQ(p.nslots, 659457);
    row("lone_2p22_c13");
  }
  {  // one window of one-shot bases
    const MsmPlan p = plan(shape((size_t)1 << 20, 20, 13, 3, false));
    EQ(p.WE, 1), EQ(p.max_entries, (size_t)1 << 20);
    geom(p, 256, 1024, 256, 8192, false);
    EQ(p.nblk, 1024), EQ(p.max_chunks, 641), EQ(p.smemA, 14352), EQ(p.smemB, 61456);
    EQ(p.gridA, 1024), EQ(p.gridB, 641), EQ(p.pfA, false), EQ(p.pfB, false);
    EQ(p.L, 4), EQ(p.T, 4), EQ(p.coop, false);
    EQ(p.max_threads, 262144), EQ(p.nslots, 786433);
    row("oneshot_window_2p20_c20");
  }
  // geometries without a kernel instantiation (tests/test_gpu_sort_geometry.py)
  const MsmShape s1027 = shape(1027, 20, 13, -1, false);
  const Env bad[] = {
      {{"QG_SORT_BLOCK_A", "384"}},
      {{"QG_SORT_BLOCK_A", "128"}},
      {{"QG_SORT_BLOCK_A", "2048"}, {"QG_SORT_TILE", "1024"}},
      {{"QG_SORT_BLOCK_A", "1024"}, {"QG_SORT_TILE", "512"}},
      {{"QG_SORT_BLOCK_A", "512"}, {"QG_SORT_TILE", "256"}},
      {{"QG_SORT_TILE", "768"}},
      {{"QG_SORT_BLOCK_B", "256"}, {"QG_SORT_CHUNK", "16384"}},
      {{"QG_SORT_BLOCK_B", "1024"}, {"QG_SORT_CHUNK", "8192"}},
      {{"QG_SORT_BLOCK_B", "512"}, {"QG_SORT_CHUNK", "4096"}},
      {{"QG_SORT_CHUNK", "0"}},
      {{"QG_SORT_BLOCK_B", "64"}},
  };
  for (const Env& e : bad) EQ(plan_error(s1027, e), QG_ERR_INVALID);
  row("geometry_without_instantiation_invalid");
  // ... and every instantiated one is accepted
  for (const char* chunk : {"8192", "16384"}) {
    EQ(plan_error(s1027, {{"QG_SORT_BLOCK_A", "256"}, {"QG_SORT_TILE", "64"},
                          {"QG_SORT_BLOCK_B", "512"}, {"QG_SORT_CHUNK", chunk}}), 0);
    EQ(plan_error(s1027, {{"QG_SORT_BLOCK_A", "512"}, {"QG_SORT_TILE", "1024"},
                          {"QG_SORT_BLOCK_B", "512"}, {"QG_SORT_CHUNK", chunk}}), 0);
  }
  EQ(plan_error(s1027, {{"QG_SORT_BLOCK_A", "1024"}, {"QG_SORT_TILE", "1024"},
                        {"QG_SORT_BLOCK_B", "1024"}, {"QG_SORT_CHUNK", "16384"}}), 0);
  row("instantiated_geometries_accepted");
  // forced scatter grids: any count in [0, 2^20]
  EQ(plan(s1027, {{"QG_SORT_GRID_A", "0"}}).gridA, 3);  // one per tile of 512
  EQ(plan(s1027, {{"QG_SORT_GRID_A", "8"}}).gridA, 8);
  EQ(plan(s1027, {{"QG_SORT_GRID_A", "1048576"}}).gridA, 1048576);
  EQ(plan_error(s1027, {{"QG_SORT_GRID_A", "1048577"}}), QG_ERR_INVALID);
  EQ(plan(s1027, {{"QG_SORT_GRID_B", "8"}}).gridB, 8);
  EQ(plan_error(s1027, {{"QG_SORT_GRID_B", "-1"}}), QG_ERR_INVALID);
  {  // a forced grid below the tile count takes the prefetching form where it exists
    const MsmPlan p = plan(s1027, {{"QG_SORT_BLOCK_A", "1024"}, {"QG_SORT_TILE", "1024"},
                                   {"QG_SORT_GRID_A", "1"}});
    EQ(p.nblk, 2), EQ(p.gridA, 1), EQ(p.pfA, true);
  }
  row("forced_scatter_grids");
  // the accumulate overrides
  EQ(plan(headline, {{"QG_MSM_ELOG", "6"}}).L, 64);
  EQ(plan(headline, {{"QG_MSM_ELOG", "16"}}).L, 65536);
  EQ(plan(headline, {{"QG_MSM_ROUNDS", "2"}}).L, 512);  // 2 rounds of 2^18 resident threads
  EQ(plan(headline, {{"QG_MSM_CPB", "1"}}).L, 128);     // capped at 2^7
  EQ(plan(small20, {{"QG_MSM_CPB", "8"}}).L, 32);
  EQ(plan(small20, {{"QG_MSM_CPB", "0"}}).L, plan(small20, {{"QG_MSM_CPB", "1"}}).L);
  EQ(plan(small20, {{"QG_MSM_CPB", "-3"}}).L, plan(small20, {{"QG_MSM_CPB", "1"}}).L);
  EQ(plan(headline, {{"QG_MSM_COOP", "0"}}).coop, false);
  EQ(plan(headline, {{"QG_MSM_COOP", "0"}}).pf, true);
  EQ(plan(headline, {{"QG_MSM_PF", "0"}}).pf, false);
  EQ(plan(small20, {{"QG_MSM_COOP", "1"}}).coop, true);
  EQ(plan(headline, {{"QG_MSM_EQSPLIT", "1"}}).L, 1112);  // 13 x 2^24 / (256 x 4 x 3 x 64) -> 4 | L
  EQ(plan(headline, {{"QG_MSM_EQSPLIT", "1"}, {"QG_MSM_COOP", "0"}, {"QG_MSM_PF", "0"}}).L, 832);
  EQ(plan(shape((size_t)1 << 20, 20, 13, -1, true), {{"QG_MSM_EQSPLIT", "0"}}).L, 16);
  row("accumulate_overrides");
  // the parser: whole numbers in range, nothing else
  for (const Env& e : {Env{{"QG_MSM_ELOG", "1"}}, Env{{"QG_MSM_ELOG", "17"}},
                       Env{{"QG_MSM_ELOG", "32"}}, Env{{"QG_MSM_EQSPLIT", "-1"}},
                       Env{{"QG_MSM_ROUNDS", "0"}}, Env{{"QG_MSM_ROUNDS", "65"}},
                       Env{{"QG_MSM_PF", "1x"}}, Env{{"QG_MSM_COOP", "yes"}},
                       Env{{"QG_MSM_CPB", ""}}, Env{{"QG_SORT_TILE", "512 "}},
                       Env{{"QG_SORT_BLOCK_A", "99999999999999999999"}},
                       Env{{"QG_SORT_GRID_A", "8.0"}}})
    EQ(plan_error(headline, e), QG_ERR_INVALID);
  {
    for (const char* v : VARS) unsetenv(v);
    const MsmTuning t = msm_tuning_from_env();
    EQ(t.sort_block_a.has_value() || t.sort_grid_b.has_value() || t.elog.has_value() ||
           t.eqsplit.has_value(), false);
    setenv("QG_MSM_PF", " +1", 1);  // what strtol takes, as atoi did
    EQ(msm_tuning_from_env().pf.value_or(0), 1);
    unsetenv("QG_MSM_PF");
  }
  row("override_parser");
  return fails ? 1 : 0;
}
