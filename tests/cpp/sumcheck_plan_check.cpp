// CPU check of the sumcheck prover's host-side decisions
// (quill-zkvm_amd/csrc/sumcheck_plan.h): whole plans of the headline, a sop
// and a staged proof, the sharded gather round, the buffer rule, the io
// region's layout and the switch parser.  Prints "ok <name>" per check; exits
// non-zero when one fails.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <utility>

#include "../../quill-zkvm_amd/csrc/sumcheck_plan.h"

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

static const char* const VARS[] = {"QG_SC_PERS_LOG", "QG_SC_BIG_BLOCKS", "QG_SC_BLOCKS",
                                   "QG_SC_STAGED",   "QG_SC_NO_SKIP0",   "QG_SC_OLD_TAIL",
                                   "QG_SC_WPE",      "QG_SC_TAIL_BPC"};
using Env = std::initializer_list<std::pair<const char*, const char*>>;

// the switches with exactly `env` set in the environment
static ScSwitches switches(Env env = {}) {
  for (const char* v : VARS) unsetenv(v);
  for (const auto& kv : env) setenv(kv.first, kv.second, 1);
  return sc_switches();
}
static int switch_error(Env env) {
  try {
    switches(env);
  } catch (const Error& e) {
    return e.code;
  }
  return 0;
}

// one GPU of `cus` CUs whose tails have `occ` resident blocks per CU: the
// plan of a proof as run_rounds derives it
struct Plan {
  ScInstance in;
  ScBig form;
  uint32_t j0;
  size_t tail_grid;  // blocks of the slice tail; 0: the streaming tail runs
};
static Plan plan(uint32_t nvars, uint32_t nslots, uint32_t np, bool pure, const ScSwitches& sw,
                 size_t cus = 256, int occ = 2) {
  Plan p;
  p.in = sc_instance(nslots, np);
  p.form = sc_big_form(p.in, pure, sw);
  const size_t gmax = slice_gmax(p.in.K, tail_grid_cap(occ, cus, sw), sw);
  p.j0 = sc_first_tail_round(nvars, sw, slice_tail_log(p.in.K, gmax));
  p.tail_grid = slice_grid(p.in.K, gmax, (size_t)1 << (nvars - p.j0));
  return p;
}

struct Elt {
  unsigned char b[32];
};
using Bufs = RoundBufsT<Elt>;

// the rule over rounds j0..nvars-1 (and the large rounds before, when jin ==
// 1) of tables whose round-j table has 2^(nvars - j) entries per slot
static void check_bufs(const Bufs& b, uint32_t first, uint32_t nvars) {
  for (uint32_t j = std::max(first, 1u); j < nvars; j++) {
    const size_t table = (size_t)1 << (nvars - j);  // entries round j writes
    for (uint32_t s = 0; s < 8; s += 7) {
      if (j > b.jin) EQ(b.src(j, s) == b.dst(j - 1, s), 1);
      if (j <= b.jin) EQ(b.src(j, s) == b.in[s], 1);
      EQ(b.src(j, s) != b.dst(j, s), 1);
    }
    EQ(((j & 1) ? b.capX : b.capY) >= table, 1);
    // slot s ends where slot s + 1 begins at the latest
    EQ(b.dst(j, 1) - b.dst(j, 0) >= (ptrdiff_t)table, 1);
  }
}

// the io region's size before ScIo, spelled out
static size_t parent_io_bytes(uint32_t nvars, uint32_t width) {
  const size_t o_bar8 = (192 + 4 * ((size_t)nvars + 2) + 127) / 128 * 128;
  const size_t o_chal = o_bar8 + 8 * 128 + 8 * 16 * 9 * 8;
  return o_chal + 32 * (size_t)nvars + 32 * (size_t)nvars * width + 32 * 9 + 4 * (size_t)nvars;
}

int main() {
  {  // the 2^20 headline: h = g0 g1 g2, nothing set, 256 CUs
    const ScSwitches sw = switches();
    const Plan p = plan(20, 3, 4, true, sw);
    EQ(p.in.K, 4);
    EQ(p.in.NP, 4);
    EQ(p.form == ScBig::pure, 1);
    EQ(p.j0, 4);  // 4 pure rounds, the slice tail from 2^16 entries
    EQ(p.tail_grid, 256);
    for (uint32_t j = 0; j < 4; j++) {
      // 2 per CU; round 3 has 2^16 pairs, one block of 256 each
      EQ(sc_round_grid(p.form, 256, ((size_t)1 << 20 >> j) / 2, sw), j < 3 ? 512 : 256);
      EQ(sc_skip0(p.form, 4, j, sw), j >= 1);
    }
    row("headline_2p20");
  }
  {  // 3 tables at degree 2, not a product: the sop form of k_sc_big
    const ScSwitches sw = switches();
    const Plan p = plan(18, 3, 3, false, sw);
    EQ(p.in.K, 4);
    EQ(p.in.NP, 4);
    EQ(p.form == ScBig::sop, 1);
    EQ(p.j0, 2);
    EQ(sc_round_grid(p.form, 256, (size_t)1 << 17, sw), 512);
    EQ(sc_round_grid(p.form, 256, (size_t)1 << 16, sw), 256);  // fewer pair groups than the cap
    EQ(sc_skip0(p.form, 3, 1, sw), 1);
    EQ(sc_skip0(p.form, 3, 1, switches({{"QG_SC_NO_SKIP0", "1"}})), 0);
    EQ(sc_big_form(p.in, false, switches({{"QG_SC_BIG_BLOCKS", "3"}})) == ScBig::sop, 1);
    EQ(sc_round_grid(p.form, 256, (size_t)1 << 17, switches({{"QG_SC_BIG_BLOCKS", "3"}})), 3);
    row("sop_2p18");
  }
  {  // 8 tables at degree 3: <8,4>, the staged kernel, 3 blocks per CU, no skip-0;
     // the <8,*> slice holds 128 entries per block: 128 blocks, 2^14 entries
    const ScSwitches sw = switches();
    const Plan p = plan(16, 8, 4, false, sw);
    EQ(p.in.K, 8);
    EQ(p.in.NP, 4);
    EQ(p.form == ScBig::staged, 1);
    EQ(p.j0, 2);
    EQ(p.tail_grid, 128);
    EQ(sc_round_grid(p.form, 256, (size_t)1 << 20, sw), 768);
    EQ(sc_round_grid(p.form, 256, (size_t)1 << 20, switches({{"QG_SC_BLOCKS", "5"}})), 5);
    EQ(sc_skip0(p.form, 4, 1, sw), 0);
    // the other staged instances, a product of 8 tables (pure), and QG_SC_STAGED
    EQ(sc_big_form(sc_instance(4, 8), false, sw) == ScBig::staged, 1);
    EQ(sc_big_form(sc_instance(5, 5), true, sw) == ScBig::staged, 1);
    EQ(sc_instance(5, 5).K * 100 + sc_instance(5, 5).NP, 808);
    EQ(sc_instance(2, 13).K * 100 + sc_instance(2, 13).NP, 816);
    EQ(sc_big_form(sc_instance(8, 4), true, sw) == ScBig::pure, 1);
    EQ(sc_big_form(sc_instance(3, 4), true, switches({{"QG_SC_STAGED", "1"}})) == ScBig::staged, 1);
    row("staged_2p16");
  }
  {  // small shapes and the streaming tail
    const ScSwitches p6 = switches({{"QG_SC_PERS_LOG", "6"}});
    EQ(plan(12, 3, 4, true, p6).j0, 6);
    EQ(plan(12, 3, 4, true, p6).tail_grid, 32);  // 2^6 entries: 32 blocks of one pair
    EQ(plan(9, 3, 4, true, p6).j0, 3);
    EQ(plan(5, 3, 4, true, p6).j0, 0);
    const ScSwitches old = switches({{"QG_SC_OLD_TAIL", "1"}});
    EQ(plan(20, 3, 4, true, old).j0, 4);  // pers_log alone decides
    EQ(plan(20, 3, 4, true, old).tail_grid, 0);
    EQ(switches({{"QG_SC_OLD_TAIL", "0"}}).old_tail, 0);
    EQ(stream_grid(256, (size_t)1 << 15, tail_pb(3, 4)), 256);
    EQ(stream_grid(256, 100, tail_pb(3, 4)), 2);
    EQ(tail_pb(3, 4), 64);   // 256 threads / 4 points; 3 x 3 x 64 x 36 B of staging
    EQ(tail_pb(8, 4), 32);   // 8 x 3 x 32 x 36 B = 27 KB; 64 would pass TAIL_FBYTES
    EQ(tail_pb(8, 16), 16);  // 256 threads / 16 points
    // a device too small for the slice: 8 CUs hold 2^11 entries
    EQ(plan(20, 3, 4, true, switches(), 8).j0, 9);
    EQ(tail_grid_cap(2, 256, switches({{"QG_SC_TAIL_BPC", "4"}})), 256);  // occupancy - 1
    EQ(tail_grid_cap(4, 256, switches({{"QG_SC_TAIL_BPC", "2"}})), 512);
    EQ(tail_grid_cap(1, 256, switches()), 256);
    row("tail_geometry");
  }
  {  // sharded: the gather round js = min(nvars + 1 - gather_log, m)
    const ScSwitches sw = switches();
    EQ(sc_gather_round(17, 1, sw), 2);
    EQ(sc_gather_round(20, 3, sw), 5);
    EQ(sc_gather_round(12, 2, sw), 0);
    EQ(sc_gather_round(12, 2, switches({{"QG_SC_PERS_LOG", "6"}})), 7);
    EQ(sc_gather_round(12, 1, switches({{"QG_SC_PERS_LOG", "6"}})), 7);
    EQ(sc_gather_round(20, 3, switches({{"QG_SC_PERS_LOG", "30"}})), 5);  // never above SC_GATHER_LOG
    row("sharded_gather_round");
    EQ(sc_gather_round(8, 2, switches({{"QG_SC_PERS_LOG", "2"}})), 6);  // js = m: one local pair left
    EQ(sc_gather_round(34, 16, sw), 18);                                 // the clamp without a switch
    row("sharded_gather_round_clamp");
  }
  {  // the buffer rule
    Elt* const base = reinterpret_cast<Elt*>(uintptr_t(1) << 40);  // addresses only
    for (uint32_t nvars = 1; nvars <= 24; nvars++) {
      const size_t N = (size_t)1 << nvars;
      // one GPU (and a rank's large rounds): X = N/2, Y = N/4 per slot, behind each other
      Bufs b = round_bufs<Elt>(1, base, base + 8 * (N / 2 + 1), N);
      for (int s = 0; s < 8; s++) b.in[s] = base - (8 - s) * N;
      EQ(b.jin, 1);
      EQ(b.capX, std::max<size_t>(1, N / 2));
      EQ(b.capY, std::max<size_t>(1, N / 4));
      EQ(b.src(0, 7) == b.in[7], 1);
      check_bufs(b, 0, nvars);  // every first tail round reads the same rule
      // sharded over 2 and 8 ranks: the tail from every gather round js
      for (uint32_t lw = 1; lw <= 3 && lw < nvars; lw += 2)
        for (uint32_t js = 0; js <= nvars - lw; js++) {
          const size_t GN = (size_t)1 << (nvars - std::max(js, 1u) + 1);  // gathered table
          Bufs g = round_bufs<Elt>(std::max(js, 1u), base, base + 8 * (GN / 2 + 1), GN);
          for (int s = 0; s < 8; s++) g.in[s] = base - (8 - s) * GN;
          EQ(g.dst(g.jin, 0) == base, 1);  // the first fold goes to the larger buffer
          check_bufs(g, js, nvars);
        }
    }
    row("buffer_rule");
  }
  {  // the io region
    for (uint32_t nvars : {1u, 20u, 40u})
      for (uint32_t width : {1u, 4u, 16u}) {
        const ScIo o = sc_io(nvars, width);
        EQ(o.bar, sizeof(ScState));
        EQ(sizeof(ScState), 192);
        EQ(o.bar8 >= o.bar + 4 * (nvars + 2), 1);
        EQ(o.bar8 % 128, 0);
        EQ(o.acc0, o.bar8 + 8 * 128);
        EQ(o.acc0 % 128, 0);
        EQ(o.chal, o.acc0 + SC_BACC_BYTES);
        EQ(o.coeffs, o.chal + 32 * (size_t)nvars);
        EQ(o.fin, o.coeffs + 32 * (size_t)nvars * width);
        EQ(o.lens, o.fin + 32 * 9);
        EQ(o.bytes, o.lens + 4 * (size_t)nvars);
        EQ(o.bytes, parent_io_bytes(nvars, width));
      }
    EQ(sc_io(1, 4).bytes, 10948);
    EQ(SC_BACC_BYTES, 9216);
    row("io_layout");
  }
  {  // the parser: defaults, range ends, bad values
    const ScSwitches d = switches();
    EQ(d.pers_log, 16);
    EQ(d.big_blocks, 0);
    EQ(d.round_blocks, 0);
    EQ(d.staged || d.no_skip0 || d.old_tail || d.wpe4, 0);
    EQ(d.tail_bpc, 1);
    const ScSwitches s = switches({{"QG_SC_PERS_LOG", "30"}, {"QG_SC_BIG_BLOCKS", "2048"},
                                   {"QG_SC_BLOCKS", "1"}, {"QG_SC_STAGED", ""},
                                   {"QG_SC_NO_SKIP0", "0"}, {"QG_SC_OLD_TAIL", "2"},
                                   {"QG_SC_WPE", "4"}, {"QG_SC_TAIL_BPC", "3"}});
    EQ(s.pers_log, 30);
    EQ(s.big_blocks, 2048);
    EQ(s.round_blocks, 1);
    EQ(s.staged && s.no_skip0 && s.old_tail && s.wpe4, 1);  // set is set, whatever the value
    EQ(s.tail_bpc, 3);
    EQ(switches({{"QG_SC_PERS_LOG", "1"}}).pers_log, 1);
    for (const char* v : {"0", "31", "-3", "six", "6x", "", "6.5"})
      EQ(switch_error({{"QG_SC_PERS_LOG", v}}), QG_ERR_INVALID);
    for (const char* v : {"0", "2049", "many"})
      EQ(switch_error({{"QG_SC_BIG_BLOCKS", v}}), QG_ERR_INVALID);
    for (const char* v : {"0", "2049", "99999999999999999999"})
      EQ(switch_error({{"QG_SC_BLOCKS", v}}), QG_ERR_INVALID);
    // the three moved in keep their lenient reading
    EQ(switches({{"QG_SC_OLD_TAIL", "off"}}).old_tail, 0);  // atoi: not a number is 0
    EQ(switches({{"QG_SC_OLD_TAIL", "-1"}}).old_tail, 1);
    EQ(switches({{"QG_SC_TAIL_BPC", "0"}}).tail_bpc, 1);
    EQ(switches({{"QG_SC_TAIL_BPC", "-7"}}).tail_bpc, 1);
    EQ(switches({{"QG_SC_TAIL_BPC", "x"}}).tail_bpc, 1);
    EQ(switches({{"QG_SC_WPE", ""}}).wpe4, 1);
    row("switch_parser");
  }
  switches();
  return fails ? 1 : 0;
}
