// The host-side decisions of the compiled sumcheck prover (sumcheck.hip): the
// tuning switches, which kernel runs which round on which grid, where the tail
// takes over, which buffer a round reads and writes, and the layout of the io
// region.  Plain integers and small structs - no HIP - so
// tests/cpp/sumcheck_plan_check.cpp pins them on the CPU.  The few functions
// the kernels call as well carry the device qualifier under hipcc only.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../include/quill_gpu.h"
#include "error.h"

#ifdef __HIPCC__
#define SC_PLAN_HD __host__ __device__ __forceinline__
#else
#define SC_PLAN_HD inline
#endif

namespace qg {

static constexpr int SC_BLOCK = 256;
// Most blocks of a large round.  Every block adds one sum (< 2p) per point to
// the round's limb accumulator, and limbsum29 holds for fewer than 2720
// summands: the cap keeps a round within it.
static constexpr int SC_MAX_BLOCKS = 2048;
static constexpr int PERS_LOG = 16;  // tables of <= 2^16 entries: the rounds run in one persistent launch
// sharded: the ranks gather their blocks once the folded tables' global size
// is at most 2^SC_GATHER_LOG (never above 2^pers_log)
static constexpr uint32_t SC_GATHER_LOG = 16;

// ---------------------------------------------------------------- switches
// The QG_SC_* tuning switches, read once per proof (tests and A/B runs toggle
// them in-process).  A number must be whole and within its range: anything
// else is QG_ERR_INVALID, never a silent default.
struct ScSwitches {
  int pers_log;      // QG_SC_PERS_LOG: where the persistent tail takes over (default PERS_LOG)
  int big_blocks;    // QG_SC_BIG_BLOCKS: grid cap of k_sc_big (0: 2 per CU)
  int round_blocks;  // QG_SC_BLOCKS: grid cap of k_sc_round (0: 3 per CU)
  bool staged;       // QG_SC_STAGED set: k_sc_round runs every large round (A/B runs)
  bool no_skip0;     // QG_SC_NO_SKIP0 set: t = 0 is evaluated in every round (A/B runs)
  bool old_tail;     // QG_SC_OLD_TAIL non-zero: the streaming k_sc_tail, never k_sc_slice (A/B runs)
  bool wpe4;         // QG_SC_WPE set: the product sweep compiled for 4 waves per SIMD (tuning)
  int tail_bpc;      // QG_SC_TAIL_BPC: blocks per CU of a tail's grid cap (default 1; below 1 counts as 1)
};
inline int sc_env_int(const char* name, long lo, long hi, int unset) {
  const char* e = getenv(name);
  if (!e) return unset;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(e, &end, 10);
  QG_CHECK(end != e && *end == '\0' && errno == 0 && v >= lo && v <= hi, QG_ERR_INVALID,
           std::string(name) + " must be a whole number in [" + std::to_string(lo) + ", " +
               std::to_string(hi) + "]");
  return (int)v;
}
inline ScSwitches sc_switches() {
  ScSwitches s;
  s.pers_log = sc_env_int("QG_SC_PERS_LOG", 1, 30, PERS_LOG);
  s.big_blocks = sc_env_int("QG_SC_BIG_BLOCKS", 1, SC_MAX_BLOCKS, 0);
  s.round_blocks = sc_env_int("QG_SC_BLOCKS", 1, SC_MAX_BLOCKS, 0);
  s.staged = getenv("QG_SC_STAGED") != nullptr;
  s.no_skip0 = getenv("QG_SC_NO_SKIP0") != nullptr;
  const char* ot = getenv("QG_SC_OLD_TAIL");
  s.old_tail = ot && atoi(ot) != 0;
  s.wpe4 = getenv("QG_SC_WPE") != nullptr;
  const char* bpc = getenv("QG_SC_TAIL_BPC");
  s.tail_bpc = bpc ? std::max(1, atoi(bpc)) : 1;
  return s;
}

// ---------------------------------------------------------------- dispatch
// the template instance <K,NP> of a proof: slots and points rounded up
struct ScInstance {
  int K, NP;
};
inline ScInstance sc_instance(uint32_t nslots, uint32_t np) {
  if (np <= 4) return {nslots <= 4 ? 4 : 8, 4};
  if (np <= 8) return {nslots <= 4 ? 4 : 8, 8};
  return {8, 16};
}

// The kernel of the large rounds: the thread-per-pair k_sc_big<K,4,true> for a
// product of distinct tables (SOP_PURE), k_sc_big<4,4,false> for any other
// expression of <= 4 slots at degree <= 3, the LDS-staged k_sc_round<K,NP> for
// the rest and under QG_SC_STAGED.
enum class ScBig { pure, sop, staged };
inline ScBig sc_big_form(ScInstance in, bool pure, const ScSwitches& sw) {
  if (sw.staged || in.NP > 4 || (!pure && in.K > 4)) return ScBig::staged;
  return pure ? ScBig::pure : ScBig::sop;
}
// Rounds j >= 1 of k_sc_big: h(0) = h_{j-1}(r_{j-1}) - h(1), exact by
// construction (the folded table's pair sums ARE the previous message at r);
// round 0 evaluates every point, so a wrong caller claim still yields the
// reference's bytes.  The staged kernel evaluates every point.
inline bool sc_skip0(ScBig form, uint32_t np, uint32_t j, const ScSwitches& sw) {
  return form != ScBig::staged && j >= 1 && np >= 2 && !sw.no_skip0;
}
// Blocks of a large round: k_sc_big 2 per CU (measured best: 256 / 512 / 2048
// blocks at 2^20: 0.289 / 0.264 / 0.333 ms), k_sc_round ~3 resident blocks per
// CU, each striding over many pair groups (2^20: 768 blocks 0.764 ms vs 2048
// blocks 0.798 ms); QG_SC_BIG_BLOCKS / QG_SC_BLOCKS override.
inline unsigned sc_round_grid(ScBig form, size_t cus, size_t npairs, const ScSwitches& sw) {
  const int ov = form == ScBig::staged ? sw.round_blocks : sw.big_blocks;
  size_t cap = ov > 0 ? (size_t)ov : (form == ScBig::staged ? 3 : 2) * cus;
  cap = std::min<size_t>(cap, SC_MAX_BLOCKS);
  return (unsigned)std::max<size_t>(1, std::min<size_t>(cap, (npairs + SC_BLOCK - 1) / SC_BLOCK));
}

// ---------------------------------------------------------------- tail geometry
static constexpr int TAIL_BLOCK = 256;
static constexpr uint32_t TAIL_FBYTES = 32 * 1024;  // LDS for k_sc_tail's staging arrays
// pairs per block step of k_sc_tail.  np: the kernel's point stride NP
// (threads per pair), not the expression's np
SC_PLAN_HD uint32_t tail_pb(uint32_t nslots, uint32_t np) {
  // F0: nslots x 2 PB entries, F1: nslots x PB entries, 36 B each
  const uint32_t per = nslots ? nslots * 108u : 108u;
  uint32_t pb = 1;
  while (pb * 2 * per <= TAIL_FBYTES && pb * 2 * np <= (uint32_t)TAIL_BLOCK) pb *= 2;
  return pb;
}
// entries per slot of a block's slice in the first round of k_sc_slice (LDS: K
// slots x 1.5 x SL_SMAX entries of 36 B: the slice and its half-size fold)
SC_PLAN_HD constexpr uint32_t sl_smax(int K) { return K <= 4 ? 256u : 128u; }

// Most co-resident blocks of a tail launch (grid barrier): bpc blocks per CU
// (QG_SC_TAIL_BPC), never more than the occupancy answer minus one: a spare
// block slot per CU keeps the barrier safe next to other kernels' blocks and
// under the gfx950 SGPR admission rule (MI355X_MICROARCH.md "Residency").
inline size_t tail_grid_cap(int occ, size_t cus, const ScSwitches& sw) {
  const int bpc = std::max(1, std::min(sw.tail_bpc, occ - 1));
  return std::max<size_t>(1, cus * (size_t)bpc);
}
// The slice tail: G blocks, a power of two <= min(cap, SMAX) so block 0 can
// gather one entry per block, each owning <= SMAX entries per slot.
// 0: QG_SC_OLD_TAIL keeps the streaming tail.
inline size_t slice_gmax(int K, size_t cap, const ScSwitches& sw) {
  if (sw.old_tail) return 0;
  const size_t gm = std::min<size_t>(cap, sl_smax(K));
  size_t G = 1;
  while (G * 2 <= gm) G *= 2;
  return G;
}
// log2 of the largest round table (entries per slot) the slice tail can start from; 0: none
inline uint32_t slice_tail_log(int K, size_t gmax) {
  if (!gmax) return 0;
  uint32_t l = 0;
  while (((size_t)1 << (l + 1)) <= gmax * sl_smax(K)) l++;
  return l;
}
// blocks of a slice tail over a first table of n0 entries per slot; 0: a
// block's slice would not fit (the streaming tail runs)
inline size_t slice_grid(int K, size_t gmax, size_t n0) {
  if (!gmax) return 0;
  size_t G = 1;
  while (G * 2 <= gmax && G * 2 <= n0 / 2) G *= 2;
  return n0 / G > sl_smax(K) ? 0 : G;
}
// blocks of a streaming tail whose first round has pairs0 pairs
inline unsigned stream_grid(size_t cap, size_t pairs0, uint32_t pb) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>(cap, (pairs0 + pb - 1) / pb));
}

// ---------------------------------------------------------------- first tail round
// one GPU: the first round whose table (2^(nvars - j) entries) fits both the
// switch and what the slice tail holds (slice_log; 0: no slice tail)
inline uint32_t sc_first_tail_round(uint32_t nvars, const ScSwitches& sw, uint32_t slice_log) {
  const uint32_t plog = slice_log ? std::min<uint32_t>(sw.pers_log, slice_log) : sw.pers_log;
  uint32_t j = 0;
  while (j < nvars && nvars - j > plog) j++;
  return j;
}
// sharded over 2^lw ranks: the large rounds 0..js-1 pair local entries; round
// js's source tables (folded through r_{js-2}, global size 2^(nvars - js + 1))
// fit the gather size; at most m = nvars - lw (local tables of 2 entries)
inline uint32_t sc_gather_round(uint32_t nvars, uint32_t lw, const ScSwitches& sw) {
  const uint32_t gl = std::min<uint32_t>(SC_GATHER_LOG, sw.pers_log);
  const uint32_t js = nvars + 1 > gl ? nvars + 1 - gl : 0;
  return std::min(js, nvars - lw);
}

// ---------------------------------------------------------------- buffers
// Where round j reads and writes.  Round 0 evaluates the input tables as they
// are; round j >= 1 folds round j - 1's table by r_{j-1} and evaluates the
// result.  The fold of round j <= jin reads the inputs, every later one the
// previous round's destination; destinations alternate X (j odd) and Y (j
// even).  One GPU and the sharded large rounds: jin = 1, X holds N/2 entries
// per slot and Y N/4.  The sharded tail from round js on: the inputs are the
// gathered tables and jin = max(js, 1).
template <class T>
struct RoundBufsT {
  const T* in[8];
  T* X;
  T* Y;
  size_t capX, capY;  // entries per slot
  uint32_t jin;
  SC_PLAN_HD const T* src(uint32_t j, uint32_t s) const { return j <= jin ? in[s] : dst(j - 1, s); }
  SC_PLAN_HD T* dst(uint32_t j, uint32_t s) const { return (j & 1) ? X + capX * s : Y + capY * s; }
};
// big (>= n / 2 per slot) and small (>= n / 4) hold the folds of the n-entry
// inputs of round jin: big becomes the buffer round jin writes
template <class T>
inline RoundBufsT<T> round_bufs(uint32_t jin, T* big, T* small, size_t n) {
  RoundBufsT<T> b{};
  const size_t cb = std::max<size_t>(1, n / 2), cs = std::max<size_t>(1, n / 4);
  b.jin = jin;
  b.X = (jin & 1) ? big : small;
  b.Y = (jin & 1) ? small : big;
  b.capX = (jin & 1) ? cb : cs;
  b.capY = (jin & 1) ? cs : cb;
  return b;
}

// ---------------------------------------------------------------- io region
// Round bookkeeping.  The transcript state, the deferred absorb, the current
// challenge in 29-bit form and the last-block election counter live in one
// small device struct.
struct ScState {
  uint32_t state[8];  // absorbed transcript state
  uint32_t pend[20];  // state' || 48 challenge bytes of the last round, not yet absorbed
  uint32_t ticket;    // accumulator shards of the current round that are complete
  uint32_t err;       // persistent-kernel barrier timeout flag
  uint32_t r29[9];    // last challenge * 2^261 mod p (< 2p), the fold multiplier
  uint32_t pad[1];
  uint32_t claim[8];  // this round's claim h_{j-1}(r_{j-1}) at scale S (big rounds, j >= 1)
};
// limb accumulators of the large rounds: [shard 8][16 points][9 limbs] u64.
// Slot 0 (even rounds) lies in the io region and is zeroed per call, slot 1
// (odd rounds) in scratch; each round's last block clears the next round's.
static constexpr size_t SC_BACC_BYTES = 8 * 16 * 9 * sizeof(uint64_t);
static constexpr size_t SC_FR_BYTES = 32;

// One device region per proof, byte offsets in order: ScState | per-round
// barrier counters (nvars + 2) | 8 barrier shards, one 128-B line each |
// accumulator slot 0 | challenges (nvars) | coefficient rows (nvars x width) |
// final values (8 slots + the evaluation) | lens (nvars).  Everything before
// the challenges is (re)initialised by the per-call header copy.
struct ScIo {
  size_t bar, bar8, acc0, chal, coeffs, fin, lens, bytes;
};
inline ScIo sc_io(uint32_t nvars, uint32_t width) {
  ScIo o;
  o.bar = sizeof(ScState);
  o.bar8 = (o.bar + sizeof(uint32_t) * (nvars + 2) + 127) & ~(size_t)127;
  o.acc0 = o.bar8 + 8 * 128;
  o.chal = o.acc0 + SC_BACC_BYTES;
  o.coeffs = o.chal + SC_FR_BYTES * nvars;
  o.fin = o.coeffs + SC_FR_BYTES * (size_t)nvars * width;
  o.lens = o.fin + SC_FR_BYTES * 9;
  o.bytes = o.lens + sizeof(uint32_t) * nvars;
  return o;
}

}  // namespace qg
