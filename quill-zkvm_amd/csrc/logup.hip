// Logup log-derivative columns for gfx950 — replaces the per-row loops of
//   MultisetEqualityProof::prove  hyperplonk/src/piops/multiset_check.rs:43-95
//   SetInclusionProof::prove      hyperplonk/src/piops/set_inclusion.rs:93-131
// which evaluate h(x) through the expression tree for every row x, call
// (beta + h(x)).inverse().unwrap() 2^n times, and multiply by m(x) in subset
// mode.  Here: out[x] = m(x) / (beta + h(x)) with ONE field inversion per
// column, in three kernels around it (the only path).
//
//  * Both expressions are compiled on the host into sums of monomials
//    (expr.h).  The coefficient of a monomial with f factors is pre-scaled by
//    2^(256 + 5f), so multiplying raw arkworks table entries (x 2^256) with
//    mul29 (x 2^-261) keeps both the denominator and the multiplier in
//    arkworks form; a coefficient that comes out as 2^261 (a bare table
//    entry) skips its multiply.
//  * Batch inversion (Montgomery's trick) at four levels: phase 1
//    (k_logup_den) stores every row's beta + h(x) in the output buffer and
//    multiplies each block's rows together; phase 2 (k_logup_scan, one block)
//    forms the exclusive prefix / suffix products of the block products and
//    their total, which the host inverts (binary GCD, bingcd.h; on the
//    device's scalar unit it took 50 us, more than the round trip); phase 3
//    (k_logup) gives each block 1/(its product) = 1/total x prefix x suffix,
//    then within the block: each thread's running prefix of its LG_K rows in
//    registers (row values in LDS), wave shuffle scans of the thread products,
//    back-substitution.  96 B/row of tables read and 32 B/row written, plus
//    the denominators' round trip through the output buffer (+64 B/row); the
//    column is VALU-bound, not HBM-bound.
//  * Domains: the denominators stay in arkworks' x 2^256 form (the raw table
//    entries add in without a conversion multiply; beta + t0 + a t1 costs one
//    multiply).  Every mul29 takes 2^261 off, so a product of j such values
//    carries 2^(261 - 5j): with N rows the column total the host receives is
//    tot = (prod v) 2^(261 - 5N) as a plain integer.  Each 1 / v_k of k_logup
//    is a product tree over tinv and the column's other N - 1 rows, whatever
//    its position, so ONE constant fixes every output: tinv = tot^-1 2^517
//    gives every 1 / v_k as (1 / v_k) 2^261, and the multiplier's x 2^256
//    domain then gives the output in arkworks form.  (A padding row is 2^261,
//    mul29's identity: it is not one of the N.)
//  * A zero denominator makes the block product zero: the kernel flags it and
//    the call returns QG_ERR_ASSERT (the reference panics in unwrap()).
//  * Per-block sums of the outputs feed SetInclusionProof's claimed sums
//    (set_inclusion.rs:162-166, 193-197) without a second pass.
//  * k_expr_column (qg_expr_column[_dev]) evaluates one compiled expression per
//    row into a column of canonical words: a lookup column that is not a plain
//    input (lookup.rs:51-59) is materialised by it before the multiplicities
//    are counted (lookup.hip compares 32-byte words).
#include <string.h>

#include <vector>

#include "bingcd.h"
#include "common.h"
#include "expr.h"
#include "field29.h"

using namespace qg;

namespace qg {

using R29 = F29<FrP>;

static constexpr int LG_BLOCK = 256;
static constexpr int LG_K = 8;                     // rows per thread
static constexpr int LG_ROWS = LG_BLOCK * LG_K;    // rows per block
static constexpr int LG_MAXM = 128;                // monomials per expression
static constexpr int LG_MAXF = 512;                // factor slots (both expressions)
static constexpr int LG_MAXT = 64;                 // distinct tables referenced

// device image of the two compiled expressions: [0] = beta + h, [1] = m
struct LgDev {
  uint32_t nm[2];
  uint32_t unit[2][LG_MAXM];  // coefficient is 2^261 (mul29 by it is the identity)
  uint32_t mlen[2][LG_MAXM];
  uint32_t fstart[2][LG_MAXM];
  L9 coef[2][LG_MAXM];
  uint32_t fac[LG_MAXF];
  const Fr* tab[LG_MAXT];
};

// the scratch slot "lg_io": one call's image and its small result words
struct LgIo {
  LgDev img;
  Fr res;                    // k_logup_sum: the column sum
  uint32_t err;              // k_logup_den: some denominator was zero
  unsigned long long first;  // k_expr_first_nonzero
};

// one expression at one row; < 2p, normalized
QG_DEV R29 lg_eval(const LgDev* __restrict__ g, int w, size_t row) {
  R29 acc = R29::zero();
  const uint32_t nm = g->nm[w];
  for (uint32_t m = 0; m < nm; m++) {
    const uint32_t len = g->mlen[w][m], fs = g->fstart[w][m];
    uint32_t j = 0;
    R29 t;
    if (g->unit[w][m]) {  // c 2^(256 + 5f) = 2^261: the first factor as loaded (< p)
      t = to29(g->tab[g->fac[fs]][row]);
      j = 1;
    } else {
      t = R29::from_l9(g->coef[w][m]);
    }
    for (; j < len; j++) t = mul29(t, to29(g->tab[g->fac[fs + j]][row]));
    acc = red2p29(add29(acc, t));
  }
  return acc;
}

// ---- block primitives: 256 threads = LG_WAVES waves -------------------------
static constexpr int LG_WAVES = LG_BLOCK / 64;

// nine limbs to / from one LDS row (a wave's total or partial sum)
QG_DEV R29 lds_get9(const uint32_t* row) {
  R29 v;
#pragma unroll
  for (int i = 0; i < 9; i++) v.l[i] = row[i];
  return v;
}
QG_DEV void lds_put9(uint32_t* row, const R29& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) row[i] = v.l[i];
}
// the same in the [k][limb][thread] layout of a block's LG_K x LG_BLOCK rows
QG_DEV R29 lds_row(const uint32_t* vs, int k, int tid) {
  R29 v;
#pragma unroll
  for (int i = 0; i < 9; i++) v.l[i] = vs[(k * 9 + i) * LG_BLOCK + tid];
  return v;
}
QG_DEV void lds_put(uint32_t* vs, int k, int tid, const R29& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) vs[(k * 9 + i) * LG_BLOCK + tid] = v.l[i];
}

// Sum over the block of one value < 2p per thread: a wave xor-tree, then the
// LG_WAVES wave partials through LDS.  Thread 0 returns the sum (< 2p).
QG_DEV R29 block_sum29(R29 acc, uint32_t (*wsum)[9]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int d = 32; d >= 1; d >>= 1) acc = red2p29(add29(acc, shfl_xor29(acc, d)));
  if (lane == 0) lds_put9(wsum[wv], acc);
  __syncthreads();
  R29 s = R29::zero();
  if (tid == 0)
#pragma unroll
    for (int w = 0; w < LG_WAVES; w++) s = red2p29(add29(s, lds_get9(wsum[w])));
  return s;
}

// Exclusive prefix (ep) and suffix (es) products over the block of one value T
// per thread: inclusive wave shuffle scans in both directions, then the fix-up
// from the wave totals, which stay in wtot.  PAIR: the two scans' products as
// one interleaved pair (field29.h mul29tn), which is k_logup's form, instead
// of two mul29; the same arithmetic.  k_logup_scan, a single block at one wave
// per SIMD, is slower with the pair (40.6 against 31.2 us at 2^22 rows,
// profiles/r13_logup_one_path.txt), so each kernel keeps the form it had.
// tot given: thread 0 multiplies the wave totals into it as well, in the
// fix-up loop (a loop of its own after it the compiler moves to the scalar
// unit, which is several times slower at these products).
template <bool PAIR>
QG_DEV void block_scan_prod29(const R29& T, uint32_t (*wtot)[9], R29& ep, R29& es,
                              R29* tot = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const R29 one = R29::from_l9(F29P<FrP>::ONE);
  R29 ip = T, is = T;  // inclusive in-wave prefix / suffix
  for (int d = 1; d < 64; d <<= 1) {
    R29 x2[2] = {shfl_up29(ip, d), is}, y2[2] = {ip, shfl_down29(is, d)};
    if constexpr (PAIR) {
      mul29tn<FrP, 2>(x2, y2, x2);
    } else {
      x2[0] = mul29(x2[0], y2[0]);
      x2[1] = mul29(x2[1], y2[1]);
    }
    if (lane >= d) ip = x2[0];
    if (lane + d < 64) is = x2[1];
  }
  if (lane == 63) lds_put9(wtot[wv], ip);
  ep = shfl_up29(ip, 1);
  es = shfl_down29(is, 1);
  if (lane == 0) ep = one;
  if (lane == 63) es = one;
  __syncthreads();
  for (int w = 0; w < LG_WAVES; w++) {  // wave products straight from LDS (uniform loop)
    const R29 t = lds_get9(wtot[w]);
    if (w < wv) ep = mul29(ep, t);
    if (w > wv) es = mul29(es, t);
    if (tot && tid == 0) *tot = mul29(*tot, t);
  }
}

// Phase 1: per row v = beta + h(row) (x 2^256), stored (< p) into the output
// buffer; the block's product of all its rows -> bprod[block].  A zero
// denominator makes the product zero (flagged).  128 threads x 16 rows per
// 2048-row block: 4096 waves at 2^22 rows, all resident in one round (256
// threads x 8 rows was 8192 waves for 6144 slots at 77 VGPRs: 1.33 rounds).
static constexpr int LG_DEN_BLOCK = 128;
static constexpr int LG_DEN_K = LG_ROWS / LG_DEN_BLOCK;
__global__ __launch_bounds__(LG_DEN_BLOCK) void k_logup_den(const LgDev* __restrict__ g, size_t n,
                                                            Fr* __restrict__ out,
                                                            Fr* __restrict__ bprod,
                                                            uint32_t* __restrict__ err) {
  __shared__ uint32_t wtot[LG_DEN_BLOCK / 64][9];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t base = (size_t)blockIdx.x * LG_ROWS + tid;
  const R29 one = R29::from_l9(F29P<FrP>::ONE);
  R29 T = one;
  bool zero = false;
  for (int k = 0; k < LG_DEN_K; k++) {
    const size_t row = base + (size_t)k * LG_DEN_BLOCK;
    if (row >= n) break;
    const R29 v = canon29(lg_eval(g, 0, row));
    zero |= is_zero29(v);
    out[row] = from29(v);
    T = mul29(T, v);
  }
  if (zero) atomicOr(err, 1u);
  for (int d = 32; d >= 1; d >>= 1) {
    const R29 o = shfl_down29(T, d);
    if (lane + d < 64) T = mul29(T, o);
  }
  if (lane == 0) lds_put9(wtot[wv], T);
  __syncthreads();
  if (tid == 0) {
    R29 p = one;
    for (int w = 0; w < LG_DEN_BLOCK / 64; w++) p = mul29(p, lds_get9(wtot[w]));
    bprod[blockIdx.x] = from29(canon29(p));
  }
}

// Phase 2 (one block): exclusive prefix and suffix products of the nb block
// products, and their total (the single value the host inverts).  256 threads,
// one contiguous segment each (sequential products), wave shuffle scans of the
// segment products and the four wave totals: ~20 dependent products per
// thread at one wave per SIMD (a 1024-thread Hillis-Steele scan through LDS
// took 49 us at 2^22 rows).
__global__ __launch_bounds__(LG_BLOCK) void k_logup_scan(const Fr* __restrict__ bprod, uint32_t nb,
                                                         Fr* __restrict__ pre, Fr* __restrict__ suf,
                                                         Fr* __restrict__ total) {
  __shared__ uint32_t wtot[LG_WAVES][9];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (nb + LG_BLOCK - 1) / LG_BLOCK;
  const uint32_t lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
  const R29 one = R29::from_l9(F29P<FrP>::ONE);
  R29 tp = one;  // product of this thread's segment
  for (uint32_t i = lo; i < hi; i++) tp = mul29(tp, to29(bprod[i]));
  R29 rp, rs, tot = one;
  block_scan_prod29<false>(tp, wtot, rp, rs, &tot);
  if (tid == 0) *total = from29(canon29(tot));
  for (uint32_t k = 0; k < hi - lo; k++) {  // prefix up, suffix down, interleaved
    const uint32_t i = lo + k, j = hi - 1 - k;
    pre[i] = from29(canon29(rp));
    suf[j] = from29(canon29(rs));
    rp = mul29(rp, to29(bprod[i]));
    rs = mul29(rs, to29(bprod[j]));
  }
}

// Phase 3: 1/v for every row of the block from inv(total) x prefix x suffix of
// the block products (block inverse), then the thread-level Montgomery trick;
// the rows' v values come back from the output buffer.
__global__ __launch_bounds__(LG_BLOCK) void k_logup(const LgDev* __restrict__ g, size_t n,
                                                    Fr* __restrict__ out,
                                                    const Fr* __restrict__ pre,
                                                    const Fr* __restrict__ suf,
                                                    const Fr* __restrict__ tinv,
                                                    Fr* __restrict__ bsum) {
  __shared__ uint32_t vs[LG_K * 9 * LG_BLOCK];  // row denominators, [k][limb][thread]
  __shared__ uint32_t wtot[LG_WAVES][9];
  __shared__ uint32_t wsum[LG_WAVES][9];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * LG_ROWS + tid;

  // 1. denominators back from HBM to LDS (a padding row is mul29's identity),
  // then the running prefix of this thread's rows
  for (int k = 0; k < LG_K; k++) {
    const size_t row = base + (size_t)k * LG_BLOCK;
    lds_put(vs, k, tid, row < n ? to29(out[row]) : R29::from_l9(F29P<FrP>::ONE));
  }
  static_assert(LG_K == 8, "prefix chain is written out for 8 rows");
  R29 pre_r[LG_K];
  pre_r[0] = lds_row(vs, 0, tid);
  pre_r[1] = mul29(pre_r[0], lds_row(vs, 1, tid));
  pre_r[2] = mul29(pre_r[1], lds_row(vs, 2, tid));
  pre_r[3] = mul29(pre_r[2], lds_row(vs, 3, tid));
  pre_r[4] = mul29(pre_r[3], lds_row(vs, 4, tid));
  pre_r[5] = mul29(pre_r[4], lds_row(vs, 5, tid));
  pre_r[6] = mul29(pre_r[5], lds_row(vs, 6, tid));
  pre_r[7] = mul29(pre_r[6], lds_row(vs, 7, tid));

  // 2. exclusive prefix / suffix products of the thread products across the block
  R29 ep, es;
  block_scan_prod29<true>(pre_r[LG_K - 1], wtot, ep, es);
  // 1 / (block product) = 1 / total x (other blocks' products)
  const R29 binv = mul29(mul29(to29(*tinv), to29(pre[blockIdx.x])), to29(suf[blockIdx.x]));
  R29 inv_run = mul29(mul29(binv, ep), es);  // 1 / (this thread's product)

  // 3. back-substitution: 1 / v_k overwrites v_k in LDS (own slots only);
  // the output product and the next running inverse as one interleaved pair
#define LG_BACK(k)                                                      \
  {                                                                     \
    R29 a2[2] = {inv_run, inv_run}, b2[2] = {pre_r[k - 1], lds_row(vs, k, tid)}; \
    mul29tn<FrP, 2>(a2, b2, a2);                                        \
    inv_run = a2[1];                                                    \
    lds_put(vs, k, tid, a2[0]);                                         \
  }
  LG_BACK(7) LG_BACK(6) LG_BACK(5) LG_BACK(4) LG_BACK(3) LG_BACK(2) LG_BACK(1)
#undef LG_BACK
  lds_put(vs, 0, tid, inv_run);

  // 4. multiplier (four rows' products interleaved), store, block sum
  R29 acc = R29::zero();
  for (int k0 = 0; k0 < LG_K; k0 += 4) {
    R29 xs[4], ms[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const size_t row = base + (size_t)(k0 + u) * LG_BLOCK;
      xs[u] = lds_row(vs, k0 + u, tid);
      ms[u] = row < n ? lg_eval(g, 1, row) : R29::zero();  // M x 2^256
    }
    mul29tn<FrP, 4>(xs, ms, xs);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const size_t row = base + (size_t)(k0 + u) * LG_BLOCK;
      if (row >= n) break;
      const R29 y = canon29(xs[u]);
      out[row] = from29(y);
      acc = red2p29(add29(acc, y));
    }
  }
  const R29 s = block_sum29(acc, wsum);
  if (tid == 0) bsum[blockIdx.x] = from29(canon29(s));
}

// sum of the per-block sums (one block)
__global__ __launch_bounds__(LG_BLOCK) void k_logup_sum(const Fr* __restrict__ bsum, uint32_t nb,
                                                        Fr* __restrict__ res) {
  __shared__ uint32_t wsum[LG_WAVES][9];
  R29 acc = R29::zero();
  for (uint32_t i = threadIdx.x; i < nb; i += LG_BLOCK) acc = red2p29(add29(acc, to29(bsum[i])));
  const R29 s = block_sum29(acc, wsum);
  if (threadIdx.x == 0) *res = from29(canon29(s));
}

// first row whose expression value (slot 0, no beta) is nonzero; atomicMin
__global__ __launch_bounds__(256) void k_expr_first_nonzero(const LgDev* __restrict__ g, size_t n,
                                                            unsigned long long* first) {
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const R29 v = canon29(lg_eval(g, 0, row));
  if (!is_zero29(v)) atomicMin(first, (unsigned long long)row);
}

// out[row] = h(row) (slot 0 compiled at scale 256, so the value is in arkworks
// Montgomery form), canonical: the lookup count compares the 32-byte words.
// One table read per factor and one 32-byte write per row.
__global__ __launch_bounds__(256) void k_expr_column(const LgDev* __restrict__ g, size_t n,
                                                     Fr* __restrict__ out) {
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  out[row] = from29(canon29(lg_eval(g, 0, row)));
}

// ---------------------------------------------------------------- host
static Fr lg_plain_mul(const Fr& x, const Fr& y) { return from_mont(to_mont(x) * to_mont(y)); }
static L9 lg_l9(const Fr& plain) {
  const R29 t = to29(plain);
  L9 r{};
  for (int i = 0; i < 9; i++) r.v[i] = t.l[i];
  return r;
}

// compile one expression into slot w of the image at scale 256 + 5f (the value
// comes out in arkworks form, x 2^256); `add_const` (Montgomery) is added to
// the constant monomial when `with_const`
static void lg_compile(LgDev& d, int w, const SopProgram& sp, const Fr& add_const, bool with_const,
                       std::vector<uint32_t>& tables_used, uint32_t& nfac) {
  std::vector<uint32_t> mlen = sp.mono_len;
  std::vector<Fr> coeff = sp.coeff;
  std::vector<std::vector<uint32_t>> facs;
  size_t off = 0;
  for (size_t m = 0; m < mlen.size(); m++) {
    std::vector<uint32_t> f;
    for (uint32_t j = 0; j < mlen[m]; j++) f.push_back(sp.used[sp.fac[off + j]]);
    off += mlen[m];
    facs.push_back(f);
  }
  if (with_const) {
    bool found = false;
    for (size_t m = 0; m < mlen.size(); m++)
      if (mlen[m] == 0) {
        coeff[m] = coeff[m] + add_const;
        found = true;
      }
    if (!found) {
      mlen.push_back(0);
      coeff.push_back(add_const);
      facs.push_back({});
    }
  }
  QG_CHECK(mlen.size() <= (size_t)LG_MAXM, QG_ERR_UNSUPPORTED, "logup expression has too many monomials");
  d.nm[w] = (uint32_t)mlen.size();
  for (size_t m = 0; m < mlen.size(); m++) {
    d.mlen[w][m] = mlen[m];
    d.fstart[w][m] = nfac;
    for (uint32_t t : facs[m]) {
      QG_CHECK(nfac < (uint32_t)LG_MAXF, QG_ERR_UNSUPPORTED, "logup expressions have too many factors");
      uint32_t slot = 0;
      while (slot < tables_used.size() && tables_used[slot] != t) slot++;
      if (slot == tables_used.size()) {
        QG_CHECK(slot < (uint32_t)LG_MAXT, QG_ERR_UNSUPPORTED, "logup expressions use too many tables");
        tables_used.push_back(t);
      }
      d.fac[nfac++] = slot;
    }
    const Fr cf = lg_plain_mul(from_mont(coeff[m]), pow2_mod_plain<FrP>(256 + 5 * mlen[m]));
    d.coef[w][m] = lg_l9(cf);
    d.unit[w][m] = mlen[m] >= 1 && cf == pow2_mod_plain<FrP>(261) ? 1u : 0u;
  }
}

// an expression as the C-ABI passes it; empty: none given
struct LgExpr {
  const qg_expr_op* prog = nullptr;
  size_t len = 0;
  const uint64_t* consts = nullptr;
  size_t nconsts = 0;
  explicit operator bool() const { return prog && len; }
};

// The one setup of every kernel here: compile into `img` (the caller's, alive
// until the call's sync), bind the tables the expressions use, upload into the
// "lg_io" slot.  beta == nullptr: slot 0 = h alone (k_expr_column,
// k_expr_first_nonzero).  Otherwise the Logup pair: slot 0 = beta + h and slot
// 1 = m, or the constant 1 when m is empty.  Only a table that is used has to
// be there.  QG_ERR_UNSUPPORTED: outside the compiled envelope (128 monomials,
// 512 factors, 64 tables).
static LgIo* lg_setup(qg_ctx* ctx, LgDev& img, uint32_t ntables, const std::vector<const Fr*>& tabs,
                      const LgExpr& h, const uint64_t* beta, const LgExpr& m) {
  memset(&img, 0, sizeof(img));
  std::vector<uint32_t> used;
  uint32_t nfac = 0;
  lg_compile(img, 0, compile_program(h.prog, h.len, h.consts, h.nconsts, ntables),
             beta ? fr_import(beta) : Fr::zero(), beta != nullptr, used, nfac);
  if (beta && m)
    lg_compile(img, 1, compile_program(m.prog, m.len, m.consts, m.nconsts, ntables), Fr::zero(),
               false, used, nfac);
  else if (beta)
    lg_compile(img, 1, SopProgram{}, Fr::one(), true, used, nfac);
  for (size_t s = 0; s < used.size(); s++) {
    QG_CHECK(tabs[used[s]], QG_ERR_INVALID, "table buffer missing or too short");
    img.tab[s] = tabs[used[s]];
  }
  QG_HIP(hipSetDevice(ctx->device));
  LgIo* io = ctx->scratch_as<LgIo>("lg_io", 1);
  QG_HIP(hipMemcpyAsync(&io->img, &img, sizeof(img), hipMemcpyHostToDevice, ctx->stream));
  return io;
}

// lg_setup, and for expressions outside the compiled envelope (it answered
// QG_ERR_UNSUPPORTED) the generic interpreter: h (and m) are materialised with
// expr_table_device, and the image runs over those columns with h = Input(0),
// m = Input(1).  Every table has to be there then.
static LgIo* lg_setup_any(qg_ctx* ctx, LgDev& img, size_t n, uint32_t ntables,
                          const std::vector<const Fr*>& tabs, const LgExpr& h, const uint64_t* beta,
                          const LgExpr& m) {
  try {
    return lg_setup(ctx, img, ntables, tabs, h, beta, m);
  } catch (const Error& e) {
    if (e.code != QG_ERR_UNSUPPORTED) throw;
  }
  for (const Fr* t : tabs) QG_CHECK(t, QG_ERR_INVALID, "table buffer missing or too short");
  const bool has_m = beta && m;
  Fr* ev = ctx->scratch_as<Fr>("lg_gen_tabs", n * (has_m ? 2 : 1));
  expr_table_device(ctx, n, ntables, tabs, h.prog, h.len, h.consts, h.nconsts, ev);
  if (has_m) expr_table_device(ctx, n, ntables, tabs, m.prog, m.len, m.consts, m.nconsts, ev + n);
  static const qg_expr_op in0[1] = {{QG_OP_INPUT, 0}}, in1[1] = {{QG_OP_INPUT, 1}};
  std::vector<const Fr*> cols{ev};
  if (has_m) cols.push_back(ev + n);
  return lg_setup(ctx, img, (uint32_t)cols.size(), cols, LgExpr{in0, 1}, beta,
                  has_m ? LgExpr{in1, 1} : LgExpr{});
}

static size_t lg_local_size(const qg_ctx* ctx, uint32_t nvars) {
  uint32_t lw = 0;
  while ((1 << lw) < ctx->world) lw++;
  QG_CHECK((1 << lw) == ctx->world, QG_ERR_INVALID, "world size must be a power of two");
  QG_CHECK(nvars >= lw, QG_ERR_INVALID, "nvars must be at least log2(world)");
  QG_CHECK(nvars < 40, QG_ERR_INVALID, "nvars too large");
  return (size_t)1 << (nvars - lw);
}

// the column sum (d_res) and the zero-denominator flag (d_err) of this rank,
// summed / or-ed over all ranks; QG_ERR_ASSERT when any rank had a zero
static Fr logup_total(qg_ctx* ctx, const Fr* d_res, const uint32_t* d_err) {
  struct {
    Fr res;
    uint32_t err;
  } h;
  QG_HIP(hipMemcpyAsync(&h.err, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
  QG_HIP(hipMemcpyAsync(&h.res, d_res, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  if (h.err) h.res = Fr::zero();
  // every rank learns whether any rank hit a zero denominator, and the global sum
  struct {
    Fr s;
    uint32_t err, pad[7];
  } mine{h.res, h.err, {}};
  Fr total = Fr::zero();
  uint32_t any_err = 0;
  if (ctx->sharded) {
    uint8_t* d_g = ctx->scratch_as<uint8_t>("lg_gather", sizeof(mine) * (ctx->world + 1));
    QG_HIP(hipMemcpyAsync(d_g, &mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream));
    comm_allgather_bytes(ctx, d_g, d_g + sizeof(mine), sizeof(mine));
    std::vector<decltype(mine)> all(ctx->world);
    QG_HIP(hipMemcpyAsync(all.data(), d_g + sizeof(mine), sizeof(mine) * ctx->world,
                          hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    for (auto& a : all) {
      total = total + a.s;
      any_err |= a.err;
    }
  } else {
    total = h.res;
    any_err = h.err;
  }
  QG_CHECK(!any_err, QG_ERR_ASSERT, "logup denominator beta + h(x) is zero (reference: inverse().unwrap())");
  return total;
}

// out[x] = m(x) / (beta + h(x)) over this rank's rows; returns sum_x out[x]
// over all ranks (Fr, i.e. arkworks Montgomery words)
static Fr logup_run(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const std::vector<const Fr*>& tabs,
                    const LgExpr& h, const LgExpr& m, const uint64_t beta[4], Fr* d_out) {
  QG_CHECK(h, QG_ERR_INVALID, "missing h expression");
  const size_t n = lg_local_size(ctx, nvars);
  LgDev img;
  LgIo* io = lg_setup_any(ctx, img, n, ntables, tabs, h, beta, m);

  const uint32_t nb = div_up(n, LG_ROWS);
  Fr* d_bsum = ctx->scratch_as<Fr>("lg_bsum", nb);
  // block products, their exclusive prefix / suffix products, total, 1/total
  Fr* d_bp = ctx->scratch_as<Fr>("lg_bprod", 3 * (size_t)nb + 2);
  Fr* d_pre = d_bp + nb;
  Fr* d_suf = d_pre + nb;
  Fr* d_tot = d_suf + nb;
  Fr* d_tinv = d_tot + 1;
  QG_HIP(hipMemsetAsync(&io->err, 0, 4, ctx->stream));
  struct {
    Fr tot;
    uint32_t err;
  } ht;
  {
    // kernel time only: the timed region closes before the D2H copies and the sync
    QgTimed tm(ctx, "logup_column");
    hipLaunchKernelGGL(k_logup_den, dim3(nb), dim3(LG_DEN_BLOCK), 0, ctx->stream, &io->img, n, d_out,
                       d_bp, &io->err);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_logup_scan, dim3(1), dim3(LG_BLOCK), 0, ctx->stream, d_bp, nb, d_pre,
                       d_suf, d_tot);
    QG_LAUNCH_CHECK();
  }
  QG_HIP(hipMemcpyAsync(&ht.tot, d_tot, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  QG_HIP(hipMemcpyAsync(&ht.err, &io->err, 4, hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  // one inversion for the whole column, of the product of every denominator:
  // tinv = tot^-1 2^517 (the domains: top of the file)
  Fr tinv = Fr::zero();
  if (!ht.err) {
    const Fr tot_plain = ht.tot;  // nonzero: no denominator was zero
    Fr inv_plain = inv_bingcd<FrP>(tot_plain);
    // one multiply checks the binary GCD (its iteration bound has little
    // slack); Fermat inversion if it ever did not converge
    if (!(lg_plain_mul(tot_plain, inv_plain) == from_mont(Fr::one())))
      inv_plain = from_mont(finv(to_mont(tot_plain)));
    tinv = lg_plain_mul(inv_plain, pow2_mod_plain<FrP>(517));
    QG_HIP(hipMemcpyAsync(d_tinv, &tinv, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    QgTimed tm(ctx, "logup_column");
    hipLaunchKernelGGL(k_logup, dim3(nb), dim3(LG_BLOCK), 0, ctx->stream, &io->img, n, d_out, d_pre,
                       d_suf, d_tinv, d_bsum);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_logup_sum, dim3(1), dim3(LG_BLOCK), 0, ctx->stream, d_bsum, nb, &io->res);
    QG_LAUNCH_CHECK();
  }
  return logup_total(ctx, &io->res, &io->err);
}

// d_out[x] = h(tabs[.][x]) over this rank's n rows, canonical Montgomery words.
// Only the compiled image: an expression beyond lg_compile's limits (128
// monomials, 512 factors, 64 tables) is QG_ERR_UNSUPPORTED, not interpreted.
static void expr_column_run(qg_ctx* ctx, size_t n, uint32_t ntables,
                            const std::vector<const Fr*>& tabs, const LgExpr& h, Fr* d_out) {
  LgDev img;
  LgIo* io = lg_setup(ctx, img, ntables, tabs, h, nullptr, LgExpr{});
  {
    QgTimed tm(ctx, "expr_column");
    hipLaunchKernelGGL(k_expr_column, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, &io->img, n,
                       d_out);
    QG_LAUNCH_CHECK();
  }
  ctx->sync();
}

// ---- the column entries' table arguments ------------------------------------
// the _dev entries: the output and every table present and at least n long, no
// table sharing an entry with the output's n (k_logup_den writes out[row] while
// other blocks still read the tables, and k_logup reads them again for m)
static std::vector<const Fr*> lg_dev_tables(uint32_t ntables, const qg_buf* const* tables, size_t n,
                                            const qg_buf* out) {
  QG_CHECK(ntables == 0 || tables, QG_ERR_INVALID, "null tables");
  QG_CHECK(out->n >= n, QG_ERR_INVALID, "output buffer too short");
  std::vector<const Fr*> tabs;
  for (uint32_t i = 0; i < ntables; i++) {
    QG_CHECK(tables[i] && tables[i]->n >= n, QG_ERR_INVALID, "table buffer missing or too short");
    QG_CHECK(!ranges_overlap(out->d, n, tables[i]->d, n), QG_ERR_INVALID,
             "output aliases an input table");
    tabs.push_back(tables[i]->d);
  }
  return tabs;
}

// the host entries: every table present, uploaded into "lg_in"; returns the
// output column, which follows the tables there
static Fr* lg_upload_tables(qg_ctx* ctx, uint32_t ntables, const uint64_t* const* tables, size_t n,
                            std::vector<const Fr*>& tabs) {
  QG_CHECK(ntables == 0 || tables, QG_ERR_INVALID, "null tables");
  for (uint32_t i = 0; i < ntables; i++) QG_CHECK(tables[i] != nullptr, QG_ERR_INVALID, "null table");
  QG_HIP(hipSetDevice(ctx->device));
  Fr* d = ctx->scratch_as<Fr>("lg_in", n * ((size_t)ntables + 1));
  for (uint32_t i = 0; i < ntables; i++) {
    fr_upload(ctx, d + n * i, tables[i], n);
    tabs.push_back(d + n * i);
  }
  return d + n * ntables;
}

}  // namespace qg

// ---------------------------------------------------------------- C-ABI
extern "C" {

int qg_expr_column(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const uint64_t* const* tables,
                   const qg_expr_op* prog, size_t len, const uint64_t* consts, size_t nconsts,
                   uint64_t* out) {
  return qg_guard(ctx, [&] {
    QG_CHECK(ctx && prog && len && out, QG_ERR_INVALID, "null argument");
    QG_CHECK(nconsts == 0 || consts, QG_ERR_INVALID, "null constants");
    const size_t n = lg_local_size(ctx, nvars);
    for (uint32_t i = 0; tables && i < ntables; i++)
      QG_CHECK(!tables[i] || !ranges_overlap(out, 4 * n, tables[i], 4 * n), QG_ERR_INVALID,
               "output aliases an input table");
    std::vector<const Fr*> tabs;
    Fr* d_out = lg_upload_tables(ctx, ntables, tables, n, tabs);
    expr_column_run(ctx, n, ntables, tabs, LgExpr{prog, len, consts, nconsts}, d_out);
    fr_download(ctx, out, d_out, n);
    ctx->sync();
  });
}

int qg_expr_column_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const qg_buf* const* tables,
                       const qg_expr_op* prog, size_t len, const uint64_t* consts, size_t nconsts,
                       qg_buf* out) {
  return qg_guard(ctx, [&] {
    QG_CHECK(ctx && prog && len && out, QG_ERR_INVALID, "null argument");
    QG_CHECK(nconsts == 0 || consts, QG_ERR_INVALID, "null constants");
    const size_t n = lg_local_size(ctx, nvars);
    const std::vector<const Fr*> tabs = lg_dev_tables(ntables, tables, n, out);
    expr_column_run(ctx, n, ntables, tabs, LgExpr{prog, len, consts, nconsts}, out->d);
  });
}

int qg_logup_column(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const uint64_t* const* tables,
                    const qg_expr_op* h_prog, size_t h_len, const uint64_t* h_consts,
                    size_t h_nconsts, const qg_expr_op* m_prog, size_t m_len,
                    const uint64_t* m_consts, size_t m_nconsts, const uint64_t beta[4],
                    uint64_t* out, uint64_t out_sum[4]) {
  return qg_guard(ctx, [&] {
    QG_CHECK(ctx && beta && out, QG_ERR_INVALID, "null argument");
    const size_t n = lg_local_size(ctx, nvars);
    std::vector<const Fr*> tabs;
    Fr* d_out = lg_upload_tables(ctx, ntables, tables, n, tabs);
    const Fr s = logup_run(ctx, nvars, ntables, tabs, LgExpr{h_prog, h_len, h_consts, h_nconsts},
                           LgExpr{m_prog, m_len, m_consts, m_nconsts}, beta, d_out);
    fr_download(ctx, out, d_out, n);
    if (out_sum) fr_export(s, out_sum);
  });
}

int qg_logup_column_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const qg_buf* const* tables,
                        const qg_expr_op* h_prog, size_t h_len, const uint64_t* h_consts,
                        size_t h_nconsts, const qg_expr_op* m_prog, size_t m_len,
                        const uint64_t* m_consts, size_t m_nconsts, const uint64_t beta[4],
                        qg_buf* out, uint64_t out_sum[4]) {
  return qg_guard(ctx, [&] {
    QG_CHECK(ctx && beta && out, QG_ERR_INVALID, "null argument");
    const size_t n = lg_local_size(ctx, nvars);
    const std::vector<const Fr*> tabs = lg_dev_tables(ntables, tables, n, out);
    const Fr s = logup_run(ctx, nvars, ntables, tabs, LgExpr{h_prog, h_len, h_consts, h_nconsts},
                           LgExpr{m_prog, m_len, m_consts, m_nconsts}, beta, out->d);
    if (out_sum) fr_export(s, out_sum);
  });
}

// Circuit::check_constraints (transition_circuit.rs:153-172): first row x
// (this rank's block) with h(x) != 0, or -1.
int qg_expr_first_nonzero_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                              const qg_buf* const* tables, const qg_expr_op* prog, size_t len,
                              const uint64_t* consts, size_t nconsts, int64_t* first_row) {
  return qg_guard(ctx, [&] {
    QG_CHECK(ctx && prog && len && first_row, QG_ERR_INVALID, "null argument");
    QG_CHECK(ntables == 0 || tables, QG_ERR_INVALID, "null tables");
    const size_t n = lg_local_size(ctx, nvars);
    *first_row = -1;
    // a table that is missing or too short counts only where it is used
    std::vector<const Fr*> tabs(ntables, nullptr);
    for (uint32_t i = 0; i < ntables; i++)
      if (tables[i] && tables[i]->n >= n) tabs[i] = tables[i]->d;
    // slot 0 alone, no beta: the value in arkworks form (x 2^256); zero test only
    LgDev img;
    LgIo* io = lg_setup_any(ctx, img, n, ntables, tabs, LgExpr{prog, len, consts, nconsts}, nullptr,
                            LgExpr{});
    const unsigned long long init = n;
    QG_HIP(hipMemcpyAsync(&io->first, &init, 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_expr_first_nonzero, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                       &io->img, n, &io->first);
    QG_LAUNCH_CHECK();
    unsigned long long f = 0;
    QG_HIP(hipMemcpyAsync(&f, &io->first, 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    *first_row = f >= n ? -1 : (int64_t)f;
  });
}

}  // extern "C"
