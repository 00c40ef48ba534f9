// Multilinear PCS opening passes for gfx950 — replaces
//   KZG::open                          pcs/src/kzg.rs:75-96
//   MLEvalProof::compute_pr / prove    pcs/src/mlpcs.rs:52-124
//   InnerProductProof::compute_s_polynomial  pcs/src/ipa.rs:122-157
//
//  * compute_pr == the eq table (identity pinned by the KATs at
//    mlpcs.rs:226-242): built in O(2^n) on the device, no IFFT.
//  * y = p(x) and q = (p - y)/(X - x) come out of ONE suffix-Horner scan
//    s_i = c_i + x s_{i+1}:  y = s_0, q_i = s_{i+1}.  The scan is blocked:
//    per-chunk zero-carry values, a recursive scan of the chunk carries with
//    multiplier x^B, then a per-chunk apply pass.
//  * S_k = sum_i (f_{i+k+1} g_i + g_{i+k+1} f_i) is the upper half of
//    h = f*rev(g) + rev(f)*g.  Two forward NTTs (F, G) suffice:
//    NTT(rev f)[j] = w^{j(M-1)} F[-j], so H[j] = w^{j(M-1)} (F[j]G[-j] + F[-j]G[j]).
//  * Every commitment is the device MSM (msm.hip) over device-resident data.
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "blake3.h"
#include "common.h"
#include "field29.h"
#include "open_plan.h"

using namespace qg;

namespace qg {

static constexpr int ML_BLOCK = 256;
static constexpr int SH_B = 32;  // suffix-Horner chunk length

// ---------------------------------------------------------------- reductions
QG_DEV Fr block_sum_fr(Fr v, Fr* lds) {
  for (int m = 32; m > 0; m >>= 1) v = v + shfl_xor_fr(v, m);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  Fr acc = Fr::zero();
  if (threadIdx.x == 0)
    for (int w = 0; w < nw; w++) acc = acc + lds[w];
  __syncthreads();
  return acc;
}

__global__ void __launch_bounds__(ML_BLOCK)
    k_dot(const Fr* __restrict__ f, const Fr* __restrict__ g, size_t n, Fr* __restrict__ partial) {
  __shared__ Fr lds[ML_BLOCK / 64];
  Fr acc = Fr::zero();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    acc = acc + f[i] * g[i];
  acc = block_sum_fr(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(ML_BLOCK)
    k_sum(const Fr* __restrict__ in, size_t n, Fr* __restrict__ out) {
  __shared__ Fr lds[ML_BLOCK / 64];
  Fr acc = Fr::zero();
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc = acc + in[i];
  acc = block_sum_fr(acc, lds);
  if (threadIdx.x == 0) *out = acc;
}

// <f, g> into device memory (no host round trip)
static void dot_to_device(qg_ctx* ctx, const Fr* f, const Fr* g, size_t n, Fr* d_out) {
  if (n == 0) {
    QG_HIP(hipMemsetAsync(d_out, 0, sizeof(Fr), ctx->stream));
    return;
  }
  QgTimed tm(ctx, "inner_product");
  unsigned blocks = (unsigned)std::min<size_t>(2048, div_up(n, ML_BLOCK));
  Fr* part = ctx->scratch_as<Fr>("dot_part", blocks);
  hipLaunchKernelGGL(k_dot, dim3(blocks), dim3(ML_BLOCK), 0, ctx->stream, f, g, n, part);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum, dim3(1), dim3(ML_BLOCK), 0, ctx->stream, part, (size_t)blocks, d_out);
  QG_LAUNCH_CHECK();
}

static Fr dot_device(qg_ctx* ctx, const Fr* f, const Fr* g, size_t n) {
  if (n == 0) return Fr::zero();
  QgTimed tm(ctx, "inner_product");
  unsigned blocks = (unsigned)std::min<size_t>(2048, div_up(n, ML_BLOCK));
  Fr* part = ctx->scratch_as<Fr>("dot_part", blocks + 1);
  hipLaunchKernelGGL(k_dot, dim3(blocks), dim3(ML_BLOCK), 0, ctx->stream, f, g, n, part);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum, dim3(1), dim3(ML_BLOCK), 0, ctx->stream, part, (size_t)blocks,
                     part + blocks);
  QG_LAUNCH_CHECK();
  Fr r;
  QG_HIP(hipMemcpyAsync(&r, part + blocks, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  return r;
}

// ---------------------------------------------------------------- suffix Horner
// s_i = c_i + x s_{i+1}, blocked: A_k = sum_{i in chunk k} c_i x^(i - start_k)
// (local pass), T_k = A_k + x^B T_{k+1} (the same scan one level up), then
// s_i for every i of chunk k from T_{k+1} (apply pass).  Up to SH_J jobs per
// launch (blockIdx.y = job), each ONE polynomial at NP points: NP = 1 is a
// plain scan; NP = 2 is the two scans the inner-product argument opens at r
// and 1/r (ipa.rs:87-92, and its TODO at :86).  A thread then carries two
// accumulators over the same coefficient strip and writes two suffix vectors:
// the coefficient loads and their to29 conversions are shared, and the
// per-chunk Horner chain runs as two independent chains per thread.  Each
// chain performs exactly the steps of an NP = 1 job, so the outputs are
// bit-identical to two single jobs.
// The arithmetic is in 9 x 29-bit limbs (each step c_i + x s_{i+1}: a canonical
// coefficient plus a product < 2p, so one conditional subtraction keeps
// s < 2p): the per-chunk Horner chain is the latency of the whole recursion,
// and the 29-bit multiply's dependent latency is half the 32-bit one's.  x is
// passed as x 2^261 (plain limbs), so mul29 keeps the arkworks scale of the
// coefficients; every stored value is canonical arkworks form.
template <int NP>
struct ShJob {
  const Fr* c;      // coefficients (arkworks form)
  size_t L;
  L9 x[NP];         // x_p 2^261 mod p
  Fr* A[NP];        // chunk values (local pass)
  const Fr* T[NP];  // chunk carries (apply pass)
  size_t nch;
  Fr* s[NP];        // output suffixes
};
static constexpr int SH_J = 4;  // jobs per launch
template <int NP>
struct ShJobs {
  ShJob<NP> j[SH_J];
};

// one Horner step of every chain on the shared (converted) coefficient
template <int NP>
__device__ __forceinline__ void sh_step(const F29<FrP>& ci, const F29<FrP> (&x)[NP],
                                        F29<FrP> (&acc)[NP]) {
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p] = red2p29(add29(ci, mul29(x[p], acc[p])));
}

// The apply pass on a full chunk runs software-pipelined: its coefficients
// come in groups of SH_G, the next group's loads issued before the current
// group's dependent products and stores (one load round trip per group instead
// of per step, which the stores would otherwise pin in program order); a short
// last chunk loops.  Every suffix value is written.
// The outputs are __restrict__ parameters of their own (out1 only at NP = 2):
// read through the job struct at every store, the NP = 2 pass waits on the
// pointer reloads between its stores and runs 17 % longer
// (profiles/r11_open_unify_ab.txt).
static constexpr int SH_G = 4;
template <int NP>
__device__ __forceinline__ void sh_apply_chunk(const Fr* __restrict__ c, Fr* __restrict__ out0,
                                               Fr* __restrict__ out1, size_t s, size_t e,
                                               const F29<FrP> (&x)[NP], F29<FrP> (&acc)[NP]) {
  static_assert(NP == 1 || NP == 2, "one or two points per polynomial");
  if (e - s == SH_B) {
    Fr cur[SH_G], nxt[SH_G];
#pragma unroll
    for (int j = 0; j < SH_G; j++) cur[j] = c[s + SH_B - SH_G + j];
#pragma unroll
    for (int g = SH_B / SH_G - 1; g >= 0; g--) {
      if (g > 0) {
#pragma unroll
        for (int j = 0; j < SH_G; j++) nxt[j] = c[s + (size_t)(g - 1) * SH_G + j];
      }
      // keeps the scheduler from hoisting later groups' loads above this
      // group's products
      asm volatile("" ::: "memory");
#pragma unroll
      for (int j = SH_G - 1; j >= 0; j--) {
        sh_step<NP>(to29(cur[j]), x, acc);
        out0[s + (size_t)g * SH_G + j] = from29(canon29(acc[0]));
        if constexpr (NP == 2) out1[s + (size_t)g * SH_G + j] = from29(canon29(acc[1]));
      }
      if (g > 0) {
#pragma unroll
        for (int j = 0; j < SH_G; j++) cur[j] = nxt[j];
      }
    }
  } else {
    for (size_t i = e; i-- > s;) {
      sh_step<NP>(to29(c[i]), x, acc);
      out0[i] = from29(canon29(acc[0]));
      if constexpr (NP == 2) out1[i] = from29(canon29(acc[1]));
    }
  }
}

template <int NP>
__global__ void k_sh_local(ShJobs<NP> jb) {
  const ShJob<NP>& J = jb.j[blockIdx.y];
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = k * SH_B;
  if (s >= J.L) return;
  const size_t e = s + SH_B < J.L ? s + SH_B : J.L;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) x[p] = F29<FrP>::from_l9(J.x[p]), acc[p] = F29<FrP>::zero();
  // no stores in this chain: an unrolled loop lets the loads run ahead
#pragma unroll 4
  for (size_t i = e; i-- > s;) sh_step<NP>(to29(J.c[i]), x, acc);
#pragma unroll
  for (int p = 0; p < NP; p++) J.A[p][k] = from29(canon29(acc[p]));
}

template <int NP>
__global__ void k_sh_apply(ShJobs<NP> jb) {
  const ShJob<NP>& J = jb.j[blockIdx.y];
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = k * SH_B;
  if (s >= J.L) return;
  const size_t e = s + SH_B < J.L ? s + SH_B : J.L;
  const bool carry = k + 1 < J.nch;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    x[p] = F29<FrP>::from_l9(J.x[p]);
    acc[p] = carry ? to29(J.T[p][k + 1]) : F29<FrP>::zero();
  }
  sh_apply_chunk<NP>(J.c, J.s[0], J.s[NP - 1], s, e, x, acc);
}

// small case: one thread per job
template <int NP>
__global__ void k_sh_serial(ShJobs<NP> jb) {
  const ShJob<NP>& J = jb.j[blockIdx.y];
  if (threadIdx.x != 0) return;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) x[p] = F29<FrP>::from_l9(J.x[p]), acc[p] = F29<FrP>::zero();
  for (size_t i = J.L; i-- > 0;) {
    sh_step<NP>(to29(J.c[i]), x, acc);
#pragma unroll
    for (int p = 0; p < NP; p++) J.s[p][i] = from29(canon29(acc[p]));
  }
}

template <int NP>
struct ShIn {
  const Fr* c;
  size_t L;
  Fr x[NP];  // Montgomery
  Fr* s[NP];
};

static L9 x261_of(const Fr& x) {
  static const Fr k261 = to_mont(pow2_mod_plain<FrP>(261));  // (261 doublings: once)
  const Fr t = from_mont(to_mont(from_mont(x)) * k261);
  const F29<FrP> r = to29(t);
  L9 o{};
  for (int i = 0; i < 9; i++) o.v[i] = r.l[i];
  return o;
}

static void suffix_horner_many(qg_ctx* ctx, const std::vector<ShIn<1>>& in, int depth);

// s^p_i = c_i + x_p s^p_{i+1}, p < NP, for up to SH_J polynomials at once.
// The chunk values of different points are different vectors, so the levels
// above run as NP = 1 jobs.
template <int NP>
static void suffix_horner(qg_ctx* ctx, const std::vector<ShIn<NP>>& in, int depth = 0) {
  QG_CHECK(in.size() <= (size_t)SH_J, QG_ERR_ASSERT, "suffix-Horner batch of at most 4");
  std::vector<ShIn<NP>> small, big;
  for (const ShIn<NP>& q : in)
    if (q.L > SH_B) big.push_back(q);
    else if (q.L > 0) small.push_back(q);
  if (!small.empty()) {
    ShJobs<NP> jb{};
    for (size_t q = 0; q < small.size(); q++) {
      ShJob<NP>& j = jb.j[q];
      j.c = small[q].c, j.L = small[q].L;
      for (int p = 0; p < NP; p++) j.x[p] = x261_of(small[q].x[p]), j.s[p] = small[q].s[p];
    }
    hipLaunchKernelGGL(k_sh_serial<NP>, dim3(1, (unsigned)small.size()), dim3(64), 0, ctx->stream,
                       jb);
    QG_LAUNCH_CHECK();
  }
  if (big.empty()) return;
  ShJobs<NP> jb{};
  std::vector<ShIn<1>> up;
  size_t maxch = 0;
  for (size_t q = 0; q < big.size(); q++) {
    const size_t nch = (big[q].L + SH_B - 1) / SH_B;
    ShJob<NP>& j = jb.j[q];
    j.c = big[q].c, j.L = big[q].L, j.nch = nch;
    for (int p = 0; p < NP; p++) {
      const std::string tag = std::to_string(depth) + "_" + std::to_string(NP * q + p);
      Fr* A = ctx->scratch_as<Fr>("sh_A" + tag, nch);
      Fr* T = ctx->scratch_as<Fr>("sh_T" + tag, nch);
      j.x[p] = x261_of(big[q].x[p]), j.A[p] = A, j.T[p] = T, j.s[p] = big[q].s[p];
      up.push_back({A, nch, {fpow_small(big[q].x[p], SH_B)}, {T}});  // T_k = A_k + x^B T_{k+1}
    }
    maxch = std::max(maxch, nch);
  }
  const dim3 grid((unsigned)div_up(maxch, ML_BLOCK), (unsigned)big.size());
  hipLaunchKernelGGL(k_sh_local<NP>, grid, dim3(ML_BLOCK), 0, ctx->stream, jb);
  QG_LAUNCH_CHECK();
  suffix_horner_many(ctx, up, depth + 1);
  hipLaunchKernelGGL(k_sh_apply<NP>, grid, dim3(ML_BLOCK), 0, ctx->stream, jb);
  QG_LAUNCH_CHECK();
}

// more than SH_J scans: groups of SH_J, one after the other in stream order
// (the groups share the recursion's chunk scratch, which no group reads after
// its own apply pass)
static void suffix_horner_many(qg_ctx* ctx, const std::vector<ShIn<1>>& in, int depth = 0) {
  for (size_t b = 0; b < in.size(); b += SH_J)
    suffix_horner<1>(
        ctx, std::vector<ShIn<1>>(in.begin() + b, in.begin() + std::min(in.size(), b + SH_J)),
        depth);
}

// ---- the folded scan: ONE polynomial h = sum_j g_j p_j of up to SHF_P source
// vectors, never materialised, at NP points.  The coefficient of every Horner
// step is formed on the fly, c_i = sum_j g_j p_j[i] (a source shorter than i
// contributes 0; g_0 = 1 skips its product), so one pass reads each source
// once and writes NP suffix vectors.  Same blocking as above; the chunk values
// A and carries T are plain vectors, so the levels above are the NP = 1 jobs.
// g_j arrives as g_j 2^261 (plain limbs, x261_of), so mul29 keeps the arkworks
// scale of the sources.
// Bounds: a term is a canonical source value (< p, g_0 = 1) or a product
// (< 2p, normalized); the lazy sum of P <= 4 of them is < 8p with limbs < 2^31.
// P = 2: < 4p, red2p29's range; P > 2: red16p29.  Either way the folded
// coefficient is normalized and < 2p, so each step c_i + x s_{i+1} is
// < 2p + 2p = 4p before red2p29 (sh_step's own bound is p + 2p) and s stays
// < 2p.  Stored values are canonical, so the bits equal those of the scan
// over a materialised canonical h (k_lincomb, then suffix_horner<NP>).
static constexpr int SHF_P = 4;
struct ShFoldSrc {
  const Fr* c[SHF_P];
  size_t n[SHF_P];  // coefficients of source j (0 past them)
  L9 g[SHF_P];      // g_j 2^261 mod p
  int P;
  int one0;         // g_0 == 1: source 0 enters unmultiplied
};
template <int NP>
struct ShFoldJob {
  ShFoldSrc src;
  size_t L;         // scan length (>= every n[j])
  L9 x[NP];
  Fr* A[NP];
  const Fr* T[NP];
  size_t nch;
  Fr* s[NP];
};

__device__ __forceinline__ F29<FrP> shf_coef(const ShFoldSrc& S, size_t i) {
  F29<FrP> c = F29<FrP>::zero();
  if (i < S.n[0]) {
    c = to29(S.c[0][i]);
    if (!S.one0) c = mul29(F29<FrP>::from_l9(S.g[0]), c);
  }
#pragma unroll
  for (int j = 1; j < SHF_P; j++)
    if (j < S.P && i < S.n[j]) c = add29(c, mul29(F29<FrP>::from_l9(S.g[j]), to29(S.c[j][i])));
  return S.P <= 2 ? red2p29(c) : red16p29(c);
}

template <int NP>
__global__ void __launch_bounds__(ML_BLOCK) k_shf_local(ShFoldJob<NP> J) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = k * SH_B;
  if (s >= J.L) return;
  const size_t e = s + SH_B < J.L ? s + SH_B : J.L;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) x[p] = F29<FrP>::from_l9(J.x[p]), acc[p] = F29<FrP>::zero();
#pragma unroll 2
  for (size_t i = e; i-- > s;) sh_step<NP>(shf_coef(J.src, i), x, acc);
#pragma unroll
  for (int p = 0; p < NP; p++) J.A[p][k] = from29(canon29(acc[p]));
}

template <int NP>
__global__ void __launch_bounds__(ML_BLOCK) k_shf_apply(ShFoldJob<NP> J) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = k * SH_B;
  if (s >= J.L) return;
  const size_t e = s + SH_B < J.L ? s + SH_B : J.L;
  const bool carry = k + 1 < J.nch;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    x[p] = F29<FrP>::from_l9(J.x[p]);
    acc[p] = carry ? to29(J.T[p][k + 1]) : F29<FrP>::zero();
  }
  Fr* __restrict__ out0 = J.s[0];
  Fr* __restrict__ out1 = J.s[NP - 1];
#pragma unroll 2
  for (size_t i = e; i-- > s;) {
    sh_step<NP>(shf_coef(J.src, i), x, acc);
    out0[i] = from29(canon29(acc[0]));
    if constexpr (NP == 2) out1[i] = from29(canon29(acc[1]));
  }
}

// small case: one thread
template <int NP>
__global__ void k_shf_serial(ShFoldJob<NP> J) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  F29<FrP> x[NP], acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) x[p] = F29<FrP>::from_l9(J.x[p]), acc[p] = F29<FrP>::zero();
  for (size_t i = J.L; i-- > 0;) {
    sh_step<NP>(shf_coef(J.src, i), x, acc);
#pragma unroll
    for (int p = 0; p < NP; p++) J.s[p][i] = from29(canon29(acc[p]));
  }
}

// h = sum_j g[j] c[j] (P sources of n[j] coefficients, g Montgomery) scanned
// over its first L coefficients at NP points: s[p][i] for i < L.
template <int NP>
struct ShFoldIn {
  const Fr* c[SHF_P];
  size_t n[SHF_P];
  Fr g[SHF_P];
  int P;
  size_t L;
  Fr x[NP];
  Fr* s[NP];
};

// Two routes, the same bits either way: the fused scan above, or the unfused
// composition - h into scratch by k_lincomb, then suffix_horner<NP>.
// QG_FOLD_FUSED (read per call) selects: 1 the fused scan, 0 the composition.
// Unset is the composition: measured at 2^22 entries (profiles/fold_open.json,
// DESIGN section 5 "Folded opening") the fused scan's region is 0.653 ms
// against 0.642 ms, beyond the spread of the repeated medians (0.009 ms; an
// earlier visit on another box: 0.642 against 0.618) - its two strided source
// reads per pass cost more than the coalesced k_lincomb pass and the 256 MB
// it writes and reads back.
template <int NP>
static void suffix_horner_fold(qg_ctx* ctx, const ShFoldIn<NP>& in) {
  static_assert(NP == 1 || NP == 2, "one or two points");
  if (in.L == 0) return;
  QG_CHECK(in.P >= 1 && in.P <= SHF_P, QG_ERR_ASSERT, "folded scan of one to four sources");
  const char* fe = getenv("QG_FOLD_FUSED");
  if (!(fe && atoi(fe) != 0)) {
    // h over [0, L): between two consecutive source lengths the live sources
    // are a fixed subset, one k_lincomb launch each (a source never read past
    // its end); a stretch with no live source is 0
    Fr* h = ctx->scratch_as<Fr>("fold_h", in.L);
    size_t a = 0;
    while (a < in.L) {
      size_t b = in.L;
      const Fr* src[SHF_P];
      Fr g[SHF_P];
      size_t m = 0;
      for (int j = 0; j < in.P; j++) {
        const size_t nj = std::min(in.n[j], in.L);
        if (nj > a) src[m] = in.c[j] + a, g[m] = in.g[j], m++, b = std::min(b, nj);
      }
      if (m) lincomb_queue(ctx, src, g, m, b - a, h + a);
      else QG_HIP(hipMemsetAsync(h + a, 0, (b - a) * sizeof(Fr), ctx->stream));
      a = b;
    }
    ShIn<NP> one{h, in.L, {}, {}};
    for (int p = 0; p < NP; p++) one.x[p] = in.x[p], one.s[p] = in.s[p];
    return suffix_horner<NP>(ctx, {one});
  }
  ShFoldJob<NP> j{};
  j.src.P = in.P;
  j.src.one0 = in.g[0] == Fr::one() ? 1 : 0;
  for (int q = 0; q < in.P; q++) {
    j.src.c[q] = in.c[q], j.src.n[q] = std::min(in.n[q], in.L);
    j.src.g[q] = x261_of(in.g[q]);
  }
  j.L = in.L;
  for (int p = 0; p < NP; p++) j.x[p] = x261_of(in.x[p]), j.s[p] = in.s[p];
  if (in.L <= (size_t)SH_B) {
    hipLaunchKernelGGL(k_shf_serial<NP>, dim3(1), dim3(64), 0, ctx->stream, j);
    QG_LAUNCH_CHECK();
    return;
  }
  const size_t nch = (in.L + SH_B - 1) / SH_B;
  j.nch = nch;
  std::vector<ShIn<1>> up;
  for (int p = 0; p < NP; p++) {  // the chunk slots of suffix_horner's job 0
    Fr* A = ctx->scratch_as<Fr>("sh_A0_" + std::to_string(p), nch);
    Fr* T = ctx->scratch_as<Fr>("sh_T0_" + std::to_string(p), nch);
    j.A[p] = A, j.T[p] = T;
    up.push_back({A, nch, {fpow_small(in.x[p], SH_B)}, {T}});
  }
  const dim3 grid((unsigned)div_up(nch, ML_BLOCK));
  hipLaunchKernelGGL(k_shf_local<NP>, grid, dim3(ML_BLOCK), 0, ctx->stream, j);
  QG_LAUNCH_CHECK();
  suffix_horner_many(ctx, up, 1);
  hipLaunchKernelGGL(k_shf_apply<NP>, grid, dim3(ML_BLOCK), 0, ctx->stream, j);
  QG_LAUNCH_CHECK();
}


// ---------------------------------------------------------------- polynomial evaluation
// DensePolynomial::evaluate (kzg.rs:78) as a reduction: sum_i c_i x^i of up to
// EV_MAXJ vectors per launch (blockIdx.y = job, like ShJobs) at NP points in
// one pass, in the 29-bit limbs of k_sh_local.  A thread loads each
// coefficient of a contiguous strip of S once and runs NP independent Horner
// chains (the folded inner-product argument evaluates f, g and S at r and
// 1/r); a block combines its 256 strip values with powers of x^S (shuffle tree
// inside a wave: lane l takes x^(S 2^k) times lane l + 2^k; then the four wave
// values through LDS) and writes one value per point and block span (256 S
// coefficients); a grid-stride loop covers the spans.  The last stage (LAST)
// is the same kernel over the span values (x -> x^span, one block): chain p
// reads its own span values c[p] and multiplies by x_p^shift (a slice's
// sigma-power offset).  The points, their strip powers and the strip length
// are the launch's - every job of a launch shares them, so EV_MAXJ jobs fit the
// kernel arguments.  One Fr product per coefficient and point against the 32
// bytes read: multiply-bound.  Stored values are canonical, so no
// output bit depends on the strip geometry.
static constexpr int EV_S = 32;    // first-stage thread strip
static constexpr int EV_T = 256;   // threads per block
static constexpr size_t EV_SPAN = (size_t)EV_S * EV_T;  // first-stage block span
static constexpr int EV_MAXJ = 8;
template <int NP>
struct EvJob {
  const Fr* c[NP];  // coefficients (arkworks form); first stage: c[0], span stage: one per point
  size_t n;
  L9 sh[NP];        // span stage: x_p^shift 2^261
  Fr* out[NP];      // out[p][g] = value of span g at x_p; span stage: out[p][0]
};
template <int NP>
struct EvJobs {
  L9 x[NP];      // x_p 2^261 mod p
  L9 xp[NP][7];  // x_p^(S 2^k) 2^261, k = 0..6
  size_t S;      // strip length (>= 1)
  EvJob<NP> j[EV_MAXJ];
};

template <int NP, bool LAST>
__global__ void __launch_bounds__(EV_T) __attribute__((amdgpu_waves_per_eu(4)))
k_poly_eval(EvJobs<NP> jb) {
  constexpr int EV_UNROLL = NP == 1 ? 4 : 2;  // of the strip loop, by measurement
  const EvJob<NP>& J = jb.j[blockIdx.y];
  __shared__ uint32_t lds[NP][EV_T / 64][9];
  F29<FrP> x[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) x[p] = F29<FrP>::from_l9(jb.x[p]);
  const size_t span = jb.S * EV_T;
  const size_t nspans = (J.n + span - 1) / span;
  if (LAST && nspans == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NP; p++) J.out[p][0] = Fr::zero();
  }
  for (size_t g = blockIdx.x; g < nspans; g += gridDim.x) {  // block-uniform
    const size_t s = g * span + (size_t)threadIdx.x * jb.S;
    F29<FrP> acc[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) acc[p] = F29<FrP>::zero();
    if (s < J.n) {
      const size_t e = jb.S < J.n - s ? s + jb.S : J.n;
#pragma unroll EV_UNROLL
      for (size_t i = e; i-- > s;) {
        const F29<FrP> c0 = to29(J.c[0][i]);
#pragma unroll
        for (int p = 0; p < NP; p++) {
          const F29<FrP> c = LAST && p ? to29(J.c[p][i]) : c0;
          acc[p] = red2p29(add29(c, mul29(x[p], acc[p])));
        }
      }
    }
    // lane l += x^(S m) * lane (l + m), m = 1, 2, .., 32, per chain: lane 0 ends
    // with the wave's 64 strips (a strip past n is 0)
#pragma unroll
    for (int k = 0; k < 6; k++) {
#pragma unroll
      for (int p = 0; p < NP; p++) {
        const F29<FrP> o = shfl_down29(acc[p], 1 << k);
        acc[p] = red2p29(add29(acc[p], mul29(F29<FrP>::from_l9(jb.xp[p][k]), o)));
      }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int p = 0; p < NP; p++)
#pragma unroll
        for (int i = 0; i < 9; i++) lds[p][wid][i] = acc[p].l[i];
    }
    __syncthreads();
    if (threadIdx.x < NP) {  // thread p finishes chain p
      const int p = threadIdx.x;
      const F29<FrP> pw = F29<FrP>::from_l9(jb.xp[p][6]);  // x_p^(64 S)
      F29<FrP> r = F29<FrP>::zero();
      for (int w = EV_T / 64 - 1; w >= 0; w--) {
        F29<FrP> v;
#pragma unroll
        for (int i = 0; i < 9; i++) v.l[i] = lds[p][w][i];
        r = red2p29(add29(v, mul29(pw, r)));
      }
      if (LAST) r = mul29(F29<FrP>::from_l9(J.sh[p]), r);
      J.out[p][g] = from29(canon29(r));
    }
    __syncthreads();
  }
}

struct EvIn {
  const Fr* c;
  size_t n;
  uint64_t shift;
};

static size_t ev_spans(size_t n) { return (n + EV_SPAN - 1) / EV_SPAN; }

// d_out[P i + j] = sum_{k < n_j} c_j[k] xs[i]^(shift_j + k), P = in.size(),
// i < NP (xs Montgomery), queued on the context stream: per EV_MAXJ vectors one
// first-stage and one span-stage launch.  QG_EVAL_BLOCKS=<k> caps the first
// stage's grid (read per call: tests make the grid-stride loop wrap at a small
// length).
template <int NP>
static void poly_eval_queue(qg_ctx* ctx, const std::vector<EvIn>& in, const Fr (&xs)[NP],
                            Fr* d_out) {
  const char* eb = getenv("QG_EVAL_BLOCKS");
  const size_t cap = eb && atoi(eb) > 0 ? (size_t)atoi(eb) : 4096;
  const size_t P = in.size();
  auto strip_powers = [](Fr b, L9 (&o)[7]) {  // b^(2^k), k = 0..6
    for (int k = 0; k < 7; k++, b = b * b) o[k] = x261_of(b);
  };
  // the span values of one launch, NP rows of `need`: one slot, sized once per
  // call for its largest launch (a slot that grows drains the streams; callers
  // that queue several calls reserve it first, poly_eval_reserve)
  size_t need = 1;
  for (size_t b = 0; b < P; b += EV_MAXJ) {
    size_t tot = 0;
    for (size_t q = b; q < std::min(P, b + EV_MAXJ); q++) tot += ev_spans(in[q].n);
    need = std::max(need, tot);
  }
  Fr* part = ctx->scratch_as<Fr>("ev_part", NP * need);
  for (size_t b = 0; b < P; b += EV_MAXJ) {
    const size_t nj = std::min<size_t>(EV_MAXJ, P - b);
    size_t maxsp = 0;
    for (size_t q = 0; q < nj; q++) maxsp = std::max(maxsp, ev_spans(in[b + q].n));
    EvJobs<NP> j1{}, j2{};
    j1.S = EV_S;
    j2.S = std::max<size_t>(1, (maxsp + EV_T - 1) / EV_T);  // one block covers every job's spans
    for (int p = 0; p < NP; p++) {
      const Fr X = fpow_small(xs[p], EV_SPAN);
      j1.x[p] = x261_of(xs[p]), j2.x[p] = x261_of(X);
      strip_powers(fpow_small(xs[p], EV_S), j1.xp[p]);
      strip_powers(fpow_small(X, j2.S), j2.xp[p]);
    }
    size_t off = 0;
    for (size_t q = 0; q < nj; q++) {
      const EvIn& I = in[b + q];
      EvJob<NP>& a = j1.j[q];
      EvJob<NP>& z = j2.j[q];
      a.n = I.n, z.n = ev_spans(I.n);
      for (int p = 0; p < NP; p++) {
        a.c[p] = I.c, a.out[p] = part + p * need + off;
        z.c[p] = a.out[p], z.sh[p] = x261_of(fpow_small(xs[p], I.shift));
        z.out[p] = d_out + p * P + b + q;
      }
      off += z.n;
    }
    if (maxsp) {
      hipLaunchKernelGGL((k_poly_eval<NP, false>),
                         dim3((unsigned)std::min(maxsp, cap), (unsigned)nj), dim3(EV_T), 0,
                         ctx->stream, j1);
      QG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_poly_eval<NP, true>), dim3(1, (unsigned)nj), dim3(EV_T), 0,
                       ctx->stream, j2);
    QG_LAUNCH_CHECK();
  }
}

// ev_part for later poly_eval_queue<np> calls of at most `jobs` vectors of at
// most `nmax` coefficients per launch (a batch reserves for its largest item up
// front).  A call needs np rows of max(1, sum of its launch's span counts) <=
// jobs * ev_spans(nmax) values, which is what this allocates, so no such call
// grows the slot (the arena reallocates only for a larger request).
static void poly_eval_reserve(qg_ctx* ctx, size_t jobs, size_t nmax, int np) {
  ctx->scratch_as<Fr>("ev_part",
                      np * std::max<size_t>(1, std::min<size_t>(jobs, EV_MAXJ) * ev_spans(nmax)));
}

// ---------------------------------------------------------------- quotient check
// KZG::open asserts q (X - x) == p - y after its division (kzg.rs:85,
// "Polynomial division failed").  Here: p(sigma) - y == q(sigma) (sigma - x) at
// the context's random point sigma (common.h: open_rng; exact in Fr, so it
// fails only with probability <= n / r for a wrong quotient), p over the
// caller's UNtrimmed length, q over the coefficients the MSM reads.
static bool open_check_on() {
  const char* e = getenv("QG_OPEN_CHECK");  // read per call; 0: A/B timing only
  return !(e && atoi(e) == 0);
}

struct OpenCk {
  const Fr* p;  // nullptr: nothing to check (no coefficients at all)
  size_t pn;
  const Fr* q;  // nullptr: the trimmed length was 0 - no quotient, y = 0, and the
  size_t qn;    // check is p(sigma) == 0 over the untrimmed length (a trim that
  const Fr* d_y;  // wrongly returned 0 would otherwise give a silent infinity proof)
  Fr x;
};
struct OpenFin {
  const Fr* ev;
  const Fr* y[4];
  Fr d[4];  // sigma - x
  int pi[4], qi[4];
  uint32_t* w;
};
// w[i] = p_i(sigma) - y_i != q_i(sigma) (sigma - x_i)
__global__ void k_open_check_fin(OpenFin f) {
  const int i = threadIdx.x;
  if (i >= 4) return;
  uint32_t bad = 0;
  if (f.pi[i] >= 0) {
    Fr r = f.ev[f.pi[i]];
    if (f.qi[i] >= 0) r = r - *f.y[i] - f.ev[f.qi[i]] * f.d[i];
    bad = r.is_zero() ? 0u : 1u;
  }
  f.w[i] = bad;
}

// queue the check of up to four quotients; d_w receives four words (nonzero:
// failed).  Equal (p, pn) are evaluated once.
static void open_check_queue(qg_ctx* ctx, const OpenCk ck[4], uint32_t* d_w) {
  QgTimed tm(ctx, "kzg_open_check");
  const Fr sigma = ctx->open_sigma;
  std::vector<EvIn> in;
  OpenFin f{};
  for (int i = 0; i < 4; i++) {
    f.pi[i] = f.qi[i] = -1;
    if (!ck[i].p) continue;
    for (int k = 0; k < i; k++)
      if (ck[k].p == ck[i].p && ck[k].pn == ck[i].pn) f.pi[i] = f.pi[k];
    if (f.pi[i] < 0) {
      f.pi[i] = (int)in.size();
      in.push_back({ck[i].p, ck[i].pn, 0});
    }
    if (!ck[i].q) continue;
    f.qi[i] = (int)in.size();
    in.push_back({ck[i].q, ck[i].qn, 0});
    f.y[i] = ck[i].d_y;
    f.d[i] = sigma - ck[i].x;
  }
  Fr* d_ev = ctx->scratch_as<Fr>("open_ck_ev", 8);
  if (!in.empty()) poly_eval_queue(ctx, in, {sigma}, d_ev);
  f.ev = d_ev;
  f.w = d_w;
  hipLaunchKernelGGL(k_open_check_fin, dim3(1), dim3(64), 0, ctx->stream, f);
  QG_LAUNCH_CHECK();
}

static const char* const OPEN_QNAME[4] = {"poly at r", "poly at 1/r", "S at r", "S at 1/r"};
static const char* const OPEN_UNAME[1] = {"univariate"};

// after the path's synchronization: count, and raise on the first failed word
// (bad[per k + i]: quotient i of opening k, `per` quotients per opening, named
// qname[i]; checked[.]: CK_QUOT it had a quotient - counted in open_checks -,
// CK_ZERO its trimmed length was 0 and p(sigma) == 0 was checked, 0 nothing).
// A failed call leaves no trimmed length remembered.
enum : uint8_t { CK_NONE = 0, CK_QUOT = 1, CK_ZERO = 2 };
static void open_check_settle(qg_ctx* ctx, const std::vector<uint32_t>& bad,
                              const std::vector<uint8_t>& checked, size_t per,
                              const char* const* qname) {
  size_t first = bad.size(), nbad = 0;
  for (size_t j = 0; j < bad.size(); j++) {
    if (!checked[j]) continue;
    if (checked[j] == CK_QUOT) ctx->open_checks++;
    if (bad[j]) {
      nbad++;
      if (first == bad.size()) first = j;
    }
  }
  if (!nbad) return;
  ctx->open_check_failures += nbad;
  ctx->arena.memo["mle_poly_len"].clear();
  QG_CHECK(false, QG_ERR_ASSERT,
           "Polynomial division failed: opening " + std::to_string(first / per) + " of " +
               std::to_string(bad.size() / per) + ", quotient " + std::to_string(first % per) +
               " (" + qname[first % per] + ")");
}

// host form of the decision (sharded paths: the ranks' partial values summed)
static bool open_check_host(const Fr& P, const Fr& y, const Fr& Q, const Fr& sigma, const Fr& x) {
  return !(P - y - Q * (sigma - x)).is_zero();
}

// ---- test-only faults (qg_debug_open_fault): consumed by the first site of
// their kind in the opening call that follows the arming
static size_t fault_short_trim(qg_ctx* ctx, size_t len) {
  if (ctx->open_fault_live != 1 || len == 0) return len;
  ctx->open_fault_live = 0;
  return len > ctx->open_fault_value ? len - (size_t)ctx->open_fault_value : 1;
}
__global__ void k_fault_add_one(Fr* q) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *q = *q + Fr::one();
}
static void fault_quotient(qg_ctx* ctx, Fr* q, size_t len) {
  if (ctx->open_fault_live != 2 || len == 0) return;
  ctx->open_fault_live = 0;
  hipLaunchKernelGGL(k_fault_add_one, dim3(1), dim3(64), 0, ctx->stream,
                     q + (size_t)(ctx->open_fault_value % len));
  QG_LAUNCH_CHECK();
}
// the first nonzero of cnt device lengths, shortened (batched sharded path)
__global__ void k_fault_short_len(unsigned long long* len, size_t cnt, unsigned long long by) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (size_t i = 0; i < cnt; i++)
    if (len[i]) {
      len[i] = len[i] > by ? len[i] - by : 1;
      return;
    }
}

// ---------------------------------------------------------------- NTT
// Radix-2 NTT passes of up to 10 stages each on LDS tiles of 1024 elements
// held as 9 x 29-bit limbs (SoA: conflict-free), so a 2^24-point transform is
// three HBM round trips instead of one per stage.  A pass over stages
// [s0, s0 + B) works on tiles of 2^B "mid" indices x L consecutive "lo"
// indices (L = 1024 / 2^B): element (mid, l) is index
//   hi 2^(s0+B) + mid 2^s0 + lo0 + l,
// so every global access is a run of L consecutive Fr (L >= 8 above the first
// pass).  36 KB tiles let four blocks share a CU (16 waves; the 2048-element
// 72 KB tiles fit two: S polynomial at 2^23 -5 %, profiles/r04_ntt_tile_ab.txt).  Forward: DIF (natural in, bit-reversed out); inverse: DIT
// (bit-reversed in, natural out) -- no bit-reversal pass at all.  Data stay in
// arkworks form (x 2^256): twiddles are stored as w^k 2^261, so mul29 keeps the
// scale.  Every value is < 2p inside a pass, canonical (< p) when stored.
#ifndef QG_NTT_LGT
#define QG_NTT_LGT 10
#endif
static constexpr int NTT_LGT = QG_NTT_LGT;
static constexpr int NTT_T = 1 << NTT_LGT;  // elements per tile
#ifndef QG_NTT_THREADS
#define QG_NTT_THREADS 256
#endif
static constexpr int NTT_THREADS = QG_NTT_THREADS;
using R29 = F29<FrP>;

struct NttPass {
  int s0, B, lgL;
};

// stage ranges: [0, min(10, logn)) first (contiguous tiles), then chunks of at
// most 7 stages (runs of >= 8 elements)
static std::vector<NttPass> ntt_plan(int logn) {
  std::vector<NttPass> v;
  int s = 0;
  while (s < logn) {
    const int B = std::min(s == 0 ? NTT_LGT : 7, logn - s);
    int lgL = std::min(NTT_LGT - B, s);  // L <= 2^s0 (lo range)
    lgL = std::min(lgL, logn - B);       // tile <= n
    v.push_back({s, B, lgL});
    s += B;
  }
  return v;
}

QG_DEV R29 lds_get29(const uint32_t* sh, int e) {
  R29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = sh[i * NTT_T + e];
  return r;
}
QG_DEV void lds_put29(uint32_t* sh, int e, const R29& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) sh[i * NTT_T + e] = v.l[i];
}

// Twiddles by stage ("pyramid"): stage s's butterflies use w^(j 2^(logn-1-s))
// for j < 2^s, stored contiguously at pyr[2^s - 1 + j] (2^logn - 1 entries,
// twice the flat table).  Neighbouring butterflies of a stage have
// neighbouring j, so a wave's twiddle loads are runs of consecutive 32-B
// entries instead of one cache line per lane (the flat table's stride is
// 2^(logn-1-s) entries).  Built once per (table, logn) from the flat powers.
__global__ void k_tw_pyramid(const Fr* __restrict__ flat, int logn, Fr* __restrict__ pyr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << logn;
  if (i + 1 >= n) return;
  const int st = 63 - __clzll((unsigned long long)(i + 1));  // stage of entry i
  const size_t j = i + 1 - ((size_t)1 << st);
  pyr[i] = flat[j << (logn - 1 - st)];
}

// DIF (forward) or DIT (inverse) stages [s0, s0+B) on every tile.
//   in:  n entries (entries >= nin read as zero)
//   out: n entries, or only indices [win_lo, win_hi) written to out - win_lo
//   tw:  w^k 2^261 (Fr words) as the stage pyramid (pyr != 0) or flat, k < n/2
template <bool DIF>
__global__ void __launch_bounds__(NTT_THREADS)
    k_ntt_pass(const Fr* __restrict__ in, size_t nin, Fr* __restrict__ out,
               const Fr* __restrict__ tw, int pyr, int logn, int s0, int B, int lgL,
               size_t win_lo, size_t win_hi) {
  __shared__ uint32_t sh[9 * NTT_T];
  const int lgT = B + lgL, T = 1 << lgT;
  const int L = 1 << lgL;
  const size_t tid = threadIdx.x;
  // tile id -> (hi, lo group)
  const size_t ngroups = ((size_t)1 << s0) >> lgL;
  const size_t hi = blockIdx.x / ngroups, lo0 = (blockIdx.x % ngroups) << lgL;
  const size_t base = (hi << (s0 + B)) + lo0;
  for (int e = (int)tid; e < T; e += NTT_THREADS) {
    const size_t i = base + ((size_t)(e >> lgL) << s0) + (e & (L - 1));
    R29 v = R29::zero();
    if (i < nin) v = to29(in[i]);
    lds_put29(sh, e, v);
  }
  __syncthreads();
  for (int k = 0; k < B; k++) {
    const int b = DIF ? B - 1 - k : k;  // mid bit of this stage
    const int s = s0 + b;
    // butterflies p and p + NTT_THREADS together: their two Montgomery products
    // run as interleaved chains (mul29t2); a lone last one alone
    for (int p0 = (int)tid; p0 < T / 2; p0 += 2 * NTT_THREADS) {
      const bool two = p0 + NTT_THREADS < T / 2;
      int e0[2], e1[2];
      R29 u[2], v[2], w[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int p = h && two ? p0 + NTT_THREADS : p0;
        const int l = p & (L - 1), q = p >> lgL;
        const int mid0 = ((q >> b) << (b + 1)) | (q & ((1 << b) - 1));
        e0[h] = (mid0 << lgL) | l;
        e1[h] = e0[h] | (1 << (b + lgL));
        const size_t j = ((size_t)(mid0 & ((1 << b) - 1)) << s0) + lo0 + l;  // i0 mod 2^s
        w[h] = to29(tw[pyr ? ((size_t)1 << s) - 1 + j : j << (logn - 1 - s)]);
        u[h] = lds_get29(sh, e0[h]);
        v[h] = lds_get29(sh, e1[h]);
      }
      R29 t[2];
      if (DIF) {
        mul29t2(sub29(u[0], v[0]), w[0], sub29(u[1], v[1]), w[1], t[0], t[1]);
      } else {
        mul29t2(v[0], w[0], v[1], w[1], t[0], t[1]);
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (h && !two) break;
        if (DIF) {
          lds_put29(sh, e0[h], red2p29(add29(u[h], v[h])));
          lds_put29(sh, e1[h], t[h]);
        } else {
          lds_put29(sh, e0[h], red2p29(add29(u[h], t[h])));
          // u + 2p - t in [0, 4p) (u, t < 2p): one conditional subtraction
          lds_put29(sh, e1[h], red2p29(subk29(u[h], t[h], F29P<FrP>::K2)));
        }
      }
    }
    __syncthreads();
  }
  for (int e = (int)tid; e < T; e += NTT_THREADS) {
    const size_t i = base + ((size_t)(e >> lgL) << s0) + (e & (L - 1));
    if (i >= win_lo && i < win_hi) out[i - win_lo] = from29(canon29(lds_get29(sh, e)));
  }
}

// the stage pyramid of the flat twiddle table in scratch slot `src` (one
// derived slot per source slot; valid for the source's current build stamp and
// its own allocation generation, never for an address)
static const Fr* ntt_pyramid(qg_ctx* ctx, const Fr* flat, const std::string& src, int logn) {
  const std::string tag = "ntt_pyr:" + src;
  const size_t n = (size_t)1 << logn;
  Fr* pyr = ctx->scratch_as<Fr>(tag, std::max<size_t>(1, n - 1));
  const uint64_t st = ctx->arena.stamp(src);
  const std::string key = ctx->arena.derived_key(std::to_string(logn), st, ctx->scratch_gen(tag));
  if (!ctx->arena.check(tag, key, st)) {
    hipLaunchKernelGGL(k_tw_pyramid, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, flat, logn,
                       pyr);
    QG_LAUNCH_CHECK();
    ctx->arena.commit(tag, key);
  }
  return pyr;
}

// runs every pass in place on `a` (the first pass reads `in`), direction by DIF
static void ntt_run(qg_ctx* ctx, bool dif, const Fr* in, size_t nin, Fr* a, const Fr* tw,
                    const std::string& tw_slot, int logn, size_t win_lo, size_t win_hi,
                    Fr* win_out) {
  // QG_NTT_FLAT=1: twiddles from the flat table (A/B runs)
  static const bool flat = [] {
    const char* e = getenv("QG_NTT_FLAT");
    return e && atoi(e) != 0;
  }();
  const Fr* pyr = flat ? tw : ntt_pyramid(ctx, tw, tw_slot, logn);
  const int pmode = flat ? 0 : 1;
  std::vector<NttPass> plan = ntt_plan(logn);
  if (dif) std::reverse(plan.begin(), plan.end());
  const size_t n = (size_t)1 << logn;
  for (size_t k = 0; k < plan.size(); k++) {
    const NttPass& P = plan[k];
    const bool last = k + 1 == plan.size();
    const Fr* src = k == 0 ? in : a;
    const size_t ns = k == 0 ? nin : n;
    Fr* dst = last && win_out ? win_out : a;
    const size_t lo = last && win_out ? win_lo : 0, hi = last && win_out ? win_hi : n;
    const unsigned blocks = (unsigned)(n >> (P.B + P.lgL));
    if (dif)
      hipLaunchKernelGGL(k_ntt_pass<true>, dim3(blocks), dim3(NTT_THREADS), 0, ctx->stream, src, ns,
                         dst, pyr, pmode, logn, P.s0, P.B, P.lgL, lo, hi);
    else
      hipLaunchKernelGGL(k_ntt_pass<false>, dim3(blocks), dim3(NTT_THREADS), 0, ctx->stream, src,
                         ns, dst, pyr, pmode, logn, P.s0, P.B, P.lgL, lo, hi);
    QG_LAUNCH_CHECK();
  }
}

// x 2^256 (arkworks) -> x 2^261 in place: mul29 by 2^266
__global__ void k_fr_to261(Fr* __restrict__ a, size_t n, L9 c) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = from29(canon29(mul29(to29(a[i]), R29::from_l9(c))));
}

// twM in the combine's order: out[k] = in[bitrev(k)] c 2^-261 (the table is
// built once per (logn, M); read in natural order by k_s_combine_br, its
// loads are coalesced instead of one line per lane)
__global__ void k_fr_to261_br(const Fr* __restrict__ in, int logn, L9 c, Fr* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ((size_t)1 << logn)) return;
  const size_t j = (size_t)(__brevll((unsigned long long)k) >> (64 - logn));
  out[k] = from29(canon29(mul29(to29(in[j]), R29::from_l9(c))));
}

// bit-reversed domain: H_br[k] = tw_k (F[j] G[-j] + F[-j] G[j]), j = bitrev(k);
// bitrev(-j) = k with every bit below k's top set bit flipped.  twMb[k] =
// twM[bitrev(k)] carries w^{j(M-1)} n^-1 2^266, so mul29 of the 2^251-scaled
// products lands in arkworks form with 1/n folded in.
__global__ void k_s_combine_br(const Fr* __restrict__ F, const Fr* __restrict__ G,
                               const Fr* __restrict__ twMb, int logn, Fr* __restrict__ H) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << logn;
  if (k >= n) return;
  size_t kn = 0;
  if (k) {
    const int hb = 63 - __clzll((unsigned long long)k);
    kn = k ^ (((size_t)1 << hb) - 1);
  }
  const R29 a = to29(F[k]), bb = to29(G[kn]), c = to29(F[kn]), d = to29(G[k]);
  const R29 v = red2p29(add29(mul29(a, bb), mul29(c, d)));
  H[k] = from29(canon29(mul29(v, to29(twMb[k]))));
}

// ---- the inverse transform at half size (round 6) ------------------------
// With P_j = F_j G_{-j} + F_{-j} G_j (P_{-j} = P_j) the S polynomial is
// S_k = p_{k+1} (k < M - 1) for p = IDFT_n(P): H_j = w^{j(M-1)} P_j / n only
// shifts p by M - 1, and p is even (p_{-d} = p_d).  Split p by parity
// (N2 = n / 2, w2 = w^2):
//   p_{2e}     = a_e / n,  a = IDFT_N2(A),  A_j = P_j + P_{j+N2}
//   p_{2e+1}   = b_e / n,  b = IDFT_N2(B),  B_j = (P_j - P_{j+N2}) w^{-j}
// A is even (A_{N2-j} = A_j), so a is even; B_{N2-j} = w2^j B_j, so
// b_{-e} = b_{e-1}.  One half-size inverse of D = A + B gives d = a + b, and
// d_e - d_{-e} = (a_e + b_e) - (a_e + b_{e-1}) = b_e - b_{e-1}: b is b_0 plus
// a prefix sum of d_e - d_{N2-e}, with b_0 = sum_j B_j, and a = d - b.  So the
// size-n inverse NTT becomes a size-n/2 one plus O(n) combine / scan passes.
// In the bit-reversed domain P_j and P_{j+N2} sit at 2t and 2t + 1
// (t = bitrev_{N2}(j)), and D_j is needed at position t of the half-size
// DIT's bit-reversed input: each thread makes one D from two adjacent P.
// twD[t] = w^{-bitrev(t)} n^-1 2^266, c1 = n^-1 2^266: mul29 of the 2^251-scaled
// values lands in arkworks form with 1/n folded in (as twM does).
// bpart[block] = the block's sum of B_j / n (for b_0).
__global__ void __launch_bounds__(256)
    k_s_combine_half(const Fr* __restrict__ F, const Fr* __restrict__ G, const Fr* __restrict__ twD,
                     L9 c1, int logn, Fr* __restrict__ D, Fr* __restrict__ bpart) {
  __shared__ Fr red[256];
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t N2 = (size_t)1 << (logn - 1);
  Fr bn = Fr::zero();
  if (t < N2) {
    R29 P[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const size_t q = 2 * t + h;
      size_t kn = 0;
      if (q) {
        const int hb = 63 - __clzll((unsigned long long)q);
        kn = q ^ (((size_t)1 << hb) - 1);
      }
      const R29 a = to29(F[q]), bb = to29(G[kn]), c = to29(F[kn]), d = to29(G[q]);
      P[h] = red2p29(add29(mul29(a, bb), mul29(c, d)));  // < 2p, x 2^251
    }
    const R29 A = add29(P[0], P[1]);                                      // < 4p, lazy
    const R29 B = normfull29(subk29(P[0], P[1], F29P<FrP>::K2));          // < 4p, normalized
    const R29 An = mul29(A, R29::from_l9(c1));
    const R29 Bn = mul29(B, to29(twD[t]));
    D[t] = from29(canon29(red2p29(add29(An, Bn))));
    bn = from29(canon29(Bn));
  }
  red[threadIdx.x] = bn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) bpart[blockIdx.x] = red[0];
}

// out[0] = sum of in[0 .. n) (one block)
__global__ void __launch_bounds__(1024) k_fr_sum(const Fr* __restrict__ in, size_t n, Fr* __restrict__ out) {
  __shared__ Fr red[1024];
  Fr acc = Fr::zero();
  for (size_t i = threadIdx.x; i < n; i += 1024) acc = acc + in[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// b_e = b_0 + sum_{t=1..e} (d_t - d_{N2-t}), e = 0 .. E: tiles of SYM_TILE
// entries, a local inclusive prefix per tile (Q) and the tile totals (tot)
static constexpr int SYM_PER = 8;
static constexpr int SYM_TILE = 256 * SYM_PER;
__global__ void __launch_bounds__(256)
    k_sym_tiles(const Fr* __restrict__ d, size_t N2, size_t E, Fr* __restrict__ Q, Fr* __restrict__ tot) {
  __shared__ Fr sh[256];
  const size_t e0 = (size_t)blockIdx.x * SYM_TILE + (size_t)threadIdx.x * SYM_PER;
  Fr v[SYM_PER];
  Fr run = Fr::zero();
#pragma unroll
  for (int k = 0; k < SYM_PER; k++) {
    const size_t e = e0 + k;
    Fr dl = Fr::zero();
    if (e >= 1 && e <= E) dl = d[e] - d[N2 - e];
    run = run + dl;
    v[k] = run;
  }
  sh[threadIdx.x] = run;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele inclusive scan of the thread totals
    const Fr add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : Fr::zero();
    __syncthreads();
    sh[threadIdx.x] = sh[threadIdx.x] + add;
    __syncthreads();
  }
  const Fr before = threadIdx.x ? sh[threadIdx.x - 1] : Fr::zero();
#pragma unroll
  for (int k = 0; k < SYM_PER; k++)
    if (e0 + k <= E) Q[e0 + k] = before + v[k];
  if (threadIdx.x == 255) tot[blockIdx.x] = sh[255];
}

// tot[i] <- b_0 + sum_{i' < i} tot[i'] (one block)
__global__ void __launch_bounds__(1024) k_sym_top(Fr* __restrict__ tot, int ntiles, const Fr* __restrict__ b0) {
  __shared__ Fr sh[1024];
  const int per = (ntiles + 1023) / 1024;
  const int base = threadIdx.x * per;
  Fr sum = Fr::zero();
  for (int k = 0; k < per; k++)
    if (base + k < ntiles) sum = sum + tot[base + k];
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const Fr add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : Fr::zero();
    __syncthreads();
    sh[threadIdx.x] = sh[threadIdx.x] + add;
    __syncthreads();
  }
  Fr run = b0[0] + (threadIdx.x ? sh[threadIdx.x - 1] : Fr::zero());
  for (int k = 0; k < per; k++)
    if (base + k < ntiles) {
      const Fr t = tot[base + k];
      tot[base + k] = run;
      run = run + t;
    }
}

// S_{2e-1} = p_{2e} = d_e - b_e (e >= 1), S_{2e} = p_{2e+1} = b_e, for the
// k = 2e - 1, 2e below M - 1
__global__ void k_sym_out(const Fr* __restrict__ d, const Fr* __restrict__ Q, const Fr* __restrict__ tot,
                          size_t M, size_t E, Fr* __restrict__ S) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > E) return;
  const Fr b = tot[e / SYM_TILE] + Q[e];
  if (2 * e + 2 <= M) S[2 * e] = b;                   // k = 2e <= M - 2
  if (e >= 1 && 2 * e + 1 <= M) S[2 * e - 1] = d[e] - b;  // k = 2e - 1 <= M - 2
}

__global__ void k_powers_ml(Fr base, size_t n, int K, Fr* out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t i0 = t * (size_t)K;
  if (i0 >= n) return;
  Fr x = fpow_small(base, (uint64_t)i0);
  for (int j = 0; j < K && i0 + j < n; j++) {
    out[i0 + j] = x;
    x = x * base;
  }
}

// host-side 256-bit exponent power
static Fr fr_pow_big(Fr a, const uint32_t e[8]) {
  Fr r = Fr::one();
  for (int i = 7; i >= 0; i--)
    for (int b = 31; b >= 0; b--) {
      r = fsqr(r);
      if ((e[i] >> b) & 1u) r = r * a;
    }
  return r;
}

// primitive 2^logn-th root of unity: 5^((r-1)/2^logn)
static Fr root_of_unity(int logn) {
  uint32_t e[8];
  for (int i = 0; i < 8; i++) e[i] = FrP::P[i];
  e[0] -= 1;  // r - 1 (low limb of r is odd)
  for (int k = 0; k < logn; k++) {  // shift right by logn
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? (e[i + 1] << 31) : 0u);
  }
  return fr_pow_big(from_u64<FrP>(5), e);
}

// plain-integer product x y mod r (host)
static Fr ml_plain_mul(const Fr& x, const Fr& y) { return from_mont(to_mont(x) * to_mont(y)); }

// twiddle tables w^k 2^261 (k < n/2) for w = root_of_unity(logn) and its
// inverse in scratch slots `tag` and `tag`+"i", cached per transform size and
// allocation generation; every build stamps both slots, which invalidates the
// tables derived from them (ntt_pyramid, ntt_tw_bitrev)
static void ntt_twiddles(qg_ctx* ctx, int logn, Fr** tw, Fr** twi,
                         const std::string& tag = "ntt_tw") {
  const size_t n = (size_t)1 << logn, h = std::max<size_t>(n / 2, 1);
  *tw = ctx->scratch_as<Fr>(tag, h);
  *twi = ctx->scratch_as<Fr>(tag + "i", h);
  const std::string key = std::to_string(logn) + "|g" + std::to_string(ctx->scratch_gen(tag)) +
                          "," + std::to_string(ctx->scratch_gen(tag + "i"));
  if (ctx->arena.check(tag, key)) return;
  const Fr w = root_of_unity(logn), wi = finv(w);
  const int K = 64;
  const L9 c = F29P<FrP>::TO261;
  hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(h, K), 256)), dim3(256), 0, ctx->stream, w, h,
                     K, *tw);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(h, K), 256)), dim3(256), 0, ctx->stream, wi,
                     h, K, *twi);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fr_to261, dim3(div_up(h, 256)), dim3(256), 0, ctx->stream, *tw, h, c);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fr_to261, dim3(div_up(h, 256)), dim3(256), 0, ctx->stream, *twi, h, c);
  QG_LAUNCH_CHECK();
  ctx->arena.bump(tag);
  ctx->arena.bump(tag + "i");
  ctx->arena.commit(tag, key);
}

// Transform of the eq table without an NTT.  g = eq(., z) over nz variables is
// the coefficient vector of G(X) = prod_t ((1 - z_t) + z_t X^(2^t)), so
//   G(w^j) = Q_0(j),  Q_t(j) = ((1 - z_t) + z_t w^(j 2^t)) Q_{t+1}(j),  Q_nz = 1,
// where Q_t depends only on j mod 2^(L-t).  In the bit-reversed order of the
// DIF outputs (k' = bitrev_{L-t}(j mod 2^(L-t))) the recursion is streaming:
//   Q_t[k'] = f_t(k') Q_{t+1}[k' >> 1].
// One level per launch, 2^(L-t) entries; ~2 multiplies per entry over all
// levels (~4 x 2^L in total) instead of L/2 per entry of a forward NTT.
// Q is kept in arkworks form (x 2^256), the factor in the 2^261 domain.
// With twb = the flat table in bit-reversed order (twb[i] = tw[bitrev_{L-1}(i)]),
// level t's twiddle w^(bitrev_{L-t}(k) 2^t) is twb[k >> 1], negated for odd k
// (the top bit of the exponent is k's low bit, w^(2^(L-1)) = -1): consecutive
// entries read consecutive table words instead of one cache line per lane.
__global__ void k_eqdft_level(const Fr* __restrict__ qnext, L9 a261, L9 z261,
                              const Fr* __restrict__ twb, int logn, int t, Fr* __restrict__ q) {
  const size_t len = (size_t)1 << (logn - t);
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= len) return;
  R29 w = to29(twb[k >> 1]);
  if (k & 1) w = sub29(R29::zero(), w);  // lazy 4p - w
  // a261 < p (host-canonical), the product < 2p: one conditional subtraction
  const R29 f = red2p29(add29(R29::from_l9(a261), mul29(R29::from_l9(z261), w)));
  const R29 qn = qnext ? to29(qnext[k >> 1]) : to29(Fr::one());
  q[k] = from29(canon29(mul29(f, qn)));
}

// The small top levels of the same recursion in ONE launch (they were ~5 us
// launches of a few thousand entries each): level tmin's entry k is
//   Q_tmin[k] = prod_{t = tmin}^{nz-1} f_t(k >> (t - tmin)),
// every factor from the same bit-reversed table (twb[k' >> 1], negated for odd
// k'), two factors per step as interleaved products.  A thread per entry of
// level tmin (2^(logn - tmin) <= EQ_TOP_LEN entries).
static constexpr int EQ_TOP_MAXL = 32;
static constexpr int EQ_TOP_LOG = 16;  // levels of <= 2^16 entries are fused
struct EqTopConsts {
  L9 a[EQ_TOP_MAXL], z[EQ_TOP_MAXL];  // level tmin + i: (1 - z_t), z_t in the 2^261 domain
};
__global__ void __launch_bounds__(256)
    k_eqdft_top(EqTopConsts cs, uint32_t nlev, const Fr* __restrict__ twb, int logn, int tmin,
                Fr* __restrict__ q) {
  const size_t len = (size_t)1 << (logn - tmin);
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= len) return;
  R29 acc = to29(Fr::one());
  for (uint32_t i = 0; i < nlev; i++) {
    const size_t kk = k >> i;
    R29 w = to29(twb[kk >> 1]);
    if (kk & 1) w = sub29(R29::zero(), w);  // lazy 4p - w
    // a < p (host-canonical), the product < 2p: one conditional subtraction
    const R29 f = red2p29(add29(R29::from_l9(cs.a[i]), mul29(R29::from_l9(cs.z[i]), w)));
    acc = mul29(f, acc);  // arkworks form (x 2^256) kept: f carries 2^261
  }
  q[k] = from29(canon29(acc));
}

// twb[i] = tw[bitrev_{L-1}(i)] for i < 2^(L-1) (one entry for L <= 1)
__global__ void k_tw_bitrev(const Fr* __restrict__ tw, int logn, size_t h, Fr* __restrict__ twb) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h) return;
  const size_t j = logn > 1 ? (size_t)(__brevll((unsigned long long)i) >> (65 - logn)) : 0;
  twb[i] = tw[j];
}

// the flat twiddle table of scratch slot `src` in bit-reversed order (keyed
// like ntt_pyramid)
static const Fr* ntt_tw_bitrev(qg_ctx* ctx, const Fr* tw, const std::string& src, int logn) {
  const std::string tag = "ntt_twb:" + src;
  const size_t h = logn > 1 ? (size_t)1 << (logn - 1) : 1;
  Fr* twb = ctx->scratch_as<Fr>(tag, h);
  const uint64_t st = ctx->arena.stamp(src);
  const std::string key = ctx->arena.derived_key(std::to_string(logn), st, ctx->scratch_gen(tag));
  if (!ctx->arena.check(tag, key, st)) {
    hipLaunchKernelGGL(k_tw_bitrev, dim3(div_up(h, 256)), dim3(256), 0, ctx->stream, tw, logn, h,
                       twb);
    QG_LAUNCH_CHECK();
    ctx->arena.commit(tag, key);
  }
  return twb;
}

static L9 l9_of29(const Fr& x) {
  const R29 t = to29(x);
  L9 c{};
  for (int i = 0; i < 9; i++) c.v[i] = t.l[i];
  return c;
}

// S polynomial (M - 1 coefficients, untrimmed) of f (nf) and g (ng), device in/out.
// eq_z (nz variables, host Montgomery): g is eq(., eq_z) over 2^nz entries, and
// its transform comes from the product formula (k_eqdft_level) instead of an NTT.
// f_id: the allocation id of the qg_buf behind f (qg_buf::alloc_id, never
// reused; 0 = unknown).  reuse_f: the caller guarantees f's contents are
// unchanged since the last call that transformed this same buffer; F is then
// reused when this context still holds that transform (arena memo "ntt_F_src":
// f's allocation id and offset, length, size, and the generation of F's slot).
static void s_poly_device(qg_ctx* ctx, const Fr* f, size_t nf, const Fr* g, size_t ng, Fr* S,
                          const uint64_t* eq_z = nullptr, size_t nz = 0, bool reuse_f = false,
                          uint64_t f_id = 0, size_t f_off = 0) {
  const size_t M = nf > ng ? nf : ng;
  if (M <= 1) return;
  QgTimed tm(ctx, "s_polynomial");
  int logn = 0;
  while (((size_t)1 << logn) < 2 * M - 1) logn++;
  QG_CHECK(logn <= 28, QG_ERR_UNSUPPORTED, "S-polynomial NTT beyond 2-adicity");
  if (logn < 1) logn = 1;
  const size_t n = (size_t)1 << logn;
  Fr* F = ctx->scratch_as<Fr>("ntt_F", n);
  Fr* G = ctx->scratch_as<Fr>("ntt_G", n);
  Fr* H = ctx->scratch_as<Fr>("ntt_H", n);
  // w^{j(M-1)} n^-1 2^266 for j < n: powers of w^{M-1} (x 2^256, staged in H),
  // then x n^-1 2^271 via mul29 into twM in bit-reversed order.  Depends on
  // (logn, M) only: cached per context in one of four slots by (logn, M), so a
  // prover alternating between a few opening sizes (HyperPlonk: the witness
  // and its public rows) does not rebuild it per opening.
  // QG_S_FULL_INVERSE=1: the size-n inverse (k_s_combine_br + DIT of H) instead
  // of the half-size one (A/B runs); read per call
  const char* fi = getenv("QG_S_FULL_INVERSE");
  const bool half_inverse = !(fi && atoi(fi) != 0);
  Fr *tw, *twi;
  ntt_twiddles(ctx, logn, &tw, &twi);
  Fr* twM = nullptr;
  Fr* twD = nullptr;
  if (half_inverse) {
    // w^{-j} n^-1 2^266 for j < n / 2 in bit-reversed order: depends on logn only
    twD = ctx->scratch_as<Fr>("ntt_twD", n / 2);
    const std::string memo = ctx->arena.derived_key(std::to_string(logn), 1, ctx->scratch_gen("ntt_twD"));
    if (!ctx->arena.check("ntt_twD", memo)) {
      const Fr wi = finv(root_of_unity(logn));
      const int K = 64;
      hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(n / 2, K), 256)), dim3(256), 0, ctx->stream,
                         wi, n / 2, K, H);
      QG_LAUNCH_CHECK();
      const Fr ninv_plain = from_mont(finv(from_u64<FrP>(n)));
      const L9 c9 = l9_of29(ml_plain_mul(ninv_plain, pow2_mod_plain<FrP>(271)));
      hipLaunchKernelGGL(k_fr_to261_br, dim3(div_up(n / 2, 256)), dim3(256), 0, ctx->stream, H,
                         logn - 1, c9, twD);
      QG_LAUNCH_CHECK();
      ctx->arena.commit("ntt_twD", memo);
    }
  }
  const std::string twm_key = std::to_string(logn) + ":" + std::to_string(M);
  bool twm_hit = false;  // the memo below decides; the LRU only picks the slot
  const std::string twm_slot =
      half_inverse ? std::string() : "ntt_twM#" + std::to_string(ctx->twm_lru.slot_for(twm_key, &twm_hit));
  if (!half_inverse) twM = ctx->scratch_as<Fr>(twm_slot, n);
  const std::string twm_memo =
      half_inverse ? std::string() : ctx->arena.derived_key(twm_key, 1, ctx->scratch_gen(twm_slot));
  if (!half_inverse && !ctx->arena.check(twm_slot, twm_memo)) {
    const Fr w = root_of_unity(logn);
    const Fr wM = fpow_small(w, (uint64_t)(M - 1));
    const int K = 64;
    hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(n, K), 256)), dim3(256), 0, ctx->stream, wM,
                       n, K, H);
    QG_LAUNCH_CHECK();
    const Fr ninv_plain = from_mont(finv(from_u64<FrP>(n)));
    const Fr cM = ml_plain_mul(ninv_plain, pow2_mod_plain<FrP>(271));
    L9 c9{};
    {
      const R29 t = to29(cM);
      for (int i = 0; i < 9; i++) c9.v[i] = t.l[i];
    }
    hipLaunchKernelGGL(k_fr_to261_br, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, H, logn, c9,
                       twM);
    QG_LAUNCH_CHECK();
    ctx->arena.commit(twm_slot, twm_memo);
  }
  // forward DIF of f and g (zero-extended), bit-reversed outputs
  const std::string fkey =
      f_id ? ctx->arena.derived_key(std::to_string(f_id) + "+" + std::to_string(f_off) + ":" +
                                        std::to_string(nf) + ":" + std::to_string(logn),
                                    ctx->arena.stamp("ntt_tw"), ctx->scratch_gen("ntt_F"))
           : std::string();
  if (!(reuse_f && f_id && ctx->arena.memo["ntt_F_src"] == fkey)) {
    ctx->arena.memo["ntt_F_src"].clear();
    ntt_run(ctx, true, f, nf, F, tw, "ntt_tw", logn, 0, 0, nullptr);
    ctx->arena.memo["ntt_F_src"] = fkey;
  }
  if (eq_z && nz >= 1 && ((size_t)1 << nz) == ng && (int)nz < logn) {
    // levels t = nz-1 .. 0 ping-pong between G and H (H is free until the combine),
    // ending in G (t = 0: 2^logn entries, bit-reversed order)
    const Fr* twb = ntt_tw_bitrev(ctx, tw, "ntt_tw", logn);
    // the levels of <= 2^EQ_TOP_LOG entries (t >= tmin) in one launch into the
    // array level tmin would have been written to, then one launch per level
    static const bool eq_top = [] {
      const char* e = getenv("QG_EQ_TOP");  // 0: one launch per level (A/B runs)
      return !(e && atoi(e) == 0);
    }();
    int t_hi = (int)nz - 1;  // highest level still to run per launch
    const int tmin = std::max(0, logn - EQ_TOP_LOG);
    if (eq_top && tmin < (int)nz && (int)nz - tmin <= EQ_TOP_MAXL) {
      EqTopConsts cs{};
      for (int t = tmin; t < (int)nz; t++) {
        const Fr z = fr_import(eq_z + 4 * t);
        const Fr zp = from_mont(z), ap = from_mont(Fr::one() - z);
        cs.z[t - tmin] = l9_of29(ml_plain_mul(zp, pow2_mod_plain<FrP>(261)));
        cs.a[t - tmin] = l9_of29(ml_plain_mul(ap, pow2_mod_plain<FrP>(261)));
      }
      Fr* dst = (tmin & 1) == 0 ? G : H;
      const size_t len = (size_t)1 << (logn - tmin);
      hipLaunchKernelGGL(k_eqdft_top, dim3(div_up(len, 256)), dim3(256), 0, ctx->stream, cs,
                         (uint32_t)(nz - tmin), twb, logn, tmin, dst);
      QG_LAUNCH_CHECK();
      t_hi = tmin - 1;
    }
    for (int t = t_hi; t >= 0; t--) {
      const Fr z = fr_import(eq_z + 4 * t);
      const Fr zp = from_mont(z), ap = from_mont(Fr::one() - z);
      const L9 z9 = l9_of29(ml_plain_mul(zp, pow2_mod_plain<FrP>(261)));
      const L9 a9 = l9_of29(ml_plain_mul(ap, pow2_mod_plain<FrP>(261)));
      Fr* dst = (t & 1) == 0 ? G : H;
      const Fr* src = t == (int)nz - 1 ? nullptr : ((t & 1) == 0 ? H : G);  // level t + 1
      const size_t len = (size_t)1 << (logn - t);
      hipLaunchKernelGGL(k_eqdft_level, dim3(div_up(len, 256)), dim3(256), 0, ctx->stream, src,
                         a9, z9, twb, logn, t, dst);
      QG_LAUNCH_CHECK();
    }
  } else {
    ntt_run(ctx, true, g, ng, G, tw, "ntt_tw", logn, 0, 0, nullptr);
  }
  if (!half_inverse) {
    hipLaunchKernelGGL(k_s_combine_br, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, F, G, twM,
                       logn, H);
    QG_LAUNCH_CHECK();
    // inverse DIT of H (bit-reversed in, natural out); the last pass writes only
    // h[M .. 2M-1) = S
    ntt_run(ctx, false, H, n, H, twi, "ntt_twi", logn, M, 2 * M - 1, S);
    return;
  }
  // the inverse at half size (k_s_combine_half): D into H's first half,
  // the half-size DIT in place, then b by a prefix scan into S
  const size_t N2 = n / 2;
  const unsigned cblocks = div_up(N2, 256);
  Fr* bpart = ctx->scratch_as<Fr>("s_bpart", (size_t)cblocks + 1);
  const Fr ninv_plain = from_mont(finv(from_u64<FrP>(n)));
  const L9 c1 = l9_of29(ml_plain_mul(ninv_plain, pow2_mod_plain<FrP>(266)));
  hipLaunchKernelGGL(k_s_combine_half, dim3(cblocks), dim3(256), 0, ctx->stream, F, G, twD, c1, logn,
                     H, bpart);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fr_sum, dim3(1), dim3(1024), 0, ctx->stream, bpart, (size_t)cblocks,
                     bpart + cblocks);
  QG_LAUNCH_CHECK();
  Fr *twh, *twhi;
  ntt_twiddles(ctx, logn - 1, &twh, &twhi, "ntt_twh");
  ntt_run(ctx, false, H, N2, H, twhi, "ntt_twhi", logn - 1, 0, 0, nullptr);
  const size_t E = (M - 1) / 2;  // b_e, a_e for e <= E cover S_0 .. S_{M-2}
  const size_t ntiles = E / SYM_TILE + 1;
  QG_CHECK(ntiles <= 1024 * 64, QG_ERR_UNSUPPORTED, "S-polynomial scan too large");
  Fr* tot = ctx->scratch_as<Fr>("s_symtot", ntiles);
  hipLaunchKernelGGL(k_sym_tiles, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, H, N2, E, G, tot);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sym_top, dim3(1), dim3(1024), 0, ctx->stream, tot, (int)ntiles,
                     bpart + cblocks);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sym_out, dim3(div_up(E + 1, 256)), dim3(256), 0, ctx->stream, H, G, tot, M, E,
                     S);
  QG_LAUNCH_CHECK();
}

// highest nonzero index + 1: per-thread max over a grid-stride range of
// [lo, hi), wave max by shuffles, one atomic per wave (a contended atomic per
// element cost 0.75 ms at 2^22) into *out.  The tail launch (the last 16K
// entries) also posts its max into *tail, which trim_launch zeroed in stream
// order just before it; the body launch skips a block when *tail is nonzero:
// the tail covered the higher indices, so any body index is below the
// answer (a full body scan at 2^23 is 110 us; most vectors end in a nonzero
// value).
//
// Round 6: the skip used to read *out itself, which the body launch's own
// blocks write: a block that started after another block of the same launch
// had posted its maximum exited without scanning its range, so the length
// came out short (81152 or 81664 instead of 81920 for HyperPlonk's trimmed
// full witness at 2^14 rows, whose tail is zero) whenever the launch's blocks
// did not all start before the first one finished - timing-dependent, seen
// with the MSM batches' side streams active (micro/handover_dbg.py,
// profiles/r06_handover_diagnosis.txt).  A short length gives a wrong
// quotient, so a wrong KZG opening proof; no opening proof enters the
// transcript, so only a verifier or a proof-by-proof comparison sees it.
__global__ void __launch_bounds__(256)
    k_last_nonzero(const Fr* __restrict__ a, size_t lo, size_t hi, unsigned long long* tail,
                   int body, unsigned long long* out) {
  if (body) {
    if (__hip_atomic_load(tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  }
  unsigned long long m = 0;
  for (size_t i = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi;
       i += (size_t)gridDim.x * blockDim.x)
    if (!a[i].is_zero()) m = i + 1;
  for (int k = 32; k > 0; k >>= 1) {
    const unsigned long long o = __shfl_xor(m, k, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) {
    atomicMax(out, m);
    if (!body) atomicMax(tail, m);
  }
}

// trimmed length of a device vector: the last 16K entries first (8 blocks),
// then the rest, skipped when the tail held a nonzero
static void trim_launch(qg_ctx* ctx, const Fr* a, size_t n, unsigned long long* d) {
  QG_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream));
  if (n == 0) return;
  constexpr size_t TAIL = 16384;
  const size_t body = n > TAIL ? n - TAIL : 0;
  // one stamp word per context, reused in stream order: zeroed before every
  // tail launch, which alone writes it (the largest nonzero index + 1 it saw),
  // so the body launch reads this call's tail result and nothing else - no
  // generation to collide or wrap, and no dependence on what the word held
  // when it was allocated
  unsigned long long* tail = ctx->scratch_as<unsigned long long>("trim_tail", 1);
  if (body) QG_HIP(hipMemsetAsync(tail, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_last_nonzero, dim3((unsigned)std::min<size_t>(8, div_up(n - body, 256))),
                     dim3(256), 0, ctx->stream, a, body, n, tail, 0, d);
  QG_LAUNCH_CHECK();
  if (body) {
    const unsigned blocks = (unsigned)std::min<size_t>(2048, div_up(body, 256));
    hipLaunchKernelGGL(k_last_nonzero, dim3(blocks), dim3(256), 0, ctx->stream, a, (size_t)0,
                       body, tail, 1, d);
    QG_LAUNCH_CHECK();
  }
}

static size_t trimmed_len(qg_ctx* ctx, const Fr* a, size_t n) {
  if (n == 0) return 0;
  unsigned long long* d = ctx->scratch_as<unsigned long long>("trim_len", 1);
  trim_launch(ctx, a, n, d);
  unsigned long long h = 0;
  QG_HIP(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  return (size_t)h;
}

// ---------------------------------------------------------------- quotient stage
// The second half of every proof here: polynomials and points in, KZG::open
// quotients (kzg.rs:75-96), their values y, kzg.rs:85's check and one MSM
// batch out.  The jobs of both stages (single-context below, sharded further
// down) come in groups of `per` - one proof's openings: 4 for an ML opening
// (OPEN_QNAME), 6 for the inner-product argument (IPA_QNAME), 1 for a bare
// KZG::open - and inside a group in pairs: jobs 2p and 2p + 1 are one
// polynomial at two points (r, 1/r).  Scratch and pinned slots are named
// open_<what>, per-job ones open_<what>#<job index>, for every protocol.

// The scans of one group's nonempty jobs, in job order: groups of SH_J (an ML
// opening's four are one suffix_horner<1>), or, where the caller's jobs may
// pair and QG_IPA_PAIRED=1 (read per call, here only), each pair as one
// suffix_horner<2> job; the same bits either way.
static void quotient_scans(qg_ctx* ctx, const std::vector<ShIn<1>>& in, bool may_pair) {
  QgTimed tm(ctx, "kzg_division");
  const char* pe = may_pair ? getenv("QG_IPA_PAIRED") : nullptr;
  if (!(pe && atoi(pe) != 0)) return suffix_horner_many(ctx, in);
  std::vector<ShIn<2>> two;
  for (size_t i = 0; i + 1 < in.size(); i += 2)
    two.push_back({in[i].c, in[i].L, {in[i].x[0], in[i + 1].x[0]}, {in[i].s[0], in[i + 1].s[0]}});
  suffix_horner<2>(ctx, two);
}

// One KZG::open on a device polynomial p of n coefficients whose trimmed
// length is Lt (the caller's: DensePolynomial::from_coefficients_slice trims
// what KZG::open is given, kzg.rs:77), at x; `out` receives x, y and the proof.
struct QuotJob {
  const Fr* p;
  size_t n, Lt;
  Fr x;
  qg_kzg_opening* out;
};

// What quotients_queue leaves for after the caller's one MSM batch over
// (qs, qns) and its synchronization: the values y = s_0 and the check words
// in pinned memory, queued without a round trip.
struct QuotStage {
  size_t per = 1, wpg = 4;  // check words per group: open_check_queue's fours
  std::vector<qg_kzg_opening*> outs;
  std::vector<const Fr*> qs;  // q_i = s_{i+1}, i < Lt - 1 (kzg.rs:88-89)
  std::vector<size_t> qns;
  const Fr* h_y = nullptr;
  const uint32_t* h_w = nullptr;
  std::vector<uint8_t> checked;  // empty: QG_OPEN_CHECK=0

  void fit(const qg_srs* srs) const {
    for (size_t n : qns)
      QG_CHECK(n <= srs->n, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
  }
  // after the synchronization: count, and raise on the first failed quotient
  void settle(qg_ctx* ctx, const char* const* qname) const {
    if (checked.empty()) return;
    std::vector<uint32_t> bad(outs.size());
    for (size_t j = 0; j < bad.size(); j++) bad[j] = h_w[j / per * wpg + j % per];
    open_check_settle(ctx, bad, checked, per, qname);
  }
  void store(const std::vector<G1Affine>& pis) const {
    for (size_t j = 0; j < outs.size(); j++) {
      fr_export(h_y[j], outs[j]->y);
      g1_export(pis[j], outs[j]->proof_xy, &outs[j]->proof_inf);
    }
  }
};

// Queues, group by group: one batched suffix-Horner recursion over the
// trimmed lengths, the test fault, the values y into pinned memory, and the
// quotient check (open_check_queue's groups of four in job order, so equal
// (p, n) are evaluated once per four) over the UNtrimmed lengths: p over all n
// coefficients, q as the MSM will read it; a job trimmed to nothing has no
// quotient, y = 0, and all n coefficients must be 0.
static QuotStage quotients_queue(qg_ctx* ctx, const std::vector<QuotJob>& jobs, size_t per,
                                 bool may_pair = false) {
  const size_t J = jobs.size(), G = J / per;
  QuotStage st;
  st.per = per, st.wpg = 4 * div_up(per, (size_t)4);
  std::vector<Fr*> s(J, nullptr);
  size_t nmax = 0;
  for (size_t j = 0; j < J; j++) {
    fr_export(jobs[j].x, jobs[j].out->x);
    st.outs.push_back(jobs[j].out);
    nmax = std::max(nmax, jobs[j].n);
    if (jobs[j].Lt) s[j] = ctx->scratch_as<Fr>("open_s#" + std::to_string(j), jobs[j].Lt);
    st.qs.push_back(s[j] ? s[j] + 1 : nullptr);
    st.qns.push_back(s[j] ? jobs[j].Lt - 1 : 0);
  }
  Fr* d_y = ctx->scratch_as<Fr>("open_y", J);
  Fr* h_y = reinterpret_cast<Fr*>(ctx->pinned_get("open_y_h", J * sizeof(Fr)));
  const bool check = open_check_on();
  uint32_t* d_w = check ? ctx->scratch_as<uint32_t>("open_ck_w", G * st.wpg) : nullptr;
  uint32_t* h_w =
      reinterpret_cast<uint32_t*>(ctx->pinned_get("open_ck_h", G * st.wpg * sizeof(uint32_t)));
  // the evaluation's span scratch at its largest before anything is queued:
  // open_check_queue evaluates up to four p and four q at sigma
  if (check) poly_eval_reserve(ctx, 8, nmax, 1);
  if (check) st.checked.assign(J, CK_NONE);
  QG_HIP(hipMemsetAsync(d_y, 0, J * sizeof(Fr), ctx->stream));
  for (size_t g = 0; g < G; g++) {
    const size_t j0 = g * per;
    std::vector<ShIn<1>> in;
    for (size_t j = j0; j < j0 + per; j++)
      if (s[j]) in.push_back({jobs[j].p, jobs[j].Lt, {jobs[j].x}, {s[j]}});
    quotient_scans(ctx, in, may_pair);
    for (size_t j = j0; j < j0 + per; j++)
      if (s[j]) fault_quotient(ctx, s[j] + 1, jobs[j].Lt - 1);
    for (size_t j = j0; j < j0 + per; j++)
      if (s[j])
        QG_HIP(hipMemcpyAsync(d_y + j, s[j], sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    QG_HIP(hipMemcpyAsync(h_y + j0, d_y + j0, per * sizeof(Fr), hipMemcpyDeviceToHost,
                          ctx->stream));
    if (!check) continue;
    std::vector<OpenCk> ck(st.wpg);
    for (size_t j = j0; j < j0 + per; j++) {
      const QuotJob& q = jobs[j];
      ck[j - j0] = {q.n ? q.p : nullptr, q.n, st.qs[j], st.qns[j], d_y + j, q.x};
      st.checked[j] = s[j] ? CK_QUOT : q.n ? CK_ZERO : CK_NONE;
    }
    for (size_t c = 0; c < st.wpg; c += 4) open_check_queue(ctx, &ck[c], d_w + g * st.wpg + c);
    QG_HIP(hipMemcpyAsync(h_w + g * st.wpg, d_w + g * st.wpg, st.wpg * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, ctx->stream));
  }
  st.h_y = h_y, st.h_w = h_w;
  return st;
}

// KZG::open on a device polynomial; fills x, y, proof.  A stage of one job in
// this path's own order: the check settles before the degree is judged and
// the quotient committed.
static void kzg_open_device(qg_ctx* ctx, const qg_srs* srs, const Fr* c, size_t L, const Fr& x,
                            qg_kzg_opening* out) {
  const size_t Lt = fault_short_trim(ctx, trimmed_len(ctx, c, L));
  const QuotStage st = quotients_queue(ctx, {{c, L, Lt, x, out}}, 1);
  ctx->sync();
  st.settle(ctx, OPEN_UNAME);
  st.fit(srs);
  st.store(msm_device_batch(ctx, srs, st.qs, st.qns));
}

// ---------------------------------------------------------------- sharded opening
// Ranks hold contiguous slices [off, off + L) of a global coefficient vector.
// Suffix-Horner is linear in its carry: the global s_i on a slice equals the
// local scan plus x^(le - i) C, C = global s at the slice end.  C comes from
// one allgather of the per-rank local values T_r = s_local[0].

// s_i += x^(le - i) C for i < le; s_le = C   (pw[k] = x^k)
__global__ void k_sh_carry(Fr* __restrict__ s, size_t le, const Fr* __restrict__ pw, Fr C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < le) s[i] = s[i] + pw[le - i] * C;
  if (i == le) s[i] = C;
}

// small host values gathered over the communicator (rank order)
static void allgather_host(qg_ctx* ctx, const void* src, size_t bytes, void* dst_all) {
  uint8_t* ds = ctx->scratch_as<uint8_t>("ag_send", bytes);
  uint8_t* dr = ctx->scratch_as<uint8_t>("ag_recv", bytes * (size_t)ctx->world);
  QG_HIP(hipMemcpyAsync(ds, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  comm_allgather_bytes(ctx, ds, dr, bytes);
  QG_HIP(hipMemcpyAsync(dst_all, dr, bytes * (size_t)ctx->world, hipMemcpyDeviceToHost,
                        ctx->stream));
  ctx->sync();
}

// One quotient of a sharded proof: this rank's slice p (L coefficients) of a
// polynomial whose global trimmed length is glt, at x.  glt and x are gathered
// or transcript values: the same on every rank.
struct ShardQuotJob {
  const Fr* p;
  size_t L, glt;
  Fr x;
  qg_kzg_opening* out;
};

// The quotient stage on a sharded context (groups and pairs as in
// quotients_queue), collective: the jobs' local suffix-Horner scans of this
// rank's live coefficients into s_j[0 .. le_j), T_j = s_j[0]; ONE allgather of
// every rank's T; the carries (x^(le - i) C) on the host and the device; the
// quotient check on the ranks' summed parts - per group p(sigma) of each pair
// over the untrimmed local slices, then every q(sigma): ONE allgather, after
// the carries, which need the first - around the quotient commitments as ONE
// sharded MSM batch; the export.  Returns the values y.  before_settle runs
// after the last synchronization and before a failed check leaves the call
// (the caller's scratch release).  The caller has judged the degrees
// (op_fits), on gathered values: nothing here ends the call on a value that
// differs between ranks.
static std::vector<Fr> quotients_sharded(qg_ctx* ctx, const qg_srs* srs,
                                         const std::vector<ShardQuotJob>& jobs, size_t per,
                                         bool may_pair, const char* const* qname,
                                         const std::function<void()>& before_settle = {}) {
  const size_t J = jobs.size(), G = J / per;
  const size_t W = (size_t)ctx->world, rank = (size_t)ctx->rank;
  std::vector<size_t> le(J);
  std::vector<Fr*> sq(J);
  size_t max_le = 0;
  for (size_t j = 0; j < J; j++) {
    le[j] = op_live(jobs[j].glt, rank, jobs[j].L);
    sq[j] = ctx->scratch_as<Fr>("open_s#" + std::to_string(j), le[j] + 1);
    max_le = std::max(max_le, le[j]);
  }
  Fr* d_T = ctx->scratch_as<Fr>("open_T", J);
  QG_HIP(hipMemsetAsync(d_T, 0, J * sizeof(Fr), ctx->stream));
  for (size_t g = 0; g < G; g++) {
    std::vector<ShIn<1>> in;
    for (size_t j = g * per; j < (g + 1) * per; j++)
      if (le[j]) in.push_back({jobs[j].p, le[j], {jobs[j].x}, {sq[j]}});
    quotient_scans(ctx, in, may_pair);
    for (size_t j = g * per; j < (g + 1) * per; j++)
      if (le[j])
        QG_HIP(hipMemcpyAsync(d_T + j, sq[j], sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
  }
  // exchange: every rank's T values
  Fr* d_Tall = ctx->scratch_as<Fr>("open_T_all", J * W);
  comm_allgather_bytes(ctx, d_T, d_Tall, J * sizeof(Fr));
  std::vector<Fr> Tall(J * W);
  QG_HIP(hipMemcpyAsync(Tall.data(), d_Tall, J * W * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  // C_rank = sum_{r' > rank} T_r' x^((r' - rank - 1) L);  y = sum_r T_r x^(r L)
  std::vector<Fr> ys(J);
  Fr* pw = ctx->scratch_as<Fr>("open_pw", max_le + 1);
  std::vector<const Fr*> qs(J);
  std::vector<size_t> qn(J);
  for (size_t j = 0; j < J; j++) {
    const Fr x = jobs[j].x, xL = fpow_small(x, jobs[j].L);
    Fr C = Fr::zero(), y = Fr::zero();
    for (size_t r = W; r-- > 0;) {
      if (r == rank) C = y;
      y = Tall[r * J + j] + xL * y;
    }
    ys[j] = y;
    if (le[j] > 0) {
      QgTimed tm(ctx, "kzg_division");
      const int KP = 64;
      hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(le[j] + 1, (size_t)KP), ML_BLOCK)),
                         dim3(ML_BLOCK), 0, ctx->stream, x, le[j] + 1, KP, pw);
      QG_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_sh_carry, dim3(div_up(le[j] + 1, ML_BLOCK)), dim3(ML_BLOCK), 0,
                         ctx->stream, sq[j], le[j], pw, C);
      QG_LAUNCH_CHECK();
    }
    // q_i = s_{i+1} for global i < glt - 1; this rank's part starts at s + 1
    qn[j] = op_qlive(jobs[j].glt, rank, jobs[j].L);
    qs[j] = sq[j] + 1;
    fault_quotient(ctx, sq[j] + 1, qn[j]);
  }
  // kzg.rs:85 on the ranks' summed parts; per group per / 2 + per values
  const bool check = open_check_on();
  const size_t E = G * (per / 2 + per);
  auto p_at = [&](size_t j) { return j / per * (per / 2 + per) + j % per / 2; };
  auto q_at = [&](size_t j) { return j / per * (per / 2 + per) + per / 2 + j % per; };
  Fr* d_ev = check ? ctx->scratch_as<Fr>("open_ck_ev_sh", E) : nullptr;
  if (check) {
    QgTimed tm(ctx, "kzg_open_check");
    std::vector<EvIn> in(E);
    for (size_t j = 0; j < J; j++) {
      const uint64_t off = (uint64_t)(rank * jobs[j].L);
      in[p_at(j)] = {jobs[j].p, jobs[j].L, off};
      in[q_at(j)] = {qs[j], qn[j], off};
    }
    poly_eval_queue(ctx, in, {ctx->open_sigma}, d_ev);
  }
  const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, qs, qn);
  std::vector<uint32_t> bad(J, 0);
  std::vector<uint8_t> checked(J, 0);
  if (check) {
    Fr* d_evall = ctx->scratch_as<Fr>("open_ck_ev_all", E * W);
    comm_allgather_bytes(ctx, d_ev, d_evall, E * sizeof(Fr));
    std::vector<Fr> ev(E * W);
    QG_HIP(hipMemcpyAsync(ev.data(), d_evall, ev.size() * sizeof(Fr), hipMemcpyDeviceToHost,
                          ctx->stream));
    ctx->sync();
    for (size_t j = 0; j < J; j++) {
      Fr P = Fr::zero(), Q = Fr::zero();
      for (size_t r = 0; r < W; r++) {
        P = P + ev[r * E + p_at(j)];
        Q = Q + ev[r * E + q_at(j)];
      }
      checked[j] = jobs[j].glt ? CK_QUOT : CK_ZERO;
      bad[j] = open_check_host(P, ys[j], Q, ctx->open_sigma, jobs[j].x);
    }
  }
  if (before_settle) before_settle();
  if (check) open_check_settle(ctx, bad, checked, per, qname);
  for (size_t j = 0; j < J; j++) {
    fr_export(jobs[j].x, jobs[j].out->x);
    fr_export(ys[j], jobs[j].out->y);
    g1_export(pis[j], jobs[j].out->proof_xy, &jobs[j].out->proof_inf);
  }
  return ys;
}

// ---------------------------------------------------------------- sharded S polynomial
// S = the window [M, 2M - 1) of h = IDFT_n(Hs), Hs[k] = w^{k(M-1)} / n (F[k] G[-k]
// + F[-k] G[k]) (the replicated s_poly_device, n = 2M), split over W ranks by
// frequency residue.  With k = k2 W + c and i = i1 B + i2 (B = n / W = 2L):
//   F[k2 W + c] = DFT_B(u_c)[k2],  u_c[i2] = w^{i2 c} sum_{i1 < W/2} w_W^{i1 c} f[i1 B + i2]
//   h[i1 B + i2] = sum_c w_W^{-i1 c} w^{-i2 c} IDFT_B(Hs[. W + c])[i2]
// Rank r owns residue c = r: it transforms u_r and the mirror residue (-r mod W,
// for the combine's F[-k] G[-k]), builds G at both residues from the eq
// product formula restricted to the residue (k_eqdft_res), combines, runs one
// B-point inverse, and sends every rank d the L values of h its slice
// S[dL, (d+1)L) = h[M + dL + m] needs (i1 = W/2 + d/2, i2 = (d mod 2) L + m),
// pre-multiplied by w_W^{-i1 c} w^{-i2 c}; one all-to-all, then each rank sums
// the W vectors it received.  Work per rank: 2 B-point DIFs + 1 DIT against
// the replicated path's two 2M-point transforms; the forward input f stays
// the gathered vector (its pre-sum is W/2 multiplies per entry).
// Bit orders as in s_poly_device: DIF outputs bit-reversed within the B block.

// u[i2] = pw[i2] * sum_{i1 < h} cw[i1] f[i1 B + i2]   (cw: w_W^{i1 c} 2^261, pw: w^{i2 c} 2^261)
static constexpr int SP_MAXW = 64;
struct SpConsts {
  L9 v[SP_MAXW];
};
// (f has M entries: W/2 whole blocks for W >= 2; at W = 1 it fills half the one
// block, the rest is the zero padding)
__global__ void k_s_presum(const Fr* __restrict__ f, size_t M, size_t B, uint32_t h, SpConsts cw,
                           const Fr* __restrict__ pw, Fr* __restrict__ u) {
  const size_t i2 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i2 >= B) return;
  R29 acc = R29::zero();
  for (uint32_t i1 = 0; i1 < h; i1++) {
    const size_t g = (size_t)i1 * B + i2;
    if (g < M) acc = red2p29(add29(acc, mul29(to29(f[g]), R29::from_l9(cw.v[i1]))));
  }
  u[i2] = from29(canon29(mul29(acc, to29(pw[i2]))));
}

// The same pre-sum for two operands f and g (a general g instead of an eq
// table: the inner-product argument) at NRES residues in one pass: residue q
// has the constants cw.v[q] and the powers pw + q B, and u + (2 op + q) B
// receives operand op (0: f, 1: g) at residue q.  Each gathered entry is read
// and converted to limbs once instead of once per (operand, residue) launch of
// k_s_presum; every output runs k_s_presum's steps on its own accumulator, so
// the words are the ones four launches write.  The constants are wave-uniform
// (scalar loads from the kernel arguments); h <= SP_MAXW / 2.
struct SpConsts2 {
  L9 v[2][SP_MAXW / 2];
};
template <int NRES>
__global__ void __launch_bounds__(256)
    k_s_presum_fg(const Fr* __restrict__ f, const Fr* __restrict__ g, size_t M, size_t B,
                  uint32_t h, SpConsts2 cw, const Fr* __restrict__ pw, Fr* __restrict__ u) {
  const size_t i2 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i2 >= B) return;
  R29 acc[2][NRES];
#pragma unroll
  for (int op = 0; op < 2; op++)
#pragma unroll
    for (int q = 0; q < NRES; q++) acc[op][q] = R29::zero();
  for (uint32_t i1 = 0; i1 < h; i1++) {
    const size_t e = (size_t)i1 * B + i2;
    if (e >= M) break;  // (only at W = 1: the upper half of the one block is padding)
    const R29 x[2] = {to29(f[e]), to29(g[e])};
#pragma unroll
    for (int q = 0; q < NRES; q++) {
      const R29 k = R29::from_l9(cw.v[q][i1]);
#pragma unroll
      for (int op = 0; op < 2; op++) acc[op][q] = red2p29(add29(acc[op][q], mul29(x[op], k)));
    }
  }
#pragma unroll
  for (int q = 0; q < NRES; q++) {
    const R29 p = to29(pw[(size_t)q * B + i2]);
#pragma unroll
    for (int op = 0; op < 2; op++)
      u[(size_t)(2 * op + q) * B + i2] = from29(canon29(mul29(acc[op][q], p)));
  }
}

// G at residue c, bit-reversed within the block, one product-formula level per
// launch (k_eqdft_level restricted to k = c mod W): level t has 2^(lb - t)
// entries e (lb = log2 B), k2 = bitrev(e), factor a_t + z_t w^{(k2 W + c) 2^t}
// = a_t + (z_t w^{c 2^t}) w_B^{k2 2^t}; Q_t[e] = factor Q_{t+1}[e >> 1].
// twBb: w_B^m 2^261 for m < B/2 (w_B^{B/2} = -1) in bit-reversed order
// (ntt_tw_bitrev): w_B^{k2 2^t} is twBb[e >> 1], negated for odd e (as in
// k_eqdft_level).
__global__ void k_eqdft_res(const Fr* __restrict__ qnext, Fr q0, L9 a261, L9 zc261,
                            const Fr* __restrict__ twBb, int lb, int t, Fr* __restrict__ q) {
  const int bits = lb - t;
  const size_t len = (size_t)1 << bits;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  R29 w = to29(twBb[e >> 1]);
  if (e & 1) w = sub29(R29::zero(), w);
  const R29 fct = red2p29(add29(R29::from_l9(a261), mul29(R29::from_l9(zc261), w)));
  const R29 qn = qnext ? to29(qnext[e >> 1]) : to29(q0);
  q[e] = from29(canon29(mul29(fct, qn)));
}

// Hs at residue c in the bit-reversed block order: p -> k2 = bitrev(p); the
// partner of -k is residue m = -c mod W at position ~p (c != 0) or, for c = 0,
// the bit-reversed negation (k_s_combine_br's rule).  Hs = (-1)^c w^{-c} / n
// w_B^{-k2} (F_c G_m' + F_m' G_c): twiBb holds w_B^{-e} 2^261 (e < B/2) in
// bit-reversed order, so w_B^{-k2} = +-twiBb[p >> 1] (the sign from k2's top
// bit, p's low bit; k2's low bit is p's top bit), cst the
// per-residue constant x 2^266 (mul29 of the 2^251-scaled products lands in
// arkworks form).
// At W = 1 the (-1)^k of w^{k(M-1)} = (-1)^k w^{-k} is (-1)^k2, not the
// residue's constant (-1)^c: `alt` negates the odd k2.
__global__ void k_s_combine_res(const Fr* __restrict__ Fc, const Fr* __restrict__ Gc,
                                const Fr* __restrict__ Fm, const Fr* __restrict__ Gm, int c,
                                const Fr* __restrict__ twiBb, int lb, L9 cst, int alt,
                                Fr* __restrict__ H) {
  const size_t B = (size_t)1 << lb;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  size_t pp;
  if (c != 0) {
    pp = ~p & (B - 1);
  } else {
    pp = 0;
    if (p) {
      const int hb = 63 - __clzll((unsigned long long)p);
      pp = p ^ (((size_t)1 << hb) - 1);
    }
  }
  const bool k2top = lb > 0 && (p & 1), k2low = lb > 0 && ((p >> (lb - 1)) & 1);
  R29 wi = to29(twiBb[p >> 1]);
  if (k2top != (alt && k2low)) wi = sub29(R29::zero(), wi);
  const R29 v = red2p29(add29(mul29(to29(Fc[p]), to29(Gm[pp])), mul29(to29(Fm[pp]), to29(Gc[p]))));
  H[p] = from29(canon29(mul29(mul29(v, red6p29(wi)), R29::from_l9(cst))));
}

// send[d L + m] = K[d] P[i2] Z[i2], i2 = ((M + d L) mod B) + m: (d mod 2) L + m
// for W >= 2 (M = W/2 blocks), L + m at W = 1 (M = L = B/2; `sh` = 1)
// (K: x 2^261, P: x 2^261)
__global__ void k_s_outgoing(const Fr* __restrict__ Z, const Fr* __restrict__ P, SpConsts K,
                             size_t L, uint32_t W, uint32_t sh, Fr* __restrict__ send) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)W * L) return;
  const uint32_t d = (uint32_t)(i / L);
  const size_t i2 = (size_t)((d + sh) & 1) * L + i % L;
  send[i] = from29(canon29(mul29(mul29(to29(Z[i2]), to29(P[i2])), R29::from_l9(K.v[d]))));
}

// out[m] = sum_s recv[s L + m]
__global__ void k_s_sum_parts(const Fr* __restrict__ recv, size_t L, uint32_t W,
                              Fr* __restrict__ out) {
  const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= L) return;
  R29 acc = R29::zero();
  for (uint32_t s = 0; s < W; s++) acc = red2p29(add29(acc, to29(recv[(size_t)s * L + m])));
  out[m] = from29(canon29(acc));
}

static L9 l9_x261(const Fr& mont) {  // Montgomery field element -> (value x 2^261) limbs
  return l9_of29(ml_plain_mul(from_mont(mont), pow2_mod_plain<FrP>(261)));
}

// this rank's slice S[rank L, rank L + L) (L = M / W; the last entry of the last
// slice is h[2M - 1] = 0, past S's M - 1 coefficients).  f: the gathered
// evaluations (M entries, every rank), point: the eq variables (nvars).
// With `g` (M gathered entries, M = 2^nvars; `point` unused) the second operand
// is that general vector instead of the eq table: its side at both residues is
// what f's is, a pre-sum and the B-point DIF, in the same bit-reversed order,
// so everything from the combine on is shared.  The four pre-sums (two when the
// residue is its own mirror) run as one k_s_presum_fg launch;
// QG_S_PRESUM_FUSED=0 (read per call) runs k_s_presum per operand and residue
// instead, with the same words out (A/B runs, tests).
static void s_poly_sharded(qg_ctx* ctx, const Fr* f, size_t M, const uint64_t* point,
                           size_t nvars, Fr* S_local, const Fr* g = nullptr) {
  QgTimed tm(ctx, "s_polynomial");
  const uint32_t W = (uint32_t)ctx->world, c = (uint32_t)ctx->rank;
  QG_CHECK(W <= SP_MAXW && (W & (W - 1)) == 0 && M == ((size_t)1 << nvars) && M >= W,
           QG_ERR_UNSUPPORTED, "sharded S polynomial geometry");
  const size_t L = M / W, B = 2 * L;
  int lb = 0;
  while (((size_t)1 << lb) < B) lb++;
  int logn = 0;
  while (((size_t)1 << logn) < 2 * M) logn++;
  QG_CHECK(logn <= 28, QG_ERR_UNSUPPORTED, "S-polynomial NTT beyond 2-adicity");
  Fr *twB, *twiB;
  ntt_twiddles(ctx, lb, &twB, &twiB, "sp_tw");
  const Fr w = root_of_unity(logn), wi = finv(w);
  const Fr wW = fpow_small(w, B);  // w_W = w^(n / W)
  const Fr ninv = finv(from_u64<FrP>((uint64_t)2 * M));
  const uint32_t cm = (W - c) % W;  // mirror residue (-c mod W)
  const int nres = cm == c ? 1 : 2;
  const uint32_t res[2] = {c, cm};
  Fr* Fb = ctx->scratch_as<Fr>("sp_F", 2 * B);
  Fr* Gb = ctx->scratch_as<Fr>("sp_G", 2 * B);
  Fr* tmp = ctx->scratch_as<Fr>("sp_tmp", 2 * B);  // u / pw scratch, then G level ping-pong
  const int K = 64;
  if (g) {
    // both operands by pre-sum + DIF: u[(2 op + q) B ..), the powers of residue q at pw + q B
    Fr* ub = ctx->scratch_as<Fr>("sp_u", 4 * B);
    Fr* pw = tmp;
    const uint32_t hb = std::max<uint32_t>(1, W / 2);  // input blocks (partial at W = 1)
    SpConsts2 cw2{};
    SpConsts cw1[2] = {};
    for (int q = 0; q < nres; q++) {
      hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(B, (size_t)K), ML_BLOCK)), dim3(ML_BLOCK),
                         0, ctx->stream, fpow_small(w, res[q]), B, K, pw + (size_t)q * B);
      QG_LAUNCH_CHECK();
      Fr wk = Fr::one();
      const Fr wWc = fpow_small(wW, res[q]);
      for (uint32_t i1 = 0; i1 < hb; i1++) {
        cw2.v[q][i1] = cw1[q].v[i1] = l9_x261(wk);
        wk = wk * wWc;
      }
    }
    hipLaunchKernelGGL(k_fr_to261, dim3(div_up((size_t)nres * B, ML_BLOCK)), dim3(ML_BLOCK), 0,
                       ctx->stream, pw, (size_t)nres * B, F29P<FrP>::TO261);
    QG_LAUNCH_CHECK();
    const char* fe = getenv("QG_S_PRESUM_FUSED");
    {
      QgTimed tp(ctx, "s_presum");  // (inside "s_polynomial": micro/ipa_sharded_cost.py)
      if (!(fe && atoi(fe) == 0)) {
        const dim3 grid(div_up(B, ML_BLOCK)), blk(ML_BLOCK);
        if (nres == 2)
          hipLaunchKernelGGL(k_s_presum_fg<2>, grid, blk, 0, ctx->stream, f, g, M, B, hb, cw2, pw,
                             ub);
        else
          hipLaunchKernelGGL(k_s_presum_fg<1>, grid, blk, 0, ctx->stream, f, g, M, B, hb, cw2, pw,
                             ub);
        QG_LAUNCH_CHECK();
      } else {
        for (int op = 0; op < 2; op++)
          for (int q = 0; q < nres; q++) {
            hipLaunchKernelGGL(k_s_presum, dim3(div_up(B, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream,
                               op ? g : f, M, B, hb, cw1[q], pw + (size_t)q * B,
                               ub + (size_t)(2 * op + q) * B);
            QG_LAUNCH_CHECK();
          }
      }
    }
    for (int op = 0; op < 2; op++)
      for (int q = 0; q < nres; q++)
        ntt_run(ctx, true, ub + (size_t)(2 * op + q) * B, B, (op ? Gb : Fb) + (size_t)q * B, twB,
                "sp_tw", lb, 0, 0, nullptr);
  }
  for (int q = 0; !g && q < nres; q++) {
    const uint32_t cc = res[q];
    Fr* Fq = Fb + (size_t)q * B;
    Fr* Gq = Gb + (size_t)q * B;
    // u_cc = w^{i2 cc} sum_i1 w_W^{i1 cc} f[i1 B + i2]
    Fr* pw = tmp + B;
    hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(B, (size_t)K), ML_BLOCK)), dim3(ML_BLOCK), 0,
                       ctx->stream, fpow_small(w, cc), B, K, pw);
    QG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fr_to261, dim3(div_up(B, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream, pw, B,
                       F29P<FrP>::TO261);
    QG_LAUNCH_CHECK();
    SpConsts cw{};
    Fr wk = Fr::one();
    const Fr wWc = fpow_small(wW, cc);
    const uint32_t hb = std::max<uint32_t>(1, W / 2);  // input blocks (partial at W = 1)
    for (uint32_t i1 = 0; i1 < hb; i1++) {
      cw.v[i1] = l9_x261(wk);
      wk = wk * wWc;
    }
    hipLaunchKernelGGL(k_s_presum, dim3(div_up(B, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream, f, M,
                       B, hb, cw, pw, tmp);
    QG_LAUNCH_CHECK();
    ntt_run(ctx, true, tmp, B, Fq, twB, "sp_tw", lb, 0, 0, nullptr);
    // G at residue cc: levels above the block collapse into a host constant,
    // then one launch per level t = lb - 1 .. 0 (ping-pong tmp / Gq; nz >= lb
    // whenever W >= 2; at W = 1, nz = lb - 1 and the top level starts from q0 = 1)
    const size_t nz = nvars;
    Fr q0 = Fr::one();
    for (size_t t = nz; t-- > (size_t)lb;) {  // levels with a single entry (t >= lb)
      const Fr zt = fr_import(point + 4 * t);
      q0 = q0 * ((Fr::one() - zt) + zt * fpow_small(w, (uint64_t)cc << t));
    }
    const int top = (int)std::min<size_t>(nz, (size_t)lb);
    const Fr* twBb = ntt_tw_bitrev(ctx, twB, "sp_tw", lb);
    const Fr* qn = nullptr;
    for (int t = top - 1; t >= 0; t--) {
      const Fr zt = fr_import(point + 4 * t);
      const L9 a9 = l9_x261(Fr::one() - zt);
      const L9 z9 = l9_x261(zt * fpow_small(w, (uint64_t)cc << t));
      Fr* dst = (t & 1) == 0 ? Gq : tmp;
      const size_t len = (size_t)1 << (lb - t);
      hipLaunchKernelGGL(k_eqdft_res, dim3(div_up(len, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream,
                         qn, q0, a9, z9, twBb, lb, t, dst);
      QG_LAUNCH_CHECK();
      qn = dst;
    }
  }
  // combine + inverse (own residue), pre-multiplied outgoing vectors, all-to-all, sum
  Fr* H = tmp;
  const Fr* Fm = nres == 2 ? Fb + B : Fb;
  const Fr* Gm = nres == 2 ? Gb + B : Gb;
  Fr cst = fpow_small(wi, c) * ninv;
  if (c & 1) cst = fneg(cst);
  const L9 cst9 = l9_of29(ml_plain_mul(from_mont(cst), pow2_mod_plain<FrP>(266)));
  hipLaunchKernelGGL(k_s_combine_res, dim3(div_up(B, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream, Fb,
                     Gb, Fm, Gm, (int)c, ntt_tw_bitrev(ctx, twiB, "sp_twi", lb), lb, cst9, W == 1 ? 1 : 0,
                     H);
  QG_LAUNCH_CHECK();
  ntt_run(ctx, false, H, B, H, twiB, "sp_twi", lb, 0, 0, nullptr);
  Fr* P = tmp + B;
  hipLaunchKernelGGL(k_powers_ml, dim3(div_up(div_up(B, (size_t)K), ML_BLOCK)), dim3(ML_BLOCK), 0,
                     ctx->stream, fpow_small(wi, c), B, K, P);
  QG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fr_to261, dim3(div_up(B, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream, P, B,
                     F29P<FrP>::TO261);
  QG_LAUNCH_CHECK();
  SpConsts Kd{};
  const Fr wWi = finv(wW);
  for (uint32_t d = 0; d < W; d++) {
    const uint64_t i1 = (M + (size_t)d * L) / B;  // W/2 + d/2 for W >= 2, 0 at W = 1
    Kd.v[d] = l9_x261(fpow_small(wWi, (i1 * c) % W));
  }
  Fr* sendb = ctx->scratch_as<Fr>("sp_send", (size_t)W * L);
  Fr* recvb = ctx->scratch_as<Fr>("sp_recv", (size_t)W * L);
  hipLaunchKernelGGL(k_s_outgoing, dim3(div_up((size_t)W * L, ML_BLOCK)), dim3(ML_BLOCK), 0,
                     ctx->stream, H, P, Kd, L, W, W == 1 ? 1u : 0u, sendb);
  QG_LAUNCH_CHECK();
  comm_alltoall_bytes(ctx, sendb, recvb, L * sizeof(Fr));
  hipLaunchKernelGGL(k_s_sum_parts, dim3(div_up(L, ML_BLOCK)), dim3(ML_BLOCK), 0, ctx->stream,
                     recvb, L, W, S_local);
  QG_LAUNCH_CHECK();
}

struct MleOpenItem {
  const Fr* poly;
  size_t n;
  const uint64_t* point;
  size_t nvars;
  bool unchanged;
  uint64_t id;
  size_t off;
};

// the transcript step of one opening (mlpcs.rs:100-107): append the point
// (Vec<Fr>), the evaluation and s_comm; draw r
struct OpenChallenge {
  Fr r, r_inv;
};
static OpenChallenge open_transcript_step(uint8_t state[32], const uint64_t* point, size_t nvars,
                                          const Fr& evaluation, const G1Affine& s_comm) {
  std::vector<uint8_t> msg(8 + 32 * nvars);
  u64_to_bytes(nvars, msg.data());
  for (size_t i = 0; i < nvars; i++) fr_to_bytes(fr_import(point + 4 * i), msg.data() + 8 + 32 * i);
  transcript_append(state, msg.data(), msg.size());
  uint8_t b32[32], b64[64];
  fr_to_bytes(evaluation, b32);
  transcript_append(state, b32, 32);
  g1_serialize(s_comm, b64);
  transcript_append(state, b64, 64);
  const Fr r = transcript_draw_fr(state);
  QG_CHECK(!r.is_zero(), QG_ERR_ASSERT, "challenge r = 0");
  return {r, finv(r)};
}
// ... and of the inner-product argument (ipa.rs:76-83): append inner_product
// and s_comm; draw r
static OpenChallenge ipa_transcript_step(uint8_t state[32], const Fr& ip, const G1Affine& s_comm) {
  uint8_t b32[32], b64[64];
  fr_to_bytes(ip, b32);
  transcript_append(state, b32, 32);
  g1_serialize(s_comm, b64);
  transcript_append(state, b64, 64);
  const Fr r = transcript_draw_fr(state);
  QG_CHECK(!r.is_zero(), QG_ERR_ASSERT, "challenge r = 0");
  return {r, finv(r)};
}

// the four KZG openings of a proof in quotient order (OPEN_QNAME)
struct Open4 {
  qg_kzg_opening* o[4];
};
static Open4 open4(qg_mle_proof& p) {
  return {{&p.poly_opening, &p.poly_opening_inv, &p.s_opening, &p.s_opening_inv}};
}
// ... and the six of an inner-product proof (IPA_QNAME)
struct Open6 {
  qg_kzg_opening* o[6];
};
static Open6 open6(qg_ipa_proof& p) {
  return {{&p.f_opening, &p.f_opening_inv, &p.g_opening, &p.g_opening_inv, &p.s_opening,
           &p.s_opening_inv}};
}

// Per-item scratch of a batch of openings (S vectors, quotient vectors, eq
// points) and the per-MSM slots of its MSM batches (msm.hip: partials, owners,
// bucket starts, plan words) stay allocated for the next batch: HyperPlonk
// reuses them trace after trace.  Beyond a working set of OPEN_KEEP items
// (4 OPEN_KEEP MSMs) they are freed when the batch ends (a batch of
// 256 items at 2^20 would otherwise pin ~70-80 GB for the context's lifetime).
static constexpr size_t OPEN_KEEP = 16;
static void open_batch_trim_scratch(qg_ctx* ctx, size_t K) {
  for (size_t k = OPEN_KEEP; k < K; k++) {
    ctx->arena.release("mleb_S#" + std::to_string(k));
    ctx->arena.release("mleb_Sl#" + std::to_string(k));
    ctx->arena.release("mleb_z#" + std::to_string(k));
  }
  for (size_t j = 4 * OPEN_KEEP; j < 4 * K; j++) {
    ctx->arena.release("open_s#" + std::to_string(j));
    for (const char* m : {"msm_partial#", "msm_owner#", "msm_bstart#", "msm_misc#"})
      ctx->arena.release(m + std::to_string(j));
  }
}

// MLEvalProof::prove for K >= 1 openings with a communicator: this rank holds
// poly[rank L, (rank+1) L) of each item's 2^nvars evaluations (L = 2^nvars /
// world) and the matching SRS shard.  The data flow is batched the way
// mle_open_batch_device batches the single-context one.  Per item the eq
// table, the local dot, the gathered vector's residue-split S slice
// (s_poly_sharded; QG_S_REPLICATED=1: the whole S on every rank, A/B runs) and
// the local trimmed lengths are queued; ONE allgather carries every item's dot
// part and local lengths and this rank's shard size, so the global trimmed
// lengths and the "Polynomial degree exceeds max degree" decision (op_fits)
// are the same on every rank; the S commitments run as ONE MSM batch (one
// allgather of the per-rank partials); the transcript steps run on the host
// in item order; the 4K quotients are quotients_sharded's (one allgather of
// the slice-end values T, one of the check's evaluations, ONE sharded MSM
// batch).  Four exchanges per call, the check's included; between the first
// collective and the last no decision that ends the call is taken on a value
// that differs between ranks.  The proofs and the final transcript state of a
// batch of K equal K batches of one, and the single-context ones
// (tests/test_gpu_multirank.py).
static void mle_open_batch_sharded(qg_ctx* ctx, const qg_srs* srs,
                                   const std::vector<MleOpenItem>& items, uint8_t state[32],
                                   qg_mle_proof* outs) {
  const size_t K = items.size();
  const size_t W = (size_t)ctx->world, rank = (size_t)ctx->rank;
  for (const MleOpenItem& it : items) {
    QG_CHECK(it.nvars <= 30, QG_ERR_INVALID, "too many variables");
    QG_CHECK(it.n * W == ((size_t)1 << it.nvars), QG_ERR_UNSUPPORTED,
             "sharded opening needs world * local length == 2^nvars");
  }
  // small values of this rank: K dot parts, 2K local trimmed lengths, the shard size
  const size_t sm_bytes = K * sizeof(Fr) + (2 * K + 1) * sizeof(unsigned long long);
  uint8_t* d_sm = ctx->scratch_as<uint8_t>("mlebs_small", sm_bytes);
  Fr* d_part = reinterpret_cast<Fr*>(d_sm);
  unsigned long long* d_len = reinterpret_cast<unsigned long long*>(d_sm + K * sizeof(Fr));
  QG_HIP(hipMemsetAsync(d_sm, 0, sm_bytes, ctx->stream));
  const unsigned long long my_n = srs->n;
  QG_HIP(hipMemcpyAsync(d_len + 2 * K, &my_n, sizeof my_n, hipMemcpyHostToDevice, ctx->stream));
  const char* rep = getenv("QG_S_REPLICATED");  // read per call: tests toggle it in-process
  const bool replicated = rep && atoi(rep) != 0;
  std::vector<Fr*> Sl(K);
  for (size_t k = 0; k < K; k++) {
    const MleOpenItem& it = items[k];
    const size_t L = it.n, N = (size_t)1 << it.nvars, off = rank * L;
    Fr* dz = ctx->scratch_as<Fr>("mleb_z#" + std::to_string(k), it.nvars ? it.nvars : 1);
    Fr* dpr = ctx->scratch_as<Fr>("mle_pr", N);
    fr_upload(ctx, dz, it.point, it.nvars);
    eq_table_device(ctx, dz, (uint32_t)it.nvars, dpr);
    dot_to_device(ctx, it.poly, dpr + off, L, d_part + k);
    trim_launch(ctx, it.poly, L, d_len + 2 * k);
    Sl[k] = ctx->scratch_as<Fr>("mleb_Sl#" + std::to_string(k), L);
    if (N > 1) {
      Fr* dfull = ctx->scratch_as<Fr>("mle_full", N);
      comm_allgather_bytes(ctx, it.poly, dfull, L * sizeof(Fr));
      if (replicated) {
        Fr* dS = ctx->scratch_as<Fr>("mle_S", N);
        s_poly_device(ctx, dfull, N, dpr, N, dS, it.point, it.nvars);
        QG_HIP(hipMemsetAsync(dS + N - 1, 0, sizeof(Fr), ctx->stream));  // h[2M - 1] = 0
        QG_HIP(hipMemcpyAsync(Sl[k], dS + off, L * sizeof(Fr), hipMemcpyDeviceToDevice,
                              ctx->stream));
      } else {
        s_poly_sharded(ctx, dfull, N, it.point, it.nvars, Sl[k]);
      }
    } else {
      QG_HIP(hipMemsetAsync(Sl[k], 0, L * sizeof(Fr), ctx->stream));
    }
    trim_launch(ctx, Sl[k], L, d_len + 2 * k + 1);
  }
  if (ctx->open_fault_live == 1) {  // test-only: this rank's first nonzero local length
    ctx->open_fault_live = 0;
    hipLaunchKernelGGL(k_fault_short_len, dim3(1), dim3(64), 0, ctx->stream, d_len, 2 * K,
                       (unsigned long long)ctx->open_fault_value);
    QG_LAUNCH_CHECK();
  }
  // exchange 1: dot parts, local lengths and shard size of every rank
  uint8_t* d_all = ctx->scratch_as<uint8_t>("mlebs_small_all", sm_bytes * W);
  comm_allgather_bytes(ctx, d_sm, d_all, sm_bytes);
  std::vector<uint8_t> h_all(sm_bytes * W);
  QG_HIP(hipMemcpyAsync(h_all.data(), d_all, sm_bytes * W, hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  auto lens_of = [&](size_t r) {
    return reinterpret_cast<const unsigned long long*>(h_all.data() + r * sm_bytes + K * sizeof(Fr));
  };
  std::vector<Fr> evaluation(K, Fr::zero());
  std::vector<size_t> Lt(K), Slen(K);  // global trimmed lengths
  std::vector<unsigned long long> shard(W), loc(W);
  for (size_t r = 0; r < W; r++) shard[r] = lens_of(r)[2 * K];
  for (size_t k = 0; k < K; k++) {
    const size_t L = items[k].n;
    for (size_t r = 0; r < W; r++)
      evaluation[k] = evaluation[k] + reinterpret_cast<const Fr*>(h_all.data() + r * sm_bytes)[k];
    for (size_t r = 0; r < W; r++) loc[r] = lens_of(r)[2 * k];
    Lt[k] = op_global_len(loc.data(), W, L);
    for (size_t r = 0; r < W; r++) loc[r] = lens_of(r)[2 * k + 1];
    Slen[k] = op_global_len(loc.data(), W, L);
    // every rank knows every rank's part lengths and bases: the same decision on all
    const size_t opened[2] = {Lt[k], Slen[k]};
    QG_CHECK(op_fits(Slen[k], opened, 2, L, shard.data(), W), QG_ERR_INVALID,
             "Polynomial degree exceeds max degree");
  }
  // the S commitments: one MSM batch over the local parts of the trimmed S
  std::vector<const Fr*> sp(Sl.begin(), Sl.end());
  std::vector<size_t> sloc(K);
  for (size_t k = 0; k < K; k++) sloc[k] = op_live(Slen[k], rank, items[k].n);
  const std::vector<G1Affine> s_comm = msm_device_batch(ctx, srs, sp, sloc);
  // the transcript steps in item order (mlpcs.rs:100-107), then the 4K
  // quotients: job 4k + i is item k's OPEN_QNAME[i]
  std::vector<ShardQuotJob> jobs;
  for (size_t k = 0; k < K; k++) {
    const OpenChallenge ch =
        open_transcript_step(state, items[k].point, items[k].nvars, evaluation[k], s_comm[k]);
    fr_export(evaluation[k], outs[k].evaluation);
    g1_export(s_comm[k], outs[k].s_comm_xy, &outs[k].s_comm_inf);
    const Open4 o4 = open4(outs[k]);
    const size_t L = items[k].n;
    jobs.push_back({items[k].poly, L, Lt[k], ch.r, o4.o[0]});
    jobs.push_back({items[k].poly, L, Lt[k], ch.r_inv, o4.o[1]});
    jobs.push_back({Sl[k], L, Slen[k], ch.r, o4.o[2]});
    jobs.push_back({Sl[k], L, Slen[k], ch.r_inv, o4.o[3]});
  }
  quotients_sharded(ctx, srs, jobs, 4, false, OPEN_QNAME,
                    [&] { open_batch_trim_scratch(ctx, K); });
}

// MLEvalProof::prove (mlpcs.rs:83-124) for K >= 1 device-resident evaluation
// vectors, the transcript steps in item order — the same proofs and final
// state as K successive batches of one — laid out around the protocol's data
// flow: S, its commitment, the evaluation and the trimmed lengths depend on
// the polynomial and the point only, and the transcript absorbs no quotient
// commitment, so
//   1. every item's evaluation, S polynomial and trimmed lengths (queued),
//   2. the K S commitments as ONE MSM batch (one synchronization),
//   3. the K transcript steps on the host (append point, evaluation, s_comm;
//      draw r),
//   4. the 4K quotients and their commitments as ONE MSM batch.
// Two host round trips per call, both for values the transcript or the caller
// needs; the inner products, the trimmed lengths (DensePolynomial trims,
// kzg.rs / ipa.rs) and the values y are queued into pinned memory and read
// after those synchronizations.  Inside a batch the bucketing of MSM i + 1
// runs on the side stream beside MSM i's accumulation, and the batch pays one
// set of reduction launches and one host round trip (msm.hip).  A sharded
// context runs mle_open_batch_sharded.  Steps 1 and 2 (open_batch_front) and
// the per-item part of step 3 (open_batch_item_step) are shared with the
// folded opening below.

// What steps 1 and 2 leave, read back after their one synchronization.
struct OpenFront {
  const unsigned long long* h_len = nullptr;  // [2k]: the vector's, [2k + 1]: S's
  const Fr* h_eval = nullptr;
  std::string memo_in;
  std::vector<std::string> lt_key;
  std::vector<char> lt_known;
  std::vector<Fr*> dS;
  std::vector<size_t> Sn;
  std::vector<G1Affine> s_comm;
  std::vector<size_t> Lt, Lq;  // Lq: the length the quotients use (Lt unless faulted)
};

static OpenFront open_batch_front(qg_ctx* ctx, const qg_srs* srs,
                                  const std::vector<MleOpenItem>& items) {
  const size_t K = items.size();
  OpenFront F;
  unsigned long long* h_len = reinterpret_cast<unsigned long long*>(
      ctx->pinned_get("mleb_len_h", 2 * K * sizeof(unsigned long long)));
  unsigned long long* d_len = ctx->scratch_as<unsigned long long>("mleb_len", 2 * K);
  Fr* h_eval = reinterpret_cast<Fr*>(ctx->pinned_get("mleb_eval_h", K * sizeof(Fr)));
  Fr* d_eval = ctx->scratch_as<Fr>("mleb_eval", K);
  QG_HIP(hipMemsetAsync(d_len, 0, 2 * K * sizeof(unsigned long long), ctx->stream));
  // the opened vectors' trimmed lengths: remembered while the caller
  // guarantees the vector unchanged (QG_OPEN_UNCHANGED contract, same
  // allocation id and offset).  The memo holds the last opened vector's key and
  // length: item k reuses it when flagged and item k - 1 (item 0: the memo
  // from before this call) opened the same vector
  F.memo_in = ctx->arena.memo["mle_poly_len"];
  const std::string& memo_in = F.memo_in;
  std::vector<std::string>& lt_key = F.lt_key;
  std::vector<char>& lt_known = F.lt_known;
  std::vector<Fr*>& dS = F.dS;
  std::vector<size_t>& Sn = F.Sn;
  lt_key.resize(K), lt_known.assign(K, 0), dS.assign(K, nullptr), Sn.assign(K, 0);
  F.Lt.resize(K), F.Lq.resize(K);
  std::vector<size_t> s_msm(K, 0);
  bool s_trim_first = false;
  for (size_t k = 0; k < K; k++) {
    const MleOpenItem& it = items[k];
    QG_CHECK(it.nvars <= 30, QG_ERR_INVALID, "too many variables");
    const size_t N = (size_t)1 << it.nvars;
    lt_key[k] = it.id ? std::to_string(it.id) + "+" + std::to_string(it.off) + ":" +
                            std::to_string(it.n) + "="
                      : std::string();
    lt_known[k] = it.unchanged && it.id &&
                  (k == 0 ? memo_in.compare(0, lt_key[k].size(), lt_key[k]) == 0
                          : lt_key[k - 1] == lt_key[k]);
    if (!lt_known[k]) trim_launch(ctx, it.poly, it.n, d_len + 2 * k);
    Fr* dz = ctx->scratch_as<Fr>("mleb_z#" + std::to_string(k), it.nvars ? it.nvars : 1);
    Fr* dpr = ctx->scratch_as<Fr>("mle_pr", N);
    fr_upload(ctx, dz, it.point, it.nvars);
    eq_table_device(ctx, dz, (uint32_t)it.nvars, dpr);
    dot_to_device(ctx, it.poly, dpr, it.n < N ? it.n : N, d_eval + k);
    const size_t M = it.n > N ? it.n : N;
    Sn[k] = M > 1 ? M - 1 : 0;
    dS[k] = ctx->scratch_as<Fr>("mleb_S#" + std::to_string(k), Sn[k] ? Sn[k] : 1);
    if (Sn[k])
      s_poly_device(ctx, it.poly, it.n, dpr, N, dS[k], it.point, it.nvars, it.unchanged, it.id,
                    it.off);
    trim_launch(ctx, dS[k], Sn[k], d_len + 2 * k + 1);
    s_msm[k] = Sn[k];
    s_trim_first = s_trim_first || Sn[k] > srs->n;
  }
  QG_HIP(hipMemcpyAsync(h_len, d_len, 2 * K * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        ctx->stream));
  QG_HIP(hipMemcpyAsync(h_eval, d_eval, K * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  if (s_trim_first) {  // an S longer than the SRS: its trimmed length decides
    ctx->sync();
    for (size_t k = 0; k < K; k++)
      if (Sn[k] > srs->n) {
        s_msm[k] = (size_t)h_len[2 * k + 1];
        QG_CHECK(s_msm[k] <= srs->n, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
      }
  }
  std::vector<const Fr*> sp(dS.begin(), dS.end());
  F.s_comm = msm_device_batch(ctx, srs, sp, s_msm);
  ctx->sync();  // (drained already unless every MSM was empty)
  F.h_len = h_len, F.h_eval = h_eval;
  return F;
}

// item k's transcript step (mlpcs.rs:100-107), in item order: its trimmed
// length (memo or device value), the memo for the next item, the evaluation
// and s_comm into the proof
static OpenChallenge open_batch_item_step(qg_ctx* ctx, OpenFront& F,
                                          const std::vector<MleOpenItem>& items, size_t k,
                                          uint8_t state[32], uint64_t evaluation_out[4],
                                          uint64_t s_comm_xy[8], uint8_t* s_comm_inf) {
  const MleOpenItem& it = items[k];
  if (F.lt_known[k]) {
    F.Lt[k] = k == 0 ? (size_t)std::stoull(F.memo_in.substr(F.lt_key[k].size())) : F.Lt[k - 1];
    F.Lq[k] = F.Lt[k];
  } else {
    F.Lt[k] = (size_t)F.h_len[2 * k];
    F.Lq[k] = fault_short_trim(ctx, F.Lt[k]);
  }
  ctx->arena.memo["mle_poly_len"] = it.id ? F.lt_key[k] + std::to_string(F.Lt[k]) : std::string();
  const Fr evaluation = F.h_eval[k];
  const OpenChallenge ch =
      open_transcript_step(state, it.point, it.nvars, evaluation, F.s_comm[k]);
  fr_export(evaluation, evaluation_out);
  g1_export(F.s_comm[k], s_comm_xy, s_comm_inf);
  return ch;
}

static void mle_open_batch_device(qg_ctx* ctx, const qg_srs* srs,
                                  const std::vector<MleOpenItem>& items, uint8_t state[32],
                                  qg_mle_proof* outs) {
  const size_t K = items.size();
  if (K == 0) return;
  if (ctx->sharded) {
    // QG_OPEN_BATCH_SHARDED=0: a sharded context opens item by item (A/B runs)
    const char* sb = getenv("QG_OPEN_BATCH_SHARDED");
    if (!(sb && atoi(sb) == 0)) return mle_open_batch_sharded(ctx, srs, items, state, outs);
    for (size_t k = 0; k < K; k++) mle_open_batch_sharded(ctx, srs, {items[k]}, state, &outs[k]);
    return;
  }
  OpenFront F = open_batch_front(ctx, srs, items);
  // the transcript steps in item order (mlpcs.rs:100-107)
  std::vector<Fr> rs(K), rinv(K);
  for (size_t k = 0; k < K; k++) {
    const OpenChallenge ch = open_batch_item_step(ctx, F, items, k, state, outs[k].evaluation,
                                                  outs[k].s_comm_xy, &outs[k].s_comm_inf);
    rs[k] = ch.r, rinv[k] = ch.r_inv;
  }
  // every item's four quotients (mlpcs.rs:108-113; job 4k + i is item k's
  // OPEN_QNAME[i]), then all 4K commitments
  std::vector<QuotJob> jobs;
  for (size_t k = 0; k < K; k++) {
    const size_t slen = fault_short_trim(ctx, (size_t)F.h_len[2 * k + 1]);
    const Open4 o4 = open4(outs[k]);
    jobs.push_back({items[k].poly, items[k].n, F.Lq[k], rs[k], o4.o[0]});
    jobs.push_back({items[k].poly, items[k].n, F.Lq[k], rinv[k], o4.o[1]});
    jobs.push_back({F.dS[k], F.Sn[k], slen, rs[k], o4.o[2]});
    jobs.push_back({F.dS[k], F.Sn[k], slen, rinv[k], o4.o[3]});
  }
  const QuotStage st = quotients_queue(ctx, jobs, 4);
  st.fit(srs);
  const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, st.qs, st.qns);
  ctx->sync();  // (drained already unless every quotient was empty)
  open_batch_trim_scratch(ctx, K);  // (before a failed check leaves the call)
  st.settle(ctx, OPEN_QNAME);
  st.store(pis);
}

// ---------------------------------------------------------------- folded opening
// f and S are opened at the same two points, so with gamma drawn after the
// four values y one quotient per point serves both: the quotient of
// h = f + gamma S at x is q_f + gamma q_S, checked against C_f + gamma s_comm
// (the same-point batching of GWC / PLONK; no counterpart in the reference,
// DESIGN section 5).  Per opening 3 MSMs (S, W_r, W_inv) instead of 5, and two
// quotient vectors instead of four.
static const char* const FOLD_QNAME[2] = {"folded at r", "folded at 1/r"};
static const char* const FOLD_XNAME[2] = {"combination at xs[0]", "combination at xs[1]"};

// The check of one folded scan's quotients at sigma.  ev: the P source values
// p_j(sigma) (over the untrimmed lengths), then the nq quotient values.
// hs = sum_q g_q ev[q]; per point j: yh = yv ? sum_q g_q yv[P j + q] (the
// values of the evaluation kernel, P per point: y_f + gamma y_S for the ML
// opening, y_f + gamma y_g + gamma^2 y_S for the inner-product argument) : the
// scan's own s_0;
// w[j] = hs - yh != q_j(sigma) (sigma - x_j), or s_0 != yh.  has_q == 0 (the
// trimmed length was 0): hs == 0 over the untrimmed lengths and yh == 0.
struct FoldFin {
  const Fr* ev;
  int P, nq, has_q;
  Fr g[SHF_P];
  Fr d[2];  // sigma - x_j
  const Fr* yv;
  const Fr* s0[2];
  uint32_t* w;
};
__global__ void k_fold_check_fin(FoldFin f) {
  const int j = threadIdx.x;
  if (blockIdx.x != 0 || j >= 2) return;
  uint32_t bad = 0;
  if (j < f.nq) {
    Fr hs = Fr::zero();
    for (int q = 0; q < f.P; q++) hs = hs + f.g[q] * f.ev[q];
    Fr yv = Fr::zero();
    if (f.yv)
      for (int q = 0; q < f.P; q++) yv = yv + f.g[q] * f.yv[f.P * j + q];
    if (f.has_q) {
      const Fr s0 = *f.s0[j];
      const Fr yh = f.yv ? yv : s0;
      const Fr r = hs - yh - f.ev[f.P + j] * f.d[j];
      bad = (r.is_zero() && s0 == yh) ? 0u : 1u;
    } else {
      bad = (hs.is_zero() && yv.is_zero()) ? 0u : 1u;
    }
  }
  f.w[j] = bad;
}

// One folded scan with everything around it, queued: h = sum_j g[j] p_j over
// L = its trimmed length (the caller's: the largest trimmed source length) at
// nx points into s[.], the test fault, and kzg.rs:85's check into d_w[0..2)
// (pn[j]: the untrimmed source lengths; yv as in FoldFin).
struct FoldScan {
  const Fr* p[SHF_P];
  size_t pn[SHF_P], pl[SHF_P];  // untrimmed / trimmed lengths
  Fr g[SHF_P];
  int P;
  size_t L;
  Fr x[2];
  int nx;
  Fr* s[2];
};
static void fold_scan_queue(qg_ctx* ctx, const FoldScan& fs, const Fr* d_yv, uint32_t* d_w) {
  if (fs.L) {
    QgTimed tm(ctx, "kzg_division");
    if (fs.nx == 2) {
      ShFoldIn<2> in{};
      for (int j = 0; j < fs.P; j++) in.c[j] = fs.p[j], in.n[j] = fs.pl[j], in.g[j] = fs.g[j];
      in.P = fs.P, in.L = fs.L;
      for (int p = 0; p < 2; p++) in.x[p] = fs.x[p], in.s[p] = fs.s[p];
      suffix_horner_fold<2>(ctx, in);
    } else {
      ShFoldIn<1> in{};
      for (int j = 0; j < fs.P; j++) in.c[j] = fs.p[j], in.n[j] = fs.pl[j], in.g[j] = fs.g[j];
      in.P = fs.P, in.L = fs.L, in.x[0] = fs.x[0], in.s[0] = fs.s[0];
      suffix_horner_fold<1>(ctx, in);
    }
  }
  if (fs.L)
    for (int p = 0; p < fs.nx; p++) fault_quotient(ctx, fs.s[p] + 1, fs.L - 1);
  if (!d_w) return;
  QgTimed tm(ctx, "kzg_open_check");
  const Fr sigma = ctx->open_sigma;
  std::vector<EvIn> in;
  for (int j = 0; j < fs.P; j++) in.push_back({fs.p[j], fs.pn[j], 0});
  if (fs.L)
    for (int p = 0; p < fs.nx; p++) in.push_back({fs.s[p] + 1, fs.L - 1, 0});
  Fr* d_ev = ctx->scratch_as<Fr>("open_ck_ev", 8);
  poly_eval_queue(ctx, in, {sigma}, d_ev);
  FoldFin f{};
  f.ev = d_ev, f.P = fs.P, f.nq = fs.nx, f.has_q = fs.L ? 1 : 0;
  for (int j = 0; j < fs.P; j++) f.g[j] = fs.g[j];
  for (int p = 0; p < fs.nx; p++) f.d[p] = sigma - fs.x[p], f.s0[p] = fs.s[p];
  f.yv = d_yv, f.w = d_w;
  hipLaunchKernelGGL(k_fold_check_fin, dim3(1), dim3(64), 0, ctx->stream, f);
  QG_LAUNCH_CHECK();
}

// The folded form of mle_open_batch_device, single context.  The first half
// is the same (open_batch_front).  Then per item, in item order: the
// transcript step, the four values y = (f(r), f(1/r), S(r), S(1/r)) by the
// evaluation kernel over the untrimmed vectors (region "fold_eval"), one host
// round trip - Fiat-Shamir forces it: gamma_k needs item k's y and item
// k + 1's r needs gamma_k's transcript state -, the four appends, gamma_k, and
// the folded scan queued.  All 2K quotient commitments are ONE MSM batch.
static void mle_open_folded_batch_device(qg_ctx* ctx, const qg_srs* srs,
                                         const std::vector<MleOpenItem>& items,
                                         uint8_t state[32], qg_mle_proof_folded* outs) {
  const size_t K = items.size();
  if (K == 0) return;
  memset(outs, 0, K * sizeof *outs);
  OpenFront F = open_batch_front(ctx, srs, items);
  const bool check = open_check_on();
  Fr* d_y = ctx->scratch_as<Fr>("fold_y", 4);
  Fr* h_y = reinterpret_cast<Fr*>(ctx->pinned_get("fold_y_h", 4 * sizeof(Fr)));
  uint32_t* d_w = check ? ctx->scratch_as<uint32_t>("open_ck_w", 2 * K) : nullptr;
  uint32_t* h_w =
      reinterpret_cast<uint32_t*>(ctx->pinned_get("open_ck_h", 2 * K * sizeof(uint32_t)));
  size_t nmax = 0;
  for (const MleOpenItem& it : items) nmax = std::max(nmax, std::max(it.n, (size_t)1 << it.nvars));
  poly_eval_reserve(ctx, 4, nmax, 1);  // fold_eval: {f, S}; the check: {f, S, W_r, W_inv}
  std::vector<const Fr*> qs(2 * K, nullptr);
  std::vector<size_t> qns(2 * K, 0);
  std::vector<uint8_t> checked(check ? 2 * K : 0, CK_NONE);
  for (size_t k = 0; k < K; k++) {
    const MleOpenItem& it = items[k];
    const OpenChallenge ch = open_batch_item_step(ctx, F, items, k, state, outs[k].evaluation,
                                                  outs[k].s_comm_xy, &outs[k].s_comm_inf);
    const size_t slen = fault_short_trim(ctx, (size_t)F.h_len[2 * k + 1]);
    {
      // d_y = f(r), S(r), f(1/r), S(1/r)
      QgTimed tm(ctx, "fold_eval");
      const std::vector<EvIn> two = {{it.poly, it.n, 0}, {F.dS[k], F.Sn[k], 0}};
      poly_eval_queue(ctx, two, {ch.r}, d_y);
      poly_eval_queue(ctx, two, {ch.r_inv}, d_y + 2);
      QG_HIP(hipMemcpyAsync(h_y, d_y, 4 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    }
    ctx->sync();
    const Fr y[4] = {h_y[0], h_y[2], h_y[1], h_y[3]};  // OPEN_QNAME order
    for (int i = 0; i < 4; i++) {
      uint8_t b32[32];
      fr_to_bytes(y[i], b32);
      transcript_append(state, b32, 32);
      fr_export(y[i], outs[k].y[i]);
    }
    const Fr gamma = transcript_draw_fr(state);
    const size_t Lh = std::max(F.Lq[k], slen);
    QG_CHECK(Lh <= srs->n + 1, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
    FoldScan fs{};
    fs.p[0] = it.poly, fs.pn[0] = it.n, fs.pl[0] = F.Lq[k], fs.g[0] = Fr::one();
    fs.p[1] = F.dS[k], fs.pn[1] = F.Sn[k], fs.pl[1] = slen, fs.g[1] = gamma;
    fs.P = 2, fs.L = Lh, fs.nx = 2, fs.x[0] = ch.r, fs.x[1] = ch.r_inv;
    for (int p = 0; p < 2; p++) {
      fs.s[p] = Lh ? ctx->scratch_as<Fr>("open_s#" + std::to_string(2 * k + p), Lh) : nullptr;
      qs[2 * k + p] = Lh ? fs.s[p] + 1 : nullptr;
      qns[2 * k + p] = Lh ? Lh - 1 : 0;
    }
    fold_scan_queue(ctx, fs, check ? d_y : nullptr, check ? d_w + 2 * k : nullptr);
    if (check) {
      QG_HIP(hipMemcpyAsync(h_w + 2 * k, d_w + 2 * k, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            ctx->stream));
      const uint8_t c = Lh ? CK_QUOT : (it.n || F.Sn[k]) ? CK_ZERO : CK_NONE;
      checked[2 * k] = checked[2 * k + 1] = c;
    }
  }
  const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, qs, qns);
  ctx->sync();  // (drained already unless every quotient was empty)
  open_batch_trim_scratch(ctx, K);  // (before a failed check leaves the call)
  if (check) {
    std::vector<uint32_t> bad(h_w, h_w + 2 * K);
    open_check_settle(ctx, bad, checked, 2, FOLD_QNAME);
  }
  for (size_t k = 0; k < K; k++) {
    g1_export(pis[2 * k], outs[k].w_xy, &outs[k].w_inf);
    g1_export(pis[2 * k + 1], outs[k].w_inv_xy, &outs[k].w_inv_inf);
  }
}

// a single opening is a batch of one
static void mle_open_device(qg_ctx* ctx, const qg_srs* srs, const Fr* dpoly, size_t n,
                            const uint64_t* point, size_t nvars, uint8_t state[32],
                            qg_mle_proof* out, bool unchanged = false, uint64_t poly_id = 0,
                            size_t poly_off = 0) {
  mle_open_batch_device(ctx, srs, {{dpoly, n, point, nvars, unchanged, poly_id, poly_off}}, state,
                        out);
}

// One opening call: draws its check point sigma and makes an armed test fault
// live for exactly this call.  sigma never touches the transcript.  The ranks
// of a sharded group need the same sigma: at the first sharded opening rank
// 0's seed is shared once (allgather_host) and every rank reseeds with it;
// opening calls are collective, so the generators then step in lockstep.
// QG_OPEN_CHECK_SEED=<u64> (read per call) fixes the point instead.
// The share runs whether or not QG_OPEN_CHECK is on, and a fixed seed does not
// step the context generator, so lockstep assumes what the other per-call
// switches assume already: every rank of a group - in a multi-process group,
// every process - runs with the same QG_OPEN_CHECK* environment.
struct OpenCall {
  qg_ctx* c;
  explicit OpenCall(qg_ctx* ctx) : c(ctx) {
    c->open_fault_live = c->open_fault_armed;
    c->open_fault_armed = 0;
    try {
      if (c->sharded && !c->open_rng_shared) {
        const uint64_t mine = c->open_rng();
        std::vector<uint64_t> all((size_t)c->world);
        allgather_host(c, &mine, sizeof mine, all.data());
        c->open_rng.seed(all[0]);
        c->open_rng_shared = true;
      }
    } catch (...) {
      c->open_fault_live = 0;
      throw;
    }
    const char* e = getenv("QG_OPEN_CHECK_SEED");
    std::mt19937_64 fixed(e ? strtoull(e, nullptr, 0) : 0);
    std::mt19937_64& g = e ? fixed : c->open_rng;
    uint64_t w[4];
    for (uint64_t& v : w) v = g();
    w[3] &= (1ull << 61) - 1;  // < 2^253 < r: a valid representative, uniform over 2^253 values
    c->open_sigma = fr_import(w);
  }
  ~OpenCall() { c->open_fault_live = 0; }
};

// ---------------------------------------------------------------- inner-product argument
// InnerProductProof::prove (ipa.rs:59-112) on two device-resident coefficient
// vectors, shaped like mle_open_batch_device: two host round trips, one for the S
// commitment the transcript absorbs, one for the six quotient commitments.
// The trimmed lengths, the inner product and the six values y are queued into
// pinned memory and read after those synchronizations.  S is computed by the
// general-g branch of s_poly_device; it is called without a buffer identity,
// so it clears the "ntt_F_src" memo: after this call no QG_OPEN_UNCHANGED
// opening finds a transform to reuse (ntt_F now holds f's).
// The six openings are three polynomials at r and 1/r (the TODO at ipa.rs:86):
// six single suffix-Horner jobs, or with QG_IPA_PAIRED=1 (read per call) three
// paired ones (suffix_horner<2>); the same bits either way.  Measured
// (profiles/ipa_cost.json): the single jobs' kzg_division is
// 2-3 % shorter at 2^20 coefficients; at 2^22 the two are within 2 %.
static const char* const IPA_QNAME[6] = {"f at r", "f at 1/r", "g at r",
                                         "g at 1/r", "S at r", "S at 1/r"};

// ipa.rs:94-100 on the six values y (IPA_QNAME order)
static void ipa_check_equation(const Fr y[6], const Fr& r, const Fr& r_inv, const Fr& ip) {
  QG_CHECK(y[0] * y[3] + y[1] * y[2] == r * y[4] + r_inv * y[5] + from_u64<FrP>(2) * ip,
           QG_ERR_ASSERT, "Inner product verification equation failed");
}

// What the first half of the argument leaves (ipa.rs:59-83), shared with the
// folded form below: S and its length, the trimmed lengths the quotients use,
// and the challenge; inner_product and s_comm are in the proof already.
struct IpaFront {
  Fr* dS;
  size_t Sn;
  Fr ip;
  size_t Lf, Lg, Ls;
  OpenChallenge ch;
};

static IpaFront ipa_front(qg_ctx* ctx, const qg_srs* srs, const Fr* df, size_t nf, const Fr* dg,
                          size_t ng, uint8_t state[32], uint64_t ip_out[4], uint64_t s_comm_xy[8],
                          uint8_t* s_comm_inf) {
  const size_t M = nf > ng ? nf : ng;  // >= 1 (the caller's check)
  const size_t Sn = M - 1;
  unsigned long long* h_len = reinterpret_cast<unsigned long long*>(
      ctx->pinned_get("ipa_len_h", 3 * sizeof(unsigned long long)));
  unsigned long long* d_len = ctx->scratch_as<unsigned long long>("ipa_len", 3);
  // DensePolynomial::from_coefficients_slice trims what KZG::open is given (kzg.rs:77)
  trim_launch(ctx, df, nf, d_len);
  trim_launch(ctx, dg, ng, d_len + 1);
  // <f, g> over the common prefix (ipa.rs:66-69)
  Fr* d_ip = ctx->scratch_as<Fr>("ipa_ip", 1);
  Fr* h_ip = reinterpret_cast<Fr*>(ctx->pinned_get("ipa_ip_h", sizeof(Fr)));
  dot_to_device(ctx, df, dg, nf < ng ? nf : ng, d_ip);
  QG_HIP(hipMemcpyAsync(h_ip, d_ip, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  // S of the zero-padded pair (ipa.rs:72, :122-157); an empty operand gives S = 0
  Fr* dS = ctx->scratch_as<Fr>("ipa_S", Sn ? Sn : 1);
  if (Sn) {
    if (nf && ng) s_poly_device(ctx, df, nf, dg, ng, dS);
    else QG_HIP(hipMemsetAsync(dS, 0, Sn * sizeof(Fr), ctx->stream));
  }
  trim_launch(ctx, dS, Sn, d_len + 2);
  QG_HIP(hipMemcpyAsync(h_len, d_len, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        ctx->stream));
  // its commitment (ipa.rs:73), as mle_open_batch_device commits its S
  size_t s_msm = Sn;
  if (Sn > srs->n) {
    ctx->sync();
    s_msm = (size_t)h_len[2];
    QG_CHECK(s_msm <= srs->n, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
  }
  const G1Affine s_comm = msm_device(ctx, srs, dS, s_msm);
  ctx->sync();  // (drained already unless the MSM was empty)
  const Fr ip = *h_ip;
  const size_t Lf = fault_short_trim(ctx, (size_t)h_len[0]);
  const size_t Lg = fault_short_trim(ctx, (size_t)h_len[1]);
  const size_t Ls = fault_short_trim(ctx, (size_t)h_len[2]);
  const OpenChallenge ch = ipa_transcript_step(state, ip, s_comm);
  fr_export(ip, ip_out);
  g1_export(s_comm, s_comm_xy, s_comm_inf);
  return {dS, Sn, ip, Lf, Lg, Ls, ch};
}

static void ipa_prove_device(qg_ctx* ctx, const qg_srs* srs, const Fr* df, size_t nf,
                             const Fr* dg, size_t ng, uint8_t state[32], qg_ipa_proof* out) {
  const IpaFront F = ipa_front(ctx, srs, df, nf, dg, ng, state, out->inner_product,
                               out->s_comm_xy, &out->s_comm_inf);
  const OpenChallenge& ch = F.ch;
  // six KZG::open (ipa.rs:87-92): the quotients (job 2p + i: polynomial p of
  // f, g, S at r, 1/r), then their commitments as one MSM batch
  const Fr* polys[3] = {df, dg, F.dS};
  const size_t ns[3] = {nf, ng, F.Sn}, lts[3] = {F.Lf, F.Lg, F.Ls};
  const Open6 o6 = open6(*out);
  std::vector<QuotJob> jobs;
  for (int i = 0; i < 6; i++)
    jobs.push_back({polys[i >> 1], ns[i >> 1], lts[i >> 1], i & 1 ? ch.r_inv : ch.r, o6.o[i]});
  const QuotStage st = quotients_queue(ctx, jobs, 6, true);
  st.fit(srs);
  const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, st.qs, st.qns);
  ctx->sync();  // (drained already unless every quotient was empty)
  st.settle(ctx, IPA_QNAME);
  st.store(pis);
  ipa_check_equation(st.h_y, ch.r, ch.r_inv, F.ip);
}

// ---------------------------------------------------------------- folded inner-product argument
// f, g and S are opened at the same two points, so with gamma drawn after the
// six values y one quotient per point serves all three: the quotient of
// h = f + gamma g + gamma^2 S at x, checked against C_f + gamma C_g +
// gamma^2 s_comm (the folded ML opening's batching at P = 3; no counterpart in
// the reference).  3 MSMs (S, W_r, W_inv) instead of 7, two
// quotient vectors instead of six.  The first half is ipa_front; then the six
// values over the untrimmed vectors (region "fold_eval"), one host round trip,
// the six appends and gamma, one folded scan and one MSM batch.
// The values come from one two-point pass over each vector (poly_eval_queue<2>)
// or from two single passes (poly_eval_queue<1> at r, then at 1/r): the same
// bits.  QG_EVAL_PAIRED (read per call) selects: 1 the two-point kernel, 0 the
// two single calls.  Unset is the two-point kernel: measured
// (profiles/fold_ipa.json, DESIGN section 5 "Folded inner-product argument")
// its fold_eval region is 0.147 ms against 0.177 ms at 2^20 coefficients and
// 0.345 against 0.384 ms at 2^22, both beyond the spread of the repeated
// medians (0.010 and 0.022 ms).  With the one-point kernel an instance of the
// same template the single calls came down to 0.154 and 0.355 ms
// (profiles/eval_unify.json), within the spread of the two-point kernel's
// 0.154 and 0.345, which reads each vector once and stays the default.
static constexpr bool EVAL_PAIRED_DEFAULT = true;
static bool eval_paired_on() {
  const char* e = getenv("QG_EVAL_PAIRED");
  return e ? atoi(e) != 0 : EVAL_PAIRED_DEFAULT;
}

static void ipa_prove_folded_device(qg_ctx* ctx, const qg_srs* srs, const Fr* df, size_t nf,
                                    const Fr* dg, size_t ng, uint8_t state[32],
                                    qg_ipa_proof_folded* out) {
  memset(out, 0, sizeof *out);
  const IpaFront F = ipa_front(ctx, srs, df, nf, dg, ng, state, out->inner_product,
                               out->s_comm_xy, &out->s_comm_inf);
  const OpenChallenge& ch = F.ch;
  const bool check = open_check_on();
  Fr* d_y = ctx->scratch_as<Fr>("ipaf_y", 6);
  Fr* h_y = reinterpret_cast<Fr*>(ctx->pinned_get("ipaf_y_h", 6 * sizeof(Fr)));
  uint32_t* d_w = check ? ctx->scratch_as<uint32_t>("open_ck_w", 2) : nullptr;
  uint32_t* h_w = reinterpret_cast<uint32_t*>(ctx->pinned_get("open_ck_h", 2 * sizeof(uint32_t)));
  // fold_eval: {f, g, S} at two points, six rows of spans; the check's
  // {f, g, S, W_r, W_inv} at sigma are five
  poly_eval_reserve(ctx, 3, nf > ng ? nf : ng, 2);
  {
    // d_y[3 i + p] = polynomial p of f, g, S at r (i = 0), 1/r (i = 1)
    QgTimed tm(ctx, "fold_eval");
    const std::vector<EvIn> three = {{df, nf, 0}, {dg, ng, 0}, {F.dS, F.Sn, 0}};
    if (eval_paired_on()) {
      poly_eval_queue(ctx, three, {ch.r, ch.r_inv}, d_y);
    } else {
      poly_eval_queue(ctx, three, {ch.r}, d_y);
      poly_eval_queue(ctx, three, {ch.r_inv}, d_y + 3);
    }
    QG_HIP(hipMemcpyAsync(h_y, d_y, 6 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
  }
  ctx->sync();
  Fr y[6];  // IPA_QNAME order
  for (int i = 0; i < 6; i++) y[i] = h_y[3 * (i & 1) + (i >> 1)];
  ipa_check_equation(y, ch.r, ch.r_inv, F.ip);
  for (int i = 0; i < 6; i++) {
    uint8_t b32[32];
    fr_to_bytes(y[i], b32);
    transcript_append(state, b32, 32);
    fr_export(y[i], out->y[i]);
  }
  const Fr gamma = transcript_draw_fr(state);
  const size_t Lh = std::max(F.Lf, std::max(F.Lg, F.Ls));
  QG_CHECK(Lh <= srs->n + 1, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
  FoldScan fs{};
  fs.p[0] = df, fs.pn[0] = nf, fs.pl[0] = F.Lf, fs.g[0] = Fr::one();
  fs.p[1] = dg, fs.pn[1] = ng, fs.pl[1] = F.Lg, fs.g[1] = gamma;
  fs.p[2] = F.dS, fs.pn[2] = F.Sn, fs.pl[2] = F.Ls, fs.g[2] = gamma * gamma;
  fs.P = 3, fs.L = Lh, fs.nx = 2, fs.x[0] = ch.r, fs.x[1] = ch.r_inv;
  std::vector<const Fr*> qs(2, nullptr);
  std::vector<size_t> qns(2, 0);
  for (int p = 0; p < 2; p++) {
    fs.s[p] = Lh ? ctx->scratch_as<Fr>("open_s#" + std::to_string(p), Lh) : nullptr;
    qs[p] = Lh ? fs.s[p] + 1 : nullptr;
    qns[p] = Lh ? Lh - 1 : 0;
  }
  fold_scan_queue(ctx, fs, check ? d_y : nullptr, d_w);
  if (check)
    QG_HIP(hipMemcpyAsync(h_w, d_w, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, qs, qns);
  ctx->sync();  // (drained already unless both quotients were empty)
  if (check)
    open_check_settle(ctx, std::vector<uint32_t>(h_w, h_w + 2),
                      std::vector<uint8_t>(2, Lh ? CK_QUOT : CK_ZERO), 2, FOLD_QNAME);
  g1_export(pis[0], out->w_xy, &out->w_inf);
  g1_export(pis[1], out->w_inv_xy, &out->w_inv_inf);
}

// The local geometry of a sharded inner-product argument, decided from this
// rank's arguments alone (before the first collective): equal local lengths L,
// world a power of two <= SP_MAXW, world * L a power of two within the NTT's
// 2-adicity.  Returns log2(world * L).
static size_t ipa_sharded_geometry(qg_ctx* ctx, size_t nf, size_t ng) {
  const size_t W = (size_t)ctx->world;
  const size_t M = W * nf;
  size_t nvars = 0;
  while (((size_t)1 << nvars) < M && nvars < 27) nvars++;
  QG_CHECK(nf == ng && nf > 0 && W <= (size_t)SP_MAXW && (W & (W - 1)) == 0 &&
               M == ((size_t)1 << nvars),
           QG_ERR_UNSUPPORTED,
           "sharded inner-product argument needs nf == ng == L with world * L a power of two "
           "(at most 2^27) and world a power of two <= " + std::to_string(SP_MAXW));
  return nvars;
}

// InnerProductProof::prove with a communicator: this rank holds f[rank L,
// (rank+1) L) and g[rank L, (rank+1) L) of two global vectors of M = world L
// coefficients and the matching SRS shard.  The flow is
// mle_open_batch_sharded's with three polynomials and six quotients:
//   1. the local dot part and local trimmed lengths of f and g (queued);
//   2. f and g gathered (two allgathers), this rank's slice of S by
//      s_poly_sharded's general-g form (one all-to-all), its local length;
//   3. ONE allgather of every rank's dot part, three local lengths and shard
//      size: the inner product, the global trimmed lengths and - because every
//      rank then knows every rank's part lengths and bases - the "Polynomial
//      degree exceeds max degree" decision, the same on all ranks;
//   4. the S commitment (sharded MSM), the transcript step on every rank;
//   5. quotients_sharded on six jobs: the local suffix-Horner scans
//      (QG_IPA_PAIRED=1: three paired ones), ONE allgather of their slice-end
//      values T, the carries, the quotient check on the ranks' summed parts
//      (ONE allgather) and the six commitments as ONE sharded MSM batch;
//   6. ipa.rs:94-100.
// Every decision that ends the call is taken on gathered values, which all
// ranks hold alike, so no rank leaves between two collectives its peers enter.
// The scratch is the flow's own and s_poly_sharded's (sp_*): no transform the
// "ntt_F_src" memo describes is touched, so the memo stays.
// An all-zero operand needs no special case: its transform is exact zeros (the
// single path also skips only a stated length of 0, which has no sharded form).
static void ipa_prove_sharded(qg_ctx* ctx, const qg_srs* srs, const Fr* df, const Fr* dg, size_t L,
                              size_t nvars, uint8_t state[32], qg_ipa_proof* out) {
  const size_t W = (size_t)ctx->world, rank = (size_t)ctx->rank;
  const size_t M = W * L;
  struct Small {
    Fr part;
    unsigned long long len[3], srs_n;
  };
  Small* d_sm = ctx->scratch_as<Small>("ipas_small", 1);
  QG_HIP(hipMemsetAsync(d_sm, 0, sizeof(Small), ctx->stream));
  const unsigned long long my_n = srs->n;
  QG_HIP(hipMemcpyAsync(&d_sm->srs_n, &my_n, sizeof my_n, hipMemcpyHostToDevice, ctx->stream));
  dot_to_device(ctx, df, dg, L, &d_sm->part);
  trim_launch(ctx, df, L, &d_sm->len[0]);
  trim_launch(ctx, dg, L, &d_sm->len[1]);
  Fr* Sl = ctx->scratch_as<Fr>("ipas_Sl", L);
  if (M > 1) {
    Fr* ffull = ctx->scratch_as<Fr>("ipas_f", M);
    Fr* gfull = ctx->scratch_as<Fr>("ipas_g", M);
    comm_allgather_bytes(ctx, df, ffull, L * sizeof(Fr));
    comm_allgather_bytes(ctx, dg, gfull, L * sizeof(Fr));
    s_poly_sharded(ctx, ffull, M, nullptr, nvars, Sl, gfull);
  } else {
    QG_HIP(hipMemsetAsync(Sl, 0, L * sizeof(Fr), ctx->stream));  // M == 1: S is empty
  }
  trim_launch(ctx, Sl, L, &d_sm->len[2]);
  if (ctx->open_fault_live == 1) {  // test-only: this rank's first nonzero local length
    ctx->open_fault_live = 0;
    hipLaunchKernelGGL(k_fault_short_len, dim3(1), dim3(64), 0, ctx->stream, d_sm->len, (size_t)3,
                       (unsigned long long)ctx->open_fault_value);
    QG_LAUNCH_CHECK();
  }
  // exchange 1: dot parts, local lengths and shard sizes of every rank
  Small* d_all = ctx->scratch_as<Small>("ipas_small_all", W);
  comm_allgather_bytes(ctx, d_sm, d_all, sizeof(Small));
  std::vector<Small> all(W);
  QG_HIP(hipMemcpyAsync(all.data(), d_all, W * sizeof(Small), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  Fr ip = Fr::zero();
  size_t glt[3];  // global trimmed lengths of f, g, S
  std::vector<unsigned long long> shard(W), loc(W);
  for (size_t r = 0; r < W; r++) {
    ip = ip + all[r].part;
    shard[r] = all[r].srs_n;
  }
  for (int p = 0; p < 3; p++) {
    for (size_t r = 0; r < W; r++) loc[r] = all[r].len[p];
    glt[p] = op_global_len(loc.data(), W, L);
  }
  QG_CHECK(op_fits(glt[2], glt, 3, L, shard.data(), W), QG_ERR_INVALID,
           "Polynomial degree exceeds max degree");
  const G1Affine s_comm = msm_device_batch(ctx, srs, {Sl}, {op_live(glt[2], rank, L)})[0];
  // the transcript step on every rank alike, then the six quotients (job
  // 2p + i: polynomial p of f, g, S at r, 1/r) and ipa.rs:94-100
  const OpenChallenge ch = ipa_transcript_step(state, ip, s_comm);
  fr_export(ip, out->inner_product);
  g1_export(s_comm, out->s_comm_xy, &out->s_comm_inf);
  const Fr* polys[3] = {df, dg, Sl};
  const Open6 o6 = open6(*out);
  std::vector<ShardQuotJob> jobs;
  for (int i = 0; i < 6; i++)
    jobs.push_back({polys[i >> 1], L, glt[i >> 1], i & 1 ? ch.r_inv : ch.r, o6.o[i]});
  const std::vector<Fr> y = quotients_sharded(ctx, srs, jobs, 6, true, IPA_QNAME);
  ipa_check_equation(y.data(), ch.r, ch.r_inv, ip);
}

}  // namespace qg

extern "C" {

int qg_poly_eval_dev(qg_ctx* ctx, const qg_buf* poly, size_t n, const uint64_t x[4],
                     uint64_t shift, uint64_t out[4]) {
  if (!ctx || !poly || n > poly->n || !x || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    Fr* d = ctx->scratch_as<Fr>("ev_out", 1);
    poly_eval_queue(ctx, {{poly->d, n, shift}}, {fr_import(x)}, d);
    Fr r;
    QG_HIP(hipMemcpyAsync(&r, d, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    fr_export(r, out);
  });
}

int qg_debug_open_fault(qg_ctx* ctx, uint32_t kind, uint64_t value) {
  if (!ctx || kind > 3) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    ctx->open_fault_armed = kind == 3 ? 0 : kind;
    ctx->open_fault_value = value;
    if (kind == 3) {  // poison trim_launch's stamp word (nothing else remains of the stamp)
      unsigned long long* tail = ctx->scratch_as<unsigned long long>("trim_tail", 1);
      const unsigned long long v = value;
      QG_HIP(hipMemcpyAsync(tail, &v, sizeof v, hipMemcpyHostToDevice, ctx->stream));
      ctx->sync();
    }
  });
}

int qg_inner_product(qg_ctx* ctx, const uint64_t* f, size_t nf, const uint64_t* g, size_t ng,
                     uint64_t out[4]) {
  if (!ctx || (!f && nf) || (!g && ng) || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    size_t n = nf < ng ? nf : ng;
    Fr* df = ctx->scratch_as<Fr>("ip_f", n ? n : 1);
    Fr* dg = ctx->scratch_as<Fr>("ip_g", n ? n : 1);
    fr_upload(ctx, df, f, n);
    fr_upload(ctx, dg, g, n);
    fr_export(dot_device(ctx, df, dg, n), out);
  });
}

int qg_s_polynomial(qg_ctx* ctx, const uint64_t* f, size_t nf, const uint64_t* g, size_t ng,
                    uint64_t* out) {
  if (!ctx || (!f && nf) || (!g && ng) || (!out && (nf > 1 || ng > 1))) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    const size_t M = nf > ng ? nf : ng;
    if (M <= 1) return;
    Fr* df = ctx->scratch_as<Fr>("sp_f", nf ? nf : 1);
    Fr* dg = ctx->scratch_as<Fr>("sp_g", ng ? ng : 1);
    Fr* dS = ctx->scratch_as<Fr>("sp_S", M - 1);
    fr_upload(ctx, df, f, nf);
    fr_upload(ctx, dg, g, ng);
    s_poly_device(ctx, df, nf, dg, ng, dS);
    fr_download(ctx, out, dS, M - 1);
    ctx->sync();
  });
}

int qg_kzg_open(qg_ctx* ctx, const qg_srs* srs, const uint64_t* poly, size_t n, const uint64_t x[4],
                qg_kzg_opening* out) {
  if (!ctx || !srs || (!poly && n) || !x || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    Fr* d = ctx->scratch_as<Fr>("open_in", n ? n : 1);
    fr_upload(ctx, d, poly, n);
    kzg_open_device(ctx, srs, d, n, fr_import(x), out);
  });
}

int qg_mle_open(qg_ctx* ctx, const qg_srs* srs, const uint64_t* poly, size_t n,
                const uint64_t* point, size_t nvars, uint8_t state[32], qg_mle_proof* out) {
  if (!ctx || !srs || (!poly && n) || (!point && nvars) || !state || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(nvars <= 30, QG_ERR_INVALID, "too many variables");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    Fr* dpoly = ctx->scratch_as<Fr>("mle_poly", n ? n : 1);
    fr_upload(ctx, dpoly, poly, n);
    mle_open_device(ctx, srs, dpoly, n, point, nvars, state, out);
  });
}

int qg_mle_open_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                    const uint64_t* point, size_t nvars, uint8_t state[32], qg_mle_proof* out) {
  if (!ctx || !srs || !poly || n > poly->n || (!point && nvars) || !state || !out)
    return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(nvars <= 30, QG_ERR_INVALID, "too many variables");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    mle_open_device(ctx, srs, poly->d, n, point, nvars, state, out);
  });
}

int qg_mle_open_batch_dev(qg_ctx* ctx, const qg_srs* srs, const qg_mle_open_item* items,
                          size_t k, uint8_t state[32], qg_mle_proof* outs) {
  if (!ctx || !srs || (!items && k) || !state || (!outs && k)) return QG_ERR_INVALID;
  for (size_t i = 0; i < k; i++)
    if (!items[i].poly || items[i].n > items[i].poly->n || (!items[i].point && items[i].nvars) ||
        items[i].nvars > 30 || (items[i].flags & ~(uint32_t)QG_OPEN_UNCHANGED))
      return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(k <= 256, QG_ERR_UNSUPPORTED, "too many openings in one batch (at most 256)");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    std::vector<MleOpenItem> v(k);
    for (size_t i = 0; i < k; i++)
      v[i] = {items[i].poly->d, items[i].n, items[i].point, items[i].nvars,
              (items[i].flags & QG_OPEN_UNCHANGED) != 0, items[i].poly->alloc_id,
              items[i].poly->base_off};
    mle_open_batch_device(ctx, srs, v, state, outs);
  });
}

int qg_mle_open_dev_ex(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                       const uint64_t* point, size_t nvars, uint8_t state[32], uint32_t flags,
                       qg_mle_proof* out) {
  if (!ctx || !srs || !poly || n > poly->n || (!point && nvars) || !state || !out ||
      (flags & ~(uint32_t)QG_OPEN_UNCHANGED))
    return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(nvars <= 30, QG_ERR_INVALID, "too many variables");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    mle_open_device(ctx, srs, poly->d, n, point, nvars, state, out,
                    (flags & QG_OPEN_UNCHANGED) != 0, poly->alloc_id, poly->base_off);
  });
}

// The folded entries are single-context: decided before OpenCall (collective on
// a sharded context) and before any device work.
static void fold_entry_checks(qg_ctx* ctx, const char* what) {
  QG_CHECK(!ctx->sharded, QG_ERR_UNSUPPORTED,
           std::string(what) + " is not supported on a sharded context (communicator "
           "attached): the folded opening runs on a single context");
}

int qg_mle_open_folded_batch_dev(qg_ctx* ctx, const qg_srs* srs, const qg_mle_open_item* items,
                                 size_t k, uint8_t state[32], qg_mle_proof_folded* outs) {
  if (!ctx || !srs || (!items && k) || !state || (!outs && k)) return QG_ERR_INVALID;
  for (size_t i = 0; i < k; i++)
    if (!items[i].poly || items[i].n > items[i].poly->n || (!items[i].point && items[i].nvars) ||
        items[i].nvars > 30 || (items[i].flags & ~(uint32_t)QG_OPEN_UNCHANGED))
      return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    fold_entry_checks(ctx, "qg_mle_open_folded_batch_dev");
    QG_CHECK(k <= 256, QG_ERR_UNSUPPORTED, "too many openings in one batch (at most 256)");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    std::vector<MleOpenItem> v(k);
    for (size_t i = 0; i < k; i++)
      v[i] = {items[i].poly->d, items[i].n, items[i].point, items[i].nvars,
              (items[i].flags & QG_OPEN_UNCHANGED) != 0, items[i].poly->alloc_id,
              items[i].poly->base_off};
    mle_open_folded_batch_device(ctx, srs, v, state, outs);
  });
}

int qg_mle_open_folded_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                           const uint64_t* point, size_t nvars, uint8_t state[32], uint32_t flags,
                           qg_mle_proof_folded* out) {
  if (!ctx || !srs || !poly || n > poly->n || (!point && nvars) || !state || !out ||
      (flags & ~(uint32_t)QG_OPEN_UNCHANGED))
    return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    fold_entry_checks(ctx, "qg_mle_open_folded_dev");
    QG_CHECK(nvars <= 30, QG_ERR_INVALID, "too many variables");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    mle_open_folded_batch_device(ctx, srs,
                                 {{poly->d, n, point, nvars, (flags & QG_OPEN_UNCHANGED) != 0,
                                   poly->alloc_id, poly->base_off}},
                                 state, out);
  });
}

int qg_kzg_open_lincomb_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* const* polys,
                            const size_t* lens, const uint64_t* coeffs, size_t P,
                            const uint64_t* xs, size_t nx, qg_kzg_opening* outs) {
  if (!ctx || !srs || !polys || !lens || !coeffs || !xs || !outs || P < 1 || P > (size_t)SHF_P ||
      nx < 1 || nx > 2)
    return QG_ERR_INVALID;
  for (size_t j = 0; j < P; j++)
    if (!polys[j] || lens[j] > polys[j]->n) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    fold_entry_checks(ctx, "qg_kzg_open_lincomb_dev");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    // KZG::open trims what it is given (kzg.rs:77): the scan runs over the
    // largest trimmed source length (zero tail coefficients of h beyond its own
    // degree only append zero quotient coefficients)
    unsigned long long* d_len = ctx->scratch_as<unsigned long long>("fold_len", SHF_P);
    unsigned long long h_len[SHF_P] = {0, 0, 0, 0};
    QG_HIP(hipMemsetAsync(d_len, 0, SHF_P * sizeof(unsigned long long), ctx->stream));
    for (size_t j = 0; j < P; j++) trim_launch(ctx, polys[j]->d, lens[j], d_len + j);
    QG_HIP(hipMemcpyAsync(h_len, d_len, sizeof h_len, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    FoldScan fs{};
    fs.P = (int)P, fs.nx = (int)nx;
    size_t nmax = 0;
    for (size_t j = 0; j < P; j++) {
      fs.p[j] = polys[j]->d, fs.pn[j] = lens[j];
      fs.pl[j] = fault_short_trim(ctx, (size_t)h_len[j]);
      fs.g[j] = fr_import(coeffs + 4 * j);
      fs.L = std::max(fs.L, fs.pl[j]);
      nmax = std::max(nmax, lens[j]);
    }
    const bool check = open_check_on();
    std::vector<const Fr*> qs(nx, nullptr);
    std::vector<size_t> qns(nx, 0);
    Fr* d_y = ctx->scratch_as<Fr>("open_y", 2);
    Fr* h_y = reinterpret_cast<Fr*>(ctx->pinned_get("open_y_h", 2 * sizeof(Fr)));
    uint32_t* d_w = check ? ctx->scratch_as<uint32_t>("open_ck_w", 2) : nullptr;
    uint32_t* h_w = reinterpret_cast<uint32_t*>(ctx->pinned_get("open_ck_h", 2 * sizeof(uint32_t)));
    if (check) poly_eval_reserve(ctx, P + nx, nmax, 1);
    QG_HIP(hipMemsetAsync(d_y, 0, 2 * sizeof(Fr), ctx->stream));
    for (size_t p = 0; p < nx; p++) {
      fs.x[p] = fr_import(xs + 4 * p);
      fs.s[p] = fs.L ? ctx->scratch_as<Fr>("open_s#" + std::to_string(p), fs.L) : nullptr;
      qs[p] = fs.L ? fs.s[p] + 1 : nullptr, qns[p] = fs.L ? fs.L - 1 : 0;
    }
    fold_scan_queue(ctx, fs, nullptr, d_w);
    for (size_t p = 0; p < nx; p++)
      if (fs.L)
        QG_HIP(hipMemcpyAsync(d_y + p, fs.s[p], sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    QG_HIP(hipMemcpyAsync(h_y, d_y, 2 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    if (check)
      QG_HIP(hipMemcpyAsync(h_w, d_w, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    // kzg_open_device's order: the check settles before the degree is judged
    ctx->sync();
    if (check) {
      const uint8_t c = fs.L ? CK_QUOT : nmax ? CK_ZERO : CK_NONE;
      open_check_settle(ctx, std::vector<uint32_t>(h_w, h_w + nx), std::vector<uint8_t>(nx, c), nx,
                        FOLD_XNAME);
    }
    for (size_t n : qns)
      QG_CHECK(n <= srs->n, QG_ERR_INVALID, "Polynomial degree exceeds max degree");
    const std::vector<G1Affine> pis = msm_device_batch(ctx, srs, qs, qns);
    ctx->sync();
    for (size_t p = 0; p < nx; p++) {
      fr_export(fs.x[p], outs[p].x);
      fr_export(h_y[p], outs[p].y);
      g1_export(pis[p], outs[p].proof_xy, &outs[p].proof_inf);
    }
  });
}

// The entry checks run before OpenCall, whose constructor is collective on a
// sharded context: a rank that fails one leaves no peer waiting.
// The host-pointer entry stays single-context: a sharded caller holds device
// blocks and calls qg_ipa_prove_dev.
static void ipa_host_entry_checks(qg_ctx* ctx, size_t nf, size_t ng) {
  QG_CHECK(!ctx->sharded, QG_ERR_UNSUPPORTED,
           "the host-pointer inner-product argument is not supported on a sharded context "
           "(communicator attached): pass device blocks to qg_ipa_prove_dev");
  QG_CHECK(nf || ng, QG_ERR_INVALID, "inner-product argument of two empty polynomials");
}
// the device entry: returns log2(world * L) on a sharded context (0 otherwise)
static size_t ipa_dev_entry_checks(qg_ctx* ctx, size_t nf, size_t ng) {
  QG_CHECK(nf || ng, QG_ERR_INVALID, "inner-product argument of two empty polynomials");
  return ctx->sharded ? ipa_sharded_geometry(ctx, nf, ng) : 0;
}

int qg_ipa_prove(qg_ctx* ctx, const qg_srs* srs, const uint64_t* f, size_t nf, const uint64_t* g,
                 size_t ng, uint8_t state[32], qg_ipa_proof* out) {
  if (!ctx || !srs || (!f && nf) || (!g && ng) || !state || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    ipa_host_entry_checks(ctx, nf, ng);
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    Fr* df = ctx->scratch_as<Fr>("ipa_f", nf ? nf : 1);
    Fr* dg = ctx->scratch_as<Fr>("ipa_g", ng ? ng : 1);
    fr_upload(ctx, df, f, nf);
    fr_upload(ctx, dg, g, ng);
    ipa_prove_device(ctx, srs, df, nf, dg, ng, state, out);
  });
}

int qg_ipa_prove_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* f, size_t nf, const qg_buf* g,
                     size_t ng, uint8_t state[32], qg_ipa_proof* out) {
  if (!ctx || !srs || !f || !g || nf > f->n || ng > g->n || !state || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    const size_t nvars = ipa_dev_entry_checks(ctx, nf, ng);
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    if (ctx->sharded) ipa_prove_sharded(ctx, srs, f->d, g->d, nf, nvars, state, out);
    else ipa_prove_device(ctx, srs, f->d, nf, g->d, ng, state, out);
  });
}

// The folded entries: qg_ipa_prove[_dev]'s argument checks; a sharded context
// is refused before OpenCall (collective there) and before any device work.
int qg_ipa_prove_folded(qg_ctx* ctx, const qg_srs* srs, const uint64_t* f, size_t nf,
                        const uint64_t* g, size_t ng, uint8_t state[32],
                        qg_ipa_proof_folded* out) {
  if (!ctx || !srs || (!f && nf) || (!g && ng) || !state || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    fold_entry_checks(ctx, "qg_ipa_prove_folded");
    QG_CHECK(nf || ng, QG_ERR_INVALID, "inner-product argument of two empty polynomials");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    Fr* df = ctx->scratch_as<Fr>("ipa_f", nf ? nf : 1);
    Fr* dg = ctx->scratch_as<Fr>("ipa_g", ng ? ng : 1);
    fr_upload(ctx, df, f, nf);
    fr_upload(ctx, dg, g, ng);
    ipa_prove_folded_device(ctx, srs, df, nf, dg, ng, state, out);
  });
}

int qg_ipa_prove_folded_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* f, size_t nf,
                            const qg_buf* g, size_t ng, uint8_t state[32],
                            qg_ipa_proof_folded* out) {
  if (!ctx || !srs || !f || !g || nf > f->n || ng > g->n || !state || !out) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(nf || ng, QG_ERR_INVALID, "inner-product argument of two empty polynomials");
    fold_entry_checks(ctx, "qg_ipa_prove_folded_dev");
    QG_HIP(hipSetDevice(ctx->device));
    OpenCall call(ctx);
    ipa_prove_folded_device(ctx, srs, f->d, nf, g->d, ng, state, out);
  });
}

int qg_poly_eval2_dev(qg_ctx* ctx, const qg_buf* const* polys, const size_t* lens, size_t P,
                      const uint64_t* xs, uint64_t* out) {
  if (!ctx || !polys || !lens || !xs || !out || P < 1 || P > (size_t)EV_MAXJ)
    return QG_ERR_INVALID;
  for (size_t j = 0; j < P; j++)
    if (!polys[j] || lens[j] > polys[j]->n) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    QG_CHECK(!ctx->sharded, QG_ERR_UNSUPPORTED,
             "qg_poly_eval2_dev is not supported on a sharded context (communicator attached)");
    QG_HIP(hipSetDevice(ctx->device));
    Fr* d = ctx->scratch_as<Fr>("ev2_out", 2 * EV_MAXJ);
    std::vector<EvIn> in;
    for (size_t j = 0; j < P; j++) in.push_back({polys[j]->d, lens[j], 0});
    poly_eval_queue(ctx, in, {fr_import(xs), fr_import(xs + 4)}, d);
    Fr r[2 * EV_MAXJ];
    QG_HIP(hipMemcpyAsync(r, d, 2 * P * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    for (size_t k = 0; k < 2 * P; k++) fr_export(r[k], out + 4 * k);
  });
}

}  // extern "C"
