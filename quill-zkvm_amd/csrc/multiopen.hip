// Streaming kernels of the multi-point batch opening (HyperPlonk paper, 3.8;
// quill_amd/multiopen.py composes the protocol over them):
//   qg_eq_multi_dev        out[x] = sum_i w_i eq(bin(x), z_i)
//   qg_mle_eval_multi_dev  out[i] = sum_x poly[x] eq(bin(x), z_i)
//   qg_lincomb_dev         out[x] = sum_j c_j f_j[x]
//
// Both eq kernels split x = x_hi 2^lb + x_lo and use eq(x, z) = eq(x_lo, z_lo)
// eq(x_hi, z_hi): per point a low table (2^lb entries) and a high table (2^hb)
// in scratch, all k points by one launch of k_eq_parts.  lb is chosen so that
// the 256 entries a block covers share one x_hi (lb >= 8, or hb = 0 below 2^8
// entries): the high factors are block-uniform, and there is one code path for
// every nvars.  No full eq table is ever materialised.
//
// Arithmetic: the 9 x 29-bit limbs of field29.h, mul29(a, b) = a b 2^-261.  HBM
// keeps Montgomery words with R = 2^256, so one factor of every product is
// pre-scaled by 2^5 on the way into its table (x 2^256 times y 2^261 gives
// x y 2^256): no conversion multiply in the streaming loops.  Sums are lazy
// limb additions with one parallel carry pass each, reduced once (red128p29).
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "field29.h"

using namespace qg;

namespace qg {
namespace {

using R29 = F29<FrP>;
constexpr uint32_t MO_BLOCK = 256;
constexpr uint32_t MO_KMAX = 256;   // points per call
constexpr uint32_t MO_PMAX = 16;    // vectors per linear combination
constexpr uint32_t MO_ROWS = 4;     // x_hi rows of one k_mle_multi tile
constexpr uint32_t MO_MAXBLOCKS = 1024;

// 32-byte Fr as two 16-byte accesses (qg_buf data and views are 32-byte aligned)
QG_DEV Fr ld_fr(const Fr* p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
QG_DEV void st_fr(Fr* p, const Fr& r) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// Low and high eq tables of all k points: low[i][r] = ls eq(bin(r), z_i[0..lb)),
// high[i][r] = hs[i] eq(bin(r), z_i[lb..lb+hb))   (the loop of k_eq_small)
__global__ void k_eq_parts(const Fr* __restrict__ z, const Fr* __restrict__ hs,
                           const Fr* __restrict__ ls, uint32_t k, uint32_t lb, uint32_t hb,
                           Fr* __restrict__ low, Fr* __restrict__ high) {
  const size_t NL = (size_t)1 << lb, NH = (size_t)1 << hb, per = NL + NH;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per * k) return;
  const uint32_t i = (uint32_t)(idx / per);
  size_t r = idx % per;
  const bool hi = r >= NL;
  if (hi) r -= NL;
  const Fr* zi = z + (size_t)i * (lb + hb) + (hi ? lb : 0);
  const uint32_t nbits = hi ? hb : lb;
  Fr acc = hi ? hs[i] : *ls;
  for (uint32_t j = 0; j < nbits; j++) {
    const Fr zj = zi[j];
    acc = acc * (((r >> j) & 1) ? zj : (Fr::one() - zj));
  }
  if (hi)
    high[(size_t)i * NH + r] = acc;
  else
    low[(size_t)i * NL + r] = acc;
}

// out[x] = sum_i low_i[x_lo] high_i[x_hi]; high carries w_i 2^5.  A block covers
// 256 consecutive x of one x_hi: the k high factors go to LDS once, the k low
// rows are read coalesced (they stay in L2), k products per element.
__global__ __launch_bounds__(MO_BLOCK) void k_eq_multi(const Fr* __restrict__ low,
                                                        const Fr* __restrict__ high, uint32_t k,
                                                        uint32_t lb, uint32_t hb, size_t n,
                                                        Fr* __restrict__ out) {
  __shared__ R29 H[MO_KMAX];
  const size_t x0 = (size_t)blockIdx.x * MO_BLOCK, x = x0 + threadIdx.x;
  const size_t NL = (size_t)1 << lb, NH = (size_t)1 << hb;
  const size_t xh = x0 >> lb, xl = x & (NL - 1);
  if (threadIdx.x < k) H[threadIdx.x] = to29(ld_fr(high + (size_t)threadIdx.x * NH + xh));
  __syncthreads();
  if (x >= n) return;
  R29 acc = R29::zero();
  uint32_t pending = 0;  // products (< 2p each) in acc since the last reduction
  for (uint32_t i = 0; i < k; i++) {
    acc = norm29(add29(acc, mul29(to29(ld_fr(low + (size_t)i * NL + xl)), H[i])));
    if (++pending == 62) {  // 2p + 62 * 2p < 128p
      acc = red128p29<FrP>(acc);
      pending = 0;
    }
  }
  st_fr(out + x, from29(canon29(red128p29<FrP>(acc))));
}

// Stage 1 of out[i] = sum_x poly[x] low_i[x_lo] high_i[x_hi] (both tables carry
// 2^5).  A tile is 256 x_lo by MO_ROWS x_hi; a thread loads its MO_ROWS entries
// of poly once, and per point sums them against the block-uniform high factors,
// multiplies by its low entry and adds into the wave sum.  Thread i of the
// block owns point i's running sum over the tiles of the block; the block
// writes k partial sums (canonical words) at the end.
__global__ __launch_bounds__(MO_BLOCK) void k_mle_multi(const Fr* __restrict__ poly,
                                                         const Fr* __restrict__ low,
                                                         const Fr* __restrict__ high, uint32_t k,
                                                         uint32_t lb, uint32_t hb,
                                                         Fr* __restrict__ partial) {
  constexpr uint32_t NW = MO_BLOCK / 64;
  __shared__ R29 red[NW][MO_KMAX];
  const size_t NL = (size_t)1 << lb, NH = (size_t)1 << hb;
  const size_t CL = (NL + MO_BLOCK - 1) / MO_BLOCK, CH = (NH + MO_ROWS - 1) / MO_ROWS;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  R29 own = R29::zero();  // point threadIdx.x, < 2p
  for (size_t tile = blockIdx.x; tile < CL * CH; tile += gridDim.x) {
    const size_t xl = (tile % CL) * MO_BLOCK + threadIdx.x, h0 = (tile / CL) * MO_ROWS;
    const bool live = xl < NL;
    const size_t xlc = live ? xl : NL - 1;
    R29 p[MO_ROWS];
#pragma unroll
    for (uint32_t t = 0; t < MO_ROWS; t++)
      p[t] = (live && h0 + t < NH) ? to29(ld_fr(poly + ((h0 + t) << lb) + xl)) : R29::zero();
    for (uint32_t i = 0; i < k; i++) {
      const Fr* hrow = high + (size_t)i * NH;
      R29 s = R29::zero();
#pragma unroll
      for (uint32_t t = 0; t < MO_ROWS; t++) {
        const size_t xh = h0 + t < NH ? h0 + t : NH - 1;  // a dead row's p is zero
        s = add29(s, mul29(p[t], to29(ld_fr(hrow + xh))));  // MO_ROWS terms < 2p: limbs < 2^32
      }
      R29 v = mul29(red16p29<FrP>(s), to29(ld_fr(low + (size_t)i * NL + xlc)));
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v = norm29(add29(v, shfl_xor29(v, m)));  // < 128p
      if (lane == 0) red[wid][i] = red128p29<FrP>(v);
    }
    __syncthreads();
    if (threadIdx.x < k) {
      R29 a = own;
#pragma unroll
      for (uint32_t w = 0; w < NW; w++) a = add29(a, red[w][threadIdx.x]);  // < 10p
      own = red16p29<FrP>(a);
    }
    __syncthreads();
  }
  if (threadIdx.x < k) st_fr(partial + (size_t)blockIdx.x * k + threadIdx.x, from29(canon29(own)));
}

// Stage 2: out[i] = sum over the nb <= 1024 partial sums of point i (one wave
// per point; a lane adds at most 16 canonical values lazily)
__global__ __launch_bounds__(64) void k_mle_multi_sum(const Fr* __restrict__ partial, uint32_t nb,
                                                      uint32_t k, Fr* __restrict__ out) {
  const uint32_t i = blockIdx.x;
  R29 a = R29::zero();
  for (uint32_t b = threadIdx.x; b < nb; b += 64)
    a = norm29(add29(a, to29(ld_fr(partial + (size_t)b * k + i))));  // < 16p
  a = red16p29<FrP>(a);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a = norm29(add29(a, shfl_xor29(a, m)));  // < 128p
  if (threadIdx.x == 0) st_fr(out + i, from29(canon29(red128p29<FrP>(a))));
}

struct LinArgs {
  const Fr* src[MO_PMAX];
  R29 c[MO_PMAX];  // coefficient x 2^5 (the 2^261 domain)
  uint32_t P;
};

// out[x] = sum_j c_j src_j[x]: P coalesced reads, one write, P products
__global__ __launch_bounds__(MO_BLOCK) void k_lincomb(const LinArgs a, size_t n,
                                                       Fr* __restrict__ out) {
  const size_t x = (size_t)blockIdx.x * MO_BLOCK + threadIdx.x;
  if (x >= n) return;
  R29 acc = R29::zero();
  for (uint32_t j = 0; j < a.P; j++)
    acc = norm29(add29(acc, mul29(to29(ld_fr(a.src[j] + x)), a.c[j])));  // < 32p
  st_fr(out + x, from29(canon29(red128p29<FrP>(acc))));
}

// x 2^5 (Montgomery words: the integer becomes x 2^261 mod p)
Fr times32(Fr x) {
  for (int i = 0; i < 5; i++) x = x + x;
  return x;
}

struct Split {
  uint32_t lb, hb;
};
Split eq_split(uint32_t nvars) {
  const uint32_t lb = nvars < 8 ? nvars : std::max(nvars / 2, 8u);
  return {lb, nvars - lb};
}

// uploads the k points and the per-point high scales, then fills the low and
// high tables (scratch slots "mo_low" / "mo_high") of all k points
void eq_parts_device(qg_ctx* ctx, const uint64_t* points, const std::vector<Fr>& hscale,
                     const Fr& lscale, uint32_t k, uint32_t nvars, Fr** low, Fr** high) {
  const Split s = eq_split(nvars);
  const size_t NL = (size_t)1 << s.lb, NH = (size_t)1 << s.hb;
  Fr* d_z = ctx->scratch_as<Fr>("mo_z", (size_t)k * nvars);
  Fr* d_s = ctx->scratch_as<Fr>("mo_scale", (size_t)k + 1);
  *low = ctx->scratch_as<Fr>("mo_low", NL * k);
  *high = ctx->scratch_as<Fr>("mo_high", NH * k);
  Fr* h_s = static_cast<Fr*>(ctx->pinned_get("mo_scale", ((size_t)k + 1) * sizeof(Fr)));
  for (uint32_t i = 0; i < k; i++) h_s[i] = hscale[i];
  h_s[k] = lscale;
  fr_upload(ctx, d_z, points, (size_t)k * nvars);
  QG_HIP(hipMemcpyAsync(d_s, h_s, ((size_t)k + 1) * sizeof(Fr), hipMemcpyHostToDevice,
                        ctx->stream));
  hipLaunchKernelGGL(k_eq_parts, dim3(div_up((NL + NH) * k, MO_BLOCK)), dim3(MO_BLOCK), 0,
                     ctx->stream, d_z, d_s, d_s + k, k, s.lb, s.hb, *low, *high);
  QG_LAUNCH_CHECK();
}

void entry_checks(qg_ctx* ctx, const char* what) {
  QG_HIP(hipSetDevice(ctx->device));
  QG_CHECK(!ctx->sharded, QG_ERR_UNSUPPORTED,
           std::string(what) + " runs on a single context (no communicator attached)");
}

}  // namespace

// out[x] = sum_{j<P} coeffs[j] src[j][x] for x < n, queued on the context
// stream (coeffs Montgomery; the folded opening's unfused route, mlpcs.hip)
void lincomb_queue(qg_ctx* ctx, const Fr* const* src, const Fr* coeffs, size_t P, size_t n,
                   Fr* out) {
  QG_CHECK(P >= 1 && P <= (size_t)MO_PMAX, QG_ERR_ASSERT, "lincomb of 1 to 16 vectors");
  if (n == 0) return;
  LinArgs a{};
  a.P = (uint32_t)P;
  for (size_t j = 0; j < P; j++) a.src[j] = src[j], a.c[j] = to29(times32(coeffs[j]));
  QgTimed tm(ctx, "lincomb");
  hipLaunchKernelGGL(k_lincomb, dim3(div_up(n, MO_BLOCK)), dim3(MO_BLOCK), 0, ctx->stream, a, n,
                     out);
  QG_LAUNCH_CHECK();
}
}  // namespace qg

extern "C" {

int qg_eq_multi_dev(qg_ctx* ctx, const uint64_t* points, const uint64_t* weights, size_t k,
                    size_t nvars, qg_buf* out) {
  if (!ctx || !points || !weights || !out || k < 1 || k > MO_KMAX || nvars < 1 || nvars > 40 ||
      ((size_t)1 << nvars) > out->n)
    return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    entry_checks(ctx, "qg_eq_multi_dev");
    const size_t n = (size_t)1 << nvars;
    const Split s = eq_split((uint32_t)nvars);
    std::vector<Fr> hs(k);
    for (size_t i = 0; i < k; i++) hs[i] = times32(fr_import(weights + 4 * i));
    {
      QgTimed tm(ctx, "eq_multi");
      Fr *low, *high;
      eq_parts_device(ctx, points, hs, Fr::one(), (uint32_t)k, (uint32_t)nvars, &low, &high);
      hipLaunchKernelGGL(k_eq_multi, dim3(div_up(n, MO_BLOCK)), dim3(MO_BLOCK), 0, ctx->stream,
                         low, high, (uint32_t)k, s.lb, s.hb, n, out->d);
      QG_LAUNCH_CHECK();
    }
    ctx->sync();
  });
}

int qg_mle_eval_multi_dev(qg_ctx* ctx, const qg_buf* poly, size_t n, const uint64_t* points,
                          size_t k, size_t nvars, uint64_t* out) {
  if (!ctx || !poly || !points || !out || k < 1 || k > MO_KMAX || nvars < 1 || nvars > 40 ||
      n != ((size_t)1 << nvars) || n > poly->n)
    return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    entry_checks(ctx, "qg_mle_eval_multi_dev");
    const Split s = eq_split((uint32_t)nvars);
    const size_t NL = (size_t)1 << s.lb, NH = (size_t)1 << s.hb;
    const size_t tiles = div_up(NL, MO_BLOCK) * (size_t)div_up(NH, MO_ROWS);
    const uint32_t nb = (uint32_t)std::min<size_t>(tiles, MO_MAXBLOCKS);
    const Fr c32 = times32(Fr::one());
    std::vector<Fr> hs(k, c32);
    Fr* partial = ctx->scratch_as<Fr>("mo_partial", (size_t)nb * k);
    Fr* d_out = ctx->scratch_as<Fr>("mo_out", k);
    {
      QgTimed tm(ctx, "mle_eval_multi");
      Fr *low, *high;
      eq_parts_device(ctx, points, hs, c32, (uint32_t)k, (uint32_t)nvars, &low, &high);
      hipLaunchKernelGGL(k_mle_multi, dim3(nb), dim3(MO_BLOCK), 0, ctx->stream, poly->d, low, high,
                         (uint32_t)k, s.lb, s.hb, partial);
      QG_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_mle_multi_sum, dim3((uint32_t)k), dim3(64), 0, ctx->stream, partial, nb,
                         (uint32_t)k, d_out);
      QG_LAUNCH_CHECK();
    }
    fr_download(ctx, out, d_out, k);
    ctx->sync();
  });
}

int qg_lincomb_dev(qg_ctx* ctx, const qg_buf* const* bufs, const uint64_t* coeffs, size_t P,
                   size_t n, qg_buf* out) {
  if (!ctx || !bufs || !coeffs || !out || P < 1 || P > MO_PMAX || n < 1 || n > out->n)
    return QG_ERR_INVALID;
  for (size_t j = 0; j < P; j++)
    if (!bufs[j] || n > bufs[j]->n || ranges_overlap(out->d, n, bufs[j]->d, n))
      return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    entry_checks(ctx, "qg_lincomb_dev");
    LinArgs a{};
    a.P = (uint32_t)P;
    for (size_t j = 0; j < P; j++) {
      a.src[j] = bufs[j]->d;
      a.c[j] = to29(times32(fr_import(coeffs + 4 * j)));
    }
    {
      QgTimed tm(ctx, "lincomb");
      hipLaunchKernelGGL(k_lincomb, dim3(div_up(n, MO_BLOCK)), dim3(MO_BLOCK), 0, ctx->stream, a,
                         n, out->d);
      QG_LAUNCH_CHECK();
    }
    ctx->sync();
  });
}

}  // extern "C"
