// SRS import / export as ark-serialize bytes, validated on the device, and the
// powers-of-tau check of an imported SRS.
//
// The reference has no SRS persistence (pcs/src/kzg.rs:35-59 makes a fresh
// random setup per run); a deployment brings its SRS as a file of
// CanonicalSerialize'd G1Affine points.  qg_srs_upload takes trusted
// Montgomery limbs and checks nothing; here every point is decoded,
// decompressed (one Fq square root, y = (x^3 + 3)^((p+1)/4), p = 3 mod 4) and
// checked by one thread, in the 9 x 29-bit-limb field of field29.h, and the
// first bad point is reported by index and reason.
#include <string.h>

#include <random>

#include "blake3.h"
#include "common.h"
#include "curve29.h"
#include "srs_io.h"

using namespace qg;

namespace qg {

// ---- constants of the decode (plain integers and R = 2^261 residues) -------
constexpr L9 l9_reduce_small(L9 x, const L9& p) {  // x < 4p -> x mod p
  for (int k = 0; k < 3; k++)
    if (l9_geq(x, p)) x = l9_sub(x, p);
  return x;
}
constexpr L9 l9_half_up(const L9& p) {  // (p + 1) / 2 for odd p
  L9 r{};
  for (int i = 0; i < 9; i++) {
    const uint32_t lo = i + 1 < 9 ? (p.v[i + 1] & 1u) : 0u;
    r.v[i] = (p.v[i] >> 1) | (lo << 28);
  }
  uint32_t c = 1;  // + 1 ((p - 1) / 2 + 1)
  for (int i = 0; i < 9 && c; i++) {
    const uint32_t t = r.v[i] + c;
    r.v[i] = i < 8 ? (t & M29) : t;
    c = i < 8 ? (t >> 29) : 0;
  }
  return r;
}

struct SrsK {
  static constexpr L9 P = F29P<FqP>::P;
  static constexpr L9 TO_DOMAIN = l9_pow2_mod(P, 522);  // mul29(x, .) = x 2^261
  static constexpr L9 B3 = l9_reduce_small(l9_mul_small(F29P<FqP>::ONE, 3), P);  // 3 in the domain
  static constexpr L9 HALF = l9_half_up(P);  // y is the larger root <=> y >= (p + 1) / 2
  // (p + 1) / 4: 252 bits, 109 set -> 251 squarings + 108 multiplications
  static constexpr uint32_t SQRT_E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                                         0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
  static constexpr int SQRT_TOP_BIT = 27;  // highest set bit of SQRT_E[7]
};
static_assert(SrsK::HALF.v[0] == 0x0c3e7ea4u && SrsK::HALF.v[8] == 0x183227u, "(p + 1) / 2");
static_assert((SrsK::SQRT_E[7] >> SrsK::SQRT_TOP_BIT) == 1u, "top bit of (p + 1) / 4");

// ---- device checks (shared by the decode and by qg_srs_validate) -----------
// canonical little-endian words >= p ?
QG_DEV bool words_geq_p(const Fq& w) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)subb32(w.v[i], FqP::P[i], br, &br);
  return br == 0;
}

// normalized limbs (each < 2^29) >= k ?
QG_DEV bool limbs_geq(const Q29& a, const L9& k) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) br = (a.l[i] - k.v[i] - br) >> 31;
  return br == 0;
}

// x^3 + 3 in the R = 2^261 domain, normalized < 2p (x normalized < 2p)
QG_DEV Q29 curve_rhs29(const Q29& x) {
  return red2p29(add29(mul29(sqr29(x), x), Q29::from_l9(SrsK::B3)));
}

// a == b mod p (both normalized < 2p)
QG_DEV bool eq_mod29(const Q29& a, const Q29& b) {
  return is_zero_mod29(normfull29(sub29(a, b)));  // a + 4p - b < 6p
}

// y^2 == x^3 + 3 (x, y in the R = 2^261 domain, normalized < 2p)
QG_DEV bool on_curve29(const Q29& x, const Q29& y) { return eq_mod29(sqr29(y), curve_rhs29(x)); }

// a^((p+1)/4): the exponent is a compile-time constant, so the loop is the
// same instruction stream for every lane (no divergence); the words are
// unrolled and the bits of a word are a rolled loop over a scalar, so no
// register array is indexed dynamically (see for_each_digit in msm.hip).
QG_DEV Q29 sqrt_candidate29(const Q29& a) {
  Q29 r = a;  // the top set bit
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t e = SrsK::SQRT_E[w];
#pragma unroll 1
    for (int bit = (w == 7 ? SrsK::SQRT_TOP_BIT - 1 : 31); bit >= 0; bit--) {
      r = sqr29(r);
      if ((e >> bit) & 1u) r = mul29(r, a);
    }
  }
  return r;
}

QG_DEV void srs_report_bad(unsigned long long* bad, size_t i, uint32_t reason) {
  atomicMin(bad, ((unsigned long long)i << SRS_REASON_BITS) | (unsigned long long)reason);
}

// One thread per point: 32 / 64 bytes -> a G1Affine (Montgomery words, (0,0) =
// infinity) in the buffer srs_build_tables consumes.  A bad point is written
// as infinity and reported through *bad (lowest index wins).
template <bool COMPRESSED>
__global__ void __launch_bounds__(256)
k_g1_decode(const uint4* __restrict__ in, size_t n, G1Affine* __restrict__ out,
            unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NV = COMPRESSED ? 2 : 4;
  uint4 v[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) v[k] = in[(size_t)NV * i + k];
  Fq xw, yw = Fq::zero();
  xw.v[0] = v[0].x; xw.v[1] = v[0].y; xw.v[2] = v[0].z; xw.v[3] = v[0].w;
  xw.v[4] = v[1].x; xw.v[5] = v[1].y; xw.v[6] = v[1].z; xw.v[7] = v[1].w;
  if (!COMPRESSED) {
    yw.v[0] = v[NV - 2].x; yw.v[1] = v[NV - 2].y; yw.v[2] = v[NV - 2].z; yw.v[3] = v[NV - 2].w;
    yw.v[4] = v[NV - 1].x; yw.v[5] = v[NV - 1].y; yw.v[6] = v[NV - 1].z; yw.v[7] = v[NV - 1].w;
  }
  // the flags: top two bits of the point's last byte
  uint32_t& top = COMPRESSED ? xw.v[7] : yw.v[7];
  const bool f_neg = (top >> 31) != 0u, f_inf = ((top >> 30) & 1u) != 0u;
  top &= 0x3fffffffu;

  uint32_t reason = 0;
  if (f_inf) {
    if (!xw.is_zero() || !yw.is_zero() || f_neg) reason = QG_SRS_BAD_INFINITY;
  } else if (words_geq_p(xw) || (!COMPRESSED && words_geq_p(yw))) {
    reason = QG_SRS_BAD_NONCANONICAL;
  }
  // the arithmetic runs for every lane (a refused or infinite point computes
  // on its masked words, < 2^254 < 8p, and the result is dropped)
  const Q29 to_dom = Q29::from_l9(SrsK::TO_DOMAIN);
  const Q29 x = mul29(to29(xw), to_dom);
  const Q29 rhs = curve_rhs29(x);
  Fq ym;  // y, Montgomery words (R = 2^256)
  if (COMPRESSED) {
    const Q29 y = sqrt_candidate29(rhs);
    if (!reason && !f_inf && !eq_mod29(sqr29(y), rhs)) reason = QG_SRS_BAD_NOT_SQUARE;
    Q29 unit = Q29::zero();
    unit.l[0] = 1;
    const Q29 yc = canon29(mul29(y, unit));  // the canonical integer
    ym = q29_export(y);
    // BN254 G1 has no point with y = 0 (-3 is not a cube), so p - y is canonical
    if (limbs_geq(yc, SrsK::HALF) != f_neg) ym = fneg(ym);
  } else {
    const Q29 yc = to29(yw);
    const Q29 y = mul29(yc, to_dom);
    if (!reason && !f_inf) {
      if (!eq_mod29(sqr29(y), rhs))
        reason = QG_SRS_BAD_NOT_ON_CURVE;
      else if (limbs_geq(yc, SrsK::HALF) != f_neg)
        reason = QG_SRS_BAD_SIGN_FLAG;
    }
    ym = q29_export(y);
  }
  if (reason) srs_report_bad(bad, i, reason);
  out[i] = (reason || f_inf) ? G1Affine::infinity() : G1Affine{q29_export(x), ym};
}

// The same checks over table rows (canonical 29-bit limbs, R = 2^261).
__global__ void __launch_bounds__(256)
k_srs_validate(const MsmPt* __restrict__ rows, size_t n, unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MsmPt row = rows[i];
  Q29 x, y;
  const bool inf = msm_pt_unpack(row, x, y);
  uint32_t hi = 0;  // a limb of 2^29 or more
#pragma unroll
  for (int k = 0; k < 9; k++) hi |= (x.l[k] | y.l[k]) >> 29;
  uint32_t reason = 0;
  if (inf) {
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 27; k++) any |= row.w[k];
    if (any) reason = QG_SRS_BAD_INFINITY;
  } else if (hi || limbs_geq(x, SrsK::P) || limbs_geq(y, SrsK::P)) {
    reason = QG_SRS_BAD_NONCANONICAL;
  } else if (!on_curve29(x, y)) {
    reason = QG_SRS_BAD_NOT_ON_CURVE;
  }
  if (reason) srs_report_bad(bad, i, reason);
}

// affine points (Montgomery words) -> canonical bytes plus flags
template <bool COMPRESSED>
__global__ void __launch_bounds__(256)
k_g1_encode(const G1Affine* __restrict__ pts, size_t n, uint4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Affine a = pts[i];
  Fq x = Fq::zero(), y = Fq::zero();
  uint32_t flags = 0x40000000u;  // infinity
  if (!a.is_inf()) {
    x = from_mont(a.x);
    y = from_mont(a.y);
    // y > p - y  <=>  2y > p: y - (p - y) without a borrow and not zero
    Fq ny;
    uint32_t br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) ny.v[k] = subb32(FqP::P[k], y.v[k], br, &br);
    br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) (void)subb32(ny.v[k], y.v[k], br, &br);
    flags = br ? 0x80000000u : 0u;  // p - y < y
  }
  constexpr int NV = COMPRESSED ? 2 : 4;
  uint4* o = out + (size_t)NV * i;
  if (COMPRESSED) {
    o[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    o[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7] | flags);
  } else {
    o[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    o[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    o[NV - 2] = make_uint4(y.v[0], y.v[1], y.v[2], y.v[3]);
    o[NV - 1] = make_uint4(y.v[4], y.v[5], y.v[6], y.v[7] | flags);
  }
}

// rho_g = low 128 bits (LE) of BLAKE3(seed || u64_le(g)), g the GLOBAL index
QG_DEV Fr srs_rho(const uint32_t (&seed)[8], uint64_t g) {
  struct Src {
    const uint32_t* s;
    uint64_t g;
    QG_DEV uint32_t operator()(uint32_t i) const {
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) w = i == (uint32_t)k ? s[k] : w;
      w = i == 8 ? (uint32_t)g : w;
      w = i == 9 ? (uint32_t)(g >> 32) : w;
      return w;
    }
  } src{seed, g};
  uint32_t o[4];
  b3_chunk_words(src, 40, o, 4);
  Fr r = Fr::zero();
#pragma unroll
  for (int k = 0; k < 4; k++) r.v[k] = o[k];
  return to_mont(r);  // < 2^128 < r
}

struct SrsSeed {
  uint32_t w[8];
};

// The two scalar vectors of the powers check over this rank's global range
// [goff, goff + n) of N points: a[i] = rho_g for g < N - 1 (else 0), b[i] =
// rho_{g-1} for g >= 1 (else 0).  One compression per index (thread 0 adds
// the one before its range).
__global__ void __launch_bounds__(256)
k_srs_rho(SrsSeed seed, uint64_t goff, size_t n, uint64_t N, Fr* __restrict__ a,
          Fr* __restrict__ b) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = goff + i;
  const Fr r = srs_rho(seed.w, g);
  a[i] = g + 1 < N ? r : Fr::zero();
  if (i + 1 < n) b[i + 1] = r;
  if (i == 0) b[0] = g ? srs_rho(seed.w, g - 1) : Fr::zero();
}

// ---- host -------------------------------------------------------------------
static unsigned long long* bad_word_reset(qg_ctx* ctx) {
  unsigned long long* d = ctx->scratch_as<unsigned long long>("srs_bad_word", 1);
  QG_HIP(hipMemsetAsync(d, 0xff, sizeof(unsigned long long), ctx->stream));  // SRS_BAD_NONE
  return d;
}

// after the work queued behind bad_word_reset: synchronizes, and throws
// QG_ERR_INVALID naming the lowest bad point
static void bad_word_check(qg_ctx* ctx, const unsigned long long* d, const char* what,
                           uint64_t* bad_index, uint32_t* bad_reason) {
  uint64_t* h = static_cast<uint64_t*>(ctx->pinned_get("srs_bad_word", sizeof(uint64_t)));
  QG_HIP(hipMemcpyAsync(h, d, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  uint64_t idx = 0;
  uint32_t reason = 0;
  if (!srs_bad_unpack(*h, &idx, &reason)) return;
  if (bad_index) *bad_index = idx;
  if (bad_reason) *bad_reason = reason;
  throw Error(QG_ERR_INVALID, srs_bad_message(what, idx, reason));
}

}  // namespace qg

extern "C" {

int qg_srs_import(qg_ctx* ctx, const uint8_t* bytes, size_t n, int format, uint32_t flags,
                  qg_srs** out, uint64_t* bad_index, uint32_t* bad_reason) {
  if (!ctx || !out || (!bytes && n)) return QG_ERR_INVALID;
  *out = nullptr;
  if (bad_index) *bad_index = 0;
  if (bad_reason) *bad_reason = 0;
  qg_srs* srs = nullptr;
  int rc = qg_guard(ctx, [&] {
    QG_CHECK((flags & ~QG_SRS_ONESHOT) == 0, QG_ERR_INVALID, "unknown SRS import flags");
    const size_t nbytes = srs_bytes_checked(n, format);
    QG_HIP(hipSetDevice(ctx->device));
    srs = srs_alloc(ctx, n, (flags & QG_SRS_ONESHOT) != 0);
    uint4* d_in = ctx->scratch_as<uint4>("srs_io_bytes", nbytes / sizeof(uint4));
    QG_HIP(hipMemcpyAsync(d_in, bytes, nbytes, hipMemcpyHostToDevice, ctx->stream));
    unsigned long long* d_bad = bad_word_reset(ctx);
    G1Affine* d_base = ctx->scratch_as<G1Affine>("srs_base", n);
    {
      QgTimed tm(ctx, "g1_decode");
      if (format == QG_G1_COMPRESSED)
        hipLaunchKernelGGL(k_g1_decode<true>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                           d_in, n, d_base, d_bad);
      else
        hipLaunchKernelGGL(k_g1_decode<false>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                           d_in, n, d_base, d_bad);
      QG_LAUNCH_CHECK();
    }
    // a refused point is infinity in d_base: the build is harmless either way
    srs_build_tables(ctx, srs, d_base);
    bad_word_check(ctx, d_bad, "SRS import", bad_index, bad_reason);
  });
  if (rc != QG_OK) {
    if (srs) {
      (void)hipFree(srs->d_table);
      delete srs;
    }
    return rc;
  }
  *out = srs;
  return QG_OK;
}

int qg_srs_export(const qg_srs* srs, size_t offset, size_t n, int format, uint8_t* out) {
  if (!srs || (!out && n) || !srs_range_ok(offset, n, srs->n)) return QG_ERR_INVALID;
  qg_ctx* ctx = srs->ctx;
  return qg_guard(ctx, [&] {
    QG_CHECK(srs_point_bytes(format) != 0, QG_ERR_INVALID, "unknown G1 point format");
    if (n == 0) return;
    const size_t nbytes = srs_bytes_checked(n, format);
    QG_HIP(hipSetDevice(ctx->device));
    G1Affine* d_pts = ctx->scratch_as<G1Affine>("srs_download", n);
    uint4* d_out = ctx->scratch_as<uint4>("srs_io_bytes", nbytes / sizeof(uint4));
    srs_unpack_rows(ctx, srs, offset, n, d_pts);
    if (format == QG_G1_COMPRESSED)
      hipLaunchKernelGGL(k_g1_encode<true>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                         d_pts, n, d_out);
    else
      hipLaunchKernelGGL(k_g1_encode<false>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                         d_pts, n, d_out);
    QG_LAUNCH_CHECK();
    QG_HIP(hipMemcpyAsync(out, d_out, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}

int qg_srs_validate(qg_ctx* ctx, const qg_srs* srs, uint64_t* bad_index, uint32_t* bad_reason) {
  if (!ctx || !srs || srs->ctx != ctx) return QG_ERR_INVALID;
  if (bad_index) *bad_index = 0;
  if (bad_reason) *bad_reason = 0;
  return qg_guard(ctx, [&] {
    QG_HIP(hipSetDevice(ctx->device));
    unsigned long long* d_bad = bad_word_reset(ctx);
    {
      QgTimed tm(ctx, "srs_validate");
      hipLaunchKernelGGL(k_srs_validate, dim3(div_up(srs->n, 256)), dim3(256), 0, ctx->stream,
                         srs->d_table, srs->n, d_bad);
      QG_LAUNCH_CHECK();
    }
    bad_word_check(ctx, d_bad, "SRS validation", bad_index, bad_reason);
  });
}

int qg_srs_check_powers(qg_ctx* ctx, const qg_srs* srs, const qg_kzg_vk* vk,
                        const uint8_t seed[32], int* ok) {
  if (!ctx || !srs || !vk || !ok || srs->ctx != ctx) return QG_ERR_INVALID;
  *ok = 0;
  return qg_guard(ctx, [&] {
    // the key first: a malformed one fails on every rank before any collective
    const G1Affine g1 = kzg_vk_g1(vk);
    QG_HIP(hipSetDevice(ctx->device));
    const size_t n = srs->n;
    const uint64_t world = ctx->sharded ? (uint64_t)ctx->world : 1;
    const uint64_t rank = ctx->sharded ? (uint64_t)ctx->rank : 0;
    QG_CHECK((uint64_t)n < SRS_MAX_POINTS / world, QG_ERR_INVALID, "SRS point count out of range");
    const uint64_t N = world * n, goff = rank * n;

    // rank 0's seed and its verdict on P_0, shared once
    struct {
      uint8_t seed[32];
      uint8_t p0_ok;
    } mine{}, first{};
    if (seed) {
      memcpy(mine.seed, seed, 32);
    } else if (rank == 0) {
      std::random_device rd;
      for (int k = 0; k < 8; k++) {
        const uint32_t w = rd();
        memcpy(mine.seed + 4 * k, &w, 4);
      }
    }
    if (rank == 0) {
      G1Affine* d_p0 = ctx->scratch_as<G1Affine>("srs_download", 1);
      G1Affine p0;
      srs_unpack_rows(ctx, srs, 0, 1, d_p0);
      QG_HIP(hipMemcpyAsync(&p0, d_p0, sizeof p0, hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      mine.p0_ok = (!p0.is_inf() && p0.x == g1.x && p0.y == g1.y) ? 1 : 0;
    }
    first = mine;
    if (ctx->sharded) {
      std::vector<uint8_t> all(sizeof mine * (size_t)ctx->world);
      const int rc = qg_comm_allgather_host(ctx, &mine, sizeof mine, all.data());
      if (rc != QG_OK) throw Error(rc, ctx->last_error);
      memcpy(&first, all.data(), sizeof first);
    }
    if (N == 1) {
      *ok = first.p0_ok;
      return;
    }
    SrsSeed sw;
    memcpy(sw.w, first.seed, 32);
    Fr* d_a = ctx->scratch_as<Fr>("srs_rho_a", n);
    Fr* d_b = ctx->scratch_as<Fr>("srs_rho_b", n);
    {
      QgTimed tm(ctx, "srs_rho");
      hipLaunchKernelGGL(k_srs_rho, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, sw, goff, n, N,
                         d_a, d_b);
      QG_LAUNCH_CHECK();
    }
    // two MSMs over the same bases; a sharded context sums the ranks' partials,
    // so every rank evaluates the same equation
    const std::vector<G1Affine> ab = msm_device_batch(ctx, srs, {d_a, d_b}, {n, n});
    const bool rel = kzg_tau_relation(vk, ab[0], ab[1]);
    *ok = (first.p0_ok && rel) ? 1 : 0;
  });
}

}  // extern "C"
