// qg_selftest_field29: the 29-bit-limb field layer (field29.h) one primitive
// at a time, raw limbs in and out, so a test can hand a primitive operands at
// the bounds its contract documents (non-canonical representatives,
// almost-normalized and lazy limbs) and read back the representation, not
// only the residue.  on_device = 0 runs the QG_HD functions as compiled for
// the host; on_device = 1 runs them as compiled for gfx950, plus the
// device-only throughput forms (mul29t ...).  One thread per case, no
// data-dependent addressing.  qg_selftest_curve29 (below) does the same for
// the XYZZ primitives of curve29.h, qg_selftest_inverse for the binary-GCD
// inversion of bingcd.h.
#include <vector>

#include "bingcd.h"
#include "common.h"
#include "curve29.h"
#include "field29.h"

using namespace qg;

namespace qg {

// field elements per case: operands a[0..7], results r[0..3] (unused: zero)
static constexpr int F29_IN = QG_SELFTEST_F29_IN / 9;
static constexpr int F29_OUT = QG_SELFTEST_F29_OUT / 9;
static constexpr size_t F29_MAX_CASES = 65536;

// the host-callable primitives; false: not one of them
template <class C>
QG_HD bool f29_op_hd(int op, const F29<C>* a, F29<C>* r) {
  switch (op) {
    case QG_F29_MUL: r[0] = mul29(a[0], a[1]); return true;
    case QG_F29_SQR: r[0] = sqr29(a[0]); return true;
    case QG_F29_MULSUB: r[0] = mulsub29(a[0], a[1], a[2], a[3]); return true;
    case QG_F29_NORM: r[0] = norm29(a[0]); return true;
    case QG_F29_NORMFULL: r[0] = normfull29(a[0]); return true;
    case QG_F29_RED2P: r[0] = red2p29(a[0]); return true;
    case QG_F29_RED6P: r[0] = red6p29(a[0]); return true;
    case QG_F29_RED16P: r[0] = red16p29(a[0]); return true;
    case QG_F29_CANON: r[0] = canon29(a[0]); return true;
    case QG_F29_ISZERO8: r[0].l[0] = is_zero_mod29_fast<C, 8>(a[0]) ? 1u : 0u; return true;
    case QG_F29_ISZERO20: r[0].l[0] = is_zero_mod29_fast<C, 20>(a[0]) ? 1u : 0u; return true;
    case QG_F29_RELIMB: r[0] = to29(from29(a[0])); return true;
    default: return false;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
template <class C, int N>
__device__ __forceinline__ void f29_tn(const F29<C>* a, F29<C>* r, bool alias) {
  F29<C> x[N], y[N], z[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    x[i] = a[i];
    y[i] = a[4 + i];
  }
  if (alias) {
    mul29tn<C, N>(x, y, x);
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = x[i];
  } else {
    mul29tn<C, N>(x, y, z);
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = z[i];
  }
}

// the device-only throughput forms
template <class C>
__device__ __forceinline__ void f29_op_dev(int op, const F29<C>* a, F29<C>* r) {
  switch (op) {
    case QG_F29_MULT: r[0] = mul29t(a[0], a[1]); break;
    case QG_F29_SQRT: r[0] = sqr29t(a[0]); break;
    case QG_F29_MULSUBT: r[0] = mulsub29t(a[0], a[1], a[2], a[3]); break;
    case QG_F29_MULT2: mul29t2(a[0], a[1], a[2], a[3], r[0], r[1]); break;
    case QG_F29_SQRT2: sqr29t2(a[0], a[1], r[0], r[1]); break;
    case QG_F29_MULTN3: f29_tn<C, 3>(a, r, false); break;
    case QG_F29_MULTN4: f29_tn<C, 4>(a, r, false); break;
    case QG_F29_MULTN3_ALIAS: f29_tn<C, 3>(a, r, true); break;
    case QG_F29_MULTN4_ALIAS: f29_tn<C, 4>(a, r, true); break;
    default: break;
  }
}
#endif

template <class C>
__global__ void __launch_bounds__(64)
    k_f29_selftest(int op, const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F29<C> a[F29_IN], r[F29_OUT];
#pragma unroll
  for (int e = 0; e < F29_IN; e++)
#pragma unroll
    for (int l = 0; l < 9; l++) a[e].l[l] = in[(i * F29_IN + e) * 9 + l];
#pragma unroll
  for (int e = 0; e < F29_OUT; e++) r[e] = F29<C>::zero();
  if (!f29_op_hd<C>(op, a, r)) f29_op_dev<C>(op, a, r);
#pragma unroll
  for (int e = 0; e < F29_OUT; e++)
#pragma unroll
    for (int l = 0; l < 9; l++) out[(i * F29_OUT + e) * 9 + l] = r[e].l[l];
#endif
}

template <class C>
static void f29_selftest(qg_ctx* ctx, int op, bool dev, const uint32_t* in, size_t n, uint32_t* out) {
  if (n == 0) return;
  if (dev) {
    QG_CHECK(ctx, QG_ERR_INVALID, "device self-test needs a context");
    QG_HIP(hipSetDevice(ctx->device));
    const size_t ni = n * QG_SELFTEST_F29_IN, no = n * QG_SELFTEST_F29_OUT;
    uint32_t* d = ctx->scratch_as<uint32_t>("f29_selftest", ni + no);
    QG_HIP(hipMemcpyAsync(d, in, ni * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_f29_selftest<C>, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, op, d, n,
                       d + ni);
    QG_LAUNCH_CHECK();
    QG_HIP(hipMemcpyAsync(out, d + ni, no * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return;
  }
  for (size_t i = 0; i < n; i++) {
    F29<C> a[F29_IN], r[F29_OUT];
    for (int e = 0; e < F29_IN; e++)
      for (int l = 0; l < 9; l++) a[e].l[l] = in[(i * F29_IN + e) * 9 + l];
    for (int e = 0; e < F29_OUT; e++) r[e] = F29<C>::zero();
    QG_CHECK(f29_op_hd<C>(op, a, r), QG_ERR_UNSUPPORTED, "device-only form: no host path");
    for (int e = 0; e < F29_OUT; e++)
      for (int l = 0; l < 9; l++) out[(i * F29_OUT + e) * 9 + l] = r[e].l[l];
  }
}

// ---- qg_selftest_curve29 ----------------------------------------------------
// The XYZZ primitives one call at a time on raw limbs (quill_gpu.h).  Values
// are computed and stored by thread index only.
static constexpr size_t X29_MAX_CASES = 65536;

QG_HD X29 x29_from_limbs(const uint32_t* w) {
  X29 p;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    p.X.l[i] = w[i];
    p.Y.l[i] = w[9 + i];
    p.ZZ.l[i] = w[18 + i];
    p.ZZZ.l[i] = w[27 + i];
  }
  return p;
}

QG_HD void x29_to_limbs(const X29& p, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w[i] = p.X.l[i];
    w[9 + i] = p.Y.l[i];
    w[18 + i] = p.ZZ.l[i];
    w[27 + i] = p.ZZZ.l[i];
  }
}

// the host-callable ops; false: not one of them
QG_HD bool x29_op_hd(int op, const X29& p, const X29& q, X29& r) {
  switch (op) {
    case QG_X29_ADD: r = x29_add(p, q); return true;
    case QG_X29_DBL: r = x29_dbl(p); return true;
    case QG_X29_ADD_AFFINE: {
      A29 a;
      a.x = q.X;
      a.y = q.Y;
      r = x29_add_affine(p, a);
      return true;
    }
    case QG_X29_ACC_FINISH: r = x29_acc_finish(p); return true;
    case QG_X29_RAW: r = x29_unraw(x29_raw(p)); return true;
    default: return false;
  }
}

// OP < QG_X29_ADD_Q4: thread i runs case i; the quad ops: lanes 4 i .. 4 i + 3
// run case i and every lane stores what it returned
template <int OP>
__global__ void __launch_bounds__(64)
    k_x29_selftest(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out,
                   uint32_t* __restrict__ flags) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr bool QUAD = OP == QG_X29_ADD_Q4 || OP == QG_X29_DBL_Q4;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = QUAD ? t >> 2 : t;
  if (i >= n) return;  // whole quads leave together
  const X29 p = x29_from_limbs(in + i * QG_SELFTEST_X29_IN);
  const X29 q = x29_from_limbs(in + i * QG_SELFTEST_X29_IN + 36);
  X29 r = p;
  uint32_t fl = 0;
  if constexpr (OP == QG_X29_ACC_MADD) {
    bool inf = false;
    if (x29_acc_madd_tp(r, q.X, q.Y)) {
      fl = QG_X29_FLAG_MAIN;
    } else {
      x29_acc_madd_exc(r, q.X, q.Y, &inf);
      fl = QG_X29_FLAG_EXC | (inf ? QG_X29_FLAG_INF : 0u);
    }
  } else if constexpr (OP == QG_X29_ADD_Q4) {
    r = x29_add_q4(p, q);
  } else if constexpr (OP == QG_X29_DBL_Q4) {
    r = x29_dbl_q4(p);
  } else {
    x29_op_hd(OP, p, q, r);
  }
  x29_to_limbs(r, out + t * QG_SELFTEST_X29_OUT);
  if (!QUAD || (t & 3u) == 0) flags[i] = fl;
#endif
}

template <int OP>
static void x29_selftest_launch(qg_ctx* ctx, const uint32_t* d_in, size_t n, uint32_t* d_out,
                                uint32_t* d_flags) {
  const size_t threads = (OP == QG_X29_ADD_Q4 || OP == QG_X29_DBL_Q4) ? 4 * n : n;
  hipLaunchKernelGGL(k_x29_selftest<OP>, dim3(div_up(threads, 64)), dim3(64), 0, ctx->stream, d_in, n,
                     d_out, d_flags);
  QG_LAUNCH_CHECK();
}

static void x29_selftest(qg_ctx* ctx, int op, bool dev, const uint32_t* in, size_t n, uint32_t* out,
                         uint32_t* flags) {
  if (n == 0) return;
  if (!dev) {
    for (size_t i = 0; i < n; i++) {
      const X29 p = x29_from_limbs(in + i * QG_SELFTEST_X29_IN);
      const X29 q = x29_from_limbs(in + i * QG_SELFTEST_X29_IN + 36);
      X29 r = p;
      QG_CHECK(x29_op_hd(op, p, q, r), QG_ERR_UNSUPPORTED, "device-only form: no host path");
      x29_to_limbs(r, out + i * QG_SELFTEST_X29_OUT);
      flags[i] = 0;
    }
    return;
  }
  QG_CHECK(ctx, QG_ERR_INVALID, "device self-test needs a context");
  QG_HIP(hipSetDevice(ctx->device));
  const bool quad = op == QG_X29_ADD_Q4 || op == QG_X29_DBL_Q4;
  const size_t ni = n * QG_SELFTEST_X29_IN;
  const size_t no = n * (quad ? QG_SELFTEST_X29_OUT_Q4 : QG_SELFTEST_X29_OUT);
  uint32_t* d = ctx->scratch_as<uint32_t>("x29_selftest", ni + no + n);
  uint32_t *d_out = d + ni, *d_flags = d_out + no;
  QG_HIP(hipMemcpyAsync(d, in, ni * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  switch (op) {
    case QG_X29_ADD: x29_selftest_launch<QG_X29_ADD>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_DBL: x29_selftest_launch<QG_X29_DBL>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_ADD_AFFINE: x29_selftest_launch<QG_X29_ADD_AFFINE>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_ACC_FINISH: x29_selftest_launch<QG_X29_ACC_FINISH>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_RAW: x29_selftest_launch<QG_X29_RAW>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_ACC_MADD: x29_selftest_launch<QG_X29_ACC_MADD>(ctx, d, n, d_out, d_flags); break;
    case QG_X29_ADD_Q4: x29_selftest_launch<QG_X29_ADD_Q4>(ctx, d, n, d_out, d_flags); break;
    default: x29_selftest_launch<QG_X29_DBL_Q4>(ctx, d, n, d_out, d_flags); break;
  }
  QG_HIP(hipMemcpyAsync(out, d_out, no * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  QG_HIP(hipMemcpyAsync(flags, d_flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
}

// ---- qg_selftest_inverse ----------------------------------------------------
// The binary-GCD inversion of bingcd.h (the Logup column's single inversion runs
// it on the host).
// qg_selftest_inverse's device path: one inversion per thread
template <class C>
__global__ void k_inv_selftest(const Fp<C>* __restrict__ in, Fp<C>* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = inv_bingcd<C>(in[i]);
}

template <class C>
static void inv_selftest(qg_ctx* ctx, bool dev, const uint64_t* in, uint64_t* out, size_t n) {
  std::vector<Fp<C>> h(n);
  for (size_t i = 0; i < n; i++)
    for (int l = 0; l < 4; l++) {
      h[i].v[2 * l] = (uint32_t)in[4 * i + l];
      h[i].v[2 * l + 1] = (uint32_t)(in[4 * i + l] >> 32);
    }
  for (size_t i = 0; i < n; i++) {
    Fp<C> t = h[i];
    reduce_full<C>(t.v);
    QG_CHECK(t == h[i], QG_ERR_INVALID, "inverse self-test input not canonical");
  }
  if (dev) {
    QG_CHECK(ctx, QG_ERR_INVALID, "device self-test needs a context");
    QG_HIP(hipSetDevice(ctx->device));
    Fp<C>* d = ctx->scratch_as<Fp<C>>("inv_selftest", 2 * n + 2);
    QG_HIP(hipMemcpyAsync(d, h.data(), n * sizeof(Fp<C>), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_inv_selftest<C>, dim3(div_up(n ? n : 1, 64)), dim3(64), 0, ctx->stream, d, d + n,
                       n);
    QG_LAUNCH_CHECK();
    QG_HIP(hipMemcpyAsync(h.data(), d + n, n * sizeof(Fp<C>), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  } else {
    for (size_t i = 0; i < n; i++) h[i] = inv_bingcd<C>(h[i]);
  }
  for (size_t i = 0; i < n; i++)
    for (int l = 0; l < 4; l++)
      out[4 * i + l] = (uint64_t)h[i].v[2 * l] | ((uint64_t)h[i].v[2 * l + 1] << 32);
}

}  // namespace qg

extern "C" {

int qg_selftest_field29(qg_ctx* ctx, int field, int op, int on_device, const uint32_t* in, size_t n,
                        uint32_t* out) {
  if (!in || !out) return QG_ERR_INVALID;
  if (field != 0 && field != 1) return QG_ERR_INVALID;
  if (op < 0 || op >= QG_F29_OP_COUNT) return QG_ERR_INVALID;
  if (n > F29_MAX_CASES) return QG_ERR_INVALID;
  if (on_device && !ctx) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    if (field == 0) f29_selftest<FrP>(ctx, op, on_device != 0, in, n, out);
    else f29_selftest<FqP>(ctx, op, on_device != 0, in, n, out);
  });
}

int qg_selftest_curve29(qg_ctx* ctx, int op, int on_device, const uint32_t* in, size_t n,
                        uint32_t* out, uint32_t* flags) {
  if (!in || !out || !flags) return QG_ERR_INVALID;
  if (op < 0 || op >= QG_X29_OP_COUNT) return QG_ERR_INVALID;
  if (n > X29_MAX_CASES) return QG_ERR_INVALID;
  if (on_device && !ctx) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] { x29_selftest(ctx, op, on_device != 0, in, n, out, flags); });
}

int qg_selftest_inverse(qg_ctx* ctx, int field, int on_device, const uint64_t* in, uint64_t* out,
                        size_t n) {
  if ((!in || !out) && n) return QG_ERR_INVALID;
  if (field != 0 && field != 1) return QG_ERR_INVALID;
  return qg_guard(ctx, [&] {
    if (field == 0) inv_selftest<FrP>(ctx, on_device != 0, in, out, n);
    else inv_selftest<FqP>(ctx, on_device != 0, in, out, n);
  });
}

}  // extern "C"
