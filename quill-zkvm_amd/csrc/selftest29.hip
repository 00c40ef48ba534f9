// qg_selftest_field29: the 29-bit-limb field layer (field29.h) one primitive
// at a time, raw limbs in and out, so a test can hand a primitive operands at
// the bounds its contract documents (non-canonical representatives,
// almost-normalized and lazy limbs) and read back the representation, not
// only the residue.  on_device = 0 runs the QG_HD functions as compiled for
// the host; on_device = 1 runs them as compiled for gfx950, plus the
// device-only throughput forms (mul29t ...).  One thread per case, no
// data-dependent addressing.
#include "common.h"
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

}  // extern "C"
