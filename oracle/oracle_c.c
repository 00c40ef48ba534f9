/*
 * oracle_c.c — C restatement of the reference's CPU algorithms.
 * TEST INFRASTRUCTURE ONLY: used by tests/ (checked against the Python oracle)
 * and by bench.py's cpu_baseline leg.  Never linked into the product.
 *
 * Restates (third-party code the reference calls; not vendored in /root/reference):
 *  - ark-ff 0.5.0 Fp256 Montgomery arithmetic (4 x u64, CIOS), Cargo.lock:56-57
 *  - ark-ec 0.5.0 short-Weierstrass Jacobian group law (dbl-2009-l,
 *    add-2007-bl, madd-2007-bl) and VariableBaseMSM::msm_bigint_wnaf:
 *    c = 3 if n < 32 else ln_without_floats(n) + 2 (log2(n)*69/100),
 *    signed digits (make_digits, last digit absorbs the carry),
 *    2^c Jacobian buckets per window, running-sum reduction, window
 *    doubling — single-threaded exactly like the reference (no rayon in
 *    Cargo.lock, so cfg_into_iter! is sequential).  Call site pcs/src/kzg.rs:72.
 *  - KZG::commit as written (pcs/src/kzg.rs:61-73): into_affine of every SRS
 *    point on every call, then the MSM.
 *  - sumcheck prover round loop (hyperplonk/src/piops/sumcheck.rs:28-114) in
 *    evaluation form for h = prod of k tables, with the BLAKE3 transcript
 *    (transcript/src/transcript.rs) — a lower bound on the reference's
 *    per-pair DensePolynomial-allocating structure.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef unsigned __int128 u128;
typedef struct { uint64_t v[4]; } fp;

typedef struct {
  uint64_t p[4];
  uint64_t inv; /* -p^{-1} mod 2^64 */
  uint64_t r2[4];
  uint64_t one[4];
} modulus;

static const modulus FR = {
    {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    0xc2e1f593efffffffull,
    {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull},
    {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full}};
static const modulus FQ = {
    {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    0x87d20782e4866389ull,
    {0xf32cfc5b538afa89ull, 0xb5e71911d44501fbull, 0x47ab1eff0a417ff6ull, 0x06d89f71cab8351full},
    {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full}};

static inline int geq(const uint64_t a[4], const uint64_t b[4]) {
  for (int i = 3; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] > b[i];
  }
  return 1;
}
static inline void sub4(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    u128 d = (u128)a[i] - b[i] - br;
    r[i] = (uint64_t)d;
    br = (uint64_t)(d >> 127);
  }
}
static inline fp f_add(const modulus* m, fp a, fp b) {
  fp r;
  uint64_t c = 0;
  for (int i = 0; i < 4; i++) {
    u128 s = (u128)a.v[i] + b.v[i] + c;
    r.v[i] = (uint64_t)s;
    c = (uint64_t)(s >> 64);
  }
  if (geq(r.v, m->p)) sub4(r.v, r.v, m->p);
  return r;
}
static inline fp f_sub(const modulus* m, fp a, fp b) {
  fp r;
  if (geq(a.v, b.v)) {
    sub4(r.v, a.v, b.v);
  } else {
    uint64_t t[4];
    sub4(t, m->p, b.v);
    uint64_t c = 0;
    for (int i = 0; i < 4; i++) {
      u128 s = (u128)a.v[i] + t[i] + c;
      r.v[i] = (uint64_t)s;
      c = (uint64_t)(s >> 64);
    }
  }
  return r;
}
/* CIOS Montgomery multiplication (ark-ff "no-carry" path applies: top limb < 2^63-1) */
static inline fp f_mul(const modulus* m, fp a, fp b) {
  uint64_t t[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 A = (u128)a.v[0] * b.v[i] + t[0];
    uint64_t t0 = (uint64_t)A;
    uint64_t k = t0 * m->inv;
    u128 C = (u128)k * m->p[0] + t0;
    for (int j = 1; j < 4; j++) {
      A = (u128)a.v[j] * b.v[i] + t[j] + (uint64_t)(A >> 64);
      C = (u128)k * m->p[j] + (uint64_t)A + (uint64_t)(C >> 64);
      t[j - 1] = (uint64_t)C;
    }
    t[3] = (uint64_t)(C >> 64) + (uint64_t)(A >> 64);
  }
  fp r = {{t[0], t[1], t[2], t[3]}};
  if (geq(r.v, m->p)) sub4(r.v, r.v, m->p);
  return r;
}
static inline int f_is_zero(fp a) { return !(a.v[0] | a.v[1] | a.v[2] | a.v[3]); }
static inline int f_eq(fp a, fp b) { return !memcmp(&a, &b, sizeof(fp)); }
static inline fp f_one(const modulus* m) {
  fp r;
  memcpy(r.v, m->one, 32);
  return r;
}
static fp f_inv(const modulus* m, fp a) {
  uint64_t e[4];
  memcpy(e, m->p, 32);
  e[0] -= 2;
  fp r = f_one(m);
  for (int i = 3; i >= 0; i--)
    for (int b = 63; b >= 0; b--) {
      r = f_mul(m, r, r);
      if ((e[i] >> b) & 1) r = f_mul(m, r, a);
    }
  return r;
}
static inline fp f_from_mont(const modulus* m, fp a) {
  fp one = {{1, 0, 0, 0}};
  return f_mul(m, a, one);
}
static inline fp f_to_mont(const modulus* m, fp a) {
  fp r2;
  memcpy(r2.v, m->r2, 32);
  return f_mul(m, a, r2);
}

/* ---------------------------------------------------------------- G1 */
typedef struct { fp x, y; int inf; } g1a;
typedef struct { fp x, y, z; } g1j; /* z = 0 -> infinity */

static inline int j_is_inf(const g1j* p) { return f_is_zero(p->z); }
static g1j j_zero(void) {
  g1j r;
  memset(&r, 0, sizeof r);
  r.y = f_one(&FQ);
  return r;
}
/* dbl-2009-l (a = 0) */
static void j_double(g1j* p) {
  if (j_is_inf(p)) return;
  const modulus* m = &FQ;
  fp A = f_mul(m, p->x, p->x), B = f_mul(m, p->y, p->y), C = f_mul(m, B, B);
  fp t = f_add(m, p->x, B);
  fp D = f_sub(m, f_sub(m, f_mul(m, t, t), A), C);
  D = f_add(m, D, D);
  fp E = f_add(m, f_add(m, A, A), A);
  fp F = f_mul(m, E, E);
  fp X3 = f_sub(m, F, f_add(m, D, D));
  fp C8 = f_add(m, C, C);
  C8 = f_add(m, C8, C8);
  C8 = f_add(m, C8, C8);
  fp Y3 = f_sub(m, f_mul(m, E, f_sub(m, D, X3)), C8);
  fp Z3 = f_mul(m, p->y, p->z);
  Z3 = f_add(m, Z3, Z3);
  p->x = X3;
  p->y = Y3;
  p->z = Z3;
}
/* madd-2007-bl: p += q (affine) */
static void j_add_affine(g1j* p, const g1a* q) {
  if (q->inf) return;
  const modulus* m = &FQ;
  if (j_is_inf(p)) {
    p->x = q->x;
    p->y = q->y;
    p->z = f_one(m);
    return;
  }
  fp Z1Z1 = f_mul(m, p->z, p->z);
  fp U2 = f_mul(m, q->x, Z1Z1);
  fp S2 = f_mul(m, f_mul(m, q->y, p->z), Z1Z1);
  if (f_eq(p->x, U2)) {
    if (f_eq(p->y, S2)) {
      j_double(p);
    } else {
      *p = j_zero();
    }
    return;
  }
  fp H = f_sub(m, U2, p->x);
  fp HH = f_mul(m, H, H);
  fp I = f_add(m, HH, HH);
  I = f_add(m, I, I);
  fp J = f_mul(m, H, I);
  fp r = f_sub(m, S2, p->y);
  r = f_add(m, r, r);
  fp V = f_mul(m, p->x, I);
  fp X3 = f_sub(m, f_sub(m, f_mul(m, r, r), J), f_add(m, V, V));
  fp Y1J = f_mul(m, p->y, J);
  fp Y3 = f_sub(m, f_mul(m, r, f_sub(m, V, X3)), f_add(m, Y1J, Y1J));
  fp t = f_add(m, p->z, H);
  fp Z3 = f_sub(m, f_sub(m, f_mul(m, t, t), Z1Z1), HH);
  p->x = X3;
  p->y = Y3;
  p->z = Z3;
}
/* add-2007-bl: p += q (Jacobian) */
static void j_add(g1j* p, const g1j* q) {
  if (j_is_inf(q)) return;
  if (j_is_inf(p)) {
    *p = *q;
    return;
  }
  const modulus* m = &FQ;
  fp Z1Z1 = f_mul(m, p->z, p->z), Z2Z2 = f_mul(m, q->z, q->z);
  fp U1 = f_mul(m, p->x, Z2Z2), U2 = f_mul(m, q->x, Z1Z1);
  fp S1 = f_mul(m, f_mul(m, p->y, q->z), Z2Z2);
  fp S2 = f_mul(m, f_mul(m, q->y, p->z), Z1Z1);
  if (f_eq(U1, U2)) {
    if (f_eq(S1, S2)) {
      j_double(p);
    } else {
      *p = j_zero();
    }
    return;
  }
  fp H = f_sub(m, U2, U1);
  fp I = f_add(m, H, H);
  I = f_mul(m, I, I);
  fp J = f_mul(m, H, I);
  fp r = f_sub(m, S2, S1);
  r = f_add(m, r, r);
  fp V = f_mul(m, U1, I);
  fp X3 = f_sub(m, f_sub(m, f_mul(m, r, r), J), f_add(m, V, V));
  fp S1J = f_mul(m, S1, J);
  fp Y3 = f_sub(m, f_mul(m, r, f_sub(m, V, X3)), f_add(m, S1J, S1J));
  fp t = f_add(m, p->z, q->z);
  fp Z3 = f_mul(m, f_sub(m, f_sub(m, f_mul(m, t, t), Z1Z1), Z2Z2), H);
  p->x = X3;
  p->y = Y3;
  p->z = Z3;
}
static g1a j_to_affine(const g1j* p) {
  g1a r;
  memset(&r, 0, sizeof r);
  if (j_is_inf(p)) {
    r.inf = 1;
    return r;
  }
  const modulus* m = &FQ;
  fp zi = f_inv(m, p->z), zi2 = f_mul(m, zi, zi);
  r.x = f_mul(m, p->x, zi2);
  r.y = f_mul(m, p->y, f_mul(m, zi2, zi));
  return r;
}

/* ---------------------------------------------------------------- ark MSM */
static size_t ln_without_floats(size_t a) { /* log2(a) * 69 / 100 */
  size_t l = 0;
  while (((size_t)1 << (l + 1)) <= a) l++;
  return l * 69 / 100;
}

/* signed digits of a canonical 254-bit scalar (ark-ec make_digits) */
static void make_digits(const uint64_t s[4], int w, int num_bits, int64_t* out) {
  const uint64_t radix = 1ull << w, mask = radix - 1;
  uint64_t carry = 0;
  const int count = (num_bits + w - 1) / w;
  for (int i = 0; i < count; i++) {
    int bit_offset = i * w, u64_idx = bit_offset / 64, bit_idx = bit_offset % 64;
    uint64_t buf;
    if (bit_idx < 64 - w || u64_idx == 3) buf = s[u64_idx] >> bit_idx;
    else buf = (s[u64_idx] >> bit_idx) | (s[u64_idx + 1] << (64 - bit_idx));
    uint64_t coef = carry + (buf & mask);
    carry = (coef + radix / 2) >> w;
    int64_t digit = (int64_t)coef - (int64_t)(carry << w);
    if (i == count - 1) digit += (int64_t)(carry << w);
    out[i] = digit;
  }
}

/* scalars: Montgomery Fr (4 x u64 each); bases affine */
static g1j msm_ark(const g1a* bases, const fp* scalars, size_t n) {
  const int c = n < 32 ? 3 : (int)ln_without_floats(n) + 2;
  const int num_bits = 254;
  const int digits = (num_bits + c - 1) / c;
  int64_t* dig = (int64_t*)malloc(sizeof(int64_t) * digits * (n ? n : 1));
  for (size_t i = 0; i < n; i++) {
    fp cs = f_from_mont(&FR, scalars[i]);
    make_digits(cs.v, c, num_bits, dig + i * digits);
  }
  g1j* buckets = (g1j*)malloc(sizeof(g1j) << c);
  g1j* win = (g1j*)malloc(sizeof(g1j) * digits);
  for (int w = 0; w < digits; w++) {
    for (size_t b = 0; b < ((size_t)1 << c); b++) buckets[b] = j_zero();
    for (size_t i = 0; i < n; i++) {
      int64_t d = dig[i * digits + w];
      if (d > 0) {
        j_add_affine(&buckets[d - 1], &bases[i]);
      } else if (d < 0) {
        g1a nb = bases[i];
        if (!nb.inf) nb.y = f_sub(&FQ, (fp){{0, 0, 0, 0}}, nb.y);
        j_add_affine(&buckets[-d - 1], &nb);
      }
    }
    g1j run = j_zero(), res = j_zero();
    for (size_t b = ((size_t)1 << c); b-- > 0;) {
      j_add(&run, &buckets[b]);
      j_add(&res, &run);
    }
    win[w] = res;
  }
  g1j total = j_zero();
  for (int w = digits - 1; w >= 1; w--) {
    j_add(&total, &win[w]);
    for (int k = 0; k < c; k++) j_double(&total);
  }
  j_add(&total, &win[0]);
  free(dig);
  free(buckets);
  free(win);
  return total;
}

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + ts.tv_nsec * 1e-9;
}

/* ---------------------------------------------------------------- exported */
/* out_xy: affine Montgomery (8 u64) + inf flag.  bases: n x 8 u64 (+ inf flags) */
int oc_msm(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n,
           uint64_t out_xy[8], uint8_t* out_inf) {
  g1a* b = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
  for (size_t i = 0; i < n; i++) {
    memcpy(b[i].x.v, bases_xy + 8 * i, 32);
    memcpy(b[i].y.v, bases_xy + 8 * i + 4, 32);
    b[i].inf = inf ? inf[i] : 0;
  }
  g1j r = msm_ark(b, (const fp*)scalars, n);
  g1a a = j_to_affine(&r);
  memcpy(out_xy, a.x.v, 32);
  memcpy(out_xy + 4, a.y.v, 32);
  *out_inf = (uint8_t)a.inf;
  free(b);
  return 0;
}

/* CPU baseline on caller-provided arrays (e.g. a prefix of the GPU bench's own
 * SRS and scalars): times msm_ark alone and KZG::commit as written, i.e. plus
 * the per-call into_affine of every (projective) SRS point (kzg.rs:67-71). */
int oc_bench_msm_arrays(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars,
                        size_t n, double* t_msm, double* t_commit, uint64_t out_xy[8],
                        uint8_t* out_inf) {
  g1a* b = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
  g1j* proj = (g1j*)malloc(sizeof(g1j) * (n ? n : 1));
  fp z = f_add(&FQ, f_one(&FQ), f_one(&FQ));
  fp z2 = f_mul(&FQ, z, z), z3 = f_mul(&FQ, z2, z);
  for (size_t i = 0; i < n; i++) {
    memcpy(b[i].x.v, bases_xy + 8 * i, 32);
    memcpy(b[i].y.v, bases_xy + 8 * i + 4, 32);
    b[i].inf = inf ? inf[i] : 0;
    proj[i].x = f_mul(&FQ, b[i].x, z2);
    proj[i].y = f_mul(&FQ, b[i].y, z3);
    proj[i].z = b[i].inf ? (fp){{0, 0, 0, 0}} : z;
  }
  double a = now_s();
  g1j r = msm_ark(b, (const fp*)scalars, n);
  double m = now_s();
  g1a* conv = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
  for (size_t i = 0; i < n; i++) conv[i] = j_to_affine(&proj[i]);
  double c = now_s();
  *t_msm = m - a;
  *t_commit = c - a;
  g1a ra = j_to_affine(&r);
  memcpy(out_xy, ra.x.v, 32);
  memcpy(out_xy + 4, ra.y.v, 32);
  *out_inf = (uint8_t)ra.inf;
  free(b);
  free(proj);
  free(conv);
  return 0;
}

/* [tau^i] g for i < n via a 32 x 256 fixed-base comb on g (bases for the baseline) */
static void gen_srs(fp tau_mont, size_t n, g1a* out) {
  const modulus* m = &FQ;
  g1a g;
  memset(&g, 0, sizeof g);
  fp one = {{1, 0, 0, 0}}, two = {{2, 0, 0, 0}};
  g.x = f_to_mont(m, one);
  g.y = f_to_mont(m, two);
  g1a* tbl = (g1a*)malloc(sizeof(g1a) * 32 * 256);
  g1j base;
  base.x = g.x;
  base.y = g.y;
  base.z = f_one(m);
  for (int k = 0; k < 32; k++) {
    g1j acc = j_zero();
    for (int j = 0; j < 256; j++) {
      tbl[k * 256 + j] = j_to_affine(&acc);
      j_add(&acc, &base);
    }
    for (int d = 0; d < 8; d++) j_double(&base);
  }
  fp t = f_one(&FR);
  for (size_t i = 0; i < n; i++) {
    fp c = f_from_mont(&FR, t);
    g1j acc = j_zero();
    for (int k = 0; k < 32; k++) {
      unsigned byte = (unsigned)((c.v[k / 8] >> (8 * (k % 8))) & 255);
      if (byte) j_add_affine(&acc, &tbl[k * 256 + byte]);
    }
    out[i] = j_to_affine(&acc);
    t = f_mul(&FR, t, tau_mont);
  }
  free(tbl);
}

static uint64_t sm_state;
static uint64_t splitmix(void) {
  uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fp rand_fr(void) {
  for (;;) {
    fp v;
    for (int i = 0; i < 4; i++) v.v[i] = splitmix();
    v.v[3] &= (1ull << 62) - 1;
    if (!geq(v.v, FR.p)) return f_to_mont(&FR, v);
  }
}

/*
 * Timed baseline on a sample of n = 2^log_n scalars (single thread):
 *   t_msm    : msm_unchecked only (bases already affine)
 *   t_commit : KZG::commit as written = into_affine of all SRS points + MSM
 * Returns 0; writes seconds.
 */
int oc_bench_msm(int log_n, uint64_t seed, double* t_msm, double* t_commit, uint64_t out_xy[8]) {
  size_t n = (size_t)1 << log_n;
  sm_state = seed;
  g1a* bases = (g1a*)malloc(sizeof(g1a) * n);
  fp* sc = (fp*)malloc(sizeof(fp) * n);
  fp tau = rand_fr();
  gen_srs(tau, n, bases);
  for (size_t i = 0; i < n; i++) sc[i] = rand_fr();
  /* KZG keeps g1_points in projective form (kzg.rs:20); convert on each commit */
  g1j* proj = (g1j*)malloc(sizeof(g1j) * n);
  for (size_t i = 0; i < n; i++) {
    proj[i].x = bases[i].x;
    proj[i].y = bases[i].y;
    proj[i].z = f_one(&FQ);
    /* scale Z so the projective representation is non-trivial, like a computed SRS */
    fp z = f_add(&FQ, f_one(&FQ), f_one(&FQ));
    fp z2 = f_mul(&FQ, z, z);
    proj[i].x = f_mul(&FQ, proj[i].x, z2);
    proj[i].y = f_mul(&FQ, proj[i].y, f_mul(&FQ, z2, z));
    proj[i].z = z;
  }
  double a = now_s();
  g1j r = msm_ark(bases, sc, n);
  double b = now_s();
  g1a* conv = (g1a*)malloc(sizeof(g1a) * n);
  for (size_t i = 0; i < n; i++) conv[i] = j_to_affine(&proj[i]);
  double c = now_s();
  *t_msm = b - a;
  *t_commit = (c - b) + (b - a);
  g1a ra = j_to_affine(&r);
  memcpy(out_xy, ra.x.v, 32);
  memcpy(out_xy + 4, ra.y.v, 32);
  free(bases);
  free(sc);
  free(proj);
  free(conv);
  return 0;
}

/* ---------------------------------------------------------------- BLAKE3 + sumcheck */
static const uint32_t B3IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
static const int B3P[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
#define ROTR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))
static void b3g(uint32_t* s, int a, int b, int c, int d, uint32_t x, uint32_t y) {
  s[a] += s[b] + x; s[d] = ROTR(s[d] ^ s[a], 16); s[c] += s[d]; s[b] = ROTR(s[b] ^ s[c], 12);
  s[a] += s[b] + y; s[d] = ROTR(s[d] ^ s[a], 8);  s[c] += s[d]; s[b] = ROTR(s[b] ^ s[c], 7);
}
static void b3c(const uint32_t cv[8], const uint32_t blk[16], uint64_t ctr, uint32_t len,
                uint32_t flags, uint32_t out[16]) {
  uint32_t s[16], m[16], t[16];
  for (int i = 0; i < 8; i++) s[i] = cv[i];
  for (int i = 0; i < 4; i++) s[8 + i] = B3IV[i];
  s[12] = (uint32_t)ctr; s[13] = (uint32_t)(ctr >> 32); s[14] = len; s[15] = flags;
  memcpy(m, blk, 64);
  for (int r = 0; r < 7; r++) {
    b3g(s, 0, 4, 8, 12, m[0], m[1]); b3g(s, 1, 5, 9, 13, m[2], m[3]);
    b3g(s, 2, 6, 10, 14, m[4], m[5]); b3g(s, 3, 7, 11, 15, m[6], m[7]);
    b3g(s, 0, 5, 10, 15, m[8], m[9]); b3g(s, 1, 6, 11, 12, m[10], m[11]);
    b3g(s, 2, 7, 8, 13, m[12], m[13]); b3g(s, 3, 4, 9, 14, m[14], m[15]);
    for (int i = 0; i < 16; i++) t[i] = m[B3P[i]];
    memcpy(m, t, 64);
  }
  for (int i = 0; i < 8; i++) { out[i] = s[i] ^ s[i + 8]; out[i + 8] = s[i + 8] ^ cv[i]; }
}
/* single-chunk BLAKE3 XOF (inputs < 1024 bytes: all sumcheck transcript messages) */
static void b3_small(const uint8_t* in, size_t len, uint8_t* out, size_t olen) {
  uint32_t cv[8], blk[16], o[16];
  memcpy(cv, B3IV, 32);
  size_t nblk = len ? (len + 63) / 64 : 1;
  for (size_t b = 0; b < nblk; b++) {
    uint8_t buf[64] = {0};
    size_t take = len - b * 64 < 64 ? len - b * 64 : 64;
    if (len) memcpy(buf, in + b * 64, take);
    for (int i = 0; i < 16; i++)
      blk[i] = buf[4*i] | (buf[4*i+1] << 8) | (buf[4*i+2] << 16) | ((uint32_t)buf[4*i+3] << 24);
    uint32_t flags = (b == 0 ? 1 : 0) | (b == nblk - 1 ? 2 : 0);
    if (b == nblk - 1) {
      size_t pos = 0;
      for (uint64_t ctr = 0; pos < olen; ctr++) {
        b3c(cv, blk, ctr, (uint32_t)(len ? take : 0), flags | 8, o);
        for (int i = 0; i < 64 && pos < olen; i++) out[pos++] = (uint8_t)(o[i / 4] >> (8 * (i % 4)));
      }
    } else {
      b3c(cv, blk, 0, 64, flags, o);
      memcpy(cv, o, 32);
    }
  }
}
static void tr_append(uint8_t st[32], const uint8_t* msg, size_t len) {
  uint8_t buf[1024];
  memcpy(buf, st, 32);
  memcpy(buf + 32, msg, len);
  b3_small(buf, 32 + len, st, 32);
}
static fp tr_draw_fr(uint8_t st[32]) {
  uint8_t buf[41], ch[48];
  memcpy(buf, st, 32);
  memcpy(buf + 32, "challenge", 9);
  b3_small(buf, 41, ch, 48);
  tr_append(st, ch, 48);
  fp lo, hi = {{0, 0, 0, 0}};
  memcpy(lo.v, ch, 32);
  memcpy(hi.v, ch + 32, 16);
  /* lo is any 256-bit value: reduce mod r first (the no-carry CIOS needs
     operands < r; 2^256 < 6r) */
  while (geq(lo.v, FR.p)) sub4(lo.v, lo.v, FR.p);
  fp r2, r3;
  memcpy(r2.v, FR.r2, 32);
  r3 = f_mul(&FR, r2, r2); /* R^2*R^2/R = R^3 */
  return f_add(&FR, f_mul(&FR, lo, r2), f_mul(&FR, hi, r3));
}
static void fr_bytes(fp x, uint8_t* out) {
  fp c = f_from_mont(&FR, x);
  memcpy(out, c.v, 32);
}

/*
 * Sumcheck prover for h = prod_{i<k} g_i, tables Montgomery (k x 2^nvars),
 * transcript state in/out.  Writes round coefficients (nvars x (k+1), trimmed
 * lengths in lens) and the point.  Tables are copied (the reference clones).
 */
int oc_sumcheck_prod(int nvars, int k, const uint64_t* tables, const uint64_t claimed[4],
                     uint8_t state[32], uint64_t* coeffs, uint32_t* lens, uint64_t* point,
                     uint64_t evaluation[4]) {
  size_t N = (size_t)1 << nvars;
  fp* g = (fp*)malloc(sizeof(fp) * N * k);
  memcpy(g, tables, sizeof(fp) * N * k);
  uint8_t m8[8];
  for (int i = 0; i < 8; i++) m8[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
  tr_append(state, m8, 8);
  uint8_t b32[32];
  fp cs;
  memcpy(cs.v, claimed, 32);
  fr_bytes(cs, b32);
  tr_append(state, b32, 32);
  const int np = k + 1;
  /* inverse Vandermonde on 0..k */
  fp V[16][16];
  for (int j = 0; j < np; j++) {
    fp poly[17] = {{{0}}};
    poly[0] = f_one(&FR);
    int deg = 0;
    fp den = f_one(&FR);
    for (int mm = 0; mm < np; mm++) {
      if (mm == j) continue;
      fp nm = {{(uint64_t)mm, 0, 0, 0}};
      nm = f_sub(&FR, (fp){{0, 0, 0, 0}}, f_to_mont(&FR, nm));
      fp np2[17] = {{{0}}};
      for (int t = 0; t <= deg; t++) {
        np2[t] = f_add(&FR, np2[t], f_mul(&FR, poly[t], nm));
        np2[t + 1] = f_add(&FR, np2[t + 1], poly[t]);
      }
      deg++;
      memcpy(poly, np2, sizeof poly);
      int64_t d = j - mm;
      fp dd = {{(uint64_t)(d < 0 ? -d : d), 0, 0, 0}};
      dd = f_to_mont(&FR, dd);
      if (d < 0) dd = f_sub(&FR, (fp){{0, 0, 0, 0}}, dd);
      den = f_mul(&FR, den, dd);
    }
    fp di = f_inv(&FR, den);
    for (int t = 0; t < np; t++) V[t][j] = f_mul(&FR, poly[t], di);
  }
  size_t half = N;
  for (int j = 0; j < nvars; j++) {
    half >>= 1;
    fp sums[16];
    for (int t = 0; t < np; t++) sums[t] = (fp){{0, 0, 0, 0}};
    for (size_t p = 0; p < half; p++) {
      fp lo[8], df[8];
      for (int i = 0; i < k; i++) {
        lo[i] = g[i * N + 2 * p];
        df[i] = f_sub(&FR, g[i * N + 2 * p + 1], lo[i]);
      }
      for (int t = 0; t < np; t++) {
        if (t) for (int i = 0; i < k; i++) lo[i] = f_add(&FR, lo[i], df[i]);
        fp prod = lo[0];
        for (int i = 1; i < k; i++) prod = f_mul(&FR, prod, lo[i]);
        sums[t] = f_add(&FR, sums[t], prod);
      }
    }
    fp co[16];
    uint32_t len = 0;
    for (int t = 0; t < np; t++) {
      fp acc = {{0, 0, 0, 0}};
      for (int u = 0; u < np; u++) acc = f_add(&FR, acc, f_mul(&FR, V[t][u], sums[u]));
      co[t] = acc;
      if (!f_is_zero(acc)) len = t + 1;
    }
    uint8_t msg[8 + 16 * 32];
    for (int i = 0; i < 8; i++) msg[i] = (uint8_t)((uint64_t)len >> (8 * i));
    for (uint32_t t = 0; t < len; t++) fr_bytes(co[t], msg + 8 + 32 * t);
    tr_append(state, msg, 8 + 32 * len);
    fp r = tr_draw_fr(state);
    for (int t = 0; t < np; t++) memcpy(coeffs + 4 * ((size_t)j * np + t), (t < (int)len ? co[t] : (fp){{0,0,0,0}}).v, 32);
    lens[j] = len;
    memcpy(point + 4 * j, r.v, 32);
    for (int i = 0; i < k; i++)
      for (size_t p = 0; p < half; p++) {
        fp a = g[i * N + 2 * p], b = g[i * N + 2 * p + 1];
        g[i * N + p] = f_add(&FR, a, f_mul(&FR, r, f_sub(&FR, b, a)));
      }
  }
  fp e = g[0];
  for (int i = 1; i < k; i++) e = f_mul(&FR, e, g[i * N]);
  memcpy(evaluation, e.v, 32);
  free(g);
  return 0;
}

/* Timed sumcheck baseline on 2^log_n, k = 3 random tables. */
int oc_bench_sumcheck(int log_n, uint64_t seed, double* seconds) {
  size_t N = (size_t)1 << log_n;
  sm_state = seed;
  fp* t = (fp*)malloc(sizeof(fp) * N * 3);
  for (size_t i = 0; i < 3 * N; i++) t[i] = rand_fr();
  uint8_t st[32] = {0};
  uint64_t cl[4] = {0, 0, 0, 0};
  uint64_t* co = (uint64_t*)malloc(sizeof(uint64_t) * 4 * 4 * log_n);
  uint32_t* lens = (uint32_t*)malloc(sizeof(uint32_t) * log_n);
  uint64_t* pt = (uint64_t*)malloc(sizeof(uint64_t) * 4 * log_n);
  uint64_t ev[4];
  double a = now_s();
  oc_sumcheck_prod(log_n, 3, (const uint64_t*)t, cl, st, co, lens, pt, ev);
  *seconds = now_s() - a;
  free(t);
  free(co);
  free(lens);
  free(pt);
  return 0;
}

/* ---------------------------------------------------------------- Logup */
static inline int u4_is_one(const uint64_t a[4]) { return a[0] == 1 && !(a[1] | a[2] | a[3]); }
static inline void u4_shr1(uint64_t a[4]) {
  for (int i = 0; i < 3; i++) a[i] = (a[i] >> 1) | (a[i + 1] << 63);
  a[3] >>= 1;
}
/* (x + p) / 2 for odd x < p (x + p < 2^255: no carry out of 256 bits) */
static inline void u4_add_p_shr1(const modulus* m, uint64_t x[4]) {
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)x[i] + m->p[i];
    x[i] = (uint64_t)c;
    c >>= 64;
  }
  u4_shr1(x);
}

/* ark-ff 0.5.0 Fp::inverse for Montgomery backends: binary extended Euclid
 * (Guide to ECC, Alg. 2.22) started at b = R^2, so aR -> a^{-1}R.  This is the
 * per-row `.inverse()` of multiset_check.rs:51,63 (zero has no inverse). */
static int f_inv_bea(const modulus* m, fp a, fp* out) {
  if (f_is_zero(a)) return -1;
  uint64_t u[4], v[4];
  fp b, c;
  memcpy(u, a.v, 32);
  memcpy(v, m->p, 32);
  memcpy(b.v, m->r2, 32);
  memset(c.v, 0, 32);
  while (!u4_is_one(u) && !u4_is_one(v)) {
    while (!(u[0] & 1)) {
      u4_shr1(u);
      if (b.v[0] & 1) u4_add_p_shr1(m, b.v);
      else u4_shr1(b.v);
    }
    while (!(v[0] & 1)) {
      u4_shr1(v);
      if (c.v[0] & 1) u4_add_p_shr1(m, c.v);
      else u4_shr1(c.v);
    }
    if (geq(u, v)) {
      sub4(u, u, v);
      b = f_sub(m, b, c);
    } else {
      sub4(v, v, u);
      c = f_sub(m, c, b);
    }
  }
  *out = u4_is_one(u) ? b : c;
  return 0;
}

/* Logup column as the reference computes it (multiset_check.rs:43-95 /
 * set_inclusion.rs:93-131) for h = t0 + a*t1 and multiplicities m = t2:
 * per row evaluate h, (beta + h).inverse(), then multiply by m.  Montgomery
 * limbs in and out; returns -1 at the first zero denominator (the panic),
 * else 0 and the single-thread wall time in *seconds. */
int oc_logup_column(const uint64_t* t0, const uint64_t* t1, const uint64_t* t2, size_t n,
                    const uint64_t a[4], const uint64_t beta[4], uint64_t* out, double* seconds) {
  fp A, B;
  memcpy(A.v, a, 32);
  memcpy(B.v, beta, 32);
  double s = now_s();
  for (size_t i = 0; i < n; i++) {
    fp x0, x1, x2, d, r;
    memcpy(x0.v, t0 + 4 * i, 32);
    memcpy(x1.v, t1 + 4 * i, 32);
    memcpy(x2.v, t2 + 4 * i, 32);
    d = f_add(&FR, B, f_add(&FR, x0, f_mul(&FR, A, x1)));
    if (f_inv_bea(&FR, d, &r)) return -1;
    r = f_mul(&FR, r, x2);
    memcpy(out + 4 * i, r.v, 32);
  }
  if (seconds) *seconds = now_s() - s;
  return 0;
}

/* ---------------------------------------------------------------- checkers
 * Size-independent checks of full-size device results (tests/, bench.py):
 * the trapdoor identity commit(p) = [p(tau)] g (kzg.rs:44-47, 61-73), MLE
 * evaluations (DenseMultilinearExtension::evaluate, bit j <-> point[j],
 * mlpcs.rs:91-94) and the sum of a product of tables (the claimed sum of
 * sumcheck.rs:28-34).  Montgomery limbs in and out. */

/* sum_i c_i x^i (Horner, ark-poly Polynomial::evaluate, kzg.rs:77-78) */
int oc_fr_horner(const uint64_t* coeffs, size_t n, const uint64_t x[4], uint64_t out[4]) {
  fp X, acc = {{0, 0, 0, 0}};
  memcpy(X.v, x, 32);
  for (size_t i = n; i-- > 0;) {
    fp c;
    memcpy(c.v, coeffs + 4 * i, 32);
    acc = f_add(&FR, f_mul(&FR, acc, X), c);
  }
  memcpy(out, acc.v, 32);
  return 0;
}

/* MLE of the first 2^nv entries at point (bit 0 folded first) */
int oc_fr_mle_eval(const uint64_t* table, int nv, const uint64_t* point, uint64_t out[4]) {
  size_t n = (size_t)1 << nv;
  fp* t = (fp*)malloc(sizeof(fp) * n);
  if (!t) return -1;
  memcpy(t, table, sizeof(fp) * n);
  for (int j = 0; j < nv; j++) {
    fp r;
    memcpy(r.v, point + 4 * j, 32);
    n >>= 1;
    for (size_t p = 0; p < n; p++)
      t[p] = f_add(&FR, t[2 * p], f_mul(&FR, r, f_sub(&FR, t[2 * p + 1], t[2 * p])));
  }
  memcpy(out, t[0].v, 32);
  free(t);
  return 0;
}

/* sum_i prod_{j<k} tables[j][i] */
int oc_fr_sum_prod(const uint64_t* const* tables, int k, size_t n, uint64_t out[4]) {
  fp acc = {{0, 0, 0, 0}};
  for (size_t i = 0; i < n; i++) {
    fp p;
    memcpy(p.v, tables[0] + 4 * i, 32);
    for (int j = 1; j < k; j++) {
      fp x;
      memcpy(x.v, tables[j] + 4 * i, 32);
      p = f_mul(&FR, p, x);
    }
    acc = f_add(&FR, acc, p);
  }
  memcpy(out, acc.v, 32);
  return 0;
}

/* [s] P (double-and-add over the canonical scalar); P affine Montgomery */
int oc_g1_mul(const uint64_t base_xy[8], uint8_t base_inf, const uint64_t s_mont[4],
              uint64_t out_xy[8], uint8_t* out_inf) {
  g1a b;
  memcpy(b.x.v, base_xy, 32);
  memcpy(b.y.v, base_xy + 4, 32);
  b.inf = base_inf;
  fp s;
  memcpy(s.v, s_mont, 32);
  s = f_from_mont(&FR, s);
  g1j acc = j_zero();
  for (int i = 3; i >= 0; i--)
    for (int bit = 63; bit >= 0; bit--) {
      j_double(&acc);
      if ((s.v[i] >> bit) & 1) j_add_affine(&acc, &b);
    }
  g1a r = j_to_affine(&acc);
  memcpy(out_xy, r.x.v, 32);
  memcpy(out_xy + 4, r.y.v, 32);
  *out_inf = (uint8_t)r.inf;
  return 0;
}

/* ================================================================ all-cores
 * Multi-threaded variants for the all-cores CPU baseline:
 * ark-ec's msm_bigint_wnaf with its `parallel` feature splits the windows
 * across threads (each window's bucket sum independent, the window combination
 * serial); the evaluation-form sumcheck splits each round's pairs.  The
 * reference itself builds without rayon, so these are labelled "all-cores
 * port", not the reference. */
#include <pthread.h>

typedef struct {
  const g1a* bases;
  const int64_t* dig;
  size_t n;
  int c, digits, w0, wstep;
  g1j* win;
} msm_task;

static void* msm_window_worker(void* arg) {
  msm_task* t = (msm_task*)arg;
  const size_t nbk = (size_t)1 << t->c;
  g1j* buckets = (g1j*)malloc(sizeof(g1j) * nbk);
  for (int w = t->w0; w < t->digits; w += t->wstep) {
    for (size_t b = 0; b < nbk; b++) buckets[b] = j_zero();
    for (size_t i = 0; i < t->n; i++) {
      int64_t d = t->dig[i * t->digits + w];
      if (d > 0) {
        j_add_affine(&buckets[d - 1], &t->bases[i]);
      } else if (d < 0) {
        g1a nb = t->bases[i];
        if (!nb.inf) nb.y = f_sub(&FQ, (fp){{0, 0, 0, 0}}, nb.y);
        j_add_affine(&buckets[-d - 1], &nb);
      }
    }
    g1j run = j_zero(), res = j_zero();
    for (size_t b = nbk; b-- > 0;) {
      j_add(&run, &buckets[b]);
      j_add(&res, &run);
    }
    t->win[w] = res;
  }
  free(buckets);
  return NULL;
}

static g1j msm_ark_mt(const g1a* bases, const fp* scalars, size_t n, int nthreads) {
  const int c = n < 32 ? 3 : (int)ln_without_floats(n) + 2;
  const int num_bits = 254;
  const int digits = (num_bits + c - 1) / c;
  int64_t* dig = (int64_t*)malloc(sizeof(int64_t) * digits * (n ? n : 1));
  for (size_t i = 0; i < n; i++) {
    fp cs = f_from_mont(&FR, scalars[i]);
    make_digits(cs.v, c, num_bits, dig + i * digits);
  }
  g1j* win = (g1j*)malloc(sizeof(g1j) * digits);
  if (nthreads > digits) nthreads = digits;
  if (nthreads < 1) nthreads = 1;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nthreads);
  msm_task* tk = (msm_task*)malloc(sizeof(msm_task) * nthreads);
  for (int t = 0; t < nthreads; t++) {
    tk[t] = (msm_task){bases, dig, n, c, digits, t, nthreads, win};
    pthread_create(&th[t], NULL, msm_window_worker, &tk[t]);
  }
  for (int t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
  g1j total = j_zero();
  for (int w = digits - 1; w >= 1; w--) {
    j_add(&total, &win[w]);
    for (int k = 0; k < c; k++) j_double(&total);
  }
  j_add(&total, &win[0]);
  free(dig);
  free(win);
  free(th);
  free(tk);
  return total;
}

/* all-cores MSM on caller arrays (same inputs as oc_bench_msm_arrays) */
int oc_bench_msm_arrays_mt(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars,
                           size_t n, int nthreads, double* t_msm, uint64_t out_xy[8],
                           uint8_t* out_inf) {
  g1a* b = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
  for (size_t i = 0; i < n; i++) {
    memcpy(b[i].x.v, bases_xy + 8 * i, 32);
    memcpy(b[i].y.v, bases_xy + 8 * i + 4, 32);
    b[i].inf = inf ? inf[i] : 0;
  }
  double a = now_s();
  g1j r = msm_ark_mt(b, (const fp*)scalars, n, nthreads);
  *t_msm = now_s() - a;
  g1a ra = j_to_affine(&r);
  memcpy(out_xy, ra.x.v, 32);
  memcpy(out_xy + 4, ra.y.v, 32);
  *out_inf = (uint8_t)ra.inf;
  free(b);
  return 0;
}

/* ------------------------------------------------ all-cores sumcheck (eval form) */
typedef struct {
  fp* g;        /* k tables of stride N (current round) */
  fp* fold_out; /* k tables of stride N (next round) */
  size_t N, p0, p1;
  int k, np;
  fp sums[16];
  fp r;
  int phase; /* 0: evaluate, 1: fold */
} sc_task;

static void* sc_worker(void* arg) {
  sc_task* t = (sc_task*)arg;
  if (t->phase == 0) {
    for (int u = 0; u < t->np; u++) t->sums[u] = (fp){{0, 0, 0, 0}};
    for (size_t p = t->p0; p < t->p1; p++) {
      fp lo[8], df[8];
      for (int i = 0; i < t->k; i++) {
        lo[i] = t->g[i * t->N + 2 * p];
        df[i] = f_sub(&FR, t->g[i * t->N + 2 * p + 1], lo[i]);
      }
      for (int u = 0; u < t->np; u++) {
        if (u) for (int i = 0; i < t->k; i++) lo[i] = f_add(&FR, lo[i], df[i]);
        fp prod = lo[0];
        for (int i = 1; i < t->k; i++) prod = f_mul(&FR, prod, lo[i]);
        t->sums[u] = f_add(&FR, t->sums[u], prod);
      }
    }
  } else {
    /* out of place (ping-pong): thread slices would race in place */
    for (int i = 0; i < t->k; i++)
      for (size_t p = t->p0; p < t->p1; p++) {
        fp a = t->g[i * t->N + 2 * p], b = t->g[i * t->N + 2 * p + 1];
        t->fold_out[i * t->N + p] = f_add(&FR, a, f_mul(&FR, t->r, f_sub(&FR, b, a)));
      }
  }
  return NULL;
}

/* inverse Vandermonde on the nodes 0..np-1 (as in oc_sumcheck_prod) */
static void sc_vandermonde(int np, fp V[16][16]) {
  for (int j = 0; j < np; j++) {
    fp poly[17] = {{{0}}};
    poly[0] = f_one(&FR);
    int deg = 0;
    fp den = f_one(&FR);
    for (int mm = 0; mm < np; mm++) {
      if (mm == j) continue;
      fp nm = {{(uint64_t)mm, 0, 0, 0}};
      nm = f_sub(&FR, (fp){{0, 0, 0, 0}}, f_to_mont(&FR, nm));
      fp np2[17] = {{{0}}};
      for (int t = 0; t <= deg; t++) {
        np2[t] = f_add(&FR, np2[t], f_mul(&FR, poly[t], nm));
        np2[t + 1] = f_add(&FR, np2[t + 1], poly[t]);
      }
      deg++;
      memcpy(poly, np2, sizeof poly);
      int64_t d = j - mm;
      fp dd = {{(uint64_t)(d < 0 ? -d : d), 0, 0, 0}};
      dd = f_to_mont(&FR, dd);
      if (d < 0) dd = f_sub(&FR, (fp){{0, 0, 0, 0}}, dd);
      den = f_mul(&FR, den, dd);
    }
    fp di = f_inv(&FR, den);
    for (int t = 0; t < np; t++) V[t][j] = f_mul(&FR, poly[t], di);
  }
}

/* round message from the np evaluations: coefficients, trim, absorb, draw r */
static fp sc_round_message(int np, fp V[16][16], const fp* sums, uint8_t state[32],
                           uint64_t* coeff_row, uint32_t* len_out) {
  fp co[16];
  uint32_t len = 0;
  for (int t = 0; t < np; t++) {
    fp acc = {{0, 0, 0, 0}};
    for (int u = 0; u < np; u++) acc = f_add(&FR, acc, f_mul(&FR, V[t][u], sums[u]));
    co[t] = acc;
    if (!f_is_zero(acc)) len = t + 1;
  }
  uint8_t msg[8 + 16 * 32];
  for (int i = 0; i < 8; i++) msg[i] = (uint8_t)((uint64_t)len >> (8 * i));
  for (uint32_t t = 0; t < len; t++) fr_bytes(co[t], msg + 8 + 32 * t);
  tr_append(state, msg, 8 + 32 * len);
  fp r = tr_draw_fr(state);
  for (int t = 0; t < np; t++)
    memcpy(coeff_row + 4 * t, (t < (int)len ? co[t] : (fp){{0, 0, 0, 0}}).v, 32);
  *len_out = len;
  return r;
}

/* evaluation-form sumcheck for h = prod of k tables on nthreads threads; same
 * transcript and outputs as oc_sumcheck_prod */
int oc_sumcheck_prod_mt(int nvars, int k, const uint64_t* tables, const uint64_t claimed[4],
                        uint8_t state[32], uint64_t* coeffs, uint32_t* lens, uint64_t* point,
                        uint64_t evaluation[4], int nthreads) {
  size_t N = (size_t)1 << nvars;
  fp* g = (fp*)malloc(sizeof(fp) * N * k);
  fp* g2 = (fp*)malloc(sizeof(fp) * N * k);
  memcpy(g, tables, sizeof(fp) * N * k);
  uint8_t m8[8];
  for (int i = 0; i < 8; i++) m8[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
  tr_append(state, m8, 8);
  uint8_t b32[32];
  fp cs;
  memcpy(cs.v, claimed, 32);
  fr_bytes(cs, b32);
  tr_append(state, b32, 32);
  const int np = k + 1;
  fp V[16][16];
  sc_vandermonde(np, V);
  if (nthreads < 1) nthreads = 1;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nthreads);
  sc_task* tk = (sc_task*)malloc(sizeof(sc_task) * nthreads);
  size_t half = N;
  for (int j = 0; j < nvars; j++) {
    half >>= 1;
    const int nt = half < (size_t)nthreads * 64 ? 1 : nthreads;
    for (int t = 0; t < nt; t++) {
      tk[t] = (sc_task){g, g2, N, half * t / nt, half * (t + 1) / nt, k, np, {{{0}}}, {{0}}, 0};
      pthread_create(&th[t], NULL, sc_worker, &tk[t]);
    }
    for (int t = 0; t < nt; t++) pthread_join(th[t], NULL);
    fp sums[16];
    for (int u = 0; u < np; u++) {
      sums[u] = (fp){{0, 0, 0, 0}};
      for (int t = 0; t < nt; t++) sums[u] = f_add(&FR, sums[u], tk[t].sums[u]);
    }
    fp r = sc_round_message(np, V, sums, state, coeffs + 4 * (size_t)j * np, &lens[j]);
    memcpy(point + 4 * j, r.v, 32);
    for (int t = 0; t < nt; t++) {
      tk[t].phase = 1;
      tk[t].r = r;
      pthread_create(&th[t], NULL, sc_worker, &tk[t]);
    }
    for (int t = 0; t < nt; t++) pthread_join(th[t], NULL);
    fp* tmp = g;
    g = g2;
    g2 = tmp;
  }
  fp e = g[0];
  for (int i = 1; i < k; i++) e = f_mul(&FR, e, g[i * N]);
  memcpy(evaluation, e.v, 32);
  free(g);
  free(g2);
  free(th);
  free(tk);
  return 0;
}

/* ======================================================= reference structure
 * The reference's prover data flow (sumcheck.rs:28-114) restated with its
 * costs: every store table cloned (:44-49); per round a Vec<Vec<Dense-
 * Polynomial>> of 2^i x k heap polynomials lo + X (hi - lo) (:52-63); per pair
 * evaluate_poly's recursive expression walk (virtual_polynomial.rs:300-320):
 * Input clones its polynomial, Mul is ark-poly's &a * &b — a
 * GeneralEvaluationDomain of the product length (its generator by powering
 * the 2^28 root, size_inv by a field inversion), FFT of both operands,
 * pointwise product, IFFT, trim — and the per-pair results are summed with
 * DensePolynomial + (a fresh trimmed vector per addition); the fold evaluates
 * every pair polynomial at r (poly.evaluate, :81-90).  For h = g0 g1 ... (a
 * left-deep Mul tree).  Same transcript and outputs as oc_sumcheck_prod. */
typedef struct { fp* c; int n; } dpoly;

static void dp_trim(dpoly* a) {
  while (a->n > 0 && f_is_zero(a->c[a->n - 1])) a->n--;
}
static dpoly dp_new(int n) {
  dpoly r = {(fp*)calloc(n ? n : 1, sizeof(fp)), n};
  return r;
}
static dpoly dp_clone(const dpoly* a) {
  dpoly r = dp_new(a->n);
  memcpy(r.c, a->c, sizeof(fp) * a->n);
  return r;
}
static void dp_free(dpoly* a) {
  free(a->c);
  a->c = NULL;
  a->n = 0;
}

/* radix-2 domain of size 2^lg: generator = (2^28-th root)^(2^(28 - lg)), its
 * inverse and size_inv by inversions (ark-poly Radix2EvaluationDomain::new) */
typedef struct { int lg; fp g, gi, size_inv; } dom;
static fp fr_root28(void) {
  /* 5^((r - 1) / 2^28) (the two-adic root of ark-bn254 Fr), cached */
  static int done = 0;
  static fp w;
  if (!done) {
    uint64_t e[4];
    memcpy(e, FR.p, 32);
    e[0] -= 1;
    for (int k = 0; k < 28; k++)
      for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i < 3 ? (e[i + 1] << 63) : 0);
    fp five = f_to_mont(&FR, (fp){{5, 0, 0, 0}});
    w = f_one(&FR);
    for (int i = 3; i >= 0; i--)
      for (int b = 63; b >= 0; b--) {
        w = f_mul(&FR, w, w);
        if ((e[i] >> b) & 1) w = f_mul(&FR, w, five);
      }
    done = 1;
  }
  return w;
}
static dom dom_new(int n) {
  dom d;
  d.lg = 0;
  while ((1 << d.lg) < n) d.lg++;
  fp g = fr_root28();
  for (int i = d.lg; i < 28; i++) g = f_mul(&FR, g, g);
  d.g = g;
  d.gi = f_inv(&FR, g);
  d.size_inv = f_inv(&FR, f_to_mont(&FR, (fp){{(uint64_t)1 << d.lg, 0, 0, 0}}));
  return d;
}
static void fft_inplace(fp* a, int lg, fp w) {
  const int n = 1 << lg;
  for (int i = 1, j = 0; i < n; i++) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      fp t = a[i];
      a[i] = a[j];
      a[j] = t;
    }
  }
  for (int len = 2; len <= n; len <<= 1) {
    fp wl = w;
    for (int k = len; k < n; k <<= 1) wl = f_mul(&FR, wl, wl);
    for (int i = 0; i < n; i += len) {
      fp x = f_one(&FR);
      for (int j = 0; j < len / 2; j++) {
        fp u = a[i + j], v = f_mul(&FR, a[i + j + len / 2], x);
        a[i + j] = f_add(&FR, u, v);
        a[i + j + len / 2] = f_sub(&FR, u, v);
        x = f_mul(&FR, x, wl);
      }
    }
  }
}
/* ark-poly &a * &b (both nonzero) */
static dpoly dp_mul(const dpoly* a, const dpoly* b) {
  if (a->n == 0 || b->n == 0) return dp_new(0);
  dom d = dom_new(a->n + b->n - 1);
  const int n = 1 << d.lg;
  fp* x = (fp*)calloc(n, sizeof(fp));
  fp* y = (fp*)calloc(n, sizeof(fp));
  memcpy(x, a->c, sizeof(fp) * a->n);
  memcpy(y, b->c, sizeof(fp) * b->n);
  fft_inplace(x, d.lg, d.g);
  fft_inplace(y, d.lg, d.g);
  for (int i = 0; i < n; i++) x[i] = f_mul(&FR, x[i], y[i]);
  fft_inplace(x, d.lg, d.gi);
  dpoly r = dp_new(n);
  for (int i = 0; i < n; i++) r.c[i] = f_mul(&FR, x[i], d.size_inv);
  free(x);
  free(y);
  dp_trim(&r);
  return r;
}
static dpoly dp_add(const dpoly* a, const dpoly* b) {
  const int n = a->n > b->n ? a->n : b->n;
  dpoly r = dp_new(n);
  for (int i = 0; i < n; i++) {
    fp u = i < a->n ? a->c[i] : (fp){{0, 0, 0, 0}};
    fp v = i < b->n ? b->c[i] : (fp){{0, 0, 0, 0}};
    r.c[i] = f_add(&FR, u, v);
  }
  dp_trim(&r);
  return r;
}

int oc_sumcheck_ref_prod(int nvars, int k, const uint64_t* tables, const uint64_t claimed[4],
                         uint8_t state[32], uint64_t* coeffs, uint32_t* lens, uint64_t* point,
                         uint64_t evaluation[4]) {
  size_t N = (size_t)1 << nvars;
  /* gs_local: a clone of every table */
  fp** gs = (fp**)malloc(sizeof(fp*) * k);
  for (int i = 0; i < k; i++) {
    gs[i] = (fp*)malloc(sizeof(fp) * N);
    memcpy(gs[i], tables + 4 * N * i, sizeof(fp) * N);
  }
  uint8_t m8[8];
  for (int i = 0; i < 8; i++) m8[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
  tr_append(state, m8, 8);
  uint8_t b32[32];
  fp cs;
  memcpy(cs.v, claimed, 32);
  fr_bytes(cs, b32);
  tr_append(state, b32, 32);
  const int np = k + 1;
  for (int j = 0; j < nvars; j++) {
    const size_t half = N >> (j + 1);
    /* r_polys: 2^i x k polynomials low + X (high - low) */
    dpoly* rp = (dpoly*)malloc(sizeof(dpoly) * half * k);
    for (size_t p = 0; p < half; p++)
      for (int i = 0; i < k; i++) {
        dpoly q = dp_new(2);
        q.c[0] = gs[i][2 * p];
        q.c[1] = f_sub(&FR, gs[i][2 * p + 1], q.c[0]);
        dp_trim(&q); /* DensePolynomial::from_coefficients_vec trims */
        rp[p * k + i] = q;
      }
    /* next_message = sum over pairs of evaluate_poly (left-deep product) */
    dpoly msg = dp_new(0);
    for (size_t p = 0; p < half; p++) {
      dpoly acc = dp_clone(&rp[p * k]); /* Input(0) clones */
      for (int i = 1; i < k; i++) {
        dpoly in = dp_clone(&rp[p * k + i]);
        dpoly prod = dp_mul(&acc, &in);
        dp_free(&acc);
        dp_free(&in);
        acc = prod;
      }
      dpoly sum = dp_add(&msg, &acc);
      dp_free(&msg);
      dp_free(&acc);
      msg = sum;
    }
    /* append the DensePolynomial (u64 length + coefficients), draw r */
    uint8_t* mb = (uint8_t*)malloc(8 + 32 * (size_t)(msg.n ? msg.n : 1));
    for (int i = 0; i < 8; i++) mb[i] = (uint8_t)((uint64_t)msg.n >> (8 * i));
    for (int t = 0; t < msg.n; t++) fr_bytes(msg.c[t], mb + 8 + 32 * t);
    tr_append(state, mb, 8 + 32 * (size_t)msg.n);
    free(mb);
    fp r = tr_draw_fr(state);
    for (int t = 0; t < np; t++)
      memcpy(coeffs + 4 * ((size_t)j * np + t), (t < msg.n ? msg.c[t] : (fp){{0, 0, 0, 0}}).v, 32);
    lens[j] = (uint32_t)msg.n;
    memcpy(point + 4 * j, r.v, 32);
    dp_free(&msg);
    /* new gs_local: every pair polynomial evaluated at r (Horner) */
    for (int i = 0; i < k; i++) {
      fp* ng = (fp*)malloc(sizeof(fp) * (half ? half : 1));
      for (size_t p = 0; p < half; p++) {
        const dpoly* q = &rp[p * k + i];
        fp e = {{0, 0, 0, 0}};
        for (int t = q->n; t-- > 0;) e = f_add(&FR, f_mul(&FR, e, r), q->c[t]);
        ng[p] = e;
      }
      free(gs[i]);
      gs[i] = ng;
    }
    for (size_t p = 0; p < half * k; p++) dp_free(&rp[p]);
    free(rp);
  }
  fp e = gs[0][0];
  for (int i = 1; i < k; i++) e = f_mul(&FR, e, gs[i][0]);
  memcpy(evaluation, e.v, 32);
  for (int i = 0; i < k; i++) free(gs[i]);
  free(gs);
  return 0;
}

/* timed baselines on 2^log_n, k = 3 random tables (same generator as
 * oc_bench_sumcheck): reference-structured single thread, eval form all cores */
int oc_bench_sumcheck_ref(int log_n, uint64_t seed, double* seconds) {
  size_t N = (size_t)1 << log_n;
  sm_state = seed;
  fp* t = (fp*)malloc(sizeof(fp) * N * 3);
  for (size_t i = 0; i < 3 * N; i++) t[i] = rand_fr();
  uint8_t st[32] = {0};
  uint64_t cl[4] = {0, 0, 0, 0};
  uint64_t* co = (uint64_t*)malloc(sizeof(uint64_t) * 4 * 4 * log_n);
  uint32_t* lens = (uint32_t*)malloc(sizeof(uint32_t) * log_n);
  uint64_t* pt = (uint64_t*)malloc(sizeof(uint64_t) * 4 * log_n);
  uint64_t ev[4];
  double a = now_s();
  oc_sumcheck_ref_prod(log_n, 3, (const uint64_t*)t, cl, st, co, lens, pt, ev);
  *seconds = now_s() - a;
  free(t);
  free(co);
  free(lens);
  free(pt);
  return 0;
}

int oc_bench_sumcheck_mt(int log_n, uint64_t seed, int nthreads, double* seconds) {
  size_t N = (size_t)1 << log_n;
  sm_state = seed;
  fp* t = (fp*)malloc(sizeof(fp) * N * 3);
  for (size_t i = 0; i < 3 * N; i++) t[i] = rand_fr();
  uint8_t st[32] = {0};
  uint64_t cl[4] = {0, 0, 0, 0};
  uint64_t* co = (uint64_t*)malloc(sizeof(uint64_t) * 4 * 4 * log_n);
  uint32_t* lens = (uint32_t*)malloc(sizeof(uint32_t) * log_n);
  uint64_t* pt = (uint64_t*)malloc(sizeof(uint64_t) * 4 * log_n);
  uint64_t ev[4];
  double a = now_s();
  oc_sumcheck_prod_mt(log_n, 3, (const uint64_t*)t, cl, st, co, lens, pt, ev, nthreads);
  *seconds = now_s() - a;
  free(t);
  free(co);
  free(lens);
  free(pt);
  return 0;
}

/* ---------------------------------------------------------------- MLEvalProof::prove
 * mlpcs.rs:83-124 as the reference runs it (single thread, ark-poly data flow):
 *   pr = compute_pr(point): eval_pr (mlpcs.rs:52-63) at the 2^n domain elements,
 *        then the domain's IFFT (mlpcs.rs:68-78);
 *   evaluation = <poly, pr> over the common prefix (mlpcs.rs:91-94);
 *   S = compute_s_polynomial(poly, pr) (ipa.rs:122-157): poly * rev(pr) +
 *       rev(poly) * pr with ark-poly FFT products (dp_mul), h[M ..], trimmed;
 *   s_comm = commit(S) (msm_ark); transcript: point, evaluation, s_comm; r;
 *   four KZG::open (kzg.rs:75-96): y = p(x) (Horner), q = (p - y) / (X - x)
 *       (long division), assert q (X - x) == p - y (an FFT product, as the
 *       reference's assert! does), commit(q).
 * Bases [tau^i] g are generated before the clock starts.  Outputs for the
 * parity test; *seconds = the timed prove. */
static fp eval_pr_c(const fp* r, int n, fp x) {
  fp acc = f_one(&FR), one = f_one(&FR);
  for (int i = 0; i < n; i++) {
    acc = f_mul(&FR, acc, f_add(&FR, f_mul(&FR, r[i], x), f_sub(&FR, one, r[i])));
    x = f_mul(&FR, x, x);
  }
  return acc;
}
static void g1_ser_c(const g1a* a, uint8_t out[64]) {
  memset(out, 0, 64);
  if (a->inf) {
    out[63] |= 0x40;
    return;
  }
  fp x = f_from_mont(&FQ, a->x), y = f_from_mont(&FQ, a->y);
  fp ny = f_from_mont(&FQ, f_sub(&FQ, (fp){{0, 0, 0, 0}}, a->y));
  memcpy(out, x.v, 32);
  memcpy(out + 32, y.v, 32);
  int gt = 0;
  for (int i = 3; i >= 0; i--)
    if (y.v[i] != ny.v[i]) {
      gt = y.v[i] > ny.v[i];
      break;
    }
  if (gt) out[63] |= 0x80;
}
static void kzg_open_c(const g1a* bases, const fp* c, int n, fp x, fp* y_out, g1a* pi_out) {
  dpoly p = dp_new(n);
  memcpy(p.c, c, sizeof(fp) * n);
  dp_trim(&p);
  fp y = (fp){{0, 0, 0, 0}};
  for (int i = p.n; i-- > 0;) y = f_add(&FR, f_mul(&FR, y, x), p.c[i]);
  /* numerator = p - y (trimmed), q = numerator / (X - x) by long division */
  dpoly num = dp_new(p.n > 0 ? p.n : 1);
  if (p.n > 0) memcpy(num.c, p.c, sizeof(fp) * (size_t)p.n);
  num.c[0] = f_sub(&FR, num.c[0], y);
  dp_trim(&num);
  dpoly q = dp_new(num.n > 1 ? num.n - 1 : 0);
  {
    fp carry = (fp){{0, 0, 0, 0}};
    for (int i = num.n - 1; i >= 1; i--) {
      carry = f_add(&FR, num.c[i], f_mul(&FR, carry, x));
      q.c[i - 1] = carry;
    }
  }
  dp_trim(&q);
  /* assert!(&q * &denominator == numerator) (kzg.rs:85) */
  dpoly den = dp_new(2);
  den.c[0] = f_sub(&FR, (fp){{0, 0, 0, 0}}, x);
  den.c[1] = f_one(&FR);
  dpoly chk = dp_mul(&q, &den);
  int ok = chk.n == num.n;
  for (int i = 0; ok && i < num.n; i++) ok = f_eq(chk.c[i], num.c[i]);
  if (!ok && num.n > 0) abort(); /* the reference panics */
  g1j acc = msm_ark(bases, q.c, (size_t)q.n);
  *pi_out = j_to_affine(&acc);
  *y_out = y;
  dp_free(&p);
  dp_free(&num);
  dp_free(&q);
  dp_free(&den);
  dp_free(&chk);
}
/* the prove over given bases: poly has n coefficients, the point nvars
 * coordinates (Montgomery); outputs evaluation, s_comm, four (y, proof) */
static void mle_open_core(const g1a* bases, const fp* poly, size_t n, const fp* r, int nvars,
                          uint8_t state[32], fp* ev_out, g1a* scomm_out, fp ys[4], g1a pis[4],
                          fp* x_out) {
  const size_t N = (size_t)1 << nvars;
  const size_t M = n > N ? n : N;
  /* compute_pr: evaluations on the domain, IFFT */
  dom d = dom_new((int)N);
  fp* pr = (fp*)malloc(sizeof(fp) * N);
  {
    fp g = f_one(&FR);
    for (size_t k = 0; k < N; k++) {
      pr[k] = eval_pr_c(r, nvars, g);
      g = f_mul(&FR, g, d.g);
    }
    fft_inplace(pr, d.lg, d.gi);
    for (size_t k = 0; k < N; k++) pr[k] = f_mul(&FR, pr[k], d.size_inv);
  }
  fp ev = (fp){{0, 0, 0, 0}};
  for (size_t i = 0; i < (n < N ? n : N); i++) ev = f_add(&FR, ev, f_mul(&FR, poly[i], pr[i]));
  /* compute_s_polynomial with both vectors padded to M */
  dpoly p1 = dp_new((int)M), p2 = dp_new((int)M), p1r = dp_new((int)M), p2r = dp_new((int)M);
  for (size_t i = 0; i < M; i++) {
    const fp a = i < n ? poly[i] : (fp){{0, 0, 0, 0}};
    const fp b = i < N ? pr[i] : (fp){{0, 0, 0, 0}};
    p1.c[i] = a;
    p2.c[i] = b;
    p1r.c[M - 1 - i] = a;
    p2r.c[M - 1 - i] = b;
  }
  dp_trim(&p1);
  dp_trim(&p2);
  dp_trim(&p1r);
  dp_trim(&p2r);
  dpoly a = dp_mul(&p1, &p2r), b = dp_mul(&p1r, &p2);
  dpoly h = dp_add(&a, &b);
  const size_t hl = 2 * M - 1;
  fp* hc = (fp*)calloc(hl, sizeof(fp));
  if (h.n > 0) memcpy(hc, h.c, sizeof(fp) * ((size_t)h.n < hl ? (size_t)h.n : hl));
  dpoly S = dp_new(M > 1 ? (int)(M - 1) : 0);
  if (M > 1) memcpy(S.c, hc + M, sizeof(fp) * (M - 1));
  dp_trim(&S);
  g1j sacc = msm_ark(bases, S.c, (size_t)S.n);
  const g1a scomm = j_to_affine(&sacc);
  /* transcript: point (Vec<Fr>), evaluation, s_comm; draw r (mlpcs.rs:100-107) */
  {
    uint8_t* msg = (uint8_t*)malloc(8 + 32 * (size_t)nvars);
    for (int i = 0; i < 8; i++) msg[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
    for (int i = 0; i < nvars; i++) fr_bytes(r[i], msg + 8 + 32 * i);
    tr_append(state, msg, 8 + 32 * (size_t)nvars);
    free(msg);
    uint8_t b32[32], b64[64];
    fr_bytes(ev, b32);
    tr_append(state, b32, 32);
    g1_ser_c(&scomm, b64);
    tr_append(state, b64, 64);
  }
  const fp x = tr_draw_fr(state), xi = f_inv(&FR, x);
  if (x_out) *x_out = x;
  kzg_open_c(bases, poly, (int)n, x, &ys[0], &pis[0]);
  kzg_open_c(bases, poly, (int)n, xi, &ys[1], &pis[1]);
  kzg_open_c(bases, S.c, S.n, x, &ys[2], &pis[2]);
  kzg_open_c(bases, S.c, S.n, xi, &ys[3], &pis[3]);
  *ev_out = ev;
  *scomm_out = scomm;
  free(pr);
  free(hc);
  dp_free(&p1);
  dp_free(&p2);
  dp_free(&p1r);
  dp_free(&p2r);
  dp_free(&a);
  dp_free(&b);
  dp_free(&h);
  dp_free(&S);
}

static void mle_out(const fp* ev, const g1a* scomm, const fp ys[4], const g1a pis[4],
                    uint64_t out_eval[4], uint64_t out_scomm_xy[8], uint8_t* out_scomm_inf,
                    uint64_t out_y[16], uint64_t out_pi_xy[32], uint8_t out_pi_inf[4]) {
  memcpy(out_eval, ev->v, 32);
  memcpy(out_scomm_xy, scomm->x.v, 32);
  memcpy(out_scomm_xy + 4, scomm->y.v, 32);
  *out_scomm_inf = (uint8_t)scomm->inf;
  for (int k = 0; k < 4; k++) {
    memcpy(out_y + 4 * k, ys[k].v, 32);
    memcpy(out_pi_xy + 8 * k, pis[k].x.v, 32);
    memcpy(out_pi_xy + 8 * k + 4, pis[k].y.v, 32);
    out_pi_inf[k] = (uint8_t)pis[k].inf;
  }
}

int oc_mle_open_ref(int nvars, const uint64_t* poly, const uint64_t* point, const uint64_t tau[4],
                    uint8_t state[32], double* seconds, uint64_t out_eval[4],
                    uint64_t out_scomm_xy[8], uint8_t* out_scomm_inf, uint64_t out_y[16],
                    uint64_t out_pi_xy[32], uint8_t out_pi_inf[4]) {
  const size_t N = (size_t)1 << nvars;
  fp tauf;
  memcpy(tauf.v, tau, 32);
  g1a* bases = (g1a*)malloc(sizeof(g1a) * (N > 1 ? N : 2));
  gen_srs(tauf, N > 1 ? N : 2, bases);
  const double t0 = now_s();
  fp ev, ys[4];
  g1a scomm, pis[4];
  mle_open_core(bases, (const fp*)poly, N, (const fp*)point, nvars, state, &ev, &scomm, ys, pis,
                NULL);
  *seconds = now_s() - t0;
  mle_out(&ev, &scomm, ys, pis, out_eval, out_scomm_xy, out_scomm_inf, out_y, out_pi_xy,
          out_pi_inf);
  free(bases);
  return 0;
}

/* ---------------------------------------------------------------- HyperPlonk building blocks
 * The heavy steps of HyperPlonk::prove (proof.rs:145-301) with the reference's
 * data flow, driven by oracle/hyperplonk_c.py (which keeps the transcript
 * order of the Python restatement).  Field inputs and outputs are CANONICAL
 * little-endian limbs (the driver converts nothing per element); every
 * function converts to Montgomery internally.  One cached SRS ([tau^i] g). */
static g1a* g_srs = NULL;
static size_t g_srs_n = 0;

static fp canon_in(const uint64_t* v) {
  fp x;
  memcpy(x.v, v, 32);
  return f_to_mont(&FR, x);
}
static void canon_out(fp x, uint64_t* v) {
  x = f_from_mont(&FR, x);
  memcpy(v, x.v, 32);
}
static fp* canon_vec(const uint64_t* v, size_t n) {
  fp* r = (fp*)malloc(sizeof(fp) * (n ? n : 1));
  for (size_t i = 0; i < n; i++) r[i] = canon_in(v + 4 * i);
  return r;
}

int oc_srs_set(const uint64_t tau_canon[4], size_t n) {
  free(g_srs);
  g_srs = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
  gen_srs(canon_in(tau_canon), n, g_srs);
  g_srs_n = n;
  return 0;
}

/* KZG::commit = msm_unchecked over the cached SRS (kzg.rs:61-73) */
int oc_commit(const uint64_t* coeffs, size_t n, uint64_t out_xy[8], uint8_t* out_inf) {
  if (n > g_srs_n) return -1;
  fp* c = canon_vec(coeffs, n);
  g1j acc = msm_ark(g_srs, c, n);
  g1a a = j_to_affine(&acc);
  memcpy(out_xy, a.x.v, 32);
  memcpy(out_xy + 4, a.y.v, 32);
  *out_inf = (uint8_t)a.inf;
  free(c);
  return 0;
}

/* MLEvalProof::prove over the cached SRS; outputs canonical field elements
 * and Montgomery G1 coordinates (like oc_mle_open_ref) */
int oc_mle_open(const uint64_t* poly, size_t n, const uint64_t* point, int nvars,
                uint8_t state[32], uint64_t out_eval[4], uint64_t out_scomm_xy[8],
                uint8_t* out_scomm_inf, uint64_t out_y[16], uint64_t out_pi_xy[32],
                uint8_t out_pi_inf[4], uint64_t out_x[4]) {
  const size_t N = (size_t)1 << nvars;
  if ((n > N ? n : N) > g_srs_n) return -1;
  fp* p = canon_vec(poly, n);
  fp* r = canon_vec(point, (size_t)nvars);
  fp ev, ys[4];
  g1a scomm, pis[4];
  fp x;
  mle_open_core(g_srs, p, n, r, nvars, state, &ev, &scomm, ys, pis, &x);
  canon_out(x, out_x);
  mle_out(&ev, &scomm, ys, pis, out_eval, out_scomm_xy, out_scomm_inf, out_y, out_pi_xy,
          out_pi_inf);
  for (int k = 0; k < 4; k++) canon_out(ys[k], out_y + 4 * k);
  canon_out(ev, out_eval);
  free(p);
  free(r);
  return 0;
}

/* postfix programs: (op, arg) pairs, 0 INPUT, 1 CONST, 2 ADD, 3 MUL */
static fp expr_eval_scalar(const uint32_t* prog, int len, const fp* consts, const fp* vals) {
  fp st[64];
  int sp = 0;
  for (int i = 0; i < len; i++) {
    const uint32_t op = prog[2 * i], arg = prog[2 * i + 1];
    if (op == 0) st[sp++] = vals[arg];
    else if (op == 1) st[sp++] = consts[arg];
    else {
      const fp b = st[--sp], a = st[--sp];
      st[sp++] = op == 2 ? f_add(&FR, a, b) : f_mul(&FR, a, b);
    }
  }
  return st[0];
}
/* evaluate_expr_poly (virtual_polynomial.rs:300-320) on the pair's linear polys */
static dpoly expr_eval_poly(const uint32_t* prog, int len, const fp* consts, const dpoly* lin) {
  dpoly st[64];
  int sp = 0;
  for (int i = 0; i < len; i++) {
    const uint32_t op = prog[2 * i], arg = prog[2 * i + 1];
    if (op == 0) {
      st[sp++] = dp_clone(&lin[arg]);
    } else if (op == 1) {
      dpoly c = dp_new(1);
      c.c[0] = consts[arg];
      dp_trim(&c);
      st[sp++] = c;
    } else {
      dpoly b = st[--sp], a = st[--sp];
      st[sp++] = op == 2 ? dp_add(&a, &b) : dp_mul(&a, &b);
      dp_free(&a);
      dp_free(&b);
    }
  }
  return st[0];
}

/* SumcheckProof::prove (sumcheck.rs:28-114), reference-structured, any
 * expression: per pair every table becomes low + X (high - low), the message is
 * the sum of evaluate_expr_poly over the pairs; all tables fold by r.  coeffs:
 * nvars x maxw canonical (trimmed length in lens); point canonical; evaluation. */
int oc_sumcheck_ref_expr(int nvars, int ntab, const uint64_t* tables, const uint32_t* prog,
                         int plen, const uint64_t* consts, int nconsts, const uint64_t claimed[4],
                         uint8_t state[32], int maxw, uint64_t* coeffs, uint32_t* lens,
                         uint64_t* point, uint64_t evaluation[4]) {
  size_t N = (size_t)1 << nvars;
  fp** gs = (fp**)malloc(sizeof(fp*) * (ntab ? ntab : 1));
  for (int i = 0; i < ntab; i++) gs[i] = canon_vec(tables + 4 * N * i, N);
  fp* cs = canon_vec(consts, (size_t)nconsts);
  uint8_t m8[8], b32[32];
  for (int i = 0; i < 8; i++) m8[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
  tr_append(state, m8, 8);
  fr_bytes(canon_in(claimed), b32);
  tr_append(state, b32, 32);
  dpoly* lin = (dpoly*)malloc(sizeof(dpoly) * (ntab ? ntab : 1));
  int rc = 0;
  for (int j = 0; j < nvars; j++) {
    const size_t half = N >> 1;
    dpoly msg = dp_new(0);
    for (size_t p = 0; p < half; p++) {
      for (int i = 0; i < ntab; i++) {
        lin[i] = dp_new(2);
        lin[i].c[0] = gs[i][2 * p];
        lin[i].c[1] = f_sub(&FR, gs[i][2 * p + 1], gs[i][2 * p]);
        dp_trim(&lin[i]);
      }
      dpoly v = expr_eval_poly(prog, plen, cs, lin);
      dpoly nm = dp_add(&msg, &v);
      dp_free(&msg);
      dp_free(&v);
      msg = nm;
      for (int i = 0; i < ntab; i++) dp_free(&lin[i]);
    }
    if (msg.n > maxw) {
      rc = -1;
      dp_free(&msg);
      break;
    }
    /* append_serializable(&poly): u64 length + coefficients */
    uint8_t* buf = (uint8_t*)malloc(8 + 32 * (size_t)msg.n);
    for (int i = 0; i < 8; i++) buf[i] = (uint8_t)((uint64_t)msg.n >> (8 * i));
    for (int i = 0; i < msg.n; i++) fr_bytes(msg.c[i], buf + 8 + 32 * i);
    tr_append(state, buf, 8 + 32 * (size_t)msg.n);
    free(buf);
    lens[j] = (uint32_t)msg.n;
    for (int i = 0; i < maxw; i++)
      canon_out(i < msg.n ? msg.c[i] : (fp){{0, 0, 0, 0}}, coeffs + 4 * ((size_t)j * maxw + i));
    dp_free(&msg);
    const fp r = tr_draw_fr(state);
    canon_out(r, point + 4 * j);
    for (int i = 0; i < ntab; i++)
      for (size_t p = 0; p < half; p++)
        gs[i][p] = f_add(&FR, gs[i][2 * p], f_mul(&FR, r, f_sub(&FR, gs[i][2 * p + 1], gs[i][2 * p])));
    N = half;
  }
  if (rc == 0) {
    fp* vals = (fp*)malloc(sizeof(fp) * (ntab ? ntab : 1));
    for (int i = 0; i < ntab; i++) vals[i] = gs[i][0];
    canon_out(expr_eval_scalar(prog, plen, cs, vals), evaluation);
    free(vals);
  }
  for (int i = 0; i < ntab; i++) free(gs[i]);
  free(gs);
  free(cs);
  free(lin);
  return rc;
}

/* SumcheckProof::prove (sumcheck.rs:28-114) for any expression in evaluation
 * form, single-threaded: the round message has degree < maxw, so it is fixed
 * by its values at t = 0..maxw-1.  Per pair every table is low + t (high - low)
 * (stepped by additions), the postfix program is evaluated at each t, the
 * values are summed over the pairs, interpolated on the nodes 0..maxw-1 and
 * trimmed of trailing zeros as ark's DensePolynomial is.  Inputs and outputs
 * as oc_sumcheck_ref_expr (canonical); with tables_mont != 0 the tables are
 * Montgomery words (arkworks' in-memory Fr) and are taken as they are.
 * -1: maxw outside 1..16. */
int oc_sumcheck_eval_expr(int nvars, int ntab, const uint64_t* tables, const uint32_t* prog,
                          int plen, const uint64_t* consts, int nconsts, const uint64_t claimed[4],
                          uint8_t state[32], int maxw, uint64_t* coeffs, uint32_t* lens,
                          uint64_t* point, uint64_t evaluation[4], int tables_mont) {
  if (maxw < 1 || maxw > 16) return -1;
  size_t N = (size_t)1 << nvars;
  const int nt = ntab ? ntab : 1;
  fp** gs = (fp**)malloc(sizeof(fp*) * nt);
  for (int i = 0; i < ntab; i++) {
    if (tables_mont) {
      gs[i] = (fp*)malloc(sizeof(fp) * N);
      memcpy(gs[i], tables + 4 * N * i, sizeof(fp) * N);
    } else {
      gs[i] = canon_vec(tables + 4 * N * i, N);
    }
  }
  fp* cs = canon_vec(consts, (size_t)nconsts);
  fp* lo = (fp*)malloc(sizeof(fp) * nt);
  fp* df = (fp*)malloc(sizeof(fp) * nt);
  uint8_t m8[8], b32[32];
  for (int i = 0; i < 8; i++) m8[i] = (uint8_t)((uint64_t)nvars >> (8 * i));
  tr_append(state, m8, 8);
  fr_bytes(canon_in(claimed), b32);
  tr_append(state, b32, 32);
  fp V[16][16];
  sc_vandermonde(maxw, V);
  const fp zero = {{0, 0, 0, 0}};
  for (int j = 0; j < nvars; j++) {
    const size_t half = N >> 1;
    fp sums[16];
    for (int t = 0; t < maxw; t++) sums[t] = zero;
    for (size_t p = 0; p < half; p++) {
      for (int i = 0; i < ntab; i++) {
        lo[i] = gs[i][2 * p];
        df[i] = f_sub(&FR, gs[i][2 * p + 1], gs[i][2 * p]);
      }
      for (int t = 0; t < maxw; t++) {
        sums[t] = f_add(&FR, sums[t], expr_eval_scalar(prog, plen, cs, lo));
        for (int i = 0; i < ntab; i++) lo[i] = f_add(&FR, lo[i], df[i]);
      }
    }
    /* coefficients, trimmed length; append_serializable(&poly): u64 length +
     * coefficients; then the challenge */
    fp co[16];
    int len = 0;
    for (int t = 0; t < maxw; t++) {
      fp acc = zero;
      for (int u = 0; u < maxw; u++) acc = f_add(&FR, acc, f_mul(&FR, V[t][u], sums[u]));
      co[t] = acc;
      if (!f_is_zero(acc)) len = t + 1;
    }
    uint8_t buf[8 + 16 * 32];
    for (int i = 0; i < 8; i++) buf[i] = (uint8_t)((uint64_t)len >> (8 * i));
    for (int t = 0; t < len; t++) fr_bytes(co[t], buf + 8 + 32 * t);
    tr_append(state, buf, 8 + 32 * (size_t)len);
    lens[j] = (uint32_t)len;
    for (int t = 0; t < maxw; t++)
      canon_out(t < len ? co[t] : zero, coeffs + 4 * ((size_t)j * maxw + t));
    const fp r = tr_draw_fr(state);
    canon_out(r, point + 4 * j);
    for (int i = 0; i < ntab; i++)
      for (size_t p = 0; p < half; p++)
        gs[i][p] = f_add(&FR, gs[i][2 * p], f_mul(&FR, r, f_sub(&FR, gs[i][2 * p + 1], gs[i][2 * p])));
    N = half;
  }
  for (int i = 0; i < ntab; i++) lo[i] = gs[i][0];
  canon_out(expr_eval_scalar(prog, plen, cs, lo), evaluation);
  for (int i = 0; i < ntab; i++) free(gs[i]);
  free(gs);
  free(cs);
  free(lo);
  free(df);
  return 0;
}

/* logup_column (multiset_check.rs:43-95): out = m(x) / (beta + h(x)); batch
 * inversion; -2 on a zero denominator (the reference's inverse().unwrap()) */
int oc_logup_expr(int ntab, size_t n, const uint64_t* tables, const uint32_t* hprog, int hlen,
                  const uint64_t* hconsts, int hn, const uint32_t* mprog, int mlen,
                  const uint64_t* mconsts, int mn, const uint64_t beta[4], uint64_t* out) {
  fp** gs = (fp**)malloc(sizeof(fp*) * (ntab ? ntab : 1));
  for (int i = 0; i < ntab; i++) gs[i] = canon_vec(tables + 4 * n * i, n);
  fp* hc = canon_vec(hconsts, (size_t)hn);
  fp* mc = canon_vec(mconsts, (size_t)mn);
  const fp b = canon_in(beta);
  fp* den = (fp*)malloc(sizeof(fp) * (n ? n : 1));
  fp* pre = (fp*)malloc(sizeof(fp) * (n ? n : 1));
  fp* vals = (fp*)malloc(sizeof(fp) * (ntab ? ntab : 1));
  fp acc = f_one(&FR);
  int rc = 0;
  for (size_t i = 0; i < n; i++) {
    for (int t = 0; t < ntab; t++) vals[t] = gs[t][i];
    den[i] = f_add(&FR, b, expr_eval_scalar(hprog, hlen, hc, vals));
    if (f_is_zero(den[i])) rc = -2;
    acc = f_mul(&FR, acc, den[i]);
    pre[i] = acc;
  }
  if (rc == 0) {
    fp inv = f_inv(&FR, acc);
    for (size_t i = n; i-- > 0;) {
      fp v = f_mul(&FR, inv, i ? pre[i - 1] : f_one(&FR));
      inv = f_mul(&FR, inv, den[i]);
      if (mprog && mlen) {
        for (int t = 0; t < ntab; t++) vals[t] = gs[t][i];
        v = f_mul(&FR, v, expr_eval_scalar(mprog, mlen, mc, vals));
      }
      canon_out(v, out + 4 * i);
    }
  }
  for (int i = 0; i < ntab; i++) free(gs[i]);
  free(gs);
  free(hc);
  free(mc);
  free(den);
  free(pre);
  free(vals);
  return rc;
}

/* fast_eq_eval_hypercube (eq_eval.rs:6-31), canonical in / out */
int oc_eq_table(const uint64_t* point, int n, uint64_t* out) {
  fp* e = (fp*)malloc(sizeof(fp) << n);
  e[0] = f_one(&FR);
  size_t len = 1;
  for (int i = n - 1; i >= 0; i--) {
    const fp r = canon_in(point + 4 * i), omr = f_sub(&FR, f_one(&FR), r);
    for (size_t k = len; k-- > 0;) {
      const fp v = e[k];
      e[2 * k] = f_mul(&FR, v, omr);
      e[2 * k + 1] = f_mul(&FR, v, r);
    }
    len <<= 1;
  }
  for (size_t k = 0; k < len; k++) canon_out(e[k], out + 4 * k);
  free(e);
  return 0;
}
