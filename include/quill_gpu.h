/*
 * quill_gpu.h — C-ABI of the MI355X (gfx950) prover hot path for Quill.
 *
 * Drop-in boundary for gio54321/quill-zkvm (reference mounted at /root/reference):
 * every entry point below names the reference item it replaces (file:line).
 * A Rust shim binds these with `extern "C"` and keeps the
 * reference's `MultilinearPCS` / `SumcheckProof` / `ZeroCheckProof` surfaces.
 *
 * Conventions
 *  - Field elements (BN254 Fr and Fq) are 4 x uint64 little-endian limbs in
 *    Montgomery form with R = 2^256: exactly arkworks' in-memory
 *    `Fp256(BigInt([u64; 4]))`, so a Rust shim passes `&[Fr]` as a pointer
 *    with no conversion.
 *  - A G1 point is `uint64_t xy[8]` (x limbs then y limbs, Montgomery) plus an
 *    infinity flag (`uint8_t`), i.e. ark-ec `Affine<G1Config>` field order.
 *  - The Fiat-Shamir transcript (transcript/src/transcript.rs:5-74) is carried
 *    as its 32-byte BLAKE3 chaining state `uint8_t state[32]`, updated in place.
 *  - Every function returns an int status: 0 = QG_OK, < 0 = error.  Nothing
 *    unwinds across the ABI; qg_last_error() describes the last failure on a
 *    context.  The reference prover panics where these return
 *    QG_ERR_INVALID / QG_ERR_ASSERT (pcs/src/kzg.rs:62-65,85,
 *    hyperplonk/src/piops/multiset_check.rs:51,63); a Rust shim maps a non-zero
 *    status to `panic!` to keep those semantics.
 *  - Calls are synchronous (they may use internal HIP streams).  A context is
 *    bound to one device; use one context per thread.
 */
#ifndef QUILL_GPU_H
#define QUILL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QG_OK 0
#define QG_ERR_INVALID (-1)     /* bad argument / size (reference: assert! panic) */
#define QG_ERR_DEVICE (-2)      /* HIP runtime error */
#define QG_ERR_OOM (-3)         /* device allocation failed */
#define QG_ERR_UNSUPPORTED (-4) /* expression / size outside the supported envelope */
#define QG_ERR_ASSERT (-5)      /* prover-side sanity check failed (reference: assert!) */
#define QG_ERR_COMM (-6)        /* RCCL failure */

typedef struct qg_ctx qg_ctx;
typedef struct qg_srs qg_srs;
typedef struct qg_buf qg_buf;
struct qg_kzg_vk; /* the verifier's part of the CRS, defined with qg_kzg_verify */

/* ---------------------------------------------------------------- context */
/* Device context (one HIP device, its streams and scratch). */
int qg_ctx_create(int device, qg_ctx** out);
int qg_ctx_destroy(qg_ctx* ctx);
const char* qg_last_error(const qg_ctx* ctx);
/* Library / build identification (e.g. "gfx950"). */
const char* qg_version(void);

/* Multi-GPU: attach an RCCL communicator (one process per GPU).  `unique_id`
 * is the 128-byte ncclUniqueId produced by qg_comm_unique_id() on rank 0 and
 * broadcast by the caller (e.g. torch.distributed).  After this, qg_msm_g1 /
 * qg_kzg_commit on an SRS *shard* return the sum over all ranks, and
 * qg_sumcheck_prove treats its tables as the rank's block of the hypercube
 * (high index bits = rank). */
int qg_comm_unique_id(uint8_t out_id[128]);
/* world == 1 detaches (plain single-GPU paths) unless QG_FORCE_RCCL=1 is set:
 * then a real one-rank RCCL communicator is attached (unique_id may be NULL)
 * and the sharded code paths run through it — a test switch so a 1-GPU box
 * executes the RCCL transport. */
int qg_ctx_attach_comm(qg_ctx* ctx, int rank, int world, const uint8_t unique_id[128]);
/* What the context exchanges through: 0 none (single GPU), 1 the in-process
 * loopback, 2 an RCCL communicator.  `sharded` = 1 when the sharded paths run. */
int qg_ctx_comm_info(const qg_ctx* ctx, int* kind, int* rank, int* world, int* sharded);
/* In-process loopback group: `world` contexts, each driven by its own host
 * thread (possibly on one device), exchange through device-to-device copies
 * instead of RCCL.  Exercises every sharded path on a single GPU. */
typedef struct qg_loopback qg_loopback;
int qg_loopback_create(int world, qg_loopback** out);
int qg_loopback_destroy(qg_loopback* lb);
int qg_ctx_attach_loopback(qg_ctx* ctx, qg_loopback* lb, int rank);
/* Allgather of `bytes` host bytes from every rank into recv (world * bytes, rank
 * order) over the attached communicator: the host-side agreement steps of the
 * sharded prover (constraint-check verdicts, boundary rows). */
int qg_comm_allgather_host(qg_ctx* ctx, const void* send, size_t bytes, void* recv);
/* Personalised exchange of host bytes: send holds world chunks of `bytes` (chunk d
 * goes to rank d), recv receives world chunks (chunk s came from rank s); the
 * collective the sharded S polynomial uses (grouped RCCL send/recv). */
int qg_comm_alltoall_host(qg_ctx* ctx, const void* send, size_t bytes, void* recv);
/* The full witness of a trace, concat(columns) (hyperplonk/src/proof/proof.rs:270),
 * as this rank's block: every rank passes its row block (rows / world entries)
 * of each of the `ncols` columns and receives entries
 * [rank * ncols * rows / world, (rank + 1) * ncols * rows / world) of the
 * column-major flattening (exchanged with one RCCL allgather of the packed
 * row blocks, then a local extraction).
 * world == 1: the plain concatenation. */
int qg_trace_full_witness(qg_ctx* ctx, const qg_buf* const* col_blocks, uint32_t ncols,
                          uint64_t rows, qg_buf* full_block);

/* ---------------------------------------------------------------- transcript */
/* Transcript::new(domain)                  transcript/src/transcript.rs:14-22 */
int qg_transcript_new(const uint8_t* domain, size_t len, uint8_t state[32]);
/* Transcript::append_bytes(msg)            transcript.rs:25-31 */
int qg_transcript_append(uint8_t state[32], const uint8_t* msg, size_t len);
/* Transcript::draw_challenge(n) (n <= 64)  transcript.rs:48-62 */
int qg_transcript_draw(uint8_t state[32], uint8_t* out, size_t n);
/* Transcript::draw_field_element::<Fr>()   transcript.rs:70-74 (out: Montgomery) */
int qg_transcript_draw_fr(uint8_t state[32], uint64_t out_fr[4]);
/* ark-serialize uncompressed encodings used with append_serializable
 * (transcript.rs:33-37): Fr -> 32 B canonical LE; G1 -> 64 B (x||y, SW flags). */
int qg_fr_serialize(const uint64_t fr[4], uint8_t out[32]);
int qg_g1_serialize(const uint64_t xy[8], uint8_t infinity, uint8_t out[64]);

/* ---------------------------------------------------------------- SRS */
/* Upload `n` affine bases (KZG::g1_points, pcs/src/kzg.rs:10-23), x||y Montgomery
 * limbs per point (n x 8 uint64) + per-point infinity flags (may be NULL).
 * The device keeps the bases affine (this removes the per-commit
 * `into_affine` of every SRS point, kzg.rs:67-71) together with the MSM's
 * precomputed window-shifted copies.  The limbs are trusted: nothing is
 * checked.  Points from a file or another party go through qg_srs_import
 * (ark-serialize bytes, every point validated) or are checked afterwards with
 * qg_srs_validate / qg_srs_check_powers. */
int qg_srs_upload(qg_ctx* ctx, const uint64_t* affine_xy, const uint8_t* infinity, size_t n,
                  qg_srs** out);
/* Bases for one-shot MSMs (VariableBaseMSM::msm_unchecked over bases used
 * once, the call at pcs/src/kzg.rs:72 with a base slice that is not a fixed
 * SRS): same layout and MSM results as qg_srs_upload, but only ONE table is
 * built (no window-shifted copies: 1/W of the HBM and none of the W - 1 shift
 * passes, 0.63 s at 2^24).  Every MSM over these bases then bins its W windows
 * in W passes and combines the window sums by Horner steps; use qg_srs_upload
 * for bases that serve many MSMs.  Any qg_* call taking a qg_srs accepts it. */
int qg_bases_upload(qg_ctx* ctx, const uint64_t* affine_xy, const uint8_t* infinity, size_t n,
                    qg_srs** out);
/* KZG::trusted_setup with an explicit tau (kzg.rs:35-59): bases [tau^i] g for
 * i < n, generated on the device.  `g_xy` NULL = the BN254 generator (1, 2). */
int qg_srs_generate(qg_ctx* ctx, const uint64_t tau[4], const uint64_t* g_xy, size_t n,
                    qg_srs** out);
/* Bases [tau^(offset+i)] g for i < n: the shard [offset, offset+n) of a larger
 * SRS (one shard per rank for the multi-GPU MSM). */
int qg_srs_generate_range(qg_ctx* ctx, const uint64_t tau[4], const uint64_t* g_xy,
                          uint64_t offset, size_t n, qg_srs** out);
int qg_srs_destroy(qg_srs* srs);
size_t qg_srs_len(const qg_srs* srs);
/* MSM window geometry of this SRS: signed-digit window bits c and window
 * count W (the tables hold W shifted copies of the bases; one table for
 * qg_bases_upload). */
int qg_srs_window_info(const qg_srs* srs, int* c, int* windows);
/* Copy bases [offset, offset+n) back to the host (affine, Montgomery). */
int qg_srs_download(const qg_srs* srs, size_t offset, size_t n, uint64_t* affine_xy,
                    uint8_t* infinity);

/* ---- SRS as ark-serialize bytes (CanonicalSerialize of G1Affine, no length
 * prefix).  Coordinates are canonical little-endian; two flag bits sit in the
 * top two bits of the LAST byte of a point: bit 7 = y is the larger root
 * (y > p - y), bit 6 = the point at infinity (every other bit zero). */
#define QG_G1_UNCOMPRESSED 0 /* 64 B/point: x || y LE, flags in y's top byte == qg_g1_serialize */
#define QG_G1_COMPRESSED 1   /* 32 B/point: x LE, flags in x's top byte */
#define QG_SRS_ONESHOT 1u    /* one table, as qg_bases_upload */
/* why a point was refused (bad_reason) */
#define QG_SRS_BAD_NONCANONICAL 1u /* coordinate >= p */
#define QG_SRS_BAD_INFINITY 2u     /* infinity flag with nonzero coordinate bits or the sign flag */
#define QG_SRS_BAD_NOT_SQUARE 3u   /* x^3 + 3 is not a square (compressed) */
#define QG_SRS_BAD_NOT_ON_CURVE 4u /* y^2 != x^3 + 3 (uncompressed, and table rows) */
#define QG_SRS_BAD_SIGN_FLAG 5u    /* sign flag inconsistent with y (uncompressed) */
/* `n` points from `bytes` (n * 64 or n * 32 bytes), decoded, decompressed and
 * validated on the device with the rules of CanonicalDeserialize under
 * Validate::Yes (G1 has cofactor 1: on the curve is in the group), then the
 * tables of qg_srs_upload (flags = 0) or qg_bases_upload (QG_SRS_ONESHOT).
 * A bad point: QG_ERR_INVALID, *out = NULL, *bad_index = the LOWEST bad index,
 * *bad_reason = that point's reason (both pointers may be NULL), and
 * qg_last_error says both in words.  On success *bad_reason = 0. */
int qg_srs_import(qg_ctx* ctx, const uint8_t* bytes, size_t n, int format, uint32_t flags,
                  qg_srs** out, uint64_t* bad_index, uint32_t* bad_reason);
/* Bases [offset, offset+n) as bytes of `format` into out (n * 64 or n * 32). */
int qg_srs_export(const qg_srs* srs, size_t offset, size_t n, int format, uint8_t* out);
/* The canonical and on-curve checks over the bases a handle holds, however it
 * was made (qg_srs_upload and qg_bases_upload check nothing).  A bad row:
 * QG_ERR_INVALID with the lowest index and its reason as for qg_srs_import
 * (QG_SRS_BAD_NONCANONICAL, QG_SRS_BAD_NOT_ON_CURVE, or QG_SRS_BAD_INFINITY
 * for an infinity flag over nonzero coordinates). */
int qg_srs_validate(qg_ctx* ctx, const qg_srs* srs, uint64_t* bad_index, uint32_t* bad_reason);
/* Are the bases P_0 .. P_{N-1} the powers [tau^i] g of the verifying key, i.e.
 * P_0 == vk.g1 and P_{i+1} = tau P_i for the tau of vk.g2_tau?  One random
 * linear combination: rho_i = the low 128 bits (LE) of BLAKE3(seed || u64_le(i)),
 * A = sum_{i<N-1} rho_i P_i, B = sum_{1<=j<N} rho_{j-1} P_j (two MSMs over the
 * same bases), and e(A, tau g2) e(-B, g2) == 1 on the host.  *ok = 1 / 0;
 * QG_ERR_INVALID only for bad arguments or a malformed vk.  N == 1 checks P_0.
 * SOUNDNESS: the seed must be unknown to whoever produced the SRS; a wrong SRS
 * then passes with probability about 2^-128.  seed == NULL draws 32 bytes from
 * std::random_device.  A fixed seed is for reproducible tests only.
 * On a sharded context the call is collective: rank r holds the global range
 * [r n, (r+1) n) (n = qg_srs_len, N = world n), the multipliers are indexed
 * globally, rank 0's seed and its P_0 verdict are shared, and every rank
 * returns the same *ok. */
int qg_srs_check_powers(qg_ctx* ctx, const qg_srs* srs, const struct qg_kzg_vk* vk,
                        const uint8_t seed[32], int* ok);

/* ---------------------------------------------------------------- device vectors */
/* Fr vectors resident in HBM (for callers that keep witnesses on the device). */
int qg_buf_create(qg_ctx* ctx, size_t n, qg_buf** out);
int qg_buf_destroy(qg_buf* buf);
size_t qg_buf_len(const qg_buf* buf);
int qg_buf_upload(qg_buf* buf, const uint64_t* fr, size_t n);
int qg_buf_download(const qg_buf* buf, uint64_t* fr, size_t n);
/* Fill with uniform Fr from splitmix64->xoshiro256** keyed by (seed, index
 * block); used for synthetic benchmark witnesses. */
int qg_buf_fill_random(qg_buf* buf, uint64_t seed);
/* Non-owning view of entries [offset, offset+n) of `base` (destroy it with
 * qg_buf_destroy; the base must outlive it).  The HyperPlonk full witness is
 * the concatenation of its columns (hyperplonk/src/proof/proof.rs:270); its
 * columns are views of it, so nothing is copied. */
int qg_buf_view(qg_buf* base, size_t offset, size_t n, qg_buf** out);
/* Upload n Montgomery Fr to entries [offset, offset+n). */
int qg_buf_upload_at(qg_buf* buf, size_t offset, const uint64_t* fr, size_t n);
/* Upload n canonical (non-Montgomery) 4 x u64 LE values < r, converted on the
 * device (QG_ERR_INVALID if some value >= r). */
int qg_buf_upload_canonical(qg_buf* buf, size_t offset, const uint64_t* canon, size_t n);
/* F::from(u64) for n values: the id / permutation index columns of
 * Circuit::permutation (hyperplonk/src/frontend/transition_circuit.rs:120-151). */
int qg_buf_upload_u64(qg_buf* buf, size_t offset, const uint64_t* v, size_t n);
/* Device-to-device copy of n entries. */
int qg_buf_copy(qg_buf* dst, size_t dst_off, const qg_buf* src, size_t src_off, size_t n);
/* First i < n with a[a_off+i] != b[b_off+i], or -1: the copy-constraint check
 * of TransitionCircuit::check_constraints (transition_circuit.rs:186-202). */
int qg_buf_first_mismatch(const qg_buf* a, size_t a_off, const qg_buf* b, size_t b_off, size_t n,
                          int64_t* first);

/* ---------------------------------------------------------------- MSM / KZG */
/* E::G1::msm_unchecked(bases, scalars) (pcs/src/kzg.rs:72): sum of
 * scalars[i] * srs[i] over i < n (n <= qg_srs_len).  Bit-exact: the affine
 * result is the unique group element. */
int qg_msm_g1(qg_ctx* ctx, const qg_srs* srs, const uint64_t* scalars, size_t n,
              uint64_t out_xy[8], uint8_t* out_inf);
int qg_msm_g1_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* scalars, size_t n,
                  uint64_t out_xy[8], uint8_t* out_inf);
/* msm_unchecked over the base slice srs[offset..] (SURVEY 8(b)'s `offset`):
 * sum of scalars[i] * srs[offset + i] over i < min(n, qg_srs_len - offset),
 * truncated like msm_unchecked; QG_ERR_INVALID when offset > qg_srs_len.
 * Host (`_at`) and device-resident (`_dev_at`) scalars. */
int qg_msm_g1_at(qg_ctx* ctx, const qg_srs* srs, size_t offset, const uint64_t* scalars,
                 size_t n, uint64_t out_xy[8], uint8_t* out_inf);
int qg_msm_g1_dev_at(qg_ctx* ctx, const qg_srs* srs, size_t offset, const qg_buf* scalars,
                     size_t n, uint64_t out_xy[8], uint8_t* out_inf);
/* k MSMs over one SRS in one call (at most 1024): out_xy[8 i ..], out_inf[i]
 * for scalars[i] (first ns[i] entries), each equal to qg_msm_g1_dev of it.
 * They run as one MSM batch (bucketing beside the previous MSM's accumulation
 * on two side streams, one set of reduction launches): the commitments a
 * caller needs together, e.g. HyperPlonk's two Logup denominator columns
 * (multiset_check.rs:43-95) or its trace witnesses (proof.rs:252-262). */
int qg_msm_g1_dev_batch(qg_ctx* ctx, const qg_srs* srs, const qg_buf* const* scalars,
                        const size_t* ns, size_t k, uint64_t* out_xy, uint8_t* out_inf);
/* KZG::commit (kzg.rs:61-73): QG_ERR_INVALID when n > max_degree + 1
 * (reference: assert! at kzg.rs:62-65). */
int qg_kzg_commit(qg_ctx* ctx, const qg_srs* srs, const uint64_t* poly, size_t n,
                  uint64_t out_xy[8], uint8_t* out_inf);

/* KZGOpeningProof (kzg.rs:25-32). */
typedef struct qg_kzg_opening {
  uint64_t x[4];
  uint64_t y[4];
  uint64_t proof_xy[8];
  uint8_t proof_inf;
  uint8_t _pad[7];
} qg_kzg_opening;

/* KZG::open (kzg.rs:75-96): y = p(x), q = (p - y)/(X - x), proof = commit(q). */
int qg_kzg_open(qg_ctx* ctx, const qg_srs* srs, const uint64_t* poly, size_t n,
                const uint64_t x[4], qg_kzg_opening* out);

/* ---------------------------------------------------------------- multilinear PCS */
/* MLEvalProof (pcs/src/mlpcs.rs:32-44) without the point (caller owns it). */
typedef struct qg_mle_proof {
  uint64_t evaluation[4];
  uint64_t s_comm_xy[8];
  uint8_t s_comm_inf;
  uint8_t _pad[7];
  qg_kzg_opening poly_opening;
  qg_kzg_opening poly_opening_inv;
  qg_kzg_opening s_opening;
  qg_kzg_opening s_opening_inv;
} qg_mle_proof;

/* MultilinearPCS::open == MLEvalProof::prove (mlpcs.rs:83-124, trait impl
 * :191-198): opens the hypercube evaluations `poly` (len n) at `point`
 * (nvars Fr).  `state` is the transcript, advanced exactly as the reference
 * (append point, evaluation, s_comm; draw r). */
int qg_mle_open(qg_ctx* ctx, const qg_srs* srs, const uint64_t* poly, size_t n,
                const uint64_t* point, size_t nvars, uint8_t state[32], qg_mle_proof* out);
/* Same, on a device-resident evaluation vector (first n entries of `poly`). */
int qg_mle_open_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                    const uint64_t* point, size_t nvars, uint8_t state[32], qg_mle_proof* out);
/* Same, with flags.  QG_OPEN_UNCHANGED: the caller guarantees that the first n
 * entries of `poly` have not changed since an earlier open of this same buffer
 * on this context; the polynomial's NTT transform from that call is then
 * reused when the context still holds it (HyperPlonk opens its full witness
 * once per column, proof.rs:203-224).  The proof is identical either way. */
#define QG_OPEN_UNCHANGED 1u
int qg_mle_open_dev_ex(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                       const uint64_t* point, size_t nvars, uint8_t state[32], uint32_t flags,
                       qg_mle_proof* out);
/* K openings in one call (at most 256), item k exactly as the k-th of K
 * successive qg_mle_open_dev_ex calls on the same transcript: same proofs, same
 * final `state`.  The S polynomial, its commitment and the evaluation depend
 * on (poly, point) only and no quotient commitment enters the transcript
 * (mlpcs.rs:83-124), so the device runs the K S commitments as one MSM batch,
 * the K transcript steps on the host, then all 4K quotient commitments as one
 * MSM batch.  HyperPlonk's openings of one trace (proof.rs:203-224).
 * HBM: the call holds every item's S (M - 1 Fr) and four quotient vectors
 * plus one partial-sum slot set per MSM until it returns (~1 GB per item of
 * 2^20 evaluations, mostly the partial slots); per-item scratch beyond the
 * first 16 items is freed when it returns, the first 16 items' is kept for
 * the next call.  A sharded
 * context (qg_ctx_attach_comm) batches too: all items must then share one SRS
 * shard (the Python mirror batches each run of equal local length). */
typedef struct qg_mle_open_item {
  const qg_buf* poly;     /* device evaluations (first n entries) */
  size_t n;
  const uint64_t* point;  /* nvars Fr */
  size_t nvars;
  uint32_t flags;         /* QG_OPEN_UNCHANGED or 0 */
  uint32_t _pad;
} qg_mle_open_item;
int qg_mle_open_batch_dev(qg_ctx* ctx, const qg_srs* srs, const qg_mle_open_item* items,
                          size_t k, uint8_t state[32], qg_mle_proof* outs);

/* ---- folded ML opening (opt-in; no counterpart in the reference).
 * An MLEvalProof opens two polynomials, f and S, each at r and 1/r.  Two
 * polynomials opened at the same point need one quotient: with gamma drawn
 * after the four values, (h - h(x))/(X - x) for h = f + gamma S is one KZG
 * claim against C_f + gamma s_comm (the same-point batching of GWC / PLONK;
 * needs g2 and tau g2 only).  Per opening 3 MSMs instead of 5, 2 KZG claims
 * instead of 4, 2 quotient vectors instead of 4, and a smaller proof.
 * Prover: as MLEvalProof::prove up to r (append point, evaluation, s_comm;
 * draw r; assert r != 0); y = (f(r), f(1/r), S(r), S(1/r)) over the untrimmed
 * vectors, appended as four Fr in that order; draw gamma (not redrawn when 0);
 * nothing further is absorbed.  h = f + gamma S over L_h = max(trimmed length
 * of f, of S) coefficients; w = commit((h - h(r))/(X - r)), w_inv the same at
 * 1/r, each over L_h - 1 coefficients (L_h = 0: both the identity, all y 0).
 * The proof carries no opening x and no folded y: the verifier derives both. */
typedef struct qg_mle_proof_folded {
  uint64_t evaluation[4];
  uint64_t s_comm_xy[8];
  uint8_t s_comm_inf;
  uint8_t _pad[7];
  uint64_t y[4][4]; /* poly at r, poly at 1/r, S at r, S at 1/r */
  uint64_t w_xy[8];
  uint8_t w_inf;
  uint8_t _pad1[7];
  uint64_t w_inv_xy[8];
  uint8_t w_inv_inf;
  uint8_t _pad2[7];
} qg_mle_proof_folded;
/* The folded form of qg_mle_open_dev_ex (flags: QG_OPEN_UNCHANGED or 0) and of
 * qg_mle_open_batch_dev (k <= 256; item k exactly as the k-th of k successive
 * single calls: same proofs, same final `state`).  The K S commitments are one
 * MSM batch and the 2K quotient commitments another; between them each item
 * costs one host round trip (gamma_k needs item k's four values, item k + 1's
 * r needs gamma_k's transcript state; timed region "fold_eval").  The two
 * quotients of an item come from the plain two-point scan over h in scratch
 * (qg_lincomb_dev's kernel), or with QG_FOLD_FUSED=1 (read per call; 0 or unset:
 * the former) from one scan that forms the coefficients of h on the fly and
 * never writes h; identical proofs, and the former measured faster (DESIGN
 * section 5).  Both are checked like every opening's
 * ("open_checks" rises by 2 per opening): at the context's sigma,
 * f(sigma) + gamma S(sigma) - (y_f + gamma y_S) == q(sigma)(sigma - x), and the
 * scan's own h(x) equals y_f + gamma y_S; a failure is QG_ERR_ASSERT
 * "Polynomial division failed: opening i of K, quotient j (folded at r)" or
 * "(folded at 1/r)".  QG_ERR_INVALID: null handles, a length beyond the
 * buffer, nvars > 30, unknown flags, L_h - 1 beyond the SRS ("Polynomial degree
 * exceeds max degree").  QG_ERR_UNSUPPORTED: a context with a communicator
 * attached ("sharded" in qg_last_error), before any device work or collective. */
int qg_mle_open_folded_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* poly, size_t n,
                           const uint64_t* point, size_t nvars, uint8_t state[32], uint32_t flags,
                           qg_mle_proof_folded* out);
int qg_mle_open_folded_batch_dev(qg_ctx* ctx, const qg_srs* srs, const qg_mle_open_item* items,
                                 size_t k, uint8_t state[32], qg_mle_proof_folded* outs);
/* The building block, for tests and for callers that batch their own
 * protocol: KZG::open of sum_j coeffs[j] polys[j] (the first lens[j] entries
 * of polys[j]; a shorter one counts as zero-padded; coeffs: P Fr on the host)
 * at the nx points xs, through the folded opening's scan (QG_FOLD_FUSED as
 * above) and with the quotient check;
 * outs[i] = (xs[i], value, proof), the same bits as qg_kzg_open of the
 * materialised combination.  Limits: 1 <= P <= 4, nx 1 or 2; anything else,
 * null pointers and a length beyond its buffer included, is QG_ERR_INVALID.
 * QG_ERR_UNSUPPORTED on a context with a communicator attached. */
int qg_kzg_open_lincomb_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* const* polys,
                            const size_t* lens, const uint64_t* coeffs, size_t P,
                            const uint64_t* xs, size_t nx, qg_kzg_opening* outs);

/* ---------------------------------------------------------------- inner-product argument */
/* InnerProductProof (pcs/src/ipa.rs:40-53), fields in the reference's order. */
typedef struct qg_ipa_proof {
  uint64_t inner_product[4];
  uint64_t s_comm_xy[8];
  uint8_t s_comm_inf;
  uint8_t _pad[7];
  qg_kzg_opening f_opening;
  qg_kzg_opening f_opening_inv;
  qg_kzg_opening g_opening;
  qg_kzg_opening g_opening_inv;
  qg_kzg_opening s_opening;
  qg_kzg_opening s_opening_inv;
} qg_ipa_proof;

/* InnerProductProof::prove (ipa.rs:59-112) for the coefficient vectors f (nf)
 * and g (ng): inner_product = sum_i f[i] g[i] over min(nf, ng); S is the
 * polynomial of the zero-padded pair (ipa.rs:122-157), trimmed before its
 * commitment and its openings; the transcript appends inner_product, then
 * s_comm, and draws r; the six KZG::open of f, g and S at r and 1/r come from
 * the trimmed polynomials, each quotient checked like every opening's
 * ("open_checks"); last the assertion of ipa.rs:94-100 on the six y.
 * Like the reference, the commitments to f and g are the caller's to absorb
 * into the transcript beforehand.
 * QG_ERR_INVALID: nf == 0 && ng == 0 (the reference underflows 2 max_len - 1),
 * a null handle or pointer, a length beyond the buffer, a quotient or S longer
 * than the SRS ("Polynomial degree exceeds max degree").  QG_ERR_ASSERT: r == 0,
 * a failed quotient check ("Polynomial division failed", naming which of
 * "f at r", "f at 1/r", "g at r", "g at 1/r", "S at r", "S at 1/r"), or
 * "Inner product verification equation failed".  QG_ERR_UNSUPPORTED: this
 * host-pointer entry on a context with a communicator attached ("sharded" in
 * qg_last_error, returned before any collective): a sharded caller holds device
 * blocks and calls qg_ipa_prove_dev, as for qg_lookup_multiplicities.
 * The call transforms f in the scratch the ML opening keeps its transform in:
 * a QG_OPEN_UNCHANGED opening after it recomputes its transform.
 * QG_IPA_PAIRED=1 (read per call) runs the six quotients as three paired
 * suffix-Horner jobs (one pass over each polynomial for r and 1/r) instead of
 * six single ones; the proof is identical. */
int qg_ipa_prove(qg_ctx* ctx, const qg_srs* srs, const uint64_t* f, size_t nf, const uint64_t* g,
                 size_t ng, uint8_t state[32], qg_ipa_proof* out);
/* Same, on device-resident vectors (the first nf / ng entries).
 * With a communicator attached, rank c of W passes its blocks f[cL, (c+1)L) and
 * g[cL, (c+1)L) of the two global coefficient vectors (nf == ng == L) and the
 * SRS shard at offset cL, as qg_mle_open_dev takes it.  W L must be a power of
 * two (at most 2^27) and W a power of two <= 64; a shorter operand is
 * zero-padded by the caller, and zero tails are trimmed globally, as
 * DensePolynomial trims them.  The proof and the final transcript state on every
 * rank equal what the single-context call returns for the concatenated vectors,
 * bit for bit (zero-padding changes neither the inner product nor the trimmed
 * polynomials; it only appends zero coefficients to S).  Any other local
 * geometry is QG_ERR_UNSUPPORTED ("sharded inner-product argument needs nf ==
 * ng == L with world * L a power of two ..."), decided from the rank's own
 * arguments before the first collective, so a rank that fails it leaves no peer
 * waiting; so are nf == 0 && ng == 0, null handles and a length beyond the
 * buffer (QG_ERR_INVALID).  "Polynomial degree exceeds max degree" is judged
 * against every rank's shard (the shard sizes travel with the local lengths) and
 * returned by all ranks together, like r == 0, a failed quotient check and the
 * final equation.  Ranks that pass different L cannot be detected by any rank:
 * a caller error, and the call may then hang or return a wrong proof.
 * QG_S_PRESUM_FUSED=0 (read per call and per rank) runs the S
 * polynomial's pre-sums as one launch per operand and residue instead of the
 * fused one; the proof is identical. */
int qg_ipa_prove_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* f, size_t nf, const qg_buf* g,
                     size_t ng, uint8_t state[32], qg_ipa_proof* out);

/* ---- folded inner-product argument (opt-in; no counterpart in the reference).
 * InnerProductProof::prove opens three polynomials, f, g and S, each at r and
 * 1/r (the TODO at ipa.rs:86).  Three polynomials opened at the same point need
 * one quotient: with gamma drawn after the six values, (h - h(x))/(X - x) for
 * h = f + gamma g + gamma^2 S is one KZG claim against
 * C_f + gamma C_g + gamma^2 s_comm (the folded ML opening's batching with three
 * sources).  Per proof 3 MSMs instead of 7, 2 KZG claims instead of 6, 2
 * quotient vectors instead of 6, and a smaller proof.
 * Prover: as InnerProductProof::prove up to r (inner_product over the common
 * prefix, S of the zero-padded pair, s_comm over the trimmed S; append
 * inner_product, s_comm; draw r; r = 0 is QG_ERR_ASSERT);
 * y = (f(r), f(1/r), g(r), g(1/r), S(r), S(1/r)) over the untrimmed vectors,
 * appended as six Fr in that order; draw gamma (not redrawn when 0); nothing
 * further is absorbed.  h over L_h = max(trimmed lengths of f, g, S)
 * coefficients, a missing coefficient counting as 0; w = commit((h - h(r))/
 * (X - r)), w_inv the same at 1/r, each over L_h - 1 coefficients (L_h = 0:
 * both the identity, all y 0).  The proof carries no opening x and no folded
 * y: the verifier derives both. */
typedef struct qg_ipa_proof_folded {
  uint64_t inner_product[4];
  uint64_t s_comm_xy[8];
  uint8_t s_comm_inf;
  uint8_t _pad[7];
  uint64_t y[6][4]; /* f at r, f at 1/r, g at r, g at 1/r, S at r, S at 1/r */
  uint64_t w_xy[8];
  uint8_t w_inf;
  uint8_t _pad1[7];
  uint64_t w_inv_xy[8];
  uint8_t w_inv_inf;
  uint8_t _pad2[7];
} qg_ipa_proof_folded;
/* The folded form of qg_ipa_prove_dev on a single context.  The first half is
 * qg_ipa_prove_dev's (same launches).  Then the six values by the evaluation
 * kernel (timed region "fold_eval": one two-point pass over f, g and S, as
 * qg_poly_eval2_dev, or with QG_EVAL_PAIRED=0 - read per call; 1 or unset:
 * the former - two one-point passes of the same kernel, as qg_poly_eval_dev;
 * identical proofs, and the former measured faster), one host round
 * trip (gamma needs the six values), the assertion of ipa.rs:94-100 on them
 * ("Inner product verification equation failed", QG_ERR_ASSERT), one folded
 * scan over three sources (QG_FOLD_FUSED as for qg_mle_open_folded_dev) and one
 * MSM batch of the two quotients.  Both quotients are checked like every
 * opening's ("open_checks" rises by 2 per proof): at the context's sigma,
 * sum_q gamma^q p_q(sigma) - sum_q gamma^q y_q == q(sigma)(sigma - x), and the
 * scan's own h(x) equals sum_q gamma^q y_q; a failure is QG_ERR_ASSERT
 * "Polynomial division failed: opening 0 of 1, quotient j (folded at r)" or
 * "(folded at 1/r)".  QG_OPEN_CHECK=0 and qg_debug_open_fault act as on the
 * other opening paths.
 * QG_ERR_INVALID: the argument checks of qg_ipa_prove_dev (null handles, a
 * length beyond the buffer, nf == 0 && ng == 0), S or L_h - 1 beyond the SRS
 * ("Polynomial degree exceeds max degree").  QG_ERR_UNSUPPORTED: a context with
 * a communicator attached ("sharded" in qg_last_error), before any device work
 * or collective.  Like qg_ipa_prove, the call transforms f in the scratch the
 * ML opening keeps its transform in. */
int qg_ipa_prove_folded_dev(qg_ctx* ctx, const qg_srs* srs, const qg_buf* f, size_t nf,
                            const qg_buf* g, size_t ng, uint8_t state[32],
                            qg_ipa_proof_folded* out);
/* Same for host vectors: uploads, then the same path (argument checks of
 * qg_ipa_prove). */
int qg_ipa_prove_folded(qg_ctx* ctx, const qg_srs* srs, const uint64_t* f, size_t nf,
                        const uint64_t* g, size_t ng, uint8_t state[32],
                        qg_ipa_proof_folded* out);

/* ---------------------------------------------------------------- verifiers (host) */
/* BN254 G2 affine points on the D-type twist E'/Fq2 (y^2 = x^3 + 3/(9 + u)):
 * x.c0, x.c1, y.c0, y.c1, each 4 u64 Montgomery limbs (like G1's Fq). */
/* the standard generator (ark-bn254's G2Affine::generator()) */
int qg_g2_generator(uint64_t out_xy[16]);
/* k * Q (k: Fr, Montgomery limbs) — builds g2_points[1] = tau g2 of
 * KZG::trusted_setup (kzg.rs:52-53).  QG_ERR_INVALID off the curve or
 * outside the prime-order subgroup ([r] Q != O; ark's Validate::Yes). */
int qg_g2_mul(const uint64_t xy[16], uint8_t inf, const uint64_t k[4], uint64_t out_xy[16],
              uint8_t* out_inf);
/* The reduced optimal-ate pairing used by E::pairing (called at
 * kzg.rs:104-105): f_{6x+2,Q}(P) with Frobenius lines, raised to
 * (p^12 - 1) / r, in Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9 + u));
 * out = c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each (re, im), Montgomery.
 * Guaranteed: bilinear, non-degenerate, of order r, so every GT equality
 * (KZG / ML-PCS verification equations) holds exactly when it does with
 * ark-bn254.  NOT guaranteed: the raw GT value equals ark-bn254's
 * `E::pairing(P, Q).0` — ark's hard-part addition chain may return a fixed
 * power of this value (parity of raw values with ark is unpinned; compare
 * GT elements only with each other).  G2 inputs must be on the twist and in
 * the prime-order subgroup (QG_ERR_INVALID otherwise). */
int qg_pairing(const uint64_t p_xy[8], uint8_t p_inf, const uint64_t q_xy[16], uint8_t q_inf,
               uint64_t out[48]);
/* The verifier's view of KZG (kzg.rs:10-23): g1, g2 = g2_points[0],
 * g2_tau = g2_points[1]. */
typedef struct qg_kzg_vk {
  uint64_t g1_xy[8];
  uint64_t g2_xy[16];
  uint64_t g2_tau_xy[16];
} qg_kzg_vk;
/* KZG::verify (kzg.rs:98-108): *ok = e(C - y g1, g2) == e(proof, g2_tau - x g2). */
int qg_kzg_verify(const qg_kzg_vk* vk, const uint64_t comm_xy[8], uint8_t comm_inf,
                  const qg_kzg_opening* opening, int* ok);
/* MLEvalProof::verify (mlpcs.rs:126-161): replays the transcript (append
 * point, evaluation, s_comm; draw r), verifies the four openings and the
 * inner-product equation at r.  `state` advances exactly as the prover's. */
int qg_mle_verify(const qg_kzg_vk* vk, const uint64_t comm_xy[8], uint8_t comm_inf,
                  const uint64_t* point, size_t nvars, const qg_mle_proof* proof,
                  uint8_t state[32], int* ok);
/* InnerProductProof::verify (ipa.rs:160-202) against the commitments to f
 * (comm1) and g (comm2): the six KZG checks first; if one fails, *ok = 0 and
 * `state` is left untouched (the reference returns before it appends).
 * Otherwise appends inner_product and s_comm, draws r and checks the equation
 * at r; `state` then advances exactly as the prover's.  Like the reference,
 * the openings' own x are not compared with r. */
int qg_ipa_verify(const qg_kzg_vk* vk, const uint64_t comm1_xy[8], uint8_t comm1_inf,
                  const uint64_t comm2_xy[8], uint8_t comm2_inf, const qg_ipa_proof* proof,
                  uint8_t state[32], int* ok);

/* ---- batched KZG verification: one pairing check for any number of openings.
 * A claim is one KZG::verify call's input: a commitment and its opening. */
typedef struct qg_kzg_claim {
  uint64_t comm_xy[8];
  uint8_t comm_inf;
  uint8_t _pad[7];
  qg_kzg_opening opening;
} qg_kzg_claim;
/* All n claims under one key hold exactly when, for weights rho_i,
 *     L = sum_i rho_i (C_i - y_i g1 + x_i pi_i),    R = sum_i rho_i pi_i,
 *     e(L, g2) e(-R, tau g2) == 1
 * (two Miller loops and one final exponentiation for the whole set), except
 * that a set with a false claim passes with probability about 2^-128 over the
 * weights.  The weights are Fiat-Shamir, so anyone can restate them: a fresh
 * transcript qg_transcript_new("quill_kzg_batch") - not the proof's - absorbs,
 * each as one qg_transcript_append, n as 8 bytes little-endian, then per claim
 * C (the 64 bytes of qg_g1_serialize), x, y (32 bytes each, qg_fr_serialize)
 * and pi (64 bytes), then the 32 `seed` bytes when seed != NULL (a verifier's
 * own randomness; NULL leaves the weights a function of the claims alone).
 * Then n - 1 field elements are drawn (qg_transcript_draw_fr): rho_0 = 1 and
 * rho_i = the i-th drawn element's canonical value mod 2^128, i >= 1.
 * As an MSM: scalars rho_i on C_i, rho_i x_i mod r on pi_i and
 * -sum_i rho_i y_i on g1 give L; rho_i on pi_i give R.
 * Every point is checked to be on the curve (QG_ERR_INVALID otherwise, as
 * qg_kzg_verify); infinity is a legal C and pi (the zero polynomial's).
 * qg_kzg_batch_fold returns L and R from the host fold, _dev from the device
 * fold (below); both are the same group elements. */
int qg_kzg_batch_fold(const qg_kzg_vk* vk, const qg_kzg_claim* claims, size_t n,
                      const uint8_t seed[32], uint64_t l_xy[8], uint8_t* l_inf, uint64_t r_xy[8],
                      uint8_t* r_inf);
int qg_kzg_batch_fold_dev(qg_ctx* ctx, const qg_kzg_vk* vk, const qg_kzg_claim* claims, size_t n,
                          const uint8_t seed[32], uint64_t l_xy[8], uint8_t* l_inf,
                          uint64_t r_xy[8], uint8_t* r_inf);
/* *ok = 1 when the folded check holds (n == 0: always).  Otherwise *ok = 0 and
 * the claims are checked one by one from index 0 like qg_kzg_verify;
 * *first_bad (nullable) receives the first that fails - a failing fold implies
 * one does, and only a rejection pays for the scan.  *first_bad is untouched
 * on acceptance.  The host entry folds with one double-and-add per point. */
int qg_kzg_verify_batch(const qg_kzg_vk* vk, const qg_kzg_claim* claims, size_t n,
                        const uint8_t seed[32], int* ok, size_t* first_bad);
/* Same, with the fold on the device: [C_0 .. C_{n-1}, pi_0 .. pi_{n-1}, g1] is
 * uploaded once as one-shot bases (qg_bases_upload), L is the MSM over all
 * 2n + 1 of them (qg_msm_g1) and R the MSM over the slice [n, 2n)
 * (qg_msm_g1_at); the two Miller loops stay on the host.  Claims are host
 * data: on a context with a communicator attached the call returns
 * QG_ERR_UNSUPPORTED ("sharded" in qg_last_error) before any device work. */
int qg_kzg_verify_batch_dev(qg_ctx* ctx, const qg_kzg_vk* vk, const qg_kzg_claim* claims,
                            size_t n, const uint8_t seed[32], int* ok, size_t* first_bad);
/* qg_mle_verify without its four pairing checks: the same transcript replay
 * and final `state`, the r = 0 assertion and the inner-product equation
 * (mlpcs.rs:155-160), which *ok reports; out receives the four (commitment,
 * opening) pairs in the reference's order (poly, poly_inv, s, s_inv), each
 * proof point checked to be on the curve.  The proof verifies when *ok = 1 and
 * a batch holding the four claims does. */
int qg_mle_verify_defer(const qg_kzg_vk* vk, const uint64_t comm_xy[8], uint8_t comm_inf,
                        const uint64_t* point, size_t nvars, const qg_mle_proof* proof,
                        uint8_t state[32], qg_kzg_claim out[4], int* ok);
/* qg_ipa_verify without its six pairing checks (ipa.rs:179-188): out receives
 * f, f_inv (comm1), g, g_inv (comm2), s, s_inv (s_comm).  One difference from
 * the sequential call: `state` ALWAYS advances (inner_product, s_comm, draw r),
 * where qg_ipa_verify returns before touching it when an opening fails. */
int qg_ipa_verify_defer(const qg_kzg_vk* vk, const uint64_t comm1_xy[8], uint8_t comm1_inf,
                        const uint64_t comm2_xy[8], uint8_t comm2_inf, const qg_ipa_proof* proof,
                        uint8_t state[32], qg_kzg_claim out[6], int* ok);
/* The folded opening's verifier (host, no context): replays the transcript as
 * qg_mle_verify does (point, evaluation, s_comm; draw r; r = 0 is
 * QG_ERR_ASSERT), appends the proof's four y, draws gamma, checks the
 * inner-product equation (mlpcs.rs:155-160) on the four y, forms
 * C_h = comm + gamma s_comm (qg_g1_lincomb's host code) and checks the two KZG
 * claims (C_h, r, y[0] + gamma y[2], w) and (C_h, 1/r, y[1] + gamma y[3], w_inv).
 * Every proof point must be on the curve (QG_ERR_INVALID).  `state` ends as the
 * prover's.  The _defer form skips the two pairing checks and hands the two
 * claims out for qg_kzg_verify_batch; *ok then reports the equation, and
 * `state` always advances. */
int qg_mle_verify_folded(const qg_kzg_vk* vk, const uint64_t comm_xy[8], uint8_t comm_inf,
                         const uint64_t* point, size_t nvars, const qg_mle_proof_folded* proof,
                         uint8_t state[32], int* ok);
int qg_mle_verify_folded_defer(const qg_kzg_vk* vk, const uint64_t comm_xy[8], uint8_t comm_inf,
                               const uint64_t* point, size_t nvars,
                               const qg_mle_proof_folded* proof, uint8_t state[32],
                               qg_kzg_claim out[2], int* ok);
/* The folded inner-product argument's verifier (host, no context) against the
 * commitments to f (comm1) and g (comm2).  gamma comes from the replay, so the
 * KZG checks cannot run first as in qg_ipa_verify: BOTH forms replay first -
 * inner_product, s_comm; draw r (r = 0 is QG_ERR_ASSERT, as in qg_ipa_verify);
 * the proof's six y; draw gamma - and `state` ALWAYS advances to the prover's
 * final state, whatever the verdict (qg_ipa_verify leaves it untouched when an
 * opening fails).  Then C_h = comm1 + gamma comm2 + gamma^2 s_comm
 * (qg_g1_lincomb's host code), the two KZG claims (C_h, r, y[0] + gamma y[2] +
 * gamma^2 y[4], w) and (C_h, 1/r, y[1] + gamma y[3] + gamma^2 y[5], w_inv), and
 * the equation of ipa.rs:198-201 on the six y.  *ok = 0 when either claim or
 * the equation fails.  Every point must be on the curve (QG_ERR_INVALID).  The
 * _defer form skips the two pairing checks and hands the two claims out for
 * qg_kzg_verify_batch; *ok then reports the equation alone. */
int qg_ipa_verify_folded(const qg_kzg_vk* vk, const uint64_t comm1_xy[8], uint8_t comm1_inf,
                         const uint64_t comm2_xy[8], uint8_t comm2_inf,
                         const qg_ipa_proof_folded* proof, uint8_t state[32], int* ok);
int qg_ipa_verify_folded_defer(const qg_kzg_vk* vk, const uint64_t comm1_xy[8],
                               uint8_t comm1_inf, const uint64_t comm2_xy[8], uint8_t comm2_inf,
                               const qg_ipa_proof_folded* proof, uint8_t state[32],
                               qg_kzg_claim out[2], int* ok);

/* Building blocks of the opening, exposed for testing and for callers that
 * batch their own protocol:
 *  compute_pr (mlpcs.rs:68-78) == eq(bin(i), point) table, untrimmed (2^nvars) */
int qg_eq_table(qg_ctx* ctx, const uint64_t* point, size_t nvars, uint64_t* out);
/*  fast_eq_eval_hypercube (hyperplonk/src/utils/eq_eval.rs:6-31) into a device
 *  vector (first 2^nvars entries of `out`).  With a communicator attached:
 *  this rank's block, the 2^(nvars - log2 world) entries whose high index bits
 *  equal the rank. */
int qg_eq_table_dev(qg_ctx* ctx, const uint64_t* point, size_t nvars, qg_buf* out);
/*  InnerProductProof::compute_s_polynomial (pcs/src/ipa.rs:122-157), untrimmed:
 *  out has max(nf, ng) - 1 entries (caller trims trailing zeros). */
int qg_s_polynomial(qg_ctx* ctx, const uint64_t* f, size_t nf, const uint64_t* g, size_t ng,
                    uint64_t* out);
/*  sum_i f[i] g[i] over min(nf, ng)  (mlpcs.rs:91-94, ipa.rs:66-69) */
int qg_inner_product(qg_ctx* ctx, const uint64_t* f, size_t nf, const uint64_t* g, size_t ng,
                     uint64_t out[4]);
/*  The streaming pieces of the multi-point batch opening (HyperPlonk paper,
 *  section 3.8; no counterpart in the reference, composed in
 *  quill_amd/multiopen.py).  Index bit j of a table corresponds to point[j];
 *  results are canonical residues.  Limits: 1 <= k <= 256, 1 <= P <= 16,
 *  1 <= nvars, 2^nvars entries fit the buffers; anything else, null pointers
 *  included, is QG_ERR_INVALID.  With a communicator attached the three device
 *  entries return QG_ERR_UNSUPPORTED (single-context only so far; the sharded
 *  form is the follow-up of DESIGN section 8).
 *
 *  out[x] = sum_{i<k} weights[i] eq(bin(x), points[i]) for x < 2^nvars.
 *  points: k x nvars Fr, weights: k Fr (host).  No eq table is materialised:
 *  per point a low and a high half-table, k products per output entry. */
int qg_eq_multi_dev(qg_ctx* ctx, const uint64_t* points, const uint64_t* weights, size_t k,
                    size_t nvars, qg_buf* out);
/*  out[i] = sum_x poly[x] eq(bin(x), points[i]) for k points (k Fr on the
 *  host), in one pass over the first n = 2^nvars entries of poly. */
int qg_mle_eval_multi_dev(qg_ctx* ctx, const qg_buf* poly, size_t n, const uint64_t* points,
                          size_t k, size_t nvars, uint64_t* out);
/*  out[x] = sum_{j<P} coeffs[j] bufs[j][x] for x < n (coeffs: P Fr on the
 *  host).  out must not overlap an input: QG_ERR_INVALID. */
int qg_lincomb_dev(qg_ctx* ctx, const qg_buf* const* bufs, const uint64_t* coeffs, size_t P,
                   size_t n, qg_buf* out);
/*  sum_i scalars[i] points[i] over n <= 65536 G1 points, on the host (no
 *  context): how a verifier forms the combined commitment of a batch opening.
 *  Identity inputs (infs[i] != 0) and an identity result are valid; a point
 *  off the curve is QG_ERR_INVALID. */
int qg_g1_lincomb(const uint64_t* points_xy, const uint8_t* infs, const uint64_t* scalars, size_t n,
                  uint64_t out_xy[8], uint8_t* out_inf);

/* ---------------------------------------------------------------- sumcheck */
/* Virtual-polynomial expression (hyperplonk/src/utils/virtual_polynomial.rs:9-18)
 * in postfix form: INPUT(i) pushes table i, CONST(c) pushes consts[c],
 * ADD / MUL pop two and push the result.  Sub is ADD(a, MUL(CONST(-1), b)) as
 * in the reference (:67-77). */
#define QG_OP_INPUT 0
#define QG_OP_CONST 1
#define QG_OP_ADD 2
#define QG_OP_MUL 3
typedef struct qg_expr_op {
  uint32_t op;
  uint32_t arg;
} qg_expr_op;

/* SumcheckProof::prove (hyperplonk/src/piops/sumcheck.rs:28-114) for
 * h(g_0..g_{k-1}) = program.  tables[i] = 2^nvars Fr evaluations of g_i
 * (host pointers).  With an attached communicator (qg_ctx_attach_comm),
 * `nvars` is the GLOBAL variable count and each rank passes its block of
 * 2^(nvars - log2(world)) entries per table (high index bits = rank); every
 * rank returns the same proof.  Absorbs num_vars and claimed_sum, then per round the
 * trimmed coefficient-form message; binds index bit 0 first.
 * Outputs (caller-allocated):
 *   round_coeffs : nvars * (max_degree+1) * 4 uint64, row j = message j
 *                  coefficients (trailing zeros trimmed, rest zero-filled)
 *   round_lens   : nvars uint32, trimmed length of each message
 *   point        : nvars Fr (the EvaluationClaim point)
 *   evaluation   : h at the point (EvaluationClaim::evaluation)
 * `max_degree` = the expression's syntactic degree (qg_expr_degree). */
int qg_expr_degree(const qg_expr_op* prog, size_t prog_len, uint32_t* out_degree);
int qg_sumcheck_prove(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                      const uint64_t* const* tables, const qg_expr_op* prog, size_t prog_len,
                      const uint64_t* consts, size_t nconsts, const uint64_t claimed_sum[4],
                      uint8_t state[32], uint64_t* round_coeffs, uint32_t* round_lens,
                      uint64_t* point, uint64_t evaluation[4]);
/* Same with device-resident tables (the caller's buffers are not modified). */
int qg_sumcheck_prove_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                          const qg_buf* const* tables, const qg_expr_op* prog, size_t prog_len,
                          const uint64_t* consts, size_t nconsts, const uint64_t claimed_sum[4],
                          uint8_t state[32], uint64_t* round_coeffs, uint32_t* round_lens,
                          uint64_t* point, uint64_t evaluation[4]);
/* The caller's transcript stays authoritative (the callback
 * form of SumcheckProof::prove, sumcheck.rs:28-114, whose `transcript:
 * &mut Transcript` is any implementation).  Per round j the library computes
 * the trimmed coefficient-form message and calls
 *   challenge(user, coeffs, len, out_r)
 * with `len` coefficients (len x 4 uint64, arkworks' in-memory Montgomery
 * limbs; len = 0 for an all-zero message); the callback appends the message
 * to its transcript (append_serializable of the DensePolynomial,
 * sumcheck.rs:80), draws r_j (draw_field_element, :82) and writes it to out_r
 * (Montgomery limbs); a nonzero return aborts the prove (QG_ERR_INVALID).
 * The caller appends num_vars and claimed_sum itself before the call
 * (sumcheck.rs:35-36); `claimed_sum` is not absorbed here.  Device tables,
 * any expression (the interpreted path; one host round trip per round), and
 * on a sharded context every rank calls its own callback (the ranks' replicas
 * must return the same r_j).  Outputs as qg_sumcheck_prove. */
typedef int (*qg_challenge_fn)(void* user, const uint64_t* coeffs, uint32_t len, uint64_t out_r[4]);
int qg_sumcheck_prove_cb(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                         const qg_buf* const* tables, const qg_expr_op* prog, size_t prog_len,
                         const uint64_t* consts, size_t nconsts, qg_challenge_fn challenge,
                         void* user, uint64_t* round_coeffs, uint32_t* round_lens,
                         uint64_t* point, uint64_t evaluation[4]);

/* ZeroCheckProof::prove (hyperplonk/src/piops/zerocheck.rs:14-49): draws
 * z (nvars challenges), builds eq(., z) on the device (eq_eval.rs:6-31),
 * runs the sumcheck of h * eq with claimed sum 0 and returns the zero-check
 * claim evaluation = sumcheck claim / eq(z, point).  If `eq_out` is not NULL
 * it receives the eq table (2^nvars Fr) so the caller can mirror the store
 * mutation of zerocheck.rs:27-29.  Outputs as qg_sumcheck_prove, with
 * round messages of degree max_degree(h) + 1. */
int qg_zerocheck_prove(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                       const uint64_t* const* tables, const qg_expr_op* prog, size_t prog_len,
                       const uint64_t* consts, size_t nconsts, uint8_t state[32],
                       uint64_t* round_coeffs, uint32_t* round_lens, uint64_t* point,
                       uint64_t evaluation[4], uint64_t* eq_out);
int qg_zerocheck_prove_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                           const qg_buf* const* tables, const qg_expr_op* prog, size_t prog_len,
                           const uint64_t* consts, size_t nconsts, uint8_t state[32],
                           uint64_t* round_coeffs, uint32_t* round_lens, uint64_t* point,
                           uint64_t evaluation[4]);

/* ---------------------------------------------------------------- Logup */
/* Log-derivative column of the Logup PIOPs: the per-row loops of
 * MultisetEqualityProof::prove (hyperplonk/src/piops/multiset_check.rs:43-95)
 * and SetInclusionProof::prove (hyperplonk/src/piops/set_inclusion.rs:93-131):
 *     out[x] = m(x) / (beta + h(x))        for every row x of the hypercube,
 * h and m given as postfix expressions over `tables` (same encoding as the
 * sumcheck above; m = 1 when m_prog is NULL, LookupMode::Equality).  Rows are
 * 2^nvars (with a communicator attached: nvars is global and each rank passes
 * and receives its 2^(nvars - log2(world)) block).  `out_sum` (nullable)
 * receives sum_x out[x] over all ranks — the claimed sums of
 * set_inclusion.rs:162-166,193-197.  Returns QG_ERR_ASSERT when some
 * beta + h(x) == 0 (the reference panics in inverse().unwrap(), :51/:63);
 * on any error the contents of `out` are undefined (the reference aborts
 * there, so no caller reads it).
 * Limits: <= 128 monomials per expression, <= 64 distinct tables. */
int qg_logup_column(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const uint64_t* const* tables,
                    const qg_expr_op* h_prog, size_t h_len, const uint64_t* h_consts,
                    size_t h_nconsts, const qg_expr_op* m_prog, size_t m_len,
                    const uint64_t* m_consts, size_t m_nconsts, const uint64_t beta[4],
                    uint64_t* out, uint64_t out_sum[4]);
/* Same with device-resident tables and output (out must not alias a table). */
int qg_logup_column_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const qg_buf* const* tables,
                        const qg_expr_op* h_prog, size_t h_len, const uint64_t* h_consts,
                        size_t h_nconsts, const qg_expr_op* m_prog, size_t m_len,
                        const uint64_t* m_consts, size_t m_nconsts, const uint64_t beta[4],
                        qg_buf* out, uint64_t out_sum[4]);

/* Multiplicities of a Logup lookup (the column the reference's callers build by
 * hand, hyperplonk/src/piops/lookup.rs:186-193): out_m[j] = #{ i : src row i ==
 * table row j } as Fr, for `ncols` source columns of `src_len` entries and
 * `ncols` table columns of `tab_len` entries.  A row is the tuple of its ncols
 * entries; two rows are equal only if every column is.  Inputs must be
 * canonical Montgomery words (values < r, as everywhere in this ABI): rows are
 * compared as 32-byte words.  Duplicate table rows: a tuple the table holds at
 * several rows is counted whole at the LOWEST such row and the others get 0 (a
 * valid Logup assignment; out_m is a function of the inputs alone and equal
 * from run to run).
 * `first_missing` (nullable) receives -1 when every source row is in the table
 * (QG_OK).  Otherwise the call returns QG_ERR_ASSERT (the prover would emit a
 * proof that cannot verify), *first_missing is the lowest source row that is in
 * no table row, qg_last_error names it, and the contents of out_m are
 * undefined.  out_m must not alias an input column (QG_ERR_INVALID).
 * Limits: 1 <= ncols <= 16, 1 <= tab_len < 2^31, 1 <= src_len < 2^32: zero
 * lengths, null pointers and buffers shorter than their stated length return
 * QG_ERR_INVALID, anything over the caps QG_ERR_UNSUPPORTED.  This host-pointer
 * entry returns QG_ERR_UNSUPPORTED on a context with a communicator attached
 * (sharded): a sharded caller holds device blocks, see the _dev entry.
 * QG_LOOKUP_HASH_BITS=<b> (read per call) keeps only the low b bits of the row
 * hash (b = 0: one probe chain; a test switch, the result does not change). */
int qg_lookup_multiplicities(qg_ctx* ctx, uint32_t ncols,
                             const uint64_t* const* src_cols, size_t src_len,
                             const uint64_t* const* tab_cols, size_t tab_len,
                             uint64_t* out_m, int64_t* first_missing);
/* Same with device-resident columns and output.
 * With a communicator attached (world W, this rank r) the call is collective:
 * `src_len` / `tab_len` are this rank's block lengths and every rank passes the
 * same ncols, src_len and tab_len.  Global source row r*src_len + i and global
 * table row r*tab_len + j are the rows of the concatenated blocks (the layout of
 * a sharded VirtualPolynomialStore); out_m receives this rank's block
 * m[r*tab_len .. (r+1)*tab_len) of the global column, which is the same function
 * of the inputs as on one context: a tuple at several global rows is counted
 * whole at the lowest one, also when those rows sit on different ranks.  The
 * table is replicated on every rank (one allgather per column) and the source
 * stays where it is; the counters travel in one all-to-all: at most ncols + 3
 * collectives per call ("lookup_collectives" of qg_ctx_counter).  The caps are
 * global: W*tab_len >= 2^31 or W*src_len >= 2^32 is QG_ERR_UNSUPPORTED.  When
 * any rank's own arguments fail their checks, or the ranks pass different
 * ncols / src_len / tab_len, EVERY rank returns QG_ERR_INVALID (a rank joins the
 * first exchange even then, so none is left waiting).  A source row in no table
 * row: every rank returns QG_ERR_ASSERT with the lowest GLOBAL source row in
 * *first_missing and in qg_last_error; a probe-sequence error on any rank is
 * QG_ERR_DEVICE on every rank. */
int qg_lookup_multiplicities_dev(qg_ctx* ctx, uint32_t ncols,
                                 const qg_buf* const* src_cols, size_t src_len,
                                 const qg_buf* const* tab_cols, size_t tab_len,
                                 qg_buf* out_m, int64_t* first_missing);
/* The same call with the sharded flow chosen by `table_mode`; the entry above
 * is this one with QG_LOOKUP_TABLE_REPLICATED.  Both modes return the same
 * out_m, first_missing and errors, bit for bit; the mode is never chosen for
 * the caller.  On a context with no communicator either mode is the
 * one-context flow (0 collectives).  An unknown mode is QG_ERR_INVALID; ranks
 * that pass different modes all return QG_ERR_INVALID together (the mode
 * travels in the first exchange).
 * QG_LOOKUP_TABLE_PARTITIONED: every tuple has one owner rank, chosen by a hash
 * of the tuple.  Each rank sends the owner one record per distinct tuple of its
 * table block and of its source block (with the local count), the owner matches
 * them, and the counts travel back to the rank that holds the winning table
 * row: 6 collectives per call whatever ncols, all of agreed fixed sizes (the
 * most records any rank sends any rank, rounded up to even).  No rank holds
 * more than its own blocks, its share of the distinct tuples and padding; at
 * most 1024 ranks (QG_ERR_UNSUPPORTED above).  For a table as large as the
 * source (memory or bus consistency, a range check over a committed column);
 * the replicated mode suits a small table under a large source.
 * QG_LOOKUP_OWNER_BITS=<b> (read per call) keeps only the low b bits of the
 * owner hash (b = 0: rank 0 owns every tuple; a test switch, the result does
 * not change).  Counters of qg_ctx_counter: "lookup_routed_tab" and
 * "lookup_routed_src" (records this rank sent), "lookup_exchange_bytes". */
#define QG_LOOKUP_TABLE_REPLICATED  0u   /* the table gathered on every rank */
#define QG_LOOKUP_TABLE_PARTITIONED 1u   /* every tuple matched on its owner rank */
int qg_lookup_multiplicities_dev_ex(qg_ctx* ctx, uint32_t ncols,
                                    const qg_buf* const* src_cols, size_t src_len,
                                    const qg_buf* const* tab_cols, size_t tab_len,
                                    qg_buf* out_m, int64_t* first_missing,
                                    uint32_t table_mode);

/* Column materialiser: out[x] = h(tables[.][x]) for every row x of the
 * hypercube, h a postfix expression over `tables` (the encoding of the sumcheck
 * and Logup entries above) - what the reference's LookupProof::prove reads
 * through get_expr for a column that is not a plain input
 * (hyperplonk/src/piops/lookup.rs:51-59), e.g. a packed column a + 256 b.  Rows
 * are 2^nvars; with a communicator attached nvars is global and each rank passes
 * and receives its 2^(nvars - log2(world)) block (no exchange).  Output words
 * are canonical Montgomery (< r), as qg_lookup_multiplicities compares them.
 * Limits: <= 128 monomials, <= 512 factors, <= 64 distinct tables; beyond them
 * QG_ERR_UNSUPPORTED (there is no interpreter fallback).  `out` must not overlap
 * a table (QG_ERR_INVALID), as are null pointers and short buffers. */
int qg_expr_column(qg_ctx* ctx, uint32_t nvars, uint32_t ntables, const uint64_t* const* tables,
                   const qg_expr_op* prog, size_t len, const uint64_t* consts, size_t nconsts,
                   uint64_t* out);
int qg_expr_column_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                       const qg_buf* const* tables, const qg_expr_op* prog, size_t len,
                       const uint64_t* consts, size_t nconsts, qg_buf* out);

/* Circuit::check_constraints for one constraint expression
 * (hyperplonk/src/frontend/transition_circuit.rs:153-172): `first_row`
 * receives the first row x of the hypercube (this rank's block) with
 * h(x) != 0, or -1 when h vanishes on every row. */
int qg_expr_first_nonzero_dev(qg_ctx* ctx, uint32_t nvars, uint32_t ntables,
                              const qg_buf* const* tables, const qg_expr_op* prog, size_t len,
                              const uint64_t* consts, size_t nconsts, int64_t* first_row);

/* ---------------------------------------------------------------- profiling */
/* Per-kernel device time (ms) of the last call on this context, measured with
 * HIP events on the stream the kernels run on.  `name` is one of the kernel
 * group names listed in DESIGN.md (e.g. "msm_accumulate", "sumcheck_round").
 * Returns total ms and the launch count. */
int qg_ctx_enable_timing(qg_ctx* ctx, int enable);
/* Device Fq Montgomery-multiplication throughput (multiplies per second) from
 * a dependent-chain microbenchmark saturating every CU: the compute roof the
 * MSM's 11-Fq-mult-per-add cost is priced against. */
int qg_microbench_fq_mul(qg_ctx* ctx, double* mul_per_s);
/* FETCH_SIZE calibration for the PMC traffic figures: `gathers` random
 * 128-B table-row gathers in k_msm_accumulate's load pattern (k_fetch_gather),
 * then one 16-B-per-lane streaming read of the whole rows x 128-B table
 * (k_fetch_stream); device ms of each.  Known byte counts for rocprofv3. */
int qg_microbench_fetch(qg_ctx* ctx, size_t rows, size_t gathers, double* gather_ms,
                        double* stream_ms);
int qg_ctx_kernel_time(const qg_ctx* ctx, const char* name, double* total_ms, uint32_t* launches);
/* Additive split of the device-busy time among the k phase names given (the
 * same groups as qg_ctx_kernel_time, timing on): every interval in which m of
 * the listed phases' regions are open - on any of the context's streams - is
 * split evenly among those m phases, so the k values sum to the time at least
 * one of them was running (<= the wall time), where qg_ctx_kernel_time's
 * per-stream spans overlap (an MSM batch's bucketing beside the other side
 * stream's accumulation).  busy_ms[i] receives the share of names[i]. */
int qg_ctx_phase_split(const qg_ctx* ctx, const char* const* names, size_t k, double* busy_ms);
/* Profiling marker: launches an empty kernel (k_trace_marker) of `tag` work-groups
 * on the context stream, so a rocprofv3 kernel trace can be cut into the
 * caller's phases (profiles/kstats.py --legs groups dispatches by the last
 * marker).  No other effect. */
int qg_trace_marker(qg_ctx* ctx, uint32_t tag);
/* Diagnostic counters of the context by name; unknown names give 0.
 * "msm_plan_refetch": MSM bucket-scan plan copies (pinned, event-ordered) that
 * did not carry their run's generation tag and were re-read synchronously.
 * "msm_handover_violation": MSM batches whose event-ordered hand-over between
 * the context stream and the side streams the device guard found unordered
 * (each was recomputed in stream order; 0 while the event ordering holds).
 * "open_checks": KZG quotients checked against p(sigma) - y == q(sigma)(sigma - x)
 * (kzg.rs:85); "open_check_failures": those that failed (each failing call
 * returned QG_ERR_ASSERT, "Polynomial division failed").
 * "events_created": HIP events the context created because its pool of
 * returned events was empty (constant once a repeated workload is warm).
 * "events_pooled": events resting in that pool now; created - pooled is the
 * number in use, which a call leaves as it found it (an event that a failed
 * call did not hand back shows here, long before the pool runs dry).
 * "lookup_collectives": collectives issued by qg_lookup_multiplicities_dev on
 * this (sharded) context, at most ncols + 3 per call with a replicated table
 * and 6 with a partitioned one.
 * "lookup_routed_tab" / "lookup_routed_src": table / source records this rank
 * sent to owner ranks in the partitioned mode (one per distinct tuple of its
 * block).  "lookup_exchange_bytes": bytes this rank received in the payload
 * collectives of either sharded mode (replicated: W*tab_len*(32*ncols + 4) per
 * call; partitioned: the two record exchanges and the counters' way back).
 * "lookup_scratch_bytes": bytes of scratch the context holds now for the lookup
 * multiplicities (grow-only: the largest call so far, all modes together).
 * The sumcheck prover's paths, counted on the host where each kernel is
 * launched (cumulative over the context's calls):
 * "sc_big_pure_rounds": large rounds run by the thread-per-pair kernel on a
 * product of distinct tables (k_sc_big<K,4,true>); "sc_big_sop_rounds": those
 * it ran on any other expression of at most 4 tables and degree at most 3
 * (k_sc_big<4,4,false>); "sc_staged_rounds": large rounds run by the
 * LDS-staged kernel (k_sc_round<K,NP>).
 * "sc_slice_tails" / "sc_stream_tails": calls whose remaining rounds ran in
 * the slice tail (k_sc_slice) / in the streaming tail (k_sc_tail).
 * "sc_generic_calls": calls proved by the interpreted path (expressions
 * outside the compiled envelope, and every qg_sumcheck_prove_cb call).
 * "sc_tail_first_round": the round the last compiled call's tail started at
 * (not cumulative); its parity selects the tail's limb accumulator.
 * Tuning switches of the compiled prover, all read from the environment once
 * per proof (csrc/sumcheck_plan.h, sc_switches):
 *   QG_SC_PERS_LOG=<1..30>    tables of at most 2^k entries go to the tail
 *                             (default 16, never above what the slice tail
 *                             holds); on a sharded context it also lowers the
 *                             gather point: the ranks gather their blocks once
 *                             the folded tables' global size is at most
 *                             2^min(16, k)
 *   QG_SC_BIG_BLOCKS=<1..2048> grid cap of k_sc_big (default 2 per CU)
 *   QG_SC_BLOCKS=<1..2048>    grid cap of k_sc_round (default 3 per CU)
 *   QG_SC_STAGED (set)        k_sc_round runs every large round
 *   QG_SC_NO_SKIP0 (set)      t = 0 is evaluated in every round
 *   QG_SC_OLD_TAIL=<non-zero> k_sc_tail instead of k_sc_slice
 *   QG_SC_WPE (set)           the product sweep built for 4 waves per SIMD
 *   QG_SC_TAIL_BPC=<k>        blocks per CU of a tail's grid cap (default 1;
 *                             below 1 counts as 1; never above occupancy - 1)
 * For the first three, a value outside its range, or not a whole number, makes
 * the call return QG_ERR_INVALID. */
int qg_ctx_counter(const qg_ctx* ctx, const char* name, uint64_t* value);
/* DensePolynomial::evaluate (pcs/src/kzg.rs:78) on a device vector:
 * out = sum_{i < n} poly[i] * x^(shift + i) (Montgomery in and out), by the
 * evaluation kernel the opening check uses.  `shift` is the power offset of a
 * slice of a sharded polynomial.  n == 0 gives 0; n > qg_buf_len or a null
 * handle gives QG_ERR_INVALID.  QG_EVAL_BLOCKS=<k> (read per call) caps the
 * kernel's grid. */
int qg_poly_eval_dev(qg_ctx* ctx, const qg_buf* poly, size_t n, const uint64_t x[4],
                     uint64_t shift, uint64_t out[4]);
/* The same at two points with one pass over each vector: out[P i + j] =
 * sum_{k < lens[j]} polys[j][k] * xs[i]^k for i < 2, j < P (xs: 2 Fr, out: 2 P
 * Fr, Montgomery), the same bits as 2 P qg_poly_eval_dev calls.  It is the
 * same kernel, built for two points: a thread loads each coefficient of its
 * strip once and runs one Horner chain per point (qg_poly_eval_dev: one
 * chain).  The folded inner-product argument's six values come from
 * it unless QG_EVAL_PAIRED=0.  Limits: 1 <= P <= 8; anything else, null
 * pointers and a length beyond its buffer included, is QG_ERR_INVALID.
 * QG_ERR_UNSUPPORTED on a context with a communicator attached ("sharded" in
 * qg_last_error).  QG_EVAL_BLOCKS as above. */
int qg_poly_eval2_dev(qg_ctx* ctx, const qg_buf* const* polys, const size_t* lens, size_t P,
                      const uint64_t* xs, uint64_t* out);
/* TEST ONLY (like qg_selftest_inverse): arms a one-shot fault that the next
 * opening call on this context consumes, so the tests can show that the
 * quotient check catches it; afterwards the context is clean.  kind 0 disarms;
 * 1 SHORT_TRIM: the first nonzero trimmed length the call computes is reduced
 * by `value` (at least 1 remains; on a sharded context the local length, before
 * the exchange); 2 QUOTIENT: 1 is added to coefficient `value mod len` of the
 * call's first non-empty quotient; 3 STAMP: `value` is written into the
 * trimmed-length scan's stamp word at once. */
int qg_debug_open_fault(qg_ctx* ctx, uint32_t kind, uint64_t value);
/* Self-test of the binary-GCD field inversion the Logup column uses per block
 * (csrc/bingcd.h): out[i] = in[i]^-1 (plain canonical integers, 4 x u64 LE;
 * 0 -> 0) in Fr (field = 0) or Fq (field = 1), on the host (ctx may be NULL)
 * or, with on_device, in a device kernel on ctx. */
int qg_selftest_inverse(qg_ctx* ctx, int field, int on_device, const uint64_t* in, uint64_t* out,
                        size_t n);

/* ---- TEST ONLY: the 29-bit-limb layer, one primitive at a time -------------
 * Field elements cross as their raw 9 x uint32 limbs (csrc/field29.h F29), so
 * a test can pass non-canonical representatives and almost-normalized / lazy
 * limb shapes, and reads back the representation, not only the residue.  Every
 * entry runs one thread (or one quad of lanes) per case, addresses nothing
 * with the data, and returns QG_ERR_INVALID for null pointers, an unknown op
 * or field, or more than 65536 cases. */

/* ops of qg_selftest_field29; operands a0..a7, results r0..r3 (unused: 0) */
#define QG_F29_MUL 0           /* r0 = mul29(a0, a1) */
#define QG_F29_SQR 1           /* r0 = sqr29(a0) */
#define QG_F29_MULSUB 2        /* r0 = mulsub29(a0, a1, a2, a3) */
#define QG_F29_MULT 3          /* r0 = mul29t(a0, a1)                (device only) */
#define QG_F29_SQRT 4          /* r0 = sqr29t(a0)                    (device only) */
#define QG_F29_MULSUBT 5       /* r0 = mulsub29t(a0, a1, a2, a3)     (device only) */
#define QG_F29_MULT2 6         /* mul29t2(a0, a1, a2, a3, r0, r1)    (device only) */
#define QG_F29_SQRT2 7         /* sqr29t2(a0, a1, r0, r1)            (device only) */
#define QG_F29_MULTN3 8        /* mul29tn<3>: r[i] = a[i] a[4 + i]   (device only) */
#define QG_F29_MULTN4 9        /* mul29tn<4>                         (device only) */
#define QG_F29_MULTN3_ALIAS 10 /* mul29tn<3> with r aliasing a       (device only) */
#define QG_F29_MULTN4_ALIAS 11 /* mul29tn<4> with r aliasing a       (device only) */
#define QG_F29_NORM 12         /* r0 = norm29(a0) */
#define QG_F29_NORMFULL 13     /* r0 = normfull29(a0) */
#define QG_F29_RED2P 14        /* r0 = red2p29(a0) */
#define QG_F29_RED6P 15        /* r0 = red6p29(a0) */
#define QG_F29_RED16P 16       /* r0 = red16p29(a0) */
#define QG_F29_CANON 17        /* r0 = canon29(a0) */
#define QG_F29_ISZERO8 18      /* r0 limb 0 = is_zero_mod29_fast<8>(a0) */
#define QG_F29_ISZERO20 19     /* r0 limb 0 = is_zero_mod29_fast<20>(a0) */
#define QG_F29_RELIMB 20       /* r0 = to29(from29(a0)) */
#define QG_F29_OP_COUNT 21
#define QG_SELFTEST_F29_IN 72  /* uint32 per case in `in`: a0..a7 */
#define QG_SELFTEST_F29_OUT 36 /* uint32 per case in `out`: r0..r3 */
/* field 0 = Fr, 1 = Fq.  on_device = 0 runs the host build of the primitives
 * (ctx may be NULL; the device-only forms give QG_ERR_UNSUPPORTED), on_device
 * = 1 their gfx950 build on ctx, one thread per case. */
int qg_selftest_field29(qg_ctx* ctx, int field, int op, int on_device, const uint32_t* in, size_t n,
                        uint32_t* out);

/* ops of qg_selftest_curve29 (csrc/curve29.h, csrc/msm.hip; Fq, R = 2^261).
 * A case's input is two points p, q of 4 x 9 limbs each (X, Y, ZZ, ZZZ); an
 * affine operand is q's X, Y. */
#define QG_X29_ADD 0        /* x29_add(p, q) */
#define QG_X29_DBL 1        /* x29_dbl(p) */
#define QG_X29_ADD_AFFINE 2 /* x29_add_affine(p, (q.X, q.Y)) */
#define QG_X29_ACC_FINISH 3 /* x29_acc_finish(p) */
#define QG_X29_RAW 4        /* x29_unraw(x29_raw(p)) */
#define QG_X29_ACC_MADD 5   /* x29_acc_madd_tp(p, q.X, q.Y), then x29_acc_madd_exc when it
                               returned false, as k_msm_accumulate does    (device only) */
#define QG_X29_ADD_Q4 6     /* x29_add_q4(p, q) on one quad of lanes      (device only) */
#define QG_X29_DBL_Q4 7     /* x29_dbl_q4(p) on one quad of lanes         (device only) */
#define QG_X29_OP_COUNT 8
#define QG_SELFTEST_X29_IN 72     /* uint32 per case in `in` */
#define QG_SELFTEST_X29_OUT 36    /* uint32 per case in `out` (one point) ... */
#define QG_SELFTEST_X29_OUT_Q4 144 /* ... or the point every lane 0..3 of the quad returned */
#define QG_X29_FLAG_MAIN 1u /* x29_acc_madd_tp returned true */
#define QG_X29_FLAG_EXC 2u  /* x29_acc_madd_exc ran */
#define QG_X29_FLAG_INF 4u  /* ... and reported infinity (the accumulator is then stale) */
/* flags[i] (one uint32 per case) is written for every op, nonzero only for
 * QG_X29_ACC_MADD.  Cases keep their order: case i of a _Q4 op runs on lanes
 * 4 i .. 4 i + 3, so neighbouring cases share a wave.  The host path (ctx may
 * be NULL) gives QG_ERR_UNSUPPORTED for the device-only ops. */
int qg_selftest_curve29(qg_ctx* ctx, int op, int on_device, const uint32_t* in, size_t n,
                        uint32_t* out, uint32_t* flags);

/* One level of the MSM's bucket-reduction fold: launches k_msm_wfold (quad-
 * cooperative when q4, groups of 16 elements; else single-lane, groups of 64)
 * on m <= 65536 elements (A_e, Y_e) per MSM of `batch` <= 16, element e of
 * MSM b at index b istride + e (istride >= m), in the kernel's input layout:
 * XYZZ of 4 x 8 uint32 words per point, plain integers < 2p in the R = 2^261
 * domain, ZZ == 0 for infinity.  Group w writes A_out[b mo + w] = sum_g A_g +
 * g Y_g over its elements (mo = ceil(m / group)) and, when want_y, Y_out[...] =
 * group sum_g Y_g in the same layout; without want_y (the last level) Y_out
 * is ignored and A_out is canonical in the host's R = 2^256 Montgomery form. */
int qg_selftest_msm_fold(qg_ctx* ctx, int q4, const uint32_t* A, const uint32_t* Y, uint32_t m,
                         uint32_t batch, size_t istride, int want_y, uint32_t* A_out,
                         uint32_t* Y_out);

#ifdef __cplusplus
}
#endif
#endif /* QUILL_GPU_H */
