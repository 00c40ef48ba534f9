// The slice geometry of the sharded openings (mlpcs.hip: mle_open_batch_sharded,
// ipa_prove_sharded, quotients_sharded).  Rank r of W holds the slice
// [r L, (r + 1) L) of a global coefficient vector, and the matching slice of the
// SRS.  Plain integers - no HIP, no field types - so
// tests/cpp/open_plan_check.cpp pins them on the CPU.
#pragma once
#include <stddef.h>

namespace qg {

// The global trimmed length from the ranks' local ones (local[r]: highest
// nonzero index + 1 inside rank r's slice, 0 for an all-zero slice): the
// largest (slice offset + local length) over the nonzero slices.
template <class T>
inline size_t op_global_len(const T* local, size_t W, size_t L) {
  size_t n = 0;
  for (size_t r = 0; r < W; r++)
    if (local[r] && r * L + (size_t)local[r] > n) n = r * L + (size_t)local[r];
  return n;
}

// rank r's live part of a polynomial of global trimmed length n: the
// coefficients i < n inside [r L, (r + 1) L)
inline size_t op_live(size_t n, size_t r, size_t L) {
  return n > r * L ? (n - r * L < L ? n - r * L : L) : 0;
}

// ... and of its KZG quotient, which has the n - 1 coefficients q_i = s_{i+1}
inline size_t op_qlive(size_t n, size_t r, size_t L) { return n ? op_live(n - 1, r, L) : 0; }

// The group-wide "Polynomial degree exceeds max degree" decision of one
// sharded proof, from values every rank holds alike (shard[r]: the bases of
// rank r's SRS shard): S, of global trimmed length ns, is committed, and the
// cnt polynomials of global trimmed lengths n[.] are opened (their quotients
// are committed).  True when every rank's shard covers all of its parts.
template <class T>
inline bool op_fits(size_t ns, const size_t* n, size_t cnt, size_t L, const T* shard, size_t W) {
  for (size_t r = 0; r < W; r++) {
    if (op_live(ns, r, L) > (size_t)shard[r]) return false;
    for (size_t p = 0; p < cnt; p++)
      if (op_qlive(n[p], r, L) > (size_t)shard[r]) return false;
  }
  return true;
}

}  // namespace qg
