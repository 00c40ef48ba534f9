// CPU check of the sharded openings' slice geometry
// (quill-zkvm_amd/csrc/open_plan.h) against brute-force counts: a rank's live
// part of a polynomial and of its quotient, the global trimmed length from
// the ranks' local ones, and the group-wide "fits" decision.  Prints
// "ok <name>" per check; exits non-zero when one fails.
#include <cstdio>
#include <vector>

#include "../../quill-zkvm_amd/csrc/open_plan.h"

using namespace qg;

static int fails = 0;
static bool row_ok = true;
static void eq(const char* what, long long got, long long want, size_t W, size_t L, size_t n) {
  if (got == want) return;
  if (row_ok) printf("  %s = %lld, expected %lld (W %zu, L %zu, n %zu)\n", what, got, want, W, L, n);
  row_ok = false;
}
#define EQ(a, b) eq(#a, (long long)(a), (long long)(b), W, L, n)
static void row(const char* name) {
  printf("%s %s\n", row_ok ? "ok" : "FAIL", name);
  if (!row_ok) fails++;
  row_ok = true;
}

// indices i < n inside rank r's slice [r L, (r + 1) L)
static size_t count_below(size_t n, size_t r, size_t L) {
  size_t c = 0;
  for (size_t i = r * L; i < (r + 1) * L; i++) c += i < n;
  return c;
}
// the quotient of n coefficients has the indices i with i + 1 < n
static size_t count_quotient(size_t n, size_t r, size_t L) {
  size_t c = 0;
  for (size_t i = r * L; i < (r + 1) * L; i++) c += i + 1 < n;
  return c;
}

static const size_t WS[] = {1, 2, 4, 8}, LS[] = {1, 2, 16};

int main() {
  for (size_t W : WS)
    for (size_t L : LS)
      for (size_t n = 0; n <= W * L; n++)
        for (size_t r = 0; r < W; r++) {
          EQ(op_live(n, r, L), count_below(n, r, L));
          EQ(op_qlive(n, r, L), count_quotient(n, r, L));
        }
  row("live_qlive");

  // 0/1 patterns of trimmed length n: only the top entry, everything below it,
  // every third entry below it; n <= (W - 1) L leaves the top slices all zero
  for (size_t W : WS)
    for (size_t L : LS)
      for (size_t n = 0; n <= W * L; n++)
        for (int kind = 0; kind < 3; kind++) {
          std::vector<int> v(W * L, 0);
          for (size_t i = 0; i + 1 < n; i++) v[i] = kind == 1 || (kind == 2 && i % 3 == 0);
          if (n) v[n - 1] = 1;
          std::vector<unsigned long long> local(W, 0);
          for (size_t r = 0; r < W; r++)  // brute-force trim of the slice
            for (size_t i = 0; i < L; i++)
              if (v[r * L + i]) local[r] = i + 1;
          EQ(op_global_len(local.data(), W, L), n);
        }
  row("global_len");

  // every assignment of shard sizes from {0, L - 1, L}: S of length ns
  // committed, polynomials of lengths n and ns opened
  for (size_t W : WS)
    for (size_t L : LS) {
      const unsigned long long sizes[3] = {0, L - 1, L};
      size_t combos = 1;
      for (size_t r = 0; r < W; r++) combos *= 3;
      std::vector<unsigned long long> shard(W);
      // the brute-force counts once per (n, r)
      std::vector<size_t> below((W * L + 1) * W), quot((W * L + 1) * W);
      for (size_t n = 0; n <= W * L; n++)
        for (size_t r = 0; r < W; r++) {
          below[n * W + r] = count_below(n, r, L);
          quot[n * W + r] = count_quotient(n, r, L);
        }
      for (size_t c = 0; c < combos; c++) {
        for (size_t r = 0, d = c; r < W; r++, d /= 3) shard[r] = sizes[d % 3];
        for (size_t n = 0; n <= W * L; n++)
          for (size_t ns : {(size_t)0, n / 2, n ? n - 1 : 0, n}) {
            bool all = true;
            for (size_t r = 0; r < W; r++)
              all = all && below[ns * W + r] <= shard[r] && quot[n * W + r] <= shard[r] &&
                    quot[ns * W + r] <= shard[r];
            const size_t opened[2] = {n, ns};
            EQ(op_fits(ns, opened, 2, L, shard.data(), W), all);
          }
      }
    }
  row("fits");
  return fails ? 1 : 0;
}
