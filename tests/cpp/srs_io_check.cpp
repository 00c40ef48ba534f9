// CPU check of the host-only part of the SRS import / export
// (quill-zkvm_amd/csrc/srs_io.h): byte-size bounds, range checks, the packed
// "lowest bad point" word and its message.  Prints "ok <name>" per check;
// exits non-zero when one fails.  Built with -fsanitize=address,undefined by
// tests/test_srs_io_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../quill-zkvm_amd/csrc/srs_io.h"

using namespace qg;

static int fails = 0;
static bool row_ok = true;
static void eq(const char* what, unsigned long long got, unsigned long long want) {
  if (got == want) return;
  printf("  %s = %llu, expected %llu\n", what, got, want);
  row_ok = false;
}
#define EQ(a, b) eq(#a, (unsigned long long)(a), (unsigned long long)(b))
#define TRUE(a) eq(#a, (a) ? 1 : 0, 1)
static void row(const char* name) {
  printf("%s %s\n", row_ok ? "ok" : "FAIL", name);
  if (!row_ok) fails++;
  row_ok = true;
}

template <class F>
static int code_of(F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code;
  }
  return 0;
}

int main() {
  EQ(srs_point_bytes(QG_G1_UNCOMPRESSED), 64);
  EQ(srs_point_bytes(QG_G1_COMPRESSED), 32);
  EQ(srs_point_bytes(2), 0);
  EQ(srs_point_bytes(-1), 0);
  row("point_bytes");

  EQ(srs_bytes_checked(1, QG_G1_COMPRESSED), 32);
  EQ(srs_bytes_checked(4097, QG_G1_UNCOMPRESSED), 4097 * 64);
  EQ(srs_bytes_checked((size_t)1 << 24, QG_G1_UNCOMPRESSED), (size_t)1 << 30);
  EQ(code_of([] { srs_bytes_checked(0, QG_G1_COMPRESSED); }), QG_ERR_INVALID);
  EQ(code_of([] { srs_bytes_checked(1, 7); }), QG_ERR_INVALID);
  EQ(code_of([] { srs_bytes_checked(SIZE_MAX, QG_G1_COMPRESSED); }), QG_ERR_INVALID);
  EQ(code_of([] { srs_bytes_checked(SIZE_MAX / 64 + 1, QG_G1_UNCOMPRESSED); }), QG_ERR_INVALID);
  EQ(code_of([] { srs_bytes_checked((size_t)SRS_MAX_POINTS, QG_G1_COMPRESSED); }), QG_ERR_INVALID);
  EQ(code_of([] { srs_bytes_checked(SIZE_MAX / 32 + 1, QG_G1_COMPRESSED); }), QG_ERR_INVALID);
  EQ(srs_bytes_checked(SIZE_MAX / 32, QG_G1_COMPRESSED), (SIZE_MAX / 32) * 32);
  row("bytes_checked");

  TRUE(srs_range_ok(0, 0, 0));
  TRUE(srs_range_ok(0, 10, 10));
  TRUE(srs_range_ok(10, 0, 10));
  TRUE(!srs_range_ok(11, 0, 10));
  TRUE(!srs_range_ok(1, 10, 10));
  TRUE(!srs_range_ok(5, SIZE_MAX, 10));  // offset + n would wrap
  TRUE(!srs_range_ok(SIZE_MAX, SIZE_MAX, SIZE_MAX - 1));
  row("range");

  uint64_t idx = 99;
  uint32_t why = 99;
  TRUE(!srs_bad_unpack(SRS_BAD_NONE, &idx, &why));
  EQ(idx, 99);
  EQ(why, 99);
  for (uint64_t i : {(uint64_t)0, (uint64_t)7, (uint64_t)300, ((uint64_t)1 << 32) + 5,
                     (uint64_t)(SRS_MAX_POINTS - 1)})
    for (uint32_t r = 1; r <= 5; r++) {
      const uint64_t w = srs_bad_pack(i, r);
      TRUE(w < SRS_BAD_NONE);
      TRUE(srs_bad_unpack(w, &idx, &why));
      EQ(idx, i);
      EQ(why, r);
    }
  // the minimum of the packed words is the lowest index, whatever its reason
  TRUE(srs_bad_pack(7, 5) < srs_bad_pack(300, 1));
  TRUE(srs_bad_pack(7, 1) < srs_bad_pack(8, 1));
  TRUE(srs_bad_pack(0, 1) < SRS_BAD_NONE);
  row("bad_word");

  for (uint32_t r = 1; r <= 5; r++) TRUE(strcmp(srs_reason_text(r), "unknown reason") != 0);
  TRUE(strcmp(srs_reason_text(0), "unknown reason") == 0);
  TRUE(strcmp(srs_reason_text(6), "unknown reason") == 0);
  const std::string m = srs_bad_message("SRS import", 7, QG_SRS_BAD_NONCANONICAL);
  TRUE(m == "SRS import: point 7: coordinate >= p (reason 1)");
  TRUE(srs_bad_message("x", ~0ull >> 3, 5).find("2305843009213693951") != std::string::npos);
  row("messages");

  return fails ? 1 : 0;
}
