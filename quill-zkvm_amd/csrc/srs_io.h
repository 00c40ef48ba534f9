// Host-side pieces of the SRS import / export (srs_io.hip): byte-size bounds,
// the packed "first bad point" word and its message.  No HIP include, so a
// plain C++ translation unit (tests/cpp/srs_io_check.cpp) can use it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/quill_gpu.h"
#include "error.h"

namespace qg {

// Every decode / validate thread that meets a bad point packs (index << 3) |
// reason and folds it into one 64-bit word with atomicMin; the word starts as
// SRS_BAD_NONE (all ones), so the lowest index wins whatever the launch order.
static constexpr uint64_t SRS_BAD_NONE = ~0ull;
static constexpr int SRS_REASON_BITS = 3;
// indices must leave room for the reason bits (and stay below SRS_BAD_NONE)
static constexpr uint64_t SRS_MAX_POINTS = 1ull << 60;

inline uint64_t srs_bad_pack(uint64_t index, uint32_t reason) {
  return (index << SRS_REASON_BITS) | (uint64_t)(reason & 7u);
}

// false: no bad point was recorded
inline bool srs_bad_unpack(uint64_t word, uint64_t* index, uint32_t* reason) {
  if (word == SRS_BAD_NONE) return false;
  *index = word >> SRS_REASON_BITS;
  *reason = (uint32_t)(word & 7u);
  return true;
}

// bytes per point of a format, 0 for an unknown one
inline size_t srs_point_bytes(int format) {
  return format == QG_G1_UNCOMPRESSED ? 64 : format == QG_G1_COMPRESSED ? 32 : 0;
}

// n points of `format` as a byte count; throws QG_ERR_INVALID for an unknown
// format, n == 0, or a count whose byte size or packed index would overflow
inline size_t srs_bytes_checked(size_t n, int format) {
  const size_t pb = srs_point_bytes(format);
  QG_CHECK(pb != 0, QG_ERR_INVALID, "unknown G1 point format");
  QG_CHECK(n > 0, QG_ERR_INVALID, "empty SRS");
  QG_CHECK((uint64_t)n < SRS_MAX_POINTS && n <= SIZE_MAX / pb, QG_ERR_INVALID,
           "SRS point count out of range");
  return n * pb;
}

// [offset, offset + n) inside a table of `len` points, without overflow
inline bool srs_range_ok(size_t offset, size_t n, size_t len) {
  return offset <= len && n <= len - offset;
}

inline const char* srs_reason_text(uint32_t reason) {
  switch (reason) {
    case QG_SRS_BAD_NONCANONICAL: return "coordinate >= p";
    case QG_SRS_BAD_INFINITY: return "malformed point at infinity";
    case QG_SRS_BAD_NOT_SQUARE: return "x^3 + 3 is not a square";
    case QG_SRS_BAD_NOT_ON_CURVE: return "point not on the curve";
    case QG_SRS_BAD_SIGN_FLAG: return "y-sign flag inconsistent with the point";
    default: return "unknown reason";
  }
}

inline std::string srs_bad_message(const char* what, uint64_t index, uint32_t reason) {
  return std::string(what) + ": point " + std::to_string(index) + ": " + srs_reason_text(reason) +
         " (reason " + std::to_string(reason) + ")";
}

}  // namespace qg
