// Error handling of libquill_gpu's host code: the exception that carries a
// C-ABI error code to qg_guard, and the check that throws it.  No HIP include,
// so a plain C++ translation unit (tests/cpp) can use the headers built on it.
#pragma once
#include <stdexcept>
#include <string>

namespace qg {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define QG_CHECK(cond, code, msg)                  \
  do {                                             \
    if (!(cond)) throw ::qg::Error((code), (msg)); \
  } while (0)

}  // namespace qg
