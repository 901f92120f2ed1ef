// csv_guard.h — where plain quote parity stops being pandas' quoting (csvin.hip,
// plan.hip): the record index toggles on every quote, and the
// kernels walk each row that holds one with this rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cdr {

namespace {

// The first byte of the row [s, e) at which the quote rule fails, or -1.  The
// row starts outside quotes.  An escaped quote ("" inside quotes) stays inside.
__device__ inline int64_t guard_walk(const uint8_t* buf, int64_t s, int64_t e) {
  bool inq = false;
  int64_t open = -1;
  for (int64_t k = s; k < e; ++k) {
    if (buf[k] != '"') continue;
    if (!inq) {
      if (k != s && buf[k - 1] != ',') return k;  // pandas keeps it as a literal
      inq = true;
      open = k;
    } else if (k + 1 < e && buf[k + 1] == '"') {
      ++k;
    } else {
      const uint8_t nx = k + 1 < e ? buf[k + 1] : (uint8_t)',';
      if (nx != ',' && nx != '\r' && nx != '\n') return k;  // pandas reads on, unquoted
      inq = false;
    }
  }
  return inq ? open : -1;  // the file ends inside quotes
}

}  // namespace

}  // namespace cdr
