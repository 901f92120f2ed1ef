// csv_parse.h — one numeric cell of a CSV as pandas reads it, for the host and
// the device.
//
// A plain C++ restatement of precise_xstrtod, the float parser behind
// pd.read_csv's default float_precision (pandas' C tokenizer), which the
// reference runs in main.py:75-81.  That parser is not correctly rounded: it
// accumulates up to 17 digits in a double (number = number * 10.0 + digit, two
// roundings), counts the rest into a decimal exponent and scales once, by a
// multiply with or a divide by one of the literals 1e0 ... 1e308.  Every step is
// one IEEE fp64 operation, so the same steps give the same bits anywhere.
// hipcc compiles this for the parse kernel of csvin.hip, g++ for the host check
// (tools/csv_parse_check.cpp); both need -ffp-contract=off (no fma in the
// digit loop), and the divide must be the correctly rounded IEEE one.
//
// A cell is one of four kinds:
//   CSVP_FLOAT  [+-] digits [. digits] [(e|E) [+-] digits], at least one digit
//               in the mantissa, nothing else: the parsed value
//   CSVP_INT    [+-] and 1..15 digits: exact, and equal to what pandas gives
//               when it types the whole column int64 and the caller casts
//   CSVP_EMPTY  no bytes: NaN (pandas' NaN, 0x7FF8000000000000)
//   CSVP_DEFER  anything else; nothing is guessed.  That is: blanks, the words
//               (NaN, inf, Infinity, NA, null, ...), an exponent mark without
//               digits, int-like text of 16 or more digits (an int64 column
//               converts it with one rounding, a float column with up to 17),
//               "-0" (0 in an int64 column, -0.0 in a float one), an adjusted
//               exponent outside [-308, 308] (pandas scales those in two steps
//               or reports a range error), a result of +-inf, and any other byte
//               (a quote among them).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSVP_HD __host__ __device__ inline
#else
#define CSVP_HD inline
#endif

enum { CSVP_INT = 0, CSVP_FLOAT = 1, CSVP_EMPTY = 2, CSVP_DEFER = 3 };

// the 309 literals 1e0 ... 1e308 (1e00 ... 1e09 are the same numbers)
#define CSVP_R10(a) a##0, a##1, a##2, a##3, a##4, a##5, a##6, a##7, a##8, a##9
#define CSVP_R100(a)                                                                   \
  CSVP_R10(a##0), CSVP_R10(a##1), CSVP_R10(a##2), CSVP_R10(a##3), CSVP_R10(a##4),     \
      CSVP_R10(a##5), CSVP_R10(a##6), CSVP_R10(a##7), CSVP_R10(a##8), CSVP_R10(a##9)

namespace csvp {

constexpr int kMaxDigits = 17;     // digits accumulated into the double
constexpr int kMaxIntDigits = 15;  // 10^15 < 2^53: the accumulation is exact
constexpr int kMaxExp = 308;

CSVP_HD bool dig(unsigned c) { return c - '0' <= 9u; }

}  // namespace csvp

// The kind of the cell p[0, len); *out is written for every kind but CSVP_DEFER.
CSVP_HD int csvp_cell(const uint8_t* p, int len, double* out) {
  using namespace csvp;
  if (len == 0) {
    const uint64_t nan = 0x7FF8000000000000ull;
    memcpy(out, &nan, 8);
    return CSVP_EMPTY;
  }
  int i = 0;
  bool neg = false;
  if (p[0] == '-' || p[0] == '+') {
    neg = p[0] == '-';
    i = 1;
  }
  double number = 0.0;
  int exponent = 0, nd = 0;
  const int i0 = i;
  bool nonzero = false;
  while (i < len && dig(p[i])) {
    if (nd < kMaxDigits) {
      number = number * 10.0 + (double)(int)(p[i] - '0');
      ++nd;
    } else {
      ++exponent;
    }
    nonzero |= p[i] != '0';
    ++i;
  }
  const int int_digits = i - i0;
  bool int_like = true;
  if (i < len && p[i] == '.') {
    int_like = false;
    ++i;
    int ndec = 0;
    while (nd < kMaxDigits && i < len && dig(p[i])) {
      number = number * 10.0 + (double)(int)(p[i] - '0');
      ++i;
      ++nd;
      ++ndec;
    }
    while (i < len && dig(p[i])) ++i;  // (only reached with 17 digits taken)
    exponent -= ndec;
  }
  if (nd == 0) return CSVP_DEFER;
  if (neg) number = -number;
  if (i < len && (p[i] == 'e' || p[i] == 'E')) {
    int_like = false;
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '-' || p[i] == '+')) {
      eneg = p[i] == '-';
      ++i;
    }
    int n = 0, ne = 0;
    while (i < len && dig(p[i])) {
      if (n < 100000) n = n * 10 + (int)(p[i] - '0');
      ++ne;
      ++i;
    }
    // no digit: pandas un-reads the mark and the cell is text; 17 or more: it
    // stops reading; a huge exponent is out of range whatever the mantissa
    if (ne == 0 || ne >= kMaxDigits || n >= 100000) return CSVP_DEFER;
    exponent += eneg ? -n : n;
  }
  if (i != len) return CSVP_DEFER;
  if (int_like) {
    if (int_digits > kMaxIntDigits || (neg && !nonzero)) return CSVP_DEFER;
    *out = number;
    return CSVP_INT;
  }
  if (exponent > kMaxExp || exponent < -kMaxExp) return CSVP_DEFER;
  const double e[kMaxExp + 1] = {CSVP_R100(1e), CSVP_R100(1e1), CSVP_R100(1e2), 1e300, 1e301,
                                 1e302,         1e303,          1e304,          1e305, 1e306,
                                 1e307,         1e308};
  if (exponent > 0)
    number *= e[exponent];
  else
    number /= e[-exponent];
  if (number - number != 0.0) return CSVP_DEFER;  // +-inf
  *out = number;
  return CSVP_FLOAT;
}
