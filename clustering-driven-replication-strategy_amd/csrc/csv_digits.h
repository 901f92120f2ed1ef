// csv_digits.h — the cell text of the features CSV, for the host and the device.
//
// A plain C++ restatement of compute_features.java_double_legacy and
// _legacy_digits (the pre-19 JDK's Double.toString) and of
// str(int(v)) for the long columns.  hipcc compiles it for the cell kernel of
// csvout.hip, g++ for the host check (tools/csv_digits_check.cpp); both need
// -ffp-contract=off, because the decimal-exponent estimate rounds every
// multiply and add separately.
//
// Range.  Every finite double with 2^-128 <= |x| < 2^128 is formatted, and so
// are NaN, +-Infinity and +-0.0; subnormals and finite values outside the range
// are deferred to the host (csvd_double returns 0).
//
// Limb count of the multi-word arm.  The arm keeps B (the scaled value), S (the
// scale), M (the scaled half gap) and TS = 10 S.  Throughout the loop r < S,
// B = 10 r < 10 S, and an M that lets the loop go on satisfies B + M < TS, so
// after one more "* 10" M < 100 S and B + M < 110 S < 2^7 S.  S is largest at
// the small end: for bin_exp < 0 the common factor is 2^b5 (b5 = -dec) and the
// m2 < 0 rescue shifts by 54 - n_fract (one more for a power of two), which
// gives S = 2^(53 - bin_exp - b5) (2^(54 - bin_exp - b5) for a power of two).
// At bin_exp = -128, dec = -39 that is 2^142 (2^143), and when the estimate of
// dec is one too high (the q == 0 case) one bit more: S <= 2^144, so every
// operand is below 2^151.  For bin_exp >= 0, S = 5^dec 2^max(0, 105 + dec -
// bin_exp) stays below 2^109.  Five 32-bit limbs (160 bits) hold all of them
// with 9 bits to spare; CSVD_TRACK_BITS makes the host check measure it.
//
// Device hygiene: no runtime-indexed local array (the limbs are indexed by
// fully unrolled loops only), digits packed as 4-bit values in two 64-bit
// words, the text packed in four 64-bit words, and every quotient digit comes
// from an fp64 estimate that is corrected by compare-and-subtract: no emulated
// 64-bit or multi-word division.  Divisions by constants compile to multiplies.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSVD_HD __host__ __device__ inline
#else
#define CSVD_HD inline
#endif
#ifdef __clang__
#define CSVD_UNROLL _Pragma("unroll")
#else
#define CSVD_UNROLL
#endif

#ifdef CSVD_TRACK_BITS
static int csvd_max_bits = 0;  // host check: widest multi-word operand seen
#endif

namespace csvd {

constexpr int kLimbs = 5;      // 160 bits (see the derivation above)
constexpr int kMaxText = 26;   // longest cell text in bytes
constexpr int kMinBinExp = -128, kMaxBinExp = 127;  // the formatted range

// ---- the text: up to 32 bytes packed little-endian in four words -----------
struct Text {
  uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  int n = 0;
};

CSVD_HD void put(Text& t, unsigned ch) {
  const uint64_t v = (uint64_t)(ch & 0xFF) << ((t.n & 7) * 8);
  const int k = t.n >> 3;
  t.w0 |= k == 0 ? v : 0;
  t.w1 |= k == 1 ? v : 0;
  t.w2 |= k == 2 ? v : 0;
  t.w3 |= k == 3 ? v : 0;
  ++t.n;
}

CSVD_HD void put8(Text& t, uint64_t chars, int count) {  // the low `count` bytes of chars
  for (int i = 0; i < count; ++i) put(t, (unsigned)(chars >> (8 * i)));
}

// ---- digits: 4 bits each, the last digit in the lowest nibble ---------------
struct Digits {
  uint64_t hi = 0, lo = 0;
  int n = 0;
};

CSVD_HD void push(Digits& d, unsigned q) {
  d.hi = (d.hi << 4) | (d.lo >> 60);
  d.lo = (d.lo << 4) | (q & 15);
  ++d.n;
}

CSVD_HD unsigned nib(const Digits& d, int pos) {  // pos counts from the last digit
  return (unsigned)((pos < 16 ? d.lo >> (4 * pos) : d.hi >> (4 * (pos - 16))) & 15);
}

CSVD_HD void nib_set(Digits& d, int pos, unsigned v) {
  if (pos < 16)
    d.lo = (d.lo & ~(15ull << (4 * pos))) | ((uint64_t)v << (4 * pos));
  else
    d.hi = (d.hi & ~(15ull << (4 * (pos - 16)))) | ((uint64_t)v << (4 * (pos - 16)));
}

CSVD_HD unsigned digit(const Digits& d, int i) { return nib(d, d.n - 1 - i); }  // from the front

// digits[-1] + 1 with the carry through 9s; 9...9 -> 10...0 and exp + 1
CSVD_HD void round_up(Digits& d, int& exp) {
  int pos = 0;
  while (nib(d, pos) == 9 && pos < d.n - 1) {
    nib_set(d, pos, 0);
    ++pos;
  }
  if (nib(d, pos) == 9) {
    nib_set(d, pos, 1);
    ++exp;
  } else {
    nib_set(d, pos, nib(d, pos) + 1);
  }
}

// a 9-digit group (v < 10^9) as nine nibbles, the last digit lowest
CSVD_HD uint64_t bcd9(uint32_t v) {
  uint64_t r = 0;
CSVD_UNROLL
  for (int i = 0; i < 9; ++i) {
    const uint32_t q = v / 10u;
    r |= (uint64_t)(v - q * 10u) << (4 * i);
    v = q;
  }
  return r;
}

// the decimal digits of v >= 1 (v < 2^63), trailing zeros stripped; returns
// the digit count of v with them
CSVD_HD int digits_of_u64(uint64_t v, Digits& d, bool strip) {
  const uint64_t a = v / 1000000000ull;                 // < 9.3e9
  const uint32_t c = (uint32_t)(v - a * 1000000000ull);
  const uint32_t top = (uint32_t)(a / 1000000000ull);   // 0..9
  const uint32_t b = (uint32_t)(a - (uint64_t)top * 1000000000ull);
  const uint64_t g0 = bcd9(c), g1 = bcd9(b);            // nibbles 0..8, 9..17
  uint64_t lo = g0 | (g1 << 36);
  uint64_t hi = (g1 >> 28) | ((uint64_t)top << 8);      // nibbles 16, 17, 18
  const int len = hi ? 16 + (67 - __builtin_clzll(hi)) / 4 : (67 - __builtin_clzll(lo)) / 4;
  int tz = 0;
  if (strip) tz = lo ? __builtin_ctzll(lo) / 4 : 16 + __builtin_ctzll(hi) / 4;
  const int sh = 4 * tz;
  if (sh >= 64) {
    lo = hi >> (sh - 64);
    hi = 0;
  } else if (sh) {
    lo = (lo >> sh) | (hi << (64 - sh));
    hi >>= sh;
  }
  d.hi = hi;
  d.lo = lo;
  d.n = len - tz;
  return len;
}

// ---- small helpers ------------------------------------------------------------
CSVD_HD int n5_bits(int i) { return ((i * 152170) >> 16) + 1; }  // bit length of 5^i, i < 27

CSVD_HD uint64_t pow5_u64(int e) {  // e < 28
  uint64_t p = 1;
  for (int i = 0; i < e; ++i) p *= 5;
  return p;
}

// floor(log10(2^p)) for 0 <= p < 64
CSVD_HD int pow2_dec_digits(int p) { return (p * 1233) >> 12; }

// ---- the 32-bit and 64-bit arms: Java's int and long arithmetic ----------------
// U is uint32_t / uint64_t and I its signed twin: products and sums wrap as
// two's complement, comparisons are signed, a shift by the width or more is 0.
template <typename U>
CSVD_HD U shl_wrap(U v, int sh) {
  return sh >= (int)(8 * sizeof(U)) ? (U)0 : (U)(v << sh);
}

// b / s for 0 <= b, 0 < s and a quotient of a few units: fp64 estimate, then
// compare-and-subtract; rem = b % s
template <typename U>
CSVD_HD unsigned small_div(U b, U s, double rs, U& rem) {
  int q = (int)((double)b * rs);
  if (q < 0) q = 0;
  U t = (U)((U)q * s);
  while (t > b) {  // the estimate was one too high
    t -= s;
    --q;
  }
  U r = b - t;
  while (r >= s) {
    r -= s;
    ++q;
  }
  rem = r;
  return (unsigned)q;
}

template <typename U, typename I>
CSVD_HD void small_arm(uint64_t fract, int b5, int b2, int s5, int s2, int m2, int& dec,
                       Digits& d, bool& low, bool& high, int& tie) {
  U b = (U)((fract * pow5_u64(b5)) << b2);
  const U s = (U)(pow5_u64(s5) << s2);
  U m = shl_wrap<U>((U)pow5_u64(b5), m2);
  const U ts = (U)(s * 10u);
  const double rs = 1.0 / (double)s;
  U r;
  unsigned q = small_div<U>(b, s, rs, r);
  b = (U)(r * 10u);
  m = (U)(m * 10u);
  low = (I)b < (I)m;
  high = (I)(U)(b + m) > (I)ts;
  if (q == 0 && !high)
    --dec;
  else
    push(d, q);
  if (dec < -3 || dec >= 8) low = high = false;
  while (!low && !high && d.n < 30) {
    q = small_div<U>(b, s, rs, r);
    b = (U)(r * 10u);
    m = (U)(m * 10u);
    if ((I)m > 0) {
      low = (I)b < (I)m;
      high = (I)(U)(b + m) > (I)ts;
    } else {
      low = high = true;
    }
    push(d, q);
  }
  const I t = (I)(U)((U)(b << 1) - ts);
  tie = t > 0 ? 1 : (t < 0 ? -1 : 0);
}

// ---- the multi-word arm: 160-bit unsigned integers ----------------------------
struct Big {
  uint32_t l[kLimbs];  // indexed by unrolled loops only
};

CSVD_HD void big_track(const Big& a) {
#ifdef CSVD_TRACK_BITS
  for (int i = kLimbs - 1; i >= 0; --i)
    if (a.l[i]) {
      const int bits = 32 * i + 32 - __builtin_clz(a.l[i]);
      if (bits > csvd_max_bits) csvd_max_bits = bits;
      break;
    }
#else
  (void)a;
#endif
}

CSVD_HD Big big_from_u64(uint64_t v) {
  Big a;
CSVD_UNROLL
  for (int i = 0; i < kLimbs; ++i) a.l[i] = 0;
  a.l[0] = (uint32_t)v;
  a.l[1] = (uint32_t)(v >> 32);
  return a;
}

CSVD_HD void big_mul_small(Big& a, uint32_t f) {
  uint64_t carry = 0;
CSVD_UNROLL
  for (int i = 0; i < kLimbs; ++i) {
    const uint64_t p = (uint64_t)a.l[i] * f + carry;
    a.l[i] = (uint32_t)p;
    carry = p >> 32;
  }
#ifdef CSVD_TRACK_BITS
  if (carry) csvd_max_bits = 32 * kLimbs + 1;  // an overflow of the limbs
#endif
  big_track(a);
}

CSVD_HD void big_mul_pow5(Big& a, int e) {
  while (e >= 13) {
    big_mul_small(a, 1220703125u);  // 5^13
    e -= 13;
  }
  uint32_t p = 1;
  for (int i = 0; i < e; ++i) p *= 5;
  if (e) big_mul_small(a, p);
}

CSVD_HD void big_shl(Big& a, int sh) {
  while (sh >= 32) {
#ifdef CSVD_TRACK_BITS
    if (a.l[kLimbs - 1]) csvd_max_bits = 32 * kLimbs + 1;
#endif
CSVD_UNROLL
    for (int i = kLimbs - 1; i > 0; --i) a.l[i] = a.l[i - 1];
    a.l[0] = 0;
    sh -= 32;
  }
  if (sh) {
#ifdef CSVD_TRACK_BITS
    if (a.l[kLimbs - 1] >> (32 - sh)) csvd_max_bits = 32 * kLimbs + 1;
#endif
CSVD_UNROLL
    for (int i = kLimbs - 1; i > 0; --i) a.l[i] = (a.l[i] << sh) | (a.l[i - 1] >> (32 - sh));
    a.l[0] <<= sh;
  }
  big_track(a);
}

CSVD_HD int big_cmp(const Big& a, const Big& b) {  // -1, 0, 1
  int r = 0;
CSVD_UNROLL
  for (int i = 0; i < kLimbs; ++i)  // the highest differing limb decides
    r = a.l[i] > b.l[i] ? 1 : (a.l[i] < b.l[i] ? -1 : r);
  return r;
}

CSVD_HD void big_add(Big& a, const Big& b) {
  uint64_t carry = 0;
CSVD_UNROLL
  for (int i = 0; i < kLimbs; ++i) {
    const uint64_t s = (uint64_t)a.l[i] + b.l[i] + carry;
    a.l[i] = (uint32_t)s;
    carry = s >> 32;
  }
#ifdef CSVD_TRACK_BITS
  if (carry) csvd_max_bits = 32 * kLimbs + 1;
#endif
  big_track(a);
}

CSVD_HD void big_sub(Big& a, const Big& b) {  // a >= b
  int64_t borrow = 0;
CSVD_UNROLL
  for (int i = 0; i < kLimbs; ++i) {
    const int64_t s = (int64_t)a.l[i] - b.l[i] + borrow;
    a.l[i] = (uint32_t)s;
    borrow = s >> 32;  // 0 or -1
  }
}

CSVD_HD double big_to_double(const Big& a) {
  double v = 0.0;
CSVD_UNROLL
  for (int i = kLimbs - 1; i >= 0; --i) v = v * 4294967296.0 + (double)a.l[i];
  return v;
}

// b / s for b < 10 s or so: fp64 estimate from all limbs, corrected by
// compare-and-subtract; b becomes the remainder
CSVD_HD unsigned big_div_digit(Big& b, const Big& s, double rs) {
  int q = (int)(big_to_double(b) * rs);
  if (q < 0) q = 0;
  Big t = s;
  big_mul_small(t, (uint32_t)q);
  while (big_cmp(t, b) > 0) {  // the estimate was one too high
    big_sub(t, s);
    --q;
  }
  big_sub(b, t);
  while (big_cmp(b, s) >= 0) {
    big_sub(b, s);
    ++q;
  }
  return (unsigned)q;
}

CSVD_HD void big_arm(uint64_t fract, int b5, int b2, int s5, int s2, int m2, int& dec, Digits& d,
                     bool& low, bool& high, int& tie) {
  Big s = big_from_u64(1);
  big_mul_pow5(s, s5);
  big_shl(s, s2);
  Big m = big_from_u64(1);
  big_mul_pow5(m, b5 + 1);
  big_shl(m, m2 + 1);
  Big ts = s;
  big_mul_small(ts, 10);
  Big b = big_from_u64(fract);
  big_mul_pow5(b, b5);
  big_shl(b, b2);
  const double rs = 1.0 / big_to_double(s);
  unsigned q = big_div_digit(b, s, rs);
  big_mul_small(b, 10);
  Big bm = b;
  big_add(bm, m);
  low = big_cmp(b, m) < 0;
  high = big_cmp(ts, bm) <= 0;
  if (q == 0 && !high)
    --dec;
  else
    push(d, q);
  if (dec < -3 || dec >= 8) low = high = false;
  while (!low && !high && d.n < 30) {
    q = big_div_digit(b, s, rs);
    big_mul_small(b, 10);
    big_mul_small(m, 10);
    bm = b;
    big_add(bm, m);
    low = big_cmp(b, m) < 0;
    high = big_cmp(ts, bm) <= 0;
    push(d, q);
  }
  tie = 0;
  if (high && low) {
    Big b2x = b;
    big_add(b2x, b);
    tie = big_cmp(b2x, ts);
  }
}

// ---- _legacy_digits ------------------------------------------------------------
// Digits and decimal exponent (value = 0.d1d2... x 10^exp) of fract * 2^(bin_exp
// - 52), fract normalised to 53 bits of which the top n_sig are significant.
// csvd_double passes n_sig = 53 (subnormals are deferred); for a double the
// width tests then give b_bits >= n_sig + 2 = 55, so only Java's float (n_sig =
// 24) reaches the 32-bit arm, which is kept as the restated code has it and
// checked on the host with n_sig = 24.
// arm (when not null): 1 integer path, 2 32-bit, 3 64-bit, 4 multi-word.
CSVD_HD void legacy_digits(int bin_exp, uint64_t fract, int n_sig, Digits& d, int& exp,
                           int* arm) {
  const int tail = __builtin_ctzll(fract);
  const int n_fract = 53 - tail;
  const int n_tiny = n_fract - bin_exp - 1 > 0 ? n_fract - bin_exp - 1 : 0;
  if (n_tiny == 0 && -21 <= bin_exp && bin_exp <= 62) {
    // an integer: all its digits, rounded (half up) at 10^drop
    const int p = bin_exp - n_sig - 1;
    const int drop = (bin_exp > n_sig && 1 < p && p < 64) ? pow2_dec_digits(p) : 0;
    uint64_t v = bin_exp >= 52 ? fract << (bin_exp - 52) : fract >> (52 - bin_exp);
    unsigned last = 0;  // the highest dropped digit decides the half-up rounding
    for (int i = 0; i < drop; ++i) {
      const uint64_t q = v / 10u;
      last = (unsigned)(v - q * 10u);
      v = q;
    }
    v += last >= 5u;
    exp = drop + digits_of_u64(v, d, true);
    if (arm) *arm = 1;
    return;
  }
  uint64_t mbits = 0x3FF0000000000000ull | (fract & ((1ull << 52) - 1));
  double mant;
  memcpy(&mant, &mbits, 8);
  const double est = (mant - 1.5) * 0.289529654 + 0.176091259 + (double)bin_exp * 0.301029995663981;
  int dec = (int)est;
  if ((double)dec > est) --dec;  // floor
  const int b5 = dec < 0 ? -dec : 0;
  int b2 = b5 + n_tiny + bin_exp;
  const int s5 = dec > 0 ? dec : 0;
  int s2 = s5 + n_tiny;
  int m2 = b2 - n_sig;
  fract >>= tail;
  b2 -= n_fract - 1;
  const int common = b2 < s2 ? b2 : s2;
  b2 -= common;
  s2 -= common;
  m2 -= common;
  if (n_fract == 1) m2 -= 1;  // a power of two: the gap below is half as wide
  if (m2 < 0) {
    b2 -= m2;
    s2 -= m2;
    m2 = 0;
  }
  const int b_bits = n_fract + b2 + (b5 < 27 ? n5_bits(b5) : 3 * b5);
  const int ts_bits = s2 + 1 + (s5 + 1 < 27 ? n5_bits(s5 + 1) : 3 * (s5 + 1));
  bool low, high;
  int tie;
  if (b_bits < 64 && ts_bits < 64) {
    if (b_bits < 32 && ts_bits < 32) {
      small_arm<uint32_t, int32_t>(fract, b5, b2, s5, s2, m2, dec, d, low, high, tie);
      if (arm) *arm = 2;
    } else {
      small_arm<uint64_t, int64_t>(fract, b5, b2, s5, s2, m2, dec, d, low, high, tie);
      if (arm) *arm = 3;
    }
  } else {
    big_arm(fract, b5, b2, s5, s2, m2, dec, d, low, high, tie);
    if (arm) *arm = 4;
  }
  exp = dec + 1;
  if (high && (!low || tie > 0 || (tie == 0 && (nib(d, 0) & 1)))) round_up(d, exp);
}

CSVD_HD void put_int(Text& t, int v) {  // |v| < 1000
  if (v < 0) {
    put(t, '-');
    v = -v;
  }
  if (v >= 100) put(t, '0' + v / 100);
  if (v >= 10) put(t, '0' + v / 10 % 10);
  put(t, '0' + v % 10);
}

}  // namespace csvd

// java_double_legacy(x): the text in t, its length returned; 0 = deferred to the
// host (a subnormal, or a finite |x| outside [2^-128, 2^128)).  arm (when not
// null): 0 special value, 1 integer path, 2 32-bit, 3 64-bit, 4 multi-word.
CSVD_HD int csvd_double(double x, csvd::Text& t, int* arm = nullptr) {
  using namespace csvd;
  uint64_t bits;
  memcpy(&bits, &x, 8);
  const bool neg = bits >> 63;
  uint64_t fract = bits & ((1ull << 52) - 1);
  const int be = (int)((bits >> 52) & 0x7FF);
  t = Text();
  if (arm) *arm = 0;
  if (be == 0x7FF) {
    if (fract)
      put8(t, 0x4E614Eull, 3);  // "NaN"
    else {
      if (neg) put(t, '-');
      put8(t, 0x7974696E69666E49ull, 8);  // "Infinity"
    }
    return t.n;
  }
  if (be == 0) {
    if (fract) return 0;  // subnormal
    if (neg) put(t, '-');
    put8(t, 0x302E30ull, 3);  // "0.0"
    return t.n;
  }
  const int bin_exp = be - 1023;
  if (bin_exp < kMinBinExp || bin_exp > kMaxBinExp) return 0;
  fract |= 1ull << 52;
  Digits d;
  int exp;
  legacy_digits(bin_exp, fract, 53, d, exp, arm);
  if (neg) put(t, '-');
  if (0 < exp && exp < 8) {
    if (d.n <= exp) {
      for (int i = 0; i < exp; ++i) put(t, i < d.n ? '0' + digit(d, i) : '0');
      put(t, '.');
      put(t, '0');
    } else {
      for (int i = 0; i < d.n; ++i) {
        if (i == exp) put(t, '.');
        put(t, '0' + digit(d, i));
      }
    }
  } else if (-3 < exp && exp <= 0) {
    put(t, '0');
    put(t, '.');
    for (int i = 0; i < -exp; ++i) put(t, '0');
    for (int i = 0; i < d.n; ++i) put(t, '0' + digit(d, i));
  } else {
    put(t, '0' + digit(d, 0));
    put(t, '.');
    if (d.n == 1) put(t, '0');
    for (int i = 1; i < d.n; ++i) put(t, '0' + digit(d, i));
    put(t, 'E');
    put_int(t, exp - 1);
  }
  return t.n;
}

// str(int(v)) for a long column: truncation toward zero, exact for |v| < 2^63;
// 0 = deferred (NaN, +-Infinity, |v| >= 2^63: the host raises or prints).
CSVD_HD int csvd_long(double v, csvd::Text& t) {
  using namespace csvd;
  t = Text();
  if (!(v > -9223372036854775808.0 && v < 9223372036854775808.0)) return 0;
  const int64_t i = (int64_t)v;
  if (i == 0) {
    put(t, '0');
    return 1;
  }
  if (i < 0) put(t, '-');
  Digits d;
  digits_of_u64(i < 0 ? (uint64_t)0 - (uint64_t)i : (uint64_t)i, d, false);
  for (int k = 0; k < d.n; ++k) put(t, '0' + digit(d, k));
  return t.n;
}
