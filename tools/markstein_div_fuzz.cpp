// Host fuzz: fl(a / S) against Markstein's q0 = fl(a y), fl(q0 + fma(-q0, S, a) y), y = fl(1 / S)
// (csrc/seed_scan.hip seg_block_kernel).
//   g++ -O2 -ffp-contract=off -o /tmp/mk tools/markstein_div_fuzz.cpp
//   /tmp/mk                      random significands (3.2e8 quotients)
//   /tmp/mk midpoint [seed [n]]  quotients next to rounding midpoints (n draws, default 4e8)
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <random>
#include <cstdint>
static inline double mk(double a, double S, double y) {
  const double q0 = a * y;
  const double r = std::fma(-q0, S, a);
  return std::fma(r, y, q0);
}
// Quotients next to rounding midpoints: random significands almost never land there, and a
// q0 that is 1.5 ulp off could round the wrong way after one correction.  A 54-bit odd M is
// the midpoint of two neighbouring 53-bit significands.  Cutting a product M s to 53 bits
// would move the quotient by up to an ulp, so a is built exactly: a 2^sh = M s + delta with
// delta = +-1, +-3, +-5, +-7, which puts a / S at M + delta / s, |delta| 2^-52 half-ulps
// from the midpoint, on either side.  With s odd that needs M = -delta / s (mod 2^sh): either
// the divisor is drawn (random, all ones and within 8 ulps of it, just above a power of two)
// and M solved for, or M is drawn (random, quotient significand just above 1, just below 2)
// and s solved for; draws whose solution is not a 54-bit M / 53-bit s / 53-bit a are skipped.
static uint64_t inv64(uint64_t x) {  // x odd: 1 / x mod 2^64 (Newton, 3 -> 96 bits)
  uint64_t r = x * 3 ^ 2;
  for (int i = 0; i < 5; ++i) r *= 2 - x * r;
  return r;
}
static int midpoint_mode(uint64_t seed, long long iters) {
  std::mt19937_64 g(seed);
  long long n = 0, bad = 0, q0bad = 0;
  const uint64_t top = 1ull << 53, half = 1ull << 52;
  for (long long it = 0; it < iters; ++it) {
    const int sh = 53 + (int)(g() & 1);  // M s in [2^105, 2^107)
    const uint64_t mask = (1ull << sh) - 1;
    const long long delta = (long long)(1 + 2 * (g() & 3)) * ((g() & 1) ? 1 : -1);
    uint64_t s, M;
    const int cls = (int)(it % 3);
    if (it & 8) {  // the divisor drawn, M solved for
      s = half | (g() & (half - 1)) | 1ull;
      if (cls == 1) s = top - 1 - 2 * (g() & 7);    // all ones, or within 8 ulps of it (odd)
      if (cls == 2) s = half + 1 + 2 * (g() & 0x7F);
      M = (uint64_t)(-delta) * inv64(s) & mask;
      if (sh == 53) M |= top;
    } else {  // the midpoint drawn, s solved for
      M = top | (g() & (top - 1)) | 1ull;
      if (cls == 1) M = top + 1 + 2 * (g() & 0xFF);      // quotient significand near 1
      if (cls == 2) M = 2 * top - 1 - 2 * (g() & 0xFF);  // ... near 2
      s = (uint64_t)(-delta) * inv64(M) & mask;
    }
    if (M < top || M >= 2 * top || s < half || s >= top) continue;
    const __int128 P = (__int128)M * s + delta;
    if ((uint64_t)P & mask) { printf("construction error\n"); return 2; }
    const uint64_t ai = (uint64_t)(P >> sh);
    if (ai < half || ai >= top) continue;
    const int es = (int)(g() % 200) - 60 - 52;  // S = s 2^es in [2^-60, 2^140)
    const int j = (int)(g() % 120);             // q = (M + delta / s) 2^(-54 - j) < 2^-j
    const double S = std::ldexp((double)s, es);
    const double y = 1.0 / S;
    const double a = std::ldexp((double)ai, es + sh - 54 - j);
    if (!(a >= std::ldexp(1.0, -960)) || a > S) continue;
    const double q1 = a / S, q2 = mk(a, S, y);
    ++n;
    if (q1 != a * y) ++q0bad;
    if (q1 != q2 && bad++ < 10) printf("a=%a S=%a div=%a mk=%a\n", a, S, q1, q2);
  }
  printf("midpoint cases %lld mismatches %lld (uncorrected q0 differs in %lld)\n", n, bad, q0bad);
  return bad ? 1 : 0;
}
int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "midpoint"))
    return midpoint_mode(argc > 2 ? strtoull(argv[2], nullptr, 0) : 7,
                         argc > 3 ? atoll(argv[3]) : 400000000);
  std::mt19937_64 g(7);
  long long n = 0, bad = 0;
  auto rnd_sig = [&](int mode) -> double {
    uint64_t m = g() & 0xFFFFFFFFFFFFFull;
    if (mode == 1) m = 0xFFFFFFFFFFFFFull - (g() & 0xFF);
    if (mode == 2) m = g() & 0xFF;
    if (mode == 3) m = (g() & 1) ? 0x8000000000000ull ^ (g() & 0xFFF) : 0x7FFFFFFFFFFFFull - (g() & 0xFFF);
    uint64_t bits = (1023ull << 52) | m;
    double x; memcpy(&x, &bits, 8); return x;  // [1, 2)
  };
  for (long long it = 0; it < 40000000; ++it) {
    const double S = std::ldexp(rnd_sig((int)(it % 4)), (int)(g() % 200) - 60);
    const double y = 1.0 / S;
    for (int t = 0; t < 8; ++t) {
      double a;
      int mode = (int)(g() % 4);
      a = std::ldexp(rnd_sig(mode), -(int)(g() % 120)) * S;  // a <= ~S
      a = std::nextafter(a, (g() & 1) ? 0.0 : INFINITY);
      if (a > S) a = S;
      if (g() % 16 == 0) a = S;
      if (!(a >= std::ldexp(1.0, -960))) continue;
      const double q1 = a / S, q2 = mk(a, S, y);
      ++n;
      if (q1 != q2 && bad++ < 10) printf("a=%a S=%a div=%a mk=%a\n", a, S, q1, q2);
    }
  }
  printf("cases %lld mismatches %lld\n", n, bad);
}
