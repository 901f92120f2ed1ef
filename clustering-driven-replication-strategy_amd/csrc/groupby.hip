// groupby.hip — the access-log group-by of src/compute_features.py:31-46 as a
// two-level MSD partition of the events by file id followed by one LDS hash
// group-by per bucket of 2^L consecutive files.  No library sort.
//
// Per event the counters are (:31-42) count, WRITE, READ, local (client ==
// primary node of its file); max_concurrency (:44-46) is the largest count of
// one (file, second) pair, the null second (unparseable timestamp) being a
// pair of its own.  All of them are order-independent sums and maxima, so the
// partition may place events of one bucket in any order.
//
//   K1  gb_hist1    per 8192-event tile: histogram of the pass-1 digit (the
//                   top B1 bits of the file id), in-chunk prefix per tile;
//                   timestamp min / max / null flag (file 4 B + ts 8 B read)
//   S1  gb_scan1    chunk bases, digit bases, pass-2 tile starts, ts range
//   --- host reads the ts range (the payload layout depends on it) ---
//   P1  gb_scatter1 tile -> LDS-ranked by digit -> coalesced runs into the
//                   digit regions; builds the packed payload
//                   [file low bits | second code | op | client code]
//                   (17 B read, 4 or 8 B written)
//   H2  gb_hist2    per pass-2 tile (a slice of one digit region): histogram
//                   of the pass-2 digit (payload read)
//   S2  gb_scan2    one workgroup per pass-1 digit: tile offsets and bucket
//                   bases
//   P2  gb_scatter2 like P1 within each digit region (payload read + written)
//   K4  gb_bucket   one workgroup per bucket: LDS hash of (file, second) ->
//                   count (one 64-bit slot = key << CB | count), per-file
//                   count / write / read / local sums and the concurrency
//                   maximum in LDS, then the (files, 6) int64 rows; buckets
//                   over the LDS capacity are listed and redone by
//                   gb_bucket_big with the hash in global memory.  A small
//                   (file, second) range takes a dense grid of counts instead
//                   (gb_bucket_dense / _wave / _wave4).
// With B <= 9 bucket bits one partition pass suffices (H2/S2/P2 skipped); a
// third pass repeats H2 / S2 / P2 over pass 2's regions.
//
// This file chooses the layout (groupby_resident).  K1..P2 are
// groupby_part.hip, K4 is groupby_bucket.hip, the payload groupby_pay.h.
#include <algorithm>
#include <cmath>

#include "groupby.h"

namespace cdr {

namespace {

int bitlen(unsigned long long v) {  // bits to hold v (0 -> 0)
  int b = 0;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

}  // namespace

// The group-by of the events resident in c.ev_* (features_aggregate_resident's
// hand-written path).  Returns false (nothing computed) when the shape is
// outside what the packed payload and bucket tables can hold; the caller then
// takes the sort-based path.
//
// Layout: fbits = bits of the file id; the top B1 = min(9, fbits) bits are the
// pass-1 digit; the remaining rem bits split into the pass-2 digit (B2 <= 9)
// and the file-local bits L (2^L files per bucket), chosen once the second
// range is known: the dense (file, second) grid when 2^(L + sbits) <= 4096,
// else the hash with about 1024 events per bucket.
bool groupby_resident(Ctx& c, int64_t ne, int64_t nf, int64_t* out, int64_t* max_ts) {
  c.gb_last_hand = 0;
  c.gb_part_rec.valid = false;  // the gb_ buffers are rewritten (or the sort-based path runs)
  if (nf < 1 || ne < 0 || ne >= (1ll << 31) || nf >= (1ll << 31)) return false;
  if (getenv("CDR_GROUPBY_SORT")) return false;  // the sort-based path, for comparisons
  const int cmax = c.ev_cmax;
  const int cbits = std::max(1, bitlen((unsigned long long)std::max(cmax, 0) + 1));
  const int fbits = bitlen((unsigned long long)(nf - 1));
  const int B1 = std::min(kGbMaxDigit, fbits);
  const int rem = fbits - B1;
  const int Lmin = std::max(0, rem - kGbMaxDigit), Lmax = std::min(rem, kGbMaxL);
  if (Lmin > Lmax) return false;
  c.ev_out.ensure(8 * 6 * (size_t)nf + 64);
  // profiling: events 0 (start), 1 (partition done), 2 (buckets done)
  prof_step_begin(c);
  prof_mark(c, 0);
  long long res[5];  // K1 + S1: ts min, max, any null, pass-2 tiles, valid events
  gb_count(c, ne, nf, fbits, B1, res);
  // payload layout from the timestamp range
  *max_ts = LLONG_MIN;
  long long sec_min = 0, sec_max = 0;
  if (ne > 0 && res[0] <= res[1]) {
    *max_ts = res[1];
    sec_min = (long long)std::floor((double)res[0] / 1000000.0);
    sec_max = (long long)std::floor((double)res[1] / 1000000.0);
  }
  if (sec_max - sec_min >= (1ll << 40)) {
    prof_drop(c);
    return false;
  }
  const int sbits = std::max(1, bitlen((unsigned long long)(sec_max - sec_min) + 1));
  const double a = (double)std::max<int64_t>(res[4], 1) / (double)nf;  // events per file
  // the bucket shape from the smallest file-local width the passes allow
  auto shape = [&](int lmin, bool& dn) -> int {
    dn = sbits + lmin <= kGbDenseBits && !exp_env("CDR_GB_HASH");
    if (dn) {
      const int Lt = (int)std::floor(std::log2(2048.0 / a));
      return std::max(lmin, std::min({Lt, Lmax, kGbDenseBits - sbits}));
    }
    const int Lt = (int)std::floor(std::log2(1024.0 / a));
    return std::max(lmin, std::min(Lt, Lmax));
  };
  bool dense;
  int L = shape(Lmin, dense);
  int B2 = rem - L, B3 = 0;
  // Two passes leave buckets over the LDS tables (about 3 million files and
  // more: the one-GPU 1B-event log's 5.95M files gave 32-file buckets of ~5400
  // events, every one through the global-memory hash): a third pass
  // (9 + 9 + B3 bits) brings the buckets back to the LDS shapes.
  // (CDR_GB_PASS3=1, tests: the third pass whenever the file bits allow it)
  const bool force3 = getenv("CDR_GB_PASS3") != nullptr;
  if (rem > kGbMaxDigit && (a * std::ldexp(1.0, L) > 0.5 * kGbLdsCap || force3)) {
    bool dn3;
    const int lmin3 = std::max(0, rem - 2 * kGbMaxDigit);
    int L3 = shape(lmin3, dn3);
    if (force3) L3 = std::max(lmin3, std::min(L3, rem - kGbMaxDigit - 1));
    if (rem - kGbMaxDigit - L3 >= 1 && L3 < L) {
      L = L3;
      dense = dn3;
      B2 = kGbMaxDigit;
      B3 = rem - kGbMaxDigit - L;
    }
  }
  if (!dense && L + sbits > 40) {  // hash key + count in 64 bits
    prof_drop(c);
    return false;
  }
  GbPay p;
  p.cbits = cbits;
  p.sshift = 2 + cbits;
  p.sbits = sbits;
  p.fshift = p.sshift + sbits;
  p.L = L;
  p.sec_min = sec_min;
  const int lowbits = fbits - B1;
  p.low_mask = lowbits >= 64 ? ~0ull : ((1ull << lowbits) - 1);
  const int pbits = p.fshift + lowbits;
  if (pbits > 64) {
    prof_drop(c);
    return false;
  }
  const GbLayout lay = {fbits, B1, B2, B3, dense, pbits <= 32 ? 4 : 8, p};
  const int64_t nb = ceil_div(nf, (int64_t)1 << L);
  c.gb_last_hand = 1;
  c.gb_last_L = L;
  c.gb_last_passes = B3 > 0 ? 3 : (B2 > 0 ? 2 : 1);
  c.gb_last_pbytes = lay.pbytes;
  c.gb_last_dense = dense ? 1 : 0;
  const unsigned* bbase = nullptr;
  const void* pay = gb_partition(c, ne, nf, lay, res, &bbase);
  prof_mark(c, 1);  // partition done
  c.gb_last_big = gb_buckets(c, pay, bbase, nb, nf, lay, res[4], &c.gb_last_grid);
  // the partition stays resident for place.hip
  c.gb_part_rec.valid = true;
  c.gb_part_rec.ne = ne;
  c.gb_part_rec.nf = nf;
  c.gb_part_rec.nb = nb;
  c.gb_part_rec.pay = pay;
  c.gb_part_rec.bbase = bbase;
  c.gb_part_rec.pbytes = lay.pbytes;
  c.gb_part_rec.p = p;
  if (out)
    HIP_CHECK(hipMemcpyAsync(out, c.ev_out.p, 8 * 6 * nf, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  return true;
}

}  // namespace cdr
