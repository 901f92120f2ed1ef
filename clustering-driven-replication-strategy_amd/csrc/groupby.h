// groupby.h — what the three files of the hand-written group-by share:
// groupby.hip (the layout choice), groupby_part.hip (the partition of the
// events by file id) and groupby_bucket.hip (the per-bucket counting).  The
// payload itself is groupby_pay.h.
#pragma once

#include "cdr_internal.h"

namespace cdr {

constexpr int kGbTile = 8192;          // events per partition tile
constexpr int kGbMaxDigit = 9;         // bits per partition pass
constexpr int kGbMaxBins = 1 << kGbMaxDigit;
constexpr int kGbLdsCap = 3072;        // events per hash bucket in LDS (load <= 3/4)
constexpr int kGbDenseBits = 12;       // dense grid: 2^(L + sbits) <= 2^12 u16 counts
constexpr int kGbDenseCap = 65535;     // events per dense bucket (u16 counts)
constexpr int kGwMaxL = 8;             // wave-per-bucket kernels: 2^L <= 256 files

// What groupby_resident chose for one run.
struct GbLayout {
  int fbits;         // bits of a file id
  int B1, B2, B3;    // digit bits of the partition passes (B2, B3: 0 = no such pass)
  bool dense;        // (file, second) grid instead of the hash
  int pbytes;        // 4 or 8 bytes per payload
  GbPay p;           // (p.L: file-local bits)
};

// c.gb_small: bucket bases of pass 1 (kGbMaxBins + 1), pass-2 tile starts
// (kGbMaxBins + 1), then the bucket kernels' count of buckets over capacity.
inline int* gb_tile2start(Ctx& c) { return c.gb_small.as<int>() + kGbMaxBins + 1; }
inline int* gb_big_count(Ctx& c) { return c.gb_small.as<int>() + 2 * (kGbMaxBins + 1); }

// groupby_part.hip.  gb_count: pass 1's histograms and scans over the resident
// events; res = {ts min, ts max, any null ts, pass-2 tiles, valid events}
// (the payload layout depends on the timestamp range, so the host reads it
// before gb_partition).  gb_partition: passes 1..3 under the layout; returns
// the payloads in bucket order and sets bbase to the nb + 1 bucket bases.
void gb_count(Ctx& c, int64_t ne, int64_t nf, int fbits, int B1, long long res[5]);
const void* gb_partition(Ctx& c, int64_t ne, int64_t nf, const GbLayout& lay,
                         const long long res[5], const unsigned** bbase);

// groupby_bucket.hip: the (files, 6) rows into c.ev_out from the partition;
// picks the bucket kernel, redoes buckets over capacity with the hash in
// global memory (the host reads their number back, so the stream is
// synchronised once).  Returns that number and sets grid to the persistent
// kernel's workgroups.  Records profile mark 2.
int gb_buckets(Ctx& c, const void* pay, const unsigned* bbase, int64_t nb, int64_t nf,
               const GbLayout& lay, int64_t nvalid, int64_t* grid);

}  // namespace cdr
