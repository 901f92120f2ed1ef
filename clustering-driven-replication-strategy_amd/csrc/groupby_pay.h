// groupby_pay.h — the packed event payload of the group-by's partition: its
// layout, the one encoder (gb_make, groupby_part.hip's pass 1) and the one
// decoder (gb_decode: the bucket kernels of groupby_bucket.hip and
// place.hip's place_bucket), and the record of the partition a context holds.
#pragma once
#include <limits.h>
#include <stdint.h>

namespace cdr {

constexpr int kGbMaxL = 10;  // files per bucket <= 1024
constexpr long long kTsNullG = LLONG_MIN;

// Payload layout (host-computed, passed by value):
// [file low bits | second code | op | client code].
struct GbPay {
  int fshift;   // bit position of the file-low field
  int sshift;   // bit position of the second code (= 2 + cbits)
  int cbits;    // client code bits (code 0 = not a node id, else client + 1)
  int sbits;    // second code bits (all ones = null)
  int L;        // file-local bits (files per bucket = 2^L)
  long long sec_min;
  unsigned long long low_mask;  // file-low field mask (fbits - B1 bits)
};

__device__ __forceinline__ long long sec_of_g(long long ts_us) {
  // Spark floor(cast(ts as double)); see features.hip sec_of
  if (ts_us >= 0 && ts_us < 9000000000000000ll) return ts_us / 1000000;
  return (long long)floor((double)ts_us / 1000000.0);
}

template <typename T>
__device__ __forceinline__ T gb_make(const GbPay& p, unsigned flow, long long ts, uint8_t op,
                                     int client) {
  const unsigned long long sc = ts == kTsNullG ? ((1ull << p.sbits) - 1)
                                               : (unsigned long long)(sec_of_g(ts) - p.sec_min);
  const unsigned long long oc = op == 1 ? 1ull : (op == 2 ? 2ull : 0ull);
  const unsigned long long cc = client >= 0 ? (unsigned long long)client + 1ull : 0ull;
  return (T)(((unsigned long long)flow << p.fshift) | (sc << p.sshift) | (oc << p.cbits) | cc);
}

// The fields of one payload inside its bucket.
struct GbFields {
  unsigned fl;            // file-local index (the low L bits of the file field)
  unsigned long long sc;  // second code (up to 41 bits on the hash path)
  unsigned oc;            // 1 WRITE, 2 READ, 0 other
  unsigned cc;            // client code: client + 1, 0 = not a node id
};

__device__ __forceinline__ GbFields gb_decode(unsigned long long v, const GbPay& p) {
  GbFields e;
  e.fl = (unsigned)(v >> p.fshift) & ((1u << p.L) - 1);
  e.sc = (v >> p.sshift) & ((1ull << p.sbits) - 1);
  e.oc = (unsigned)(v >> p.cbits) & 3u;
  e.cc = (unsigned)(v & ((1ull << p.cbits) - 1));  // cbits reaches 32 (client 2^31 - 1)
  return e;
}

// The client id of a client code (-1 for code 0); code 2^31 is client 2^31 - 1.
__device__ __forceinline__ int gb_client(unsigned cc) { return (int)(cc - 1u); }

// The resident partition: what the last groupby_resident left in the context's
// gb_ buffers, and the events it belongs to.  Every writer of the resident
// events drops it (drop_partition, cdr_internal.h).
struct GbPartition {
  bool valid = false;
  int64_t ne = -1, nf = -1;        // the events and files it was built from
  int64_t nb = 0;                  // buckets of 2^p.L consecutive files
  const void* pay = nullptr;       // ne payloads, bucket by bucket (gb_p1 or gb_p2)
  const unsigned* bbase = nullptr; // nb + 1 bucket bases into pay
  int pbytes = 0;                  // 4 or 8 bytes per payload
  GbPay p{};
};

}  // namespace cdr
