// groupby_pay.h — the packed event payload of the group-by's partition
// (groupby.hip builds it, place.hip reads it again) and the record of the
// partition a context holds.
#pragma once
#include <stdint.h>

namespace cdr {

constexpr int kGbMaxL = 10;  // files per bucket <= 1024

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
