// f64sum.h — what the exact F64 sums (f64sum.hip), the fused F64 assignment
// (f64_assign.hip) and the sharded programs (f64_sharded.hip) share: the
// block geometry, the binade transfers and their composition, and the host
// entry points between the three files.  The method is described at the head
// of f64sum.hip.
#pragma once

#include <cmath>

#include "cdr_internal.h"

namespace cdr {

constexpr int kFB = 256;               // rows per block
constexpr int kFMaxK = 64;             // clusters handled here (LDS state)
constexpr int kENone = -100000;        // no prediction (no member before the block)

// The summed type T: double (F64 mode) or float (the reference's float32
// runs: the same algorithm on a 24-bit significand).  MB = significand bits
// after the point; binades below kMinE are subnormal (no fixed grid): those
// blocks are re-added element by element.
template <typename T>
struct SumTraits {
  static constexpr int MB = 52;
  static constexpr int kMinE = -1022;
};
template <>
struct SumTraits<float> {
  static constexpr int MB = 23;
  static constexpr int kMinE = -126;
};

struct Xfer {
  long long d0;  // grid steps added for an even entry
  int dd;        // d1 - d0
  int flags;     // bit0 P0, bit1 P1 (exit parities), bit2 invalid, bit3 members
};

// One element x >= 0 of a (cluster, feature) sequence added to a transfer
// state (m0: grid steps for an even entry, mdd: odd - even, mfl: bit0 P0,
// bit1 P1, bit2 invalid, bit3 members) under the predicted binade e.  With
// x = mx 2^ex (integer significand), y = x / 2^(e - MB) = mx 2^-sh: q =
// mx >> sh and the rounding of the fraction from the shifted-out bits — the
// same q and fraction as ldexp / floor in fp64, in integer instructions.
// Split in two so that a thread can run the part that does not depend on
// the state (xfer_pre: q, the rounding of the fraction, validity) for a whole
// chunk of rows as independent, branch-free work before the short serial
// updates (xfer_apply) — f64_transfer was bound by the dependent latency of
// the branchy combined form at two waves per SIMD.
struct XPre {
  long long q;
  int r;  // bit0 fraction above one half, bit1 exactly one half, bit2 invalid
};
template <typename TA>
__device__ __forceinline__ XPre xfer_pre(double x, int e) {
  // In fp64 instructions: y = x 2^(MB - e) is exact (a power-of-two scale;
  // where it would underflow, y < 2^-1022 and the answer is q = 0 below one
  // half either way), q = floor(y), and the fraction y - q is exact.  The
  // integer form (shifts and masks of the significand, ~70 instructions) was
  // a large part of f64_transfer's issue time (128 -> 121 us); both forms
  // agree on every (x, e) of a 2e7-case host fuzz (tools/xfer_pre_fuzz.cpp).
  constexpr int MB = SumTraits<TA>::MB;
  const double y = ldexp(x, MB - (e < -2000 ? -2000 : e));
  const double qf = floor(y);
  const double fr = y - qf;
  const bool bad = e == kENone || e < SumTraits<TA>::kMinE || !(x >= 0.0) ||
                   !(y < (double)(1ll << (MB + 1)));
  const double hf = floor(ldexp(qf, -32));
  const unsigned hi = bad ? 0u : (unsigned)hf;
  const unsigned lo = bad ? 0u : (unsigned)fma(hf, -4294967296.0, qf);
  return XPre{(long long)(((unsigned long long)hi << 32) | lo),
              (fr > 0.5 ? 1 : 0) | (fr == 0.5 ? 2 : 0) | (bad ? 4 : 0)};
}
__device__ __forceinline__ void xfer_apply(XPre p, long long& m0, int& mdd, int& mfl) {
  const int fl = mfl | 8;
  const int p0 = fl & 1, p1 = (fl >> 1) & 1;
  const long long i0 = p.q + ((p.r & 1) ? 1 : ((p.r & 2) ? ((p0 + p.q) & 1) : 0));
  const long long i1 = p.q + ((p.r & 1) ? 1 : ((p.r & 2) ? ((p1 + p.q) & 1) : 0));
  const bool bad = p.r & 4;
  m0 += bad ? 0 : i0;
  mdd += bad ? 0 : (int)(i1 - i0);
  mfl = bad ? (fl | 4) : ((fl & ~3) | (int)((p0 + i0) & 1) | ((int)((p1 + i1) & 1) << 1));
}

// The binade of an approximate running value P (the predictions of
// f64_predict_c and of the sharded offsets): kENone when it has none.
__device__ __forceinline__ int binade_e(double P) {
  if (!(P > 0.0) || !isfinite(P)) return kENone;
  int ex;
  frexp(P, &ex);  // P in [2^(ex-1), 2^ex)
  return ex - 1;
}
// A running value that has a binade: positive and finite.  frexp of inf
// leaves no usable exponent (0 here) and (long long)ldexp(inf, .) no usable
// grid count: once a sum had overflowed, f64_walk's integer state turned the
// running inf into 2^63 2^-53 = 1024 after the group and went on adding to
// that.  An inf (or nan) running value only ever takes real additions.
__device__ __forceinline__ bool has_binade(double s) { return s > 0.0 && s < INFINITY; }

// Transfer composition: entering with parity p, A then B gives
// D_p = D^A_p + D^B_(P^A_p) and the exit parity P^B_(P^A_p).  Associative,
// so a run of blocks that stay in one binade is one transfer: as the
// addends are >= 0 the running value only grows, and when it is still in
// the binade after the whole run it was inside it after every block.
struct XferC {
  long long d0, d1;
  int p;  // bit0 P0, bit1 P1
};
__device__ __forceinline__ XferC xc_compose(const XferC& a, const XferC& b) {
  XferC r;
  const int a0 = a.p & 1, a1 = (a.p >> 1) & 1;
  r.d0 = a.d0 + (a0 ? b.d1 : b.d0);
  r.d1 = a.d1 + (a1 ? b.d1 : b.d0);
  r.p = ((b.p >> a0) & 1) | (((b.p >> a1) & 1) << 1);
  return r;
}

// A group of 64 blocks' composed transfer (f64_group), read by f64_walk and
// by the sharded programs (f64s_program).
struct GXfer {
  long long d0, d1;
  int e;
  int p;  // bit0 P0, bit1 P1, bit2 usable, bit3 any member
};

// One shard of sharded rows (f64_sharded.hip): the earlier shards'
// approximate sums (off, k d), the predicted binade at this shard's end
// (Eend, k d; null: no crossing condition), and either the walk from the
// exact entry state `entry` (null: the sequences start here) or no walk (the
// ranks that build programs from the transfers and group compositions
// instead).  The default is the whole, unsharded row range.
struct F64Shard {
  const double* off = nullptr;
  const int* Eend = nullptr;
  const double* entry = nullptr;
  bool walk = true;
};

// The transfer cache of a device F64 run (f64_step_fused, tcache != 0): the
// assignment's per-block label-change flags, the per-block stamps of moved
// predictions, this step's stamp, whether every block is formed, the list and
// its counter pair.
struct F64TCache {
  const int* dlab = nullptr;
  int* dE = nullptr;
  int stamp = 0;
  int all = 1;
  int* list = nullptr;
  int* counters = nullptr;
  int par = 0;
};

// f64sum.hip: after a block pass over c.x64 left the block sums and counts in
// c.f64x_A / c.f64x_cnt (f64_assign_block): the binade predictions, the
// transfers under them (tc: only the cache's dirty blocks), the group
// compositions and, with sh.walk, the walk into d_sums (k d; with sh.entry
// the exit state after them).  d_counts non-null: the clusters' member counts.
void enqueue_f64_sums_after_block(Ctx& c, int k, double* d_sums, const F64Shard& sh,
                                  unsigned long long* d_counts, const F64TCache* tc);

// f64_assign.hip: the step's screen table (f64_cent_prep<D>) and the fused
// assignment and block pass (f64_assign_block<D>), 2 <= c.d <= 16 and
// k <= kFMaxK: labels, c.f64x_A, c.f64x_cnt.  gate (device, may be null): a
// zero there skips the assignment; dlab (may be null): per block, whether
// any of its labels changed.
void enqueue_f64_assign(Ctx& c, int k, const double* dC, const long long* gate, int* dlab);

}  // namespace cdr
