// screen_big.h — what the files of the large-k Lloyd step share (overview at
// the head of screen_big.hip): the vector types, the kernels' argument struct,
// the centroid order of a block, the plan buffer's layout, and the host entry
// points between the files.
//   screen_big_plan.hip  the plan (fragments, C operand, thresholds), host and device
//   screen_big_l1.hip    L1: the fp16 copy of the points and the MFMA screen
//   screen_big_l2.hip    L2 candidates and L3 exact
//   screen_big_sums.hip  the sums: full pass or DELTA fix-up
//   screen_big.hip       the step's driver
#pragma once

#include <cstddef>
#include <cstdint>

#include "cdr_internal.h"

namespace cdr {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

// L1's arguments; L2 takes a copy whose in_* name L1's regions.
struct BigArgs {
  const h8* XB;        // fp16 B fragments per 64-point group (big_frag_copy)
  int64_t n, n_pad;
  int d, k, Q, KB;      // Q = stored feature quads, KB = ceil(k / 32)
  const h8* frag;       // A fragments [KB][DQ][64] (big_frag_lane)
  const float* cinit;   // [KB * 32] C operand per centroid row (1e30 past k)
  float thr0, thr_rel;
  const float* thr_dev;   // device plan: {thr0, thr_rel} in device memory (else the values above)
  const long long* gate;  // device loop state: nothing runs once gate[0] == 0
  unsigned jkeep;       // bits of a keyed value kept when its block is merged
  // DELTA steps (labels of the previous large-k step in place): a label is
  // written only when it changes, and the change {pt, old << 16 | new} goes
  // to L1's per-wave regions (mv1, same capacity as out_list) or, from L2 /
  // L3, to the flat list mv2 (count at mv2_count)
  int delta;
  int2* mv1;
  int32_t* mv1_count;
  int2* mv2;
  int32_t* mv2_count;
  const float* XA;      // the points row-major [n_pad][d4] (ensure_rowmajor)
  int d4;
  int32_t* labels;
  // L2's input: L1's per-wave regions (null / 0 in L1's own copy)
  const int32_t* in_list;
  const int32_t* in_count;
  int in_cap, in_regions;
  // uncertified output: one region of out_cap entries per wave
  int32_t* out_list;
  float* out_best;     // L1: the point's best screen value (truncated key), same slots
  int32_t* out_count;  // [nwaves + 1]: per-wave counts, then the total
  int out_cap;
};

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  h2 h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}

// Centroid order inside a 32-row block: MFMA row r (the A-operand row of lane
// r and r + 32) holds centroid 32 b + big_row(r), chosen so that output value
// i of lane half h (row 8 (i >> 2) + 4 h + (i & 3)) is centroid 32 b + 16 h + i:
// a lane's keyed top-2 then carries the centroid's low bits directly.
__host__ __device__ inline int big_row(int r) { return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3); }

constexpr int kMaxCand = 16;       // candidates per point L2 evaluates; more go to L3
constexpr int kMaxRegions = 8192;  // L1 waves (regions) the candidate level can index

// DQ: 16-feature K chunks (d <= 16 DQ), the kernels' template argument.
inline int big_dq(int d) { return (d + 15) / 16; }

// L1's keys keep the centroid index in their low JB bits: 5 for the row of a
// block, the rest for the block (screen_big_sp; thr_rel follows from it).
__host__ __device__ inline int big_jbits(int KB) {
  int JB = 5;
  while ((1 << (JB - 5)) < KB) ++JB;
  return JB;
}

// LDS of L1: the C operand rows and the A fragments of all k centroids.
inline size_t big_l1_lds(int k, int d) {
  const int KB = (k + 31) / 32;
  return (size_t)KB * 32 * 4 + (size_t)KB * big_dq(d) * 64 * 16;
}

// Plan buffer (c.frag): frag1 | cinit | C (fp64) | {thr1, thr_rel}.
struct BigLayout {
  size_t b1, bc, bC, bt;       // bytes of the four parts
  size_t o_cinit, o_C, o_thr;  // their offsets (frag1 at 0)
  size_t used, all;            // end of the thresholds; the allocation (16-byte multiple)
};
inline BigLayout big_layout(int k, int d) {
  const int DQ = big_dq(d), KB = (k + 31) / 32;
  BigLayout l;
  l.b1 = (size_t)KB * DQ * 64 * sizeof(h8);
  l.bc = (size_t)KB * 32 * sizeof(float);
  l.bC = sizeof(double) * (size_t)k * d;
  l.bt = 16;
  l.o_cinit = l.b1;
  l.o_C = l.o_cinit + l.bc;
  l.o_thr = l.o_C + l.bC;
  l.used = l.o_thr + l.bt;
  l.all = (l.used + 15) / 16 * 16;
  return l;
}

// screen_big_plan.hip: the host plan of centroids C built and uploaded into
// c.frag (enqueued); thr = {thr1, thr_rel}, which a host plan passes by value.
void big_plan_host(Ctx& c, const double* C, int k, float thr[2]);

// screen_big_l1.hip.  big_sp_threads: L1's workgroup size.  big_ensure_xb:
// the fp16 copy of the points (c.xb16), built if it is not there.
// big_launch_l1: L1 on nwg workgroups.
int big_sp_threads(int DQ);
const h8* big_ensure_xb(Ctx& c);
void big_launch_l1(Ctx& c, const BigArgs& a, int nwg);

// screen_big_l2.hip: L2 on L1's regions (a2.in_*), in the form that fits the
// LDS (c.big_info[5]), then L3 on L2's overflow list; dC = the fp64 centroids,
// chunk_pre = in_regions + 1 words for the LDS form's chunk numbering.
void big_launch_l2_l3(Ctx& c, const BigArgs& a2, const double* dC, int32_t* ovf,
                      int32_t* ovf_count, int32_t* chunk_pre);

// screen_big_sums.hip.  big_fg: features per pass of the sums' LDS table (0:
// k too large).  big_launch_sums: the (k, d+1) int64 sums bs of the labels,
// by a full pass or, on a DELTA step, from the moves of a2 (regions in_*).
int big_fg(int k);
void big_launch_sums(Ctx& c, const BigArgs& a2, unsigned long long* bs);

}  // namespace cdr
