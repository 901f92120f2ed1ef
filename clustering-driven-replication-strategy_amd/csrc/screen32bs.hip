// screen32bs.hip — the bounded screen deciding in registers (device loop;
// d <= 16, k <= 64): the headline kernel.  Its default form keeps 2-byte bound
// words (reported as screen32bs16<Q,MT>), the form
// screen32bs<Q, MT, true> decides the lists of screen32bz (screen32b.hip).
//
// Phase 1 is screen32b's (screen32b.hip has the bounds).  Phase 2 gathers the listed points' fp32
// rows (XA: one 64-byte line per point at d = 16, the same memory
// transactions as screen32b's 32-byte hi row) and decides each batch of 64
// without a queue, a list or a fixup pass:
//   * xhat32 = fma(x, 2^sigma, -mu 2^sigma) (split_copy_kernel's values) and
//     the direct test: fp32 distances to c32_a and its two
//     nearest centroids with rigorous intervals, every other centroid bounded
//     through h3_a (CDR_S32BS_DIRECT=0: the triangle test against c32_a
//     alone, E_a >= dn + ec covering ||xhat32 - xhat|| + ||c32_a - chat_a||);
//   * a few undecided lanes of a batch go to the wave's tail list as "not
//     screened" records; kDirectDense or more (and every undecided lane of
//     the split form) take the SPLIT screen of the whole batch
//     (the full screen's 2-3 MFMA per centroid tile on the hi / lo halves of
//     xhat32, formed in registers: one permlane32 swap per operand dword turns
//     the lanes' own rows into both 32-point B operands) and its
//     certificate vs > vb thr_rel + thr0, the K-case bounds from (vb, vs)
//     relative to xhat32 (|S_j - (D + ||chat_j||^2 - 2 chat_j . xhat32)| <= E
//     <= thr0 / 2), then the rounding of xhat32 (dn32 <= 2^-24 ||xhat32||);
//   * when any lane is not certified (near ties), fixup_regions' candidate set
//     (every key within the threshold of the best) evaluated in exact fp64
//     NumPy order: np.argmin of the reference's norms
//     (src/kmeans_plusplus.py:33-34); such a point keeps "no bound".
// Moves go into a per-workgroup int64 table in LDS ([k][d + 1], run_sums'
// layout) flushed into one run_sums slice at the end when the workgroup moved
// anything.  The split screen is ~2^8 tighter than the hi-only one, so almost
// no point needs the exact fp64 pass.
// SPLIT: phase 1 ran in screen32bz (same grid, so wave w decides the list of
// screen32bz's wave w and decodes its entries with the same chunk range); the
// batches come from that list, entries two batches ahead and rows one batch
// ahead of the decision.
// WATCH: phase 1 streams the wave's watch list
// (zh_watch_kernel, screen32b.hip: the points whose word could fail within
// the drift budget) instead of every bound word; the rest is the default
// form's code, and a new word goes to the point's entry too.  The list's count
// and first loads go out with the plan's loads, and a tail record carries the
// point's offset beside the entry's slot.
// The forms are one text, screen32bs_body.h, included into the kernels here:
// screen32bs<Q, MT, SPLIT, WATCH> holds one form; screen32bsw<Q, MT>, the
// list path's one launch per step, reads the mode word once and runs the WATCH
// or the default form on one set of LDS arrays (<4,1>, which does not fit one
// kernel's registers, keeps a launch per form).
#include "screen32_common.h"
#include "screen32_fix.h"

namespace cdr {

#ifndef CDR_S32BS_DEPTH
#define CDR_S32BS_DEPTH 2  // gathered batches in flight in screen32bs's phase 2 (experiments: 3)
#endif
#ifndef CDR_S32BS_LAZY
#define CDR_S32BS_LAZY 1  // screen32bs: phase 2 interleaved with the stream (0: in bursts)
#endif

#ifndef CDR_S32BS_DENSE
#define CDR_S32BS_DENSE 8  // kDirectDense (A/B at config 3: 4, 8, 16)
#endif
// A gathered batch with at least this many lanes the direct test leaves
// undecided takes the in-batch split screen; with fewer, those lanes go to
// the wave's tail list as "not screened" records
constexpr int kDirectDense = CDR_S32BS_DENSE;
// ... whose key no screen produces: the keys are fp32 bit patterns with the
// low 6 bits cleared, and a NaN grown from fp16 operands has mantissa bits
// 6-12 clear
constexpr unsigned kNotScreened = 0xFFFFFFC0u;

// The workgroup's LDS, declared once per kernel: the two forms of screen32bsw
// share it (two sets would be ~79 KB and halve the occupancy).
// flist, per wave: points whose bound failed (screen32b's entries); room for
// the kBPD chunks streamed between two phase-2 passes, so phase 2 has one call
// site (code size: the decision is inlined once)
constexpr int kSList = kBPD * kBChunk + 256;
#define S32BS_LDS                                                                         \
  __shared__ __attribute__((aligned(16))) float c32s[64 * kPrStr + 128];                  \
  __shared__ __attribute__((aligned(16))) unsigned flist[4][SPLIT ? 1 : kSList];          \
  __shared__ unsigned long long mtab[64 * 17]; /* this workgroup's moves, [k][d + 1] */   \
  __shared__ float msl[16];                    /* -mu_f 2^sigma */                        \
  __shared__ unsigned tls[64];                 /* 2-byte words: the code thresholds */    \
  __shared__ h8 sA[MT * 2 * 64];               /* the plan */                             \
  __shared__ __attribute__((aligned(16))) float sC[MT * 4 * 2 * 4];

// One form in a kernel of its own: the default form (and, SPLIT, the form
// deciding screen32bz's lists).  With a watch list in the arguments a form
// runs only while the mode word asks for it; the list path launches
// screen32bsw instead, except where kS32bsMerged says otherwise: there the
// WATCH form is launched beside the default form, each gated on the mode word.
template <int Q, int MT, bool SPLIT = false, bool WATCH = false>
__global__ __launch_bounds__(256, 4) void screen32bs(S32BArgs B) {
  constexpr bool MERGED = false;
  S32BS_LDS
#include "screen32bs_body.h"
}


// The list path's one launch per step (B.watch != null): the
// mode word is read once and picks the body - WATCH on kWatchList with no
// overflowed region, the default form otherwise.
template <int Q, int MT>
__global__ __launch_bounds__(256, 4) void screen32bsw(S32BArgs B) {
  constexpr bool SPLIT = false, MERGED = true;
  S32BS_LDS
  if (B.dyn && blockIdx.x == 0 && threadIdx.x < 32)
    B.dyn[((B.dyn_par ^ 1) * 32 + threadIdx.x) * 32] = 0u;
  if (B.p.gate && B.p.gate[0] == 0) return;
  const bool list = B.watch[kWMode] == kWatchList && B.watch[kWOvf] == 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (cdr_lloyd_watch_info)
    B.watch[list ? kWListN : kWFullN] += 1;
    B.watch[kWLast] = list ? kWatchList : kWatchFull;
  }
  if (list) {
    constexpr bool WATCH = true;
#include "screen32bs_body.h"
  } else {
    constexpr bool WATCH = false;
#include "screen32bs_body.h"
  }
}

// screen32bsw<4,1> does not fit the 128 VGPRs of four workgroups per CU (the
// compiler spills one register to scratch), so that shape alone keeps a launch
// per form, which fit.
#ifndef CDR_S32BS_MERGE
#define CDR_S32BS_MERGE 1  // (A/B: 0 keeps a launch per form for every shape)
#endif
template <int Q, int MT>
constexpr bool kS32bsMerged = CDR_S32BS_MERGE && !(Q == 4 && MT == 1);

// (the occupancy of the kernel the fused path launches - list: screen32bsw, or
// the WATCH form's own kernel; the split form runs on the default form's grid)
int screen32bs_blocks_per_cu(int Q, int MT, bool list) {
  static int cache[2][4][2] = {};
  int& nb = cache[list][Q - 1][MT - 1];
  if (!nb)
    dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
      constexpr int Q_ = decltype(q)::value, MT_ = decltype(m)::value;
      if (!list) nb = occupancy_blocks(screen32bs<Q_, MT_>, 0);
      else if constexpr (kS32bsMerged<Q_, MT_>) nb = occupancy_blocks(screen32bsw<Q_, MT_>, 0);
      else nb = occupancy_blocks(screen32bs<Q_, MT_, false, true>, 0);
    });
  return nb;
}

void screen32bs_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32BArgs& p, bool split) {
  // (the bodies of screen32bsw are told that the first Q - 1 feature quads are
  // all real features)
  if (p.p.d <= 4 * (Q - 1) || p.p.d > 4 * Q) CDR_FAIL(CDR_ERR_STATE, "screen32bs: Q is not d4_of(d) / 4");
  if (split && p.watch) CDR_FAIL(CDR_ERR_STATE, "screen32bs: a watch list with the split form");
  dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
    constexpr int Q_ = decltype(q)::value, MT_ = decltype(m)::value;
    if (split) {
      hipLaunchKernelGGL((screen32bs<Q_, MT_, true>), grid, dim3(256), 0, s, p);
    } else if (!p.watch) {
      hipLaunchKernelGGL((screen32bs<Q_, MT_>), grid, dim3(256), 0, s, p);
    } else if constexpr (kS32bsMerged<Q_, MT_>) {
      hipLaunchKernelGGL((screen32bsw<Q_, MT_>), grid, dim3(256), 0, s, p);
    } else {  // (each gated on the mode word; one exits at once)
      hipLaunchKernelGGL((screen32bs<Q_, MT_, false, true>), grid, dim3(256), 0, s, p);
      hipLaunchKernelGGL((screen32bs<Q_, MT_>), grid, dim3(256), 0, s, p);
    }
  });
}

}  // namespace cdr
