// screen_big.hip — Lloyd step for the large-k / large-d regime (BASELINE
// config 5: 50M x d=64, k=1024), reference src/kmeans_plusplus.py:33-41.
// This file is the step's driver; the levels are in screen_big_plan.hip,
// screen_big_l1.hip, screen_big_l2.hip and screen_big_sums.hip, what they
// share in screen_big.h.
//
// At k*d this large the distance computation is a dense contraction
// (2nkd = 6.6 TFLOP per step) and belongs on the matrix cores; the update
// table k x (d+1) (520 KB) no longer fits a workgroup's LDS, so assign and
// update are separate passes:
//
//  L1  screen_big_sp<DQ, NT>: every point, ONE fp16 MFMA product per 32x32
//      block, S_j = fl32(C_j - 2 chi_j . xhi) with C_j = ||chat_j||^2 + D (the
//      MFMA C operand), xhat = (x - mu) 2^sigma the exact pre-centred copy,
//      xhi its fp16 copy in B-fragment order (big_frag_copy).  The
//      fp16 A fragments of all k centroids (128 KB at k = 1024, d = 64) and
//      the C operand rows sit in LDS for the whole persistent launch; a wave
//      takes 64 points (two 32-point B tiles sharing every A fragment read)
//      and issues one block's MFMAs while it reduces the block before.
//      Per 32-centroid block each lane reduces its 16 values to a keyed
//      top-2 (v_min3/v_med3 on (bits & ~15) | reg), then merges that into
//      running (best, runner-up) keys that carry the centroid index in their
//      low JB bits.  A point is certified
//      when runner > best (1 + 2^(JB-21)) + T1 (T1 = twice the rigorous bound on
//      |S_j - exact shifted distance| + the reference's rounding slack);
//      the rest go to per-wave regions.
//  L2  cand_big_lds<DQ> (fragments in LDS) or, at the largest KB, cand_big<DQ>
//      (fragments from global memory; see big_launch_l2_l3): the L1
//      leftovers, 64 per wave (chunks of L1's regions
//      numbered through a prefix): the same one-product screen is
//      recomputed and every centroid with S_j <= best (1 + 2^(JB-21)) + T1 is a
//      candidate (the exact argmin is among them); each lane then takes one
//      point and evaluates its few candidates in exact fp64 NumPy order.
//  L3  exact_big: points with more than kMaxCand candidates, one wave per
//      point in exact fp64 NumPy order over all k (8 lanes per centroid = the
//      8 pairwise accumulators, combined in NumPy's tree by shfl_xor 1, 2, 4),
//      correctly rounded sqrt, first minimum of the roots (np.argmin of
//      np.linalg.norm).
//  U   update_big<FG>: sums per (cluster, feature) from the labels, in passes
//      of FG features: one workgroup per CU holds an LDS table [FG][k] of
//      fp64 sums (exact: grid values) fed by ds_add_f64, then adds its table
//      as exact int64 fixed point into the (k, d+1) output with atomics.
//      DELTA steps (the labels of the previous large-k step in place) apply
//      only the moves the levels recorded: fixup_big<FG>.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "screen_big.h"

namespace cdr {

void ensure_precentered(Ctx& c);
void ensure_rowmajor(Ctx& c);

bool big_supported(const Ctx& c, int k) {
  return c.mode == CDR_MODE_F32X && c.pre_ok && c.d >= 8 && c.d <= 64 && k >= 1 &&
         big_l1_lds(k, c.d) <= 150 * 1024 && big_fg(k) > 0;
}

static bool big_launch(Ctx& c, int k, float thr1, float thr_rel, const float* thr_dev,
                       const long long* gate, long long* dout, bool prof);

// One F32X Lloyd step in the large regime: labels for every point and the
// exact int64 (k, d+1) sums/counts in dout (device).  Returns false when the
// shape is not covered (nothing launched).
bool big_step(Ctx& c, const double* C, int k, long long* dout, bool prof) {
  if (!big_supported(c, k)) return false;
  ensure_precentered(c);
  float thr[2];
  big_plan_host(c, C, k, thr);
  return big_launch(c, k, thr[0], thr[1], nullptr, nullptr, dout, prof);
}

// One step on the device plan in c.frag (big_plan_device; no host round
// trip); gate = the loop state.
bool big_step_dev(Ctx& c, int k, long long* dout, bool prof, const long long* gate) {
  if (!big_supported(c, k)) return false;
  ensure_precentered(c);
  const float* thr = reinterpret_cast<const float*>(static_cast<char*>(c.frag.p) +
                                                    big_layout(k, c.d).o_thr);
  return big_launch(c, k, 0.0f, 0.0f, thr, gate, dout, prof);
}

static bool big_launch(Ctx& c, int k, float thr1, float thr_rel, const float* thr_dev,
                       const long long* gate, long long* dout, bool prof) {
  const int d = c.d, DQ = big_dq(d), KB = (k + 31) / 32, JB = big_jbits(KB);
  const int cus = lloyd_num_cus(c.device);
  const BigLayout L = big_layout(k, d);
  char* dp = static_cast<char*>(c.frag.p);
  const double* dC = reinterpret_cast<const double*>(dp + L.o_C);

  // level 1: persistent, one workgroup per CU (LDS-bound)
  const int64_t groups = (c.n + 63) / 64;
  const int wpb1 = big_sp_threads(DQ) / 64;
  const int nwg1 = (int)std::max<int64_t>(1, std::min<int64_t>(cus, (groups + wpb1 - 1) / wpb1));
  const int nw1 = nwg1 * wpb1;
  if (nw1 > kMaxRegions) return false;
  const int cap1 = (int)(((groups + nw1 - 1) / nw1) * 64);
  // L1 regions (point, best screen value); L2 overflow list (flat)
  const size_t slots = (size_t)nw1 * cap1;
  c.fb_list.ensure(sizeof(int32_t) * 3 * slots);
  c.fb_count.ensure(sizeof(int32_t) * (size_t)(nw1 + 2));
  HIP_CHECK(hipMemsetAsync(c.fb_count.p, 0, sizeof(int32_t) * (size_t)(nw1 + 2), c.stream));
  int32_t* list1 = c.fb_list.as<int32_t>();
  float* best1 = reinterpret_cast<float*>(list1 + slots);
  int32_t* ovf = list1 + 2 * slots;
  int32_t* cnt1 = c.fb_count.as<int32_t>();
  int32_t* ovf_count = cnt1 + nw1 + 1;
  c.big_chunks.ensure(sizeof(int32_t) * (size_t)(nw1 + 1));
  int32_t* chunk_pre = c.big_chunks.as<int32_t>();
  c.fb_regions = nw1;
  c.fb_total_slot = nw1;  // L1 leftovers: the "fallback" statistic
  c.fb_layout = -1;       // screen32 must re-zero its counter layout
  BigArgs a;
  a.XB = big_ensure_xb(c);
  a.n = c.n;
  a.n_pad = c.n_pad;
  a.d = d;
  a.k = k;
  a.Q = d4_of(d) / 4;
  a.KB = KB;
  a.frag = reinterpret_cast<const h8*>(dp);
  a.cinit = reinterpret_cast<const float*>(dp + L.o_cinit);
  a.thr0 = thr1;
  a.thr_rel = thr_rel;
  a.thr_dev = thr_dev;
  a.gate = gate;
  a.jkeep = ~((1u << JB) - 1u) | 15u;
  // DELTA: the running sums follow the labels of the previous large-k step
  // of this k; moves go to c.mv_list, the sums are updated by fixup_big
  // instead of a pass over every point
  static const bool nodelta = exp_env("CDR_BIG_NODELTA") != nullptr;
  const bool delta = !nodelta && c.big_valid && c.big_k == k;
  a.delta = delta ? 1 : 0;
  a.mv1 = nullptr;
  a.mv1_count = nullptr;
  a.mv2 = nullptr;
  a.mv2_count = nullptr;
  ensure_rowmajor(c);
  a.XA = c.xa32.as<float>();
  a.d4 = d4_of(d);
  if (delta) {
    c.mv_list.ensure(sizeof(int2) * 2 * slots);
    c.mv_count.ensure(sizeof(int32_t) * (size_t)(nw1 + 2));
    HIP_CHECK(hipMemsetAsync(c.mv_count.p, 0, sizeof(int32_t) * (size_t)(nw1 + 2), c.stream));
    a.mv1 = c.mv_list.as<int2>();
    a.mv1_count = c.mv_count.as<int32_t>();
    a.mv2 = a.mv1 + slots;
    a.mv2_count = a.mv1_count + nw1;
  }
  a.labels = c.labels.as<int32_t>();
  a.in_list = nullptr;
  a.in_count = nullptr;
  a.in_cap = 0;
  a.in_regions = 0;
  a.out_list = list1;
  a.out_best = best1;
  a.out_count = cnt1;
  a.out_cap = cap1;
  BigArgs a2 = a;  // L2 reads L1's regions and the same fragments / thresholds
  a2.in_list = list1;
  a2.in_count = cnt1;
  a2.in_cap = cap1;
  a2.in_regions = nw1;
  snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen_big_sp<%d,%d>", DQ, wpb1 * 64);
  if (prof) prof_mark(c, 0);
  big_launch_l1(c, a, nwg1);
  if (prof) prof_mark(c, 1);  // the L1 screen alone
  big_launch_l2_l3(c, a2, dC, ovf, ovf_count, chunk_pre);
  // the sums: a full pass over the points (first step) or the moves only
  const int len = k * (d + 1);
  c.big_sums.ensure(sizeof(long long) * len);
  unsigned long long* bs = c.big_sums.as<unsigned long long>();
  big_launch_sums(c, a2, bs);
  // what this launch chose (cdr_lloyd_big_layout); [5], the L2 form, is set
  // by big_launch_l2_l3
  c.big_info[0] = DQ;
  c.big_info[1] = KB;
  c.big_info[2] = big_fg(k);
  c.big_info[3] = JB;
  c.big_info[4] = wpb1 * 64;
  c.big_info[6] = delta ? 1 : 0;
  c.big_info[7] = nw1;
  c.big_info[8] = cap1;
  c.big_info[9] = groups;
  c.big_info[10] = thr_dev ? 1 : 0;
  c.big_thr_host[0] = thr1;
  c.big_thr_host[1] = thr_rel;
  HIP_CHECK(hipMemcpyAsync(dout, bs, sizeof(long long) * len, hipMemcpyDeviceToDevice, c.stream));
  drop_running_state(c);  // the large-k running sums are the only ones that follow these labels
  c.big_valid = true;
  c.big_k = k;
  return true;
}

// cdr_lloyd_big_layout (tests): what the last big_launch chose, and what its
// levels counted.  out = {DQ, KB, FG, JB, L1 threads, L2 form, delta, plan,
// L1 regions, cap1, groups, L1 leftovers, L3 points, mv1 moves, mv2 moves}.
// The counters are read from the launch's own buffers after a stream
// synchronise here, never on the step's path: they are those of the last
// large-k step only until another step of the context reuses the buffers.
void big_layout_read(Ctx& c, int64_t out[15]) {
  for (int i = 0; i < 15; ++i) out[i] = 0;
  if (c.big_info[0] == 0) return;
  for (int i = 0; i < 7; ++i) out[i] = c.big_info[i];
  out[7] = c.big_info[10];
  out[8] = c.big_info[7];
  out[9] = c.big_info[8];
  out[10] = c.big_info[9];
  const size_t nw1 = (size_t)c.big_info[7];
  const size_t cb = sizeof(int32_t) * (nw1 + 2);
  if (c.fb_count.bytes < cb) return;
  std::vector<int32_t> cnt(nw1 + 2), mv;
  HIP_CHECK(hipMemcpyAsync(cnt.data(), c.fb_count.p, cb, hipMemcpyDeviceToHost, c.stream));
  const bool delta = c.big_info[6] != 0 && c.mv_count.bytes >= cb;
  if (delta) {
    mv.resize(nw1 + 2);
    HIP_CHECK(hipMemcpyAsync(mv.data(), c.mv_count.p, cb, hipMemcpyDeviceToHost, c.stream));
  }
  HIP_CHECK(hipStreamSynchronize(c.stream));
  out[11] = cnt[nw1];
  out[12] = cnt[nw1 + 1];
  if (delta) {
    for (size_t w = 0; w < nw1; ++w) out[13] += mv[w];
    out[14] = mv[nw1];
  }
}

}  // namespace cdr
