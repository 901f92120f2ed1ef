// screen32_common.h — what the screen32 kernel families (screen32_full.hip,
// screen32p.hip, screen32b.hip, screen32bs.hip) and their host side
// (screen32.hip) share: vector types, the fp16 split and top-2 helpers, the
// argument structs, the chunk and dynamic-tail constants with the chunk
// ranges of the bounded screens, the bound-word packers, and each family's
// launch interface with the one (Q, MT) dispatch behind it.
#pragma once
#include <type_traits>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>

#include "cdr_internal.h"
#include "exact_math.h"
#include "plan32.h"

namespace cdr {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16 __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  h2 h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}

// hi = fp16(x) pairs (round to nearest even), lo = fp16(x - hi) pairs:
// 2 v_cvt_pk_f16_f32 + 4 v_fma_mix.
// x - hi is exact in fp32; v_fma_mix reads hi as f16 (op_sel_hi) and rounds
// x - hi once to f16 into the low / high half of the destination.
__device__ __forceinline__ void split4(const f4& x, unsigned& h01, unsigned& h23,
                                       unsigned& l01, unsigned& l23) {
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h01) : "v"(x[0]), "v"(x[1]));
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h23) : "v"(x[2]), "v"(x[3]));
  unsigned a, b;
  asm volatile(
      "v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %1, %3, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %2, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(a), "=&v"(b)
      : "v"(h01), "v"(h23), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]));
  l01 = a;
  l23 = b;
}

__device__ __forceinline__ void merge_top2(unsigned& b, unsigned& s, unsigned b2, unsigned s2) {
  const unsigned nb = min(b, b2);
  s = min(max(b, b2), min(s, s2));
  b = nb;
}

__device__ __forceinline__ void swap32(unsigned& x, unsigned& y) {
  auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}

// fp32 (lo / hi fp16 half of w) - c, one rounding (v_fma_mix_f32)
__device__ __forceinline__ float mix_sub_lo(unsigned w, float c) {
  float r;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(w), "v"(c));
  return r;
}
__device__ __forceinline__ float mix_sub_hi(unsigned w, float c) {
  float r;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r)
      : "v"(w), "v"(c));
  return r;
}

// the full screen (screen32_full.hip)
struct S32Args {
  const float* X;
  const float* X0;     // original points (x32): the exact fallback reads them
  const double* cent;  // k x d fp64 centroids (the exact fallback)
  int64_t n, n_pad;
  int d, k, Q;         // Q = number of stored feature quads (d4 / 4)
  const h8* frag;      // [MT][2][64]: A1, A3
  const float* cinit;  // [MT][16][64]
  const float* mu_s;   // [d] -mu_f 2^sigma
  float sig;
  float thr0, thr_rel;
  int32_t* labels;
  unsigned long long* run_sums;  // kRunSlices x (k, d+1) int64 running sums
  const long long* muf;          // PRE: int64 mu_f 2^S (null otherwise)
  double fx;                     // 2^(S - sigma) (PRE) or 2^S: table value -> fixed point
  int KP;
  int32_t* fb_list;
  int32_t* fb_count;
  int fb_cap;
  float* dbg;  // tests only: screen values (n_pad x dbg_ld) when non-null
  int dbg_ld;   // ceil(k / 16) * 16 (the cdr_debug_screen layout)
  const long long* gate;  // device loop: run only while gate[0] != 0 (null: always)
  const float* thr_dev;   // device loop: thr0 written by plan32_kernel (null: thr0)
};

// the fixup fused into screen32p / screen32b (screen32_fix.h: fixup_regions)
struct FixArgs {
  const float* XA;     // the points row-major, d4 floats per point (one line each)
  int64_t n_pad;
  const double* cent;  // k x d fp64 centroids of the step
  int k, d;
  int32_t* labels;
  uint8_t* lab8;  // kept equal to labels (the DELTA screens read it)
  const int2* fb_list;  // {pt, old label}
  const int32_t* fb_count;
  const int2* mv_list;
  const int32_t* mv_count;
  int cap;
  int regions;  // screen waves
  int fr;       // screen waves (list regions) per workgroup: 4, the screen's own
  double fx;    // 2^S
  unsigned long long* run_sums;  // kRunSlices x (k, d+1)
  const long long* gate;
  int abl;  // timing experiments only (0 in the product build): 1 no moves, 2 no fallback,
           // 4 no flush, 8 first candidate only, 16 no point gather, 32 no label / table change
  // the step's screen (the uncertified points are screened again)
  const unsigned char* XS;
  const h8* frag;
  const float* cinit;
  float thr0, thr_rel;
  const float* thr_dev;
  // hi-only screen copy (always): the re-screen splits the points itself
  // from XA, with split4 (the hi bits of the screen copy and their lo halves)
  int ho;
  const float* ms;  // -mu_f 2^sigma
  float sig;
  // screen32b's per-point bound words (null otherwise): a label change here
  // leaves the point's word "no bound" with its new label
  uint32_t* zb;
};

// screen32b's bound word of a point whose bound is unknown (a quiet NaN: the
// bound test fails) — the low 6 bits carry the label
constexpr unsigned kZbStale = 0x7FC00000u;

// the pruned screen (screen32p.hip)
struct S32PArgs {
  const unsigned char* XS;  // hi-only screen copy (split_copy_kernel's tiles)
  int64_t n, n_pad;
  int k, d;
  const float* prune;  // the plan's prune block (plan32.h: c32 | E | h)
  // the k-way screen of the queued points: the step's plan
  const h8* frag;
  const float* cinit;
  float thr0, thr_rel, Dv;
  const float* thr_dev;
  const long long* gate;
  int32_t* labels;
  uint8_t* lab8;
  int2* fb_list;  // per-wave regions {pt, old label}
  int32_t* fb_count;
  int2* mv_list;  // per-wave regions {pt, old | new << 16}
  int32_t* mv_count;
  int cap;
  long long* q_acc;  // profiling: points queued for the k-way screen, per wave (null: off)
  FixArgs fx;        // the fused fixup
  int fuse;
  int abl;  // timing experiments only (0 in the product build): 1 no drains,
            // 2 no per-point work (loads and the label byte only)
};

// the bounded screens (screen32b.hip, screen32bs.hip)
constexpr int kBChunk = 256;  // points per wave-chunk of the bound stream (4 per lane)
constexpr int kBList = 512;   // per-wave LDS list of the points whose bound failed
constexpr int kBPD = 4;       // chunks in flight per wave (phase 1)

struct S32BArgs {
  S32PArgs p;                // the pruned screen's plan, lists and fused fixup
  const unsigned char* XH;   // AoS hi-only copy: 2 x 16 B (d <= 8: 2 x 8 B) per point
  uint32_t* zb;              // per point: Z bits | label (n_pad words)
  const float* wup;          // [64] W_j of this step's centroids, rounded up
  const float* wdn;          // [64] rounded down
  int64_t nchunks;           // n_pad / kBChunk
  long long* t_acc;          // profiling: points whose bound failed, per wave (null: off)
  int dbg;                   // tests only (CDR_BOUNDS_DBG): 1 = every bound fails
  int direct;                // screen32bs: the direct test decides first (CDR_S32BS_DIRECT=0: off)
  unsigned long long* tprof; // experiments build only: per-wave timestamps (null: off)
  // screen32bs: chunk shares per CU slot (the workgroups blockIdx / slot_wg
  // = s share chunks [R_s, R_s+1) in proportion wsl[s]); slot_wg 0: one
  // strided split over all waves
  int slot_wg;
  int wsl[4];
  // split form (screen32bz streams the words, screen32bs<Q, MT, true> decides):
  // per-wave lists of the failed points in screen32bz's entry format, their
  // lengths, and the entries each list has room for
  uint32_t* zl;
  int32_t* zn;
  int64_t zcap;
  // the fused screen32bs: 2-byte words and their tables in
  // Ctx::bnd (plan32.h kBnd*)
  uint16_t* zh;
  const unsigned char* bt;
  // the 2-byte screen's dynamic tail (slot_wg > 0; null: off): each
  // generation region streams its first dyn_pct % statically (strided over
  // its waves) and hands the rest out kBPD chunks at a time from a counter
  // (dyn[((par * 4 + region) * 8 + xcd) * 32]: per XCD, a 128-byte line
  // each; the launch zeroes the other parity's counters for the next one)
  unsigned* dyn;
  int dyn_par, dyn_pct;
  // the watch list (watch null: the list path is off): the
  // watch words of Ctx::bnd (plan32.h kW*: the default form runs on
  // kWatchFull, the WATCH form on kWatchList with no overflow), wave w's
  // entries wl[w wcap .. + wn[w]) of the points [w wrange, (w + 1) wrange),
  // and the failed entries per wave of the last screen
  int* watch;
  uint32_t* wl;
  int32_t* wn;
  int32_t* wf;
  int wcap, wrange;
};
constexpr int kZ16Chunk = 512;  // points per wave-chunk of the 2-byte word stream (8 per lane)
// the dynamic tail's static percent (100: off; 90: 3-5 us less per config-3
// step than 100, profiles/r05_dynamic_tail_ab.txt)
constexpr int kS32DynPct = 90;
// ... from this many chunks per wave: a wave's last claim (the one that finds
// the pool empty) is an exposed atomic round trip, and with a few chunks per
// wave the tail costs more than it balances (12.5M x 16: 0.050 ms per step
// without, 0.055 with; 10M x 8: 0.036 / 0.040)
constexpr int kS32DynMinChunks = 24;

// The chunks wave `wv` of this workgroup streams: wbase + i * wstride below
// wend.  With slot_wg > 0 the workgroups of one CU slot (launch generation)
// share a region in proportion to its weight: the later generations on a CU
// get fewer issue slots (oldest-first) and otherwise finish last.
__device__ __forceinline__ void bs_range(const S32BArgs& B, int wv, int64_t& wbase, int& wstride,
                                         int64_t& wend, int64_t* rr0 = nullptr,
                                         int* rsl = nullptr) {
  const int64_t nchunks = B.nchunks;
  wbase = (int64_t)blockIdx.x * 4 + wv;
  wend = nchunks;
  wstride = (int)gridDim.x * 4;
  if (B.slot_wg < 0) {
    // contiguous ranges: wave w streams chunks [w cpw, (w + 1) cpw), so the
    // rows its failed points gather lie in one ~cpw * 16 KiB stretch of the
    // row-major copy (a few pages: the gathers stay TLB-resident) instead of
    // spread over the whole copy
    const int64_t nw = (int64_t)gridDim.x * 4, cpw = (nchunks + nw - 1) / nw;
    wbase = wbase * cpw;
    wend = wbase + cpw < nchunks ? wbase + cpw : nchunks;
    wstride = 1;
  } else if (B.slot_wg > 0) {
    const int ns = (int)gridDim.x / B.slot_wg;
    const int sl = (int)blockIdx.x / B.slot_wg;
    int wsum = 0, wpre = 0;
    for (int q = 0; q < ns; ++q) {
      wsum += B.wsl[q];
      if (q < sl) wpre += B.wsl[q];
    }
    const int64_t R0 = nchunks * wpre / wsum, R1 = nchunks * (wpre + B.wsl[sl]) / wsum;
    wstride = B.slot_wg * 4;
    wbase = R0 + (int64_t)((int)blockIdx.x - sl * B.slot_wg) * 4 + wv;
    wend = R1;
    if (rr0) *rr0 = R0;
    if (rsl) *rsl = sl;
  }
  wbase = __builtin_amdgcn_readfirstlane((int)wbase);
}

// Host mirrors of bs_range.  The largest generation region (chunks;
// slot_wg > 0):
inline int64_t bs_max_region(const S32BArgs& B, int nwg) {
  const int ns = nwg / B.slot_wg;
  int wsum = 0;
  for (int q = 0; q < ns; ++q) wsum += B.wsl[q];
  int64_t mx = 0, wpre = 0;
  for (int q = 0; q < ns; ++q) {
    mx = std::max<int64_t>(mx, B.nchunks * (wpre + B.wsl[q]) / wsum - B.nchunks * wpre / wsum);
    wpre += B.wsl[q];
  }
  return mx;
}

// ... and the most chunks any wave of the grid streams:
inline int64_t bs_max_chunks(const S32BArgs& B, int nwg) {
  const int64_t nchunks = B.nchunks;
  if (B.slot_wg <= 0) return ceil_div(nchunks, (int64_t)nwg * 4);  // (strided or contiguous)
  const int ns = nwg / B.slot_wg;
  int wsum = 0;
  for (int q = 0; q < ns; ++q) wsum += B.wsl[q];
  int64_t mx = 0, wpre = 0;
  for (int q = 0; q < ns; ++q) {
    const int64_t R0 = nchunks * wpre / wsum, R1 = nchunks * (wpre + B.wsl[q]) / wsum;
    mx = std::max<int64_t>(mx, ceil_div(R1 - R0, (int64_t)B.slot_wg * 4));
    wpre += B.wsl[q];
  }
  return mx;
}

// The stored word of bounds (l0, u0) and W_a rounded down (screen32b.hip):
// Z = l0 (1 - 2^-20) - u0 + w minus 2^-21 (|l0| + u0 + w), which covers the
// three fp32 roundings of the sum; no usable bound -> -1 (the test fails).
__device__ __forceinline__ unsigned zb_pack(float l0, float u0, float w, unsigned label) {
  if (!(l0 > 0.0f) || !(u0 >= 0.0f) || !(w >= 0.0f)) return 0xBF800000u | label;
  l0 = fminf(l0, 0x1p60f) * (1.0f - 0x1p-20f);
  const float s = (l0 - u0) + w;
  const float m = 0x1p-21f * ((l0 + u0) + w);
  const float z = s - m;
  return (z > 0.0f ? (__float_as_uint(z) & ~63u) : 0xBF800000u) | label;
}

// The 2-byte word of a decided point: zb_pack's Z relative to the point's
// base (w = W_a - G_a rounded down), truncated to its code (plan32.h); no
// bound (code 0) when Z <= G_a + 2^E0.
__device__ __forceinline__ unsigned short zb16_pack(float l0, float u0, float w, int e0,
                                                    unsigned label) {
  if (!(l0 > 0.0f) || !(u0 >= 0.0f) || !(w >= 0.0f)) return (unsigned short)label;
  l0 = fminf(l0, 0x1p60f) * (1.0f - 0x1p-20f);
  const float s = (l0 - u0) + w;
  const float m = 0x1p-21f * ((l0 + u0) + w);
  int c = zb16_code(s - m, e0);
  c = c < 0 ? 0 : (c > 1022 ? 1022 : c);
  return (unsigned short)((unsigned)c << 6 | label);
}

// ---------------------------------------------------------------------------
// Launch interface.  Every family is instantiated for Q = 1..4 feature quads
// (the full screen: QH = 1, 2 quads per lane half) and MT = 1, 2 centroid
// tiles, and exposes its occupancy (workgroups per CU, 1..8) and its launch.
// ---------------------------------------------------------------------------

// f(integral_constant<int, Q>, integral_constant<int, MT>) for the runtime
// (Q, MT), Q = 1..QMAX and MT = 1, 2; anything else is a caller's error.
template <int QMAX, class F>
inline void dispatch_q_mt(int Q, int MT, F&& f) {
  static_assert(QMAX == 2 || QMAX == 4, "feature quads: 1..2 per lane half or 1..4 per point");
  if (Q < 1 || Q > QMAX || MT < 1 || MT > 2)
    CDR_FAIL(CDR_ERR_STATE, "screen32: no kernel for this (Q, MT)");
  auto with_q = [&](auto q) {
    if (MT == 1) f(q, std::integral_constant<int, 1>{});
    else f(q, std::integral_constant<int, 2>{});
  };
  if constexpr (QMAX == 4) {
    if (Q == 3) return with_q(std::integral_constant<int, 3>{});
    if (Q == 4) return with_q(std::integral_constant<int, 4>{});
  }
  if (Q == 1) with_q(std::integral_constant<int, 1>{});
  else with_q(std::integral_constant<int, 2>{});
}

// Workgroups of 256 threads per CU the runtime reports for `kernel`, 1..8
// (2 when the query fails).
template <class K>
inline int occupancy_blocks(K kernel, size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, lds) != hipSuccess || nb < 1)
    nb = 2;
  return nb > 8 ? 8 : nb;
}

// screen32_full.hip: screen32<QH, MT, FULLQ, DBG, PRE> with `lds` bytes of
// dynamic LDS (FULLQ: a.Q == 2 QH; DBG: a.dbg != null; PRE: a.muf != null)
int screen32_blocks_per_cu(int QH, int MT, size_t lds);
void screen32_launch(int QH, int MT, dim3 grid, hipStream_t s, size_t lds, const S32Args& a);
// screen32p.hip: screen32p<Q, MT, 3> (3 groups in flight per wave)
int screen32p_blocks_per_cu(int Q, int MT);
void screen32p_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32PArgs& p);
// screen32b.hip: screen32b<Q, MT>; the stream of the two-launch form
// (screen32bz) and the bound-word kernels: reset of every point's word to
// "no bound" (z16: 2-byte words), and the rebase of the 2-byte words
int screen32b_blocks_per_cu(int Q, int MT);
void screen32b_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32BArgs& p);
void screen32bz_launch(dim3 grid, hipStream_t s, const S32BArgs& p);
void bound_words_reset(bool z16, hipStream_t s, const uint8_t* lab8, void* zb, int64_t n,
                       int64_t n_pad, const long long* gate);
void zh_rebase(Ctx& c, const long long* gate);
// screen32bs.hip: screen32bs<Q, MT, split> (split: the lists of screen32bz),
// or with a watch list in the arguments (p.watch; list: its occupancy)
// screen32bsw<Q, MT>, one launch running the default or the WATCH form
// (<4,1>: the two forms' own kernels, each gated on the mode word)
int screen32bs_blocks_per_cu(int Q, int MT, bool list);
void screen32bs_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32BArgs& p, bool split);

}  // namespace cdr
