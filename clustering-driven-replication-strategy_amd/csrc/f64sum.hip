// f64sum.hip — exact, parallel F64-mode centroid sums (src/kmeans_plusplus.py:
// 41, `X[labels == j].mean(axis=0)`): for d >= 2 NumPy adds the selected rows
// one after another, so sums[j][f] is the SEQUENTIAL fp64 sum of the column in
// row order.  Floating-point addition is not associative; this reproduces the
// sequential result bit for bit without a serial pass over n.
//
// While the running value s stays inside one binade [2^e, 2^(e+1)) it is
// m * g with g = 2^(e-52) and 2^52 <= m < 2^53, and adding x >= 0 gives
// m + q + (rounding of the fraction r of x / g: up when r > 1/2, down when
// r < 1/2, to even when r == 1/2).  Only the tie depends on m, through its
// parity, so a run of additions inside one binade is an integer transfer that
// depends only on the parity of m when the run starts: (D0, P0) for an even
// entry and (D1, P1) for an odd one (the same idea as the seeding cumsum,
// csrc/seed_common.h).
//
//   A  f64_blocksum   per 256-row block: approximate per-(cluster, feature)
//                     sums (any order) and member counts
//   B  f64_predict_a/b/c  per (cluster, feature): running approximate prefix
//                     (group sums, group prefix, in-group prefix) -> the
//                     binade the exact running value is expected to be in
//                     when each block starts
//   C  f64_transfer   per (block, feature): the block's transfer for every
//                     cluster in its predicted binade (flagged when an addend
//                     is negative or not below the binade's top)
//   G  f64_group      per (cluster, feature) and group of 64 blocks: the
//                     group's composed transfer when all its blocks share one
//                     predicted binade
//   D  f64_walk       per (cluster, feature), sequential over the groups (one
//                     step each) and, where a group cannot be applied whole,
//                     its blocks: the exact running value; a block whose prediction missed,
//                     whose transfer is flagged or would leave the binade is
//                     re-added element by element in real fp64 (so the result
//                     is exact whatever the data; the prediction only decides
//                     how often that happens: about once per binade crossing,
//                     ~log2(n) times per sequence for non-negative data).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "cdr_internal.h"
#include "f64sum.h"

namespace cdr {

namespace {

template <typename T>
__global__ __launch_bounds__(kFB) void f64_blocksum(const T* __restrict__ X, int64_t n,
                                                    int64_t n_pad, int d, int k,
                                                    const int32_t* __restrict__ labels,
                                                    double* __restrict__ A,
                                                    unsigned* __restrict__ cnt) {
  extern __shared__ double sh[];
  double* tab = sh;                                   // [k][d]
  unsigned* c = reinterpret_cast<unsigned*>(sh + k * d);  // [k]
  const int64_t b = blockIdx.x;
  for (int i = threadIdx.x; i < k * d; i += kFB) tab[i] = 0.0;
  for (int i = threadIdx.x; i < k; i += kFB) c[i] = 0;
  __syncthreads();
  const int64_t row = b * kFB + threadIdx.x;
  if (row < n) {
    const int j = labels[row];
    atomicAdd(&c[j], 1u);
    for (int f = 0; f < d; ++f) atomicAdd(&tab[j * d + f], (double)X[xidx(X, f, row, n_pad)]);
  }
  __syncthreads();
  // sequence-major ([cluster * d + feature][block], [cluster][block]): the
  // later passes walk one sequence over the blocks with the lanes, so their
  // loads are contiguous
  const int64_t nbk = gridDim.x;
  for (int i = threadIdx.x; i < k * d; i += kFB) A[(int64_t)i * nbk + b] = tab[i];
  for (int i = threadIdx.x; i < k; i += kFB) cnt[(int64_t)i * nbk + b] = c[i];
}

// The predicted binade of each block's start: an exclusive prefix of the
// approximate block sums per (cluster, feature), any order (it only
// predicts), in three parallel passes over groups of 64 blocks: group sums
// (one wave per sequence and group), the groups' exclusive prefix (one wave
// per sequence), the blocks' prefix inside each group.
// (GC: the clusters' member counts per group as well, from the waves of
// feature 0 - f64_predict_b adds them up; null: not wanted)
__global__ __launch_bounds__(256) void f64_predict_a(const double* __restrict__ A,
                                                     const unsigned* __restrict__ cnt,
                                                     int64_t nb, int d, int k, int64_t ng,
                                                     double* __restrict__ GS,
                                                     unsigned long long* __restrict__ GC) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)k * d * ng) return;
  const int t = (int)(w / ng);
  const int64_t g = w % ng;
  const int j = t / d;
  const int64_t b = g * 64 + lane;
  const unsigned cb = b < nb ? cnt[(int64_t)j * nb + b] : 0u;
  double v = cb ? A[(int64_t)t * nb + b] : 0.0;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) GS[w] = v;
  if (GC && t % d == 0) {  // (wave-uniform)
    unsigned long long s = cb;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) GC[(int64_t)j * ng + g] = s;
  }
}
// (GC non-null: the waves of feature 0 also write cluster t / d's member
// count, the sum of its group counts - the fused step's counts)
__global__ __launch_bounds__(256) void f64_predict_b(double* __restrict__ GS, int kd,
                                                     int64_t ng, const double* __restrict__ off,
                                                     const unsigned long long* __restrict__ GC,
                                                     int d,
                                                     unsigned long long* __restrict__ counts) {
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (t >= kd) return;
  if (GC && t % d == 0) {  // (wave-uniform)
    const unsigned long long* gc = GC + (int64_t)(t / d) * ng;
    unsigned long long s = 0;
    for (int64_t g = lane; g < ng; g += 64) s += gc[g];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) counts[t / d] = s;
  }
  double* gs = GS + (int64_t)t * ng;
  // a shard of sharded rows starts from the earlier shards' approximate sum
  double carry = off ? off[t] : 0.0;
  for (int64_t g0 = 0; g0 < ng; g0 += 64) {
    const int64_t g = g0 + lane;
    const double v = g < ng ? gs[g] : 0.0;
    double inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (g < ng) gs[g] = carry + (inc - v);
    carry += __shfl(inc, 63);
  }
}
__global__ __launch_bounds__(256) void f64_predict_c(const double* __restrict__ A,
                                                     const unsigned* __restrict__ cnt,
                                                     int64_t nb, int d, int k, int64_t ng,
                                                     const double* __restrict__ GS,
                                                     int* __restrict__ E,
                                                     int* __restrict__ dE, int stamp) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)k * d * ng) return;
  const int t = (int)(w / ng);
  const int64_t g = w % ng;
  const int j = t / d;
  const int64_t b = g * 64 + lane;
  const double v = (b < nb && cnt[(int64_t)j * nb + b]) ? A[(int64_t)t * nb + b] : 0.0;
  double inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (b < nb) {
    const int e = binade_e(GS[w] + (inc - v));
    // (the transfer cache: a block whose prediction moved for any sequence
    // gets this step's stamp, so its transfers are formed again; every
    // writer of one block writes the same value)
    if (dE && E[(int64_t)t * nb + b] != e) dE[b] = stamp;
    E[(int64_t)t * nb + b] = e;
  }
}

// The transfer cache's work list: the blocks whose transfers are formed this
// step (all, or those whose labels changed in the assignment or whose binade
// predictions moved), compacted in any order into list with one atomic per
// workgroup (one per wave, on a single address, serialised to ~9 us per
// launch); counters[par] is this step's count, and the other counter is
// zeroed for the next step (the one that read it last has finished: stream
// order).
__global__ __launch_bounds__(256) void f64_dirty_list(const int* __restrict__ dlab,
                                                      const int* __restrict__ dE, int stamp,
                                                      int all, int64_t nb, int* __restrict__ list,
                                                      int* __restrict__ counters, int par) {
  __shared__ int wsum[4], wbase;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool need = b < nb && (all || dlab[b] != 0 || dE[b] == stamp);
  const unsigned long long m = __ballot(need);
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    wbase = tot ? atomicAdd(&counters[par], tot) : 0;
  }
  __syncthreads();
  int base = wbase;
  for (int q = 0; q < w; ++q) base += wsum[q];
  if (need) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)b;
  if (b == 0) counters[par ^ 1] = 0;
}

// One block's transfers for every cluster, split over kTQ threads per (block,
// feature): thread q walks the rows [q R, (q + 1) R), R = kFB / kTQ, with its
// per-cluster states in LDS, cluster-major ([cluster][thread]): a lane's
// state for cluster j sits at j * nt + lane, so the lanes of a wave hit
// distinct banks whatever clusters their rows belong to.  The kTQ parts are
// then composed in row order with shuffles (xfer_join).  Each row's update
// is a serial LDS read-modify-write, so a wave's time is its rows' chain:
// with the whole block in one thread (256 rows) a launch could not go below
// one ~80 us chain however few blocks the transfer cache leaves.  Measured
// over the bench's F64 window (10M x 5, k = 16, steps 3-22, with the cache):
// 1, 2 and 4 parts 0.413-0.417 / 0.404-0.405 / 0.414-0.415 ms per step (more
// parts shorten the chains but add the per-thread setup and joins).
constexpr int kTQ = 2;
// a then b, both Xfer (d0: steps for an even entry, dd: odd - even, flags:
// bit0 P0, bit1 P1, bit2 invalid, bit3 members)
__device__ __forceinline__ void xfer_join(long long& d0, int& dd, int& fl, long long bd0, int bdd,
                                          int bfl) {
  const int p0 = fl & 1, p1 = (fl >> 1) & 1;
  const int q0 = bfl & 1, q1 = (bfl >> 1) & 1;
  d0 += bd0 + (p0 ? bdd : 0);
  dd += (p1 ? bdd : 0) - (p0 ? bdd : 0);
  fl = (p0 ? q1 : q0) | ((p1 ? q1 : q0) << 1) | ((fl | bfl) & 12);
}
// NTS: log2 of the workgroup size (the state rows' stride: shifts, not
// quarter-rate multiplies, in the per-row LDS addresses)
template <typename TA, typename S, int NTS>
__global__ __launch_bounds__(256) void f64_transfer(const S* __restrict__ X, int64_t n, int64_t n_pad, int d,
                             int k, int64_t nb, const int32_t* __restrict__ labels,
                             const int* __restrict__ E, Xfer* __restrict__ T,
                             const int* __restrict__ list, const int* __restrict__ lcount) {
  extern __shared__ unsigned char smem[];
  constexpr int nt = 1 << NTS;
  long long* s0 = reinterpret_cast<long long*>(smem);   // [k][nt]
  int* sdd = reinterpret_cast<int*>(s0 + (size_t)nt * k);  // [k][nt]
  int* sfl = sdd + (size_t)nt * k;                        // [k][nt]
  int* se = sfl + (size_t)nt * k;                         // [k][nt]
  const int64_t t = (int64_t)blockIdx.x * nt + threadIdx.x;
  // the d * kTQ threads of one block are neighbours (they share its label
  // stream), the kTQ parts of one (block, feature) in consecutive lanes.
  // (list: the transfer cache's blocks, lcount[0] of them; the others keep
  // the transfers they have)
  const int64_t item = t / (d * kTQ);
  const bool live = list ? item < (int64_t)lcount[0] : item < nb;
  const int64_t b = live ? (list ? (int64_t)list[item] : item) : 0;
  const int f = live ? (int)(t / kTQ % d) : 0;
  const int q = (int)(t % kTQ);
  long long* m0 = s0 + threadIdx.x;  // [j * nt]
  int* mdd = sdd + threadIdx.x;
  int* mfl = sfl + threadIdx.x;
  int* me = se + threadIdx.x;
  if (!live) return;  // (whole groups of kTQ lanes)
  for (int j = 0; j < k; ++j) {
    m0[j * nt] = 0;
    mdd[j * nt] = 0;
    mfl[j * nt] = 2;  // P0 = 0, P1 = 1
    me[j * nt] = E[((int64_t)j * d + f) * nb + b];
  }
  constexpr int kR = kFB / kTQ;
  const int64_t r0 = b * kFB + q * kR, r1 = min(n, r0 + kR);
  // rows in chunks of 16, the next chunk's labels and values loaded while
  // the current one goes through the (serial, LDS-dependent) updates: at two
  // waves per SIMD (LDS-bound) the memory latency is not hidden otherwise
  // (0.27 ms at 10M x 5, k = 16 with the loads of a chunk issued only at its start)
  constexpr int kCh = 16;
  static_assert(kR % kCh == 0, "whole chunks per part");
  int lj[kCh], nj[kCh];
  double lx[kCh], nx[kCh];
  auto load = [&](int64_t rc, int* jj, double* xx) {
    if (rc + kCh <= r1) {  // (all but the last chunk of the last block)
#pragma unroll
      for (int u = 0; u < kCh; ++u) {
        jj[u] = labels[rc + u];
        xx[u] = (double)X[xidx(X, f, rc + u, n_pad)];
      }
    } else {
#pragma unroll
      for (int u = 0; u < kCh; ++u) {
        const int64_t row = rc + u;
        jj[u] = row < r1 ? labels[row] : -1;
        xx[u] = row < r1 ? (double)X[xidx(X, f, row, n_pad)] : 0.0;
      }
    }
  };
  if (r0 < r1) load(r0, lj, lx);
  for (int64_t rc = r0; rc < r1; rc += kCh) {
    if (rc + kCh < r1) load(rc + kCh, nj, nx);
    // the chunk's binades (read-only), then its state-free parts, then the
    // serial state updates
    int le[kCh];
#pragma unroll
    for (int u = 0; u < kCh; ++u) {
      const int ev = me[(lj[u] < 0 ? 0 : lj[u]) * nt];
      le[u] = lj[u] >= 0 ? ev : kENone;
    }
    XPre pr[kCh];
#pragma unroll
    for (int u = 0; u < kCh; ++u) pr[u] = xfer_pre<TA>(lx[u], le[u]);
    // branch-free (a row past the end rewrites cluster 0's state unchanged),
    // the row's three state words read together before its writes
#pragma unroll
    for (int u = 0; u < kCh; ++u) {
      const bool live_row = lj[u] >= 0;
      const int o = (live_row ? lj[u] : 0) * nt;
      long long a = m0[o];
      int bq = mdd[o], c = mfl[o];
      const long long a0 = a;
      const int b0 = bq, c0 = c;
      xfer_apply(pr[u], a, bq, c);
      m0[o] = live_row ? a : a0;
      mdd[o] = live_row ? bq : b0;
      mfl[o] = live_row ? c : c0;
    }
#pragma unroll
    for (int u = 0; u < kCh; ++u) {
      lj[u] = nj[u];
      lx[u] = nx[u];
    }
  }
  // the parts in row order: lane q takes q + o's composition when q is a
  // multiple of 2o (a tree over the kTQ consecutive lanes), lane 0 writes
  for (int j = 0; j < k; ++j) {
    long long x0 = m0[j * nt];
    int xdd = mdd[j * nt], xfl = mfl[j * nt];
#pragma unroll
    for (int o = 1; o < kTQ; o <<= 1) {
      const long long y0 = __shfl_down(x0, o, kTQ);
      const int ydd = __shfl_down(xdd, o, kTQ);
      const int yfl = __shfl_down(xfl, o, kTQ);
      if ((q & (2 * o - 1)) == 0) xfer_join(x0, xdd, xfl, y0, ydd, yfl);
    }
    if (q == 0) T[((int64_t)j * d + f) * nb + b] = Xfer{x0, xdd, xfl};
  }
}

// Group transfers: one wave per (cluster, feature) and group of 64 blocks
// (all groups in parallel): when every non-empty block of the group is
// predicted in one binade with a usable transfer, their composition (the
// same 6-level shuffle tree as f64_walk's) so that the walk applies the
// whole group in one step.
__global__ __launch_bounds__(256) void f64_group(const unsigned* __restrict__ cnt,
                                                 const int* __restrict__ E,
                                                 const Xfer* __restrict__ T, int64_t nb, int d,
                                                 int k, int64_t ng, GXfer* __restrict__ G,
                                                 const int* __restrict__ Eend) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int kd = k * d;
  if (w >= (int64_t)kd * ng) return;
  const int t = (int)(w / ng);
  const int64_t g = w % ng;
  const int j = t / d;
  const int64_t bl = g * 64 + lane;
  const bool in = bl < nb;
  const unsigned c = in ? cnt[(int64_t)j * nb + bl] : 0u;
  const int el = in ? E[(int64_t)t * nb + bl] : kENone;
  const Xfer xl = in ? T[(int64_t)t * nb + bl] : Xfer{0, 0, 4};
  const unsigned long long live = __ballot(c != 0);
  int e0 = kENone;
  if (live) e0 = __shfl(el, __ffsll((long long)live) - 1);
  // Eend (sharded programs, f64s_program): a block is usable only when the
  // predicted binade at its end (the next block's start; Eend[t] after the
  // last block) is its start binade too, so no crossing falls inside it
  const int eafter = !Eend ? e0 : (bl + 1 < nb ? E[(int64_t)t * nb + bl + 1] : Eend[t]);
  const bool ok = c == 0 || (e0 != kENone && el == e0 && !(xl.flags & 4) && eafter == e0);
  const bool usable = live && __ballot(!ok) == 0ull;
  XferC x;
  const bool on = c != 0;
  x.d0 = on ? xl.d0 : 0;
  x.d1 = on ? xl.d0 + xl.dd : 0;
  x.p = on ? (xl.flags & 3) : 2;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    XferC y;
    y.d0 = __shfl_down(x.d0, o);
    y.d1 = __shfl_down(x.d1, o);
    y.p = __shfl_down(x.p, o);
    if ((lane & (2 * o - 1)) == 0 && lane + o < 64) x = xc_compose(x, y);
  }
  if (lane == 0)
    G[w] = GXfer{x.d0, x.d1, e0, (x.p & 3) | (usable ? 4 : 0) | (live ? 8 : 0)};
}

// One wave per (cluster, feature), the running value uniform across it.  The
// lanes load 64 blocks' (count, prediction, transfer) per round; the wave
// takes the longest run of blocks from the current one that are empty or
// predicted in the running value's binade with a valid transfer, composes
// their transfers with a 6-level shuffle tree (in block order) and applies
// the result at once.  A block that breaks a run (another binade, a flagged
// transfer, the first member of the sequence) or a run that would leave the
// binade is applied block by block, re-adding a block element by element in
// real fp64 whenever its transfer cannot be used.  (Stepping every block
// through the transfer one at a time cost 8 ms at 10M x 5, k = 16.)
template <typename TA, typename S>
__global__ __launch_bounds__(256) void f64_walk(const S* __restrict__ X, int64_t n,
                                                int64_t n_pad, int d, int k, int64_t nb,
                                                const int32_t* __restrict__ labels,
                                                const unsigned* __restrict__ cnt,
                                                const int* __restrict__ E,
                                                const Xfer* __restrict__ T,
                                                const GXfer* __restrict__ G, int64_t ng,
                                                double* __restrict__ sums,
                                                long long* __restrict__ walked,
                                                long long* __restrict__ prof,
                                                const double* __restrict__ entry) {
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (t >= k * d) return;
  const int j = t / d, f = t % d;
  constexpr int MB = SumTraits<TA>::MB, kMinE = SumTraits<TA>::kMinE;
  constexpr long long kTop = 1ll << (MB + 1);
  // (entry: a shard of sharded rows continues the earlier shards' exact
  // running values {s [k d], any [k d]}; else the sequence starts here)
  double s = entry ? entry[t] : 0.0;  // (a T value)
  bool any = entry ? entry[k * d + t] != 0.0 : false;  // NumPy's reduce starts from the first selected row
  long long nwalk = 0;
  long long pc_el = 0, pc_slow = 0, n_slow = 0;  // CDR_F64_PROF: cycles
  const long long pc0 = prof ? (long long)clock64() : 0;
  // one block by transfer or element by element (wave-uniform b)
  auto step_block = [&](int64_t b, int e, int flags, long long d0, int dd) {
    bool ok = false;
    if (!(flags & 4) && has_binade(s)) {
      int ex;
      frexp(s, &ex);
      if (ex - 1 == e && e >= kMinE) {
        const long long m = (long long)ldexp(s, MB - e);  // exact: s is on the grid
        const long long m2 = m + ((m & 1) ? d0 + dd : d0);
        if (m2 < kTop) {
          s = ldexp((double)m2, e - MB);
          ok = true;
        }
      }
    }
    if (!ok) {  // element by element, in real fp64 (row order)
      ++nwalk;
      const long long pe0 = prof ? (long long)clock64() : 0;
      const int64_t r0 = b * kFB;
      // the block's labels and values all issued first (independent loads:
      // one memory round trip, not two per 64 rows)
      static_assert(kFB == 256, "four rows per lane");
      int lj[4];
      double lx[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = r0 + 64 * q + lane;
        lj[q] = row < n ? labels[row] : -1;
        lx[q] = row < n ? (double)X[xidx(X, f, row, n_pad)] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool mine = lj[q] == j;
        const double x = lx[q];
        unsigned long long mk = __ballot(mine);
        while (mk) {
          const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
          mk &= mk - 1;
          const long long xb = __double_as_longlong(x);
          const double v = __longlong_as_double(
              (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                               (int)(xb >> 32), l)
                           << 32) |
                          (unsigned)__builtin_amdgcn_readlane((int)xb, l)));
          s = any ? (double)((TA)s + (TA)v) : v;  // (TA arithmetic: one rounding)
          any = true;
        }
      }
      if (prof) pc_el += (long long)clock64() - pe0;
    }
  };
  // a group's (count, prediction, transfer) per lane
  auto fetch = [&](int64_t b0, unsigned& c, int& el, Xfer& xl) {
    const int64_t bl = b0 + lane;
    const bool in = bl < nb;
    c = in ? cnt[(int64_t)j * nb + bl] : 0u;
    el = in ? E[(int64_t)t * nb + bl] : kENone;
    xl = in ? T[(int64_t)t * nb + bl] : Xfer{0, 0, 4};
  };
  // Groups are read 64 at a time (one load per lane, the next 64 prefetched)
  // and taken from registers: a group that applies in one step costs no
  // memory round trip.  The per-block records are loaded only for a group
  // that does not (about one per binade crossing).
  const GXfer* Gt = G + (int64_t)t * ng;
  auto gfetch = [&](int64_t g0) {
    return g0 + lane < ng ? Gt[g0 + lane] : GXfer{0, 0, kENone, 0};
  };
  // The running value as (binade sE, grid count sN) while groups apply whole
  // (integer work on scalar registers: readlane, no LDS shuffles and no
  // double <-> integer conversions per group); s is refreshed from it before
  // a group is walked block by block, and it from s afterwards.
  int sE = kENone;
  long long sN = 0;
  auto to_int = [&]() {
    sE = kENone;
    if (has_binade(s)) {
      int ex;
      frexp(s, &ex);
      if (ex - 1 >= kMinE) {
        sE = ex - 1;
        sN = (long long)ldexp(s, MB - sE);  // exact: s is on the grid
      }
    }
  };
  GXfer gnext = gfetch(0);
  for (int64_t g0 = 0; g0 < ng; g0 += 64) {
    const GXfer gl = gnext;
    if (g0 + 64 < ng) gnext = gfetch(g0 + 64);
    const unsigned long long gl_live = __ballot((gl.p & 8) != 0);
    unsigned long long todo = gl_live;
    while (todo) {
      // a run of whole groups in the running value's binade, composed in one
      // step: the ordered prefix of their transfers (a 6-level shuffle
      // tree), then the longest prefix that stays in the binade (the values
      // only grow, so staying there at the end means staying throughout).
      // Stepping them one at a time cost ~430 cycles per group
      if (sE != kENone) {
        const int i0 = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const bool lv = (gl.p & 8) != 0;
        const bool okg = !lv || ((gl.p & 4) && gl.e == sE);
        const unsigned long long brk = ~__ballot(okg) & (~0ull << i0);
        const int r = __builtin_amdgcn_readfirstlane(brk ? __ffsll((long long)brk) - 1 : 64);
        if (r > i0 + 1) {
          const bool on = lane >= i0 && lane < r && lv;
          XferC x;
          x.d0 = on ? gl.d0 : 0;
          x.d1 = on ? gl.d1 : 0;
          x.p = on ? (gl.p & 3) : 2;  // identity: P0 = 0, P1 = 1
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            XferC y;
            y.d0 = __shfl_up(x.d0, o);
            y.d1 = __shfl_up(x.d1, o);
            y.p = __shfl_up(x.p, o);
            if (lane >= o) x = xc_compose(y, x);
          }
          const long long mq = sN + ((sN & 1) ? x.d1 : x.d0);
          const bool inrun = lane >= i0 && lane < r;
          const unsigned long long bad = __ballot(inrun && !(mq < kTop));
          const int L = __builtin_amdgcn_readfirstlane(bad ? __ffsll((long long)bad) - 1 : r);
          if (L > i0) {  // groups i0 .. L-1 at once
            sN = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                                  (int)(mq >> 32), L - 1)
                              << 32) |
                             (unsigned)__builtin_amdgcn_readlane((int)mq, L - 1));
            todo &= L >= 64 ? 0ull : (~0ull << L);
            continue;
          }
        }
      }
      const int gi = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int gp = __builtin_amdgcn_readlane(gl.p, gi);
      if ((gp & 4) && sE != kENone) {  // the whole group in one step
        const int ge = __builtin_amdgcn_readlane(gl.e, gi);
        if (sE == ge) {
          const long long gd =
              (sN & 1) ? (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                                          (int)(gl.d1 >> 32), gi)
                                      << 32) |
                                     (unsigned)__builtin_amdgcn_readlane((int)gl.d1, gi))
                       : (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                                          (int)(gl.d0 >> 32), gi)
                                      << 32) |
                                     (unsigned)__builtin_amdgcn_readlane((int)gl.d0, gi));
          const long long m2 = sN + gd;
          if (m2 < kTop) {
            sN = m2;
            continue;
          }
        }
      }
      if (sE != kENone) s = ldexp((double)sN, sE - MB);  // s from the integer state
      const long long ps0 = prof ? (long long)clock64() : 0;
      ++n_slow;
      const int64_t b0 = (g0 + gi) * 64;
      unsigned c;
      int el;
      Xfer xl;
      fetch(b0, c, el, xl);
      if (!c) xl = Xfer{0, 0, 4};
      const unsigned long long live = __ballot(c != 0);
      int i = 0;  // next block of this group (wave-uniform)
      while (i < 64) {
        const unsigned long long rest = live & (~0ull << i);
        if (!rest) break;
        i = __builtin_amdgcn_readfirstlane(__ffsll((long long)rest) - 1);  // skip empty blocks
        int es = kENone;
        if (has_binade(s)) {
          int ex;
          frexp(s, &ex);
          if (ex - 1 >= kMinE) es = ex - 1;
        }
        // blocks i.. that are empty or can take a transfer in binade es
        const bool compat = c == 0 || (es != kENone && !(xl.flags & 4) && el == es);
        const unsigned long long brk = ~__ballot(compat) & (~0ull << i);
        const int r = __builtin_amdgcn_readfirstlane(brk ? __ffsll((long long)brk) - 1 : 64);  // run [i, r)
        if (r > i + 1) {
          // inclusive ordered prefix of the run's transfers (lanes outside it
          // are the identity), then the longest prefix that stays in the
          // binade is applied at once and the block that leaves it is
          // stepped alone: one scan per binade crossing, not one per block
          XferC x;
          const bool on = lane >= i && lane < r && c != 0;
          x.d0 = on ? xl.d0 : 0;
          x.d1 = on ? xl.d0 + xl.dd : 0;
          x.p = on ? (xl.flags & 3) : 2;  // identity: P0 = 0, P1 = 1
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            XferC y;
            y.d0 = __shfl_up(x.d0, o);
            y.d1 = __shfl_up(x.d1, o);
            y.p = __shfl_up(x.p, o);
            if (lane >= o) x = xc_compose(y, x);
          }
          const long long m = (long long)ldexp(s, MB - es);
          const long long mq = m + ((m & 1) ? x.d1 : x.d0);
          const bool inrun = lane >= i && lane < r;
          const unsigned long long bad = __ballot(inrun && !(mq < kTop));
          const int L = __builtin_amdgcn_readfirstlane(bad ? __ffsll((long long)bad) - 1 : r);
          if (L > i) {  // blocks i .. L-1 in one step
            const long long mL =
                (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                                 (int)(mq >> 32), L - 1)
                             << 32) |
                            (unsigned)__builtin_amdgcn_readlane((int)mq, L - 1));
            s = ldexp((double)mL, es - MB);
            i = L;
            if (i >= r) continue;
          }
          // block L leaves the binade: stepped alone below
        }
        const int e = __builtin_amdgcn_readlane(el, i);
        const int flags = __builtin_amdgcn_readlane(xl.flags, i);
        const long long d0 = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(
                                             (int)(xl.d0 >> 32), i)
                                         << 32) |
                                        (unsigned)__builtin_amdgcn_readlane((int)xl.d0, i));
        const int dd = __builtin_amdgcn_readlane(xl.dd, i);
        step_block(b0 + i, e, flags, d0, dd);
        ++i;
      }
      to_int();
      if (prof) pc_slow += (long long)clock64() - ps0;
    }
  }
  if (sE != kENone) s = ldexp((double)sN, sE - MB);
  if (prof && lane == 0) {
    prof[4 * t] = (long long)clock64() - pc0;
    prof[4 * t + 1] = pc_slow;
    prof[4 * t + 2] = pc_el;
    prof[4 * t + 3] = n_slow;
  }

  if (lane == 0) {
    sums[(int64_t)j * d + f] = s;
    walked[t] = nwalk;
    if (entry) sums[k * d + t] = any ? 1.0 : 0.0;  // (the exit state for the next shard)
  }
}

}  // namespace

// After the block pass (c.f64x_A, c.f64x_cnt): the binade predictions into
// c.f64x_E, the transfers under them (tc: only the cache's dirty blocks), the
// group compositions and, with sh.walk, the walk.  TA: the summed
// (arithmetic) type; S: the storage type of X.
template <typename TA, typename S>
static void sums_after_block(Ctx& c, const S* X, int k, double* d_sums, const F64Shard& sh,
                             unsigned long long* d_counts, const F64TCache* tc) {
  const int d = c.d;
  const int64_t n = c.n, nb = ceil_div(n, kFB);
  const size_t kd = (size_t)k * d;
  const int64_t ng = ceil_div(nb, (int64_t)64);
  c.f64x_E.ensure(sizeof(int) * nb * kd);
  c.f64x_T.ensure(sizeof(Xfer) * nb * kd);
  c.f64x_walk.ensure(sizeof(long long) * kd);
  c.f64x_GS.ensure(sizeof(double) * ng * kd);
  const dim3 gwaves((unsigned)ceil_div((int64_t)kd * ng, (int64_t)4));
  unsigned long long* GC = nullptr;
  if (d_counts) {
    c.f64x_GC.ensure(sizeof(unsigned long long) * ng * k);
    GC = c.f64x_GC.as<unsigned long long>();
  }
  int* E = c.f64x_E.as<int>();
  hipLaunchKernelGGL(f64_predict_a, gwaves, dim3(256), 0, c.stream, c.f64x_A.as<double>(),
                     c.f64x_cnt.as<unsigned>(), nb, d, k, ng, c.f64x_GS.as<double>(), GC);
  hipLaunchKernelGGL(f64_predict_b, dim3(ceil_div((int64_t)kd, 4)), dim3(256), 0, c.stream,
                     c.f64x_GS.as<double>(), (int)kd, ng, sh.off, GC, d, d_counts);
  hipLaunchKernelGGL(f64_predict_c, gwaves, dim3(256), 0, c.stream, c.f64x_A.as<double>(),
                     c.f64x_cnt.as<unsigned>(), nb, d, k, ng, c.f64x_GS.as<double>(), E,
                     tc ? tc->dE : nullptr, tc ? tc->stamp : 0);
  HIP_CHECK(hipGetLastError());
  const int* tlist = nullptr;
  const int* tcount = nullptr;
  if (tc) {
    hipLaunchKernelGGL(f64_dirty_list, dim3((unsigned)ceil_div(nb, (int64_t)256)), dim3(256), 0,
                       c.stream, tc->dlab, tc->dE, tc->stamp, tc->all, nb, tc->list,
                       tc->counters, tc->par);
    HIP_CHECK(hipGetLastError());
    tlist = tc->list;
    tcount = tc->counters + tc->par;
  }
  // 80 KB of per-thread states per workgroup (k <= 64): two workgroups per CU
  const int nts = k <= 16 ? 8 : (k <= 32 ? 7 : 6);
  const int nt = 1 << nts;
  const size_t lds = (size_t)nt * k * (8 + 4 + 4 + 4);
  auto fn = nts == 8 ? f64_transfer<TA, S, 8> : (nts == 7 ? f64_transfer<TA, S, 7>
                                                            : f64_transfer<TA, S, 6>);
  hipLaunchKernelGGL(fn, dim3(ceil_div(nb * d * kTQ, (int64_t)nt)), dim3(nt), lds, c.stream,
                     X, n, c.n_pad, d, k, nb, c.labels.as<int32_t>(), E, c.f64x_T.as<Xfer>(),
                     tlist, tcount);
  HIP_CHECK(hipGetLastError());
  c.f64x_G.ensure(sizeof(GXfer) * ng * kd);
  static const bool prof_on = exp_env("CDR_F64_PROF") != nullptr;
  if (prof_on) c.f64x_prof.ensure(sizeof(long long) * 4 * kd);
  hipLaunchKernelGGL(f64_group, dim3(ceil_div((int64_t)kd * ng, (int64_t)4)), dim3(256), 0,
                     c.stream, c.f64x_cnt.as<unsigned>(), E, c.f64x_T.as<Xfer>(), nb, d, k, ng,
                     c.f64x_G.as<GXfer>(), sh.Eend);
  HIP_CHECK(hipGetLastError());
  if (!sh.walk) return;
  hipLaunchKernelGGL((f64_walk<TA, S>), dim3(ceil_div((int64_t)kd, 4)), dim3(256), 0, c.stream,
                     X, n, c.n_pad, d, k, nb, c.labels.as<int32_t>(),
                     c.f64x_cnt.as<unsigned>(), E, c.f64x_T.as<Xfer>(),
                     c.f64x_G.as<GXfer>(), ng, d_sums, c.f64x_walk.as<long long>(),
                     prof_on ? c.f64x_prof.as<long long>() : nullptr, sh.entry);
  HIP_CHECK(hipGetLastError());
  if (prof_on) {
    std::vector<long long> h(4 * kd);
    HIP_CHECK(hipMemcpyAsync(h.data(), c.f64x_prof.p, 8 * h.size(), hipMemcpyDeviceToHost,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    long long mx[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < kd; ++i)
      for (int q = 0; q < 4; ++q) mx[q] = std::max(mx[q], h[4 * i + q]);
    fprintf(stderr, "f64_walk max cycles: total %lld slow-groups %lld element-walks %lld; slow groups %lld\n",
            mx[0], mx[1], mx[2], mx[3]);
  }
}

void enqueue_f64_sums_after_block(Ctx& c, int k, double* d_sums, const F64Shard& sh,
                                  unsigned long long* d_counts, const F64TCache* tc) {
  sums_after_block<double, double>(c, c.x64.as<double>(), k, d_sums, sh, d_counts, tc);
}

// sums (k, d) on the device from c.labels, exact sequential row-order sums
// in TA arithmetic; returns false when the shape is not covered (d < 2,
// k > 64): the caller runs the serial kernel.
template <typename TA, typename S>
static bool sums_parallel(Ctx& c, const S* X, int k, double* d_sums) {
  const int d = c.d;
  if (d < 2 || k < 1 || k > kFMaxK || c.n < 1) return false;
  const int64_t n = c.n, nb = ceil_div(n, kFB);
  const size_t kd = (size_t)k * d;
  c.f64x_A.ensure(sizeof(double) * nb * kd);
  c.f64x_cnt.ensure(sizeof(unsigned) * nb * k);
  hipLaunchKernelGGL(f64_blocksum<S>, dim3(nb), dim3(kFB), sizeof(double) * kd + 4 * k, c.stream,
                     X, n, c.n_pad, d, k, c.labels.as<int32_t>(), c.f64x_A.as<double>(),
                     c.f64x_cnt.as<unsigned>());
  HIP_CHECK(hipGetLastError());
  sums_after_block<TA, S>(c, X, k, d_sums, F64Shard(), nullptr, nullptr);
  return true;
}

bool f64_sums_parallel(Ctx& c, int k, double* d_sums) {
  return sums_parallel<double, double>(c, c.x64.as<double>(), k, d_sums);
}

// The reference's float32 runs: sequential fp32 sums of fp32 points (X:
// F32X storage, or F64 storage holding fp32 values), returned as doubles.
bool f32_sums_parallel(Ctx& c, int k, double* d_sums) {
  if (c.mode == CDR_MODE_F32X) return sums_parallel<float, float>(c, c.x32.as<float>(), k, d_sums);
  return sums_parallel<float, double>(c, c.x64.as<double>(), k, d_sums);
}

}  // namespace cdr
