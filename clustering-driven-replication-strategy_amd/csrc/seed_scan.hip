// seed_scan.hip — the exact cumulative sum of the k-means++ draw
// (src/kmeans_plusplus.py:19; the transfer algebra: seed_common.h): the
// cumsum program (seg_* kernels), its fallback the block walk (xfer_kernel,
// walk_kernel) and the search of the drawn element (search_kernel).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "cdr_internal.h"
#include "exact_math.h"
#include "seed_common.h"

namespace cdr {

// ---- cumulative-sum emulation --------------------------------------------

__device__ __forceinline__ void compose(long long L0, long long L1, long long R0, long long R1,
                                        long long& o0, long long& o1) {
  o0 = L0 + ((L0 & 1) ? R1 : R0);
  o1 = L1 + ((L1 & 1) ? R0 : R1);
}

// Transfer of elements [lo, hi) (values v(i)) under binade exponent e.
template <typename V>
__device__ __forceinline__ void range_transfer_v(V v, double S, int64_t lo, int64_t hi, int e,
                                                 long long& D0, long long& D1, int& valid) {
  D0 = 0;
  D1 = 0;
  valid = 1;
  for (int64_t i = lo; i < hi; ++i) {
    const double p = v(i) / S;
    const double f = ldexp(p, 52 - e);
    if (!(f < 4503599627370496.0)) {  // >= 2^52 (or NaN): leaves the binade
      valid = 0;
      continue;
    }
    const double fl = floor(f);
    const double frac = f - fl;
    const long long k = (long long)fl;
    const long long up = frac > 0.5 ? 1 : 0;
    const bool tie = frac == 0.5;
    // incoming parity q = 0
    {
      const long long par = (D0 ^ k) & 1;  // parity of N + fl with N even + D0
      D0 += k + up + ((tie && par) ? 1 : 0);
    }
    {
      const long long par = (1 ^ D1 ^ k) & 1;
      D1 += k + up + ((tie && par) ? 1 : 0);
    }
  }
  if (D0 >= (1ll << 52) || D1 >= (1ll << 52)) valid = 0;
}

__device__ void range_transfer(const double* __restrict__ dmin, double S, int64_t lo,
                               int64_t hi, int e, long long& D0, long long& D1, int& valid) {
  range_transfer_v([&](int64_t i) { return dmin[i]; }, S, lo, hi, e, D0, D1, valid);
}

__device__ __forceinline__ bool binade_of(double c, int& e, long long& N) {
  const unsigned long long bits = __double_as_longlong(c);
  const int ef = (int)((bits >> 52) & 0x7FF);
  if (ef == 0 || ef >= 2046 || (bits >> 63)) return false;  // zero/subnormal/huge/neg
  e = ef - 1023;
  N = (long long)((bits & 0xFFFFFFFFFFFFFull) | (1ull << 52));
  return true;
}
__device__ __forceinline__ double from_binade(int e, long long N) {
  const unsigned long long bits =
      ((unsigned long long)(e + 1023) << 52) | ((unsigned long long)N & 0xFFFFFFFFFFFFFull);
  return __longlong_as_double(bits);
}

// Per-block transfers under the guessed binade of the block's start.  One
// wave per 8192-element block, in 8 passes of 1024: the pass is loaded
// coalesced (16 B per lane per load) into LDS with one pad slot per 16
// elements, then lane l walks elements [16 l, 16 l + 16) of the pass from LDS
// (conflict-free ds_read_b64), the 64 lane transfers are composed in order and
// the pass transfer is composed onto the block's.
constexpr int kPass = 1024;
constexpr int kPassPad = kPass + kPass / 16;

__global__ __launch_bounds__(256) void xfer_kernel(const double* __restrict__ dmin, int64_t n,
                                                   double S, const double* __restrict__ approx,
                                                   int64_t nblocks, Xfer* __restrict__ out,
    SeedDev dv) {
  if (dv.gate && dv.gate[0] != 0.0) return;
  if (dv.S) S = dv.S[0];
  __shared__ double sbuf[4][kPassPad];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  const bool live = b < nblocks;
  double* sb = sbuf[w];
  int e = 0;
  long long Ndummy;
  const bool okg = live && binade_of(approx[b], e, Ndummy);
  const int64_t base = b * kSeedBlock;
  long long T0 = 0, T1 = 0;
  int tv = okg ? 1 : 0;
  for (int ps = 0; ps < kSeedBlock / kPass; ++ps) {
    const int64_t pb = base + (int64_t)ps * kPass;
    const bool act = okg && pb < n;  // wave-uniform
    if (act) {
      // dmin is allocated to n_pad (a multiple of the block): whole passes load
      const double2* src = reinterpret_cast<const double2*>(dmin + pb);
#pragma unroll
      for (int j = 0; j < kPass / 128; ++j) {
        const double2 v = src[j * 64 + lane];
        const int el = j * 128 + 2 * lane;
        const int pos = el + (el >> 4);
        sb[pos] = v.x;
        sb[pos + 1] = v.y;
      }
    }
    __syncthreads();
    if (act) {
      const int64_t lo = pb + (int64_t)lane * 16;
      const int64_t hi = (lo + 16) < n ? (lo + 16) : n;
      long long D0 = 0, D1 = 0;
      int valid = 1;
      const double* sl = sb + lane * 17;
      if (lo < hi)
        range_transfer_v([&](int64_t i) { return sl[i - lo]; }, S, lo, hi, e, D0, D1, valid);
      // ordered reduction over lanes: lane l absorbs lane l+o
      for (int o = 1; o < 64; o <<= 1) {
        const long long r0 = __shfl_down(D0, o), r1 = __shfl_down(D1, o);
        const int rv = __shfl_down(valid, o);
        if ((lane & (2 * o - 1)) == 0 && lane + o < 64) {
          long long n0, n1;
          compose(D0, D1, r0, r1, n0, n1);
          D0 = n0;
          D1 = n1;
          valid &= rv;
        }
      }
      long long n0, n1;
      compose(T0, T1, D0, D1, n0, n1);
      tv &= valid;
      // saturate: keeps the composition of later passes from overflowing
      if (n0 >= (1ll << 52) || n1 >= (1ll << 52)) {
        tv = 0;
        n0 = n1 = 0;
      }
      T0 = n0;
      T1 = n1;
    }
    __syncthreads();
  }
  if (live && lane == 0) out[b] = Xfer{T0, T1, e, tv, 0};
}

// approx[b] = c_in + sum_{b' < b} blocksums[b'] / S   (guesses only: any
// summation order will do).  Each thread's run of block sums is loaded 8 at a
// time (the loads in flight together), the 1024 partials are scanned by waves
// (shfl) and then across the 16 waves.
__global__ __launch_bounds__(1024) void approx_prefix_kernel(const double* __restrict__ bs,
                                                             int64_t nb, double S, double c_in,
                                                             double* __restrict__ approx,
    SeedDev dv) {
  if (dv.gate && dv.gate[0] != 0.0) return;
  if (dv.S) S = dv.S[0];
  if (dv.c_in) c_in = dv.c_in[0];
  __shared__ double wsum[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t lo = t * per, hi = (lo + per) < nb ? (lo + per) : nb;
  constexpr int kB = 8;
  double s = 0.0;
  for (int64_t b0 = lo; b0 < hi; b0 += kB) {
    double v[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) v[j] = bs[b0 + j < hi ? b0 + j : lo];
#pragma unroll
    for (int j = 0; j < kB; ++j)
      if (b0 + j < hi) s += v[j] / S;
  }
  double inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  double acc = c_in;
  for (int i = 0; i < w; ++i) acc += wsum[i];
  acc += inc - s;  // the exclusive prefix of this thread's run
  for (int64_t b0 = lo; b0 < hi; b0 += kB) {
    double v[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) v[j] = bs[b0 + j < hi ? b0 + j : lo];
#pragma unroll
    for (int j = 0; j < kB; ++j) {
      if (b0 + j < hi) {
        approx[b0 + j] = acc;
        acc += v[j] / S;
      }
    }
  }
}

// Wave-parallel exact walk of elements [lo, hi) starting from running value c.
// If `search`, stops at the first element m with fl(c_m / c_last) > u and
// returns its index in *found (else *found stays -1).  Returns the running
// value after the last element processed.  Executed by all 64 lanes of a
// single-wave workgroup (it synchronises the workgroup).
//
// The range is taken in segments of 4096: p = fl(dmin / S) of the segment is
// staged in LDS (coalesced loads, one pad slot per 64 so that lane l's
// sub-chunk [64 l, 64 l + 64) reads conflict-free), then sub-chunk transfers
// are applied in bulk while they stay in the binade and the sub-chunk that
// leaves it is walked element by element.
constexpr int kSeg = 4096;
constexpr int kSegSub = kSeg / 64;

__device__ double fine_walk(const double* __restrict__ dmin, double S, int64_t lo, int64_t hi,
                            double c, bool search, double c_last, double u, int64_t* found) {
  __shared__ double sp[kSeg + kSeg / kSegSub];
  const int lane = threadIdx.x & 63;
  for (int64_t s0 = lo; s0 < hi; s0 += kSeg) {
    const int m = (int)((hi - s0) < kSeg ? (hi - s0) : kSeg);
    __syncthreads();  // the previous segment's reads are done
    if (m == kSeg && (s0 & 1) == 0) {
      // whole segment: 32 independent 16-byte loads per lane in flight
      // (a rolled load/divide/store loop would pay the full HBM latency per
      // element pair)
      const double2* src = reinterpret_cast<const double2*>(dmin + s0);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = src[(h * 16 + j) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int i = ((h * 16 + j) * 64 + lane) * 2;
          sp[i + i / kSegSub] = v[j].x / S;
          sp[i + 1 + (i + 1) / kSegSub] = v[j].y / S;
        }
      }
    } else {
      for (int i0 = 0; i0 < m; i0 += 64 * 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = i0 + j * 64 + lane;
          v[j] = i < m ? dmin[s0 + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = i0 + j * 64 + lane;
          if (i < m) sp[i + i / kSegSub] = v[j] / S;
        }
      }
    }
    __syncthreads();
    auto pv = [&](int i) { return sp[i + i / kSegSub]; };
    int pos = 0;
    while (pos < m) {
      int e;
      long long N;
      const bool inb = binade_of(c, e, N);
      int L = 0;  // sub-chunks applied in bulk
      if (inb) {
        const int slo = pos + lane * kSegSub;
        const int shi = (slo + kSegSub) < m ? (slo + kSegSub) : m;
        long long D0 = 0, D1 = 0;
        int valid = 1;
        if (slo < m)
          range_transfer_v([&](int64_t i) { return pv((int)i); }, 1.0, slo, shi, e, D0, D1,
                           valid);
        else
          valid = 0;
        // inclusive ordered prefix over lanes
        for (int o = 1; o < 64; o <<= 1) {
          const long long l0 = __shfl_up(D0, o), l1 = __shfl_up(D1, o);
          const int lv = __shfl_up(valid, o);
          if (lane >= o) {
            long long n0, n1;
            compose(l0, l1, D0, D1, n0, n1);
            D0 = n0;
            D1 = n1;
            valid &= lv;
          }
        }
        const long long Dq = (N & 1) ? D1 : D0;
        const long long Nend = N + Dq;
        bool ok = valid && slo < m && Dq < (1ll << 52) && Nend < (1ll << 53);
        bool hit = false;
        if (ok && search) hit = (from_binade(e, Nend) / c_last) > u;
        const unsigned long long okm = __ballot(ok && !hit);
        // number of leading lanes that are ok and not yet past the target
        L = (okm == ~0ull) ? 64 : __builtin_ctzll(~okm);
        if (L > 0) {
          const long long DL = __shfl(Dq, L - 1);
          c = from_binade(e, N + DL);
          pos += L * kSegSub;
          if (pos > m) pos = m;
        }
        if (pos >= m) break;
        if (L == 64) continue;  // every sub-chunk applied: next bulk round
      }
      // element-wise over (at most) one sub-chunk; lane 0 computes, broadcasts
      const int ehi = (pos + kSegSub) < m ? (pos + kSegSub) : m;
      double cc = c;
      int hitidx = -1;
      if (lane == 0) {
        for (int i = pos; i < ehi; ++i) {
          cc = cc + pv(i);
          if (search && (cc / c_last) > u) {
            hitidx = i;
            break;
          }
        }
      }
      cc = __shfl(cc, 0);
      hitidx = __shfl(hitidx, 0);
      c = cc;
      if (hitidx >= 0) {
        *found = s0 + hitidx;
        return c;
      }
      pos = ehi;
    }
  }
  return c;
}

// Single wave: exact running value through every block, cend[b] = value after
// block b.  Each round takes the next 64 blocks: the leading run of blocks
// whose transfers apply in the current binade is applied at once (an ordered
// prefix of the transfers), the first block that does not is done alone
// (its transfer if it applies from the new value, else an element walk), and
// the next round starts after it.
constexpr int kXWin = 1024;  // block transfers staged in LDS per window (32 KB)

__global__ __launch_bounds__(64) void walk_kernel(const double* __restrict__ dmin, int64_t n,
                                                  double S, const Xfer* __restrict__ xf,
                                                  int64_t nblocks, double c_in,
                                                  double* __restrict__ cend,
                                                  double* __restrict__ c_out,
                                                  long long* __restrict__ stats,
    SeedDev dv) {
  if (dv.gate && dv.gate[0] != 0.0) return;
  if (dv.S) S = dv.S[0];
  __shared__ Xfer sx[kXWin];
  const int lane = threadIdx.x;
  double c = c_in;
  int64_t dummy = -1;
  int64_t b0 = 0;
  int64_t win0 = -1;  // first block of the staged window
  long long st_rounds = 0, st_single = 0, st_fine = 0, st_fcyc = 0;
  const long long st_t0 = stats ? (long long)clock64() : 0;
  while (b0 < nblocks) {
    const int nb = (int)((nblocks - b0) < 64 ? (nblocks - b0) : 64);
    if (win0 < 0 || b0 + nb > win0 + kXWin) {
      // restage [b0, b0 + kXWin): 16 independent loads per lane in flight
      __syncthreads();
      win0 = b0;
      Xfer v[kXWin / 64];
#pragma unroll
      for (int j = 0; j < kXWin / 64; ++j) {
        const int64_t bb = b0 + j * 64 + lane;
        v[j] = bb < nblocks ? xf[bb] : Xfer{0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < kXWin / 64; ++j) sx[j * 64 + lane] = v[j];
      __syncthreads();
    }
    const Xfer r = lane < nb ? sx[b0 - win0 + lane] : Xfer{0, 0, 0, 0, 0};
    int e;
    long long N;
    const bool inb = binade_of(c, e, N);
    // inclusive ordered prefix of the round's transfers
    long long D0 = r.d0, D1 = r.d1;
    int valid = (lane < nb) && r.valid && inb && r.e == e;
    for (int o = 1; o < 64; o <<= 1) {
      const long long l0 = __shfl_up(D0, o), l1 = __shfl_up(D1, o);
      const int lv = __shfl_up(valid, o);
      if (lane >= o) {
        long long n0, n1;
        compose(l0, l1, D0, D1, n0, n1);
        D0 = n0;
        D1 = n1;
        valid &= lv;
      }
    }
    const long long Dq = (N & 1) ? D1 : D0;
    const bool ok = inb && valid && Dq < (1ll << 52) && (N + Dq) < (1ll << 53);
    const unsigned long long okm = __ballot(ok);
    int L = (okm == ~0ull) ? 64 : __builtin_ctzll(~okm);
    if (L > nb) L = nb;
    if (L > 0) {
      if (lane < L) cend[b0 + lane] = from_binade(e, N + Dq);
      c = from_binade(e, N + __shfl(Dq, L - 1));
    }
    ++st_rounds;
    if (L == nb) {
      b0 += nb;
      continue;
    }
    ++st_single;
    // block bj alone
    const int64_t bj = b0 + L;
    const Xfer rj = sx[bj - win0];
    int ej;
    long long Nj;
    bool done = false;
    if (binade_of(c, ej, Nj) && rj.valid && rj.e == ej) {
      const long long Dj = (Nj & 1) ? rj.d1 : rj.d0;
      if (Dj < (1ll << 52) && Nj + Dj < (1ll << 53)) {
        c = from_binade(ej, Nj + Dj);
        done = true;
      }
    }
    if (!done) {
      const int64_t lo = bj * kSeedBlock;
      const int64_t hi = (lo + kSeedBlock) < n ? (lo + kSeedBlock) : n;
      const long long tf = stats ? (long long)clock64() : 0;
      c = fine_walk(dmin, S, lo, hi, c, false, 1.0, 0.0, &dummy);
      if (stats) st_fcyc += (long long)clock64() - tf;
      ++st_fine;
    }
    if (lane == 0) cend[bj] = c;
    b0 = bj + 1;
  }
  if (lane == 0) *c_out = c;
  if (stats && lane == 0) {
    stats[0] += st_rounds;
    stats[1] += st_single;
    stats[2] += st_fine;
    stats[3] += st_fcyc;
    stats[4] += (long long)clock64() - st_t0;
  }
}

// Single wave: first local index m with fl(c_m / c_last) > u (or -1).  The
// running values cend are non-decreasing, so hit(b) = fl(cend[b] / c_last) > u
// is monotone in b: a 64-ary search (64 probes per round) finds the first hit
// block, then an exact walk of that block finds the element.
__global__ __launch_bounds__(64) void search_kernel(const double* __restrict__ dmin, int64_t n,
                                                    double S, const double* __restrict__ cend,
                                                    int64_t nblocks, double c_in, double c_last,
                                                    double u, int64_t* __restrict__ result,
    SeedDev dv) {
  if (dv.S) S = dv.S[0];
  if (dv.c_last) c_last = dv.c_last[0];
  if (dv.u) u = dv.u[0];
  if (dv.c_in) c_in = dv.c_in[0];
  const int lane = threadIdx.x;
  // invariant: every block < lo misses, block hi hits (hi == nblocks: none)
  int64_t lo = 0, hi = nblocks;
  while (hi - lo > 0) {
    const int64_t span = hi - lo;
    const int64_t step = (span + 63) / 64;
    const int64_t pb = lo + (int64_t)lane * step;
    const bool probe = pb < hi;
    const bool hit = probe && (cend[pb] / c_last) > u;
    const unsigned long long m = __ballot(hit);
    const unsigned long long pm = __ballot(probe);
    if (step == 1) {
      if (m) hi = lo + __builtin_ctzll(m);
      break;
    }
    // first probing lane that hits: the answer is in (probe[j-1], probe[j]]
    if (m) {
      const int j = __builtin_ctzll(m);
      hi = lo + (int64_t)j * step;
      lo = j > 0 ? lo + (int64_t)(j - 1) * step + 1 : lo;
    } else {
      const int jl = 63 - __builtin_clzll(pm);  // last probe misses
      lo = lo + (int64_t)jl * step + 1;
    }
  }
  const int64_t bstar = hi < nblocks ? hi : -1;
  int64_t found = -1;
  if (bstar >= 0) {
    const double c0 = bstar == 0 ? c_in : cend[bstar - 1];
    const int64_t lo2 = bstar * kSeedBlock;
    const int64_t hi2 = (lo2 + kSeedBlock) < n ? (lo2 + kSeedBlock) : n;
    fine_walk(dmin, S, lo2, hi2, c0, true, c_last, u, &found);
  }
  if (lane == 0) *result = found;
}

// ---- cumulative-sum programs ----------------------------------------------
//
// The exact running value through the shard in three parallel passes and one
// short sequential one, instead of walk_kernel's block-by-block walk (which
// also stays, as the fallback):
//  seg_block_kernel  per block: the binade of every element's running value
//                    is guessed from an approximate prefix (approx[b] plus
//                    in-block sums).  An element whose guessed value stays in
//                    one binade joins the current run (a transfer, as above);
//                    one whose guessed value changes binade is a crossing,
//                    added exactly at evaluation.  The block becomes
//                    run x run x ... run (at most kKC crossings; more, or a
//                    guess that breaks a run, make it opaque: walked element
//                    by element at evaluation).
//  seg_plan_kernel   a segmented scan of the block tails over the blocks
//                    (segments start at blocks with crossings) and the
//                    shard's program: RUN / CROSS / FINE / MARK items, a few
//                    per crossing (~log2(c_last / c_first) of them).
//  seg_eval_kernel   one wave runs the program from the exact c_in.  A RUN
//                    applies when the running value is in its binade and
//                    stays there (N + D < 2^53), the transfer test above; a
//                    failed test is a wrong guess and the scan falls back to
//                    walk_kernel.
//  seg_fill_kernel   cend[b] from the value at the block's segment head and
//                    the scanned transfer.
// A program without FINE items is the shard's exact function c_in -> c_out:
// sharded seeding all-gathers the programs and every rank composes them
// (cdr_seed_program_eval) instead of a rank-ordered chain of scans.
// (Part, SeedItem and the Seg* records: seed_common.h.)

__device__ __forceinline__ Part shfl_up_part(const Part& P, int o) {
  return Part{__shfl_up(P.d0, o), __shfl_up(P.d1, o), __shfl_up(P.e, o), __shfl_up(P.st, o)};
}
__device__ __forceinline__ Part shfl_part(const Part& P, int l) {
  return Part{__shfl(P.d0, l), __shfl(P.d1, l), __shfl(P.e, l), __shfl(P.st, l)};
}

__device__ __forceinline__ int gbin(double c) {
  int e;
  long long N;
  return sp_binade(c, e, N) ? e : kNoE;
}

// A guessed running value within 2^-24 (relative) of its binade's edges: the
// exact value may sit on either side (a sequential fp64 sum of n terms is
// within n 2^-53 of the real sum, < 2^-24 for n < 2^29), so elements next to
// it are crossings, added exactly whatever the binade turns out to be.
__device__ __forceinline__ bool gnear(double c) {
  const unsigned long long m = __builtin_bit_cast(unsigned long long, c) & 0xFFFFFFFFFFFFFull;
  return m < (1ull << 28) || m > (1ull << 52) - (1ull << 28);
}

// One workgroup per block, one wave per 1024-element pass (8 waves); lane l
// of wave w owns elements [1024 w + 16 l, +16).  The passes are linked
// through LDS: their sums (the guessed running value at each pass start),
// their crossing counts (where each pass's entries go) and their tail runs
// (the run open at each pass start).
constexpr int kSegWaves = kSeedBlock / kPass;  // 8
__global__ __launch_bounds__(512) void seg_block_kernel(const double* __restrict__ dmin,
                                                        int64_t n, double S,
                                                        const double* __restrict__ approx,
                                                        int64_t nblocks,
                                                        SegTail* __restrict__ tails,
                                                        SegEnt* __restrict__ ents,
    SeedDev dv) {
  if (dv.S) S = dv.S[0];
  __shared__ double s_sum[kSegWaves];
  __shared__ int s_m[kSegWaves], s_bad[kSegWaves], s_h[kSegWaves];
  __shared__ Part s_t[kSegWaves];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t base = b * kSeedBlock;
  SegEnt* eb = ents + b * kKC;
  const int64_t lo = base + (int64_t)w * kPass + (int64_t)lane * 16;
  const int cnt = lo >= n ? 0 : (n - lo < 16 ? (int)(n - lo) : 16);
  // dmin is allocated to n_pad (a multiple of the block): whole lanes load
  double p[16];
  {
    const double2* src = reinterpret_cast<const double2*>(dmin + lo);
    double2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[j];
    // p = fl(dmin / S) by Markstein's correction from y = fl(1 / S): q0 =
    // fl(a y), r = a - S q0 (exact in one fma), fl(q0 + r y) is the correctly
    // rounded quotient (no underflow: a >= 2^-960, S < 2^1000; others divide).
    // 3 fp64 instructions per element instead of the ~11 of a division
    // (tools/markstein_div_fuzz.cpp: 3.2e8 quotients, none differs).
    const double y = 1.0 / S;
    const bool fastS = S < 0x1p1000;
    auto quo = [&](double a) {
      const double q0 = a * y;
      double q = fma(fma(-q0, S, a), y, q0);
      if (!(fastS && a >= 0x1p-960)) q = a / S;
      return q;
    };
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[2 * j] = 2 * j < cnt ? quo(v[j].x) : 0.0;
      p[2 * j + 1] = 2 * j + 1 < cnt ? quo(v[j].y) : 0.0;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += p[j];
  double inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_sum[w] = inc;
  __syncthreads();
  // guessed running value at each pass start: the same sequence in every wave
  double A = approx[b], Anext = 0.0;
  for (int v = 0; v <= w; ++v) {
    Anext = A + s_sum[v];
    if (v < w) A = Anext;
  }
  const double Aend = (b + 1 < nblocks) ? approx[b + 1] : -1.0;
  const double ex = __shfl_up(inc, 1);
  const double a0 = A + (lane ? ex : 0.0);
  double a1 = __shfl_down(a0, 1);
  if (lane == 63) a1 = (w == kSegWaves - 1 && Aend >= 0.0) ? Aend : Anext;
  // crossings under the guess
  unsigned xm = 0;
  {
    double cb = a0;
    int gb = gbin(cb);
    bool nb_ = gnear(cb);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < cnt) {
        const double ca = (j == cnt - 1) ? a1 : cb + p[j];
        const int ga = gbin(ca);
        const bool na = gnear(ca);
        if (gb == kNoE || ga != gb || nb_ || na) xm |= 1u << j;
        cb = ca;
        gb = ga;
        nb_ = na;
      }
    }
  }
  const int m = __popc(xm);
  int mi = m;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(mi, o);
    if (lane >= o) mi += t;
  }
  if (lane == 63) s_m[w] = mi;
  __syncthreads();
  int basew = 0, mtot = 0;
  for (int v = 0; v < kSegWaves; ++v) {
    if (v < w) basew += s_m[v];
    mtot += s_m[v];
  }
  const bool over = mtot > kKC;  // block-uniform
  Part Sx = part_empty();
  Part F = part_empty();
  double p0 = 0.0;
  bool bad = false;
  const int bl = basew + mi - m;  // this lane's first entry
  if (!over) {
    PartD cur = partd_empty();
    int jj = 0;
    double cb = a0;
    int gb = gbin(cb);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < cnt) {
        const double ca = (j == cnt - 1) ? a1 : cb + p[j];
        if ((xm >> j) & 1) {
          if (jj == 0) {
            F = to_part(cur);
            p0 = p[j];
          } else {
            eb[bl + jj] = SegEnt{to_part(cur), p[j]};
            bad |= cur.st == 2;
          }
          ++jj;
          cur = partd_empty();
        } else {
          partd_add(cur, p[j], gb);
        }
        cb = ca;
        gb = gbin(ca);
      }
    }
    // segmented inclusive scan of the lane tails (heads: lanes with a crossing)
    Sx = to_part(cur);
    int hs = m > 0;
    for (int o = 1; o < 64; o <<= 1) {
      const Part L = shfl_up_part(Sx, o);
      const int hl = __shfl_up(hs, o);
      if (lane >= o) {
        if (!hs) Sx = part_compose(L, Sx);
        hs |= hl;
      }
    }
  }
  const unsigned long long hm = __ballot(m > 0);
  const Part S63 = shfl_part(Sx, 63);
  if (lane == 0) {
    s_t[w] = S63;
    s_h[w] = hm != 0ull;
  }
  Part Sp = shfl_up_part(Sx, 1);
  if (lane == 0) Sp = part_empty();
  const int anybad = __ballot(bad) != 0ull;
  if (lane == 0) s_bad[w] = anybad;
  __syncthreads();
  // the run open at this pass's start: passes since the last one with a crossing
  Part open = part_empty();
  for (int v = 0; v < w; ++v) open = s_h[v] ? s_t[v] : part_compose(open, s_t[v]);
  bool badw = false;
  if (!over && m > 0) {
    const bool prevh = (hm & ((1ull << lane) - 1)) != 0;
    const Part pre = part_compose(prevh ? Sp : part_compose(open, Sp), F);
    eb[bl] = SegEnt{pre, p0};
    badw = pre.st == 2;
  }
  const int badf = __ballot(badw) != 0ull;
  __syncthreads();
  if (lane == 0 && badf) s_bad[w] = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    Part t = part_empty();
    int anyb = 0;
    for (int v = 0; v < kSegWaves; ++v) {
      t = s_h[v] ? s_t[v] : part_compose(t, s_t[v]);
      anyb |= s_bad[v];
    }
    const bool opq = over || anyb || t.st == 2;
    tails[b] = SegTail{t, opq ? 0 : mtot, opq ? 1 : 0};
  }
}

constexpr int kPlanT = 1024;
constexpr int64_t kItemCap = 1 << 16;  // program items per shard (more: fallback)

// Single workgroup: segmented scan of the block tails and the program.
__global__ __launch_bounds__(1024) void seg_plan_kernel(const SegTail* __restrict__ tails,
                                                        const SegEnt* __restrict__ ents,
                                                        int64_t nb, SegScan* __restrict__ scan,
                                                        SeedItem* __restrict__ items, int64_t cap,
                                                        long long* __restrict__ meta) {
  __shared__ Part sP[kPlanT];
  __shared__ int sH[kPlanT];
  __shared__ long long sI[kPlanT], sL[kPlanT], sF[kPlanT];
  const int t = threadIdx.x;
  const int64_t per = (nb + kPlanT - 1) / kPlanT;
  const int64_t lo = (int64_t)t * per;
  const int64_t hi = (lo + per) < nb ? (lo + per) : nb;
  // a thread's tails are loaded kPB at a time, the loads in flight together
  // (one at a time paid a memory latency per block: 60 us at 12 208 blocks)
  constexpr int kPB = 4;
  auto load_tails = [&](int64_t b0, SegTail (&T)[kPB]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kPB; ++j) T[j] = tails[b0 + j < hi ? b0 + j : lo];
  };
  {
    Part agg = part_empty();
    int hh = 0;
    long long ni = 0, lh = -1, nf = 0;
    for (int64_t b0 = lo; b0 < hi; b0 += kPB) {
      SegTail TT[kPB];
      load_tails(b0, TT);
#pragma unroll
      for (int j = 0; j < kPB; ++j) {
        const int64_t b = b0 + j;
        if (b >= hi) break;
        const SegTail& T = TT[j];
        if (T.ncross > 0 || T.opaque) {
          agg = T.opaque ? part_empty() : T.t;
          hh = 1;
          lh = b;
          ni += T.opaque ? 3 : 2 + 2 * (long long)T.ncross;
          nf += T.opaque;
        } else {
          agg = part_compose(agg, T.t);
        }
      }
    }
    sP[t] = agg;
    sH[t] = hh;
    sI[t] = ni;
    sL[t] = lh;
    sF[t] = nf;
  }
  __syncthreads();
  for (int o = 1; o < kPlanT; o <<= 1) {
    Part L = part_empty();
    int hl = 0;
    long long il = 0, ll = -1, fl = 0;
    if (t >= o) {
      L = sP[t - o];
      hl = sH[t - o];
      il = sI[t - o];
      ll = sL[t - o];
      fl = sF[t - o];
    }
    __syncthreads();
    if (t >= o) {
      if (!sH[t]) sP[t] = part_compose(L, sP[t]);
      sH[t] |= hl;
      sI[t] += il;
      if (ll > sL[t]) sL[t] = ll;
      sF[t] += fl;
    }
    __syncthreads();
  }
  Part run = t ? sP[t - 1] : part_empty();
  long long off = t ? sI[t - 1] : 0;
  long long lastH = t ? sL[t - 1] : -1;
  const long long total = sI[kPlanT - 1];
  const bool over = total + 2 > cap;
  for (int64_t b0 = lo; b0 < hi; b0 += kPB) {
    SegTail TT[kPB];
    load_tails(b0, TT);
#pragma unroll
    for (int jb = 0; jb < kPB; ++jb) {
      const int64_t b = b0 + jb;
      if (b >= hi) break;
      const SegTail& T = TT[jb];
      if (T.ncross > 0 || T.opaque) {
        if (!over) {
          items[off++] = run_item(run);
          if (T.opaque) {
            items[off++] = SeedItem{b, 0, 0.0, 0, kItFine};
          } else {
            for (int j = 0; j < T.ncross; ++j) {
              const SegEnt E = ents[b * kKC + j];
              items[off++] = run_item(E.pre);
              items[off++] = SeedItem{0, 0, E.p, 0, kItCross};
            }
          }
          items[off++] = SeedItem{b, 0, 0.0, 0, kItMark};
        }
        run = T.opaque ? part_empty() : T.t;
        lastH = b;
      } else {
        run = part_compose(run, T.t);
      }
      scan[b] = SegScan{run, lastH};
    }
  }
  if (t == 0) {
    if (!over) {
      items[total] = run_item(sP[kPlanT - 1]);
      items[total + 1] = SeedItem{0, 0, 0.0, 0, kItEnd};
    }
    meta[0] = total + 2;
    meta[1] = sF[kPlanT - 1];
    meta[2] = over ? 1 : 0;
  }
}

// Single wave: the program from the exact c_in.  Items are staged through
// LDS a window at a time (one round trip for the whole window); each item's
// fields go to scalar registers (readfirstlane) so the walk over the items is
// uniform scalar control flow with no per-item memory latency.
// res[0] = running value after the shard, res[1] = 1 when every item held.
constexpr int kEvalWin = 256;
__global__ __launch_bounds__(64) void seg_eval_kernel(const double* __restrict__ dmin, int64_t n,
                                                      double S,
                                                      const SeedItem* __restrict__ items,
                                                      const long long* __restrict__ meta,
                                                      double c_in, double* __restrict__ markc,
                                                      double* __restrict__ res,
    SeedDev dv) {
  if (dv.S) S = dv.S[0];
  if (dv.c_in) c_in = dv.c_in[0];
  __shared__ SeedItem sit[kEvalWin];
  const int lane = threadIdx.x;
  double c = c_in;
  bool ok = meta[2] == 0;
  const long long cnt = ok ? meta[0] : 0;
  int64_t dummy = -1;
  bool end = false;
  for (long long w0 = 0; ok && !end && w0 < cnt; w0 += kEvalWin) {
    const int m = (int)((cnt - w0) < kEvalWin ? (cnt - w0) : kEvalWin);
    __syncthreads();
    {
      const double4* src = reinterpret_cast<const double4*>(items + w0);
      double4* dst = reinterpret_cast<double4*>(sit);
      double4 v[kEvalWin / 64];
#pragma unroll
      for (int j = 0; j < kEvalWin / 64; ++j)
        if (j * 64 + lane < m) v[j] = src[j * 64 + lane];
#pragma unroll
      for (int j = 0; j < kEvalWin / 64; ++j)
        if (j * 64 + lane < m) dst[j * 64 + lane] = v[j];
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      const int kind = __builtin_amdgcn_readfirstlane(sit[i].kind);
      if (kind == kItEnd) {
        end = true;
        break;
      }
      if (kind == kItFine) {
        const int64_t lo = sgpr64(sit[i].d0) * kSeedBlock;
        const int64_t hi = (lo + kSeedBlock) < n ? (lo + kSeedBlock) : n;
        c = fine_walk(dmin, S, lo, hi, c, false, 1.0, 0.0, &dummy);
      } else if (kind == kItMark) {
        if (lane == 0) markc[sgpr64(sit[i].d0)] = c;
      } else {
        SeedItem it;
        it.kind = kind;
        it.e = __builtin_amdgcn_readfirstlane(sit[i].e);
        it.d0 = sgpr64(sit[i].d0);
        it.d1 = sgpr64(sit[i].d1);
        it.p = __builtin_bit_cast(double, sgpr64(__builtin_bit_cast(long long, sit[i].p)));
        if (!item_apply(it, c)) {
          ok = false;
          break;
        }
      }
    }
  }
  if (lane == 0) {
    res[0] = c;
    res[1] = ok ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void seg_fill_kernel(const SegScan* __restrict__ scan,
                                                       int64_t nb,
                                                       const double* __restrict__ markc,
                                                       const double* __restrict__ res,
                                                       double c_in, double* __restrict__ cend,
                                                       const double* __restrict__ c_in_dev) {
  if (res[1] == 0.0) return;
  if (c_in_dev) c_in = c_in_dev[0];
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const SegScan s = scan[b];
  const double c0 = s.lh < 0 ? c_in : markc[s.lh];
  double v = c0;
  if (s.s.st == 1) {
    int e;
    long long N;
    sp_binade(c0, e, N);
    v = sp_value(e, N + ((N & 1) ? s.s.d1 : s.s.d0));
  }
  cend[b] = v;
}

// The block-by-block walk (exact from any c_in; the fallback of the program).
// Device-resident mode (seed_run): dv carries S / gate, the running value at
// the end goes to dres_dev, and nothing is read back (c_out == nullptr).
static void seed_scan_walk(Ctx& c, double total, double c_in, double* c_out,
                           const SeedDev& dv = SeedDev{}, double* dres_dev = nullptr) {
  const int64_t nb = c.nblocks();
  c.xfer.ensure(sizeof(Xfer) * nb);
  c.cend.ensure(sizeof(double) * nb * 2);
  double* approx = c.cend.as<double>() + nb;
  hipLaunchKernelGGL(approx_prefix_kernel, dim3(1), dim3(1024), 0, c.stream,
                     c.blocksums.as<double>(), nb, total, c_in, approx, dv);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(xfer_kernel, dim3((int)ceil_div(nb, 4)), dim3(256), 0, c.stream,
                     c.dmin.as<double>(), c.n, total, approx, nb, c.xfer.as<Xfer>(), dv);
  HIP_CHECK(hipGetLastError());
  c.seed_scalar.ensure(sizeof(double) * (2 * c.d + 8));
  double* dres = dres_dev ? dres_dev : c.seed_scalar.as<double>() + c.d;
  static const bool want_stats = exp_env("CDR_SEED_STATS") != nullptr;
  long long* dstats = nullptr;
  if (want_stats) {
    static long long* ds = nullptr;
    if (!ds) {
      HIP_CHECK(hipMalloc(&ds, 8 * sizeof(long long)));
      HIP_CHECK(hipMemset(ds, 0, 8 * sizeof(long long)));
    }
    dstats = ds;
  }
  hipLaunchKernelGGL(walk_kernel, dim3(1), dim3(64), 0, c.stream, c.dmin.as<double>(), c.n,
                     total, c.xfer.as<Xfer>(), nb, c_in, c.cend.as<double>(), dres, dstats, dv);
  if (!c_out) {
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (want_stats) {
    long long hs[8];
    HIP_CHECK(hipMemcpyAsync(hs, dstats, sizeof(hs), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    fprintf(stderr,
            "seed walk stats (cumulative): rounds %lld single %lld fine %lld nb %lld "
            "fine_cycles %lld total_cycles %lld\n",
            hs[0], hs[1], hs[2], (long long)nb, hs[3], hs[4]);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(c_out, dres, sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.seed_c_in = c_in;
  c.seed_total = total;
  c.seed_scanned = true;
}

// This shard's cumsum program under the guess c_guess of the running value at
// its first element (seg_block_kernel, seg_plan_kernel).
void seed_scan_program(Ctx& c, double total, double c_guess, const SeedDev& dv) {
  const int64_t nb = c.nblocks();
  c.cend.ensure(sizeof(double) * nb * 2);
  double* approx = c.cend.as<double>() + nb;
  c.seg_tails.ensure(sizeof(SegTail) * nb);
  c.seg_ents.ensure(sizeof(SegEnt) * nb * kKC);
  c.seg_scan.ensure(sizeof(SegScan) * nb);
  c.seg_items.ensure(sizeof(SeedItem) * kItemCap);
  c.seg_meta.ensure(sizeof(long long) * 8);
  SeedDev dvs;  // the program is always built (no gate)
  dvs.S = dv.S;
  dvs.c_in = dv.c_in;
  hipLaunchKernelGGL(approx_prefix_kernel, dim3(1), dim3(1024), 0, c.stream,
                     c.blocksums.as<double>(), nb, total, c_guess, approx, dvs);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(seg_block_kernel, dim3((int)nb), dim3(kSegWaves * 64), 0, c.stream,
                     c.dmin.as<double>(), c.n, total, approx, nb, c.seg_tails.as<SegTail>(),
                     c.seg_ents.as<SegEnt>(), dvs);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(kPlanT), 0, c.stream,
                     c.seg_tails.as<SegTail>(), c.seg_ents.as<SegEnt>(), nb,
                     c.seg_scan.as<SegScan>(), c.seg_items.as<SeedItem>(), kItemCap,
                     c.seg_meta.as<long long>());
  HIP_CHECK(hipGetLastError());
  c.seed_prog_total = total;
  c.seed_prog_ready = true;
  ++c.seed_programs;
}

// Runs the program from the exact c_in and fills cend; false when a guess
// failed (nothing usable written).
// Device-resident mode: c_out == nullptr, nothing is read back (res[0] the
// running value, res[1] the success flag stay on the device).
bool seed_scan_finish(Ctx& c, double c_in, double* c_out, const SeedDev& dv) {
  const int64_t nb = c.nblocks();
  double* markc = c.cend.as<double>() + nb;  // the guesses are consumed
  double* res = seed_res(c);
  SeedDev dvs;
  dvs.S = dv.S;
  dvs.c_in = dv.c_in;
  hipLaunchKernelGGL(seg_eval_kernel, dim3(1), dim3(64), 0, c.stream, c.dmin.as<double>(), c.n,
                     c.seed_prog_total, c.seg_items.as<SeedItem>(), c.seg_meta.as<long long>(),
                     c_in, markc, res, dvs);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(seg_fill_kernel, dim3((int)ceil_div(nb, 256)), dim3(256), 0, c.stream,
                     c.seg_scan.as<SegScan>(), nb, markc, res, c_in, c.cend.as<double>(), dv.c_in);
  HIP_CHECK(hipGetLastError());
  if (!c_out) return true;
  double h[2];
  HIP_CHECK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  static const bool want_stats = exp_env("CDR_SEED_STATS") != nullptr;
  if (want_stats) {
    long long m[3];
    HIP_CHECK(hipMemcpy(m, c.seg_meta.p, sizeof(m), hipMemcpyDeviceToHost));
    fprintf(stderr, "seed program: items %lld fine %lld over %lld ok %d\n", m[0], m[1], m[2],
            h[1] != 0.0);
  }
  if (h[1] == 0.0) return false;
  *c_out = h[0];
  return true;
}

static void seed_scan_done(Ctx& c, double total, double c_in) {
  c.seed_c_in = c_in;
  c.seed_total = total;
  c.seed_scanned = true;
  c.seed_prog_ready = false;
}

void seed_scan(Ctx& c, double total, double c_in, double* c_out) {
  check_points(c);
  const int64_t nb = c.nblocks();
  if (nb == 0) {
    *c_out = c_in;
    return;
  }
  static const bool walk_only = exp_env("CDR_SEED_WALK") != nullptr;
  bool done = false;
  if (!walk_only) {
    seed_scan_program(c, total, c_in);
    done = seed_scan_finish(c, c_in, c_out);
    if (!done) ++c.seed_fallbacks;
  }
  if (!done) seed_scan_walk(c, total, c_in, c_out);
  seed_scan_done(c, total, c_in);
}

void seed_scan_begin(Ctx& c, double total, double c_guess, int64_t* n_items, int64_t* n_fine) {
  check_points(c);
  const int64_t nb = c.nblocks();
  c.seed_scanned = false;
  if (nb == 0) {
    *n_items = 0;
    *n_fine = 0;
    c.seed_prog_total = total;
    c.seed_prog_ready = true;
    return;
  }
  seed_scan_program(c, total, c_guess);
  long long m[3];
  HIP_CHECK(hipMemcpyAsync(m, c.seg_meta.p, sizeof(m), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  *n_items = m[2] ? -1 : m[0];
  *n_fine = m[1];
}

void seed_scan_items(Ctx& c, cdr_seed_item* out, int64_t cap, int64_t* n_items) {
  if (!c.seed_prog_ready) CDR_FAIL(CDR_ERR_STATE, "cdr_seed_scan_items before cdr_seed_scan_begin");
  const int64_t nb = c.nblocks();
  if (nb == 0) {
    *n_items = 0;
    return;
  }
  long long m[3];
  HIP_CHECK(hipMemcpyAsync(m, c.seg_meta.p, sizeof(m), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (m[2]) CDR_FAIL(CDR_ERR_UNSUPPORTED, "seed program over its item capacity");
  if (m[0] > cap) CDR_FAIL(CDR_ERR_ARG, "output capacity below the program's item count");
  HIP_CHECK(hipMemcpyAsync(out, c.seg_items.p, sizeof(SeedItem) * m[0], hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  *n_items = m[0];
}

void seed_scan_end(Ctx& c, double c_in, double* c_out) {
  if (!c.seed_prog_ready) CDR_FAIL(CDR_ERR_STATE, "cdr_seed_scan_end before cdr_seed_scan_begin");
  const double total = c.seed_prog_total;
  const int64_t nb = c.nblocks();
  if (nb == 0) {
    *c_out = c_in;
  } else if (!seed_scan_finish(c, c_in, c_out)) {
    ++c.seed_fallbacks;
    seed_scan_walk(c, total, c_in, c_out);
  }
  seed_scan_done(c, total, c_in);
}

void seed_search_enqueue(Ctx& c, double total, double c_in, double c_last, double u,
                         int64_t* out, const SeedDev& dv) {
  hipLaunchKernelGGL(search_kernel, dim3(1), dim3(64), 0, c.stream, c.dmin.as<double>(), c.n,
                     total, c.cend.as<double>(), c.nblocks(), c_in, c_last, u, out, dv);
  HIP_CHECK(hipGetLastError());
}

void seed_search(Ctx& c, double c_last, double u, int64_t* idx) {
  check_points(c);
  if (!c.seed_scanned) CDR_FAIL(CDR_ERR_STATE, "cdr_seed_search before cdr_seed_scan");
  const int64_t nb = c.nblocks();
  if (nb == 0) {
    *idx = -1;
    return;
  }
  c.seed_scalar.ensure(sizeof(double) * (c.d + 8));
  int64_t* dres = reinterpret_cast<int64_t*>(c.seed_scalar.as<double>() + c.d + 1);
  seed_search_enqueue(c, c.seed_total, c.seed_c_in, c_last, u, dres, SeedDev{});
  HIP_CHECK(hipMemcpyAsync(idx, dres, sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

void seed_step_resident(Ctx& c, const double* S, const double* u, int64_t* pick,
                        bool walk_only) {
  double* res = seed_res(c);
  SeedDev dv;
  dv.S = S;
  if (!walk_only) {
    seed_scan_program(c, 1.0, 0.0, dv);
    seed_scan_finish(c, 0.0, nullptr, dv);
    dv.gate = res + 1;  // the fallback runs only when the program failed
  } else {
    HIP_CHECK(hipMemsetAsync(res, 0, sizeof(double) * 2, c.stream));
  }
  seed_scan_walk(c, 1.0, 0.0, nullptr, dv, res);
  SeedDev ds;
  ds.S = S;
  ds.c_last = res;
  ds.u = u;
  seed_search_enqueue(c, 1.0, 0.0, 1.0, 0.5, pick, ds);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_seed_scan(cdr_ctx* h, double total, double c_in, double* c_out) {
  CDR_TRY
  if (!h || !c_out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  if (!(total > 0.0) || std::isinf(total)) CDR_FAIL(CDR_ERR_NAN, "Probabilities contain NaN");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_scan(h->c, total, c_in, c_out);
  CDR_CATCH
}

int cdr_seed_scan_begin(cdr_ctx* h, double total, double c_guess, int64_t* n_items,
                        int64_t* n_fine) {
  CDR_TRY
  if (!h || !n_items || !n_fine) CDR_FAIL(CDR_ERR_ARG, "null argument");
  if (!(total > 0.0) || std::isinf(total)) CDR_FAIL(CDR_ERR_NAN, "Probabilities contain NaN");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_scan_begin(h->c, total, c_guess, n_items, n_fine);
  CDR_CATCH
}

int cdr_seed_scan_items(cdr_ctx* h, cdr_seed_item* out, int64_t cap, int64_t* n_items) {
  CDR_TRY
  if (!h || !n_items || (!out && cap > 0)) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_scan_items(h->c, out, cap, n_items);
  CDR_CATCH
}

int cdr_seed_scan_end(cdr_ctx* h, double c_in, double* c_out) {
  CDR_TRY
  if (!h || !c_out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_scan_end(h->c, c_in, c_out);
  CDR_CATCH
}

int cdr_seed_stats(cdr_ctx* h, int64_t* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  out[0] = h->c.seed_programs;
  out[1] = h->c.seed_fallbacks;
  CDR_CATCH
}

int cdr_seed_program_eval(const cdr_seed_item* items, int64_t n_items, double c_in,
                          double* c_out, int32_t* ok) {
  CDR_TRY
  if (!c_out || !ok || (!items && n_items > 0) || n_items < 0)
    CDR_FAIL(CDR_ERR_ARG, "bad argument");
  double c = c_in;
  int32_t good = 1;
  for (int64_t i = 0; i < n_items && good; ++i) {
    SeedItem it;
    std::memcpy(&it, items + i, sizeof(it));
    if (it.kind == kItEnd) break;
    if (it.kind == kItFine || !item_apply(it, c)) good = 0;
  }
  *c_out = c;
  *ok = good;
  CDR_CATCH
}

int cdr_seed_search(cdr_ctx* h, double c_last, double u, int64_t* idx) {
  CDR_TRY
  if (!h || !idx) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_search(h->c, c_last, u, idx);
  CDR_CATCH
}

}  // extern "C"
