// seed_update.hip — the k-means++ D^2 update (src/kmeans_plusplus.py:14-18):
// dist_sq = min(dist_sq, norm(X - c)**2), exact (min is order free), and the
// pairwise sum of every 8192-element block of it.  seed_update picks the
// kernel:
//   F32X, d in {8, 16}    seed_update16c_kernel   fp16 certificate, compacted
//   F32X, d in {32, 64}   seed_update16_kernel    prune, then fp16 certificate
//   F32X, any other d     seed_update_kernel<float, d or 0>
//   F64                   seed_update_kernel<double, 0>
#include <algorithm>
#include <array>
#include <cmath>
#include <vector>

#include <hip/hip_fp16.h>

#include "cdr_internal.h"
#include "exact_math.h"
#include "seed_common.h"

namespace cdr {

void ensure_rowmajor(Ctx& c);  // screen32.hip: the row-major copy xa32

__global__ void fill_inf(double* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = INFINITY;
}

// One workgroup (256 threads) per 8192-point block.  The block is handled in
// two halves of 4096 (pw(8192) = pw(4096) + pw(4096)); each half's values sit
// in LDS (one pad slot per 16).
//
// Full blocks: the 32 pairwise leaves of 128 of a half are
// summed by 8 threads each — thread (leaf L, j) adds NumPy's accumulator r_j
// = a(j) + a(j + 8) + ... sequentially, shfl_xor 1, 2, 4 forms
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), shfl_xor 8, 16, 32 and
// then a 4-wave LDS step combine the leaves in the balanced tree of
// pw(4096).
// The one partial block (m < 8192) is the grid's last workgroup: it updates
// its dmin values with the others and leaves its pairwise sum to
// seed_tail_sum_kernel (a stack walk of the tree: scratch memory, kept out
// of this kernel).
// D > 0 (float points, d == D <= 16): each thread takes 4 points per
// iteration with all their 16-byte feature-quad loads and dmin loads issued
// before any arithmetic, and the NumPy-order distance unrolled for that d.
// Exact pruning of the running minimum (the k-means++ D^2 step,
// src/kmeans_plusplus.py:14-17): the point's nearest centre so far, c_a =
// near[i], is at distance r with dmin = fl(r^2); if the new centre is at
// least 2 r (1 + 2^-30) from c_a, the triangle inequality puts it at least
// r (1 + 2^-30) from the point, so its computed squared distance (NumPy
// order, relative error < 2^-45 at d <= 128) is >= dmin and min(dmin, .)
// leaves dmin unchanged bit for bit: the point is not read at all.
// ccd[j] = ||c_j - c_new|| (fp64, relative error < 2^-48).  dmin = +inf (no
// centre yet) never prunes.
__device__ __forceinline__ bool seed_prunable(double ccd_a, double dmin_old) {
  return ccd_a >= 2.0 * sqrt(dmin_old) * (1.0 + 0x1p-30);
}

// ccd[j] = ||cents[j] - cen|| for the j < count centres so far.
__global__ void seed_ccd_kernel(const double* __restrict__ cents, int count, int d,
                                const double* __restrict__ cen, double* __restrict__ ccd) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int f = 0; f < d; ++f) {
      const double t = cents[(size_t)j * d + f] - cen[f];
      s += t * t;
    }
    ccd[j] = sqrt(s);
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void seed_update_kernel(
    const T* __restrict__ X, int64_t n, int64_t n_pad, int d, const double* __restrict__ cen,
    double* __restrict__ dmin, double* __restrict__ blocksums, int32_t* __restrict__ near,
    const double* __restrict__ ccd, int cidx) {
  constexpr int kHalf = 4096;
  __shared__ double sdm[kHalf + kHalf / 16];
  __shared__ double swave[4];
  const int64_t b = blockIdx.x;
  const int64_t base = b * kSeedBlock;
  const int m = (n - base) < kSeedBlock ? (int)(n - base) : kSeedBlock;
  const bool TAIL = m < kSeedBlock;  // workgroup-uniform: the partial last block
  auto spos = [](int q) { return q + (q >> 4); };
  double halves[2] = {0.0, 0.0};
  for (int h = 0; h < 2; ++h) {
    if constexpr (D > 0) {
      constexpr int Q = (D + 3) / 4;
      // points per thread and iteration: all their loads issue before any
      // arithmetic (fewer for wide rows: registers)
      constexpr int U = D <= 16 ? 4 : (D <= 32 ? 2 : 1);
      // the centre in registers for narrow rows, else uniform (scalar) loads
      constexpr int CR = D <= 16 ? D : 1;
      typedef float f4v __attribute__((ext_vector_type(4)));
      const f4v* X4 = reinterpret_cast<const f4v*>(X);
      double cr[CR];
#pragma unroll
      for (int f = 0; f < CR; ++f) cr[f] = cen[f];
      for (int q0 = threadIdx.x; q0 < kHalf; q0 += U * 256) {
        f4v xv[U][Q];
        double old[U];
        bool go[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int qi = h * kHalf + q0 + 256 * u;
          const int64_t i = base + qi;
          go[u] = false;
          if (!TAIL || qi < m) {
            old[u] = dmin[i];
            go[u] = cidx == 0 || !seed_prunable(ccd[near[i]], old[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = base + h * kHalf + q0 + 256 * u;
          if (go[u]) {
#pragma unroll
            for (int qq = 0; qq < Q; ++qq) xv[u][qq] = X4[(int64_t)qq * n_pad + i];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int q = q0 + 256 * u;
          const int qi = h * kHalf + q;
          double v = 0.0;
          if (!TAIL || qi < m) {
            v = old[u];
            if (go[u]) {
              auto xf = [&](int f) { return (double)xv[u][f >> 2][f & 3]; };
              auto cf = [&](int f) { return D <= 16 ? cr[f < CR ? f : 0] : cen[f]; };
              const double R = np_sqdist(xf, cf, D);
              const double r = sqrt(R);
              const double t = r * r;
              if (t < old[u]) {
                v = t;
                dmin[base + qi] = t;
                near[base + qi] = cidx;
              }
            }
          }
          sdm[spos(q)] = v;
        }
      }
    } else {
      for (int q = threadIdx.x; q < kHalf; q += blockDim.x) {
        const int qi = h * kHalf + q;
        const int64_t i = base + qi;
        double v = 0.0;
        if (!TAIL || qi < m) {
          const double old = dmin[i];
          v = old;
          if (cidx == 0 || !seed_prunable(ccd[near[i]], old)) {
            auto xv = [&](int f) { return (double)X[xidx(X, f, i, n_pad)]; };
            auto cv = [&](int f) { return cen[f]; };
            const double R = np_sqdist(xv, cv, d);
            const double r = sqrt(R);
            const double t = r * r;
            if (t < old) {
              v = t;
              dmin[i] = t;
              near[i] = cidx;
            }
          }
        }
        sdm[spos(q)] = v;
      }
    }
    __syncthreads();
    if (!TAIL) {
      const int t = threadIdx.x;
      const int L = t >> 3, j = t & 7;
      double r = sdm[spos(128 * L + j)];
#pragma unroll
      for (int i = 1; i < 16; ++i) r = r + sdm[spos(128 * L + j + 8 * i)];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) r = r + __shfl_xor(r, o);
      if ((t & 63) == 0) swave[t >> 6] = r;
      __syncthreads();
      if (t == 0) halves[h] = (swave[0] + swave[1]) + (swave[2] + swave[3]);
      __syncthreads();
    }
  }
  if (!TAIL && threadIdx.x == 0) blocksums[b] = halves[0] + halves[1];
}

// ---- fp16-certified update (F32X points, d in {8, 16, 32, 64}) --------------
// A k-means++ step changes few minima: most points are farther from the new
// centre than from their nearest one.  A half-size copy proves that for most
// points without reading them in fp32: x16 = fp16 of xh = (x - mu) 2^tau
// (tau = sigma + 14, |xh| < 2^14), grouped by 8 features, [G][n_pad] x 16 B,
// with e16[i] >= ||xh_i - x16_i|| (computed exactly in fp64 when the copy is
// built, rounded up to fp16).  With ch = (c - mu) 2^tau rounded to fp32 (Ec >=
// ||ch32 - ch||), the fp32 a = ||x16_i - ch32|| has relative error below
// (D + 8) 2^-23, so
//     ||x_i - c|| >= (a (1 - (D + 8) 2^-23) - e16[i] - Ec) 2^-tau = r_lo,
// and r_lo^2 >= dmin (1 + 2^-30) proves the NumPy-order distance (relative
// error < 2^-45, as seed_prunable) is >= dmin: min(dmin, .) leaves it
// unchanged.  Only the points it cannot prove read the fp32 row and take the
// exact path; the triangle-inequality pruning (seed_prunable) runs first.
constexpr int kSeed16Tau = 14;

__global__ __launch_bounds__(256) void seed16_pack_kernel(const float* __restrict__ x32,
                                                          int64_t n, int64_t n_pad, int d,
                                                          const float* __restrict__ mu,
                                                          double scale,
                                                          uint4* __restrict__ x16,
                                                          unsigned short* __restrict__ e16) {
  const int G = (d + 7) / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += (int64_t)gridDim.x * blockDim.x) {
    double err = 0.0;
    for (int g = 0; g < G; ++g) {
      unsigned short hv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int f = 8 * g + j;
        double v = 0.0;
        if (f < d && i < n) v = ((double)x32[xidx(x32, f, i, n_pad)] - (double)mu[f]) * scale;
        const __half h = __float2half_rn((float)v);
        const double dv = v - (double)__half2float(h);
        err += dv * dv;
        hv[j] = __half_as_ushort(h);
      }
      uint4 w;
      w.x = hv[0] | ((unsigned)hv[1] << 16);
      w.y = hv[2] | ((unsigned)hv[3] << 16);
      w.z = hv[4] | ((unsigned)hv[5] << 16);
      w.w = hv[6] | ((unsigned)hv[7] << 16);
      x16[(int64_t)g * n_pad + i] = w;
    }
    // stored as fp16 rounded up (an upper bound; 2 bytes a point, not 4);
    // non-finite (an fp16 overflow) and anything past fp16's range is +inf,
    // which never certifies
    const double e = sqrt(err) * (1.0 + 0x1p-20) + 0x1p-60;
    unsigned short eb = 0x7C00u;
    if (isfinite(e) && e < 65504.0) {
      const __half h = __float2half_rn((float)e);
      eb = __half_as_ushort(h);
      if ((double)__half2float(h) < e) ++eb;  // the next fp16 up (e > 0)
    }
    e16[i] = eb;
  }
}

// The centre in the copy's coordinates: ch = fp32 of (c - mu) 2^tau and Ec >=
// ||ch - (c - mu) 2^tau|| (rounded up), from the device copy of the centre.
__global__ void seed_ch_kernel(const double* __restrict__ cen, const float* __restrict__ mu,
                               int d, double scale, float* __restrict__ ch,
                               float* __restrict__ Ec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ec = 0.0;
  for (int f = 0; f < d; ++f) {
    const double v = (cen[f] - (double)mu[f]) * scale;
    const float h = (float)v;
    ch[f] = h;
    const double r = v - (double)h;
    ec += r * r;
  }
  Ec[0] = (float)(sqrt(ec) * (1.0 + 0x1p-20) + 0x1p-60);
}

// Wide rows (D = 32, 64): the triangle-inequality pruning (seed_prunable)
// first, so that a pruned point does not read its copy.  (For d <= 16 the
// dependent near / ccd loads cost more than the 32-byte copy they save:
// seed_update16c_kernel loads dmin and the copy in one round trip instead.)
template <int D>
__global__ __launch_bounds__(256) void seed_update16_kernel(
    const float* __restrict__ X, const uint4* __restrict__ x16, const unsigned short* __restrict__ e16,
    int64_t n, int64_t n_pad, const double* __restrict__ cen, const float* __restrict__ ch,
    const float* __restrict__ Ecp, double rscale, double* __restrict__ dmin,
    double* __restrict__ blocksums,
    int32_t* __restrict__ near, const double* __restrict__ ccd, int cidx) {
  constexpr int kHalf = 4096;
  constexpr int G = (D + 7) / 8;
  constexpr int Q = (D + 3) / 4;
  static_assert(D == 32 || D == 64, "narrower rows take seed_update16c_kernel");
  constexpr int U = D <= 32 ? 2 : 1;
  constexpr float kRel = 1.0f - (float)(D + 8) * 0x1p-23f;
  const float Ec = Ecp[0];
  __shared__ double sdm[kHalf + kHalf / 16];
  __shared__ double swave[4];
  const int64_t b = blockIdx.x;
  const int64_t base = b * kSeedBlock;
  const int m = (n - base) < kSeedBlock ? (int)(n - base) : kSeedBlock;
  const bool TAIL = m < kSeedBlock;
  auto spos = [](int q) { return q + (q >> 4); };
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v* X4 = reinterpret_cast<const f4v*>(X);
  double halves[2] = {0.0, 0.0};
  for (int h = 0; h < 2; ++h) {
    for (int q0 = threadIdx.x; q0 < kHalf; q0 += U * 256) {
      double old[U];
      bool go[U];
      uint4 hv[U][G];
      float ev[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int qi = h * kHalf + q0 + 256 * u;
        const int64_t i = base + qi;
        go[u] = false;
        old[u] = 0.0;
        if (qi < m) {
          old[u] = dmin[i];
          go[u] = cidx == 0 || !seed_prunable(ccd[near[i]], old[u]);
        }
      }
      // the fp16 certificate
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + h * kHalf + q0 + 256 * u;
        if (go[u]) {
#pragma unroll
          for (int g = 0; g < G; ++g) hv[u][g] = x16[(int64_t)g * n_pad + i];
          ev[u] = __half2float(__ushort_as_half(e16[i]));
        }
      }
      bool need[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        need[u] = go[u];
        if (go[u] && cidx > 0) {
          float s = 0.0f;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const unsigned w[4] = {hv[u][g].x, hv[u][g].y, hv[u][g].z, hv[u][g].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (8 * g + j < D) {
                const float xv = __half2float(
                    __ushort_as_half((unsigned short)(w[j >> 1] >> (16 * (j & 1)))));
                const float t = xv - ch[8 * g + j];
                s = fmaf(t, t, s);
              }
            }
          }
          const float lo = sqrtf(s) * kRel - ev[u] - Ec;
          if (lo > 0.0f) {
            const double r = (double)lo * rscale;
            need[u] = !(r * r >= old[u] * (1.0 + 0x1p-30));
          }
        }
      }
      // the exact path for the points left
      f4v xv[U][Q];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + h * kHalf + q0 + 256 * u;
        if (need[u]) {
#pragma unroll
          for (int qq = 0; qq < Q; ++qq) xv[u][qq] = X4[(int64_t)qq * n_pad + i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = q0 + 256 * u;
        const int qi = h * kHalf + q;
        double v = old[u];
        if (need[u]) {
          auto xf = [&](int f) { return (double)xv[u][f >> 2][f & 3]; };
          auto cf = [&](int f) { return cen[f]; };
          const double R = np_sqdist(xf, cf, D);
          const double r = sqrt(R);
          const double t = r * r;
          if (t < old[u]) {
            v = t;
            dmin[base + qi] = t;
            near[base + qi] = cidx;
          }
        }
        sdm[spos(q)] = qi < m ? v : 0.0;
      }
    }
    __syncthreads();
    if (!TAIL) {
      const int t = threadIdx.x;
      const int L = t >> 3, j = t & 7;
      double r = sdm[spos(128 * L + j)];
#pragma unroll
      for (int i = 1; i < 16; ++i) r = r + sdm[spos(128 * L + j + 8 * i)];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) r = r + __shfl_xor(r, o);
      if ((t & 63) == 0) swave[t >> 6] = r;
      __syncthreads();
      if (t == 0) halves[h] = (swave[0] + swave[1]) + (swave[2] + swave[3]);
      __syncthreads();
    }
  }
  if (!TAIL && threadIdx.x == 0) blocksums[b] = halves[0] + halves[1];
}

// The update with the block's pairwise tree kept in registers (d = 8 and 16;
// the exact path's rows come from the row-major copy xa32).  One
// 512-thread workgroup per 8192-row block; thread (half h, leaf L, j) owns
// NumPy's accumulator j of the 128-element leaf L of half h, i.e. the rows
// 128 L + j + 8 i (i = 0 .. 15), and adds its 16 updated minima in NumPy's
// order (r = v_0, then r += v_i) from registers: no LDS staging of the
// half's 4096 values (34 KB per workgroup capped seed_update16_kernel at 4
// workgroups per CU) and no transposed re-read.  Accumulators combine by
// shuffles ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and the leaves
// and waves by the same perfect tree, exactly seed_update16_kernel's sums.
// A wave's load instruction reads 8 runs of 8 consecutive rows (64 B of
// dmin, 128 B of each copy group).  Rows are taken 4 per batch, the batch's
// loads issued together; the fp32 row is read only where the fp16
// certificate cannot prove the minimum unchanged.
// The exact path is compacted per wave (round 6).  PMC put the previous form
// (each batch gathering its uncertified rows in place) at TD 97 % / TA 81 %
// busy with 44K vector-memory instructions per CU and launch, ~19K of them
// the exact path's row gathers: a batch ran them whenever any lane of the
// wave could not certify a row, with one or two lanes active.  Here phase 1 streams every row of the thread (certificate
// only) and keeps its 16 current minima in registers with a 16-bit mask of
// the rows left; phase 2 lists the wave's (lane, row) pairs in LDS and
// evaluates them 64 at a time, one per lane (a full-width gather); phase 3
// adds the thread's 16 values in NumPy's order as before.  Same values, same
// order: dmin, near and the block sums are bit-identical.  1.15 -> 1.08 ms per
// launch on average at config 3 (the converged steps stay ~0.91 ms: the
// streamed 42 B per row at ~4.8 TB/s), seeding 0.1075 -> 0.1055 s.
template <int D>
__global__ __launch_bounds__(512) void seed_update16c_kernel(
    const float* __restrict__ XA, const uint4* __restrict__ x16, const unsigned short* __restrict__ e16,
    int64_t n, int64_t n_pad, const double* __restrict__ cen, const float* __restrict__ ch,
    const float* __restrict__ Ecp, double rscale, double* __restrict__ dmin,
    double* __restrict__ blocksums, int32_t* __restrict__ near, int cidx) {
  constexpr int G = (D + 7) / 8;
  constexpr int Q = (D + 3) / 4;
  constexpr int kB = D <= 8 ? 4 : 2;
  constexpr float kRel = 1.0f - (float)(D + 8) * 0x1p-23f;
  constexpr int kCap = 256;  // exact rows per wave and round
  __shared__ double swave[8];
  __shared__ unsigned short slist[8][kCap];
  __shared__ double supd[8][kCap];
  const float Ec = Ecp[0];
  const int64_t b = blockIdx.x;
  const int64_t base = b * kSeedBlock;
  const int m = (n - base) < kSeedBlock ? (int)(n - base) : kSeedBlock;
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int h = t >> 8, L = (t >> 3) & 31, j = t & 7;
  const int r0 = h * 4096 + 128 * L + j;  // row of i = 0 (row of i: r0 + 8 i)
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v* XA4 = reinterpret_cast<const f4v*>(XA);
  float chv[D];
#pragma unroll
  for (int f = 0; f < D; ++f) chv[f] = ch[f];
  struct SB {
    double old[kB];
    uint4 hv[kB][G];
    float ev[kB];
  };
  auto sload = [&](SB& sb, int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      const int r = r0 + 8 * (i0 + u);
      const int64_t i = base + (r < m ? r : 0);
      sb.old[u] = dmin[i];
#pragma unroll
      for (int g = 0; g < G; ++g) sb.hv[u][g] = x16[(int64_t)g * n_pad + i];
      sb.ev[u] = __half2float(__ushort_as_half(e16[i]));
    }
  };
  // phase 1: the certificate over the thread's 16 rows
  double ov[16];
  unsigned nm = 0;
  if (cidx == 0) {
    // the first centre: every minimum is +inf, nothing to certify - the
    // exact distances straight from the rows, 4 rows' loads in flight (not
    // the stream of copies and bounds plus a list of every row)
#pragma unroll
    for (int i0 = 0; i0 < 16; i0 += 4) {
      f4v xv[4][Q];
      double old[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + 8 * (i0 + u);
        const int64_t row = base + (r < m ? r : 0);
        old[u] = dmin[row];
#pragma unroll
        for (int qq = 0; qq < Q; ++qq) xv[u][qq] = XA4[row * Q + qq];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + 8 * (i0 + u);
        double v = 0.0;
        if (r < m) {
          auto xf = [&](int f) { return (double)xv[u][f >> 2][f & 3]; };
          auto cf = [&](int f) { return cen[f]; };
          const double R = np_sqdist(xf, cf, D);
          const double rt = sqrt(R);
          const double tt = rt * rt;
          v = old[u];
          if (tt < old[u]) {
            v = tt;
            dmin[base + r] = tt;
            near[base + r] = cidx;
          }
        }
        ov[i0 + u] = v;
      }
    }
  } else {
    SB sbuf[2];
    sload(sbuf[0], 0);
#pragma unroll
    for (int bi = 0; bi < 16 / kB; ++bi) {
      const int i0 = bi * kB;
      if (bi + 1 < 16 / kB) sload(sbuf[(bi + 1) & 1], i0 + kB);
      const SB& sb = sbuf[bi & 1];
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const bool in = r0 + 8 * (i0 + u) < m;
        bool need = in;
        if (in && cidx > 0) {
          float sacc = 0.0f;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const unsigned w[4] = {sb.hv[u][g].x, sb.hv[u][g].y, sb.hv[u][g].z, sb.hv[u][g].w};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              if (8 * g + q < D) {
                const float xv = __half2float(
                    __ushort_as_half((unsigned short)(w[q >> 1] >> (16 * (q & 1)))));
                const float dd = xv - chv[8 * g + q];
                sacc = fmaf(dd, dd, sacc);
              }
            }
          }
          const float lo = sqrtf(sacc) * kRel - sb.ev[u] - Ec;
          if (lo > 0.0f) {
            const double rr = (double)lo * rscale;
            need = !(rr * rr >= sb.old[u] * (1.0 + 0x1p-30));
          }
        }
        ov[i0 + u] = in ? sb.old[u] : 0.0;
        if (need) nm |= 1u << (i0 + u);
      }
    }
  }
  // phase 2: the wave's uncertified rows, one per lane
  const int cnt = __popc(nm);
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  const int total = __shfl(incl, 63);
  const int myoff = incl - cnt;
  for (int e0 = 0; e0 < total; e0 += kCap) {  // (wave-uniform)
    {
      unsigned mm = nm;
      int e = myoff;
      while (mm) {
        const int i = __builtin_ctz(mm);
        mm &= mm - 1u;
        if (e >= e0 && e < e0 + kCap) slist[wv][e - e0] = (unsigned short)((lane << 4) | i);
        ++e;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int nr = total - e0 < kCap ? total - e0 : kCap;
    for (int k0 = 0; k0 < nr; k0 += 64) {
      const int k = k0 + lane;
      if (k < nr) {
        const int ent = slist[wv][k];
        const int ts = wv * 64 + (ent >> 4), i = ent & 15;
        const int64_t row =
            base + (ts >> 8) * 4096 + 128 * ((ts >> 3) & 31) + (ts & 7) + 8 * i;
        f4v xv[Q];
#pragma unroll
        for (int qq = 0; qq < Q; ++qq) xv[qq] = XA4[row * Q + qq];
        const double old = dmin[row];
        auto xf = [&](int f) { return (double)xv[f >> 2][f & 3]; };
        auto cf = [&](int f) { return cen[f]; };
        const double R = np_sqdist(xf, cf, D);
        const double rt = sqrt(R);
        const double tt = rt * rt;
        double v = old;
        if (tt < old) {
          v = tt;
          dmin[row] = tt;
          near[row] = cidx;
        }
        supd[wv][k] = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if ((nm >> i) & 1u) {
        const int e = myoff + __popc(nm & ((1u << i) - 1u));
        if (e >= e0 && e < e0 + kCap) ov[i] = supd[wv][e - e0];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (m < kSeedBlock) return;  // the partial last block: seed_tail_sum_kernel sums it
  // phase 3: NumPy's accumulator j of its leaf: r = v_0, then r += v_i
  double acc = ov[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) acc = acc + ov[i];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) acc = acc + __shfl_xor(acc, o);
  if ((t & 63) == 0) swave[t >> 6] = acc;
  __syncthreads();
  if (t == 0)
    blocksums[b] = ((swave[0] + swave[1]) + (swave[2] + swave[3])) +
                   ((swave[4] + swave[5]) + (swave[6] + swave[7]));
}

// The partial last block's pairwise sum (m < 8192 elements at base): its
// pairwise tree depends on m alone, so the host lays it out once
// (seed_tail_plan): the leaves' (offset, length) pairs, then the internal
// nodes grouped by height (node ids: leaves 0..L-1, internal nodes L.. in
// height order; each internal node = (left id, right id)).  The block is
// staged in LDS with coalesced loads, the leaves are summed in parallel, and
// each height's nodes are added in parallel (<= 7 heights for m < 8192).
// Its dmin values come from the seed_update_kernel launch before it (the
// block is that grid's last workgroup, updated with the other blocks).
constexpr int kTailLeaves = 160;
constexpr int kTailHeights = 16;
__global__ __launch_bounds__(256) void seed_tail_sum_kernel(const double* __restrict__ dmin,
                                                            int64_t b,
                                                            const int* __restrict__ plan,
                                                            int nleaves, int nheights,
                                                            double* __restrict__ blocksums) {
  __shared__ double snode[2 * kTailLeaves];
  __shared__ double sv[kSeedBlock];
  const int64_t base = b * kSeedBlock;
  const int t = threadIdx.x;
  {
    // the whole block, coalesced, 32 loads per thread in flight (dmin is
    // allocated to n_pad: padding slots load, the leaves never read them)
    double v[kSeedBlock / 256];
#pragma unroll
    for (int j = 0; j < kSeedBlock / 256; ++j) v[j] = dmin[base + j * 256 + t];
#pragma unroll
    for (int j = 0; j < kSeedBlock / 256; ++j) sv[j * 256 + t] = v[j];
  }
  __syncthreads();
  if (t < nleaves) {
    const int off = plan[2 * t], len = plan[2 * t + 1];
    snode[t] = np_pw_leaf([&](int i) { return sv[off + i]; }, len);
  }
  const int* hstart = plan + 2 * nleaves;  // nheights + 1 entries
  const int* nodes = hstart + nheights + 1;
  for (int h = 0; h < nheights; ++h) {
    __syncthreads();
    const int a = hstart[h] + t;
    if (a < hstart[h + 1]) snode[nleaves + a] = snode[nodes[2 * a]] + snode[nodes[2 * a + 1]];
  }
  __syncthreads();
  if (t == 0) blocksums[b] = snode[nleaves > 1 ? nleaves + hstart[nheights] - 1 : 0];
}

void seed_reset(Ctx& c) {
  check_points(c);
  c.dmin.ensure(sizeof(double) * c.n_pad);
  hipLaunchKernelGGL(fill_inf, dim3(1024), dim3(256), 0, c.stream, c.dmin.as<double>(), c.n_pad);
  HIP_CHECK(hipGetLastError());
  c.seed_near.ensure(sizeof(int32_t) * c.n_pad);
  HIP_CHECK(hipMemsetAsync(c.seed_near.p, 0, sizeof(int32_t) * c.n_pad, c.stream));
  c.seed_count = 0;
  c.seed_scanned = false;
}

// Append the new centre (device copy in seed_scalar) to the centre list and
// compute its distances to the earlier ones (the pruning table).
static void seed_track(Ctx& c) {
  const int d = c.d;
  const size_t need = sizeof(double) * (size_t)(c.seed_count + 1) * d;
  if (c.seed_cents.bytes < need) {
    DevBuf grown;
    grown.ensure(std::max(need, 2 * c.seed_cents.bytes));
    if (c.seed_count > 0)
      HIP_CHECK(hipMemcpyAsync(grown.p, c.seed_cents.p, sizeof(double) * (size_t)c.seed_count * d,
                               hipMemcpyDeviceToDevice, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    c.seed_cents.release();
    c.seed_cents = grown;
    grown.p = nullptr;
    grown.bytes = 0;
  }
  c.seed_ccd.ensure(sizeof(double) * (size_t)(c.seed_count + 1));
  if (c.seed_count > 0)
    hipLaunchKernelGGL(seed_ccd_kernel, dim3((c.seed_count + 255) / 256), dim3(256), 0, c.stream,
                       c.seed_cents.as<double>(), c.seed_count, d, c.seed_scalar.as<double>(),
                       c.seed_ccd.as<double>());
  HIP_CHECK(hipMemcpyAsync(c.seed_cents.as<double>() + (size_t)c.seed_count * d,
                           c.seed_scalar.p, sizeof(double) * d, hipMemcpyDeviceToDevice,
                           c.stream));
}

// NumPy's pairwise tree over m elements (np_pairwise): leaves of <= 128, split
// at n/2 rounded down to a multiple of 8.  Returns the node's height (leaves
// 0); internal nodes are collected as (height, left, right) with leaf ids
// and internal ids (-1 - index into `inner`).
static int pw_layout(int64_t off, int64_t m, std::vector<int>& leaves,
                     std::vector<std::array<int, 3>>& inner, int& id) {
  if (m <= 128) {
    id = (int)leaves.size() / 2;
    leaves.push_back((int)off);
    leaves.push_back((int)m);
    return 0;
  }
  int64_t m2 = m / 2;
  m2 -= m2 % 8;
  int l, r;
  const int hl = pw_layout(off, m2, leaves, inner, l);
  const int hr = pw_layout(off + m2, m - m2, leaves, inner, r);
  const int h = 1 + (hl > hr ? hl : hr);
  inner.push_back({h, l, r});
  id = -(int)inner.size();  // internal node -1 - index
  return h;
}

static void seed_tail_plan(Ctx& c, int64_t m) {
  if (c.seed_tail_m == m) return;
  std::vector<int> leaves;
  std::vector<std::array<int, 3>> inner;
  int root;
  const int H = pw_layout(0, m, leaves, inner, root);
  const int nl = (int)leaves.size() / 2;
  if (nl > kTailLeaves || H > kTailHeights)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "pairwise tail layout too large");
  // internal nodes in height order; ids: leaves 0..nl-1, internal nl + rank
  std::vector<int> order(inner.size()), rank(inner.size());
  for (size_t i = 0; i < inner.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return inner[a][0] < inner[b][0]; });
  for (size_t r = 0; r < order.size(); ++r) rank[order[r]] = (int)r;
  auto nid = [&](int x) { return x >= 0 ? x : nl + rank[-1 - x]; };
  std::vector<int> plan(leaves);
  std::vector<int> hstart(H + 1, 0);
  for (int h = 1, r = 0; h <= H; ++h) {
    hstart[h - 1] = r;
    while (r < (int)order.size() && inner[order[r]][0] == h) ++r;
    hstart[h] = r;
  }
  plan.insert(plan.end(), hstart.begin(), hstart.end());
  for (int r : order) {
    plan.push_back(nid(inner[r][1]));
    plan.push_back(nid(inner[r][2]));
  }
  c.seed_tail_plan.ensure(sizeof(int) * plan.size());
  HIP_CHECK(hipMemcpy(c.seed_tail_plan.p, plan.data(), sizeof(int) * plan.size(),
                      hipMemcpyHostToDevice));
  c.seed_tail_nleaves = nl;
  c.seed_tail_nheights = H;
  c.seed_tail_m = m;
}

// The fp16-certified update of an F32X point set with d in {8, 16, 32, 64}:
// the half-size copy (built once per point set), the centre in its
// coordinates, then the kernel for that d.
static void seed_update_certified(Ctx& c, int64_t nb) {
  const int d = c.d;
  const int tau = c.sigma + kSeed16Tau;
  const int G = (d + 7) / 8;
  if (!c.seed16_valid) {
    c.seed_x16.ensure(sizeof(uint4) * (size_t)G * c.n_pad);
    c.seed_e16.ensure(sizeof(unsigned short) * c.n_pad);
    c.seed_mu.ensure(sizeof(float) * d);
    HIP_CHECK(hipMemcpyAsync(c.seed_mu.p, c.mu.data(), sizeof(float) * d,
                             hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(seed16_pack_kernel, dim3(4096), dim3(256), 0, c.stream,
                       c.x32.as<float>(), c.n, c.n_pad, d, c.seed_mu.as<float>(),
                       std::ldexp(1.0, tau), c.seed_x16.as<uint4>(), c.seed_e16.as<unsigned short>());
    HIP_CHECK(hipGetLastError());
    c.seed16_valid = true;
  }
  // the centre in the copy's coordinates (fp32) and its rounding error
  float* dch = reinterpret_cast<float*>(c.seed_scalar.as<double>() + d + 8);
  float* dEc = dch + d;
  hipLaunchKernelGGL(seed_ch_kernel, dim3(1), dim3(64), 0, c.stream,
                     c.seed_scalar.as<double>(), c.seed_mu.as<float>(), d,
                     std::ldexp(1.0, tau), dch, dEc);
  int32_t* near = c.seed_near.as<int32_t>();
  const int cidx = c.seed_count;
  if (d <= 16) {
    // the pairwise tree in registers; the exact path's rows from the
    // row-major copy (built once per point set; the bounded Lloyd screen
    // gathers from it too)
    ensure_rowmajor(c);
    hipLaunchKernelGGL(d == 8 ? seed_update16c_kernel<8> : seed_update16c_kernel<16>,
                       dim3(nb), dim3(512), 0, c.stream, c.xa32.as<float>(),
                       c.seed_x16.as<uint4>(), c.seed_e16.as<unsigned short>(), c.n, c.n_pad,
                       c.seed_scalar.as<double>(), dch, dEc, std::ldexp(1.0, -tau),
                       c.dmin.as<double>(), c.blocksums.as<double>(), near, cidx);
  } else {
    hipLaunchKernelGGL(d == 32 ? seed_update16_kernel<32> : seed_update16_kernel<64>,
                       dim3(nb), dim3(256), 0, c.stream, c.x32.as<float>(),
                       c.seed_x16.as<uint4>(), c.seed_e16.as<unsigned short>(), c.n, c.n_pad,
                       c.seed_scalar.as<double>(), dch, dEc, std::ldexp(1.0, -tau),
                       c.dmin.as<double>(), c.blocksums.as<double>(), near,
                       c.seed_ccd.as<double>(), cidx);
  }
}

// cen: the new centre on the host, or nullptr when seed_run has already put
// it at the start of c.seed_scalar on the device.
void seed_update(Ctx& c, const double* cen) {
  check_points(c);
  if (!c.dmin.p) seed_reset(c);
  const int64_t nb = c.nblocks();
  c.blocksums.ensure(sizeof(double) * (nb > 0 ? nb : 1));
  c.seed_scalar.ensure(sizeof(double) * (2 * c.d + 8));
  if (cen)
    HIP_CHECK(hipMemcpyAsync(c.seed_scalar.p, cen, sizeof(double) * c.d, hipMemcpyHostToDevice,
                             c.stream));
  if (!c.seed_near.p) {  // dmin from an earlier session without the tracking buffers
    c.seed_near.ensure(sizeof(int32_t) * c.n_pad);
    HIP_CHECK(hipMemsetAsync(c.seed_near.p, 0, sizeof(int32_t) * c.n_pad, c.stream));
  }
  seed_track(c);
  const int d = c.d;
  if (nb > 0) {
    if (c.mode == CDR_MODE_F32X && (d == 8 || d == 16 || d == 32 || d == 64)) {
      seed_update_certified(c, nb);
    } else if (c.mode == CDR_MODE_F32X) {
      // the distance unrolled for d < 16 (8: the certified update above)
      typedef void (*SeedFn)(const float*, int64_t, int64_t, int, const double*, double*,
                             double*, int32_t*, const double*, int);
#define CDR_SU(D_) seed_update_kernel<float, D_>
      static const SeedFn fns[16] = {CDR_SU(0),  CDR_SU(1),  CDR_SU(2),  CDR_SU(3),
                                     CDR_SU(4),  CDR_SU(5),  CDR_SU(6),  CDR_SU(7),
                                     nullptr,    CDR_SU(9),  CDR_SU(10), CDR_SU(11),
                                     CDR_SU(12), CDR_SU(13), CDR_SU(14), CDR_SU(15)};
#undef CDR_SU
      hipLaunchKernelGGL(fns[d < 16 ? d : 0], dim3(nb), dim3(256), 0, c.stream,
                         c.x32.as<float>(), c.n, c.n_pad, d, c.seed_scalar.as<double>(),
                         c.dmin.as<double>(), c.blocksums.as<double>(),
                         c.seed_near.as<int32_t>(), c.seed_ccd.as<double>(), c.seed_count);
    } else {
      hipLaunchKernelGGL((seed_update_kernel<double, 0>), dim3(nb), dim3(256), 0, c.stream,
                         c.x64.as<double>(), c.n, c.n_pad, d, c.seed_scalar.as<double>(),
                         c.dmin.as<double>(), c.blocksums.as<double>(),
                         c.seed_near.as<int32_t>(), c.seed_ccd.as<double>(), c.seed_count);
    }
    HIP_CHECK(hipGetLastError());
  }
  // the partial last block's pairwise sum (its dmin values are updated above)
  const int64_t nfull = c.n / kSeedBlock;
  if (nb > nfull) {
    seed_tail_plan(c, c.n - nfull * kSeedBlock);
    hipLaunchKernelGGL(seed_tail_sum_kernel, dim3(1), dim3(256), 0, c.stream,
                       c.dmin.as<double>(), nfull, c.seed_tail_plan.as<int>(),
                       c.seed_tail_nleaves, c.seed_tail_nheights, c.blocksums.as<double>());
    HIP_CHECK(hipGetLastError());
  }
  c.seed_count += 1;
  c.seed_scanned = false;
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_seed_reset(cdr_ctx* h) {
  CDR_TRY
  if (!h) CDR_FAIL(CDR_ERR_ARG, "null ctx");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_reset(h->c);
  CDR_CATCH
}

int cdr_seed_update(cdr_ctx* h, const double* c) {
  CDR_TRY
  if (!h || !c) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  seed_update(h->c, c);
  CDR_CATCH
}

int cdr_seed_num_blocks(cdr_ctx* h, int64_t* nblocks) {
  CDR_TRY
  if (!h || !nblocks) CDR_FAIL(CDR_ERR_ARG, "null argument");
  *nblocks = h->c.nblocks();
  CDR_CATCH
}

int cdr_seed_block_sums(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  const int64_t nb = c.nblocks();
  if (nb > 0) {
    HIP_CHECK(hipMemcpyAsync(out, c.blocksums.p, sizeof(double) * nb, hipMemcpyDeviceToHost,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }
  CDR_CATCH
}

}  // extern "C"
