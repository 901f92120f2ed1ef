// screen_big_sums.hip — the sums of the large-k Lloyd step (screen_big.hip):
// the exact int64 (k, d+1) sums and counts of the labels, by a full pass over
// the points or, on a DELTA step, from the moves the levels recorded.
#include <cmath>

#include "screen_big.h"

namespace cdr {

namespace {

// Sums per (cluster, feature) of features [FG g, FG g + FG) from the labels,
// blockIdx.y = g; each workgroup takes a contiguous point range.  The LDS
// table [FG][k] is exact (fp64 of grid values, |sum| < 2^53 grid units);
// it is added to out (k, d+1) int64 as x 2^S with atomics; g = 0 also counts.
template <int FG>
__global__ __launch_bounds__(1024) void update_big(const float* __restrict__ X, int64_t n,
                                                   int64_t n_pad, int d, int k,
                                                   const int32_t* __restrict__ labels,
                                                   double fx, unsigned long long* __restrict__ out,
                                                   const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* tsum = reinterpret_cast<double*>(smem);        // [FG][k]
  int* tcnt = reinterpret_cast<int*>(tsum + (size_t)FG * k);  // [k]
  const int g = blockIdx.y;
  const int f0 = FG * g;
  for (int i = threadIdx.x; i < FG * k; i += blockDim.x) tsum[i] = 0.0;
  for (int i = threadIdx.x; i < k; i += blockDim.x) tcnt[i] = 0;
  __syncthreads();
  const int64_t per = ((n + gridDim.x - 1) / gridDim.x + 63) & ~63ll;
  const int64_t i0 = (int64_t)blockIdx.x * per;
  const int64_t i1 = (i0 + per) < n ? (i0 + per) : n;
  const f4* X4 = reinterpret_cast<const f4*>(X);
  constexpr int FQ = FG / 4;
  const int Q = d4_of(d) / 4;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const int l = labels[i];
    f4 v[FQ];
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
      const int qq = f0 / 4 + q;
      v[q] = qq < Q ? X4[(int64_t)qq * n_pad + i] : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int q = 0; q < FQ; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (f0 + 4 * q + c < d) atomicAdd(&tsum[(4 * q + c) * k + l], (double)v[q][c]);
    if (g == 0) atomicAdd(&tcnt[l], 1);
  }
  __syncthreads();
  const int d1 = d + 1;
  for (int i = threadIdx.x; i < FG * k; i += blockDim.x) {
    const int f = f0 + i / k, j = i % k;
    const double s = tsum[i];
    if (f < d && s != 0.0)
      atomicAdd(&out[(size_t)j * d1 + f], (unsigned long long)__double2ll_rn(s * fx));
  }
  if (g == 0)
    for (int j = threadIdx.x; j < k; j += blockDim.x)
      if (tcnt[j]) atomicAdd(&out[(size_t)j * d1 + d], (unsigned long long)(long long)tcnt[j]);
}

__global__ void zero_big_gated(long long* __restrict__ p, int64_t n,
                               const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
}

// DELTA update: the moves {pt, old << 16 | new} of L1's per-wave regions
// (mv1, counts cnt1) and of L2 / L3 (flat mv2, count *cnt2) applied to the
// running (k, d+1) int64 sums: +x into the new cluster, -x out of the old,
// x gathered from the row-major copy.  blockIdx.y = feature group (FG
// features), blockIdx.x = slice of the moves; an LDS table [FG][k] of fp64
// (exact: grid values) per workgroup, then its nonzero cells as exact int64
// fixed point with atomics.  Integer sums: equal to a full recompute.
constexpr int kFixSlices = 32;

template <int FG>
__global__ __launch_bounds__(1024) void fixup_big(const float* __restrict__ XA, int d4, int d,
                                                  int k, const int2* __restrict__ mv1,
                                                  const int32_t* __restrict__ cnt1, int nw1,
                                                  int cap1, const int2* __restrict__ mv2,
                                                  const int32_t* __restrict__ cnt2, double fx,
                                                  unsigned long long* __restrict__ out,
                                                  const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* tsum = reinterpret_cast<double*>(smem);              // [FG][k]
  int* tcnt = reinterpret_cast<int*>(tsum + (size_t)FG * k);   // [k]
  const int g = blockIdx.y, f0 = FG * g;
  const int G = gridDim.x, sl = blockIdx.x;
  for (int i = threadIdx.x; i < FG * k; i += blockDim.x) tsum[i] = 0.0;
  for (int i = threadIdx.x; i < k; i += blockDim.x) tcnt[i] = 0;
  __syncthreads();
  auto apply = [&](const int2* list, int64_t cnt) {
    for (int64_t idx = threadIdx.x; idx < cnt * FG; idx += blockDim.x) {
      const int64_t e = idx / FG;
      const int ff = (int)(idx - e * FG);
      const int f = f0 + ff;
      const int2 m = list[e];
      const int oldl = (int)((unsigned)m.y >> 16), newl = m.y & 0xFFFF;
      if (f < d) {
        const double x = (double)XA[(int64_t)m.x * d4 + f];
        atomicAdd(&tsum[ff * k + newl], x);
        atomicAdd(&tsum[ff * k + oldl], -x);
      }
      if (ff == 0 && g == 0) {
        atomicAdd(&tcnt[newl], 1);
        atomicAdd(&tcnt[oldl], -1);
      }
    }
  };
  for (int r = sl; r < nw1; r += G) apply(mv1 + (size_t)r * cap1, cnt1[r]);
  {
    const int64_t n2 = *cnt2, per = (n2 + G - 1) / G;
    const int64_t e0 = (int64_t)sl * per, e1 = min(n2, e0 + per);
    if (e1 > e0) apply(mv2 + e0, e1 - e0);
  }
  __syncthreads();
  const int d1 = d + 1;
  for (int i = threadIdx.x; i < FG * k; i += blockDim.x) {
    const int f = f0 + i / k, j = i % k;
    const double s = tsum[i];
    if (f < d && s != 0.0)
      atomicAdd(&out[(size_t)j * d1 + f], (unsigned long long)__double2ll_rn(s * fx));
  }
  if (g == 0)
    for (int j = threadIdx.x; j < k; j += blockDim.x)
      if (tcnt[j]) atomicAdd(&out[(size_t)j * d1 + d], (unsigned long long)(long long)tcnt[j]);
}

}  // namespace

// The largest of 16, 8, 4 features whose table [FG][k] of fp64 sums plus the
// [k] counts fits 150 KiB of LDS.
int big_fg(int k) {
  const size_t lim = 150 * 1024;
  if ((size_t)k * (16 * 8 + 4) <= lim) return 16;
  if ((size_t)k * (8 * 8 + 4) <= lim) return 8;
  if ((size_t)k * (4 * 8 + 4) <= lim) return 4;
  return 0;
}

void big_launch_sums(Ctx& c, const BigArgs& a2, unsigned long long* bs) {
  struct Fns {
    void (*update)(const float*, int64_t, int64_t, int, int, const int32_t*, double,
                   unsigned long long*, const long long*);
    void (*fixup)(const float*, int, int, int, const int2*, const int32_t*, int, int, const int2*,
                  const int32_t*, double, unsigned long long*, const long long*);
  };
  // [FG / 8]: FG = 4, 8, 16
  static const Fns fns[3] = {{update_big<4>, fixup_big<4>},
                             {update_big<8>, fixup_big<8>},
                             {update_big<16>, fixup_big<16>}};
  static bool attr = false;
  if (!attr) {
    for (const Fns& f : fns)
      for (const void* fn : {reinterpret_cast<const void*>(f.update),
                             reinterpret_cast<const void*>(f.fixup)})
        HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  const int d = a2.d, k = a2.k, FG = big_fg(k);
  const Fns& f = fns[FG / 8];
  const int ngrp = (d + FG - 1) / FG;
  const size_t ldsu = (size_t)FG * k * 8 + (size_t)k * 4;
  const double fx = std::ldexp(1.0, c.scale_bits);
  if (!a2.delta) {
    hipLaunchKernelGGL(zero_big_gated, dim3(64), dim3(256), 0, c.stream,
                       reinterpret_cast<long long*>(bs), (int64_t)k * (d + 1), a2.gate);
    hipLaunchKernelGGL(f.update, dim3(lloyd_num_cus(c.device), ngrp), dim3(1024), ldsu, c.stream,
                       c.x32.as<float>(), a2.n, a2.n_pad, d, k, a2.labels, fx, bs, a2.gate);
  } else {
    hipLaunchKernelGGL(f.fixup, dim3(kFixSlices, ngrp), dim3(1024), ldsu, c.stream, a2.XA, a2.d4,
                       d, k, a2.mv1, a2.mv1_count, a2.in_regions, a2.in_cap, a2.mv2, a2.mv2_count,
                       fx, bs, a2.gate);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace cdr
