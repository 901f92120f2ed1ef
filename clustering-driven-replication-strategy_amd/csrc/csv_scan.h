// csv_scan.h — the fixed-order sums and scans of the text writers (csvout.hip,
// plan.hip): pairs of int64 (output bytes, deferred rows) over the 256 threads
// of a workgroup, and the one-workgroup scan over the workgroups' sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cdr {

namespace {

// Sum of (a, b) over the workgroup's 256 threads, in a fixed tree order.
__device__ inline void block_sum2(long long& a, long long& b, long long* sh) {
  const int t = threadIdx.x;
  sh[t] = a;
  sh[256 + t] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      sh[t] += sh[t + o];
      sh[256 + t] += sh[256 + t + o];
    }
    __syncthreads();
  }
  a = sh[0];
  b = sh[256];
  __syncthreads();
}

// Exclusive scan of (a, b) over the workgroup's 256 threads (Hillis-Steele).
__device__ inline void block_exscan2(long long& a, long long& b, long long* sh) {
  const int t = threadIdx.x;
  long long ia = a, ib = b;
  for (int o = 1; o < 256; o <<= 1) {
    sh[t] = ia;
    sh[256 + t] = ib;
    __syncthreads();
    if (t >= o) {
      ia += sh[t - o];
      ib += sh[256 + t - o];
    }
    __syncthreads();
  }
  a = ia - a;
  b = ib - b;
}

// One workgroup: part[2 g], part[2 g + 1] become the exclusive prefix sums over
// the workgroups g; total[0], total[1] the sums.
__global__ __launch_bounds__(256) void csv_scan_top(long long* __restrict__ part, int64_t n_parts,
                                                    long long* __restrict__ total) {
  __shared__ long long sh[512];
  const int t = threadIdx.x;
  const int64_t per = (n_parts + 255) / 256;
  const int64_t g0 = t * per < n_parts ? t * per : n_parts;
  const int64_t g1 = g0 + per < n_parts ? g0 + per : n_parts;
  long long a = 0, b = 0;
  for (int64_t g = g0; g < g1; ++g) {
    a += part[2 * g];
    b += part[2 * g + 1];
  }
  long long ta = a, tb = b;
  block_exscan2(a, b, sh);
  if (t == 255) {
    total[0] = a + ta;
    total[1] = b + tb;
  }
  for (int64_t g = g0; g < g1; ++g) {
    const long long va = part[2 * g], vb = part[2 * g + 1];
    part[2 * g] = a;
    part[2 * g + 1] = b;
    a += va;
    b += vb;
  }
}

}  // namespace

}  // namespace cdr
