// What bounds place_eval_events (csrc/place_eval.hip): the same
// loop over 124 806 839 synthetic events (files, clients and ops drawn
// uniformly by a hash; 744 000 files, k = 4; 4 and 32 nodes) in three forms:
//   full          as the library's kernel without the per-file table
//   small-gather  the file's 16-byte record read from a 1024-entry table
//                 (16 KiB, cache resident) instead of the 12 MB one
//   no-lds        the record gathered as in full, every LDS add replaced by
//                 one register sum per lane
// Four rounds, the forms alternating; ms from HIP events.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o place_eval_ablate place_eval_ablate.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct alignas(16) Rec { unsigned long long mask; int first; unsigned lc; };

__device__ __host__ inline uint64_t mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

__global__ void gen_events(int32_t* f, int32_t* c, uint8_t* o, int64_t ne, int nf, int nn) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t h = mix(e + 1);
    f[e] = (int)(h % (uint64_t)nf);
    c[e] = (int)((h >> 32) % (uint64_t)nn);
    o[e] = (uint8_t)((h >> 48) % 3);
  }
}
__global__ void gen_recs(Rec* r, int nf, int nn, int k) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const uint64_t h = mix(i + 77);
    unsigned long long m = 0;
    int first = (int)(h % nn);
    m |= 1ull << first;
    m |= 1ull << ((h >> 8) % nn);
    if ((h >> 16) & 1) m |= 1ull << ((h >> 24) % nn);
    Rec x; x.mask = m; x.first = first; x.lc = (unsigned)((h >> 40) % k) | ((unsigned)__popcll(m) << 16);
    r[i] = x;
  }
}

constexpr int U = 8, WAVES = 4, CHUNK = WAVES * 64 * U;

template <int MODE>
__global__ __launch_bounds__(256) void ev(const int32_t* __restrict__ file, const int32_t* __restrict__ client,
                                          const uint8_t* __restrict__ op, const Rec* __restrict__ rec,
                                          int64_t ne, int nf, int nn, int k, unsigned long long* csum,
                                          unsigned long long* nsum) {
  extern __shared__ unsigned long long lds[];
  const int lane = threadIdx.x & 63;
  const int ncw = 6 * k, nnw = 4 * nn;
  unsigned long long* lc = lds;
  unsigned long long* ln = lds + ncw;
  for (int t = threadIdx.x; t < ncw + nnw; t += blockDim.x) lds[t] = 0ull;
  __syncthreads();
  unsigned long long racc = 0;
  const int64_t stride = (int64_t)gridDim.x * CHUNK;
  for (int64_t base = (int64_t)blockIdx.x * CHUNK + (threadIdx.x >> 6) * 64 * U; base < ne; base += stride) {
    int f[U], cl[U], o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e = base + u * 64 + lane;
      const bool ok = e < ne;
      f[u] = ok ? file[e] : -1;
      cl[u] = ok ? client[e] : -1;
      o[u] = ok ? (int)op[e] : 0;
    }
    Rec r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = f[u] >= 0 && f[u] < nf;
      Rec z; z.mask = 0; z.first = -1; z.lc = 0xFFFFu;
      const int idx = MODE == 1 ? (f[u] & 1023) : f[u];
      r[u] = ok ? rec[idx] : z;
      if (!ok) f[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (f[u] < 0) continue;
      const int c = cl[u];
      const bool node = c >= 0 && c < nn;
      const bool in = node && ((r[u].mask >> (c & 63)) & 1ull);
      const bool rd = o[u] == 2, wr = o[u] == 1;
      const unsigned lab = r[u].lc & 0xFFFFu;
      const unsigned copies = r[u].lc >> 16;
      if (MODE == 2) {
        racc += 1 + in + rd + wr * copies + lab + (unsigned)r[u].first + __popcll(r[u].mask);
        continue;
      }
      if (lab < (unsigned)k) {
        unsigned long long* row = lc + 6 * lab;
        atomicAdd(&row[0], 1ull);
        if (in) atomicAdd(&row[1], 1ull);
        if (rd) {
          atomicAdd(&row[2], 1ull);
          if (in) atomicAdd(&row[3], 1ull);
        }
        if (wr) {
          atomicAdd(&row[4], 1ull);
          if (copies) atomicAdd(&row[5], (unsigned long long)copies);
        }
      }
      if (node) {
        atomicAdd(&ln[4 * c], 1ull);
        if (in) atomicAdd(&ln[4 * c + 1], 1ull);
      }
      if (rd) {
        const int srv = in ? c : r[u].first;
        if (srv >= 0) atomicAdd(&ln[4 * srv + 2], 1ull);
      }
      if (wr) {
        unsigned long long m = r[u].mask;
        while (m) {
          const int j = __ffsll((long long)m) - 1;
          m &= m - 1;
          atomicAdd(&ln[4 * j + 3], 1ull);
        }
      }
    }
  }
  __syncthreads();
  if (MODE == 2) { if (racc) atomicAdd(&csum[0], racc); return; }
  for (int t = threadIdx.x; t < ncw; t += blockDim.x) if (lc[t]) atomicAdd(&csum[t], lc[t]);
  for (int t = threadIdx.x; t < nnw; t += blockDim.x) if (ln[t]) atomicAdd(&nsum[t], ln[t]);
}

template <int MODE>
float run(const int32_t* f, const int32_t* c, const uint8_t* o, const Rec* r, int64_t ne, int nf, int nn, int k,
          unsigned long long* sums, int cus) {
  const size_t lds = 8 * (6 * (size_t)k + 4 * (size_t)nn);
  int per_cu = 0;
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ev<MODE>, 256, lds));
  const int grid = (int)std::min<int64_t>((ne + CHUNK - 1) / CHUNK, (int64_t)cus * std::max(per_cu, 1));
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  CK(hipMemset(sums, 0, 8 * (6 * k + 4 * nn)));
  CK(hipEventRecord(a, 0));
  hipLaunchKernelGGL(ev<MODE>, dim3(grid), dim3(256), lds, 0, f, c, o, r, ne, nf, nn, k, sums, sums + 6 * k);
  CK(hipGetLastError());
  CK(hipEventRecord(b, 0));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
  return ms;
}

int main() {
  const int64_t ne = 124806839;
  const int nf = 744000, k = 4;
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  int32_t *f, *c; uint8_t* o; Rec* r; unsigned long long* sums;
  CK(hipMalloc(&f, 4 * ne)); CK(hipMalloc(&c, 4 * ne)); CK(hipMalloc(&o, ne));
  CK(hipMalloc(&r, sizeof(Rec) * nf)); CK(hipMalloc(&sums, 8 * (6 * k + 4 * 64)));
  for (int nn : {4, 32}) {
    hipLaunchKernelGGL(gen_events, dim3(4096), dim3(256), 0, 0, f, c, o, ne, nf, nn);
    hipLaunchKernelGGL(gen_recs, dim3(1024), dim3(256), 0, 0, r, nf, nn, k);
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> h0(6 * k + 4 * nn);
    for (int rep = 0; rep < 4; ++rep) {
      const float m0 = run<0>(f, c, o, r, ne, nf, nn, k, sums, cus);
      CK(hipMemcpy(h0.data(), sums, 8 * h0.size(), hipMemcpyDeviceToHost));
      const float m1 = run<1>(f, c, o, r, ne, nf, nn, k, sums, cus);
      const float m2 = run<2>(f, c, o, r, ne, nf, nn, k, sums, cus);
      printf("nn=%d rep=%d full %.3f  small-gather %.3f  no-lds %.3f ms  events=%llu\n", nn, rep, m0,
             m1, m2, h0[0] + h0[6] + h0[12] + h0[18]);
      fflush(stdout);
    }
  }
  return 0;
}
