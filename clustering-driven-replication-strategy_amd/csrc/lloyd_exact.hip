// lloyd_exact.hip — the exact assignment of every point, the sums and counts
// taken from labels, and the reduction of per-workgroup tables: the kernels
// the Lloyd steps share when no screen decides a shape, each with its host
// enqueue (a kernel is launched from the file that defines it).
#include <cmath>

#include "cdr_internal.h"
#include "exact_math.h"

namespace cdr {

// Sum the per-workgroup tables: block (x, y) covers 64 entries and the y-th
// slice of the workgroups; 4 waves split that slice, combine in LDS and add
// into the (zeroed) output with one integer atomic per entry and slice.
constexpr int kReduceSlices = 16;
__global__ __launch_bounds__(256) void reduce_partials(const long long* __restrict__ part,
                                                       int nwg, int len, int d, int KS,
                                                       unsigned long long* __restrict__ out) {
  __shared__ long long red[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);  // (j, f) of the (k, d+1) output
  const int sub = threadIdx.x >> 6;
  const int per = (nwg + kReduceSlices - 1) / kReduceSlices;
  const int w0 = blockIdx.y * per, w1 = min(nwg, w0 + per);
  const int j = e / (d + 1), f = e % (d + 1);
  const int src = j * KS + (f < d ? f : KS - 1);
  const int slen = (len / (d + 1)) * KS;
  long long s = 0;
  if (e < len)
    for (int w = w0 + sub; w < w1; w += 4) s += part[(size_t)w * slen + src];
  red[sub][threadIdx.x & 63] = s;
  __syncthreads();
  if (sub == 0 && e < len) {
    const long long t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                        red[3][threadIdx.x];
    if (t) atomicAdd(&out[e], (unsigned long long)t);
  }
}

// Exact assignment of every point (F64 mode, or shapes the screen does not
// cover).  T = float (F32X storage) or double (F64 storage).
template <typename T>
__global__ void assign_exact_all(const T* __restrict__ X, int64_t n, int64_t n_pad, int d,
                                 const double* __restrict__ C, int k,
                                 int32_t* __restrict__ labels) {
  for (int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pt < n;
       pt += (int64_t)gridDim.x * blockDim.x) {
    auto xv = [&](int f) { return (double)X[xidx(X, f, pt, n_pad)]; };
    labels[pt] = exact_argmin(xv, C, k, d);
  }
}

// The same with the point's d <= 16 features loaded into registers once
// (assign_exact_all re-reads them from memory for every centroid) and the
// NumPy-order distance unrolled for that d; the centroid values are uniform
// (scalar) loads.
template <typename T, int D>
__global__ __launch_bounds__(256) void assign_exact_d(const T* __restrict__ X, int64_t n,
                                                      int64_t n_pad,
                                                      const double* __restrict__ C, int k,
                                                      int32_t* __restrict__ labels) {
  for (int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pt < n;
       pt += (int64_t)gridDim.x * blockDim.x) {
    double xr[D];
#pragma unroll
    for (int f = 0; f < D; ++f) xr[f] = (double)X[xidx(X, f, pt, n_pad)];
    labels[pt] = exact_argmin([&](int f) { return xr[f]; }, C, k, D);
  }
}

template <typename T>
static void launch_assign_exact(Ctx& c, const T* X, int k) {
  typedef void (*Fn)(const T*, int64_t, int64_t, const double*, int, int32_t*);
#define CDR_AE(D_) assign_exact_d<T, D_>
  static const Fn fns[17] = {nullptr,     CDR_AE(1),  CDR_AE(2),  CDR_AE(3),  CDR_AE(4),
                             CDR_AE(5),   CDR_AE(6),  CDR_AE(7),  CDR_AE(8),  CDR_AE(9),
                             CDR_AE(10),  CDR_AE(11), CDR_AE(12), CDR_AE(13), CDR_AE(14),
                             CDR_AE(15),  CDR_AE(16)};
#undef CDR_AE
  const int d = c.d;
  const double* C = c.cent64.as<double>();
  int32_t* labels = c.labels.as<int32_t>();
  const dim3 grid(std::max(
      1, (int)std::min<int64_t>(ceil_div(c.n, 256), (int64_t)lloyd_num_cus(c.device) * 8)));
  if (d >= 1 && d <= 16)
    hipLaunchKernelGGL(fns[d], grid, dim3(256), 0, c.stream, X, c.n, c.n_pad, C, k, labels);
  else
    hipLaunchKernelGGL(assign_exact_all<T>, grid, dim3(256), 0, c.stream, X, c.n, c.n_pad, d, C, k,
                       labels);
  HIP_CHECK(hipGetLastError());
}

void enqueue_assign_exact(Ctx& c, int k) {
  if (c.mode == CDR_MODE_F32X) launch_assign_exact(c, c.x32.as<float>(), k);
  else launch_assign_exact(c, c.x64.as<double>(), k);
}

// Fixed-point sums from labels (F32X shapes without the screen): LDS table per
// workgroup, plain stores of the table, reduce_partials afterwards.
__global__ __launch_bounds__(256) void update_from_labels_f32x(
    const float* __restrict__ X, int64_t n, int64_t n_pad, int d, int k,
    const int32_t* __restrict__ labels, float fx, unsigned long long* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* tbl = reinterpret_cast<unsigned long long*>(smem);
  const int kd1 = d + 1;
  for (int i = threadIdx.x; i < k * kd1; i += blockDim.x) tbl[i] = 0ull;
  __syncthreads();
  for (int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pt < n;
       pt += (int64_t)gridDim.x * blockDim.x) {
    const int j = labels[pt];
    unsigned long long* row = tbl + (size_t)j * kd1;
    for (int f = 0; f < d; ++f)
      atomicAdd(&row[f], (unsigned long long)(long long)(int)(X[xidx(X, f, pt, n_pad)] * fx));
    atomicAdd(&row[d], 1ull);
  }
  __syncthreads();
  unsigned long long* dst = partials + (size_t)blockIdx.x * k * kd1;
  for (int i = threadIdx.x; i < k * kd1; i += blockDim.x) dst[i] = tbl[i];
}

// Cluster sizes of the labels: one LDS histogram per wave (k <= kCountLds),
// added into the global counts once per (workgroup, cluster).  (One global
// atomic per point serialised on the k addresses: 28 ms at 10M points, k = 16.)
constexpr int kCountLds = 4096;
__global__ __launch_bounds__(256) void count_labels(const int32_t* __restrict__ labels, int64_t n,
                                                    int k, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned hist[];  // [4 waves][k] when k <= kCountLds
  const bool lds = k <= kCountLds;
  if (lds) {
    for (int i = threadIdx.x; i < 4 * k; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
  }
  unsigned* wh = hist + (threadIdx.x >> 6) * k;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int l = labels[i];
    if (lds) atomicAdd(&wh[l], 1u);
    else atomicAdd(&counts[l], 1ull);
  }
  if (!lds) return;
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const unsigned long long v = (unsigned long long)hist[j] + hist[k + j] + hist[2 * k + j] +
                                 hist[3 * k + j];
    if (v) atomicAdd(&counts[j], v);
  }
}

void enqueue_reduce_partials(Ctx& c, int nwg, int len, int KS, long long* dout) {
  hipLaunchKernelGGL(reduce_partials, dim3((len + 63) / 64, kReduceSlices), dim3(256), 0,
                     c.stream, c.partials.as<long long>(), nwg, len, c.d, KS,
                     reinterpret_cast<unsigned long long*>(dout));
  HIP_CHECK(hipGetLastError());
}

void enqueue_update_from_labels(Ctx& c, int k, long long* dout) {
  const int d = c.d, len = k * (d + 1);
  // the update table of large k without screen_big (pre_ok false) takes more
  // than the default 64 KiB of dynamic LDS; a workgroup can have 160 KiB.
  // (The flag is per process and the attribute may be per device: DESIGN.md §9.000000.)
  static bool uattr = false;
  if (!uattr) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&update_from_labels_f32x),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    uattr = true;
  }
  const int cus = lloyd_num_cus(c.device);
  int nwg = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(c.n, 256), cus * 2));
  c.partials.ensure(sizeof(long long) * (size_t)nwg * len);
  hipLaunchKernelGGL(update_from_labels_f32x, dim3(nwg), dim3(256), (size_t)len * 8, c.stream,
                     c.x32.as<float>(), c.n, c.n_pad, d, k, c.labels.as<int32_t>(),
                     (float)std::ldexp(1.0, c.scale_bits), c.partials.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  enqueue_reduce_partials(c, nwg, len, d + 1, dout);
}

void enqueue_count_labels(Ctx& c, int k, long long* d_counts) {
  const int cus = lloyd_num_cus(c.device);
  HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(long long) * k, c.stream));
  hipLaunchKernelGGL(count_labels, dim3(std::max(1, (int)std::min<int64_t>(ceil_div(c.n, 256), cus * 2))),
                     dim3(256), k <= kCountLds ? sizeof(unsigned) * 4 * k : 0, c.stream,
                     c.labels.as<int32_t>(), c.n, k, reinterpret_cast<unsigned long long*>(d_counts));
  HIP_CHECK(hipGetLastError());
}

}  // namespace cdr
