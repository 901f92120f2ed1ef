// medians.hip — per-cluster per-feature medians (reference src/scoring.py:40-55).
//
// np.median(list) of m values: the elements of sorted rank (m-1)/2 and m/2
// (0-based), then np.mean of those one or two values, i.e. ((0.0 + a) + b) / 2
// (or (0.0 + a) / 1): the sum starts from +0.0, so median([-0.0]) is +0.0.
// Empty -> NaN; any NaN -> NaN (numpy _median_nancheck).
//
// Selection is an MSB radix select over order-preserving unsigned keys, one
// workgroup per segment: each pass histograms (in LDS) the 8-bit digit of the
// elements that still match the prefix found so far, for both target ranks.
// 64-bit keys (fp64 values) take 8 passes, 32-bit keys (F32X points) take 4.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cdr_internal.h"

namespace cdr {

__device__ __forceinline__ unsigned long long okey64(double v) {
  const unsigned long long b = __double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_okey64(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double(b);
}
__device__ __forceinline__ unsigned okey32(float v) {
  const unsigned b = __float_as_uint(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_okey32(unsigned k) {
  const unsigned b = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
  return __uint_as_float(b);
}

template <typename V>
struct KeyOf;
template <>
struct KeyOf<double> {
  typedef unsigned long long K;
  static constexpr int BITS = 64;
  __device__ static K key(double v) { return okey64(v); }
  __device__ static double val(K k) { return from_okey64(k); }
  __device__ static bool isnan_(double v) { return isnan(v); }
};
template <>
struct KeyOf<float> {
  typedef unsigned K;
  static constexpr int BITS = 32;
  __device__ static K key(float v) { return okey32(v); }
  __device__ static double val(K k) { return (double)from_okey32(k); }
  __device__ static bool isnan_(float v) { return isnan(v); }
};

// Segment s = vals[off[s] .. off[s+1]) (element stride 1).  out[s] = median.
template <typename V>
__global__ __launch_bounds__(256) void seg_median_kernel(const V* __restrict__ vals,
                                                         const int64_t* __restrict__ off,
                                                         int64_t nseg, double* __restrict__ out) {
  typedef typename KeyOf<V>::K K;
  __shared__ unsigned hist[2][256];
  __shared__ K sprefix[2];
  __shared__ long long srank[2];
  __shared__ int snan;
  for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
    const int64_t lo = off[s], hi = off[s + 1];
    const int64_t m = hi - lo;
    if (m <= 0) {
      if (threadIdx.x == 0) out[s] = NAN;
      continue;
    }
    if (threadIdx.x == 0) snan = 0;
    __syncthreads();
    int anynan = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) anynan |= KeyOf<V>::isnan_(vals[i]);
    if (anynan) atomicOr(&snan, 1);
    __syncthreads();
    if (snan) {
      if (threadIdx.x == 0) out[s] = NAN;
      __syncthreads();
      continue;
    }
    if (threadIdx.x == 0) {
      sprefix[0] = 0;
      sprefix[1] = 0;
      srank[0] = (m - 1) / 2;
      srank[1] = m / 2;
    }
    __syncthreads();
    K mask = 0;
    for (int shift = KeyOf<V>::BITS - 8; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0;
      __syncthreads();
      const K p0 = sprefix[0], p1 = sprefix[1];
      const bool two = p0 != p1;
      for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const K key = KeyOf<V>::key(vals[i]);
        const unsigned dig = (unsigned)((key >> shift) & 0xFF);
        if ((key & mask) == p0) atomicAdd(&hist[0][dig], 1u);
        if (two && (key & mask) == p1) atomicAdd(&hist[1][dig], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 2) {
        const int w = threadIdx.x;
        const int hsel = (w == 1 && !two) ? 0 : w;
        long long r = srank[w];
        unsigned dsel = 255;
        for (unsigned dgt = 0; dgt < 256; ++dgt) {
          const long long c = hist[hsel][dgt];
          if (r < c) {
            dsel = dgt;
            break;
          }
          r -= c;
        }
        srank[w] = r;
        sprefix[w] = (w == 0 ? p0 : p1) | ((K)dsel << shift);
      }
      mask |= ((K)0xFF << shift);
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double a = KeyOf<V>::val(sprefix[0]);
      if (m & 1) {
        out[s] = (0.0 + a) / 1.0;
      } else {
        const double b = KeyOf<V>::val(sprefix[1]);
        out[s] = ((0.0 + a) + b) / 2.0;
      }
    }
    __syncthreads();
  }
}

// ---- medians of the resident points grouped by label (main.py:96-107) ----
// The rows of each cluster are gathered once into a point-major copy (a
// two-pass counting sort: per-block LDS label counts, a column scan for the
// block offsets, a scatter with LDS ranks: no global cursor atomics), then
// every (cluster, feature) pair is selected by an MSB radix select over
// order-preserving keys, 8 bits per pass, for both middle ranks at once: one
// workgroup per cluster and 64-feature chunk histograms its rows in LDS
// ([64][2][256] counters), the histograms go to global memory (where a
// sharded run all-reduces them), and one thread per pair
// picks the next digit of each rank.  Ranks are of the global cluster sizes.
constexpr int kMgBlock = 4096;   // points per counting-sort block
constexpr int kMgRange = 64;     // blocks per column-scan range
constexpr int kMgMaxK = 8192;
constexpr int kMgFeat = 64;      // features per histogram workgroup

__global__ __launch_bounds__(256) void mg_count(const int32_t* __restrict__ labels, int64_t n,
                                                int k, unsigned* __restrict__ cnt) {
  extern __shared__ unsigned hc[];
  for (int j = threadIdx.x; j < k; j += 256) hc[j] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kMgBlock;
  for (int i = threadIdx.x; i < kMgBlock; i += 256)
    if (i0 + i < n) atomicAdd(&hc[labels[i0 + i]], 1u);
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += 256) cnt[(int64_t)blockIdx.x * k + j] = hc[j];
}

// column scan of cnt [nblk][k]: a) range sums, b) range bases + label totals
// and bases (one workgroup), c) absolute block offsets in place
__global__ __launch_bounds__(256) void mg_scan_a(const unsigned* __restrict__ cnt, int64_t nblk,
                                                 int k, unsigned long long* __restrict__ rsum) {
  const int64_t r0 = (int64_t)blockIdx.x * kMgRange;
  for (int j = threadIdx.x; j < k; j += 256) {
    unsigned long long s = 0;
    for (int r = 0; r < kMgRange && r0 + r < nblk; ++r) s += cnt[(r0 + r) * k + j];
    rsum[(int64_t)blockIdx.x * k + j] = s;
  }
}

__global__ __launch_bounds__(1024) void mg_scan_b(unsigned long long* __restrict__ rsum,
                                                  int64_t nr, int k,
                                                  long long* __restrict__ base,
                                                  long long* __restrict__ total) {
  __shared__ long long wsum[16];
  __shared__ long long carry;
  for (int j = threadIdx.x; j < k; j += 1024) {
    unsigned long long run = 0;
    for (int64_t r = 0; r < nr; ++r) {
      const unsigned long long v = rsum[r * k + j];
      rsum[r * k + j] = run;
      run += v;
    }
    total[j] = (long long)run;
  }
  __syncthreads();
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int j0 = 0; j0 < k; j0 += 1024) {
    const int j = j0 + threadIdx.x;
    const long long v = j < k ? total[j] : 0;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long long pre = carry;
    for (int q = 0; q < w; ++q) pre += wsum[q];
    if (j < k) base[j] = pre + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = pre + inc;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mg_scan_c(unsigned* __restrict__ cnt, int64_t nblk, int k,
                                                 const unsigned long long* __restrict__ rbase,
                                                 const long long* __restrict__ base) {
  const int64_t r0 = (int64_t)blockIdx.x * kMgRange;
  for (int j = threadIdx.x; j < k; j += 256) {
    unsigned long long run = (unsigned long long)base[j] + rbase[(int64_t)blockIdx.x * k + j];
    for (int r = 0; r < kMgRange && r0 + r < nblk; ++r) {
      const unsigned v = cnt[(r0 + r) * k + j];
      cnt[(r0 + r) * k + j] = (unsigned)run;
      run += v;
    }
  }
}

// Ranks first (one thread per point, LDS cursors), then the rows copied with
// the lanes of a wave over (point, feature): each point's row is written as
// one contiguous run.
template <typename V>
__global__ __launch_bounds__(256) void mg_scatter(const V* __restrict__ X, int64_t n,
                                                  int64_t n_pad, int d,
                                                  const int32_t* __restrict__ labels, int k,
                                                  const unsigned* __restrict__ off,
                                                  V* __restrict__ rows) {
  extern __shared__ unsigned cur[];
  __shared__ unsigned pos[kMgBlock];
  for (int j = threadIdx.x; j < k; j += 256) cur[j] = off[(int64_t)blockIdx.x * k + j];
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kMgBlock;
  const int np = (int)min((int64_t)kMgBlock, n - i0);
  for (int i = threadIdx.x; i < np; i += 256) pos[i] = atomicAdd(&cur[labels[i0 + i]], 1u);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int D2 = 1;
  while (D2 < d && D2 < 64) D2 <<= 1;
  const int rpw = 64 / D2;                    // points per wave step
  const int sub = lane / D2, fl = lane % D2;
  for (int p0 = w * rpw; p0 < np; p0 += 4 * rpw) {
    const int pi = p0 + sub;
    if (pi >= np) continue;
    V* dst = rows + (int64_t)pos[pi] * d;
    for (int f = fl; f < d; f += D2) dst[f] = X[xidx(X, f, i0 + pi, n_pad)];
  }
}

// Pass p (digit shift sh) for cluster j = blockIdx.x, features [f0, f0 + 64):
// counts of the digit among the rows whose key matches each rank's prefix.
// Both ranks share one histogram while their prefixes are equal (flag in
// two[]), as the selection step reads it.
template <typename V>
__global__ __launch_bounds__(1024) void mg_hist(const V* __restrict__ rows, int d, int k,
                                                const long long* __restrict__ base,
                                                const long long* __restrict__ cnt_local,
                                                const unsigned long long* __restrict__ pref,
                                                int sh, unsigned* __restrict__ H) {
  typedef typename KeyOf<V>::K K;
  // counters of feature f, rank t, digit g at f * kMgHs + t * 257 + g: the
  // odd strides put the lanes of a wave (different features, often the same
  // digit) in different banks
  constexpr int kMgHs = 515;
  constexpr int kU = 8;  // rows in flight per lane
  __shared__ unsigned h[kMgFeat * kMgHs];
  __shared__ K sp[kMgFeat][2];
  const int j = blockIdx.x;
  const int f0 = blockIdx.y * kMgFeat;
  const int nfc = min(kMgFeat, d - f0);
  for (int i = threadIdx.x; i < kMgFeat * kMgHs; i += 1024) h[i] = 0;
  for (int i = threadIdx.x; i < 2 * nfc; i += 1024)
    sp[i >> 1][i & 1] = (K)pref[((int64_t)j * d + f0) * 2 + i];
  __syncthreads();
  const K mask = sh + 8 >= KeyOf<V>::BITS ? (K)0 : (K)(~(K)0 << (sh + 8));
  const int64_t lo = base[j], m = cnt_local[j];
  // lanes over (row, feature): a wave reads whole rows (contiguous) and, for
  // d >= 64, its lanes count different features (no counter shared in a
  // wave); kU rows per lane are loaded before any is counted
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int D2 = 1;
  while (D2 < nfc) D2 <<= 1;
  const int rpw = 64 / D2;
  const int sub = lane / D2, f = lane % D2;
  if (f < nfc) {
    const K p0 = sp[f][0], p1 = sp[f][1];
    const bool two = p1 != p0;
    const int64_t step = (int64_t)16 * rpw;  // 16 waves
    for (int64_t r0 = (int64_t)w * rpw + sub; r0 < m; r0 += kU * step) {
      V v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t r = r0 + u * step;
        v[u] = r < m ? rows[(lo + r) * d + f0 + f] : (V)0;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (r0 + u * step >= m) break;
        const K key = KeyOf<V>::key(v[u]);
        const unsigned dig = (unsigned)((key >> sh) & 0xFF);
        if ((key & mask) == p0) atomicAdd(&h[f * kMgHs + dig], 1u);
        if (two && (key & mask) == p1) atomicAdd(&h[f * kMgHs + 257 + dig], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nfc * 512; i += 1024) {
    const int ff = i >> 9, t = (i >> 8) & 1, g = i & 255;
    H[((int64_t)j * d + f0) * 512 + i] = h[ff * kMgHs + t * 257 + g];
  }
}

// One thread per (cluster, feature): the next digit of both ranks.
template <typename V>
__global__ void mg_select(const unsigned* __restrict__ H, int d, int k,
                          const long long* __restrict__ cnt_global, int sh,
                          unsigned long long* __restrict__ pref, long long* __restrict__ rank) {
  typedef typename KeyOf<V>::K K;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * d) return;
  if (cnt_global[t / d] <= 0) return;
  const K p0 = (K)pref[2 * t], p1 = (K)pref[2 * t + 1];
  const bool two = p0 != p1;
  for (int w = 0; w < 2; ++w) {
    const unsigned* hist = H + (int64_t)t * 512 + ((w == 1 && two) ? 256 : 0);
    long long r = rank[2 * t + w];
    unsigned dsel = 255;
    for (unsigned g = 0; g < 256; ++g) {
      const long long c = hist[g];
      if (r < c) {
        dsel = g;
        break;
      }
      r -= c;
    }
    rank[2 * t + w] = r;
    pref[2 * t + w] = (unsigned long long)((w == 0 ? p0 : p1) | ((K)dsel << sh));
  }
}

template <typename V>
__global__ void mg_finish(const long long* __restrict__ cnt_global, int d, int k,
                          const unsigned long long* __restrict__ pref, double* __restrict__ out) {
  typedef typename KeyOf<V>::K K;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * d) return;
  const long long m = cnt_global[t / d];
  if (m <= 0) {
    out[t] = NAN;
    return;
  }
  const double a = KeyOf<V>::val((K)pref[2 * t]);
  if (m & 1) {
    out[t] = (0.0 + a) / 1.0;
  } else {
    const double b = KeyOf<V>::val((K)pref[2 * t + 1]);
    out[t] = ((0.0 + a) + b) / 2.0;
  }
}

__global__ void mg_begin(const long long* __restrict__ cnt_global, int d, int k,
                         unsigned long long* __restrict__ pref, long long* __restrict__ rank) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * d) return;
  const long long m = cnt_global[t / d];
  pref[2 * t] = 0;
  pref[2 * t + 1] = 0;
  rank[2 * t] = m > 0 ? (m - 1) / 2 : 0;
  rank[2 * t + 1] = m > 0 ? m / 2 : 0;
}

static int grid_cap(int64_t work, int threads, int cap) {
  int64_t g = (work + threads - 1) / threads;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

void medians_segmented(Ctx& c, const double* values, const int64_t* offsets, int64_t nseg,
                       double* out) {
  if (nseg < 0) CDR_FAIL(CDR_ERR_ARG, "n_segments < 0");
  if (nseg == 0) return;
  const int64_t total = offsets[nseg] - offsets[0];
  if (total < 0) CDR_FAIL(CDR_ERR_ARG, "offsets must be non-decreasing");
  for (int64_t s = 0; s < nseg; ++s)
    if (offsets[s + 1] < offsets[s]) CDR_FAIL(CDR_ERR_ARG, "offsets must be non-decreasing");
  c.med_k = 0;  // the grouped rows of cdr_medians_group live in these buffers
  c.med_vals.ensure(sizeof(double) * (total > 0 ? total : 1));
  c.med_off.ensure(sizeof(int64_t) * (nseg + 1));
  c.med_out.ensure(sizeof(double) * nseg);
  std::vector<int64_t> off0(nseg + 1);
  for (int64_t s = 0; s <= nseg; ++s) off0[s] = offsets[s] - offsets[0];
  if (total > 0)
    HIP_CHECK(hipMemcpyAsync(c.med_vals.p, values + offsets[0], sizeof(double) * total,
                             hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemcpyAsync(c.med_off.p, off0.data(), sizeof(int64_t) * (nseg + 1),
                           hipMemcpyHostToDevice, c.stream));
  hipLaunchKernelGGL(seg_median_kernel<double>, dim3(grid_cap(nseg, 1, 65536)), dim3(256), 0,
                     c.stream, c.med_vals.as<double>(), c.med_off.as<int64_t>(), nseg,
                     c.med_out.as<double>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, c.med_out.p, sizeof(double) * nseg, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

// ---- host side of the label medians (single shard or one rank of several) --
static int mg_passes(const Ctx& c) { return c.mode == CDR_MODE_F32X ? 4 : 8; }

// The grouped state (med_k, med_vals, med_off, and med_out once begun) is
// valid only for the points, labels and buffers it was built from; whoever
// changes one of them clears med_k.
static void mg_need_group(const Ctx& c, bool begun) {
  if (c.med_k <= 0)
    CDR_FAIL(CDR_ERR_STATE,
             "medians: no grouped rows of the current points and labels: call "
             "cdr_medians_group first");
  if (begun && !c.med_begun)
    CDR_FAIL(CDR_ERR_STATE, "medians: call cdr_medians_begin after cdr_medians_group");
}

void medians_group(Ctx& c, int32_t k, int64_t* counts) {
  if (!c.have_labels) CDR_FAIL(CDR_ERR_STATE, "no Lloyd labels: run cdr_lloyd_step first");
  if (k < 1 || k < c.last_k) CDR_FAIL(CDR_ERR_ARG, "k smaller than the labels' k");
  if (k > kMgMaxK) CDR_FAIL(CDR_ERR_UNSUPPORTED, "medians: k > 8192");
  c.med_k = 0;
  c.med_begun = false;
  const int d = c.d;
  const int64_t n = c.n;
  if (n >= (1ll << 32)) CDR_FAIL(CDR_ERR_UNSUPPORTED, "medians: 2^32 points or more per shard");
  const bool f32 = c.mode == CDR_MODE_F32X;
  const size_t vsz = f32 ? 4 : 8;
  const int64_t nblk = std::max<int64_t>(1, ceil_div(n, kMgBlock));
  const int64_t nr = ceil_div(nblk, kMgRange);
  c.med_tmp.ensure(sizeof(unsigned) * (size_t)nblk * k);
  c.med_tmp2.ensure(sizeof(unsigned long long) * (size_t)nr * k);
  c.med_off.ensure(sizeof(long long) * 2 * (size_t)k);
  unsigned* cnt = c.med_tmp.as<unsigned>();
  long long* base = c.med_off.as<long long>();
  long long* total = base + k;
  const size_t lds = sizeof(unsigned) * k;
  hipLaunchKernelGGL(mg_count, dim3(nblk), dim3(256), lds, c.stream, c.labels.as<int32_t>(), n,
                     k, cnt);
  hipLaunchKernelGGL(mg_scan_a, dim3(nr), dim3(256), 0, c.stream, cnt, nblk, k,
                     c.med_tmp2.as<unsigned long long>());
  hipLaunchKernelGGL(mg_scan_b, dim3(1), dim3(1024), 0, c.stream,
                     c.med_tmp2.as<unsigned long long>(), nr, k, base, total);
  hipLaunchKernelGGL(mg_scan_c, dim3(nr), dim3(256), 0, c.stream, cnt, nblk, k,
                     c.med_tmp2.as<unsigned long long>(), base);
  HIP_CHECK(hipGetLastError());
  c.med_vals.ensure(vsz * (size_t)d * (n > 0 ? n : 1));
  if (n > 0) {
    if (f32)
      hipLaunchKernelGGL(mg_scatter<float>, dim3(nblk), dim3(256), lds, c.stream,
                         c.x32.as<float>(), n, c.n_pad, d, c.labels.as<int32_t>(), k, cnt,
                         c.med_vals.as<float>());
    else
      hipLaunchKernelGGL(mg_scatter<double>, dim3(nblk), dim3(256), lds, c.stream,
                         c.x64.as<double>(), n, c.n_pad, d, c.labels.as<int32_t>(), k, cnt,
                         c.med_vals.as<double>());
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipMemcpyAsync(counts, total, sizeof(long long) * k, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.med_k = k;
}

int medians_begin(Ctx& c, const int64_t* global_counts) {
  mg_need_group(c, false);
  const int k = c.med_k, d = c.d;
  for (int j = 0; j < k; ++j)
    if (global_counts[j] >= (1ll << 32))
      CDR_FAIL(CDR_ERR_UNSUPPORTED, "medians: a cluster of 2^32 points or more");
  const size_t kd = (size_t)k * d;
  c.med_out.ensure(sizeof(long long) * k + sizeof(unsigned long long) * 2 * kd +
                   sizeof(long long) * 2 * kd + sizeof(double) * kd);
  long long* gcnt = c.med_out.as<long long>();
  unsigned long long* pref = reinterpret_cast<unsigned long long*>(gcnt + k);
  long long* rank = reinterpret_cast<long long*>(pref + 2 * kd);
  HIP_CHECK(hipMemcpyAsync(gcnt, global_counts, sizeof(long long) * k, hipMemcpyHostToDevice,
                           c.stream));
  hipLaunchKernelGGL(mg_begin, dim3(ceil_div((int64_t)kd, 256)), dim3(256), 0, c.stream, gcnt, d,
                     k, pref, rank);
  HIP_CHECK(hipGetLastError());
  c.med_hist.ensure(sizeof(unsigned) * 512 * kd);
  c.med_begun = true;
  return mg_passes(c);
}

// hist: where the pass's histograms go ([k][d][2][256] u32; host or device
// memory; nullptr = leave them in the context for the select step)
void medians_pass_hist(Ctx& c, int pass, void* hist) {
  mg_need_group(c, true);
  const int k = c.med_k, d = c.d, P = mg_passes(c);
  if (pass < 0 || pass >= P) CDR_FAIL(CDR_ERR_ARG, "medians: pass out of range");
  const size_t kd = (size_t)k * d;
  long long* gcnt = c.med_out.as<long long>();
  unsigned long long* pref = reinterpret_cast<unsigned long long*>(gcnt + k);
  const int sh = (P - 1 - pass) * 8;
  const long long* base = c.med_off.as<long long>();
  const long long* total = base + k;
  dim3 grid(k, (unsigned)ceil_div(d, kMgFeat));
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(mg_hist<float>, grid, dim3(1024), 0, c.stream, c.med_vals.as<float>(), d, k,
                       base, total, pref, sh, c.med_hist.as<unsigned>());
  else
    hipLaunchKernelGGL(mg_hist<double>, grid, dim3(1024), 0, c.stream, c.med_vals.as<double>(), d,
                       k, base, total, pref, sh, c.med_hist.as<unsigned>());
  HIP_CHECK(hipGetLastError());
  if (hist) {
    HIP_CHECK(hipMemcpyAsync(hist, c.med_hist.p, sizeof(unsigned) * 512 * kd, hipMemcpyDefault,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }
}

void medians_pass_select(Ctx& c, int pass, const void* hist) {
  mg_need_group(c, true);
  const int k = c.med_k, d = c.d, P = mg_passes(c);
  if (pass < 0 || pass >= P) CDR_FAIL(CDR_ERR_ARG, "medians: pass out of range");
  const size_t kd = (size_t)k * d;
  long long* gcnt = c.med_out.as<long long>();
  unsigned long long* pref = reinterpret_cast<unsigned long long*>(gcnt + k);
  long long* rank = reinterpret_cast<long long*>(pref + 2 * kd);
  if (hist)
    HIP_CHECK(hipMemcpyAsync(c.med_hist.p, hist, sizeof(unsigned) * 512 * kd, hipMemcpyDefault,
                             c.stream));
  const int sh = (P - 1 - pass) * 8;
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(mg_select<float>, dim3(ceil_div((int64_t)kd, 256)), dim3(256), 0, c.stream,
                       c.med_hist.as<unsigned>(), d, k, gcnt, sh, pref, rank);
  else
    hipLaunchKernelGGL(mg_select<double>, dim3(ceil_div((int64_t)kd, 256)), dim3(256), 0,
                       c.stream, c.med_hist.as<unsigned>(), d, k, gcnt, sh, pref, rank);
  HIP_CHECK(hipGetLastError());
}

void medians_finish(Ctx& c, double* out) {
  mg_need_group(c, true);
  const int k = c.med_k, d = c.d;
  const size_t kd = (size_t)k * d;
  long long* gcnt = c.med_out.as<long long>();
  unsigned long long* pref = reinterpret_cast<unsigned long long*>(gcnt + k);
  double* res = reinterpret_cast<double*>(reinterpret_cast<long long*>(pref + 2 * kd) + 2 * kd);
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(mg_finish<float>, dim3(ceil_div((int64_t)kd, 256)), dim3(256), 0, c.stream,
                       gcnt, d, k, pref, res);
  else
    hipLaunchKernelGGL(mg_finish<double>, dim3(ceil_div((int64_t)kd, 256)), dim3(256), 0,
                       c.stream, gcnt, d, k, pref, res);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, res, sizeof(double) * kd, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

void medians_by_label(Ctx& c, int32_t k, double* out) {
  std::vector<int64_t> counts(k);
  medians_group(c, k, counts.data());
  const int P = medians_begin(c, counts.data());
  for (int p = 0; p < P; ++p) {
    medians_pass_hist(c, p, nullptr);
    medians_pass_select(c, p, nullptr);
  }
  medians_finish(c, out);
}

// ---- medians of all resident points (main.py:31-38: global_medians) --------
// The same radix select as the label medians with one "cluster" that holds
// every row, so nothing is grouped or copied: each pass streams the resident
// layout itself (x32 quad SoA, x64 planar) on a full grid and counts, per
// feature, the digit of the values that still match each rank's prefix.  The
// counters of a workgroup live in LDS ([kGmFeat][2][256] u32, 32 KiB: up to
// five workgroups per CU); the non-zero ones are added to the global
// [d][2][256] table with integer atomics at the end, so the result does not
// depend on the order.  mg_begin / mg_select / mg_finish run with k = 1 and
// the global row count.
//
// A wave's lanes always count the same feature, so its 64 LDS adds differ in
// the digit alone, and in the first passes (and in every pass of a constant
// column) nearly all of them name one counter: 64 adds on one address
// serialise.  gm_add therefore peels digit groups off the wave: the first
// active lane's digit is broadcast, a ballot counts the active lanes that
// share it, and that lane adds the count once.  It goes on while the groups
// are large (>= kGmPeel lanes) and leaves the rest to per-lane adds: one
// round and one add per value on a constant column; on random digits one
// round per batch of loads (the probe below), then per-lane adds, few of
// which share a counter.
constexpr int kGmFeat = 16;    // features per histogram workgroup (4 quads)
constexpr int kGmThreads = 256;
constexpr int kGmU = 8;        // 16-byte loads in flight per lane
constexpr int kGmRows = 512;   // rows per wave turn: 64 kGmU (x32), 128 (kGmU / 2) (x64)
constexpr int kGmPeel = 8;     // smallest digit group worth another peel round
constexpr int kGmWgPerCu = 4;

// hot (wave-uniform, one per feature and rank in the caller): the last probe
// found a large group.  A probe value (the first of each batch of loads)
// always peels; the others only while hot, so random digits pay one peel
// round per batch and not per value.
__device__ __forceinline__ void gm_add(unsigned* __restrict__ hb, unsigned dg, bool act,
                                       int lane, bool probe, bool& hot) {
  unsigned long long rem = __ballot(act);
  if (probe || hot) {
    bool first = true;
    hot = false;
    while (rem) {
      const int lead = __ffsll((long long)rem) - 1;
      const unsigned g = (unsigned)__builtin_amdgcn_readlane((int)dg, lead);
      const unsigned long long m = __ballot(act && dg == g);
      const int c = __popcll(m);
      if (lane == lead) atomicAdd(&hb[g], (unsigned)c);
      rem &= ~m;
      if (first) hot = c >= kGmPeel;
      first = false;
      if (c < kGmPeel) break;
    }
  }
  if ((rem >> lane) & 1ull) atomicAdd(&hb[dg], 1u);
}

// one value of feature slot fl (prefixes p0, p1) into the LDS table
template <typename V>
__device__ __forceinline__ void gm_count(unsigned* __restrict__ h, int fl, V v, bool live,
                                         typename KeyOf<V>::K p0, typename KeyOf<V>::K p1,
                                         typename KeyOf<V>::K mask, int sh, int lane, bool probe,
                                         bool& hot0, bool& hot1) {
  typedef typename KeyOf<V>::K K;
  const K key = KeyOf<V>::key(v);
  const unsigned dg = (unsigned)((key >> sh) & 0xFF);
  const K top = key & mask;
  gm_add(h + fl * 512, dg, live && top == p0, lane, probe, hot0);
  if (p1 != p0)  // uniform branch
    gm_add(h + fl * 512 + 256, dg, live && top == p1, lane, probe, hot1);
}

// F32X points.  blockIdx.y = chunk of kGmFeat features (nq quads of it real);
// the waves of the grid take (512-row group, quad) items with a grid stride.
__global__ __launch_bounds__(kGmThreads) void gm_hist32(const float* __restrict__ X, int64_t n,
                                                        int64_t n_pad, int d,
                                                        const unsigned long long* __restrict__ pref,
                                                        int sh, unsigned* __restrict__ H) {
  __shared__ unsigned h[kGmFeat * 512];
  __shared__ unsigned sp[kGmFeat][2];
  const int f0 = blockIdx.y * kGmFeat;
  const int nfc = min(kGmFeat, d - f0);
  const int nq = (nfc + 3) >> 2;
  for (int i = threadIdx.x; i < kGmFeat * 512; i += kGmThreads) h[i] = 0;
  for (int i = threadIdx.x; i < 2 * nfc; i += kGmThreads)
    sp[i >> 1][i & 1] = (unsigned)pref[(int64_t)f0 * 2 + i];
  __syncthreads();
  const unsigned mask = sh + 8 >= 32 ? 0u : (~0u << (sh + 8));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int kW = kGmThreads / 64;
  const int64_t groups = (n + kGmRows - 1) / kGmRows;
  const int64_t items = groups * nq;
  const float4* __restrict__ X4 = reinterpret_cast<const float4*>(X);
  for (int64_t it = (int64_t)blockIdx.x * kW + w; it < items; it += (int64_t)gridDim.x * kW) {
    const int64_t g = it / nq;
    const int q = (int)(it - g * nq);
    const int64_t r0 = g * kGmRows + lane;  // rows r0 + 64 u < n_pad (a multiple of kGmRows)
    const float4* __restrict__ src = X4 + (int64_t)((f0 >> 2) + q) * n_pad + r0;
    float4 v[kGmU];
#pragma unroll
    for (int u = 0; u < kGmU; ++u) v[u] = src[u * 64];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int fl = q * 4 + c;
      if (fl >= nfc) break;  // the zero features that pad d to d4
      const unsigned p0 = sp[fl][0], p1 = sp[fl][1];
      bool hot0 = false, hot1 = false;
#pragma unroll
      for (int u = 0; u < kGmU; ++u) {
        const float x = c == 0 ? v[u].x : c == 1 ? v[u].y : c == 2 ? v[u].z : v[u].w;
        gm_count<float>(h, fl, x, r0 + u * 64 < n, p0, p1, mask, sh, lane, u == 0, hot0, hot1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nfc * 512; i += kGmThreads) {
    const unsigned cnt = h[i];
    if (cnt) atomicAdd(&H[(int64_t)f0 * 512 + i], cnt);
  }
}

// F64 points (planar): items are (512-row group, feature); a lane loads two
// consecutive rows of the feature per 16-byte load.
__global__ __launch_bounds__(kGmThreads) void gm_hist64(const double* __restrict__ X, int64_t n,
                                                        int64_t n_pad, int d,
                                                        const unsigned long long* __restrict__ pref,
                                                        int sh, unsigned* __restrict__ H) {
  __shared__ unsigned h[kGmFeat * 512];
  __shared__ unsigned long long sp[kGmFeat][2];
  const int f0 = blockIdx.y * kGmFeat;
  const int nfc = min(kGmFeat, d - f0);
  for (int i = threadIdx.x; i < kGmFeat * 512; i += kGmThreads) h[i] = 0;
  for (int i = threadIdx.x; i < 2 * nfc; i += kGmThreads) sp[i >> 1][i & 1] = pref[(int64_t)f0 * 2 + i];
  __syncthreads();
  const unsigned long long mask = sh + 8 >= 64 ? 0ull : (~0ull << (sh + 8));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int kW = kGmThreads / 64;
  constexpr int kU2 = kGmU / 2;
  const int64_t groups = (n + kGmRows - 1) / kGmRows;
  const int64_t items = groups * nfc;
  for (int64_t it = (int64_t)blockIdx.x * kW + w; it < items; it += (int64_t)gridDim.x * kW) {
    const int64_t g = it / nfc;
    const int fl = (int)(it - g * nfc);
    const int64_t r0 = g * kGmRows + 2 * lane;  // rows r0 + 128 u + {0, 1} < n_pad
    const double2* __restrict__ src =
        reinterpret_cast<const double2*>(X + (int64_t)(f0 + fl) * n_pad + r0);
    double2 v[kU2];
#pragma unroll
    for (int u = 0; u < kU2; ++u) v[u] = src[u * 64];
    const unsigned long long p0 = sp[fl][0], p1 = sp[fl][1];
    bool hot0 = false, hot1 = false;
#pragma unroll
    for (int u = 0; u < kU2; ++u) {
      const int64_t r = r0 + u * 128;
      gm_count<double>(h, fl, v[u].x, r < n, p0, p1, mask, sh, lane, u == 0, hot0, hot1);
      gm_count<double>(h, fl, v[u].y, r + 1 < n, p0, p1, mask, sh, lane, false, hot0, hot1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nfc * 512; i += kGmThreads) {
    const unsigned cnt = h[i];
    if (cnt) atomicAdd(&H[(int64_t)f0 * 512 + i], cnt);
  }
}

static void gm_need_points(const Ctx& c) {
  if (c.mode != CDR_MODE_F32X && c.mode != CDR_MODE_F64)
    CDR_FAIL(CDR_ERR_STATE, "global medians: no points loaded");
  if (c.n >= (1ll << 32))
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "global medians: 2^32 points or more per shard");
}

static void gm_need_begun(const Ctx& c) {
  gm_need_points(c);
  if (!c.gmed_begun)
    CDR_FAIL(CDR_ERR_STATE,
             "global medians: no pass state of the current points: call "
             "cdr_medians_global_begin first");
}

// gmed_state: the global row count, then pref[2d], rank[2d], out[d]
static unsigned long long* gm_pref(const Ctx& c) {
  return reinterpret_cast<unsigned long long*>(c.gmed_state.as<long long>() + 1);
}
static long long* gm_rank(const Ctx& c) {
  return reinterpret_cast<long long*>(gm_pref(c) + 2 * (size_t)c.d);
}

int medians_global_begin(Ctx& c, int64_t n_total) {
  gm_need_points(c);
  c.gmed_begun = false;
  if (n_total < c.n) CDR_FAIL(CDR_ERR_ARG, "global medians: n_total below the local row count");
  if (n_total >= (1ll << 32))
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "global medians: 2^32 points or more");
  const size_t d = (size_t)c.d;
  c.gmed_state.ensure(sizeof(long long) * (1 + 2 * d + 2 * d) + sizeof(double) * d);
  c.gmed_hist.ensure(sizeof(unsigned) * 512 * d);
  long long* gcnt = c.gmed_state.as<long long>();
  const long long nt = n_total;
  HIP_CHECK(hipMemcpyAsync(gcnt, &nt, sizeof(long long), hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));  // nt is a stack variable
  hipLaunchKernelGGL(mg_begin, dim3(ceil_div((int64_t)d, 256)), dim3(256), 0, c.stream, gcnt,
                     c.d, 1, gm_pref(c), gm_rank(c));
  HIP_CHECK(hipGetLastError());
  c.gmed_begun = true;
  return mg_passes(c);
}

// The histogram launch alone (the table zeroed first), for both entry forms.
static void gm_launch_hist(Ctx& c, int pass) {
  const int d = c.d, P = mg_passes(c);
  const int sh = (P - 1 - pass) * 8;
  unsigned* H = c.gmed_hist.as<unsigned>();
  HIP_CHECK(hipMemsetAsync(H, 0, sizeof(unsigned) * 512 * (size_t)d, c.stream));
  if (c.n <= 0) return;
  const bool f32 = c.mode == CDR_MODE_F32X;
  const int chunks = (int)ceil_div(d, kGmFeat);
  // items of the fullest chunk, four waves per workgroup
  const int per = std::min(d, kGmFeat);
  const int64_t items = ceil_div(c.n, kGmRows) * (f32 ? (per + 3) / 4 : per);
  int64_t gx = std::max<int64_t>(1, (int64_t)lloyd_num_cus(c.device) * kGmWgPerCu / chunks);
  gx = std::min<int64_t>(gx, ceil_div(items, kGmThreads / 64));
  // (CDR_GMED_GRID: fewer workgroups per chunk, for tests of the grid stride at small n)
  if (const char* e = std::getenv("CDR_GMED_GRID"))
    gx = std::min<int64_t>(gx, std::max<int64_t>(1, std::atoll(e)));
  const dim3 grid((unsigned)gx, (unsigned)chunks);
  if (f32)
    hipLaunchKernelGGL(gm_hist32, grid, dim3(kGmThreads), 0, c.stream, c.x32.as<float>(), c.n,
                       c.n_pad, d, gm_pref(c), sh, H);
  else
    hipLaunchKernelGGL(gm_hist64, grid, dim3(kGmThreads), 0, c.stream, c.x64.as<double>(), c.n,
                       c.n_pad, d, gm_pref(c), sh, H);
  HIP_CHECK(hipGetLastError());
}

static void gm_launch_select(Ctx& c, int pass) {
  const int d = c.d, P = mg_passes(c);
  const int sh = (P - 1 - pass) * 8;
  const long long* gcnt = c.gmed_state.as<long long>();
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(mg_select<float>, dim3(ceil_div(d, 256)), dim3(256), 0, c.stream,
                       c.gmed_hist.as<unsigned>(), d, 1, gcnt, sh, gm_pref(c), gm_rank(c));
  else
    hipLaunchKernelGGL(mg_select<double>, dim3(ceil_div(d, 256)), dim3(256), 0, c.stream,
                       c.gmed_hist.as<unsigned>(), d, 1, gcnt, sh, gm_pref(c), gm_rank(c));
  HIP_CHECK(hipGetLastError());
}

static void gm_check_pass(const Ctx& c, int pass) {
  gm_need_begun(c);
  if (pass < 0 || pass >= mg_passes(c)) CDR_FAIL(CDR_ERR_ARG, "global medians: pass out of range");
}

void medians_global_pass_hist(Ctx& c, int pass, void* hist) {
  gm_check_pass(c, pass);
  gm_launch_hist(c, pass);
  HIP_CHECK(hipMemcpyAsync(hist, c.gmed_hist.p, sizeof(unsigned) * 512 * (size_t)c.d,
                           hipMemcpyDefault, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

void medians_global_pass_select(Ctx& c, int pass, const void* hist) {
  gm_check_pass(c, pass);
  HIP_CHECK(hipMemcpyAsync(c.gmed_hist.p, hist, sizeof(unsigned) * 512 * (size_t)c.d,
                           hipMemcpyDefault, c.stream));
  gm_launch_select(c, pass);
}

void medians_global_finish(Ctx& c, double* out) {
  gm_need_begun(c);
  const int d = c.d;
  const long long* gcnt = c.gmed_state.as<long long>();
  double* res = reinterpret_cast<double*>(gm_rank(c) + 2 * (size_t)d);
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(mg_finish<float>, dim3(ceil_div(d, 256)), dim3(256), 0, c.stream, gcnt, d,
                       1, gm_pref(c), res);
  else
    hipLaunchKernelGGL(mg_finish<double>, dim3(ceil_div(d, 256)), dim3(256), 0, c.stream, gcnt, d,
                       1, gm_pref(c), res);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, res, sizeof(double) * d, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

// One shard: every pass enqueued back to back, one wait at the end.  The
// histogram launches are bracketed by events (cdr_medians_global_timing).
void medians_global(Ctx& c, double* out) {
  const int P = medians_global_begin(c, c.n);
  std::vector<hipEvent_t> ev(2 * (size_t)P, nullptr);
  for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
  try {
    for (int p = 0; p < P; ++p) {
      HIP_CHECK(hipEventRecord(ev[2 * p], c.stream));
      gm_launch_hist(c, p);
      HIP_CHECK(hipEventRecord(ev[2 * p + 1], c.stream));
      gm_launch_select(c, p);
    }
    medians_global_finish(c, out);
    double total = 0.0, longest = 0.0;
    for (int p = 0; p < 8; ++p) c.gmed_ms[3 + p] = 0.0;
    for (int p = 0; p < P; ++p) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * p], ev[2 * p + 1]));
      total += ms;
      longest = std::max(longest, (double)ms);
      c.gmed_ms[3 + p] = ms;
    }
    c.gmed_ms[0] = total;
    c.gmed_ms[1] = longest;
    c.gmed_ms[2] = (double)P;
  } catch (...) {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    throw;
  }
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

/* ---- medians of all points: src/main.py:31-38, src/scoring.py:50-54 ---- */
int cdr_medians_global(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_global(h->c, out);
  CDR_CATCH
}

int cdr_medians_global_begin(cdr_ctx* h, int64_t n_total, int32_t* passes, int64_t* hist_words) {
  CDR_TRY
  if (!h || !passes || !hist_words) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  *passes = medians_global_begin(h->c, n_total);
  *hist_words = (int64_t)h->c.d * 512;
  CDR_CATCH
}

int cdr_medians_global_pass_hist(cdr_ctx* h, int32_t pass, void* hist) {
  CDR_TRY
  if (!h || !hist) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_global_pass_hist(h->c, pass, hist);
  CDR_CATCH
}

int cdr_medians_global_pass_select(cdr_ctx* h, int32_t pass, const void* hist) {
  CDR_TRY
  if (!h || !hist) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_global_pass_select(h->c, pass, hist);
  CDR_CATCH
}

int cdr_medians_global_finish(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_global_finish(h->c, out);
  CDR_CATCH
}

int cdr_medians_global_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 11; ++i) out[i] = h->c.gmed_ms[i];
  CDR_CATCH
}

int cdr_medians_segmented(cdr_ctx* h, const double* values, const int64_t* offsets,
                          int64_t n_segments, double* out) {
  CDR_TRY
  if (!h || !offsets || (n_segments > 0 && !out)) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_segmented(h->c, values, offsets, n_segments, out);
  CDR_CATCH
}

int cdr_medians_group(cdr_ctx* h, int32_t k, int64_t* counts) {
  CDR_TRY
  if (!h || !counts) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_group(h->c, k, counts);
  CDR_CATCH
}

int cdr_medians_begin(cdr_ctx* h, const int64_t* global_counts, int32_t* passes,
                      int64_t* hist_words) {
  CDR_TRY
  if (!h || !global_counts || !passes || !hist_words) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  *passes = medians_begin(h->c, global_counts);
  *hist_words = (int64_t)h->c.med_k * h->c.d * 512;
  CDR_CATCH
}

int cdr_medians_pass_hist(cdr_ctx* h, int32_t pass, void* hist) {
  CDR_TRY
  if (!h || !hist) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_pass_hist(h->c, pass, hist);
  CDR_CATCH
}

int cdr_medians_pass_select(cdr_ctx* h, int32_t pass, const void* hist) {
  CDR_TRY
  if (!h || !hist) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_pass_select(h->c, pass, hist);
  CDR_CATCH
}

int cdr_medians_finish(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_finish(h->c, out);
  CDR_CATCH
}

int cdr_medians_by_label(cdr_ctx* h, int32_t k, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  medians_by_label(h->c, k, out);
  CDR_CATCH
}

}  // extern "C"
