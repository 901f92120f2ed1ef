// seed_f32r.hip — the reference's float32 k-means++ seeding, step by step
// from the host (f32r_seed_update) and device-resident (f32r_seed_run).
#include <algorithm>
#include <cmath>
#include <vector>

#include "cdr_internal.h"
#include "exact_math.h"
#include "seed_common.h"

namespace cdr {

// ---------------------------------------------------------------------------
// The reference's float32 runs (X float32 keeps its dtype:
// src/kmeans_plusplus.py:6): dist_sq, its sum and the probabilities are
// float32 arrays there.
//   t       = np.linalg.norm(X - c, axis=2)   fp32 NumPy order, one rounded sqrt (:15)
//   dist_sq = min(dist_sq, t ** 2)            fp32 square; np.min keeps NaN (:14)
//   total   = dist_sq.sum()                   fp32: 8192-element chunks pairwise,
//                                             chunks added left to right (:18)
//   probs   = dist_sq / total                 fp32 (:18)
// and Generator.choice converts p to float64 before its cumsum (:19), so the
// exact cumsum scan (seed_scan) runs unchanged on p as doubles with S = 1.
// ---------------------------------------------------------------------------
template <typename S, int D>
__global__ __launch_bounds__(256) void f32r_min_kernel(const S* __restrict__ X, int64_t n,
                                                       int64_t n_pad, int d,
                                                       const float* __restrict__ cen,
                                                       float* __restrict__ dmin32,
                                                       int* __restrict__ infflag) {
  const int dd = D ? D : d;
  bool inf = false;
  for (int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pt < n;
       pt += (int64_t)gridDim.x * blockDim.x) {
    auto xv = [&](int f) { return (float)X[xidx(X, f, pt, n_pad)]; };  // exact: fp32 values
    auto cv = [&](int f) { return cen[f]; };
    const float R = np_sqdist<decltype(xv), decltype(cv), float>(xv, cv, dd);
    const float t = (float)sqrt((double)R);  // = the correctly rounded fp32 sqrt
    const float t2 = t * t;
    const float m = dmin32[pt];
    const float v = (m != m || t2 != t2) ? NAN : (t2 < m ? t2 : m);
    dmin32[pt] = v;
    inf = inf || isinf(v);
  }
  // (device-resident run: an infinite dist_sq makes probs inf / inf = NaN)
  if (infflag && __ballot(inf)) {
    if ((threadIdx.x & 63) == __ffsll((long long)__ballot(inf)) - 1) atomicOr(infflag, 1);
  }
}
// f32r_min_kernel for the context's points (S) and d (unrolled for D = 2, 5,
// 8, 16); infflag: nullptr when the host takes the total.
template <typename S>
static void f32r_min_launch(Ctx& c, const S* X, const float* dcen, int* infflag) {
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(c.n, 256), 4096)));
  auto fn = f32r_min_kernel<S, 0>;
  switch (c.d) {
    case 2: fn = f32r_min_kernel<S, 2>; break;
    case 5: fn = f32r_min_kernel<S, 5>; break;
    case 8: fn = f32r_min_kernel<S, 8>; break;
    case 16: fn = f32r_min_kernel<S, 16>; break;
  }
  hipLaunchKernelGGL(fn, grid, dim3(256), 0, c.stream, X, c.n, c.n_pad, c.d, dcen,
                     c.dmin32.as<float>(), infflag);
  HIP_CHECK(hipGetLastError());
}
static void f32r_min_enqueue(Ctx& c, const float* dcen, int* infflag) {
  if (c.mode == CDR_MODE_F32X)
    f32r_min_launch(c, c.x32.as<float>(), dcen, infflag);
  else
    f32r_min_launch(c, c.x64.as<double>(), dcen, infflag);
}
__global__ void f32r_fill_kernel(float* __restrict__ p, int64_t n_pad, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = i < n ? INFINITY : 0.0f;
}
// fp32 pairwise sum of each 8192-element chunk: a full chunk is the perfect
// tree over 64 leaves of 128 (lane l: leaf l, combined left + right by
// shuffles); the partial last chunk runs the whole recursion on one lane.
__global__ __launch_bounds__(64) void f32r_block_kernel(const float* __restrict__ dmin32,
                                                        int64_t n, float* __restrict__ bs32) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t base = b * kSeedBlock;
  if (base + kSeedBlock <= n) {
    const float* src = dmin32 + base + lane * 128;
    auto leaf = [&](int i) { return src[i]; };
    float v = np_pw_leaf<decltype(leaf), float>(leaf, 128);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float r = __shfl_down(v, o);
      if ((lane & (2 * o - 1)) == 0) v = v + r;
    }
    if (lane == 0) bs32[b] = v;
  } else if (lane == 0) {
    auto all = [&](int64_t i) { return dmin32[base + i]; };
    bs32[b] = np_pairwise<decltype(all), float>(all, n - base);
  }
}
// p = fl32(dist_sq / total) as doubles (the scan's dmin, rows >= n zero) and
// each chunk's sum in any order (the scan's binade guesses only)
__global__ __launch_bounds__(256) void f32r_prob_kernel(const float* __restrict__ dmin32,
                                                        int64_t n, float total_v,
                                                        double* __restrict__ dmin,
                                                        double* __restrict__ bs,
                                                        const float* __restrict__ dtotal) {
  __shared__ double red[4];
  const int64_t b = blockIdx.x;
  const float total = dtotal ? dtotal[0] : total_v;
  double acc = 0.0;
  for (int i = threadIdx.x; i < kSeedBlock; i += 256) {
    const int64_t pt = b * kSeedBlock + i;
    // fp32 division via fp64: fl32(fl64(a / b)) = fl32(a / b) for fp32 a, b
    const double p = pt < n ? (double)(float)((double)dmin32[pt] / (double)total) : 0.0;
    dmin[pt] = p;
    acc += p;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) bs[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

void f32r_seed_update(Ctx& c, const float* cen, int reset, float* total_out) {
  check_points(c);
  const int64_t nb = c.nblocks();
  c.dmin32.ensure(sizeof(float) * (size_t)(c.n_pad > 0 ? c.n_pad : 1));
  c.dmin.ensure(sizeof(double) * (size_t)(c.n_pad > 0 ? c.n_pad : 1));
  c.blocksums.ensure(sizeof(double) * (nb > 0 ? nb : 1));
  c.bs32.ensure(sizeof(float) * (nb > 0 ? nb : 1));
  c.seed_scalar.ensure(sizeof(double) * (2 * c.d + 8));
  if (reset) {
    hipLaunchKernelGGL(f32r_fill_kernel, dim3(2048), dim3(256), 0,
                       c.stream, c.dmin32.as<float>(), c.n_pad, c.n);
    HIP_CHECK(hipGetLastError());
  }
  float* dcen = reinterpret_cast<float*>(c.seed_scalar.p);
  HIP_CHECK(hipMemcpyAsync(dcen, cen, sizeof(float) * c.d, hipMemcpyHostToDevice, c.stream));
  f32r_min_enqueue(c, dcen, nullptr);
  float total = 0.0f;
  if (nb > 0) {
    hipLaunchKernelGGL(f32r_block_kernel, dim3((unsigned)nb), dim3(64), 0, c.stream,
                       c.dmin32.as<float>(), c.n, c.bs32.as<float>());
    HIP_CHECK(hipGetLastError());
    std::vector<float> bs((size_t)nb);
    HIP_CHECK(hipMemcpyAsync(bs.data(), c.bs32.p, sizeof(float) * nb, hipMemcpyDeviceToHost,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    for (float v : bs) total = total + v;  // NumPy: the chunks from 0, left to right (fp32)
  }
  *total_out = total;
  if (!(total > 0.0f) || std::isinf(total)) CDR_FAIL(CDR_ERR_NAN, "Probabilities contain NaN");
  if (nb > 0) {
    hipLaunchKernelGGL(f32r_prob_kernel, dim3((unsigned)nb), dim3(256), 0, c.stream,
                       c.dmin32.as<float>(), c.n, total, c.dmin.as<double>(),
                       c.blocksums.as<double>(), nullptr);
    HIP_CHECK(hipGetLastError());
  }
  c.seed_scanned = false;
  c.seed_prog_ready = false;
}

// ---- the reference's float32 seeding, every step on the device ----------
// The pick's row as the fp32 centre.
__global__ __launch_bounds__(64) void f32r_gather_kernel(const float* __restrict__ x32,
                                                         const double* __restrict__ x64,
                                                         const int64_t* __restrict__ pick, int d,
                                                         int64_t n_pad, float* __restrict__ cen) {
  // (a step after a bad total searches probabilities that may all be 0 and
  // find no row, -1: its pick is never used, the run raises; row 0 keeps the
  // gather in bounds)
  int64_t p = pick[0];
  if (p < 0 || p >= n_pad) p = 0;
  for (int f = threadIdx.x; f < d; f += 64)
    cen[f] = x32 ? x32[xidx(x32, f, p, n_pad)] : (float)x64[xidx(x64, f, p, n_pad)];
}
// dist_sq.sum() in fp32: the chunk sums from 0, left to right (one lane:
// the additions are sequential), and the step's verdict as Generator.choice
// gives it: a NaN, zero or infinite total with an infinite dist_sq
// (probs inf / inf) or a NaN is "Probabilities contain NaN" (code 1); an
// infinite total from finite dist_sq (overflow: probs all 0) is
// "probabilities do not sum to 1" (code 2).  The first bad step's code is
// kept; later steps run on total 1 (their picks are never used).
__global__ __launch_bounds__(64) void f32r_total_kernel(const float* __restrict__ bs32,
                                                        int64_t nb, int* __restrict__ infflag,
                                                        float* __restrict__ dtotal,
                                                        double* __restrict__ dbad) {
  float total = wave_seq_sum(bs32, nb);
  if (threadIdx.x != 0) return;
  if (!(total > 0.0f) || isinf(total)) {
    const double code = (isinf(total) && total > 0.0f && infflag[0] == 0) ? 2.0 : 1.0;
    if (dbad[0] == 0.0) dbad[0] = code;
    total = 1.0f;
  }
  infflag[0] = 0;
  dtotal[0] = total;
}

void f32r_seed_run(Ctx& c, int64_t first, int k, const double* u, int64_t* picks) {
  check_points(c);
  if (k < 1) CDR_FAIL(CDR_ERR_ARG, "k >= 1");
  if (first < 0 || first >= c.n) CDR_FAIL(CDR_ERR_ARG, "first row out of range");
  picks[0] = first;
  if (k == 1) return;
  const int64_t nb = c.nblocks();
  const int d = c.d;
  // [u: k-1][picks: k][bad x2][total f32 | inf flag][centre f32 x d]
  const size_t words = (size_t)(k - 1) + (size_t)k + 3 + (size_t)(d + 1) / 2 + 1;
  c.seed_run_buf.ensure(sizeof(double) * words);
  double* du = c.seed_run_buf.as<double>();
  int64_t* dpick = reinterpret_cast<int64_t*>(du + (k - 1));
  double* dbad = du + (k - 1) + k;
  float* dtotal = reinterpret_cast<float*>(dbad + 2);
  int* dinf = reinterpret_cast<int*>(dtotal + 1);
  float* dcen = reinterpret_cast<float*>(dbad + 3);
  HIP_CHECK(hipMemcpyAsync(du, u, sizeof(double) * (k - 1), hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemcpyAsync(dpick, &first, sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemsetAsync(dbad, 0, sizeof(double) * 3, c.stream));
  c.dmin32.ensure(sizeof(float) * (size_t)(c.n_pad > 0 ? c.n_pad : 1));
  c.dmin.ensure(sizeof(double) * (size_t)(c.n_pad > 0 ? c.n_pad : 1));
  c.blocksums.ensure(sizeof(double) * (nb > 0 ? nb : 1));
  c.bs32.ensure(sizeof(float) * (nb > 0 ? nb : 1));
  c.cend.ensure(sizeof(double) * nb * 2);
  c.seg_meta.ensure(sizeof(long long) * 8);
  hipLaunchKernelGGL(f32r_fill_kernel, dim3(2048), dim3(256), 0, c.stream, c.dmin32.as<float>(),
                     c.n_pad, c.n);
  HIP_CHECK(hipGetLastError());
  const float* x32 = c.mode == CDR_MODE_F32X ? c.x32.as<float>() : nullptr;
  const double* x64 = c.mode == CDR_MODE_F64 ? c.x64.as<double>() : nullptr;
  for (int i = 1; i < k; ++i) {
    hipLaunchKernelGGL(f32r_gather_kernel, dim3(1), dim3(64), 0, c.stream, x32, x64,
                       dpick + (i - 1), d, c.n_pad, dcen);
    f32r_min_enqueue(c, dcen, dinf);
    hipLaunchKernelGGL(f32r_block_kernel, dim3((unsigned)std::max<int64_t>(nb, 1)), dim3(64), 0,
                       c.stream, c.dmin32.as<float>(), c.n, c.bs32.as<float>());
    hipLaunchKernelGGL(f32r_total_kernel, dim3(1), dim3(64), 0, c.stream, c.bs32.as<float>(), nb,
                       dinf, dtotal, dbad);
    hipLaunchKernelGGL(f32r_prob_kernel, dim3((unsigned)std::max<int64_t>(nb, 1)), dim3(256), 0,
                       c.stream, c.dmin32.as<float>(), c.n, 1.0f, c.dmin.as<double>(),
                       c.blocksums.as<double>(), dtotal);
    HIP_CHECK(hipGetLastError());
    // Generator.choice on the float64 probabilities: the exact cumsum scan
    // (program, then the gated block walk) and the search, S = 1
    seed_step_resident(c, nullptr, du + (i - 1), dpick + i);
  }
  double bad[2];
  HIP_CHECK(hipMemcpyAsync(picks, dpick, sizeof(int64_t) * k, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipMemcpyAsync(bad, dbad, sizeof(bad), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.seed_scanned = false;
  c.seed_prog_ready = false;
  if (bad[0] == 2.0) CDR_FAIL(CDR_ERR_NAN, "probabilities do not sum to 1");
  if (bad[0] != 0.0) CDR_FAIL(CDR_ERR_NAN, "Probabilities contain NaN");
  if (bad[1] != 0.0) CDR_FAIL(CDR_ERR_STATE, "k-means++ sampler found no index");
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_f32r_seed_run(cdr_ctx* h, int64_t first, int32_t k, const double* u, int64_t* picks) {
  CDR_TRY
  if (!h || !picks || (k > 1 && !u)) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  f32r_seed_run(h->c, first, (int)k, u, picks);
  CDR_CATCH
}

int cdr_f32r_seed_update(cdr_ctx* h, const float* c, int32_t reset, float* total) {
  CDR_TRY
  if (!h || !c || !total) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  f32r_seed_update(h->c, c, reset, total);
  CDR_CATCH
}

}  // extern "C"
