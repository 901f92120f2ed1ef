// f64_assign.hip — the F64 step's assignment fused with the block pass of
// the exact sums (f64sum.hip): labels by the exact argmin behind an fp32
// screen, and each 256-row block's approximate sums and member counts, in
// one pass over the points (2 <= d <= 16, k <= 64); f64_step_fused, the whole
// step on the context stream.
#include <cmath>

#include "cdr_internal.h"
#include "exact_math.h"
#include "f64sum.h"

namespace cdr {

namespace {

// The exact argmin (exact_argmin: the first index of the smallest correctly
// rounded NumPy-order root) behind an fp32 screen, for k <= kF64ScrK.  With
// every x_f and c_f zero or within [2^-60, 2^60] (normal fp32 squares), the
// fp32 value S = fma-chain sum of fl32(fl32(x) - fl32(c))^2 is within
//   (d + 5.01) 2^-24 sum_f (|x_f| + |c_f|)^2 <= (d + 5.01) 2^-23 (|x|^2 + |c|^2)
// of the real squared distance (two conversions and a subtraction per term,
// d fused steps of non-negative terms), plus 2^-126 per step for a result
// flushed below the normal range.  E = (d + 12) 2^-23 (xx + cc) + d 2^-125
// (xx, cc: the fp32 squared norms) covers that, the two roundings of S -+ E,
// the fp64 NumPy sum's own error and a relative gap of 2^-48 beyond it.  So a
// centroid with S - E > min_i (S_i + E_i) has an fp64 square at least 2^-48
// above the winner's and a strictly larger rounded root: it can neither win
// nor tie.  The rest (usually the winner alone) go through exact_argmin's
// comparison in index order, which gives exact_argmin's answer.  fp64 VALU is
// a quarter of the fp32 rate on gfx950 and the full pass was issue-bound
// (PMC: 66 % of wave cycles stalled on issue).
constexpr int kF64ScrK = 16;
// a centroid's fp32 row in LDS: its d values, then its squared norm, padded
// to whole 16-byte reads
template <int D>
struct F64ScrRow {
  static constexpr int P = (D + 1 + 3) & ~3;
};
__device__ __forceinline__ bool f64_screen_ok(double v) {
  const double a = fabs(v);
  return v == 0.0 || (a >= 0x1p-60 && a <= 0x1p60);
}
template <int D>
__device__ __forceinline__ int f64_screen_argmin(const double (&xr)[D], const double* cs64,
                                                 const float* cs32, int k) {
  constexpr int DP = F64ScrRow<D>::P;
  typedef float f4v __attribute__((ext_vector_type(4)));
  float xs[D];
  float xx = 0.0f;
  bool ok = true;
#pragma unroll
  for (int f = 0; f < D; ++f) {
    ok &= f64_screen_ok(xr[f]);
    xs[f] = (float)xr[f];
    xx = fmaf(xs[f], xs[f], xx);
  }
  if (!ok) return exact_argmin([&](int f) { return xr[f]; }, cs64, k, D);
  const float kE = (float)(D + 12) * 0x1p-23f, eabs = (float)D * 0x1p-125f;
  float lo[kF64ScrK];
  float best = INFINITY;
#pragma unroll
  for (int jj = 0; jj < kF64ScrK; ++jj) {
    lo[jj] = INFINITY;
    if (jj < k) {
      f4v cr[DP / 4];
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) cr[q] = reinterpret_cast<const f4v*>(cs32 + jj * DP)[q];
      float acc = 0.0f;
#pragma unroll
      for (int f = 0; f < D; ++f) {
        const float t = xs[f] - cr[f >> 2][f & 3];
        acc = fmaf(t, t, acc);
      }
      const float e = fmaf(kE, xx + cr[D >> 2][D & 3], eabs);
      lo[jj] = acc - e;
      best = fminf(best, acc + e);
    }
  }
  unsigned cand = 0;
#pragma unroll
  for (int jj = 0; jj < kF64ScrK; ++jj)
    if (lo[jj] <= best) cand |= 1u << jj;
  double Rb = INFINITY, rb = INFINITY;
  int jb = 0;
  while (cand) {
    const int jj = __builtin_ctz(cand);
    cand &= cand - 1u;
    const double* cj = cs64 + jj * D;
    const double R = np_sqdist([&](int f) { return xr[f]; }, [&](int f) { return cj[f]; }, D);
    if (R < Rb) {
      const double r = sqrt(R);
      if (r < rb) {
        rb = r;
        Rb = R;
        jb = jj;
      }
    }
  }
  return jb;
}

// The screen's centroid table for one step (every f64_assign_block workgroup
// staged it in LDS before): the fp32 rows with their fp32 squared norms, as
// f64_screen_argmin reads them, and ok[0] = 1 when the screen applies (k <= 16,
// every value 0 or within [2^-60, 2^60]).  The assignment reads the rows with
// uniform addresses, i.e. scalar loads, instead of 32 LDS reads per row.
template <int D>
__global__ __launch_bounds__(64) void f64_cent_prep(const double* __restrict__ C, int k,
                                                    float* __restrict__ cs32, int* __restrict__ ok) {
  constexpr int DP = F64ScrRow<D>::P;
  const int t = threadIdx.x;
  bool bad = k > kF64ScrK;
  if (t < kF64ScrK) {
    float row[DP];
#pragma unroll
    for (int q = 0; q < DP; ++q) row[q] = 0.0f;
    if (t < k) {
#pragma unroll
      for (int f = 0; f < D; ++f) {
        const double v = C[t * D + f];
        row[f] = (float)v;
        bad |= !f64_screen_ok(v);
      }
      float sq = 0.0f;
#pragma unroll
      for (int f = 0; f < D; ++f) sq = fmaf(row[f], row[f], sq);
      row[D] = sq;
    }
#pragma unroll
    for (int q = 0; q < DP; ++q) cs32[t * DP + q] = row[q];
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (t == 0) ok[0] = any_bad ? 0 : 1;
}

// F64 mode, the assignment fused with the block pass (one workgroup per
// block of kFB rows): labels (exact_argmin, src/kmeans_plusplus.py:33-34)
// and the block's approximate sums and exact counts in f64_blocksum's
// layout.  cs32g, scr_ok: f64_cent_prep's table and whether the screen
// applies.  2 <= D <= 16, k <= 64.
template <int D>
__global__ __launch_bounds__(kFB) void f64_assign_block(const double* __restrict__ X, int64_t n,
                                                        int64_t n_pad,
                                                        const double* __restrict__ C, int k,
                                                        int32_t* __restrict__ labels,
                                                        double* __restrict__ A,
                                                        unsigned* __restrict__ cnt,
                                                        const long long* __restrict__ gate,
                                                        const float* __restrict__ cs32g,
                                                        const int* __restrict__ scr_ok,
                                                        int* __restrict__ dlab) {
  // (the device-resident F64 run: a stopped run keeps the labels of the
  // assignment that stopped it)
  if (gate && gate[0] == 0) return;
  __shared__ double tab[kFMaxK * D];
  __shared__ unsigned cc[kFMaxK];
  // Workgroups are dealt round-robin over the 8 XCDs; XCD x takes the
  // contiguous block range x * (nb / 8) + min(x, nb % 8) + [0, its share), so
  // the 8-byte writes of consecutive blocks into the sequence-major A and cnt
  // rows meet in one L2 and leave it as whole lines (with blockIdx.x as the
  // block, neighbouring blocks sit in different L2s and every write is partial)
  const int64_t nb = gridDim.x;
  const int64_t bq = nb >> 3, brm = nb & 7, bx = blockIdx.x & 7;
  const int64_t b = bx * bq + (bx < brm ? bx : brm) + (blockIdx.x >> 3);
  for (int i = threadIdx.x; i < k * D; i += kFB) tab[i] = 0.0;
  if (threadIdx.x < kFMaxK) cc[threadIdx.x] = 0u;
  const int64_t row = b * kFB + threadIdx.x;
  double xr[D];
  int jold = -1;  // (dlab: the previous label, for the transfer cache)
  if (row < n) {
#pragma unroll
    for (int f = 0; f < D; ++f) xr[f] = X[xidx(X, f, row, n_pad)];
    if (dlab) jold = labels[row];
  }
  // the screen's table (f64_cent_prep: fp32 rows and their fp32 squared
  // norms, read with uniform addresses) and the fp64 centroids for its
  // candidates, straight from global memory
  __syncthreads();  // (the zeroed tables)
  int j = -1;
  if (row < n) {
    j = scr_ok[0] ? f64_screen_argmin<D>(xr, C, cs32g, k)
                  : exact_argmin([&](int f) { return xr[f]; }, C, k, D);
    labels[row] = j;
  }
  // (the barrier; with dlab also whether any row of the block changed label)
  const int moved = __syncthreads_or(j != jold && dlab != nullptr);
  if (dlab && threadIdx.x == 0) dlab[b] = moved;
  if (j >= 0) {
    atomicAdd(&cc[j], 1u);
#pragma unroll
    for (int f = 0; f < D; ++f) atomicAdd(&tab[j * D + f], xr[f]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k * D; i += kFB) A[(int64_t)i * nb + b] = tab[i];
  for (int i = threadIdx.x; i < k; i += kFB) cnt[(int64_t)i * nb + b] = cc[i];
}

}  // namespace

void enqueue_f64_assign(Ctx& c, int k, const double* dC, const long long* gate, int* dlab) {
  const int d = c.d;
  if (d < 2 || d > 16 || k < 1 || k > kFMaxK || c.n < 1)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "F64 assignment: 2 <= d <= 16, k <= 64 and a point");
  const int64_t n = c.n, nb = ceil_div(n, kFB);
  c.f64x_A.ensure(sizeof(double) * nb * k * d);
  c.f64x_cnt.ensure(sizeof(unsigned) * nb * k);
  constexpr int kRows = kF64ScrK * 20;  // (DP <= 20 floats at d <= 16)
  c.f64x_cs.ensure(sizeof(float) * kRows + 64);
  float* cs = c.f64x_cs.as<float>();
  int* ok = reinterpret_cast<int*>(cs + kRows);
  struct Fns {
    void (*prep)(const double*, int, float*, int*);
    void (*assign)(const double*, int64_t, int64_t, const double*, int, int32_t*, double*,
                   unsigned*, const long long*, const float*, const int*, int*);
  };
#define CDR_F64_D(D_) {f64_cent_prep<D_>, f64_assign_block<D_>}
  static const Fns fns[15] = {CDR_F64_D(2),  CDR_F64_D(3),  CDR_F64_D(4),  CDR_F64_D(5),
                              CDR_F64_D(6),  CDR_F64_D(7),  CDR_F64_D(8),  CDR_F64_D(9),
                              CDR_F64_D(10), CDR_F64_D(11), CDR_F64_D(12), CDR_F64_D(13),
                              CDR_F64_D(14), CDR_F64_D(15), CDR_F64_D(16)};
#undef CDR_F64_D
  const Fns& fn = fns[d - 2];
  hipLaunchKernelGGL(fn.prep, dim3(1), dim3(64), 0, c.stream, dC, k, cs, ok);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fn.assign, dim3((unsigned)nb), dim3(kFB), 0, c.stream, c.x64.as<double>(), n,
                     c.n_pad, dC, k, c.labels.as<int32_t>(), c.f64x_A.as<double>(),
                     c.f64x_cnt.as<unsigned>(), gate, cs, ok, dlab);
  HIP_CHECK(hipGetLastError());
}

// The F64 step's assignment and sums as one pipeline: f64_assign_block
// (labels, block sums and counts), then the cluster counts, the binade
// predictions, the transfers, groups and walk (f64sum.hip).  false: shape not
// covered (d > 16, d < 2, k > 64), nothing launched.
bool f64_step_fused(Ctx& c, int k, const double* dC, double* d_sums,
                    unsigned long long* d_counts, bool prof, const long long* gate,
                    int tcache) {
  const int d = c.d;
  if (d < 2 || d > 16 || k < 1 || k > kFMaxK || c.n < 1) return false;
  const int64_t nb = ceil_div(c.n, kFB);
  // The transfer cache (tcache != 0, the device run's steps): a block keeps
  // its transfers when none of its labels changed in this assignment and none
  // of its binade predictions moved since they were formed — its (cluster,
  // feature) sequences then hold the same values under the same binades, so
  // the transfers are the same integers.  Near convergence few blocks change.
  F64TCache tc;
  const bool use_tc = tcache != 0;
  if (use_tc) {
    const size_t need = sizeof(int) * (3 * (size_t)nb + 2);
    const bool fresh = c.f64x_dirty.bytes < need;
    c.f64x_dirty.ensure(need);
    int* base = c.f64x_dirty.as<int>();
    tc.dlab = base;
    tc.dE = base + nb;
    tc.list = base + 2 * nb;
    tc.counters = base + 3 * nb;
    tc.stamp = ++c.f64x_stamp;
    tc.par = tc.stamp & 1;
    tc.all = tcache == 1 || fresh;
    if (tc.all) HIP_CHECK(hipMemsetAsync(tc.counters, 0, 2 * sizeof(int), c.stream));
  }
  enqueue_f64_assign(c, k, dC, gate, use_tc ? const_cast<int*>(tc.dlab) : nullptr);
  if (prof) prof_mark(c, 1);
  // (the counts: written by f64_predict_b from f64_predict_a's group counts)
  enqueue_f64_sums_after_block(c, k, d_sums, F64Shard(), d_counts, use_tc ? &tc : nullptr);
  return true;
}

}  // namespace cdr

