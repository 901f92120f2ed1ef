// lloyd_f64.hip — the F64 Lloyd step (arbitrary fp64 data): exact fp64
// assignment for every point and a row-ordered fp64 sum per (cluster,
// feature) — NumPy's X[mask].mean(axis=0) is a sequential row-order sum for
// d >= 2 and the blocked pairwise sum for d == 1 (oracle/kmeans_oracle.py
// pins both against NumPy); the device-resident F64 run and the sharded F64
// sums' entry points (their other kernels: f64sum.hip, f64_assign.hip,
// f64_sharded.hip, lloyd_exact.hip).
#include <cstdio>
#include <cmath>

#include "cdr_internal.h"
#include "exact_math.h"

namespace cdr {

void read_walked(Ctx& c, int k) {
  std::vector<long long> w((size_t)k * c.d);
  HIP_CHECK(hipMemcpyAsync(w.data(), c.f64x_walk.p, sizeof(long long) * w.size(),
                           hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.f64x_walked = 0;
  for (long long v : w) c.f64x_walked += v;
}

void copy_back_sums(Ctx& c, int k, const long long* d_counts, double* sums, int64_t* counts,
                    bool walked) {
  HIP_CHECK(hipMemcpyAsync(sums, c.f64_sums.p, sizeof(double) * (size_t)k * c.d,
                           hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipMemcpyAsync(counts, d_counts, sizeof(long long) * k, hipMemcpyDeviceToHost,
                           c.stream));
  if (walked) read_walked(c, k);
  else HIP_CHECK(hipStreamSynchronize(c.stream));
}

// F64 mode: sums[j][f] = row-ordered fp64 sum of X[labels == j][:, f] and
// counts[j].  One thread per (j, f); f == d counts.  d == 1 follows NumPy's
// contiguous reduction instead: blocked (8192) pairwise over the selection.
__global__ void seq_sums_f64(const double* __restrict__ X, int64_t n, int64_t n_pad, int d,
                             int k, const int32_t* __restrict__ labels,
                             const long long* __restrict__ counts_in,
                             double* __restrict__ sums, long long* __restrict__ counts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * (d + 1)) return;
  const int j = t / (d + 1), f = t % (d + 1);
  if (f == d) {
    long long c = 0;
    for (int64_t i = 0; i < n; ++i) c += (labels[i] == j);
    counts[j] = c;
    return;
  }
  auto col = [&](int64_t i) { return X[xidx(X, f, i, n_pad)]; };
  if (d >= 2) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i)
      if (labels[i] == j) s = s + col(i);
    sums[(size_t)j * d + f] = s;
    return;
  }
  // d == 1: res = 0; res += pairwise(block) for each 8192-block of the selection.
  const long long m = counts_in[j];
  int64_t cursor = 0;
  auto next = [&](int64_t) -> double {
    while (labels[cursor] != j) ++cursor;
    return col(cursor++);
  };
  double res = 0.0;
  for (long long done = 0; done < m; done += kSeedBlock) {
    const long long blk = (m - done) < kSeedBlock ? (m - done) : kSeedBlock;
    res = res + np_pairwise(next, blk);
  }
  sums[j] = res;
}

// The device-resident F64 run's update (one workgroup, after each fused
// step): means = sums / counts (np.mean's true division), shift =
// ||means - C|| (src/kmeans_plusplus.py:37-48).  The step is applied on the
// device when every cluster has members and the shift is clear of tol: C =
// means, and the run stops once shift < tol.  An empty cluster (the reference
// reseeds it from np.random) or a shift within 2^-36 of tol (the reference's
// BLAS summation order is not ours) stops the run WITHOUT applying the step:
// the host finishes that step from the kept means and counts.  The shift's
// square is summed in a fixed tree: <= 1024 non-negative terms, within 2^-42
// of any other order's, so the margin decides both sides rigorously.
constexpr int kF64RunThreads = 1024;
__global__ __launch_bounds__(kF64RunThreads) void f64_run_update(
    const double* __restrict__ sums, unsigned long long* __restrict__ counts,
    double* __restrict__ C, double* __restrict__ keep, int k, int d, double tol,
    long long* __restrict__ st) {
  __shared__ double red[kF64RunThreads / 64];
  __shared__ int empty_any;
  if (st[0] == 0) return;  // (uniform) stopped: this step's kernels ran for nothing
  const int t = threadIdx.x, kd = k * d;
  if (t == 0) empty_any = 0;
  __syncthreads();
  double m = 0.0, sq = 0.0;
  if (t < kd) {
    const unsigned long long cnt = counts[t / d];
    m = sums[t] / (double)cnt;
    if (cnt == 0) {
      empty_any = 1;
    } else {
      const double df = m - C[t];
      sq = df * df;
    }
    keep[t] = m;
    if (t % d == 0) reinterpret_cast<long long*>(keep + kd)[t / d] = (long long)cnt;
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if ((t & 63) == 0) red[t >> 6] = sq;
  __syncthreads();
  double ss = 0.0;
#pragma unroll
  for (int w = 0; w < kF64RunThreads / 64; ++w) ss += red[w];
  const double sh = sqrt(ss);
  const double mg = 0x1p-36;
  long long reason = 0;  // 0: applied, go on; 1: applied, converged; 2: the host's step
  if (empty_any) reason = 2;
  else if (tol > 0.0 && !(sh > tol * (1.0 + mg))) reason = sh < tol * (1.0 - mg) ? 1 : 2;
  if (reason != 2 && t < kd) C[t] = m;
  if (t == 0) {
    if (reason != 2) st[1] += 1;
    st[2] = reason;
    st[3] = __double_as_longlong(ss);
    if (reason != 0) st[0] = 0;
  }
}

// cdr_lloyd_f64_run: up to max_steps fused F64 steps (f64_assign.hip) with the
// update above on the device; one synchronisation at the end.
static void lloyd_run_f64(Ctx& c, const double* C, int32_t k, int32_t max_steps, double tol,
                          double* C_out, double* means_out, int64_t* counts_out, int32_t* info) {
  check_k(c, k);
  if (c.mode != CDR_MODE_F64) CDR_FAIL(CDR_ERR_STATE, "lloyd_run_f64: points are not F64");
  const int d = c.d;
  if (d < 2 || d > 16 || k > 64 || k * d > kF64RunThreads)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "device F64 run: needs 2 <= d <= 16 and k <= 64");
  if (max_steps < 0) CDR_FAIL(CDR_ERR_ARG, "max_steps < 0");
  drop_running_state(c);
  upload_centroids(c, C, k);
  const size_t kd = (size_t)k * d;
  c.f64_sums.ensure(sizeof(double) * kd);
  c.f64_counts.ensure(sizeof(long long) * k * 2);
  c.f64r_state.ensure(sizeof(long long) * 4);
  c.f64r_keep.ensure(sizeof(double) * kd + sizeof(long long) * k);
  c.h_small.ensure(sizeof(long long) * 4);
  long long* hst = c.h_small.as<long long>();
  hst[0] = 1;
  hst[1] = hst[2] = hst[3] = 0;
  long long* st = c.f64r_state.as<long long>();
  HIP_CHECK(hipMemcpyAsync(st, hst, sizeof(long long) * 4, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemsetAsync(c.f64r_keep.p, 0, c.f64r_keep.bytes, c.stream));
  snprintf(c.prof_kernel, sizeof(c.prof_kernel), "f64_assign_block<%d>", d);
  // Steps are queued in chunks (4, 8, then 16 at a time) with the state word
  // read back between chunks: only f64_assign_block and f64_run_update test
  // it, so a run that stopped (converged, or handed to the host) would still
  // run the rest of every queued step's kernels.  One host sync
  // per chunk costs ~20 us against ~0.5 ms per step.
  int chunk = 4, queued = 0;
  // the transfer cache across the run's steps (f64_step_fused; the first step
  // forms every transfer).  CDR_F64_TCACHE=0 forms every transfer every step
  // (tests/test_gpu_f64_update.py compares the two).
  const char* tce = getenv("CDR_F64_TCACHE");
  const bool tc_on = !tce || std::atoi(tce) != 0;
  for (int s = 0; s < max_steps; ++s) {
    if (queued == chunk) {
      HIP_CHECK(hipMemcpyAsync(hst, st, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
      HIP_CHECK(hipStreamSynchronize(c.stream));
      if (hst[0] == 0) break;
      queued = 0;
      chunk = chunk < 16 ? 2 * chunk : 16;
    }
    ++queued;
    const bool prof = prof_step_begin(c);
    if (prof) prof_mark(c, 0);
    if (!f64_step_fused(c, k, c.cent64.as<double>(), c.f64_sums.as<double>(),
                        reinterpret_cast<unsigned long long*>(c.f64_counts.as<long long>()), prof,
                        st, tc_on ? (s == 0 ? 1 : 2) : 0))
      CDR_FAIL(CDR_ERR_UNSUPPORTED, "device F64 run: shape not covered");
    hipLaunchKernelGGL(f64_run_update, dim3(1), dim3(kF64RunThreads), 0, c.stream,
                       c.f64_sums.as<double>(),
                       reinterpret_cast<unsigned long long*>(c.f64_counts.as<long long>()),
                       c.cent64.as<double>(), c.f64r_keep.as<double>(), k, d, tol, st);
    HIP_CHECK(hipGetLastError());
    if (prof) prof_mark(c, 2);
  }
  HIP_CHECK(hipMemcpyAsync(hst, st, sizeof(long long) * 4, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipMemcpyAsync(C_out, c.cent64.p, sizeof(double) * kd, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipMemcpyAsync(means_out, c.f64r_keep.p, sizeof(double) * kd, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipMemcpyAsync(counts_out, c.f64r_keep.as<double>() + kd, sizeof(long long) * k,
                           hipMemcpyDeviceToHost, c.stream));
  read_walked(c, k);
  info[0] = (int32_t)hst[1];
  info[1] = max_steps == 0 ? 0 : (int32_t)hst[2];
  const bool had_labels = c.have_labels;
  step_done(c, k, c.n);
  if (max_steps == 0) c.have_labels = had_labels;  // no step ran: no new labels
}

static void lloyd_step_f64(Ctx& c, const double* C, int32_t k, double* sums, int64_t* counts) {
  check_k(c, k);
  if (c.mode != CDR_MODE_F64) CDR_FAIL(CDR_ERR_STATE, "lloyd_step_f64: points are not F64");
  drop_running_state(c);
  const int d = c.d;
  upload_centroids(c, C, k);
  const bool prof = prof_step_begin(c);
  c.f64_sums.ensure(sizeof(double) * (size_t)k * d);
  c.f64_counts.ensure(sizeof(long long) * k * 2);
  long long* cnt_pre = c.f64_counts.as<long long>() + k;
  // the fused pipeline (f64_assign.hip: assignment + block pass, then the
  // sums of f64sum.hip; CDR_F64_FUSE=0: separate passes)
  static const bool fuse_env = !exp_env("CDR_F64_FUSE") || atoi(exp_env("CDR_F64_FUSE"));
  if (fuse_env && !getenv("CDR_F64_SERIAL")) {
    snprintf(c.prof_kernel, sizeof(c.prof_kernel), "f64_assign_block<%d>", d);
    if (prof) prof_mark(c, 0);
    if (f64_step_fused(c, k, c.cent64.as<double>(), c.f64_sums.as<double>(),
                       reinterpret_cast<unsigned long long*>(c.f64_counts.as<long long>()),
                       prof)) {
      if (prof) prof_mark(c, 2);
      copy_back_sums(c, k, c.f64_counts.as<long long>(), sums, counts, true);
      step_done(c, k, c.n);
      return;
    }
  }
  snprintf(c.prof_kernel, sizeof(c.prof_kernel),
           d <= 16 ? "assign_exact_d<double, %d>" : "assign_exact_all<double>", d);
  if (prof) prof_mark(c, 0);
  enqueue_assign_exact(c, k);
  if (prof) prof_mark(c, 1);
  enqueue_count_labels(c, k, cnt_pre);
  if (!getenv("CDR_F64_SERIAL") && f64_sums_parallel(c, k, c.f64_sums.as<double>())) {
    // f64sum.hip: exact row-order sums in parallel; counts from count_labels
    HIP_CHECK(hipMemcpyAsync(c.f64_counts.p, cnt_pre, sizeof(long long) * k,
                             hipMemcpyDeviceToDevice, c.stream));
    if (prof) prof_mark(c, 2);
    read_walked(c, k);
  } else {
    const int threads = k * (d + 1);
    hipLaunchKernelGGL(seq_sums_f64, dim3((threads + 63) / 64), dim3(64), 0, c.stream,
                       c.x64.as<double>(), c.n, c.n_pad, d, k, c.labels.as<int32_t>(), cnt_pre,
                       c.f64_sums.as<double>(), c.f64_counts.as<long long>());
    HIP_CHECK(hipGetLastError());
    if (prof) prof_mark(c, 2);
    c.f64x_walked = -1;
  }
  copy_back_sums(c, k, c.f64_counts.as<long long>(), sums, counts, false);
  step_done(c, k, c.n);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_lloyd_step_f64(cdr_ctx* h, const double* C, int32_t k, double* sums,
                       int64_t* counts) {
  CDR_TRY
  if (!h || !C || !sums || !counts) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  lloyd_step_f64(h->c, C, k, sums, counts);
  CDR_CATCH
}

int cdr_lloyd_f64_run(cdr_ctx* h, const double* C, int32_t k, int32_t max_steps, double tol,
                      double* C_out, double* means_out, int64_t* counts_out, int32_t* info) {
  CDR_TRY
  if (!h || !C || !C_out || !means_out || !counts_out || !info) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  lloyd_run_f64(h->c, C, k, max_steps, tol, C_out, means_out, counts_out, info);
  CDR_CATCH
}

int cdr_lloyd_f64_walked(cdr_ctx* h, int64_t* walked) {
  CDR_TRY
  if (!h || !walked) CDR_FAIL(CDR_ERR_ARG, "null argument");
  *walked = h->c.f64x_walked;
  CDR_CATCH
}

// ---- sharded F64 sums (f64_sharded.hip, include/cdr.h cdr_f64s_*) ----
int cdr_f64s_begin(cdr_ctx* h, const double* C, int32_t k, int32_t nranks, int32_t rank,
                   void* tot_buf, int64_t* sizes) {
  CDR_TRY
  if (!h || !C || !tot_buf || !sizes) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  check_k(c, k);
  if (c.mode != CDR_MODE_F64) CDR_FAIL(CDR_ERR_STATE, "cdr_f64s_begin: points are not F64");
  if (nranks < 1 || rank < 0 || rank >= nranks) CDR_FAIL(CDR_ERR_ARG, "bad ranks");
  if (c.d < 2 || c.d > 16 || k > 64)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "sharded F64 sums need 2 <= d <= 16 and k <= 64");
  drop_running_state(c);
  upload_centroids(c, C, k);
  const int kd = k * c.d;
  double* slot = static_cast<double*>(tot_buf) + (size_t)rank * (kd + k);
  snprintf(c.prof_kernel, sizeof(c.prof_kernel), "f64_assign_block<%d>", c.d);
  const bool prof = prof_step_begin(c);
  if (prof) prof_mark(c, 0);
  if (!f64s_assign_totals(c, k, c.cent64.as<double>(), slot))
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "sharded F64 sums: shape not covered");
  if (prof) prof_mark(c, 1);
  c.f64s_k = k;
  c.f64s_nranks = nranks;
  c.f64s_rank = rank;
  sizes[0] = (int64_t)sizeof(double) * (kd + k);
  sizes[1] = (int64_t)24 * kd * (f64s_cap() + 1);
  step_done(c, k, c.last_fallback);  // (this entry leaves the fallback count as it was)
  CDR_CATCH
}

int cdr_f64s_build(cdr_ctx* h, const void* tot_buf, void* prog_buf) {
  CDR_TRY
  if (!h || !tot_buf || !prog_buf) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  if (c.f64s_k < 1) CDR_FAIL(CDR_ERR_STATE, "cdr_f64s_begin first");
  f64s_build(c, c.f64s_k, c.f64s_nranks, c.f64s_rank, static_cast<const double*>(tot_buf),
             prog_buf);
  CDR_CATCH
}

int cdr_f64s_finish(cdr_ctx* h, const void* tot_buf, const void* prog_buf, double* sums,
                    int64_t* counts, int32_t* status) {
  CDR_TRY
  if (!h || !tot_buf || !prog_buf || !sums || !counts || !status)
    CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  const int k = c.f64s_k, kd = k * c.d;
  if (k < 1) CDR_FAIL(CDR_ERR_STATE, "cdr_f64s_begin first");
  c.f64_sums.ensure(sizeof(double) * 2 * kd);
  c.f64_counts.ensure(sizeof(long long) * k * 2 + sizeof(int));
  int* dst = reinterpret_cast<int*>(c.f64_counts.as<long long>() + 2 * k);
  f64s_compose_all(c, k, c.f64s_nranks, static_cast<const double*>(tot_buf), prog_buf,
                   c.f64_sums.as<double>(), c.f64_counts.as<long long>(), dst);
  if (c.prof_cur >= 0) prof_mark(c, 2);  // (the step's kernels end here)
  HIP_CHECK(hipMemcpyAsync(status, dst, sizeof(int), hipMemcpyDeviceToHost, c.stream));
  copy_back_sums(c, k, c.f64_counts.as<long long>(), sums, counts, false);
  const bool force = getenv("CDR_F64S_FORCE_CHAIN") && atoi(getenv("CDR_F64S_FORCE_CHAIN"));
  if (force) *status |= 1;  // (tests: the exact rank chain on every rank)
  CDR_CATCH
}

int cdr_f64s_chain(cdr_ctx* h, void* chain_buf) {
  CDR_TRY
  if (!h || !chain_buf) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  if (c.f64s_k < 1) CDR_FAIL(CDR_ERR_STATE, "cdr_f64s_begin first");
  f64s_chain_walk(c, c.f64s_k, static_cast<double*>(chain_buf));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  CDR_CATCH
}

}  // extern "C"
