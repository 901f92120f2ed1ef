// lloyd.hip — one Lloyd iteration on F32X points (grid data, fp32 storage;
// reference src/kmeans_plusplus.py:31-43).
//
//   labels = argmin_j sqrt(pw_d((x - c_j)^2))          (:33-34, first index on ties)
//   new_c[j] = mean(X[labels == j])                     (:37-41; host divides)
//
// lloyd_step_f32x offers the step to the screens in turn — screen32
// (screen32.hip: d <= 16, k <= 64), the medium screens (screen_mid.hip), the
// large-k levels (screen_big.hip) — and assigns every point exactly
// (lloyd_exact.hip) when none takes the shape.  Every path gives the labels
// of the fp64 reference and the exact int64 fixed-point sums.
// The F64 and float32-reference steps: lloyd_f64.hip, lloyd_f32r.hip.
#include <cstdio>
#include <cmath>
#include <cstring>

#include "cdr_internal.h"

namespace cdr {

int lloyd_num_cus(int device) {
  static int cached[64] = {0};
  if (device >= 0 && device < 64 && cached[device]) return cached[device];
  int v = 0;
  HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
  if (device >= 0 && device < 64) cached[device] = v;
  return v;
}

void upload_centroids(Ctx& c, const double* C, int k) {
  c.cent64.ensure(sizeof(double) * (size_t)k * c.d);
  HIP_CHECK(hipMemcpyAsync(c.cent64.p, C, sizeof(double) * (size_t)k * c.d,
                           hipMemcpyHostToDevice, c.stream));
}

void check_k(const Ctx& c, int k) {
  if (c.mode == 0) CDR_FAIL(CDR_ERR_STATE, "no points loaded");
  if (k < 1) CDR_FAIL(CDR_ERR_ARG, "k must be >= 1");
  if (c.d > 128) CDR_FAIL(CDR_ERR_UNSUPPORTED, "d > 128 is not supported yet");
}

// Exact assignment for every point, then fixed-point sums from labels.
static void exact_step(Ctx& c, int k, long long* dout) {
  drop_running_state(c);
  // Checked before the assignment, so an unsupported shape launches no kernel
  if ((size_t)k * (c.d + 1) * 8 > 160 * 1024)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "k*(d+1) too large for the update table");
  enqueue_assign_exact(c, k);
  snprintf(c.prof_kernel, sizeof(c.prof_kernel), "assign_exact_all<%d>", c.d);
  enqueue_update_from_labels(c, k, dout);
}

void lloyd_step_f32x(Ctx& c, const double* C, int32_t k, int64_t* out, bool out_dev) {
  check_k(c, k);
  if (c.mode != CDR_MODE_F32X) CDR_FAIL(CDR_ERR_STATE, "lloyd_step: points are not F32X");
  const int len = k * (c.d + 1);
  long long* dout;
  if (out_dev) {
    dout = reinterpret_cast<long long*>(out);
  } else {
    c.out_sums.ensure(sizeof(long long) * len);
    dout = c.out_sums.as<long long>();
  }
  const bool prof = prof_step_begin(c);
  // host path: the sums and the fallback total arrive in pinned memory
  // (h_small), which screen32 publishes into itself (mapped)
  if (!out_dev) c.h_small.ensure(sizeof(long long) * (len + 1) + 64);
  long long* hs = c.h_small.as<long long>();
  // CDR_EXACT_ASSIGN=1 (read per step; tests): the exact fp64 NumPy-order
  // assignment of every point (assign_exact_all), no screen
  const bool exact_only = std::getenv("CDR_EXACT_ASSIGN") && std::atoi(std::getenv("CDR_EXACT_ASSIGN"));
  // screen32 uploads its own operands (one pinned copy) and leaves the totals
  // in c.run_sums; it copies them to a device `out` itself
  const bool s32 = !exact_only && screen32_supported(c, k) &&
                   screen32_step(c, C, k, out_dev ? dout : nullptr, out_dev ? nullptr : hs, prof,
                                 c.dbg_vals, c.dbg_vals ? c.dbg_thr : nullptr, nullptr);
  if (!s32) {
    upload_centroids(c, C, k);
    HIP_CHECK(hipMemsetAsync(dout, 0, sizeof(long long) * len, c.stream));
    c.fb_list.ensure(sizeof(int32_t) * (c.n > 0 ? c.n : 1));
  }
  const bool screened =
      s32 || (!exact_only && (mid_step(c, C, k, dout, prof) || big_step(c, C, k, dout, prof)));
  if (!screened) exact_step(c, k, dout);
  c.last_screened = screened;
  if (prof) {
    if (!screened) {  // no screen kernel: an empty triple keeps the pairing
      prof_mark(c, 0);
      prof_mark(c, 1);
    }
    // screen32's publish32 sums its fallback total itself
    if (screened && !s32) prof_end_screened(c);
    else prof_mark(c, 2);
  }
  int64_t fallback = -1;  // device `out`: unknown until cdr_lloyd_stats synchronises
  if (!out_dev) {
    int32_t* hfb = reinterpret_cast<int32_t*>(hs + len);
    if (!s32) {
      HIP_CHECK(hipMemcpyAsync(hs, dout, sizeof(long long) * len, hipMemcpyDeviceToHost, c.stream));
      *hfb = 0;
      if (screened)
        HIP_CHECK(hipMemcpyAsync(hfb, c.fb_count.as<int32_t>() + c.fb_total_slot,
                                 sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    }
    HIP_CHECK(hipStreamSynchronize(c.stream));
    fallback = screened ? *hfb : c.n;
    memcpy(out, hs, sizeof(long long) * len);
  }
  step_done(c, k, fallback);
}

__global__ void labels_to_i64(const int32_t* __restrict__ a, int64_t n, long long* __restrict__ b) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    b[i] = a[i];
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_lloyd_step(cdr_ctx* h, const double* C, int32_t k, int64_t* out,
                   int32_t out_on_device) {
  CDR_TRY
  if (!h || !C || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  lloyd_step_f32x(h->c, C, k, out, out_on_device != 0);
  CDR_CATCH
}

int cdr_lloyd_labels(cdr_ctx* h, int64_t* labels) {
  CDR_TRY
  if (!h || (!labels && h->c.n > 0)) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  if (!c.have_labels) CDR_FAIL(CDR_ERR_STATE, "no Lloyd step has run");
  if (c.n == 0) return CDR_OK;
  HIP_CHECK(hipSetDevice(c.device));
  DevBuf tmp;
  tmp.ensure(sizeof(long long) * c.n);
  hipLaunchKernelGGL(labels_to_i64, dim3((int)std::min<int64_t>(ceil_div(c.n, 256), 4096)),
                     dim3(256), 0, c.stream, c.labels.as<int32_t>(), c.n, tmp.as<long long>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(labels, tmp.p, sizeof(long long) * c.n, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  CDR_CATCH
}

int cdr_lloyd_stats(cdr_ctx* h, int64_t* n_fallback) {
  CDR_TRY
  if (!h || !n_fallback) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  if (c.last_fallback < 0) {
    HIP_CHECK(hipSetDevice(c.device));
    int32_t fb = 0;
    if (c.last_screened)
      HIP_CHECK(hipMemcpyAsync(&fb, c.fb_count.as<int32_t>() + c.fb_total_slot, sizeof(int32_t),
                               hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    c.last_fallback = c.last_screened ? fb : c.n;
  }
  *n_fallback = c.last_fallback;
  CDR_CATCH
}

#ifdef CDR_EXPERIMENTS
// Timing experiments only (not in the product build or include/cdr.h): skip
// parts of the screen kernel; results are garbage while mask != 0.
int cdr_debug_screen_ablate(cdr_ctx* h, int32_t mask) {
  CDR_TRY
  if (!h) CDR_FAIL(CDR_ERR_ARG, "null ctx");
  h->c.screen_ablate = mask;
  CDR_CATCH
}
#endif

int cdr_lloyd_screen_layout(cdr_ctx* h, int32_t out[6]) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 6; ++i) out[i] = h->c.s32_layout[i];
  CDR_CATCH
}

// Test hook: the screen32 plan's prune block of centroids C (screen32.hip).
int cdr_debug_plan32(cdr_ctx* h, int32_t which, const double* C, int32_t k, float* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  debug_plan32(h->c, which, C, k, out);
  CDR_CATCH
}

int cdr_lloyd_big_layout(cdr_ctx* h, int64_t out[15]) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  big_layout_read(h->c, out);
  CDR_CATCH
}

// Test hook: the large-k plan buffer of the last large-k step (screen_big_plan.hip).
int cdr_debug_big_plan(cdr_ctx* h, int32_t k, void* out, int64_t bytes, int64_t* written) {
  CDR_TRY
  if (!h || !written) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  *written = debug_big_plan(h->c, k, out, bytes);
  CDR_CATCH
}

// Test hook: screen values of every point (n_pad x ceil(k/16)*16 floats, host
// buffer) from one F32X step with centroids C.  Not part of the product path.
int cdr_debug_screen(cdr_ctx* h, const double* C, int32_t k, float* out_vals,
                     float* thr_a0a1) {
  CDR_TRY
  if (!h || !C || !out_vals) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  if (!screen_supported(c, k)) CDR_FAIL(CDR_ERR_UNSUPPORTED, "screen not used for this shape");
  const int KT = (k + 15) / 16;
  DevBuf dbg;
  dbg.ensure(sizeof(float) * (size_t)c.n_pad * KT * 16);
  HIP_CHECK(hipMemsetAsync(dbg.p, 0, sizeof(float) * (size_t)c.n_pad * KT * 16, c.stream));
  std::vector<long long> tmp((size_t)k * (c.d + 1));
  c.dbg_vals = dbg.as<float>();
  try {
    lloyd_step_f32x(c, C, k, reinterpret_cast<int64_t*>(tmp.data()), false);
  } catch (...) {
    c.dbg_vals = nullptr;
    throw;
  }
  c.dbg_vals = nullptr;
  HIP_CHECK(hipMemcpy(out_vals, dbg.p, sizeof(float) * (size_t)c.n_pad * KT * 16,
                      hipMemcpyDeviceToHost));
  if (thr_a0a1) {
    if (screen32_supported(c, k)) {
      thr_a0a1[0] = c.dbg_thr[0];
      thr_a0a1[1] = c.dbg_thr[1];
    } else {
      mid_thresholds(c, C, k, thr_a0a1);
    }
  }
  CDR_CATCH
}

}  // extern "C"
