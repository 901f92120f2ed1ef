// profile.hip — the step profiler (cdr_profile_*): per profiled step HIP
// events on the context stream, taken from a pool and only resolved by
// cdr_profile_read, so that profiling never makes the host wait inside an
// enqueued loop (cdr_internal.h: the prof_ fields of Ctx).
#include <cstdio>

#include "cdr_internal.h"

namespace cdr {

// Adds a screen's published fallback total to the profiling accumulator.
__global__ void fb_accumulate(const int32_t* __restrict__ total, long long* __restrict__ acc) {
  if (threadIdx.x == 0) acc[0] += total[0];
}

bool prof_step_begin(Ctx& c) {
  c.prof_cur = -1;
  if (!c.prof_on) return false;
  if (c.prof_seen++ % c.prof_period != 0) return false;
  if (c.prof_used + 4 > (size_t)(4 << 16)) return false;  // session cap: 65536 steps
  while (c.prof_pool.size() < c.prof_used + 4) {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreate(&e));
    c.prof_pool.push_back(e);
  }
  c.prof_cur = (int64_t)c.prof_used;
  c.prof_used += 4;
  c.prof_sub.resize(c.prof_used / 4);
  c.prof_sub[c.prof_used / 4 - 1] = 0;
  return true;
}

void prof_mark(Ctx& c, int i) {
  if (c.prof_cur >= 0) HIP_CHECK(hipEventRecord(c.prof_pool[(size_t)c.prof_cur + i], c.stream));
}

void prof_mark_sub(Ctx& c) {
  if (c.prof_cur < 0) return;
  HIP_CHECK(hipEventRecord(c.prof_pool[(size_t)c.prof_cur + 3], c.stream));
  c.prof_sub[(size_t)c.prof_cur / 4] = 1;
}

void prof_end_screened(Ctx& c) {
  if (c.prof_cur < 0) return;
  c.fb_accum.ensure(2 * sizeof(long long));
  hipLaunchKernelGGL(fb_accumulate, dim3(1), dim3(64), 0, c.stream,
                     c.fb_count.as<int32_t>() + c.fb_total_slot, c.fb_accum.as<long long>());
  HIP_CHECK(hipGetLastError());
  prof_mark(c, 2);
}

void prof_drop(Ctx& c) {
  if (c.prof_cur >= 0) {
    c.prof_used -= 4;
    c.prof_cur = -1;
  }
}

// Fold every recorded step's events into the profile accumulators (waits
// for the last one).
static void prof_collect(Ctx& c) {
  if (c.prof_used == 0) return;
  HIP_CHECK(hipEventSynchronize(c.prof_pool[c.prof_used - 2]));  // (the last step's end)
  for (size_t t = 0; t + 4 <= c.prof_used; t += 4) {
    float a = 0.f, b = 0.f;
    HIP_CHECK(hipEventElapsedTime(&a, c.prof_pool[t], c.prof_pool[t + 1]));
    HIP_CHECK(hipEventElapsedTime(&b, c.prof_pool[t], c.prof_pool[t + 2]));
    c.prof_screen_ms += a;
    c.prof_step_ms += b;
    c.prof_launches += 1;
    if (c.prof_sub[t / 4]) {
      float s = 0.f;
      HIP_CHECK(hipEventElapsedTime(&s, c.prof_pool[t], c.prof_pool[t + 3]));
      c.prof_sub_ms += s;
      c.prof_sub_launches += 1;
    }
  }
  c.prof_used = 0;
  c.prof_cur = -1;
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_profile_reset(cdr_ctx* h, int32_t enable) {
  CDR_TRY
  if (!h) CDR_FAIL(CDR_ERR_ARG, "null ctx");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.prof_used = 0;
  c.prof_cur = -1;
  c.prof_on = enable != 0;
  c.prof_period = enable > 1 ? enable : 1;
  c.prof_seen = 0;
  c.prof_screen_ms = c.prof_step_ms = c.prof_fb_points = 0.0;
  c.prof_launches = 0;
  c.prof_sub_ms = 0.0;
  c.prof_sub_launches = 0;
  c.fb_accum.ensure(2 * sizeof(long long));
  HIP_CHECK(hipMemsetAsync(c.fb_accum.p, 0, 2 * sizeof(long long), c.stream));
  if (c.q_acc.p) HIP_CHECK(hipMemsetAsync(c.q_acc.p, 0, c.q_acc.bytes, c.stream));
  if (c.t_acc.p) HIP_CHECK(hipMemsetAsync(c.t_acc.p, 0, c.t_acc.bytes, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  CDR_CATCH
}

int cdr_profile_read(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  prof_collect(c);
  long long fb[2] = {0, 0};
  std::vector<long long> q(c.q_acc.bytes / sizeof(long long));
  std::vector<long long> tq(c.t_acc.bytes / sizeof(long long));
  if (c.fb_accum.p)
    HIP_CHECK(hipMemcpyAsync(fb, c.fb_accum.p, std::min(c.fb_accum.bytes, sizeof(fb)),
                             hipMemcpyDeviceToHost, c.stream));
  if (!q.empty())
    HIP_CHECK(hipMemcpyAsync(q.data(), c.q_acc.p, c.q_acc.bytes, hipMemcpyDeviceToHost, c.stream));
  if (!tq.empty())
    HIP_CHECK(hipMemcpyAsync(tq.data(), c.t_acc.p, c.t_acc.bytes, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  for (long long v : q) fb[1] += v;
  long long tight = 0;
  for (long long v : tq) tight += v;
  out[0] = c.prof_screen_ms;
  out[1] = (double)c.prof_launches;
  out[2] = c.prof_step_ms;
  out[3] = c.prof_fb_points + (double)fb[0];
  out[4] = (double)fb[1];
  out[5] = (double)tight;
  CDR_CATCH
}

int cdr_profile_read_sub(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  Ctx& c = h->c;
  HIP_CHECK(hipSetDevice(c.device));
  prof_collect(c);
  out[0] = c.prof_sub_ms;
  out[1] = (double)c.prof_sub_launches;
  CDR_CATCH
}

int cdr_profile_kernel(cdr_ctx* h, char* buf, int32_t len) {
  CDR_TRY
  if (!h || !buf || len < 1) CDR_FAIL(CDR_ERR_ARG, "null argument");
  snprintf(buf, (size_t)len, "%s", h->c.prof_kernel);
  CDR_CATCH
}

}  // extern "C"
