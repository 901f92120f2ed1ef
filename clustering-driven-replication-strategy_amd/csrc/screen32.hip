// screen32.hip — the host side of the small-shape Lloyd step (F32X points,
// d <= 16, k <= 64: BASELINE configs 2 and 3): the step's plan (build_plan32
// on the host, plan32_kernel on the device), the layout copies of a point set
// and their ensure_* functions, the small kernels around a step (publish32,
// zero_gated, pull_host_kernel) and the two step drivers: screen32_step (the
// full screen, screen32_full.hip) and screen32_delta_step (screen32p.hip,
// screen32b.hip, screen32bs.hip).
#include "screen32_common.h"

namespace cdr {

// One block after the screen (the kernel boundary orders it after every
// workgroup's atomics): the sum of the kRunSlices slices of the running sums
// -> dout (device, e.g. for the all-reduce) and/or hout (mapped pinned host
// memory, with the fallback total at hout[cells]); the screen's fallback
// counter fbc[nwaves] moves to fbc[nwaves + 1] and is cleared for the next
// step.
__global__ __launch_bounds__(256) void publish32(const long long* __restrict__ out, int cells,
                                                 long long* __restrict__ dout,
                                                 long long* __restrict__ hout,
                                                 int* __restrict__ fbc, int nwaves,
                                                 long long* __restrict__ fb_acc,
                                                 const long long* __restrict__ gate) {
  // (one cell per thread over as many workgroups as needed: a single
  // workgroup looping over the cells paid one memory round trip per pass)
  if (gate && gate[0] == 0) {  // a stopped loop contributes nothing to the all-reduce
    if (dout)
      for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x)
        dout[i] = 0;
    return;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += gridDim.x * blockDim.x) {
    long long v = 0;
#pragma unroll
    for (int sl = 0; sl < kRunSlices; ++sl) v += out[(size_t)sl * cells + i];
    if (dout) dout[i] = v;
    if (hout) hout[i] = v;
  }
  if (fbc && blockIdx.x == 0) {  // (uniform)
    const int fb = block_sum_counts(fbc, nwaves);
    if (threadIdx.x == 0) {
      fbc[nwaves] = 0;
      fbc[nwaves + 1] = fb;
      if (hout) hout[cells] = fb;
      if (fb_acc) fb_acc[0] += fb;
    }
  }
}

// Zeroes n int64 (the running sums before a full, non-DELTA step) unless
// the device loop has stopped.
__global__ void zero_gated(long long* __restrict__ p, int n, const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0;
}

// xt = (x - mu) 2^sigma = fma(x, 2^sigma, -mu 2^sigma), exact (Ctx::pre_ok).
// Padding rows and feature slots >= d stay 0.
__global__ void precenter_kernel(const float* __restrict__ x, int64_t n, int64_t n_pad, int d,
                                 const float* __restrict__ ms, float sig, float* __restrict__ xt) {
  const int d4 = d4_of(d);
  const int64_t total = (int64_t)d4 * n_pad;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = t / (4 * n_pad);  // SoA [d4/4][n_pad][4]
    const int64_t r = t - q * 4 * n_pad;
    const int64_t i = r >> 2;
    const int f = (int)(4 * q + (r & 3));
    xt[t] = (f < d && i < n) ? fmaf(x[t], sig, ms[f]) : 0.0f;
  }
}

// The hi-only screen copy xs16 of the DELTA screens (screen32p streams it,
// screen32b gathers its row-major form): tiles of 32 points [h = 0, 1]
// [p = 0..31][hi(QH quads)] as fp16, hi = fp16(xhat) with xhat =
// fma(x, 2^sigma, -mu 2^sigma), where lane half h owns quads QH h .. QH h +
// QH - 1 (screen32's layout): 16 bytes per (point, half) with QH = 2, 8 with
// QH = 1.  Missing features and padding rows are 0.
template <int QH>
__global__ void split_copy_kernel(const float* __restrict__ x, int64_t n, int64_t n_pad, int d,
                                  const float* __restrict__ ms, float sig,
                                  uint4* __restrict__ xs) {
  const int64_t total = n_pad * 2;  // (point, half) pairs
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tile = t >> 6;
    const int h = (int)((t >> 5) & 1), p = (int)(t & 31);
    const int64_t i = tile * 32 + p;
    unsigned hw[2 * QH], lw[2 * QH];
#pragma unroll
    for (int u = 0; u < QH; ++u) {
      f4 xt;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int f = 4 * (QH * h + u) + c;
        xt[c] = (f < d && i < n) ? fmaf(x[xidx(x, f, i, n_pad)], sig, ms[f]) : 0.0f;
      }
      split4(xt, hw[2 * u], hw[2 * u + 1], lw[2 * u], lw[2 * u + 1]);
    }
    if constexpr (QH == 1) reinterpret_cast<uint2*>(xs)[t] = uint2{hw[0], hw[1]};
    else xs[t] = uint4{hw[0], hw[1], hw[2], hw[3]};
  }
}

// labels -> their one-byte copy (k <= 64), once per run of DELTA steps
__global__ void lab8_kernel(const int32_t* __restrict__ labels, uint8_t* __restrict__ lab8,
                            int64_t n_pad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n_pad; i += stride) {
    const int4 v = *reinterpret_cast<const int4*>(labels + i);  // n_pad: a multiple of 64
    const unsigned w = (unsigned)(v.x & 255) | (unsigned)(v.y & 255) << 8 |
                       (unsigned)(v.z & 255) << 16 | (unsigned)(v.w & 255) << 24;
    *reinterpret_cast<unsigned*>(lab8 + i) = w;
  }
}

// The hi-only screen copy row by row (XH: screen32b's gathers read one line
// per point), from the tiled copy: tile of 32 points [2 halves][32][kPB].
template <int kPB>
__global__ void aos_hi_kernel(const unsigned char* __restrict__ xs, int64_t n_pad,
                              unsigned char* __restrict__ xh) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_pad * 2;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pt = t >> 1;
    const int hh = (int)(t & 1);
    const unsigned char* s = xs + (pt >> 5) * (64 * kPB) + hh * (32 * kPB) + (pt & 31) * kPB;
    unsigned char* d = xh + pt * (2 * kPB) + hh * kPB;
    if constexpr (kPB == 16) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    else *reinterpret_cast<uint2*>(d) = *reinterpret_cast<const uint2*>(s);
  }
}

// ---------------------------------------------------------------------------
// the step's plan
// ---------------------------------------------------------------------------
struct Plan32 {
  int QH, MT;
  float thr0, thr_rel;
  float Dv = 0.0f;  // the offset D (device plan: in the plan buffer)
  std::vector<h8> frag;      // [MT][2][64]
  std::vector<float> cinit;  // [MT][16][64]
  std::vector<float> prune;  // the prune block (plan32.h: c32 | E | h)
};

// dst[i] = src[i] for 16-byte words; src is mapped pinned host memory.
__global__ __launch_bounds__(256) void pull_host_kernel(const uint4* __restrict__ src,
                                                        uint4* __restrict__ dst, int64_t n16) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

// Shapes and data this kernel covers: F32X points, d <= 16, k <= 64, and every
// per-workgroup fp64 sum exact: |x| 2^S < 2^30 (F32X) and a workgroup sees at
// most ceil(groups / nwg) * 64 points, so its sums stay below 2^53 grid units
// when that count is < 2^23.  nwg >= #CUs (screen32_step).
bool screen32_supported(const Ctx& c, int k) {
  if (c.mode != CDR_MODE_F32X || c.d > 16 || k > 64 || k < 1) return false;
  if (exp_env("CDR_NO_SCREEN32")) return false;
  const int64_t groups = c.n_pad / 64;
  const int64_t per_wg = ceil_div(groups, lloyd_num_cus(c.device)) * 64;
  return per_wg < (int64_t(1) << 23);
}

// Point side of the bound: |xhat_f| <= max(fmax - mu, mu - fmin) 2^sigma.
void plan32_point_side(const Ctx& c, double& xxmax, double& l1x) {
  const double sc = std::ldexp(1.0, c.sigma);
  xxmax = 0.0;
  l1x = 0.0;
  for (int f = 0; f < c.d; ++f) {
    // (also bounds |fp16(xhat_f)|: the hi-only screen treats h as the point)
    const double dev =
        std::fmax(c.fmax[f] - (double)c.mu[f], (double)c.mu[f] - c.fmin[f]) * sc *
            (1.0 + std::ldexp(1.0, -11)) + std::ldexp(1.0, -25);
    xxmax += dev * dev;
    l1x += dev;
  }
  xxmax *= 1.0 + 1e-6;
}

// Fragments, C operand and certification constants.
static bool build_plan32(const Ctx& c, const double* C, int k, Plan32& pl) {
  const int d = c.d;
  const int Q = d4_of(d) / 4;
  pl.QH = Q <= 2 ? 1 : 2;
  pl.MT = k <= 32 ? 1 : 2;
  const double sc = std::ldexp(1.0, c.sigma);
  std::vector<double> ch((size_t)k * d), cc(k, 0.0);
  double ccmax = 0.0, l1c = 0.0, cabs = 0.0;
  for (int j = 0; j < k; ++j) {
    double s = 0.0, l1 = 0.0;
    for (int f = 0; f < d; ++f) {
      const double v = (C[(size_t)j * d + f] - (double)c.mu[f]) * sc;
      ch[(size_t)j * d + f] = v;
      s += v * v;
      l1 += std::fabs(v);
      cabs = std::fmax(cabs, std::fabs(v));
    }
    cc[j] = s;
    ccmax = std::fmax(ccmax, s);
    l1c = std::fmax(l1c, l1);
  }
  if (!(cabs <= 1024.0)) return false;  // fp16 split range (and NaN) guard
  double xxmax, l1x, D;
  plan32_point_side(c, xxmax, l1x);
  plan32_bounds(ccmax, l1c, xxmax, l1x, pl.QH, D, pl.thr0);
  pl.Dv = (float)D;
  pl.thr_rel = 1.0f + std::ldexp(1.0f, -16);  // the 64-ulp key truncation (2^-18 rel.)
  const int MT = pl.MT;
  pl.frag.assign((size_t)MT * 2 * 64, h8{});
  pl.cinit.assign((size_t)MT * 16 * 64, 0.0f);
  for (int m = 0; m < MT; ++m)
    for (int lane = 0; lane < 64; ++lane) {
      float cin[16];
      plan32_lane(ch.data(), cc.data(), D, k, d, pl.QH, m, lane, pl.frag[(m * 2 + 0) * 64 + lane],
                  pl.frag[(m * 2 + 1) * 64 + lane], cin);
      for (int i = 0; i < 16; ++i) pl.cinit[(m * 16 + i) * 64 + lane] = cin[i];
    }
  // prune block (screen32p), the quantities plan32_build computes on the device
  pl.prune.assign(kPrBytes / sizeof(float), 0.0f);
  float* pc = pl.prune.data();
  float* pE = pc + 64 * kPrStr;
  float* ph = pE + 64;
  std::vector<double> ec(64, 0.0);
  double ecmax = 0.0;
  const double dn = plan32_prune_dn(xxmax);
  for (int j = 0; j < 64; ++j) {
    double e2 = 0.0, n2 = 0.0;
    for (int f = 0; f < d && j < k; ++f) {
      const double v = (C[(size_t)j * d + f] - (double)c.mu[f]) * sc;
      const float cf = (float)v;
      pc[j * kPrStr + f] = cf;
      const double r = (double)cf - v;
      e2 += r * r;
      n2 += v * v;
    }
    ec[j] = plan32_prune_ec(e2, n2);
    pE[j] = plan32_prune_E(dn, ec[j]);
    if (j < k) ecmax = std::fmax(ecmax, ec[j]);
  }
  for (int r = 0; r < 64; ++r) {
    double sm = INFINITY;
    plan_key t3[3] = {kPlanNoKey, kPlanNoKey, kPlanNoKey};
    for (int j = 0; j < k && r < k; ++j) {
      if (j == r) continue;
      double s2 = 0.0;
      for (int f = 0; f < 16; ++f) {
        const double df = (double)pc[r * kPrStr + f] - (double)pc[j * kPrStr + f];
        s2 += df * df;
      }
      sm = std::fmin(sm, s2);
      plan32_top3(t3, plan32_key(s2, j));
    }
    ph[r] = r < k ? plan32_prune_h(sm, ec[r], ecmax) : INFINITY;
    // the direct test's neighbours (screen32bs; rows past k: none)
    plan32_near(t3, r < k ? ec[r] : 0.0, ecmax, pc + r * kPrStr);
  }
  return true;
}

// Device plan of the loop's centroids (c.ll_C) at begin / resume; later
// steps are planned by ll_finalize right after it moves the centroids.
__global__ __launch_bounds__(256) void plan32_kernel(const double* __restrict__ C, int k, int d,
                                                     int QH, int MT,
                                                     const double* __restrict__ mu, double sc,
                                                     double xxmax, double l1x,
                                                     long long* __restrict__ state,
                                                     unsigned char* __restrict__ plan) {
  if (state[0] == 0) return;
  plan32_build(C, k, d, QH, MT, mu, sc, xxmax, l1x, state, plan);
}

// Device plan of the loop's current centroids (c.ll_C; mu as fp64 after the
// d reference values in c.ll_ref) into c.frag.
void plan32_launch(Ctx& c, int k, int QH, int MT) {
  hipLaunchKernelGGL(plan32_kernel, dim3(1), dim3(256), 0, c.stream, c.ll_C.as<double>(), k, c.d,
                     QH, MT, c.ll_ref.as<double>() + c.d, std::ldexp(1.0, c.sigma), c.ll_xxmax,
                     c.ll_l1x, c.ll_state.as<long long>(), static_cast<unsigned char*>(c.frag.p));
  HIP_CHECK(hipGetLastError());
}

// Test hook (cdr_debug_plan32): the prune block (plan32.h: kPrBytes) of
// centroids C from the host plan (which = 0) or plan32_kernel (1), or the one
// the device loop's last finalize left in the plan buffer (2; C unused).
void debug_plan32(Ctx& c, int which, const double* C, int k, float* out) {
  const int d = c.d;
  if (c.mode != CDR_MODE_F32X || d > 16 || k < 1 || k > 64)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "no screen32 plan for this shape");
  const int QH = d4_of(d) / 4 <= 2 ? 1 : 2, MT = k <= 32 ? 1 : 2;
  const Plan32Layout L = plan32_layout(MT, k, d);
  if (which == 0) {
    Plan32 pl;
    if (!C || !build_plan32(c, C, k, pl)) CDR_FAIL(CDR_ERR_ARG, "centroids out of the plan's range");
    std::memcpy(out, pl.prune.data(), kPrBytes);
  } else if (which == 1) {
    if (!C) CDR_FAIL(CDR_ERR_ARG, "null centroids");
    DevBuf dC, dmu, dst, dplan;
    std::vector<double> mu(d);
    for (int f = 0; f < d; ++f) mu[f] = (double)c.mu[f];
    const long long st[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    dC.ensure(sizeof(double) * (size_t)k * d);
    dmu.ensure(sizeof(double) * d);
    dst.ensure(sizeof(st));
    dplan.ensure(L.all);
    HIP_CHECK(hipMemcpyAsync(dC.p, C, sizeof(double) * (size_t)k * d, hipMemcpyHostToDevice, c.stream));
    HIP_CHECK(hipMemcpyAsync(dmu.p, mu.data(), sizeof(double) * d, hipMemcpyHostToDevice, c.stream));
    HIP_CHECK(hipMemcpyAsync(dst.p, st, sizeof(st), hipMemcpyHostToDevice, c.stream));
    double xxmax, l1x;
    plan32_point_side(c, xxmax, l1x);
    hipLaunchKernelGGL(plan32_kernel, dim3(1), dim3(256), 0, c.stream, dC.as<double>(), k, d, QH, MT,
                       dmu.as<double>(), std::ldexp(1.0, c.sigma), xxmax, l1x, dst.as<long long>(),
                       static_cast<unsigned char*>(dplan.p));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, static_cast<unsigned char*>(dplan.p) + L.prune, kPrBytes,
                             hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    for (DevBuf* b : {&dC, &dmu, &dst, &dplan}) b->release();
  } else {
    if (!c.ll_on || c.frag.bytes < L.all) CDR_FAIL(CDR_ERR_STATE, "no device loop plan");
    HIP_CHECK(hipMemcpyAsync(out, static_cast<unsigned char*>(c.frag.p) + L.prune, kPrBytes,
                             hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }
}

// Build the exact pre-centred copy xt = (x - mu) 2^sigma once per point set
// (Ctx::pre_ok) and the int64 mu 2^S that restores x sums from xt sums.
void ensure_precentered(Ctx& c) {
  if (!c.pre_ok || c.xt_valid) return;
  const int d = c.d;
  c.xt32.ensure(sizeof(float) * (size_t)d4_of(d) * c.n_pad);
  hipLaunchKernelGGL(precenter_kernel, dim3(4096), dim3(256), 0, c.stream, c.x32.as<float>(),
                     c.n, c.n_pad, d, c.mu_s.as<float>(), (float)std::ldexp(1.0, c.sigma),
                     c.xt32.as<float>());
  HIP_CHECK(hipGetLastError());
  std::vector<long long> muf(d);
  for (int f = 0; f < d; ++f) muf[f] = std::llrint(std::ldexp((double)c.mu[f], c.scale_bits));
  c.muf.ensure(sizeof(long long) * d);
  HIP_CHECK(hipMemcpyAsync(c.muf.p, muf.data(), sizeof(long long) * d, hipMemcpyHostToDevice,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));  // muf is a stack vector
  c.xt_valid = true;
}

// Row-major copy of the points (d4 floats per point): the gathers of the
// fused fixup and of screen32bs touch one line (and one page) per point
// instead of one per feature quad.
__global__ void aos_copy_kernel(const float4* __restrict__ x, int64_t n_pad, int Q,
                                float4* __restrict__ xa) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_pad * Q;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / Q;
    const int q = (int)(t - i * Q);
    xa[t] = x[(int64_t)q * n_pad + i];
  }
}

// The row-major copy, built once per point set (also the large-k path's
// gathers, screen_big.hip, and the seeding's, seed_update.hip).
void ensure_rowmajor(Ctx& c) {
  if (c.xa_valid) return;
  const int Q = d4_of(c.d) / 4;
  c.xa32.ensure(sizeof(float) * (size_t)c.n_pad * 4 * Q);
  hipLaunchKernelGGL(aos_copy_kernel, dim3(4096), dim3(256), 0, c.stream, c.x32.as<float4>(),
                     c.n_pad, Q, c.xa32.as<float4>());
  HIP_CHECK(hipGetLastError());
  c.xa_valid = true;
}

// The hi-only screen copy (32 bytes per point with QH = 2, 16 with QH = 1) and
// the row-major copy, built once per point set.
static void ensure_split(Ctx& c, int QH) {
  if (c.xs_valid) return;
  ensure_rowmajor(c);
  c.xs16.ensure((size_t)c.n_pad * (QH == 1 ? 16 : 32));
  const float sig = (float)std::ldexp(1.0, c.sigma);
  if (QH == 1)
    hipLaunchKernelGGL(split_copy_kernel<1>, dim3(4096), dim3(256), 0, c.stream, c.x32.as<float>(),
                       c.n, c.n_pad, c.d, c.mu_s.as<float>(), sig, c.xs16.as<uint4>());
  else
    hipLaunchKernelGGL(split_copy_kernel<2>, dim3(4096), dim3(256), 0, c.stream, c.x32.as<float>(),
                       c.n, c.n_pad, c.d, c.mu_s.as<float>(), sig, c.xs16.as<uint4>());
  HIP_CHECK(hipGetLastError());
  c.xs_valid = true;
}

// ---------------------------------------------------------------------------
// the step drivers
// ---------------------------------------------------------------------------

// Per-wave fallback counts | running total (screen32) | published total:
// zeroed once per layout (nwaves); publish32 clears the running total every
// step.
static void fb_count_layout(Ctx& c, int nwaves) {
  if (c.fb_count.bytes < sizeof(int32_t) * (nwaves + 3) || c.fb_layout != nwaves) {
    c.fb_count.ensure(sizeof(int32_t) * (nwaves + 3));
    HIP_CHECK(hipMemsetAsync(c.fb_count.p, 0, sizeof(int32_t) * (nwaves + 3), c.stream));
    c.fb_layout = nwaves;
  }
  c.fb_regions = nwaves;
  c.fb_total_slot = nwaves + 1;
}

// The step's sums (k, d + 1) out of the running sums' slices, after the
// screen.  A device-loop step with no all-reduce buffer publishes nothing:
// ll_finalize reads the slices and moves the fallback counter itself.
static void publish32_launch(Ctx& c, int k, int nwaves, long long* dout, long long* hout,
                             const long long* gate) {
  const int len = k * (c.d + 1);
  long long* hout_dev = nullptr;
  if (hout) {
    void* hp = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&hp, hout, 0));
    hout_dev = static_cast<long long*>(hp);
  }
  c.fb_accum.ensure(2 * sizeof(long long));
  if (dout || hout_dev || !gate) {
    hipLaunchKernelGGL(publish32, dim3((unsigned)std::max(1, (len + 255) / 256)), dim3(256), 0,
                       c.stream, c.run_sums.as<long long>(),
                       len, dout, hout_dev, gate ? nullptr : c.fb_count.as<int32_t>(), nwaves,
                       c.prof_on ? c.fb_accum.as<long long>() : nullptr, gate);
    HIP_CHECK(hipGetLastError());
  }
}

#ifdef CDR_EXPERIMENTS
// CDR_S32BS_TPROF: screen32bs's per-wave phase times (100 MHz counter) of the
// launch just enqueued, to stderr (and raw to CDR_S32BS_TPROF_FILE)
static void s32bs_tprof_report(Ctx& c, const unsigned long long* tprof_buf, int nwaves,
                               bool split_env) {
  std::vector<unsigned long long> h((size_t)nwaves * 8);
  HIP_CHECK(hipStreamSynchronize(c.stream));
  HIP_CHECK(hipMemcpy(h.data(), tprof_buf, h.size() * 8, hipMemcpyDeviceToHost));
  unsigned long long t0 = ~0ull, t4 = 0;
  double sum[6] = {}, mx[6] = {}, mv = 0, nb = 0, mvt = 0;
  for (int w = 0; w < nwaves; ++w) {
    const unsigned long long* r = &h[(size_t)w * 8];
    t0 = std::min(t0, r[0]);
    t4 = std::max(t4, r[4]);
  }
  for (int w = 0; w < nwaves; ++w) {
    const unsigned long long* r = &h[(size_t)w * 8];
    const double v[6] = {double(r[0] - t0), double(r[1] - r[0]), double(r[2] - r[1]),
                         double(r[3] - r[2]), double(r[4] - r[3]), double(t4 - r[4])};
    for (int q = 0; q < 6; ++q) {
      sum[q] += v[q];
      mx[q] = std::max(mx[q], v[q]);
    }
    mvt += double(r[5]);
    nb += double(r[6]);
    mv += double(r[7]);
  }
  if (const char* path = exp_env("CDR_S32BS_TPROF_FILE")) {  // raw, appended
    if (FILE* fo = std::fopen(path, "ab")) {
      std::fwrite(h.data(), 8, h.size(), fo);
      std::fclose(fo);
    }
  }
  std::fprintf(stderr,
               "TPROF waves %d span %.1f us | avg/max us: start %.1f/%.1f prologue %.1f/%.1f "
               "phases %.1f/%.1f tail %.1f/%.1f flush %.1f/%.1f idle-end %.1f/%.1f | "
               "| (split form: tail batches/wave, moves/wave, move us/wave; fused: batches/wave, "
               "row-wait us/wave, decide us/wave) %.2f %.1f %.2f\n",
               nwaves, (t4 - t0) / 100.0, sum[0] / nwaves / 100, mx[0] / 100,
               sum[1] / nwaves / 100, mx[1] / 100, sum[2] / nwaves / 100, mx[2] / 100,
               sum[3] / nwaves / 100, mx[3] / 100, sum[4] / nwaves / 100, mx[4] / 100,
               sum[5] / nwaves / 100, mx[5] / 100, nb / nwaves, split_env ? mv / nwaves : mv / nwaves / 100,
               mvt / nwaves / 100);
}
#endif

// The watch list's switches that do not depend on the grid:
// 2-byte words of the fused screen32bs (z16), not with every bound failing
// (dbg: CDR_BOUNDS_DBG), from kS32WatchMinPts padded points (tests:
// CDR_S32BS_WATCH_MIN); CDR_S32BS_WATCH=0: off.  Read on every call.
static bool s32_watch_wanted(const Ctx& c, bool z16, int dbg) {
  if (!z16 || (dbg & 1)) return false;
  if (const char* e = std::getenv("CDR_S32BS_WATCH"))
    if (std::atoi(e) == 0) return false;
  int64_t wmin = kS32WatchMinPts;
  if (const char* e = std::getenv("CDR_S32BS_WATCH_MIN")) {
    const long long v = std::atoll(e);
    if (v >= 1) wmin = v;
  }
  return c.n_pad >= wmin;
}

// A DELTA step (labels and running sums as the full screen's): the pruned
// screen, or in the device loop, where ll_finalize32 keeps the drift bounds of
// every centroid move, a bounded screen: screen32bs in its fused 2-byte form
// (the default) or behind screen32bz (CDR_S32BS_SPLIT=1), or screen32b
// (CDR_S32B_SPLIT=0).  All read the hi-only screen copy or the row-major
// copy, keep lab8 equal to the labels and apply the moves themselves (fused
// fixup, or screen32bs's own table).
static void screen32_delta_step(Ctx& c, int QH, int MT, int k, const h8* dfrag,
                                const float* dcinit, const double* dcent, float thr0,
                                float thr_rel, float Dv, const float* dthr, long long* dout,
                                long long* hout, bool prof, long long* gate) {
  ensure_split(c, QH);
  int cus = lloyd_num_cus(c.device);
  const int Q = d4_of(c.d) / 4;
  // bounded screen (CDR_BOUNDS=0 turns it off)
  const bool bnd_env = !std::getenv("CDR_BOUNDS") || std::atoi(std::getenv("CDR_BOUNDS"));
  const bool BND = bnd_env && gate && dthr && c.ll_on && c.bnd_ok && c.n_pad < (int64_t(1) << 31);
  // ... deciding in registers (screen32bs; CDR_S32B_SPLIT=0: screen32b with
  // its queue and fused fixup)
  const bool BS = BND && (!std::getenv("CDR_S32B_SPLIT") || std::atoi(std::getenv("CDR_S32B_SPLIT")));
  if (!BND) c.zb_valid = false;  // another path decides this step's labels
  // tests: screen32bs's grid sized as on a device of CDR_S32BS_CUS CUs (a
  // multiple of 8, at most the real count; anything else is ignored), so the
  // generation regions and the dynamic tail run at small n; read on every call
  if (BS) {
    const char* e = std::getenv("CDR_S32BS_CUS");
    const int v = e ? std::atoi(e) : 0;
    if (v >= 8 && v % 8 == 0 && v <= cus) cus = v;
  }
  int bpc;
  // (the list path launches screen32bsw; whether the waves' ranges fit the
  // list is known only with the grid, so that grid fits both kernels)
  // (the switches of the bounded launch below, read once here: the split form
  // CDR_S32BS_SPLIT=1 and 2-byte words otherwise; CDR_BOUNDS_DBG, a test
  // switch whose bit 0 makes every bound fail)
  const bool split_env =
      BS && std::getenv("CDR_S32BS_SPLIT") && std::atoi(std::getenv("CDR_S32BS_SPLIT"));
  const bool z16 = BS && !split_env;
  int bdbg = std::getenv("CDR_BOUNDS_DBG") ? std::atoi(std::getenv("CDR_BOUNDS_DBG")) : 0;
#ifndef CDR_EXPERIMENTS
  bdbg &= 1;  // (the other bits are timing experiments: experiments build only)
#endif
  const bool watch_wanted = s32_watch_wanted(c, z16, bdbg);
  if (BS) {
    bpc = screen32bs_blocks_per_cu(Q, MT, false);
    if (watch_wanted) bpc = std::min(bpc, screen32bs_blocks_per_cu(Q, MT, true));
    // (experiments: fewer workgroups per CU, CDR_S32BS_BPC=1..3)
    static const int bsb_env = exp_env("CDR_S32BS_BPC") ? std::atoi(exp_env("CDR_S32BS_BPC")) : 0;
    if (bsb_env >= 1 && bsb_env < bpc) bpc = bsb_env;
  } else if (BND) {
    bpc = screen32b_blocks_per_cu(Q, MT);
  } else {
    bpc = screen32p_blocks_per_cu(Q, MT);
    static const int bpc_env = exp_env("CDR_S32P_BPC") ? std::atoi(exp_env("CDR_S32P_BPC")) : 0;
    if (bpc_env >= 1 && bpc_env < bpc) bpc = bpc_env;
  }
  // (a wave's unit: a chunk of kBChunk points of the bounded screens, a
  // 64-point group of the pruned one)
  const int64_t units = BND ? c.n_pad / kBChunk : c.n_pad / 64;
  const int unit_pts = BND ? kBChunk : 64;
  int nwg = (int)std::min<int64_t>(ceil_div(units, 4), (int64_t)cus * bpc);
  if (nwg < 1) nwg = 1;
  const int nwaves = nwg * 4;
  const int cap = (int)(ceil_div(units, nwaves) * unit_pts);
  c.fb_list.ensure(sizeof(int2) * (size_t)nwaves * cap);
  if (!BS) c.mv_list.ensure(sizeof(int2) * (size_t)nwaves * cap);  // (screen32bs: no move list)
  c.mv_count.ensure(sizeof(int32_t) * (size_t)nwaves);
  fb_count_layout(c, nwaves);
  if (!c.lab8_valid) {  // first DELTA step since another path wrote the labels
    c.lab8.ensure((size_t)c.n_pad);
    hipLaunchKernelGGL(lab8_kernel, dim3(2048), dim3(256), 0, c.stream, c.labels.as<int32_t>(),
                       c.lab8.as<uint8_t>(), c.n_pad);
    HIP_CHECK(hipGetLastError());
    c.lab8_valid = true;
  }
  FixArgs f;
  f.XA = c.xa32.as<float>();
  f.n_pad = c.n_pad;
  f.cent = dcent;
  f.k = k;
  f.d = c.d;
  f.labels = c.labels.as<int32_t>();
  f.lab8 = c.lab8.as<uint8_t>();
  f.fb_list = c.fb_list.as<int2>();
  f.fb_count = c.fb_count.as<int32_t>();
  f.mv_list = c.mv_list.as<int2>();
  f.mv_count = c.mv_count.as<int32_t>();
  f.cap = cap;
  f.regions = nwaves;
  f.fr = 4;
  f.fx = std::ldexp(1.0, c.scale_bits);
  f.run_sums = c.run_sums.as<unsigned long long>();
  f.gate = gate;
  f.abl = 0;
  f.XS = c.xs16.as<unsigned char>();
  f.frag = dfrag;
  f.cinit = dcinit;
  f.thr0 = thr0;
  f.thr_rel = thr_rel;
  f.thr_dev = dthr;
  f.ho = 1;
  f.ms = c.mu_s.as<float>();
  f.sig = (float)std::ldexp(1.0, c.sigma);
  f.zb = nullptr;
#ifdef CDR_EXPERIMENTS
  if (const char* e = exp_env("CDR_FIX_ABL")) f.abl = std::atoi(e);
#endif
  S32PArgs p;
  p.XS = c.xs16.as<unsigned char>();
  p.n = c.n;
  p.n_pad = c.n_pad;
  p.k = k;
  p.d = c.d;
  p.prune = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(dfrag) +
                                           plan32_layout(MT, k, c.d).prune);
  p.gate = gate;
  p.labels = f.labels;
  p.lab8 = f.lab8;
  p.fb_list = c.fb_list.as<int2>();
  p.fb_count = c.fb_count.as<int32_t>();
  p.mv_list = c.mv_list.as<int2>();
  p.mv_count = c.mv_count.as<int32_t>();
  p.cap = cap;
  p.frag = dfrag;
  p.cinit = dcinit;
  p.thr0 = thr0;
  p.thr_rel = thr_rel;
  p.Dv = Dv;
  p.thr_dev = dthr;
  if (c.prof_on && c.q_acc.bytes < sizeof(long long) * nwaves) {  // (zeroed when grown)
    c.q_acc.ensure(sizeof(long long) * nwaves);
    HIP_CHECK(hipMemsetAsync(c.q_acc.p, 0, c.q_acc.bytes, c.stream));
  }
  p.q_acc = c.prof_on ? c.q_acc.as<long long>() : nullptr;
  p.abl = 0;
#ifdef CDR_EXPERIMENTS
  if (const char* e = exp_env("CDR_S32P_ABL")) p.abl = std::atoi(e);
#endif
  p.fx = f;
  p.fuse = 1;
  const dim3 grid(nwg);
  if (!BND) {
    snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen32p<%d,%d,3>+fixup", Q, MT);
    if (prof) prof_mark(c, 0);
    screen32p_launch(Q, MT, grid, c.stream, p);
  } else {
    // bound words: reset (every point "no bound", labels from lab8) at the
    // first bounded step of a run; the row-major hi copy (screen32b) once
    // per point set.  The fused screen32bs keeps 2-byte words (DESIGN.md
    // 4.3g); the split form (CDR_S32BS_SPLIT=1) and screen32b 4-byte ones
    const int zfmt = z16 ? 16 : 32;
    if (c.zb_fmt != zfmt) c.zb_valid = false;
    c.zb_fmt = zfmt;
    c.zb.ensure(sizeof(uint32_t) * (size_t)c.n_pad);
    // the watch list belongs to the words: whatever resets
    // them (the first bounded step, a host take-over, a resume, another word
    // format) leaves no list
    bool watch_reset = !c.zb_valid;
    if (!c.zb_valid) {
      bound_words_reset(z16, c.stream, c.lab8.as<uint8_t>(), c.zb.p, c.n, c.n_pad, gate);
      HIP_CHECK(hipGetLastError());
    }
    if (!BS && !c.xh_valid) {
      c.xh16.ensure((size_t)c.n_pad * (QH == 1 ? 16 : 32));
      if (QH == 1)
        hipLaunchKernelGGL(aos_hi_kernel<8>, dim3(4096), dim3(256), 0, c.stream,
                           c.xs16.as<unsigned char>(), c.n_pad, c.xh16.as<unsigned char>());
      else
        hipLaunchKernelGGL(aos_hi_kernel<16>, dim3(4096), dim3(256), 0, c.stream,
                           c.xs16.as<unsigned char>(), c.n_pad, c.xh16.as<unsigned char>());
      HIP_CHECK(hipGetLastError());
      c.xh_valid = true;
    }
    if (c.prof_on && c.t_acc.bytes < sizeof(long long) * nwaves) {  // (zeroed when grown)
      c.t_acc.ensure(sizeof(long long) * nwaves);
      HIP_CHECK(hipMemsetAsync(c.t_acc.p, 0, c.t_acc.bytes, c.stream));
    }
    S32BArgs b;
    b.p = p;
    b.p.fx.zb = c.zb.as<uint32_t>();
    b.XH = c.xh16.as<unsigned char>();
    b.zb = c.zb.as<uint32_t>();
    b.wup = reinterpret_cast<const float*>(c.bnd.as<long long>() + 64);
    b.wdn = b.wup + 64;
    b.nchunks = c.n_pad / (z16 ? kZ16Chunk : kBChunk);
    b.zh = z16 ? c.zb.as<uint16_t>() : nullptr;
    b.bt = reinterpret_cast<const unsigned char*>(c.bnd.p);
    b.t_acc = c.prof_on ? c.t_acc.as<long long>() : nullptr;
    b.dbg = bdbg;
    // screen32bs's direct test; CDR_S32BS_DIRECT=0 (tests, A/B):
    // the triangle test and the split screen decide, read on every call
    b.direct = !std::getenv("CDR_S32BS_DIRECT") || std::atoi(std::getenv("CDR_S32BS_DIRECT"));
    c.zb_valid = true;
    b.tprof = nullptr;
    b.slot_wg = 0;
    // chunk shares of screen32bs's 4 launch generations (workgroups per CU):
    // one region per generation (4-byte words, A/B at 100M: 180 -> 166 us
    // against one strided split; speed-proportional weights 100,82,68,61
    // 166 us); 2-byte words: 115,105,95,85 (0.161-0.163 ms per step against
    // 0.168-0.178 equal, profiles/r05_generation_weights.txt);
    // CDR_S32BS_W="w0,w1,w2,w3" sets them, CDR_S32BS_W=0 the split
    if (BS) {
      static int wenv[4] = {-1, 0, 0, 0};
      if (wenv[0] < 0) {
        const int wdef[4] = {115, 105, 95, 85};
        for (int q = 0; q < 4; ++q) wenv[q] = split_env ? 100 : wdef[q];
        if (const char* e = exp_env("CDR_S32BS_W")) {
          wenv[0] = 0;
          int v[4] = {0, 0, 0, 0};
          if (std::sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4 && v[0] > 0 &&
              v[1] > 0 && v[2] > 0 && v[3] > 0)
            for (int q = 0; q < 4; ++q) wenv[q] = v[q];
        }
      }
      if (wenv[0] > 0 && nwg == cus * bpc && bpc == 4) {
        b.slot_wg = cus;
        for (int q = 0; q < 4; ++q) b.wsl[q] = wenv[q];
      }
      // contiguous chunk ranges per wave (CDR_S32BS_CONTIG=1)
      if (exp_env("CDR_S32BS_CONTIG") && std::atoi(exp_env("CDR_S32BS_CONTIG")))
        b.slot_wg = -1;
    }
    // the dynamic tail (2-byte words in generation regions): CDR_S32BS_DYN
    // = the statically streamed percent (100: off)
    b.dyn = nullptr;
    b.dyn_par = 0;
    b.dyn_pct = 100;
    if (BS && z16 && !split_env && b.slot_wg > 0) {
      static int dyn_env = -1;
      if (dyn_env < 0) {
        dyn_env = kS32DynPct;
        if (const char* e = exp_env("CDR_S32BS_DYN")) dyn_env = std::atoi(e);
        dyn_env = std::min(std::max(dyn_env, 0), 100);
      }
      // (tests: CDR_S32BS_DYN_MIN = m >= 1 in place of kS32DynMinChunks;
      // read on every call)
      int dyn_min = kS32DynMinChunks;
      if (const char* e = std::getenv("CDR_S32BS_DYN_MIN")) {
        const int v = std::atoi(e);
        if (v >= 1) dyn_min = v;
      }
      if (dyn_env < 100 && bs_max_region(b, nwg) < (1 << 17) && b.slot_wg % 8 == 0 &&
          bs_max_chunks(b, nwg) >= dyn_min) {
        if (c.s32_dyn.bytes < sizeof(unsigned) * 2 * 32 * 32) {
          c.s32_dyn.ensure(sizeof(unsigned) * 2 * 32 * 32);
          HIP_CHECK(hipMemsetAsync(c.s32_dyn.p, 0, c.s32_dyn.bytes, c.stream));
        }
        b.dyn = c.s32_dyn.as<unsigned>();
        b.dyn_par = c.s32_dyn_par;
        b.dyn_pct = dyn_env;
        c.s32_dyn_par ^= 1;
      }
    }
    // the launch's work distribution (cdr_lloyd_screen_layout)
    c.s32_layout[0] = nwg;
    c.s32_layout[1] = b.slot_wg;
    c.s32_layout[2] = b.dyn_pct;
    c.s32_layout[3] = (int32_t)bs_max_chunks(b, nwg);
    c.s32_layout[4] = (int32_t)b.nchunks;
    c.s32_layout[5] = z16 ? 2 : 4;
#ifdef CDR_EXPERIMENTS
    static unsigned long long* tprof_buf = nullptr;
    const bool tprof_on = BS && exp_env("CDR_S32BS_TPROF");
    if (tprof_on) {
      if (!tprof_buf) HIP_CHECK(hipMalloc(&tprof_buf, sizeof(unsigned long long) * 8 * 65536));
      b.tprof = tprof_buf;
    }
#endif
    if (BS) {
      // the near-tie list holds at most the points of a wave's chunks
      // (the dynamic tail: twice the static share plus the two groups a
      // claiming wave may hold, so the waves' budgets cover the pool)
      int64_t need =
          (b.dyn ? 2 * bs_max_chunks(b, nwg) + 2 * kBPD + 1 : bs_max_chunks(b, nwg)) *
          (z16 ? kZ16Chunk : kBChunk);
      // The watch list: wave w of this grid keeps the points [w wrange,
      // (w + 1) wrange) in a region of wcap entries.  On for 2-byte words from
      // kS32WatchMinPts padded points (s32_watch_wanted) while the
      // range fits the entries' 16-bit offset.  The
      // capacity is half the range: a longer list (4 bytes an entry) streams
      // more bytes than the words (2 bytes a point), and the largest list of
      // the beta sweep at config 3 stayed far below it (tests:
      // CDR_S32BS_WATCH_CAP entries, up to the range; read on every call).
      b.watch = nullptr;
      b.wl = nullptr;
      b.wn = b.wf = nullptr;
      b.wcap = b.wrange = 0;
      const int64_t wrange = ceil_div(b.nchunks, (int64_t)nwaves) * kZ16Chunk;
      const bool watch = watch_wanted && wrange <= kS32WatchMaxRange;
      if (watch) {
        int64_t wcap = ceil_div(wrange / 2, (int64_t)256) * 256;
        if (const char* e = std::getenv("CDR_S32BS_WATCH_CAP")) {
          const long long v = std::atoll(e);
          if (v >= 1) wcap = ceil_div(std::min<int64_t>(v, wrange), (int64_t)256) * 256;
        }
        if (!c.watch_on || c.watch_waves != nwaves || c.watch_range != wrange || c.watch_cap != wcap)
          watch_reset = true;  // (a list of another geometry)
        c.watch_waves = nwaves;
        c.watch_range = (int32_t)wrange;
        c.watch_cap = (int32_t)wcap;
        c.wl.ensure(sizeof(uint32_t) * (size_t)nwaves * (size_t)wcap);
        c.wn.ensure(sizeof(int32_t) * (size_t)nwaves);
        c.wf.ensure(sizeof(int32_t) * (size_t)nwaves);
        b.watch = reinterpret_cast<int*>(static_cast<unsigned char*>(c.bnd.p) + kBndWatch);
        b.wl = c.wl.as<uint32_t>();
        b.wn = c.wn.as<int32_t>();
        b.wf = c.wf.as<int32_t>();
        b.wcap = (int)wcap;
        b.wrange = (int)wrange;
        need = std::max(need, wrange);  // (the WATCH form's tail records: at most its entries)
      } else if (c.watch_on) {
        watch_reset = true;  // (this screen writes words the list does not see)
      }
      const bool was_on = c.watch_on;
      c.watch_on = watch;
      if (watch_reset && (watch || was_on))  // mode FULL, no list (kWMode .. kWHold)
        HIP_CHECK(hipMemsetAsync(static_cast<unsigned char*>(c.bnd.p) + kBndWatch, 0,
                                 5 * sizeof(int), c.stream));
      if (need > b.p.cap) {
        c.fb_list.ensure(sizeof(int2) * (size_t)nwaves * (size_t)need);
        b.p.fb_list = c.fb_list.as<int2>();
        b.p.cap = (int)need;
      }
      // split form (CDR_S32BS_SPLIT=1; default: the fused kernel): screen32bz
      // streams the words and lists the failed points, screen32bs<.., true>
      // decides the lists.  Measured at config 3 (profiles/r05_split_ab.txt):
      // the stream alone takes ~80 us and the decisions ~100-130 us as their
      // own launch, so the fused kernel (~165-180 us) stays the default
      b.zl = nullptr;
      b.zn = nullptr;
      b.zcap = 0;
      if (split_env) {
        b.zcap = ceil_div(bs_max_chunks(b, nwg) * kBChunk, 64) * 64;
        c.zl.ensure(sizeof(uint32_t) * (size_t)nwaves * (size_t)b.zcap);
        c.zn.ensure(sizeof(int32_t) * (size_t)nwaves);
        b.zl = c.zl.as<uint32_t>();
        b.zn = c.zn.as<int32_t>();
      }
      snprintf(c.prof_kernel, sizeof(c.prof_kernel),
               split_env ? "screen32bs<%d,%d>split" : "screen32bs16<%d,%d>", Q, MT);
      if (prof) prof_mark(c, 0);
      if (split_env) {
        screen32bz_launch(grid, c.stream, b);
        if (prof) prof_mark_sub(c);
      }
      // (the list path, b.watch: one launch, the mode word picks the form;
      // <4,1>: a launch per form, each gated on the mode word)
      screen32bs_launch(Q, MT, grid, c.stream, b, split_env);
#ifdef CDR_EXPERIMENTS
      if (tprof_on) s32bs_tprof_report(c, tprof_buf, nwaves, split_env);
#endif
    } else {
      snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen32b<%d,%d>+fixup", Q, MT);
      if (prof) prof_mark(c, 0);
      screen32b_launch(Q, MT, grid, c.stream, b);
    }
  }
  HIP_CHECK(hipGetLastError());
  if (prof) prof_mark(c, 1);
  publish32_launch(c, k, nwaves, dout, hout, gate);
}

// One F32X Lloyd step through screen32.  C != null: host plan (built here,
// uploaded with the step); returns false (nothing launched) when the
// centroids are out of the fp16 split range.  C == null: device-resident loop
// (loop.hip) — plan32_kernel builds the plan from c.ll_C on the device and
// every kernel of the step runs only while gate[0] != 0.  A step whose labels
// and running sums follow from the previous one (delta) goes to
// screen32_delta_step; the rest of this function is the full screen.
bool screen32_step(Ctx& c, const double* C, int k, long long* dout, long long* hout, bool prof,
                   float* dbg, float* thr_out, long long* gate) {
  const bool devplan = C == nullptr;
  Plan32 pl;
  if (devplan) {
    const int Q4 = d4_of(c.d) / 4;
    pl.QH = Q4 <= 2 ? 1 : 2;
    pl.MT = k <= 32 ? 1 : 2;
    pl.thr0 = 0.0f;
    pl.thr_rel = 1.0f + std::ldexp(1.0f, -16);
  } else if (!build_plan32(c, C, k, pl)) {
    return false;
  }
  // incremental update when the device labels and running sums belong to the
  // previous step of this point set and k
  const bool delta = c.run_valid && c.run_k == k && !dbg && !std::getenv("CDR_NO_DELTA");
  const int len = k * (c.d + 1);
  c.run_sums.ensure(sizeof(long long) * len * kRunSlices);
  if (!delta) {
    if (gate) {
      hipLaunchKernelGGL(zero_gated, dim3(4), dim3(256), 0, c.stream, c.run_sums.as<long long>(),
                         len * kRunSlices, gate);
      HIP_CHECK(hipGetLastError());
    } else {
      HIP_CHECK(hipMemsetAsync(c.run_sums.p, 0, sizeof(long long) * len * kRunSlices, c.stream));
    }
  }
  c.run_valid = false;
  c.big_valid = false;  // screen32 writes the labels the large-k running sums follow
  c.last_delta = delta;
  if (thr_out) {
    thr_out[0] = pl.thr0;
    thr_out[1] = 0.0f;
  }
  const int d = c.d, Q = d4_of(d) / 4;
  const int KP = 32 * pl.MT, NF = 8 * pl.QH;
  // plan buffer: fragments | C operand | centroids (fp64, for the fused
  // exact fallback) | thr0 (device plan only)
  const Plan32Layout PL = plan32_layout(pl.MT, k, c.d);
  const size_t b_frag = PL.cinit;
  const size_t b_cinit = PL.cent - PL.cinit;
  const size_t b_cent = PL.thr - PL.cent;
  const size_t b_all = PL.thr;
  c.frag.ensure(PL.all);
  if (!devplan) {  // (device plan: built by plan32_kernel / ll_finalize)
    // one pinned upload per step; the previous step's copy must have left the
    // staging buffer
    if (c.up_pending) HIP_CHECK(hipEventSynchronize(c.up_event));
    c.h_up.ensure(PL.all);
    memcpy(c.h_up.p, pl.frag.data(), b_frag);
    memcpy(static_cast<char*>(c.h_up.p) + b_frag, pl.cinit.data(), b_cinit);
    memcpy(static_cast<char*>(c.h_up.p) + b_frag + b_cinit, C, b_cent);
    memcpy(static_cast<char*>(c.h_up.p) + PL.prune, pl.prune.data(), kPrBytes);
    // the device pulls the staging buffer itself (pinned, mapped host memory)
    // with one small kernel on the stream: no DMA-engine copy in the step (a
    // runtime H2D copy here stalled the host for 7-16 ms once per run)
    void* hdev = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&hdev, c.h_up.p, 0));
    const int64_t n16 = (int64_t)(PL.all / 16);
    hipLaunchKernelGGL(pull_host_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0,
                       c.stream, static_cast<const uint4*>(hdev), static_cast<uint4*>(c.frag.p),
                       n16);
    HIP_CHECK(hipGetLastError());
    if (!c.up_event) HIP_CHECK(hipEventCreateWithFlags(&c.up_event, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(c.up_event, c.stream));
    c.up_pending = true;
  }
  h8* dfrag = c.frag.as<h8>();
  float* dcinit = reinterpret_cast<float*>(static_cast<char*>(c.frag.p) + b_frag);
  const double* dcent =
      reinterpret_cast<const double*>(static_cast<char*>(c.frag.p) + b_frag + b_cinit);
  const float* dthr =
      devplan ? reinterpret_cast<const float*>(static_cast<char*>(c.frag.p) + b_all) : nullptr;
  if (delta) {
    screen32_delta_step(c, pl.QH, pl.MT, k, dfrag, dcinit, dcent, pl.thr0, pl.thr_rel, pl.Dv,
                        dthr, dout, hout, prof, gate);
    c.run_valid = true;
    c.run_k = k;
    return true;
  }
  c.lab8_valid = false;  // the full screen writes the labels alone
  const size_t lds = (size_t)NF * KP * 8 + (size_t)KP * 4 + (size_t)k * 17 * 8;
  const int64_t groups = c.n_pad / 64;
  const int cus = lloyd_num_cus(c.device);
  const int bpc = screen32_blocks_per_cu(pl.QH, pl.MT, lds);
  int nwg = (int)std::min<int64_t>(ceil_div(groups, 4), (int64_t)cus * bpc);
  if (nwg < 1) nwg = 1;
  const int nwaves = nwg * 4;
  const int cap = (int)(ceil_div(groups, nwaves) * 64);
  c.fb_list.ensure(sizeof(int32_t) * (size_t)nwaves * cap);
  fb_count_layout(c, nwaves);
  // pre-centred screen copy (exact; built once per point set)
  const bool pre = c.pre_ok && !exp_env("CDR_NO_PRE");
  if (pre) ensure_precentered(c);
  S32Args a;
  a.X = pre ? c.xt32.as<float>() : c.x32.as<float>();
  a.X0 = c.x32.as<float>();
  a.cent = dcent;
  a.n = c.n;
  a.n_pad = c.n_pad;
  a.d = d;
  a.k = k;
  a.Q = Q;
  a.frag = dfrag;
  a.cinit = dcinit;
  a.mu_s = c.mu_s.as<float>();
  a.sig = (float)std::ldexp(1.0, c.sigma);
  a.thr0 = pl.thr0;
  a.thr_rel = pl.thr_rel;
  a.labels = c.labels.as<int32_t>();
  a.run_sums = c.run_sums.as<unsigned long long>();
  a.muf = pre ? c.muf.as<long long>() : nullptr;
  a.fx = std::ldexp(1.0, c.scale_bits - (pre ? c.sigma : 0));
  a.KP = KP;
  a.fb_list = c.fb_list.as<int32_t>();
  a.fb_count = c.fb_count.as<int32_t>();
  a.fb_cap = cap;
  a.dbg = dbg;
  a.dbg_ld = (k + 15) / 16 * 16;
  a.gate = gate;
  a.thr_dev = dthr;
  // (the fourth argument was the DELTA form of this kernel: always false)
  snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen32<%d,%d,%s,false,%s,%s>", pl.QH, pl.MT,
           Q == 2 * pl.QH ? "true" : "false", dbg ? "true" : "false", pre ? "true" : "false");
  if (prof) prof_mark(c, 0);
  screen32_launch(pl.QH, pl.MT, dim3(nwg), c.stream, lds, a);
  HIP_CHECK(hipGetLastError());
  if (prof) prof_mark(c, 1);
  publish32_launch(c, k, nwaves, dout, hout, gate);
  c.run_valid = dbg == nullptr;
  c.run_k = k;
  return true;
}

}  // namespace cdr
