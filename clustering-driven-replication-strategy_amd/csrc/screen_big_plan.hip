// screen_big_plan.hip — the plan of one large-k Lloyd step (screen_big.hip):
// the fp16 A fragments of the centroids, the C operand rows, the fp64
// centroids and the two thresholds, in the layout of big_layout.  Built on
// the host and uploaded (big_plan_host), or built on the device from the
// device loop's centroids (big_plan_device); both give the same bytes.
#include <cmath>
#include <cstring>
#include <vector>

#include "exact_math.h"
#include "screen_big.h"

namespace cdr {

namespace {

// dst[i] = src[i] for 16-byte words; src is mapped pinned host memory.
__global__ __launch_bounds__(256) void pull_host_big(const uint4* __restrict__ src,
                                                     uint4* __restrict__ dst, int64_t n16) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

struct PlanBig {
  std::vector<h8> frag1;
  std::vector<float> cinit;
  float thr1, thr_rel;
  int jbits;
};

// Rigorous screen error bounds (see the head of screen_big.hip); mirrors
// build_plan32's terms with N = fp32 additions in the MFMA chain.  Shared by
// the host plan (build_plan_big) and the device plan (big_plan_kernel): the
// same fp64 operations in the same order, so both give the same bits.
struct BigBounds {
  double D;
  float thr1, thr_rel;
  int jbits;
};

__host__ __device__ inline BigBounds big_bounds(double ccmax, double l1c, double xxmax,
                                                double l1x, int DQ, int KB) {
  BigBounds r;
  const double u = ldexp(1.0, -24);
  const double eps = ldexp(1.0, -11), eta = ldexp(1.0, -25);
  const double cx = sqrt(ccmax * xxmax);
  // one product: |c.x - chi.xhi| <= 2 eps (1 + eps) ||c|| ||x|| + eta (l1x + (1 + eps) l1c)
  const double P1 = 2.0 * eps * (1.0 + eps) * cx + eta * (l1x + (1.0 + eps) * l1c);
  const double N1 = 16.0 * DQ + 1.0;
  const double g1 = 2.0 * u * N1 / (1.0 - 2.0 * u * N1);
  const double E1a = 2.0 * P1 + g1 * (ccmax + 2.0 * xxmax + 4.0 * cx + 4.0) + u * (ccmax + 2.0 * xxmax + 4.0);
  // D >= max ||xhat||^2 + margin keeps every screen value >= 0
  const double D = xxmax + 4.0 * E1a + ldexp(1.0, -20);
  const double sum1 = (ccmax + D) * (1.0 + u) + 2.0 * (1.0 + eps) * (1.0 + eps) * cx;
  const double E1 = 2.0 * P1 + g1 * sum1 + u * (ccmax + D) + ldexp(1.0, -46) * (ccmax + D);
  // reference slack: the fp64 distances and roots must not tie or flip
  const double Wmax = (sqrt(ccmax) + sqrt(xxmax)) * (sqrt(ccmax) + sqrt(xxmax));
  const double slack = ldexp(Wmax + 1.0, -38);
  r.D = D;
  r.thr1 = (float)((2.0 * E1 + slack) * 1.001);
  // keys keep the centroid index in their low JB bits (screen_big_sp): best
  // and runner-up are each within 2^JB ulps (2^(JB-23) relative) of their
  // screen values, covered by 1 + 4 * 2^(JB-23)
  r.jbits = big_jbits(KB);
  r.thr_rel = 1.0f + ldexpf(1.0f, r.jbits - 21);
  return r;
}

// The point side of the bounds: max ||xhat||^2 (with a 1e-6 margin) and max
// ||xhat||_1 over the data's bounding box.
void big_point_side(const Ctx& c, double& xxmax, double& l1x) {
  const double sc = std::ldexp(1.0, c.sigma);
  xxmax = 0.0;
  l1x = 0.0;
  for (int f = 0; f < c.d; ++f) {
    const double dev =
        std::fmax(c.fmax[f] - (double)c.mu[f], (double)c.mu[f] - c.fmin[f]) * sc;
    xxmax += dev * dev;
    l1x += dev;
  }
  xxmax *= 1.0 + 1e-6;
}

// A fragment of one lane of centroid block b, feature chunk cq (the L1 / L2
// A operand: -2 chi, rows in big_row order).
__host__ __device__ inline h8 big_frag_lane(const double* C, const double* mu, double sc, int k,
                                            int d, int b, int cq, int lane) {
  const int j = 32 * b + big_row(lane & 31);
  const int hh = lane >> 5;
  h8 A1 = {};
  for (int i = 0; i < 8; ++i) {
    const int f = 16 * cq + 8 * hh + i;
    if (j >= k || f >= d) continue;
    const double v = (C[(size_t)j * d + f] - mu[f]) * sc;
    const _Float16 hi = f64_to_f16(v);
    A1[i] = f64_to_f16(-2.0 * (double)hi);
  }
  return A1;
}

void build_plan_big(const Ctx& c, const double* C, int k, PlanBig& pl) {
  const int d = c.d, DQ = big_dq(d), KB = (k + 31) / 32;
  const double sc = std::ldexp(1.0, c.sigma);
  std::vector<double> mu(d), cc(k, 0.0);
  for (int f = 0; f < d; ++f) mu[f] = (double)c.mu[f];
  double ccmax = 0.0, l1c = 0.0;
  for (int j = 0; j < k; ++j) {
    double s = 0.0, l1 = 0.0;
    for (int f = 0; f < d; ++f) {
      const double v = (C[(size_t)j * d + f] - mu[f]) * sc;
      s += v * v;
      l1 += std::fabs(v);
    }
    cc[j] = s;
    ccmax = std::fmax(ccmax, s);
    l1c = std::fmax(l1c, l1);
  }
  double xxmax, l1x;
  big_point_side(c, xxmax, l1x);
  const BigBounds bb = big_bounds(ccmax, l1c, xxmax, l1x, DQ, KB);
  pl.thr1 = bb.thr1;
  pl.thr_rel = bb.thr_rel;
  pl.jbits = bb.jbits;
  pl.cinit.assign((size_t)KB * 32, 1.0e30f);
  for (int r = 0; r < KB * 32; ++r) {
    const int j = 32 * (r / 32) + big_row(r % 32);
    if (j < k) pl.cinit[r] = (float)(cc[j] + bb.D);
  }
  pl.frag1.assign((size_t)KB * DQ * 64, h8{});
  for (int b = 0; b < KB; ++b)
    for (int cq = 0; cq < DQ; ++cq)
      for (int lane = 0; lane < 64; ++lane)
        pl.frag1[((size_t)b * DQ + cq) * 64 + lane] =
            big_frag_lane(C, mu.data(), sc, k, d, b, cq, lane);
}

// Device-resident loop (loop.hip): the same plan built on the device from the
// loop's centroids, into the layout big_plan_host uploads.  One 1024-thread
// workgroup; gated on the loop state.
struct BigPlanArgs {
  const double* C;
  const double* mu;  // double[d]
  double sc, xxmax, l1x;
  int k, d, DQ, KB;
  h8* frag1;
  float* cinit;
  double* C64;
  float* thr;
  const long long* gate;
};

__global__ __launch_bounds__(1024) void big_plan_kernel(BigPlanArgs a) {
  if (a.gate && a.gate[0] == 0) return;
  extern __shared__ double scc[];  // [k]
  __shared__ double rmax[2][16];
  __shared__ double sD;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int k = a.k, d = a.d;
  double m0 = 0.0, m1 = 0.0;
  for (int j = t; j < k; j += blockDim.x) {
    double s = 0.0, l1 = 0.0;
    for (int f = 0; f < d; ++f) {
      const double v = (a.C[(size_t)j * d + f] - a.mu[f]) * a.sc;
      s += v * v;
      l1 += fabs(v);
    }
    scc[j] = s;
    m0 = fmax(m0, s);
    m1 = fmax(m1, l1);
  }
  for (int o = 32; o > 0; o >>= 1) {
    m0 = fmax(m0, __shfl_xor(m0, o));
    m1 = fmax(m1, __shfl_xor(m1, o));
  }
  if (lane == 0) {
    rmax[0][w] = m0;
    rmax[1][w] = m1;
  }
  __syncthreads();
  if (t == 0) {
    double ccmax = 0.0, l1c = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
      ccmax = fmax(ccmax, rmax[0][i]);
      l1c = fmax(l1c, rmax[1][i]);
    }
    const BigBounds bb = big_bounds(ccmax, l1c, a.xxmax, a.l1x, a.DQ, a.KB);
    sD = bb.D;
    a.thr[0] = bb.thr1;
    a.thr[1] = bb.thr_rel;
  }
  __syncthreads();
  const double D = sD;
  for (int r = t; r < a.KB * 32; r += blockDim.x) {
    const int j = 32 * (r / 32) + big_row(r % 32);
    a.cinit[r] = j < k ? (float)(scc[j] + D) : 1.0e30f;
  }
  for (int e = t; e < a.KB * a.DQ * 64; e += blockDim.x) {
    const int l = e & 63, bc = e >> 6;
    a.frag1[e] = big_frag_lane(a.C, a.mu, a.sc, k, d, bc / a.DQ, bc % a.DQ, l);
  }
  for (int e = t; e < k * d; e += blockDim.x) a.C64[e] = a.C[e];
}

}  // namespace

void big_plan_host(Ctx& c, const double* C, int k, float thr[2]) {
  PlanBig pl;
  build_plan_big(c, C, k, pl);
  const BigLayout L = big_layout(k, c.d);
  // one upload: frag1 | cinit | C (fp64)
  if (c.up_pending) HIP_CHECK(hipEventSynchronize(c.up_event));
  c.h_up.ensure(L.all);
  char* hp = static_cast<char*>(c.h_up.p);
  memcpy(hp, pl.frag1.data(), L.b1);
  memcpy(hp + L.o_cinit, pl.cinit.data(), L.bc);
  memcpy(hp + L.o_C, C, L.bC);
  c.frag.ensure(L.all);
  {
    void* hdev = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&hdev, c.h_up.p, 0));
    const int64_t n16 = (int64_t)((L.o_thr + 15) / 16);
    hipLaunchKernelGGL(pull_host_big, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0,
                       c.stream, static_cast<const uint4*>(hdev), static_cast<uint4*>(c.frag.p),
                       n16);
    HIP_CHECK(hipGetLastError());
  }
  if (!c.up_event) HIP_CHECK(hipEventCreateWithFlags(&c.up_event, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(c.up_event, c.stream));
  c.up_pending = true;
  thr[0] = pl.thr1;
  thr[1] = pl.thr_rel;
}

// The device-resident loop's plan (loop.hip): built on the device from the
// loop's centroids dC (fp64, k x d) into c.frag; gate = the loop state.
void big_plan_device(Ctx& c, int k, const double* dC, const double* dmu, const long long* gate) {
  const int d = c.d;
  const BigLayout L = big_layout(k, d);
  c.frag.ensure(L.all);
  char* dp = static_cast<char*>(c.frag.p);
  BigPlanArgs a;
  a.C = dC;
  a.mu = dmu;
  a.sc = std::ldexp(1.0, c.sigma);
  big_point_side(c, a.xxmax, a.l1x);
  a.k = k;
  a.d = d;
  a.DQ = big_dq(d);
  a.KB = (k + 31) / 32;
  a.frag1 = reinterpret_cast<h8*>(dp);
  a.cinit = reinterpret_cast<float*>(dp + L.o_cinit);
  a.C64 = reinterpret_cast<double*>(dp + L.o_C);
  a.thr = reinterpret_cast<float*>(dp + L.o_thr);
  a.gate = gate;
  hipLaunchKernelGGL(big_plan_kernel, dim3(1), dim3(1024), sizeof(double) * (size_t)k, c.stream,
                     a);
  HIP_CHECK(hipGetLastError());
}

// cdr_debug_big_plan (tests): the plan buffer of the last large-k step of k
// centroids, frag1 | cinit | C | {thr1, thr_rel} (big_layout).  A host plan
// passes its thresholds to the kernels by value; they are put in their slot
// here.  Returns the bytes written; out may be null to ask for the size.
int64_t debug_big_plan(Ctx& c, int k, void* out, int64_t bytes) {
  if (c.big_info[0] == 0 || c.big_k != k)
    CDR_FAIL(CDR_ERR_STATE, "debug_big_plan: the last large-k step was not of this k");
  const BigLayout L = big_layout(k, c.d);
  if (!out) return (int64_t)L.used;
  if (bytes < (int64_t)L.used || c.frag.bytes < L.used)
    CDR_FAIL(CDR_ERR_ARG, "debug_big_plan: buffer too small");
  HIP_CHECK(hipMemcpyAsync(out, c.frag.p, L.used, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (c.big_info[10] == 0) {
    char* t = static_cast<char*>(out) + L.o_thr;
    memset(t, 0, L.bt);
    memcpy(t, c.big_thr_host, sizeof(c.big_thr_host));
  }
  return (int64_t)L.used;
}

}  // namespace cdr
