// screen_mid.hip — the host-plan screens of the medium shapes (F32X points,
// d <= 64, fragments + update table within 64 KiB of LDS) that screen32 does
// not take: three kernels per step (mid_step):
//   1. screen_fast (KT * DCH <= 4) or screen_kernel — fp16 hi/lo split MFMA
//      (v_mfma_f32_16x16x32_f16) screen of T_j ~ ||xhat - chat_j||^2 for every
//      centroid, a wave-level certified argmin (best and runner-up keys), and
//      — for certified points — the exact int64 fixed-point centroid
//      sums/counts privatised in LDS.  Uncertified points are appended to a
//      fallback list.
//   2. fallback_exact_wave — NumPy-order fp64 distances + correctly rounded
//      sqrt for the listed points, added into the screen's partial rows.
//   3. reduce_partials (lloyd_exact.hip) — sums the per-workgroup tables (no
//      float atomics, integer sums are order independent, hence
//      bit-reproducible).
// The certification bound makes the labels identical to the
// fp64 reference: a point is certified only when its runner-up screen value
// exceeds the best by more than twice the rigorous screen error plus the
// reference's own rounding slack.
#include <cstdio>
#include <cmath>
#include <type_traits>

#include "cdr_internal.h"
#include "exact_math.h"
#include "screen_fast.h"

namespace cdr {

// Running (best, runner-up) of unsigned keys: second = med3(best, v, second)
// holds because best <= second.
__device__ __forceinline__ void push_key(unsigned& bk, unsigned& sk, unsigned v) {
  sk = max(min(bk, v), min(max(bk, v), sk));  // v_med3_u32
  bk = min(bk, v);
}

// DCH = 4 is only instantiated with PACK6: its fragments and table do not fit
// 64 KiB once KT >= 5.
template <int DCH, bool PACK6, bool DBG>
__global__ __launch_bounds__(256) void screen_kernel(ScreenArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nfrag = a.KT * DCH * 2 * 64;
  h8* sfrag = reinterpret_cast<h8*>(smem);
  unsigned long long* tbl =
      reinterpret_cast<unsigned long long*>(smem + (size_t)nfrag * sizeof(h8));
  const int d = a.d;
  const int kd1 = d + 1;
  for (int i = threadIdx.x; i < nfrag; i += blockDim.x) sfrag[i] = a.frag[i];
  for (int i = threadIdx.x; i < a.k * kd1; i += blockDim.x) tbl[i] = 0ull;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;    // lane group: k-slots 8g..8g+7, centroid rows 4g..4g+3
  const int col = lane & 15;  // point column of the 16x16 tile
  float ms[DCH][4];
  bool fok[DCH][4];
#pragma unroll
  for (int c = 0; c < DCH; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 16 * c + 4 * g + i;
      fok[c][i] = f < d;
      ms[c][i] = fok[c][i] ? a.mu_s[f] : 0.0f;
    }
  const unsigned kmask = PACK6 ? 63u : 15u;
  const int wpb = blockDim.x >> 6;
  const int64_t ngroups = a.n_pad >> 6;
  const int wave_id = blockIdx.x * wpb + (threadIdx.x >> 6);
  int32_t* fb_region = a.fb_list + (size_t)wave_id * a.fb_cap;
  int fb_used = 0;
  for (int64_t G = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); G < ngroups;
       G += (int64_t)gridDim.x * wpb) {
    const int64_t base = G << 6;
    if (base >= a.n) continue;  // wave-uniform: padding groups
    float xr[4][DCH][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < DCH; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = 16 * c + 4 * g + i;
          xr[p][c][i] = fok[c][i] ? a.X[xidx(a.X, f, base + 16 * p + col, a.n_pad)] : 0.0f;
        }
    if (a.ablate & 8) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < DCH; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) xr[p][c][i] = (float)((int)(base + p * 16 + col + i) & 255) * 0x1p-8f;
    }
    h8 b1[4][DCH], b2[4][DCH];
    float xx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < DCH; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xt = fmaf(xr[p][c][i], a.sig, ms[c][i]);  // (x - mu) 2^sigma
          const _Float16 hi = (_Float16)xt;
          const _Float16 lo = (_Float16)(xt - (float)hi);
          s = fmaf(xt, xt, s);
          b1[p][c][2 * i] = hi;
          b1[p][c][2 * i + 1] = lo;
          b2[p][c][2 * i] = hi;
          b2[p][c][2 * i + 1] = (_Float16)0.0f;
        }
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      xx[p] = s;
      // chunk-0 spare slots: lane group 0 carries ||xhat||^2 (3-way fp16
      // split, paired with 1.0 in A), group 1 carries 1.0 (paired with the
      // 3-way split of ||chat_j||^2 + eps in A).
      _Float16 e0, e1, e2;
      if (g == 0) {
        e0 = (_Float16)s;
        float r = s - (float)e0;
        e1 = (_Float16)r;
        r = r - (float)e1;
        e2 = (_Float16)r;
      } else if (g == 1) {
        e0 = e1 = e2 = (_Float16)1.0f;
      } else {
        e0 = e1 = e2 = (_Float16)0.0f;
      }
      b2[p][0][1] = e0;
      b2[p][0][3] = e1;
      b2[p][0][5] = e2;
    }

    unsigned bk[4], sk[4];
    int bt[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      bk[p] = 0xFFFFFFFFu;
      sk[p] = 0xFFFFFFFFu;
      bt[p] = 0;
    }
    for (int t = 0; t < a.KT; ++t) {
      h8 A1[DCH], A2[DCH];
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        A1[c] = sfrag[((t * DCH + c) * 2 + 0) * 64 + lane];
        A2[c] = sfrag[((t * DCH + c) * 2 + 1) * 64 + lane];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.ablate & 4) {
          acc[0] = (float)b1[p][0][0] + (float)A1[0][1];
          acc[1] = (float)b2[p][0][1] + (float)A2[0][2];
          acc[2] = (float)b1[p][0][2] + t;
          acc[3] = xx[p];
        } else {
#pragma unroll
          for (int c = 0; c < DCH; ++c) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1[c], b1[p][c], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A2[c], b2[p][c], acc, 0, 0, 0);
          }
        }
        if (a.ablate & 2) {
          bk[p] ^= __float_as_uint(acc[0] + acc[1] + acc[2] + acc[3]);
          continue;
        }
        if constexpr (DBG) {
          const int64_t pt = base + 16 * p + col;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            a.dbg[pt * (int64_t)(a.KT * 16) + 16 * t + 4 * g + r] = acc[r];
        }
        if constexpr (PACK6) {
          const unsigned jb = 16u * (unsigned)t;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            push_key(bk[p], sk[p], (__float_as_uint(acc[r]) & ~63u) | (jb + r));
        } else {
          unsigned tb = (__float_as_uint(acc[0]) & ~15u) | 0u, ts = 0xFFFFFFFFu;
          push_key(tb, ts, (__float_as_uint(acc[1]) & ~15u) | 1u);
          push_key(tb, ts, (__float_as_uint(acc[2]) & ~15u) | 2u);
          push_key(tb, ts, (__float_as_uint(acc[3]) & ~15u) | 3u);
          const bool take = tb < bk[p];
          const unsigned nsk = min(max(bk[p], tb), min(sk[p], ts));
          bt[p] = take ? t : bt[p];
          bk[p] = min(bk[p], tb);
          sk[p] = nsk;
        }
      }
    }

#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned b = bk[p] | ((unsigned)g << 2), s = sk[p] | ((unsigned)g << 2);
      int tsel = bt[p];
#pragma unroll
      for (int m = 16; m <= 32; m <<= 1) {
        const unsigned ob = (unsigned)__shfl_xor((int)b, m);
        const unsigned os = (unsigned)__shfl_xor((int)s, m);
        const int ot = PACK6 ? 0 : __shfl_xor(tsel, m);
        const unsigned ns = min(max(b, ob), min(s, os));
        if (!PACK6) tsel = ob < b ? ot : tsel;
        b = min(b, ob);
        s = ns;
      }
      const int label = PACK6 ? (int)(b & 63u) : tsel * 16 + (int)(b & 15u);
      const float vb = __uint_as_float(b & ~kmask);
      const float vs = __uint_as_float(s & ~kmask);
      const float lim = fmaf(vb, 1.0f + 0x1p-15f, fmaf(a.thrA1, xx[p], a.thrA0));
      const bool cert = (a.ablate & 2) ? true : vs > lim;  // NaN: never certifies
      const int64_t pt = base + 16 * p + col;
      const bool real = pt < a.n;
      if (g == 0 && real) a.labels[pt] = label;
      const bool need = (g == 0) && real && !cert;
      const unsigned long long m = __ballot(need);
      if (m) {
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (need) fb_region[fb_used + rank] = (int32_t)pt;
        fb_used += __popcll(m);
      }
      if (a.ablate & 1) {
        asm volatile("" ::"v"(xr[p][0][0]), "v"(xr[p][0][3]), "v"(label));
        continue;
      }
      if (real && cert) {
        unsigned long long* row = tbl + (size_t)((unsigned)label < (unsigned)a.k ? label : 0) * kd1;
#pragma unroll
        for (int c = 0; c < DCH; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (fok[c][i]) {
              const long long u = (long long)(int)(xr[p][c][i] * a.fx);
              atomicAdd(&row[16 * c + 4 * g + i], (unsigned long long)u);
            }
        if (g == 0) atomicAdd(&row[d], 1ull);
      }
    }
  }
  if (lane == 0) {
    a.fb_count[wave_id] = fb_used;
    if (fb_used) atomicAdd(a.fb_count + (int64_t)gridDim.x * wpb, fb_used);
  }
  __syncthreads();
  unsigned long long* dst = a.partials + (size_t)blockIdx.x * a.k * kd1;
  for (int i = threadIdx.x; i < a.k * kd1; i += blockDim.x) dst[i] = tbl[i];
}

// Wave-wide minimum, result in every lane: row_ror 8/4/2/1 inside each row of
// 16 lanes (DPP), then the permlane16 / permlane32 swaps across rows.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xF, 0xF, false);
  const unsigned hi =
      (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_min_f64(double v) {
  v = fmin(v, dpp_f64<0x128>(v));
  v = fmin(v, dpp_f64<0x124>(v));
  v = fmin(v, dpp_f64<0x122>(v));
  v = fmin(v, dpp_f64<0x121>(v));
  auto mk = [](unsigned lo, unsigned hi) {
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  };
  unsigned long long u = (unsigned long long)__double_as_longlong(v);
  auto l16 = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
  auto h16 = __builtin_amdgcn_permlane16_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
  v = fmin(mk(l16[0], h16[0]), mk(l16[1], h16[1]));
  u = (unsigned long long)__double_as_longlong(v);
  auto l32 = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);
  auto h32 = __builtin_amdgcn_permlane32_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
  return fmin(mk(l32[0], h32[0]), mk(l32[1], h32[1]));
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false));
  v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false));
  v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x122, 0xF, 0xF, false));
  v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x121, 0xF, 0xF, false));
  auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = min(r16[0], r16[1]);
  auto r32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return min(r32[0], r32[1]);
}

// Exact assignment of the points the screen did not certify: one wave per
// point, lane j computes the NumPy-order fp64 distance to centroids j, j+64,
// ... and its correctly rounded sqrt; first index on ties of the roots, as
// np.argmin sees them (reference src/kmeans_plusplus.py:33-34).  Workgroup b's
// waves take the screen's fallback regions 4b..4b+3, so the grid equals the
// screen's; lane f holds feature f of the point (prefetched one point ahead)
// and broadcasts it with readlane.  Sums go to an LDS table laid out like the
// screen's (row stride KS, count at KS-1), which is then added into the
// screen's partial row b — reduce_partials runs afterwards, so there are no
// global atomics.  The centroids are staged transposed ([d][k]) in LDS behind
// the table: they fit whenever the screen itself does.
// Requires d <= 64.
__global__ __launch_bounds__(256) void fallback_exact_wave(
    const float* __restrict__ X, int64_t n_pad, int d, const double* __restrict__ C, int k,
    const int32_t* __restrict__ list, const int32_t* __restrict__ count, int cap, int KS,
    int32_t* __restrict__ labels, unsigned long long* __restrict__ partials, float fx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* tbl = reinterpret_cast<unsigned long long*>(smem);
  double* ct = reinterpret_cast<double*>(tbl + (size_t)k * KS);
  const int tk = k * KS;
  for (int i = threadIdx.x; i < tk; i += blockDim.x) tbl[i] = 0ull;
  for (int i = threadIdx.x; i < k * d; i += blockDim.x) {
    const int j = i / d, f = i - j * d;
    ct[f * k + j] = C[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int reg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int cnt = count[reg];
  const int32_t* lst = list + (size_t)reg * cap;
  auto cval = [&](int f, int j) -> double { return ct[f * k + j]; };
  int chunk = 0;  // list entries 64m .. 64m+63, one per lane
  int64_t pt = 0;
  float xf = 0.0f;
  if (cnt > 0) {
    chunk = lst[lane < cnt ? lane : 0];
    pt = __builtin_amdgcn_readfirstlane(chunk);
    if (lane < d) xf = X[xidx(X, lane, pt, n_pad)];
  }
  for (int e = 0; e < cnt; ++e) {
    const int64_t cpt = pt;
    const int cx = __float_as_int(xf);
    if (e + 1 < cnt) {  // prefetch the next point
      const int e1 = e + 1;
      if ((e1 & 63) == 0) chunk = lst[e1 + lane < cnt ? e1 + lane : e1];
      pt = __builtin_amdgcn_readlane(chunk, e1 & 63);
      if (lane < d) xf = X[xidx(X, lane, pt, n_pad)];
    }
    auto xv = [&](int f) { return (double)__int_as_float(__builtin_amdgcn_readlane(cx, f)); };
    double rb = INFINITY;
    int jb = k;
    for (int j = lane; j < k; j += 64) {
      const double r = sqrt(np_sqdist(xv, [&](int f) { return cval(f, j); }, d));
      if (r < rb) {  // j increases per lane: strict < keeps the first index
        rb = r;
        jb = j;
      }
    }
    const double m = wave_min_f64(rb);
    int jmin;
    if (k <= 64) {
      jmin = (int)__builtin_ctzll(__ballot(rb == m));  // lane == j
    } else {
      jmin = (int)wave_min_u32(rb == m ? (unsigned)jb : 0xFFFFFFFFu);
    }
    if (lane == 0) labels[cpt] = jmin;
    if (lane < d)
      atomicAdd(&tbl[(size_t)jmin * KS + lane],
                (unsigned long long)(long long)(int)(__int_as_float(cx) * fx));
    if (lane == 0) atomicAdd(&tbl[(size_t)jmin * KS + KS - 1], 1ull);  // d may be 64
  }
  __syncthreads();
  unsigned long long* dst = partials + (size_t)blockIdx.x * tk;
  for (int i = threadIdx.x; i < tk; i += blockDim.x) {
    const unsigned long long v = tbl[i];
    if (v) dst[i] += v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct ScreenPlan {
  int DCH, KT;
  bool pack6, fast;
  float thrA0, thrA1;
  std::vector<h8> frag;
};

// Build the fp16 A-operand fragments and the certification constants
// (derivation: DESIGN.md §3 "screen error bound").
static void build_screen_plan(const Ctx& c, const double* C, int k, ScreenPlan& pl,
                              bool allow_fast = true) {
  const int d = c.d;
  pl.DCH = (d + 15) / 16;
  pl.KT = (k + 15) / 16;
  pl.pack6 = pl.KT <= 4;
  const double sc = std::ldexp(1.0, c.sigma);
  std::vector<double> ch((size_t)k * d);
  double ccmax = 0.0;
  std::vector<double> cc(k, 0.0);
  for (int j = 0; j < k; ++j) {
    double s = 0.0;
    for (int f = 0; f < d; ++f) {
      const double v = (C[(size_t)j * d + f] - (double)c.mu[f]) * sc;
      ch[(size_t)j * d + f] = v;
      s += v * v;
    }
    cc[j] = s;
    ccmax = std::fmax(ccmax, s);
  }
  const double u = std::ldexp(1.0, -24);
  const double N = 64.0 * pl.DCH + 1.0;
  // factor 2 on the accumulation term: no assumption on the MFMA's internal
  // rounding beyond "each of its N additions errs by at most 2u".
  const double a = (2.0 * 2.02 * N + 14.0) * u;
  const double b = (4.04 * d + 8.0) * u + std::ldexp(1.0, -30);
  const double xxmax = d * (1.0 + 1e-6);
  const double eps = a * (ccmax + xxmax) + b;
  const double ccp = ccmax + eps;
  pl.thrA0 = (float)(2.02 * (a * ccp + b) + std::ldexp(ccp, -40));
  pl.thrA1 = (float)(2.02 * a * (1.0 + std::ldexp(1.0, -10)) + std::ldexp(1.0, -40));
  pl.thrA0 *= 1.0001f;
  pl.thrA1 *= 1.0001f;

  pl.fast = allow_fast && pl.KT * pl.DCH <= 4;
  pl.frag.assign((size_t)pl.KT * pl.DCH * 2 * 64, h8{});
  for (int t = 0; t < pl.KT; ++t)
    for (int cch = 0; cch < pl.DCH; ++cch)
      for (int lane = 0; lane < 64; ++lane) {
        const int j = 16 * t + (lane & 15);
        const int g = lane >> 4;
        h8 A1 = {}, A2 = {};
        // k-slot of (feature i, part): fast kernel [hi0..3 | lo0..3],
        // generic kernel interleaved [hi0, lo0, hi1, lo1, ...]
        auto slot_hi = [&](int i) { return pl.fast ? i : 2 * i; };
        auto slot_lo = [&](int i) { return pl.fast ? 4 + i : 2 * i + 1; };
        auto slot_ex = [&](int e) { return pl.fast ? 4 + e : 2 * e + 1; };
        for (int i = 0; i < 4; ++i) {
          const int f = 16 * cch + 4 * g + i;
          if (j < k && f < d) {
            const double v = ch[(size_t)j * d + f];
            const _Float16 hi = (_Float16)v;
            const _Float16 lo = (_Float16)(v - (double)hi);
            A1[slot_hi(i)] = (_Float16)(-2.0 * (double)hi);
            A1[slot_lo(i)] = (_Float16)(-2.0 * (double)hi);
            A2[slot_hi(i)] = (_Float16)(-2.0 * (double)lo);
          }
        }
        if (cch == 0) {
          if (g == 0) {
            A2[slot_ex(0)] = A2[slot_ex(1)] = A2[slot_ex(2)] = (_Float16)1.0f;
          } else if (g == 1) {
            if (j < k) {
              const double v = cc[j] + eps;
              const _Float16 p0 = (_Float16)v;
              const double r1 = v - (double)p0;
              const _Float16 p1 = (_Float16)r1;
              const double r2 = r1 - (double)p1;
              const _Float16 p2 = (_Float16)r2;
              A2[slot_ex(0)] = p0;
              A2[slot_ex(1)] = p1;
              A2[slot_ex(2)] = p2;
            } else {
              A2[slot_ex(0)] = (_Float16)30000.0f;  // padding centroid: never the best
            }
          }
        }
        pl.frag[(((size_t)t * pl.DCH + cch) * 2 + 0) * 64 + lane] = A1;
        pl.frag[(((size_t)t * pl.DCH + cch) * 2 + 1) * 64 + lane] = A2;
      }
}

// f(integral_constant<int, DCH>, integral_constant<int, KT>) for the runtime
// (DCH, KT) of screen_fast: the eight shapes with KT * DCH <= 4; anything
// else is a caller's error.
template <class F>
static void dispatch_dch_kt(int DCH, int KT, F&& f) {
  using std::integral_constant;
  switch (10 * DCH + KT) {
    case 11: return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
    case 12: return f(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    case 13: return f(integral_constant<int, 1>{}, integral_constant<int, 3>{});
    case 14: return f(integral_constant<int, 1>{}, integral_constant<int, 4>{});
    case 21: return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    case 22: return f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
    case 31: return f(integral_constant<int, 3>{}, integral_constant<int, 1>{});
    case 41: return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    default: CDR_FAIL(CDR_ERR_STATE, "screen_fast: no kernel for this (DCH, KT)");
  }
}

// Workgroups per CU of screen_fast<DCH, KT>, 1..8 (2 when the query fails)
static int fast_blocks_per_cu(int DCH, int KT, size_t lds) {
  int nb = 0;
  hipError_t e = hipErrorInvalidValue;
  dispatch_dch_kt(DCH, KT, [&](auto dch, auto kt) {
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nb, screen_fast<decltype(dch)::value, decltype(kt)::value, true, true>, 256, lds);
  });
  if (e != hipSuccess || nb < 1) nb = 2;
  return nb > 8 ? 8 : nb;
}

static void launch_fast(int DCH, int KT, bool nonneg, bool full, dim3 grid, size_t lds,
                        hipStream_t s, const ScreenArgs& a) {
#ifdef CDR_EXPERIMENTS
  if (a.ablate && DCH == 1 && KT == 4 && nonneg && full) {  // timing experiments
    switch (a.ablate) {
      case 1: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 1>), grid, dim3(256), lds, s, a); return;
      case 2: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 2>), grid, dim3(256), lds, s, a); return;
      case 8: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 8>), grid, dim3(256), lds, s, a); return;
      case 9: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 9>), grid, dim3(256), lds, s, a); return;
      case 10: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 10>), grid, dim3(256), lds, s, a); return;
      case 16: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 0, 2>), grid, dim3(256), lds, s, a); return;
      case 18: hipLaunchKernelGGL((screen_fast<1, 4, true, true, 0, 1>), grid, dim3(256), lds, s, a); return;
      default: break;
    }
  }
#endif
  dispatch_dch_kt(DCH, KT, [&](auto dch, auto kt) {
    constexpr int D_ = decltype(dch)::value, K_ = decltype(kt)::value;
    if (nonneg) {
      if (full) hipLaunchKernelGGL((screen_fast<D_, K_, true, true>), grid, dim3(256), lds, s, a);
      else hipLaunchKernelGGL((screen_fast<D_, K_, true, false>), grid, dim3(256), lds, s, a);
    } else {
      if (full) hipLaunchKernelGGL((screen_fast<D_, K_, false, true>), grid, dim3(256), lds, s, a);
      else hipLaunchKernelGGL((screen_fast<D_, K_, false, false>), grid, dim3(256), lds, s, a);
    }
  });
}

template <int DCH>
static void launch_screen(bool pack6, bool dbg, dim3 grid, size_t lds, hipStream_t s,
                          const ScreenArgs& a) {
  if (pack6) {
    if (dbg) hipLaunchKernelGGL((screen_kernel<DCH, true, true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((screen_kernel<DCH, true, false>), grid, dim3(256), lds, s, a);
  } else if constexpr (DCH < 4) {
    if (dbg) hipLaunchKernelGGL((screen_kernel<DCH, false, true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((screen_kernel<DCH, false, false>), grid, dim3(256), lds, s, a);
  } else {
    CDR_FAIL(CDR_ERR_STATE, "screen_kernel: DCH = 4 with KT >= 5 does not fit the LDS");
  }
}

static size_t screen_lds_bytes(int KT, int DCH, int k, int d) {
  return (size_t)KT * DCH * 2 * 64 * sizeof(h8) + (size_t)k * (d + 1) * 8;
}

bool screen_supported(const Ctx& c, int k) {
  const int DCH = (c.d + 15) / 16, KT = (k + 15) / 16;
  return c.d <= 64 && DCH <= 4 && screen_lds_bytes(KT, DCH, k, c.d) <= 64 * 1024;
}

void mid_thresholds(const Ctx& c, const double* C, int k, float thr[2]) {
  ScreenPlan pl;
  build_screen_plan(c, C, k, pl);
  thr[0] = pl.thrA0;
  thr[1] = pl.thrA1;
}

bool mid_step(Ctx& c, const double* C, int k, long long* dout, bool prof) {
  if (!screen_supported(c, k)) return false;
  drop_running_state(c);  // the screen_fast / screen_kernel path keeps no running sums
  const int d = c.d, kd1 = d + 1, len = k * kd1;
  const float fx = (float)std::ldexp(1.0, c.scale_bits);
  const bool dbg = c.dbg_vals != nullptr;
  ScreenPlan pl;
  build_screen_plan(c, C, k, pl, !dbg);
  c.frag.ensure(pl.frag.size() * sizeof(h8));
  HIP_CHECK(hipMemcpyAsync(c.frag.p, pl.frag.data(), pl.frag.size() * sizeof(h8),
                           hipMemcpyHostToDevice, c.stream));
  const int d4 = d4_of(d);
  const int KS = pl.fast ? d4 + 1 : kd1;
  const size_t lds = pl.fast ? (size_t)k * KS * 8 : screen_lds_bytes(pl.KT, pl.DCH, k, d);
  const int64_t groups = c.n_pad / 64;
  const int bpc = pl.fast ? fast_blocks_per_cu(pl.DCH, pl.KT, lds) : 4;
  int nwg = (int)std::min<int64_t>(ceil_div(groups, 4), (int64_t)lloyd_num_cus(c.device) * bpc);
  if (nwg < 1) nwg = 1;
  c.partials.ensure(sizeof(long long) * (size_t)nwg * k * KS);
  const int nwaves = nwg * 4;
  const int cap = (int)(ceil_div(groups, nwaves) * 64);
  c.fb_list.ensure(sizeof(int32_t) * (size_t)nwaves * cap);
  c.fb_count.ensure(sizeof(int32_t) * (nwaves + 1));
  HIP_CHECK(hipMemsetAsync(c.fb_count.p, 0, sizeof(int32_t) * (nwaves + 1), c.stream));
  c.fb_regions = nwaves;
  c.fb_total_slot = nwaves;
  c.fb_layout = -1;  // screen32 must re-zero its counter layout
  ScreenArgs a;
  a.X = c.x32.as<float>();
  a.n = c.n;
  a.n_pad = c.n_pad;
  a.d = d;
  a.k = k;
  a.KT = pl.KT;
  a.frag = c.frag.as<h8>();
  a.mu_s = c.mu_s.as<float>();
  a.sig = (float)std::ldexp(1.0, c.sigma);
  a.fx = fx;
  a.thrA0 = pl.thrA0;
  a.thrA1 = pl.thrA1;
  a.labels = c.labels.as<int32_t>();
  a.partials = c.partials.as<unsigned long long>();
  a.fb_list = c.fb_list.as<int32_t>();
  a.fb_count = c.fb_count.as<int32_t>();
  a.fb_cap = cap;
  a.dbg = c.dbg_vals;
#ifdef CDR_EXPERIMENTS
  a.ablate = c.screen_ablate;
#else
  a.ablate = 0;
#endif
  if (pl.fast)
    snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen_fast<%d,%d>", pl.DCH, pl.KT);
  else
    snprintf(c.prof_kernel, sizeof(c.prof_kernel), "screen_kernel<%d>", pl.DCH);
  if (prof) prof_mark(c, 0);
  if (pl.fast) {
    bool nonneg = true;
    for (int f = 0; f < d; ++f) nonneg = nonneg && c.fmin[f] >= 0.0;
    launch_fast(pl.DCH, pl.KT, nonneg, d4 == 16 * pl.DCH, dim3(nwg), lds, c.stream, a);
  } else {
    switch (pl.DCH) {
      case 1: launch_screen<1>(pl.pack6, dbg, dim3(nwg), lds, c.stream, a); break;
      case 2: launch_screen<2>(pl.pack6, dbg, dim3(nwg), lds, c.stream, a); break;
      case 3: launch_screen<3>(pl.pack6, dbg, dim3(nwg), lds, c.stream, a); break;
      default: launch_screen<4>(pl.pack6, dbg, dim3(nwg), lds, c.stream, a); break;
    }
  }
  HIP_CHECK(hipGetLastError());
  if (prof) prof_mark(c, 1);
  // fallback first: it adds into the screen's partial rows
  hipLaunchKernelGGL(fallback_exact_wave, dim3(nwg), dim3(256),
                     (size_t)k * KS * 8 + (size_t)k * d * 8, c.stream, c.x32.as<float>(), c.n_pad,
                     d, c.cent64.as<double>(), k, c.fb_list.as<int32_t>(),
                     c.fb_count.as<int32_t>(), cap, KS, c.labels.as<int32_t>(),
                     c.partials.as<unsigned long long>(), fx);
  HIP_CHECK(hipGetLastError());
  enqueue_reduce_partials(c, nwg, len, KS, dout);
  return true;
}

}  // namespace cdr
