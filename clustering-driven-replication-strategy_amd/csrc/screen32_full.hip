// screen32_full.hip — the full screen: Lloyd assign + fused update of every
// point for small d and k (d <= 16, k <= 64: BASELINE configs 2 and 3),
// reference src/kmeans_plusplus.py:33-41.  The first step of a run, and every
// step whose labels or running sums another path wrote; the later (DELTA)
// steps go to screen32p / screen32b / screen32bs.
//
// One wave handles a group of 64 points as two 32-point tiles.  Distances come
// from v_mfma_f32_32x32x16_f16 in the ||x||^2 - 2 x.c + ||c||^2 form with the
// point norm replaced by a launch constant D (argmin is unchanged by a per-point
// shift; D keeps every screen value >= 0 so raw fp32 bits order as unsigned):
//
//   S_j = fl32( C_j + sum_f -2 chi_jf (hi_f + lo_f) - 2 clo_jf hi_f ),
//   C_j = fl32(||chat_j||^2 + D)  (the MFMA C operand, a per-lane constant)
//
// with xhat = (x - mu) 2^sigma split into fp16 hi + lo and chat likewise
// (chi + clo).  Per 32 centroids and 32 points that is three MFMAs for d = 16:
//   A1 x H  (H = [hi(q0), hi(q1)],  A1 = [-2chi(q0), -2chi(q1)])
//   A1 x L  (L = [lo(q0), lo(q1)])
//   A3 x H  (A3 = [-2clo(q0), -2clo(q1)])
// where lane half h owns the feature quads q0 = QH*h, q1 = QH*h + 1; for d <= 8
// (QH = 1) H = [hi(q0), lo(q0)], A1 = [-2chi, -2chi], A3 = [-2clo, 0] and the
// two MFMAs are A1 x H, A3 x H.  Every B operand is one 4-register tuple.
//
// Argmin: every lane keeps (best, runner-up) unsigned keys of its 32 values
// (value bits with the low 6 replaced by the row index), the two lane halves
// of a point are merged with one permlane32 swap per pair of tiles, after which
// lane l owns point base + l: one coalesced label store, one certification
// test, one fallback ballot.  A point is certified when
//     key_s > key_b * (1 + 2^-17) + T0
// (T0 = twice the rigorous screen error + the reference's rounding slack,
// derived in build_plan32 / DESIGN.md §4); uncertified points go to a per-wave
// fallback region and are re-done in exact fp64 NumPy order (fallback_points).
//
// Update: certified points add their fp32 features (exact in fp64: grid data,
// see screen32_supported) into a per-workgroup LDS table sum[f][j] with
// ds_add_f64 and their count with ds_add_u32; the workgroup's tail converts
// its sums to exact int64 fixed point and adds them to the running sums.
#include "screen32_common.h"

namespace cdr {

// Exact assignment of the points the screen could not certify, run by the
// wave that found them after its last group (its region of the fallback
// list; the LDS table is still live, so no global read-modify-write and no
// extra launch).  4 lanes per point, 16 points per pass: lane c walks the
// centroids c, c + 4, c + 8, ... (fp64 rows staged in LDS with stride 17
// doubles) computing the NumPy-order fp64 squared distance and its correctly
// rounded sqrt and keeping the first minimum of its roots; the 4 candidates
// merge on (root, index) — np.argmin of np.linalg.norm, first index on ties
// (src/kmeans_plusplus.py:33-34).  The point's change goes into the table.
// Loads run ahead of the arithmetic: list entries two passes, the points'
// feature quads one pass.
template <int D>
__device__ __forceinline__ void fallback_points(const S32Args& a, const int32_t* region, int cnt,
                                                double* tsum, int* tcnt, const double* cs,
                                                int KP, bool delta, bool pre) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 2, c4 = lane & 3;
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int Q = (D + 3) / 4;
  const f4* X4 = reinterpret_cast<const f4*>(a.X0);
  __threadfence_block();  // the region was just written by this wave's lanes
  auto load_pt = [&](int e) -> int32_t { return e < cnt ? region[e] : 0; };
  auto load_x = [&](int32_t pt, f4 (&v)[Q]) {
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = X4[(int64_t)q * a.n_pad + pt];
  };
  int32_t pt0 = load_pt(g), pt1 = load_pt(16 + g);
  f4 x0[Q];
  load_x(pt0, x0);
  for (int e0 = 0; e0 < cnt; e0 += 16) {
    const int e = e0 + g;
    const bool live = e < cnt;
    const int32_t pt = pt0;
    double x[D];
#pragma unroll
    for (int f = 0; f < D; ++f) x[f] = (double)x0[f >> 2][f & 3];
    if (e0 + 16 < cnt) {  // wave-uniform
      pt0 = pt1;
      load_x(pt0, x0);
      pt1 = load_pt(e0 + 32 + g);
    }
    double sb = INFINITY, rb = INFINITY;
    int jmin = 0x7fffffff;
    for (int j = c4; j < a.k; j += 4) {
      const double* cj = cs + j * 17;
      const double s = np_sqdist([&](int f) { return x[f]; }, [&](int f) { return cj[f]; }, D);
      // sqrt is monotone: a root can only undercut the best root when s < sb,
      // and then the roots decide (strict: first index on ties of the roots)
      if (s < sb) {
        const double r2 = sqrt(s);
        sb = s;
        if (r2 < rb) {
          rb = r2;
          jmin = j;
        }
      }
    }
#pragma unroll
    for (int o = 2; o > 0; o >>= 1) {
      const double ro = __shfl_xor(rb, o, 4);
      const int jo = __shfl_xor(jmin, o, 4);
      if (ro < rb || (ro == rb && jo < jmin)) {
        rb = ro;
        jmin = jo;
      }
    }
    if (live && c4 == 0) {
      if (jmin >= a.k) jmin = 0;  // every root NaN: np.argmin of all-NaN is 0
      const int old = delta ? a.labels[pt] : -1;  // the screen left it untouched
      if (jmin != old) {
        a.labels[pt] = jmin;
        if (pre) {  // the tables hold xt = (x - mu) 2^sigma (exact)
#pragma unroll
          for (int f = 0; f < D; ++f) x[f] = (double)fmaf((float)x[f], a.sig, a.mu_s[f]);
        }
#pragma unroll
        for (int f = 0; f < D; ++f) atomicAdd(&tsum[f * KP + jmin], x[f]);
        atomicAdd(&tcnt[jmin], 1);
        if (old >= 0) {
#pragma unroll
          for (int f = 0; f < D; ++f) atomicAdd(&tsum[f * KP + old], -x[f]);
          atomicAdd(&tcnt[old], -1);
        }
      }
    }
  }
}

__device__ __forceinline__ void fallback_tail(const S32Args& a, const int32_t* region, int cnt,
                                           double* tsum, int* tcnt, const double* cs, int KP,
                                           bool delta, bool pre) {
  switch (a.d) {
#define CDR_FBT(D_) \
  case D_: fallback_points<D_>(a, region, cnt, tsum, tcnt, cs, KP, delta, pre); break;
    CDR_FBT(1) CDR_FBT(2) CDR_FBT(3) CDR_FBT(4) CDR_FBT(5) CDR_FBT(6) CDR_FBT(7) CDR_FBT(8)
    CDR_FBT(9) CDR_FBT(10) CDR_FBT(11) CDR_FBT(12) CDR_FBT(13) CDR_FBT(14) CDR_FBT(15)
    CDR_FBT(16)
#undef CDR_FBT
    default: break;
  }
}

// QH: feature quads per lane half (1: d <= 8, 2: d <= 16); MT: 32-centroid
// tiles (1: k <= 32, 2: k <= 64).
// FULLQ: all 2*QH quads of the lane halves exist in memory (d4 == 8 QH).
// LDS table: sums [8 QH][KP] (rows of missing quads stay 0) + counts [KP].
// DBG (tests only): the screen values go to a.dbg.
// PRE: a.X is the pre-centred copy xt = (x - mu) 2^sigma (exact, Ctx::pre_ok):
// the screen uses it as loaded and the tables sum xt (the tail restores x).
template <int QH, int MT, bool FULLQ, bool DBG, bool PRE>
__global__ __launch_bounds__(256) void screen32(S32Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KP = 32 * MT;
  constexpr int NF = 8 * QH;
  if (a.gate && a.gate[0] == 0) return;  // device loop stopped: uniform exit
  double* tsum = reinterpret_cast<double*>(smem);                      // [NF][KP]
  int* tcnt = reinterpret_cast<int*>(tsum + (size_t)NF * KP);          // [KP]
  double* cs = reinterpret_cast<double*>(tcnt + KP);                   // [k][17]
  for (int i = threadIdx.x; i < NF * KP; i += blockDim.x) tsum[i] = 0.0;
  for (int i = threadIdx.x; i < KP; i += blockDim.x) tcnt[i] = 0;
  for (int i = threadIdx.x; i < a.k * a.d; i += blockDim.x)
    cs[(i / a.d) * 17 + i % a.d] = a.cent[i];

  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int p = lane & 31;
  h8 A[MT][2];  // [0] = A1 (-2chi), [1] = A3 (-2clo)
  f16v Ci[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int u = 0; u < 2; ++u) A[m][u] = a.frag[(m * 2 + u) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 16; ++i) Ci[m][i] = a.cinit[(m * 16 + i) * 64 + lane];
  }
  // this lane's quads and centering constants
  int qd[QH];
  bool qok[QH];
  f4 ms[QH];
#pragma unroll
  for (int u = 0; u < QH; ++u) {
    qd[u] = QH * h + u;
    qok[u] = FULLQ || qd[u] < a.Q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 4 * qd[u] + i;
      ms[u][i] = f < a.d ? a.mu_s[f] : 0.0f;
    }
  }
  const float sig = a.sig, thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0, thr_rel = a.thr_rel;
  const f4* Xq = reinterpret_cast<const f4*>(a.X);
  const int wpb = blockDim.x >> 6;
  const int64_t ngroups = a.n_pad >> 6;
  const int64_t gstride = (int64_t)gridDim.x * wpb;
  int64_t G = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  const int wave_id = (int)G;
  int32_t* fb_region = a.fb_list + (size_t)wave_id * a.fb_cap;
  int fb_used = 0;
  __syncthreads();

  // running per-lane pointers of the next group to load (quad u), advanced
  // by one grid stride per prefetch
  const int64_t gstep = (int64_t)gridDim.x * wpb * 64;
  const f4* pq[QH];
#pragma unroll
  for (int u = 0; u < QH; ++u) pq[u] = Xq + (int64_t)qd[u] * a.n_pad + (G << 6) + p;
  auto load = [&](f4 (&buf)[2][QH]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < QH; ++u) {
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (FULLQ || qok[u]) v = pq[u][32 * t];  // tile t: immediate offset 512 B
        buf[t][u] = v;
      }
  };

  // screen values of one 32-point tile -> (best, runner-up) keys of this lane
  auto tile = [&](const f4 (&xq)[QH], unsigned& bk, unsigned& sk, int64_t tbase) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    u4v H, L;
#pragma unroll
    for (int u = 0; u < QH; ++u) {
      f4 xt;
      if constexpr (PRE) {
        xt = xq[u];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) xt[i] = fmaf(xq[u][i], sig, ms[u][i]);
      }
      unsigned h01, h23, l01, l23;
      split4(xt, h01, h23, l01, l23);
      if (QH == 1) {
        H = u4v{h01, h23, l01, l23};
      } else {
        H[2 * u] = h01;
        H[2 * u + 1] = h23;
        L[2 * u] = l01;
        L[2 * u + 1] = l23;
      }
    }
    const h8 BH = __builtin_bit_cast(h8, H);
    f16v acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[m][0], BH, Ci[m], 0, 0, 0);
      if constexpr (QH == 2) {
        const h8 BL = __builtin_bit_cast(h8, L);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[m][0], BL, acc[m], 0, 0, 0);
      }
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[m][1], BH, acc[m], 0, 0, 0);
    }
    if constexpr (DBG) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
          const int row = 32 * m + 8 * (i >> 2) + 4 * h + (i & 3);
          if (row < a.dbg_ld) a.dbg[(tbase + p) * a.dbg_ld + row] = acc[m][i];
        }
    }
    // keys: reg i of tile m is row 32m + 8(i/4) + 4h + (i%4); 4h is OR-ed later
    auto key = [&](int m, int i) {
      return (__float_as_uint(acc[m][i]) & ~63u) | (unsigned)(32 * m + 8 * (i >> 2) + (i & 3));
    };
    unsigned b, s;
    {
      const unsigned k0 = key(0, 0), k1 = key(0, 1);
      b = min(k0, k1);
      s = max(k0, k1);
    }
#pragma unroll
    for (int q = 2; q < 16 * MT; q += 2) {
      const unsigned x = key(q >> 4, q & 15), y = key(q >> 4, (q & 15) + 1);
      unsigned t;  // second smallest of {b, x, y}; then b = min of the three
      asm("v_med3_u32 %0, %1, %2, %3" : "=v"(t) : "v"(b), "v"(x), "v"(y));
      asm("v_min3_u32 %0, %1, %2, %3" : "=v"(b) : "v"(b), "v"(x), "v"(y));
      s = min(s, t);
    }
    bk = b | ((unsigned)h << 2);
    sk = s | ((unsigned)h << 2);
  };

  // one group of 64 points (the wave's registers xb)
  auto process = [&](const f4 (&xb)[2][QH], int64_t Gp) {
    const int64_t base = Gp << 6;
    if (base >= a.n) return;  // wave-uniform: padding groups have no real points
    unsigned bA, sA, bB, sB;
    tile(xb[0], bA, sA, base);
    tile(xb[1], bB, sB, base + 32);
    // lanes < 32: tile A's point l; lanes >= 32: tile B's point l - 32
    swap32(bA, bB);
    swap32(sA, sB);
    merge_top2(bA, sA, bB, sB);
    const int64_t pt = base + lane;
    const int label = (int)(bA & 63u);
    const float vb = __uint_as_float(bA & ~63u);
    const float vs = __uint_as_float(sA & ~63u);
    const bool cert = vs > fmaf(vb, thr_rel, thr0);  // NaN: never certified
    const bool real = pt < a.n;
    const bool put = cert && real;
    if (put) a.labels[pt] = label;
    const unsigned long long need = __ballot(real && !cert);
    if (need) {
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
      if (real && !cert) fb_region[fb_used + rank] = (int32_t)pt;
      fb_used += __popcll(need);
    }
    // verdicts of tile A / tile B point p to both lane halves
    unsigned vA = put ? (unsigned)label : 0xFFFFFFFFu;
    unsigned vB = vA;
    swap32(vA, vB);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int lp = (int)(t == 0 ? vA : vB);
      if (lp >= 0) {
        double* row = tsum + 4 * QH * h * KP + lp;  // feature 4 qd[0] of label lp
#pragma unroll
        for (int u = 0; u < QH; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i) atomicAdd(&row[(4 * u + i) * KP], (double)xb[t][u][i]);
      }
    }
    const int lc = (int)(h == 0 ? vA : vB);
    if (lc >= 0) atomicAdd(&tcnt[lc], 1);
  };
  auto prefetch = [&](f4 (&buf)[2][QH], int64_t Gp) {
    if (Gp < ngroups) load(buf);
#pragma unroll
    for (int u = 0; u < QH; ++u) pq[u] += gstep;
  };

#ifndef CDR_S32_DEPTH
#define CDR_S32_DEPTH 1
#endif
#if CDR_S32_DEPTH == 3
  // three register sets: loads run two groups ahead
  f4 x0[2][QH], x1[2][QH], x2[2][QH];
  prefetch(x0, G);
  prefetch(x1, G + gstride);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see below
  for (; G < ngroups; G += 3 * gstride) {
    prefetch(x2, G + 2 * gstride);
    process(x0, G);
    if (G + gstride >= ngroups) break;
    prefetch(x0, G + 3 * gstride);
    process(x1, G + gstride);
    if (G + 2 * gstride >= ngroups) break;
    prefetch(x1, G + 4 * gstride);
    process(x2, G + 2 * gstride);
  }
#elif CDR_S32_DEPTH == 2
  // two register sets used alternately (no copies between iterations)
  f4 xa[2][QH], xb2[2][QH];
  prefetch(xa, G);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see below
  for (; G < ngroups; G += 2 * gstride) {
    prefetch(xb2, G + gstride);
    process(xa, G);
    if (G + gstride >= ngroups) break;
    prefetch(xa, G + 2 * gstride);
    process(xb2, G + gstride);
  }
#else
  f4 cur[2][QH], nxt[2][QH];
  prefetch(cur, G);
  // drain before the loop, otherwise the waitcnt pass merges these loads into
  // the loop-header state and waits for the fresh prefetch in every iteration
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  for (; G < ngroups; G += gstride) {
    prefetch(nxt, G + gstride);
    process(cur, G);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < QH; ++u) cur[t][u] = nxt[t][u];
  }
#endif
  if (lane == 0) {
    a.fb_count[wave_id] = fb_used;
    if (fb_used) atomicAdd(a.fb_count + gstride, fb_used);
  }
  // (delta = false: the table receives every point, none leaves a cluster)
  if (fb_used) fallback_tail(a, fb_region, fb_used, tsum, tcnt, cs, KP, false, PRE);
  __syncthreads();
  // This workgroup's table as exact int64 fixed point, added into slice
  // (blockIdx % kRunSlices) of the running sums: sum x 2^S = sum xt 2^(S -
  // sigma) + count mu 2^S (PRE), both exact integers.  Lanes walk the (k,
  // d+1) output contiguously; zero contributions (clusters no point of this
  // workgroup entered or left) are skipped.
  {
    const int d1 = a.d + 1, cells = a.k * d1;
    unsigned long long* out = a.run_sums + (size_t)(blockIdx.x % kRunSlices) * cells;
    for (int e = threadIdx.x; e < cells; e += blockDim.x) {
      const int j = e / d1, r = e - j * d1;
      const int cnt = tcnt[j];
      long long v;
      if (r < a.d) {
        v = __double2ll_rn(tsum[r * KP + j] * a.fx);
        if (PRE) v += (long long)cnt * a.muf[r];
      } else {
        v = cnt;
      }
      if (v) atomicAdd(&out[e], (unsigned long long)v);
    }
  }
}

// (the occupancy of the product's common form: FULLQ, PRE)
int screen32_blocks_per_cu(int QH, int MT, size_t lds) {
  int nb = 0;
  dispatch_q_mt<2>(QH, MT, [&](auto q, auto m) {
    nb = occupancy_blocks(screen32<decltype(q)::value, decltype(m)::value, true, false, true>, lds);
  });
  return nb;
}

void screen32_launch(int QH, int MT, dim3 grid, hipStream_t s, size_t lds, const S32Args& a) {
  const bool fullq = a.Q == 2 * QH;
  dispatch_q_mt<2>(QH, MT, [&](auto q, auto m) {
    constexpr int QH_ = decltype(q)::value, MT_ = decltype(m)::value;
    auto pre = [&](auto p) {
      constexpr bool P_ = decltype(p)::value;
      // (the debug form takes the guarded loads: its shapes are tests')
      if (a.dbg) hipLaunchKernelGGL((screen32<QH_, MT_, false, true, P_>), grid, dim3(256), lds, s, a);
      else if (fullq) hipLaunchKernelGGL((screen32<QH_, MT_, true, false, P_>), grid, dim3(256), lds, s, a);
      else hipLaunchKernelGGL((screen32<QH_, MT_, false, false, P_>), grid, dim3(256), lds, s, a);
    };
    if (a.muf) pre(std::true_type{});
    else pre(std::false_type{});
  });
}

}  // namespace cdr
