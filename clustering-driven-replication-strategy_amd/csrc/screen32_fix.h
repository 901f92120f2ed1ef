// screen32_fix.h — the fixup fused into the tails of screen32p and screen32b
// (device code): one workgroup applies the move and fallback lists of its
// four waves to an LDS table and adds the table into the int64 running sums.
// Integer sums, so the result equals a full recompute.
//
// The hi-only certificate.  The drains of screen32p and screen32b screen
// h = fp16(xhat) alone (the hi-only screen copy: 32 bytes per point at d = 16,
// 16 at d <= 8) with two MFMAs per tile, A1 x H and A3 x H (d <= 8: one, H =
// [hi, hi] against [-2 chi, -2 clo]): the screen values are those of the point
// h, S_j = Shat_j +- E with Shat_j = D + ||chat_j||^2 - 2 chat_j.h (E: the
// plan's bound, thr0 >= 2E + the reference slack).  The true decision values
// T_j = ||chat_j||^2 - 2 chat_j.xhat differ by 2 (chat_j - chat_b).delta,
// delta = h - xhat, |delta| <= dn = 2^-11 (1 + 2^-9) ||h|| + 2^-23 (fp16 round
// to nearest, subnormals), and |chat_j - chat_b| <= sqrt(G_j) + sqrt(G_b) with
// G_j = ||h - chat_j||^2 <= S_j + E - D + ||h||^2.  A point is certified when
//     v_s > v_b (1 + 2^-16) + thr0 + 2 dn (sqrt(G_s) + sqrt(G_b))
// (v: the truncated keys, S_b <= v_b (1 + 2^-17), S_j >= v_s for every j != b).
// Then sqrt(G_s) > 2 dn, so S - 2 dn sqrt(S + E - D + ||h||^2) grows with S
// above v_s and the bound holds for every j != b: T_j - T_b > slack.  The
// points it does not certify go to the wave's fallback list, and
// fixup_regions below screens them again with both halves (hi and lo, split
// from the fp32 row as the screen copy was) before the exact fp64 decision.
#pragma once
#include "screen32_common.h"

namespace cdr {

constexpr int kFixMaxR = 16;  // list regions per workgroup the LDS layout has room for

template <int Q>
struct FixDims {
  static constexpr int QH = Q <= 2 ? 1 : 2;  // quads per lane half of the split screen
  static constexpr int DM = 4 * Q;           // features a point row holds (d <= DM)
};
constexpr int kFixTS = 65;  // table row stride
// LDS of one fixup workgroup: tsum [16][kFixTS] | cs [64][17] (fp64) | tcnt [64] |
// s_mv, s_fb [kFixMaxR + 1]
constexpr size_t kFixLdsBytes =
    sizeof(double) * (16 * kFixTS + 64 * 17) + sizeof(int) * (64 + 2 * (kFixMaxR + 1));
struct FixLds {
  double* tsum;
  double* cs;
  int* tcnt;
  int* s_mv;
  int* s_fb;
  __device__ explicit FixLds(unsigned char* base) {
    tsum = reinterpret_cast<double*>(base);
    cs = tsum + 16 * kFixTS;
    tcnt = reinterpret_cast<int*>(cs + 64 * 17);
    s_mv = tcnt + 64;
    s_fb = s_mv + kFixMaxR + 1;
  }
};

// np_sqdist (exact_math.h: NumPy's pairwise order of sum((x - c)^2)) for a
// runtime d <= 16 with every index a constant, so that x stays in registers:
// d < 8 sequential from 0.0; else 8 accumulators over the first 8 (d & ~7)
// features, the fixed tree, then the tail in order.
__device__ __forceinline__ double np_sqdist16(const float (&x)[16], const double* c, int d) {
  auto sq = [&](int f) {
    const double u = (double)x[f] - c[f];
    return u * u;
  };
  if (d < 8) {
    double res = 0.0;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (f < d) res = res + sq(f);
    return res;
  }
  double r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = sq(i);
  if (d >= 16) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = r[i] + sq(8 + i);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  const int dd = d - (d & 7);
#pragma unroll
  for (int f = 8; f < 16; ++f)
    if (f >= dd && f < d) res = res + sq(f);
  return res;
}

// Plan operands of the re-screen: the screen's LDS copies (sA [MT][2][64] h8,
// sC [MT][4][2][4] f32), or null for the plan in global memory.
struct FixPlan {
  const h8* sA;
  const float* sC;
};

// The lists of screen waves r0 .. r0 + FR - 1 applied by one workgroup to an
// LDS table (rows padded to 65: the lanes of one point hit different banks),
// then to slice `slice` of the running sums.  The caller has put the regions'
// counts in s_mv[1 .. FR] / s_fb[1 .. FR]; every thread calls it.  Q: feature
// quads of a point row (d <= 4 Q; d itself is a runtime value).
// * Moves, 4 lanes per point (lane q: feature quad q): +x into the new
//   cluster, -x out of the old one.
// * Uncertified points, 64 per wave: the split screen (hi and lo halves) is
//   computed for them (the step's plan), and every centroid
//   whose key is within the certification threshold of the best key is a
//   candidate (|S_j - T_j| <= E for all j: the reference's argmin is among
//   them; a point is certified exactly when the best is the only one).  The
//   lane owning the point evaluates its candidates in index order in exact fp64
//   NumPy order with a correctly rounded sqrt: np.argmin of np.linalg.norm,
//   first index on ties (src/kmeans_plusplus.py:33-34).
template <int Q, int MT>
__device__ __forceinline__ void fixup_regions(const FixArgs& a, int r0, int FR, int slice,
                                              const FixLds& L, FixPlan P = FixPlan{nullptr, nullptr}) {
  constexpr int CS = 17;
  constexpr int TS = kFixTS;
  constexpr int QH = FixDims<Q>::QH;
  constexpr int DM = FixDims<Q>::DM;
  double* tsum = L.tsum;
  double* cs = L.cs;
  int* tcnt = L.tcnt;
  int* s_mv = L.s_mv;
  int* s_fb = L.s_fb;
  const int k = a.k, d = a.d;
  // the step's centroids (fp64), loaded by every thread at once
#pragma unroll 4
  for (int i = threadIdx.x; i < k * d; i += blockDim.x) {
    const double v = a.cent[i];
    cs[(i / d) * CS + i % d] = v;
  }
  for (int i = threadIdx.x; i < DM * TS; i += blockDim.x) tsum[i] = 0.0;
  for (int i = threadIdx.x; i < 64; i += blockDim.x) tcnt[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    s_mv[0] = s_fb[0] = 0;
    for (int r = 1; r <= FR; ++r) {
      s_mv[r] += s_mv[r - 1];
      s_fb[r] += s_fb[r - 1];
    }
  }
  __syncthreads();
  const int nmv = s_mv[FR], nfb = s_fb[FR];
  if (nmv == 0 && nfb == 0) return;  // uniform: nothing changes here
  const f4* XA4 = reinterpret_cast<const f4*>(a.XA);  // point i: XA4[i * Q + q]
  auto region_of = [&](const int* pre, int e, int& r, int& i) {
    r = 0;
    while (r < FR - 1 && e >= pre[r + 1]) ++r;
    i = e - pre[r];
  };
  const int g = threadIdx.x >> 2, q4 = threadIdx.x & 3;
  // moved points: 64 per pass, lane q4 adds feature quad q4
  for (int e0 = 0; e0 < ((a.abl & 1) ? 0 : nmv); e0 += 64) {
    const int e = e0 + g;
    if (e < nmv && q4 < Q) {
      int r, i;
      region_of(s_mv, e, r, i);
      const int2 rec = a.mv_list[(size_t)(r0 + r) * a.cap + i];
      const f4 xq = XA4[(int64_t)rec.x * Q + q4];
      const int to = rec.y >> 16, from = rec.y & 0xFFFF;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int f = 4 * q4 + c;
        if (f < d) {
          atomicAdd(&tsum[f * TS + to], (double)xq[c]);
          atomicAdd(&tsum[f * TS + from], -(double)xq[c]);
        }
      }
      if (q4 == 0) {
        atomicAdd(&tcnt[to], 1);
        atomicAdd(&tcnt[from], -1);
      }
    }
  }
  if (nfb && !(a.abl & 2)) {
    constexpr int kTile = 1024 * QH;
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int h = lane >> 5, p = lane & 31;
    // centroid tile m's screen values of B (one tile's accumulator live at a
    // time: this body also runs in screen32p's tail, beside its registers)
    auto screen_m = [&](int m, const u4v (&vt)[QH]) -> f16v {
      const h8 A0 = P.sA ? P.sA[(m * 2 + 0) * 64 + lane] : a.frag[(m * 2 + 0) * 64 + lane];
      const h8 A1 = P.sA ? P.sA[(m * 2 + 1) * 64 + lane] : a.frag[(m * 2 + 1) * 64 + lane];
      f16v acc;
      if (P.sC) {
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
          const f4 c4v = *reinterpret_cast<const f4*>(P.sC + ((m * 4 + i4) * 2 + h) * 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[4 * i4 + i] = c4v[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = a.cinit[(m * 16 + i) * 64 + lane];
      }
      const h8 BH = __builtin_bit_cast(h8, vt[0]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, BH, acc, 0, 0, 0);
      if constexpr (QH == 2) {
        const h8 BL = __builtin_bit_cast(h8, vt[QH - 1]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, BL, acc, 0, 0, 0);
      }
      return __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, BH, acc, 0, 0, 0);
    };
    const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0, thr_rel = a.thr_rel;
    auto rec_of = [&](int e) -> int2 {
      int r, i;
      region_of(s_fb, e, r, i);
      return a.fb_list[(size_t)(r0 + r) * a.cap + i];
    };
    for (int e0 = wv * 64; e0 < nfb; e0 += blockDim.x) {
      // tile t holds list entries e0 + 32 t .. + 31; lane (h, p) the B
      // operand of entry e0 + 32 t + p (its half h), as the screen copy's tiles hold it
      int32_t ptt[2], oldt[2];
      u4v v[2][QH];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = e0 + 32 * t + p;
        const int2 rec = e < nfb ? rec_of(e) : int2{-1, 0};
        ptt[t] = rec.x;
        oldt[t] = rec.y;
        const int32_t q = ptt[t] < 0 ? 0 : ptt[t];
        if (a.ho) {  // QH quads of half h, split as split_copy_kernel does
          unsigned hw[4], lw[4];
#pragma unroll
          for (int u = 0; u < QH; ++u) {
            const int qq = QH * h + u;
            const f4 xr = qq < Q ? XA4[(int64_t)q * Q + qq] : f4{0.f, 0.f, 0.f, 0.f};
            f4 xt;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int f = 4 * qq + c;
              xt[c] = f < d ? fmaf(xr[c], a.sig, a.ms[f]) : 0.0f;
            }
            split4(xt, hw[2 * u], hw[2 * u + 1], lw[2 * u], lw[2 * u + 1]);
          }
          if constexpr (QH == 1) {
            v[t][0] = u4v{hw[0], hw[1], lw[0], lw[1]};
          } else {
            v[t][0] = u4v{hw[0], hw[1], hw[2], hw[3]};
            v[t][QH - 1] = u4v{lw[0], lw[1], lw[2], lw[3]};
          }
        } else {
          const unsigned char* src =
              a.XS + (size_t)(q >> 5) * kTile + (h * 32 + (q & 31)) * 16 * QH;
#pragma unroll
          for (int u = 0; u < QH; ++u) v[t][u] = *reinterpret_cast<const u4v*>(src + 16 * u);
        }
      }
      // this lane's point after the half swap: entry e0 + lane (tile lane >> 5)
      const int own = h ? ptt[1] : ptt[0];  // lane (h, p) owns entry e0 + 32 h + p
      const int old = h ? oldt[1] : oldt[0];   // (selects: no indexed private arrays)
      const int e_own = e0 + lane;
      const bool live = e_own < nfb;
      f4 xq[Q];
      if (live) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
          xq[q] = (a.abl & 16) ? f4{0.f, 0.f, 0.f, 0.f} : XA4[(int64_t)own * Q + q];
      }
      // screen values and candidate masks per tile: bit 16 m + i of a lane's
      // mask = value i of centroid tile m in its half (row 32 m + 8 (i / 4) +
      // 4 h + i % 4); immediates only, so nothing is hoisted into registers
      unsigned mine[2], other[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        // best key of the point over both halves (the screens' keys)
        unsigned bk = 0xFFFFFFFFu;
#pragma nounroll
        for (int m = 0; m < MT; ++m) {
          const f16v acc = screen_m(m, v[t]);
          const unsigned rb = 32u * (unsigned)m;
#pragma unroll
          for (int i = 0; i < 16; ++i)
            bk = min(bk, (__float_as_uint(acc[i]) & ~63u) | (rb + (unsigned)(8 * (i >> 2) + (i & 3))));
        }
        bk |= (unsigned)h << 2;
        bk = min(bk, (unsigned)__shfl_xor((int)bk, 32));
        const float tau = fmaf(__uint_as_float(bk & ~63u), thr_rel, thr0);
        unsigned cm = 0;
#pragma nounroll
        for (int m = 0; m < MT; ++m) {  // the same values again (recomputed, bit-identical)
          const f16v acc = screen_m(m, v[t]);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            // not excluded: key value <= tau (NaN: a candidate)
            const float kv = __uint_as_float(__float_as_uint(acc[i]) & ~63u);
            if (!(kv > tau)) cm |= 1u << (16 * m + i);
          }
        }
        mine[t] = cm;
        other[t] = (unsigned)__shfl_xor((int)cm, 32);
      }
      // lane (h, p) owns tile h's point p: its rows of half h are in mine[h],
      // those of half 1 - h in other[h]; as a 64-bit row mask
      unsigned long long cand = 0;
      {
        const unsigned mh0 = h == 0 ? mine[0] : other[1], mh1 = h == 0 ? other[0] : mine[1];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          unsigned mm = hh ? mh1 : mh0;  // rows of half hh of tile h
          while (mm) {
            const int bb = __builtin_ctz(mm);
            mm &= mm - 1;
            const int m = bb >> 4, i = bb & 15;
            cand |= 1ull << (32 * m + 8 * (i >> 2) + 4 * hh + (i & 3));
          }
        }
        if (k < 64) cand &= (1ull << k) - 1;
      }
      if (live) {
        float x[16];  // (fp32 data: converted exactly where used)
#pragma unroll
        for (int f = 0; f < 16; ++f) x[f] = f < DM ? xq[f >> 2][f & 3] : 0.0f;
        double sb = INFINITY, rb = INFINITY;
        int jmin = 0x7fffffff;
        unsigned long long cmk = (a.abl & 8) ? (cand & (~cand + 1)) : cand;
        while (cmk) {  // increasing j
          const int j = __builtin_ctzll(cmk);
          cmk &= cmk - 1;
          const double sq = np_sqdist16(x, cs + j * CS, d);
          if (sq < sb) {  // sqrt is monotone: only a smaller square can give a smaller root
            const double rt = sqrt(sq);
            sb = sq;
            if (rt < rb) {
              rb = rt;
              jmin = j;
            }
          }
        }
        if (jmin >= k) jmin = 0;  // every root NaN: np.argmin of all-NaN is 0
        if (jmin != old && !(a.abl & 32)) {
          a.labels[own] = jmin;
          a.lab8[own] = (uint8_t)jmin;
          if (a.zb) a.zb[own] = kZbStale | (unsigned)jmin;  // (screen32b: bound unknown)
#pragma unroll
          for (int f = 0; f < DM; ++f) {
            if (f < d) {
              atomicAdd(&tsum[f * TS + jmin], (double)x[f]);
              atomicAdd(&tsum[f * TS + old], -(double)x[f]);
            }
          }
          atomicAdd(&tcnt[jmin], 1);
          atomicAdd(&tcnt[old], -1);
        }
      }
    }
  }
  __syncthreads();
  if (a.abl & 4) return;
  const int d1 = d + 1, cells = k * d1;
  unsigned long long* out = a.run_sums + (size_t)slice * cells;
  for (int e = threadIdx.x; e < cells; e += blockDim.x) {
    const int j = e / d1, r = e - j * d1;
    const long long v = r < d ? __double2ll_rn(tsum[r * TS + j] * a.fx) : (long long)tcnt[j];
    if (v) atomicAdd(&out[e], (unsigned long long)v);
  }
}

}  // namespace cdr
