// screen_fast.h — the medium screens' kernel arguments and screen_fast, the
// kernel of the shapes whose fragments stay in registers (screen_mid.hip
// launches it and holds the other kernels of the step).
#pragma once
#include "cdr_internal.h"

namespace cdr {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

struct ScreenArgs {
  const float* X;
  int64_t n, n_pad;
  int d, k, KT;
  const h8* frag;
  const float* mu_s;  // -mu_f * 2^sigma
  float sig;          // 2^sigma
  float fx;           // 2^S (fixed-point scale)
  float thrA0, thrA1;
  int32_t* labels;
  unsigned long long* partials;
  int32_t* fb_list;   // per-wave regions of fb_cap entries
  int32_t* fb_count;  // [waves] entries per region, [waves] = total
  int fb_cap;
  float* dbg;  // optional: screen values (n_pad x KT*16) for tests
  int ablate;  // timing experiments only (CDR_SCREEN_ABLATE): 1 no update,
               // 2 no argmin, 4 no MFMA, 8 no loads; results are garbage
};

// ---------------------------------------------------------------------------
// screen_fast: the k*d <= 64*16 regime (KT*DCH <= 4), the BASELINE configs.
// A fragments live in registers for the whole kernel; one wave processes a
// 64-point group per iteration as four 16-point tiles and prefetches the
// next group's quads while it computes.  Per tile and lane: one 16-byte load
// per 16 features, packed fp32->fp16 hi/lo split, 2*KT*DCH MFMAs whose first
// C operand is the point norm ||xhat||^2, 2.5 VALU ops per screen value for
// the running (best, runner-up) keys.  Per group: the four tiles' (best,
// runner-up) pairs are reduced across the lane groups by a 4x4 permlane
// transpose, after which lane group g owns tile g's points — one coalesced
// label store, one certification test, one fallback ballot — and the
// per-point verdicts are broadcast back for the LDS u64 adds (4 per 16
// features, +1 count) of the certified points.
// Fragment k-slot order (must match build_screen_plan):
//   B1 = [hi0..3, lo0..3]      B2 = [hi0..3, (g==1: 1, 1, 1, 0)]
//   A1 = [-2chi0..3, -2chi0..3]  A2 = [-2clo0..3, (g==1: cc parts p0, p1, p2, 0)]
// ---------------------------------------------------------------------------
typedef float f4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  h2v h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
  return max(min(a, b), min(max(a, b), c));  // v_med3_u32
}

// (best, runner-up) of two (best, runner-up) pairs
__device__ __forceinline__ void merge_top2(unsigned& b, unsigned& s, unsigned b2, unsigned s2) {
  const unsigned nb = min(b, b2);
  s = min(max(b, b2), min(s, s2));
  b = nb;
}

// Exchange halves between x and y: permlane32 pairs lane L < 32 with L + 32,
// permlane16 pairs row 2r with row 2r + 1 (rows of 16 lanes).
__device__ __forceinline__ void swap32(unsigned& x, unsigned& y) {
  auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}
__device__ __forceinline__ void swap16(unsigned& x, unsigned& y) {
  auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}

template <int DCH, int KT, bool NONNEG, bool FULL, int ABL = 0, int WAVES = 4>
__global__ __launch_bounds__(256, WAVES) void screen_fast(ScreenArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* tbl = reinterpret_cast<unsigned long long*>(smem);
  const int d = a.d;
  const int d4 = (d + 3) & ~3;
  const int KS = d4 + 1;  // table row: d4 sums (padding features add 0) + count
  for (int i = threadIdx.x; i < a.k * KS; i += blockDim.x) tbl[i] = 0ull;

  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int col = lane & 15;
  h8 A1[KT][DCH], A2[KT][DCH];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      A1[t][c] = a.frag[((t * DCH + c) * 2 + 0) * 64 + lane];
      A2[t][c] = a.frag[((t * DCH + c) * 2 + 1) * 64 + lane];
    }
  f4v ms[DCH];
  bool qok[DCH];
  const f4v* Xq = reinterpret_cast<const f4v*>(a.X);
#pragma unroll
  for (int c = 0; c < DCH; ++c) {
    const int f0 = 16 * c + 4 * g;
    qok[c] = FULL || f0 < d4;
#pragma unroll
    for (int i = 0; i < 4; ++i) ms[c][i] = (f0 + i < d) ? a.mu_s[f0 + i] : 0.0f;
  }
  // chunk-0 spare k-slots: lane group 1 holds the 1.0 multipliers of the
  // three fp16 parts of ||c_j||^2 + eps (constants, no per-tile work)
  const unsigned one01 = g == 1 ? pack_h2(1.0f, 1.0f) : 0u;
  const unsigned one2 = g == 1 ? pack_h2(1.0f, 0.0f) : 0u;
  const float sig = a.sig, fx = a.fx, thrA0 = a.thrA0, thrA1 = a.thrA1;
  const int wpb = blockDim.x >> 6;
  const int64_t ngroups = a.n_pad >> 6;
  const int64_t gstride = (int64_t)gridDim.x * wpb;
  int64_t G = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  const int wave_id = (int)G;
  int32_t* fb_region = a.fb_list + (size_t)wave_id * a.fb_cap;
  int fb_used = 0;
  constexpr int ablate = ABL;  // timing experiments only (separate instances)
  __syncthreads();

  auto load = [&](f4v (&buf)[4][DCH], int64_t grp) {
    if constexpr ((ablate & 8) != 0) {  // synthetic points, no HBM reads
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < DCH; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            buf[p][c][i] = (float)(((int)grp + 7 * p + 3 * i + col) & 255) * 0x1p-8f;
      return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        if (FULL) {
          buf[p][c] = Xq[(int64_t)(4 * c + g) * a.n_pad + (grp << 6) + 16 * p + col];
        } else {
          f4v v = {0.f, 0.f, 0.f, 0.f};
          if (qok[c]) v = Xq[(int64_t)(4 * c + g) * a.n_pad + (grp << 6) + 16 * p + col];
          buf[p][c] = v;
        }
      }
  };

  // B fragments + MFMAs of one 16-point tile; the point norm (summed over the
  // four lane groups) enters as the first MFMA's C operand.  Returns it.
  auto screen_tile = [&](const f4v (&xq)[DCH], f4 (&acc)[KT]) -> float {
    h8 b1[DCH], b2[DCH];
    float xxp = 0.0f;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      f4v xt;
#pragma unroll
      for (int i = 0; i < 4; ++i) xt[i] = fmaf(xq[c][i], sig, ms[c][i]);
      const unsigned h01 = pack_h2(xt[0], xt[1]), h23 = pack_h2(xt[2], xt[3]);
      const h2v hh01 = __builtin_bit_cast(h2v, h01), hh23 = __builtin_bit_cast(h2v, h23);
      // residual x - hi straight from the packed halves (v_fma_mix_f32)
      const unsigned l01 = pack_h2(fmaf((float)hh01[0], -1.0f, xt[0]),
                                   fmaf((float)hh01[1], -1.0f, xt[1]));
      const unsigned l23 = pack_h2(fmaf((float)hh23[0], -1.0f, xt[2]),
                                   fmaf((float)hh23[1], -1.0f, xt[3]));
      xxp = fmaf(xt[0], xt[0], xxp);
      xxp = fmaf(xt[1], xt[1], xxp);
      xxp = fmaf(xt[2], xt[2], xxp);
      xxp = fmaf(xt[3], xt[3], xxp);
      u4v w1 = {h01, h23, l01, l23};
      u4v w2 = {h01, h23, c == 0 ? one01 : 0u, c == 0 ? one2 : 0u};
      b1[c] = __builtin_bit_cast(h8, w1);
      b2[c] = __builtin_bit_cast(h8, w2);
    }
    {
      auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xxp), __float_as_uint(xxp),
                                                  false, false);
      xxp = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
      auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(xxp), __float_as_uint(xxp),
                                                  false, false);
      xxp = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      acc[t] = f4{xxp, xxp, xxp, xxp};
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1[t][c], b1[c], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A2[t][c], b2[c], acc[t], 0, 0, 0);
      }
    }
    return xxp;
  };

  // (best, runner-up) keys of the lane's 4*KT screen values: value bits with
  // the low 6 replaced by the row index 16t + r (the lane group's 4g is added
  // once per group); values taken in pairs, b = min3, s = min(s, med3)
  auto tile_top2 = [&](const f4 (&acc)[KT], unsigned& bk, unsigned& sk) {
    auto key = [&](int t, int r) {
      return (__float_as_uint(acc[t][r]) & ~63u) | (unsigned)(16 * t + r);
    };
    auto chain = [&](int t0, int t1, unsigned& b, unsigned& s) {
      const unsigned k0 = key(t0, 0), k1 = key(t0, 1);
      b = min(k0, k1);
      s = max(k0, k1);
#pragma unroll
      for (int q = 2; q < 4 * (t1 - t0); q += 2) {
        const unsigned x = key(t0 + q / 4, q & 3), y = key(t0 + q / 4, (q & 3) + 1);
        s = min(s, umed3(b, x, y));
        b = min(min(b, x), y);
      }
    };
    if constexpr (KT >= 2) {  // two independent chains, one merge
      unsigned b2, s2;
      chain(0, KT / 2, bk, sk);
      chain(KT / 2, KT, b2, s2);
      merge_top2(bk, sk, b2, s2);
    } else {
      chain(0, 1, bk, sk);
    }
  };

  auto process = [&](const f4v (&buf)[4][DCH], int64_t grp) {
    const int64_t base = grp << 6;
    if (base >= a.n) return;  // wave-uniform: padding group
    unsigned bk[4], sk[4];
    float xx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      f4 acc[KT];
      xx[p] = screen_tile(buf[p], acc);
      if constexpr ((ablate & 2) != 0) {  // no argmin / update
        float z = xx[p];
#pragma unroll
        for (int t = 0; t < KT; ++t) z += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
        asm volatile("" ::"v"(z));
      } else {
        tile_top2(acc, bk[p], sk[p]);
        bk[p] |= (unsigned)g << 2;
      }
    }
    if constexpr ((ablate & 2) != 0) return;
    // 4x4 transpose-reduce across lane groups: afterwards lane group g holds
    // the (best, runner-up) of tile g's point `col` (merges are symmetric,
    // so the swap orientation does not matter here)
    swap32(bk[0], bk[2]);
    swap32(sk[0], sk[2]);
    merge_top2(bk[0], sk[0], bk[2], sk[2]);
    swap32(bk[1], bk[3]);
    swap32(sk[1], sk[3]);
    merge_top2(bk[1], sk[1], bk[3], sk[3]);
    swap16(bk[0], bk[1]);
    swap16(sk[0], sk[1]);
    merge_top2(bk[0], sk[0], bk[1], sk[1]);
    const float xxg = g == 0 ? xx[0] : g == 1 ? xx[1] : g == 2 ? xx[2] : xx[3];
    const int64_t pt = base + 16 * g + col;  // < n_pad
    const int label = (int)(bk[0] & 63u);
    const float vb = __uint_as_float(bk[0] & ~63u);
    const float vs = __uint_as_float(sk[0] & ~63u);
    const bool cert = vs > fmaf(vb, 1.0f + 0x1p-15f, fmaf(thrA1, xxg, thrA0));
    a.labels[pt] = label;  // one coalesced 256-byte store per group
    const bool real = pt < a.n;
    const unsigned long long need = __ballot(real && !cert);
    if (need) {  // private region: no returning atomic, no vmcnt(0) stall
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
      if (real && !cert) fb_region[fb_used + rank] = (int32_t)pt;
      fb_used += __popcll(need);
    }
    if constexpr ((ablate & 1) != 0) return;  // no update
    // broadcast each tile's verdict (label, or -1) to all four lane groups
    unsigned v0 = (cert && real) ? (unsigned)label : 0xFFFFFFFFu;
    unsigned v1 = v0;
    swap16(v0, v1);  // rows (0,1): v0 = tile 0, v1 = tile 1; rows (2,3): tiles 2, 3
    unsigned v2 = v0, v3 = v1;
    swap32(v0, v2);  // v0 = tile 0, v2 = tile 2 in every lane
    swap32(v1, v3);  // v1 = tile 1, v3 = tile 3
    const unsigned vt[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int lp = (int)vt[p];
      if (lp >= 0) {
        unsigned long long* row = tbl + (size_t)lp * KS;
#pragma unroll
        for (int c = 0; c < DCH; ++c)
          if (qok[c]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int u = (int)(buf[p][c][i] * fx);
              const unsigned long long v =
                  NONNEG ? (unsigned long long)(unsigned)u : (unsigned long long)(long long)u;
              atomicAdd(&row[16 * c + 4 * g + i], v);
            }
          }
        if (g == 0) atomicAdd(&row[d4], 1ull);
      }
    }
  };

  // one group in flight ahead of the one being processed
  f4v cur[4][DCH], nxt[4][DCH];
  if (G < ngroups) load(cur, G);
  // drain before the loop: otherwise the waitcnt pass merges this load into
  // the loop header state and puts a vmcnt wait for the freshly issued
  // prefetch in front of every tile (vmcnt(0), lgkmcnt/expcnt untouched)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (; G < ngroups; G += gstride) {
    const int64_t Gn = G + gstride;
    if (Gn < ngroups) load(nxt, Gn);
    process(cur, G);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < DCH; ++c) cur[p][c] = nxt[p][c];
  }
  if (lane == 0) {
    a.fb_count[wave_id] = fb_used;
    if (fb_used) atomicAdd(a.fb_count + (int64_t)gstride, fb_used);
  }
  __syncthreads();
  unsigned long long* dst = a.partials + (size_t)blockIdx.x * a.k * KS;
  for (int i = threadIdx.x; i < a.k * KS; i += blockDim.x) dst[i] = tbl[i];
}

}  // namespace cdr
