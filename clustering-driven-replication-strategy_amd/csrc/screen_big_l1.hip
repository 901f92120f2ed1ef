// screen_big_l1.hip — level 1 of the large-k Lloyd step (screen_big.hip): the
// fp16 copy of the points in MFMA B-fragment order, and the software-pipelined
// MFMA screen over every point.
#include <cmath>
#include <cstdlib>

#include "screen_big.h"

namespace cdr {

namespace {

__device__ __forceinline__ void swap32(unsigned& x, unsigned& y) {
  auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}

// The L1 B fragments of every 64-point group, built once per point set from
// the pre-centred copy XT ([Q][n_pad][4] fp32): [g][t][c][lane] h8, lane
// (h, p) = features 16 c + 8 h .. + 8 of point 64 g + 32 t + p.  Half the
// bytes of the fp32 copy, and a wave's fragment loads are 1 KiB contiguous.
__global__ void big_frag_copy(const float* __restrict__ XT, int64_t n, int64_t n_pad, int Q,
                              int DQ, uint4* __restrict__ xb) {
  const f4* X4 = reinterpret_cast<const f4*>(XT);
  const int64_t total = (n_pad >> 6) * 2 * DQ * 64;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    const int64_t r = e >> 6;
    const int c = (int)(r % DQ);
    const int64_t gt = r / DQ;
    const int t = (int)(gt & 1);
    const int64_t g = gt >> 1;
    const int h = lane >> 5, p = lane & 31;
    const int64_t pt = g * 64 + 32 * t + p;
    const int q0 = 4 * c + 2 * h;
    f4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (pt < n && q0 < Q) v0 = X4[(int64_t)q0 * n_pad + pt];
    if (pt < n && q0 + 1 < Q) v1 = X4[(int64_t)(q0 + 1) * n_pad + pt];
    xb[e] = uint4{pack_h2(v0[0], v0[1]), pack_h2(v0[2], v0[3]), pack_h2(v1[0], v1[1]),
                  pack_h2(v1[2], v1[3])};
  }
}

// L1, software-pipelined.  Per 32-centroid block a wave issues the block's
// MFMAs into one accumulator pair while it reduces the previous block's
// values from the other pair, so its own VALU runs beside its matrix work
// (PMC of an unpipelined form: MFMA busy 0.45 + VALU 0.38 of the cycles, i.e.
// serialised).  Keys: the local top-2 keys value i as
// (bits & ~15) | i (inline constants); with the row order of big_row, i is
// centroid 32 b + 16 h + i, so the block merge is one v_and_or that writes
// (b, h) above i, and the running (best, runner-up) keys carry the centroid
// index in their low JB bits (no separate index or float compare).
// NT threads per workgroup (one workgroup per CU): 768 = 3 waves per SIMD
// (<= 168 VGPRs), 512 = 2 waves per SIMD (<= 256 VGPRs, no spills at DQ = 4)
template <int DQ, int NT>
__global__ __launch_bounds__(NT) void screen_big_sp(BigArgs a) {
  if (a.gate && a.gate[0] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0;
  const float thr_rel = a.thr_dev ? a.thr_dev[1] : a.thr_rel;
  float* scin = reinterpret_cast<float*>(smem);                     // [KB * 32]
  h8* sfrag = reinterpret_cast<h8*>(smem + (size_t)a.KB * 32 * 4);  // [KB][DQ][64]
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  const int p = lane & 31;
  for (int i = threadIdx.x; i < a.KB * 32; i += blockDim.x) scin[i] = a.cinit[i];
  {
    const int nf = a.KB * DQ * 64;
    for (int i = threadIdx.x; i < nf; i += blockDim.x) sfrag[i] = a.frag[i];
  }
  __syncthreads();
  const int wpb = blockDim.x >> 6;
  const int wave_id = blockIdx.x * wpb + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * wpb;
  int32_t* region = a.out_list + (size_t)wave_id * a.out_cap;
  float* region_best = a.out_best + (size_t)wave_id * a.out_cap;
  int used = 0;
  const h8* XB = a.XB;
  const unsigned jkeep = a.jkeep;
  const int KB = a.KB;
  const int64_t items = (a.n + 63) >> 6;
  // the group's B fragments: 2 DQ coalesced 16-byte loads per lane, the next
  // group's issued before this group's blocks (one group of prefetch)
  h8 BN[2][DQ];
  auto fetch = [&](int64_t gg) {
    if (gg < items) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < DQ; ++c) BN[t][c] = XB[((gg * 2 + t) * DQ + c) * 64 + lane];
    }
  };
  fetch(wave_id);
  int2* mv_region = a.delta ? a.mv1 + (size_t)wave_id * a.out_cap : nullptr;
  int mv_used = 0;
  for (int64_t g = wave_id; g < items; g += nwaves) {
    const int64_t base = g << 6;
    const int64_t pt[2] = {base + p, base + 32 + p};
    const bool real[2] = {pt[0] < a.n, pt[1] < a.n};
    // DELTA: the previous label of this lane's point (after the swap below:
    // lanes < 32 tile 0's point, lanes >= 32 tile 1's), loaded now
    const int64_t lpt = base + lane;
    const int oldl = a.delta && lpt < a.n ? a.labels[lpt] : -1;
    h8 BH[2][DQ];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < DQ; ++c) BH[t][c] = BN[t][c];
    fetch(g + nwaves);
    unsigned RB[2] = {~0u, ~0u}, RS[2] = {~0u, ~0u};
    // the block's MFMAs: C operand rows from LDS, A fragments from LDS
    auto mm = [&](int b, f16v (&acc)[2]) {
      const f4* cr = reinterpret_cast<const f4*>(scin + 32 * b + 4 * h);
      f16v ci;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 v = cr[2 * q];  // rows 8q + 4h .. + 4
#pragma unroll
        for (int i = 0; i < 4; ++i) ci[4 * q + i] = v[i];
      }
      h8 A[DQ];
#pragma unroll
      for (int c = 0; c < DQ; ++c) A[c] = sfrag[((size_t)b * DQ + c) * 64 + lane];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], BH[0][0], ci, 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], BH[1][0], ci, 0, 0, 0);
#pragma unroll
      for (int c = 1; c < DQ; ++c) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[c], BH[0][c], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[c], BH[1][c], acc[1], 0, 0, 0);
      }
    };
    // keyed top-2 of each tile's 16 values (all >= 0: bits order), merged
    // into the running keys with the block and lane half written above i
    auto red = [&](int b, const f16v (&acc)[2]) {
      const unsigned bo = ((unsigned)b << 5) | ((unsigned)h << 4);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        auto key = [&](int i) { return (__float_as_uint(acc[t][i]) & ~15u) | (unsigned)i; };
        unsigned kb = min(key(0), key(1)), ks = max(key(0), key(1));
#pragma unroll
        for (int i = 2; i < 16; i += 2) {
          const unsigned x = key(i), y = key(i + 1);
          unsigned m;
          asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(kb), "v"(x), "v"(y));
          asm("v_min3_u32 %0, %1, %2, %3" : "=v"(kb) : "v"(kb), "v"(x), "v"(y));
          ks = min(ks, m);
        }
        const unsigned kj = (kb & jkeep) | bo;
        unsigned ms;
        asm("v_min3_u32 %0, %1, %2, %3" : "=v"(ms) : "v"(max(RB[t], kj)), "v"(RS[t]), "v"(ks));
        RS[t] = ms;
        RB[t] = min(RB[t], kj);
      }
    };
    f16v accA[2], accB[2];
    mm(0, accA);
    int b = 1;
    for (; b + 1 < KB; b += 2) {
      mm(b, accB);
      red(b - 1, accA);
      mm(b + 1, accA);
      red(b, accB);
    }
    if (b < KB) {
      mm(b, accB);
      red(b - 1, accA);
      red(b, accB);
    } else {
      red(b - 1, accA);
    }
    // lanes < 32 end with tile 0's point p (both halves), lanes >= 32 with
    // tile 1's
    unsigned b0 = RB[0], b1 = RB[1], s0 = RS[0], s1 = RS[1];
    swap32(b0, b1);
    swap32(s0, s1);
    const unsigned kbest = min(b0, b1);
    unsigned krun;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(krun) : "v"(max(b0, b1)), "v"(s0), "v"(s1));
    const float best = __uint_as_float(kbest);
    const int label = (int)(kbest & ~jkeep) | (int)(kbest & 15u);
    const int64_t mypt = h == 0 ? pt[0] : pt[1];
    const bool myreal = h == 0 ? real[0] : real[1];
    // rows past k carry C = 1e30: never best, never a close runner-up
    const bool cert = __uint_as_float(krun) > fmaf(best, thr_rel, thr0);
    if (!a.delta) {
      if (myreal && cert) a.labels[mypt] = label;
    } else {
      const bool moved = myreal && cert && label != oldl;
      if (moved) a.labels[mypt] = label;
      const unsigned long long mvb = __ballot(moved);
      if (mvb) {
        const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(mvb >> 32),
                                                __builtin_amdgcn_mbcnt_lo((unsigned)mvb, 0u));
        if (moved) mv_region[mv_used + r] = int2{(int)mypt, (oldl << 16) | label};
        mv_used += __popcll(mvb);
      }
    }
    const unsigned long long need = __ballot(myreal && !cert);
    if (need) {
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
      if (myreal && !cert) {
        region[used + rank] = (int32_t)mypt;
        region_best[used + rank] = best;
      }
      used += __popcll(need);
    }
  }
  if (lane == 0) {
    a.out_count[wave_id] = used;
    if (used) atomicAdd(a.out_count + nwaves, used);
    if (a.delta) a.mv1_count[wave_id] = mv_used;
  }
}

}  // namespace

// L1 workgroup size: 3 waves per SIMD while the pipelined kernel fits 168
// VGPRs (DQ <= 2), else 2 (CDR_BIG_SP_NT=512|768 overrides, for comparisons)
int big_sp_threads(int DQ) {
  static const int env = exp_env("CDR_BIG_SP_NT") ? std::atoi(exp_env("CDR_BIG_SP_NT")) : 0;
  if (env == 512 || env == 768) return env;
  return DQ <= 2 ? 768 : 512;
}

const h8* big_ensure_xb(Ctx& c) {
  if (!c.xb_valid) {
    const int DQ = big_dq(c.d);
    c.xb16.ensure((size_t)(c.n_pad >> 6) * 2 * DQ * 64 * 16);
    hipLaunchKernelGGL(big_frag_copy, dim3(4096), dim3(256), 0, c.stream, c.xt32.as<float>(),
                       c.n, c.n_pad, d4_of(c.d) / 4, DQ, c.xb16.as<uint4>());
    HIP_CHECK(hipGetLastError());
    c.xb_valid = true;
  }
  return c.xb16.as<h8>();
}

void big_launch_l1(Ctx& c, const BigArgs& a, int nwg) {
  const int DQ = big_dq(a.d);
  // [DQ - 1][NT == 768]
  using Fn = void (*)(BigArgs);
#define CDR_BIG_SP(DQ_) {screen_big_sp<DQ_, 512>, screen_big_sp<DQ_, 768>}
  static const Fn fns[4][2] = {CDR_BIG_SP(1), CDR_BIG_SP(2), CDR_BIG_SP(3), CDR_BIG_SP(4)};
#undef CDR_BIG_SP
  static bool attr = false;
  if (!attr) {
    for (const auto& row : fns)
      for (const Fn f : row)
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  const int NT = big_sp_threads(DQ);
  hipLaunchKernelGGL(fns[DQ - 1][NT == 768], dim3(nwg), dim3(NT), big_l1_lds(a.k, a.d), c.stream,
                     a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace cdr
