// screen_big_l2.hip — levels 2 and 3 of the large-k Lloyd step
// (screen_big.hip): the candidates of the points L1 could not certify, and the
// exact assignment of the points with too many candidates.
#include <cmath>

#include "exact_math.h"
#include "screen_big.h"

namespace cdr {

namespace {

// L2: the points L1 could not certify, 64 per wave (chunks of L1's regions).
// The one-product screen is recomputed (bit-identical to L1's: same
// fragments, same B operands from the fp16 copy) and every
// centroid with S_j <= best_L1 thr_rel + T1 is a candidate: the exact
// argmin is among them (|S_j - T_j| <= E for every j, T1 >= 2E + the
// reference's rounding slack).  Candidates go to a per-point LDS list; then
// each lane takes one point and evaluates its candidates in exact fp64 NumPy
// order (np_sqdist, correctly rounded sqrt, first minimum by (root, index)).
// A point with more than kMaxCand candidates goes to the flat overflow list
// for exact_big (all k centroids).
// np_sqdist (exact_math.h) for d >= 8 with the point's features in
// registers (DMAX >= d, a compile-time bound so every index is static)
template <int DMAX>
__device__ __forceinline__ double np_sqdist_reg(const float (&x)[DMAX],
                                                const double* __restrict__ cj, int d) {
  double r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double t = (double)x[i] - cj[i];
    r[i] = t * t;
  }
  const int dd = d - (d & 7);
#pragma unroll
  for (int f = 8; f < DMAX; f += 8) {
    if (f < dd) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double t = (double)x[f + i] - cj[f + i];
        r[i] = r[i] + t * t;
      }
    }
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
  for (int f = 8; f < DMAX; ++f) {
    if (f >= dd && f < d) {
      const double t = (double)x[f] - cj[f];
      res = res + t * t;
    }
  }
  return res;
}

// L2 with the A fragments read from global memory per chunk (7x L1's cost
// per point): the form for the largest KB, where the fragments and the
// candidate lists do not fit the LDS together (big_launch_l2_l3).  256
// threads, the chunk numbering of L1's regions in LDS.
template <int DQ>
__global__ __launch_bounds__(256) void cand_big(BigArgs a, const double* __restrict__ C64,
                                                int32_t* __restrict__ ovf,
                                                int32_t* __restrict__ ovf_count) {
  if (a.gate && a.gate[0] == 0) return;
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0;
  const float thr_rel = a.thr_dev ? a.thr_dev[1] : a.thr_rel;
  __shared__ int scnt[4][64];
  __shared__ int scand[4][64 * kMaxCand];
  __shared__ int schunk[kMaxRegions + 1];  // exclusive prefix of 64-point chunks per region
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int h = lane >> 5;
  const int p = lane & 31;
  const int wave_id = blockIdx.x * 4 + w;
  const int nwaves = gridDim.x * 4;
  // chunk numbering: region r owns chunks [schunk[r], schunk[r + 1])
  const int R = a.in_regions;
  for (int r = threadIdx.x; r < R; r += blockDim.x) schunk[r + 1] = (a.in_count[r] + 63) >> 6;
  if (threadIdx.x == 0) schunk[0] = 0;
  __syncthreads();
  if (w == 0) {  // one wave scans: lane l sums a contiguous slice, then a wave scan
    const int per = (R + 63) / 64;
    const int lo = 1 + lane * per, hi = min(R + 1, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += schunk[i];
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    int run = incl - sum;
    for (int i = lo; i < hi; ++i) {
      run += schunk[i];
      schunk[i] = run;
    }
  }
  __syncthreads();
  const int nchunks = schunk[R];
  for (int ch = wave_id; ch < nchunks; ch += nwaves) {
    int lo = 0, hi = R;  // last r with schunk[r] <= ch
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (schunk[mid] <= ch) lo = mid; else hi = mid;
    }
    const int r = lo;
    const int cnt = a.in_count[r];
    const int e0 = (ch - schunk[r]) * 64;
    const int32_t* src = a.in_list + (size_t)r * a.in_cap;
    const float* srcb = a.out_best + (size_t)r * a.in_cap;
    {
      int64_t pt[2];
      bool real[2];
      float lim[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = e0 + 32 * t + p;
        real[t] = e < cnt;
        pt[t] = real[t] ? (int64_t)src[e] : 0;
        lim[t] = real[t] ? fmaf(srcb[e], thr_rel, thr0) : -1.0f;
      }
      scnt[w][lane] = 0;
      h8 BH[2][DQ];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < DQ; ++c) {
          // the point's fragment in its group's block of the fp16 copy (one
          // 8 KB block per point)
          const int64_t q = pt[t];
          const int64_t idx = (((q >> 6) * 2 + ((q >> 5) & 1)) * DQ + c) * 64 + h * 32 + (q & 31);
          BH[t][c] = real[t] ? a.XB[idx] : h8{};
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int b = 0; b < a.KB; ++b) {
        f16v acc[2];
        {
          const f4* cr = reinterpret_cast<const f4*>(a.cinit + 32 * b + 4 * h);
          f16v ci;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f4 v = cr[2 * q];
#pragma unroll
            for (int i = 0; i < 4; ++i) ci[4 * q + i] = v[i];
          }
          acc[0] = ci;
          acc[1] = ci;
        }
#pragma unroll
        for (int c = 0; c < DQ; ++c) {
          const h8 A1 = a.frag[((size_t)b * DQ + c) * 64 + lane];
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, BH[0][c], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, BH[1][c], acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (acc[t][i] <= lim[t]) {
              const int j = 32 * b + 16 * h + i;
              const int slot = atomicAdd(&scnt[w][32 * t + p], 1);
              if (slot < kMaxCand) scand[w][(32 * t + p) * kMaxCand + slot] = j;
            }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // lane l: point l of the chunk (tile l / 32, column l % 32)
      const int e = e0 + lane;
      if (e < cnt) {
        const int64_t mypt = (int64_t)src[e];
        const int nc = scnt[w][lane];
        if (nc > kMaxCand || nc == 0) {
          ovf[atomicAdd(ovf_count, 1)] = (int32_t)mypt;
        } else {
          // the point's features once (one batch of quad loads), then each
          // candidate's fp64 row (L2-resident) in NumPy's pairwise order
          float xv[16 * DQ];
          const f4* XA4 = reinterpret_cast<const f4*>(a.XA);
#pragma unroll
          for (int q = 0; q < 4 * DQ; ++q) {
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < a.Q) v = XA4[mypt * a.Q + q];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[4 * q + i] = v[i];
          }
          double rb = INFINITY;
          int jb = 0x7fffffff;
          for (int s2 = 0; s2 < nc; ++s2) {
            const int j = scand[w][lane * kMaxCand + s2];
            const double R = np_sqdist_reg<16 * DQ>(xv, C64 + (size_t)j * a.d, a.d);
            const double root = sqrt(R);
            if (root < rb || (root == rb && j < jb)) {
              rb = root;
              jb = j;
            }
          }
          if (!a.delta) {
            a.labels[mypt] = jb;
          } else {
            const int oldl = a.labels[mypt];
            if (jb != oldl) {
              a.labels[mypt] = jb;
              a.mv2[atomicAdd(a.mv2_count, 1)] = int2{(int)mypt, (oldl << 16) | jb};
            }
          }
        }
      }
    }
  }
}

// The chunk numbering of L1's regions for cand_big_lds, in global memory (its
// LDS holds the fragments): pre[r] = 64-point chunks before region r,
// pre[R] = all.
__global__ __launch_bounds__(1024) void big_chunk_prefix(const int32_t* __restrict__ cnt, int R,
                                                         int32_t* __restrict__ pre) {
  __shared__ int wsum[16];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r0 = 0; r0 < R; r0 += 1024) {
    const int r = r0 + threadIdx.x;
    const int v = r < R ? (cnt[r] + 63) >> 6 : 0;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int base = carry;
    for (int q = 0; q < w; ++q) base += wsum[q];
    if (r < R) pre[r] = base + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = base + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) pre[R] = carry;
}

// L2 with the A fragments and C rows in LDS: the form while the fragments
// and its candidate lists fit 160 KiB of LDS (L1's lds1 <= 145,408 B).  Above
// that, up to big_supported's 150 KiB, the step runs cand_big: a product path
// too, e.g. d = 64, k = 1100 (KB 35..36 at DQ 4, 46..48 at DQ 3, 67..70 at
// DQ 2, 127..133 at DQ 1).  One NT-thread workgroup per CU; the chunk
// numbering of L1's regions comes from big_chunk_prefix.  Per chunk of 64
// points: the same one-product screen as L1, pipelined as L1's, candidates
// S_j <= best thr_rel + T1 into per-point LDS lists (u16), then the exact
// fp64 evaluation of each point's candidates as cand_big.
template <int DQ, int NT>
__global__ __launch_bounds__(NT) void cand_big_lds(BigArgs a, const double* __restrict__ C64,
                                                   const int32_t* __restrict__ chunk_pre,
                                                   int32_t* __restrict__ ovf,
                                                   int32_t* __restrict__ ovf_count) {
  if (a.gate && a.gate[0] == 0) return;
  constexpr int NW = NT / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* scin = reinterpret_cast<float*>(smem);                     // [KB * 32]
  h8* sfrag = reinterpret_cast<h8*>(smem + (size_t)a.KB * 32 * 4);  // [KB][DQ][64]
  int* scnt = reinterpret_cast<int*>(sfrag + (size_t)a.KB * DQ * 64);  // [NW][64]
  unsigned short* scand = reinterpret_cast<unsigned short*>(scnt + NW * 64);  // [NW][64][kMaxCand]
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0;
  const float thr_rel = a.thr_dev ? a.thr_dev[1] : a.thr_rel;
  const int R = a.in_regions;
  const int nchunks = chunk_pre[R];
  if (nchunks == 0) return;  // uniform over the grid
  for (int i = threadIdx.x; i < a.KB * 32; i += blockDim.x) scin[i] = a.cinit[i];
  for (int i = threadIdx.x; i < a.KB * DQ * 64; i += blockDim.x) sfrag[i] = a.frag[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int h = lane >> 5;
  const int p = lane & 31;
  const int wave_id = blockIdx.x * NW + w;
  const int nwaves = gridDim.x * NW;
  int* mycnt = scnt + w * 64;
  unsigned short* mycand = scand + (size_t)w * 64 * kMaxCand;
  const f4* XA4 = reinterpret_cast<const f4*>(a.XA);
  for (int ch = wave_id; ch < nchunks; ch += nwaves) {
    int lo = 0, hi = R;  // last r with chunk_pre[r] <= ch
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (chunk_pre[mid] <= ch) lo = mid; else hi = mid;
    }
    const int r = lo;
    const int cnt = a.in_count[r];
    const int e0 = (ch - chunk_pre[r]) * 64;
    const int32_t* src = a.in_list + (size_t)r * a.in_cap;
    const float* srcb = a.out_best + (size_t)r * a.in_cap;
    int64_t pt[2];
    bool real[2];
    float lim[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = e0 + 32 * t + p;
      real[t] = e < cnt;
      pt[t] = real[t] ? (int64_t)src[e] : 0;
      lim[t] = real[t] ? fmaf(srcb[e], thr_rel, thr0) : -1.0f;
    }
    mycnt[lane] = 0;
    h8 BH[2][DQ];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < DQ; ++c) {
        const int64_t q = pt[t];
        const int64_t idx = (((q >> 6) * 2 + ((q >> 5) & 1)) * DQ + c) * 64 + h * 32 + (q & 31);
        BH[t][c] = real[t] ? a.XB[idx] : h8{};
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    auto mm = [&](int b, f16v (&acc)[2]) {
      const f4* cr = reinterpret_cast<const f4*>(scin + 32 * b + 4 * h);
      f16v ci;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 v = cr[2 * q];
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
    auto take = [&](int b, const f16v (&acc)[2]) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (acc[t][i] <= lim[t]) {
            const int slot = atomicAdd(&mycnt[32 * t + p], 1);
            if (slot < kMaxCand)
              mycand[(32 * t + p) * kMaxCand + slot] = (unsigned short)(32 * b + 16 * h + i);
          }
    };
    f16v accA[2], accB[2];
    mm(0, accA);
    int b = 1;
    for (; b + 1 < a.KB; b += 2) {
      mm(b, accB);
      take(b - 1, accA);
      mm(b + 1, accA);
      take(b, accB);
    }
    if (b < a.KB) {
      mm(b, accB);
      take(b - 1, accA);
      take(b, accB);
    } else {
      take(b - 1, accA);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // lane l: point l of the chunk (tile l / 32, column l % 32)
    const int e = e0 + lane;
    if (e < cnt) {
      const int64_t mypt = (int64_t)src[e];
      const int nc = mycnt[lane];
      if (nc > kMaxCand || nc == 0) {
        ovf[atomicAdd(ovf_count, 1)] = (int32_t)mypt;
      } else {
        float xv[16 * DQ];
#pragma unroll
        for (int q = 0; q < 4 * DQ; ++q) {
          const f4 v = q < a.Q ? XA4[mypt * a.Q + q] : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < 4; ++i) xv[4 * q + i] = v[i];
        }
        double rb = INFINITY;
        int jb = 0x7fffffff;
        for (int s2 = 0; s2 < nc; ++s2) {
          const int j = mycand[lane * kMaxCand + s2];
          const double Rd = np_sqdist_reg<16 * DQ>(xv, C64 + (size_t)j * a.d, a.d);
          const double root = sqrt(Rd);
          if (root < rb || (root == rb && j < jb)) {
            rb = root;
            jb = j;
          }
        }
        if (!a.delta) {
          a.labels[mypt] = jb;
        } else {
          const int oldl = a.labels[mypt];
          if (jb != oldl) {
            a.labels[mypt] = jb;
            a.mv2[atomicAdd(a.mv2_count, 1)] = int2{(int)mypt, (oldl << 16) | jb};
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// L3: exact fp64 assignment of the overflow list (flat, count at *count):
// one wave per point.  Lane (c, r) = (lane >> 3, lane & 7) takes centroids
// c, c + 8, ... and NumPy's pairwise accumulator r (features r, r + 8, ...,
// summed sequentially), shfl_xor 1, 2, 4 combine ((r0+r1)+(r2+r3))+
// ((r4+r5)+(r6+r7)), the d % 8 tail is added in order; sqrt is correctly
// rounded; first minimum of the roots (src/kmeans_plusplus.py:33-34).
// d >= 8 here (the large regime); the point sits in LDS.
__global__ __launch_bounds__(64) void exact_big(const float* __restrict__ X, int64_t n_pad,
                                                int d, const double* __restrict__ C, int k,
                                                const int32_t* __restrict__ list,
                                                const int32_t* __restrict__ count,
                                                int32_t* __restrict__ labels,
                                                const long long* __restrict__ gate,
                                                int2* __restrict__ mv2,
                                                int32_t* __restrict__ mv2_count) {
  if (gate && gate[0] == 0) return;
  __shared__ double sx[128];
  const int lane = threadIdx.x;
  const int c8 = lane >> 3, r = lane & 7;
  const int dd = d - (d & 7);
  const int total = *count;
  for (int e = blockIdx.x; e < total; e += gridDim.x) {
    const int64_t pt = list[e];
    __syncthreads();
    for (int f = lane; f < d; f += 64) sx[f] = (double)X[xidx(X, f, pt, n_pad)];
    __syncthreads();
    double rb = INFINITY;
    int jmin = 0x7fffffff;
    for (int j0 = 0; j0 < k; j0 += 8) {
      const int j = j0 + c8;
      const double* cj = C + (size_t)(j < k ? j : 0) * d;
      double acc;
      {
        const double t = sx[r] - cj[r];
        acc = t * t;
      }
      for (int f = 8 + r; f < dd; f += 8) {
        const double t = sx[f] - cj[f];
        acc = acc + t * t;
      }
      acc = acc + __shfl_xor(acc, 1);
      acc = acc + __shfl_xor(acc, 2);
      acc = acc + __shfl_xor(acc, 4);
      for (int f = dd; f < d; ++f) {
        const double t = sx[f] - cj[f];
        acc = acc + t * t;
      }
      const double root = sqrt(acc);
      if (j < k && root < rb) {  // strict: first index on ties
        rb = root;
        jmin = j;
      }
    }
    for (int o = 8; o < 64; o <<= 1) {
      const double ro = __shfl_xor(rb, o);
      const int jo = __shfl_xor(jmin, o);
      if (ro < rb || (ro == rb && jo < jmin)) {
        rb = ro;
        jmin = jo;
      }
    }
    if (lane == 0) {
      const int jl = jmin < k ? jmin : 0;
      if (!mv2) {
        labels[pt] = jl;
      } else {  // DELTA step: record a change
        const int oldl = labels[pt];
        if (jl != oldl) {
          labels[pt] = jl;
          mv2[atomicAdd(mv2_count, 1)] = int2{(int)pt, (oldl << 16) | jl};
        }
      }
    }
  }
}

}  // namespace

void big_launch_l2_l3(Ctx& c, const BigArgs& a2, const double* dC, int32_t* ovf,
                      int32_t* ovf_count, int32_t* chunk_pre) {
  struct Fns {
    void (*lds)(BigArgs, const double*, const int32_t*, int32_t*, int32_t*);
    void (*global)(BigArgs, const double*, int32_t*, int32_t*);
  };
#define CDR_BIG_L2(DQ_) {cand_big_lds<DQ_, 512>, cand_big<DQ_>}
  static const Fns fns[4] = {CDR_BIG_L2(1), CDR_BIG_L2(2), CDR_BIG_L2(3), CDR_BIG_L2(4)};
#undef CDR_BIG_L2
  static bool attr = false;
  if (!attr) {
    for (const Fns& f : fns)
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(f.lds),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  const Fns& f = fns[big_dq(a2.d) - 1];
  const int cus = lloyd_num_cus(c.device);
  const size_t lds2 = big_l1_lds(a2.k, a2.d) + (size_t)8 * 64 * 4 + (size_t)8 * 64 * kMaxCand * 2;
  if (lds2 <= 160 * 1024) {
    // L2 on LDS-resident fragments: chunk numbering first (global), then
    // one workgroup per CU
    c.big_info[5] = 0;
    hipLaunchKernelGGL(big_chunk_prefix, dim3(1), dim3(1024), 0, c.stream, a2.in_count,
                       a2.in_regions, chunk_pre);
    hipLaunchKernelGGL(f.lds, dim3(cus), dim3(512), lds2, c.stream, a2, dC, chunk_pre, ovf,
                       ovf_count);
  } else {
    c.big_info[5] = 1;
    hipLaunchKernelGGL(f.global, dim3(cus * 2), dim3(256), 0, c.stream, a2, dC, ovf, ovf_count);
  }
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(exact_big, dim3(cus * 4), dim3(64), 0, c.stream, c.x32.as<float>(), c.n_pad,
                     a2.d, dC, a2.k, ovf, ovf_count, a2.labels, a2.gate, a2.mv2, a2.mv2_count);
  HIP_CHECK(hipGetLastError());
}

}  // namespace cdr
