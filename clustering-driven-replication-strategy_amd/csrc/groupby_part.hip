// groupby_part.hip — the group-by's partition of the resident events by file
// id (the method and the kernel list are at the head of groupby.hip): the
// histogram and scans of pass 1 (K1, S1), the scatters of passes 1..3 (P1,
// H2 / S2 / P2 and the same kernels again over pass 2's regions), and the
// producers' timestamp range.  What comes out is the packed payloads
// (groupby_pay.h) in bucket order and the bucket bases.
#include <algorithm>

#include "groupby.h"

namespace cdr {

namespace {

constexpr int kGbThreads = 512;                 // partition / histogram workgroups
constexpr int kGbPer = kGbTile / kGbThreads;    // events per thread in a tile
constexpr int kGbChunkTiles = 8;                // tiles per gb_hist1 workgroup
constexpr int kGbRange = 16;                    // chunks per gb_scan1a/c workgroup

// Exclusive scan of n <= 512 LDS counters by a 512-thread workgroup (one
// counter per thread).
__device__ __forceinline__ void lds_scan(const unsigned* cnt, unsigned* lp, int n,
                                         unsigned* wsum) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const unsigned v = t < n ? cnt[t] : 0u;
  unsigned inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned base = 0;
  for (int i = 0; i < w; ++i) base += wsum[i];
  if (t < n) lp[t] = base + inc - v;
  __syncthreads();
}

// ---- K1 --------------------------------------------------------------------
// TS = false: the producer already has the timestamp range (events_ts_range),
// only the file ids are read (4 B per event instead of 12).
template <bool TS>
__global__ __launch_bounds__(kGbThreads) void gb_hist1(
    const int32_t* __restrict__ file, const long long* __restrict__ ts, int64_t ne, int64_t nf,
    int shift1, int R1, unsigned* __restrict__ tilepref, unsigned* __restrict__ chunksum,
    long long* __restrict__ part) {
  __shared__ unsigned hist[kGbMaxBins];
  __shared__ long long red[3][kGbThreads / 64];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  unsigned run = 0;  // thread r owns digit r
  long long lo = LLONG_MAX, hi = LLONG_MIN;
  long long nul = 0;
  for (int tt = 0; tt < kGbChunkTiles; ++tt) {
    const int64_t t = c * kGbChunkTiles + tt;
    const int64_t base = t * kGbTile;
    if (base >= ne) break;
    if (tid < R1) hist[tid] = 0;
    int fr[kGbPer];
    long long tv[kGbPer];
#pragma unroll
    for (int j = 0; j < kGbPer; ++j) {
      const int64_t e = base + j * kGbThreads + tid;
      fr[j] = e < ne ? file[e] : -1;
      tv[j] = (TS && e < ne) ? ts[e] : kTsNullG;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGbPer; ++j) {
      const int64_t e = base + j * kGbThreads + tid;
      if (!TS) {
      } else if (tv[j] == kTsNullG) {
        nul |= e < ne;
      } else {
        lo = min(lo, tv[j]);
        hi = max(hi, tv[j]);
      }
      if (fr[j] >= 0 && fr[j] < nf) atomicAdd(&hist[(unsigned)fr[j] >> shift1], 1u);
    }
    __syncthreads();
    if (tid < R1) {
      tilepref[t * R1 + tid] = run;
      run += hist[tid];
    }
  }
  if (tid < R1) chunksum[c * R1 + tid] = run;
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
    nul |= __shfl_xor(nul, o);
  }
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    red[0][w] = lo;
    red[1][w] = hi;
    red[2][w] = nul;
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < kGbThreads / 64; ++i) {
      lo = min(lo, red[0][i]);
      hi = max(hi, red[1][i]);
      nul |= red[2][i];
    }
    part[3 * c] = lo;
    part[3 * c + 1] = hi;
    part[3 * c + 2] = nul;
  }
}

// ---- S1: chunk bases in three small kernels ---------------------------------
// a: per range of kGbRange chunks, the digit sums; b (one workgroup): range
// bases per digit, digit bases, pass-2 tile starts, the timestamp range;
// c: absolute chunk bases (digit base + range base + in-range prefix).
__global__ __launch_bounds__(kGbMaxBins) void gb_scan1a(const unsigned* __restrict__ chunk,
                                                        int64_t C, int R1,
                                                        unsigned* __restrict__ rsum) {
  const int r = threadIdx.x;
  if (r >= R1) return;
  const int64_t c0 = (int64_t)blockIdx.x * kGbRange;
  unsigned v[kGbRange];
#pragma unroll
  for (int j = 0; j < kGbRange; ++j) v[j] = c0 + j < C ? chunk[(c0 + j) * R1 + r] : 0u;
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < kGbRange; ++j) s += v[j];
  rsum[(int64_t)blockIdx.x * R1 + r] = s;
}

__global__ __launch_bounds__(kGbMaxBins) void gb_scan1b(unsigned* __restrict__ rsum, int64_t G,
                                                        int R1, const long long* __restrict__ part,
                                                        int64_t C, unsigned* __restrict__ binbase,
                                                        int* __restrict__ tile2start,
                                                        long long* __restrict__ res,
                                                        const long long* __restrict__ tsr) {
  __shared__ long long wred[3][8];
  __shared__ unsigned wsum[8], wt[8];
  const int tid = threadIdx.x;
  unsigned run = 0;
  if (tid < R1) {
    for (int64_t g0 = 0; g0 < G; g0 += 16) {
      unsigned v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = g0 + j < G ? rsum[(g0 + j) * R1 + tid] : 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (g0 + j < G) rsum[(g0 + j) * R1 + tid] = run;
        run += v[j];
      }
    }
  }
  long long lo = LLONG_MAX, hi = LLONG_MIN, nul = 0;
  for (int64_t c = tid; c < C; c += kGbMaxBins) {
    lo = min(lo, part[3 * c]);
    hi = max(hi, part[3 * c + 1]);
    nul |= part[3 * c + 2];
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
    nul |= __shfl_xor(nul, o);
  }
  const int lane = tid & 63, w = tid >> 6;
  if (lane == 0) {
    wred[0][w] = lo;
    wred[1][w] = hi;
    wred[2][w] = nul;
  }
  // exclusive scans over the digits (events and pass-2 tile counts)
  const unsigned v = tid < R1 ? run : 0u;
  const unsigned tl = (unsigned)((v + kGbTile - 1) / kGbTile);
  unsigned iv = v, it = tl;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned a = __shfl_up(iv, o), b = __shfl_up(it, o);
    if (lane >= o) {
      iv += a;
      it += b;
    }
  }
  if (lane == 63) {
    wsum[w] = iv;
    wt[w] = it;
  }
  __syncthreads();
  unsigned bv = 0, bt = 0;
  for (int i = 0; i < w; ++i) {
    bv += wsum[i];
    bt += wt[i];
  }
  if (tid < R1) {
    binbase[tid] = bv + iv - v;
    tile2start[tid] = (int)(bt + it - tl);
  }
  if (tid == kGbMaxBins - 1) {
    binbase[R1] = bv + iv;
    tile2start[R1] = (int)(bt + it);
    res[3] = bt + it;
    res[4] = bv + iv;
  }
  if (tid == 0) {
    for (int i = 1; i < 8; ++i) {
      lo = min(lo, wred[0][i]);
      hi = max(hi, wred[1][i]);
      nul |= wred[2][i];
    }
    res[0] = tsr ? tsr[0] : lo;
    res[1] = tsr ? tsr[1] : hi;
    res[2] = tsr ? tsr[2] : nul;
  }
}

// Timestamp range of n events (min and max of the non-null ones, any null):
// per-workgroup partials, then one workgroup.
__global__ __launch_bounds__(256) void gb_tsr_part(const long long* __restrict__ ts, int64_t n,
                                                   long long* __restrict__ part) {
  long long lo = LLONG_MAX, hi = LLONG_MIN, nul = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const long long t = ts[i];
    if (t == kTsNullG) {
      nul = 1;
    } else {
      lo = min(lo, t);
      hi = max(hi, t);
    }
  }
  __shared__ long long red[3][4];
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
    nul |= __shfl_xor(nul, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = lo;
    red[1][w] = hi;
    red[2][w] = nul;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      lo = min(lo, red[0][i]);
      hi = max(hi, red[1][i]);
      nul |= red[2][i];
    }
    part[3 * blockIdx.x] = lo;
    part[3 * blockIdx.x + 1] = hi;
    part[3 * blockIdx.x + 2] = nul;
  }
}

__global__ __launch_bounds__(64) void gb_tsr_fin(const long long* __restrict__ part, int nb,
                                                 long long* __restrict__ out) {
  long long lo = LLONG_MAX, hi = LLONG_MIN, nul = 0;
  for (int b = threadIdx.x; b < nb; b += 64) {
    lo = min(lo, part[3 * b]);
    hi = max(hi, part[3 * b + 1]);
    nul |= part[3 * b + 2];
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
    nul |= __shfl_xor(nul, o);
  }
  if (threadIdx.x == 0) {
    out[0] = lo;
    out[1] = hi;
    out[2] = nul;
  }
}

__global__ __launch_bounds__(kGbMaxBins) void gb_scan1c(unsigned* __restrict__ chunk, int64_t C,
                                                        int R1, const unsigned* __restrict__ rbase,
                                                        const unsigned* __restrict__ binbase) {
  const int r = threadIdx.x;
  if (r >= R1) return;
  const int64_t c0 = (int64_t)blockIdx.x * kGbRange;
  unsigned v[kGbRange];
#pragma unroll
  for (int j = 0; j < kGbRange; ++j) v[j] = c0 + j < C ? chunk[(c0 + j) * R1 + r] : 0u;
  unsigned run = binbase[r] + rbase[(int64_t)blockIdx.x * R1 + r];
#pragma unroll
  for (int j = 0; j < kGbRange; ++j) {
    if (c0 + j < C) chunk[(c0 + j) * R1 + r] = run;
    run += v[j];
  }
}

// ---- P1 / P2 ----------------------------------------------------------------
// Tile order: blocks are dealt round-robin over the 8 XCDs, so block b works
// on tile (b % 8) * per + b / 8: each XCD walks one contiguous range of tiles
// and a digit's consecutive runs are written from one L2.
__device__ __forceinline__ int64_t xcd_tile(int64_t per) {
  return (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
}

template <typename T>
struct GbStage {
  T val[kGbTile];
  uint16_t dig[kGbTile];
  unsigned cnt[kGbMaxBins], lp[kGbMaxBins], goff[kGbMaxBins];
  unsigned wsum[8];
};

// Rank the tile's events by digit in LDS, stage them digit-contiguous, and
// write each digit's run to its region (goff[d] = the run's first position).
// dr[j] = digit of event j, or ~0u when the event is not placed.
template <typename T>
__device__ __forceinline__ void gb_place(GbStage<T>& s, const T* val, unsigned* dr, int R,
                                         T* __restrict__ out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kGbPer; ++j)
    if (dr[j] != ~0u) dr[j] = (dr[j] << 16) | atomicAdd(&s.cnt[dr[j]], 1u);
  __syncthreads();
  lds_scan(s.cnt, s.lp, R, s.wsum);
#pragma unroll
  for (int j = 0; j < kGbPer; ++j) {
    if (dr[j] != ~0u) {
      const unsigned d = dr[j] >> 16;
      const unsigned slot = s.lp[d] + (dr[j] & 0xFFFFu);
      s.val[slot] = val[j];
      s.dig[slot] = (uint16_t)d;
    }
  }
  __syncthreads();
  const unsigned nv = s.lp[R - 1] + s.cnt[R - 1];
  for (unsigned i = tid; i < nv; i += kGbThreads) {
    const unsigned d = s.dig[i];
    out[s.goff[d] + (i - s.lp[d])] = s.val[i];
  }
}

template <typename T>
__global__ __launch_bounds__(kGbThreads) __attribute__((amdgpu_waves_per_eu(4))) void gb_scatter1(
    const int32_t* __restrict__ file, const uint8_t* __restrict__ op,
    const int32_t* __restrict__ client, const long long* __restrict__ ts, int64_t ne, int64_t nf,
    GbPay p, int shift1, int R1, int64_t T1, int64_t per, const unsigned* __restrict__ tilepref,
    const unsigned* __restrict__ chunkbase, T* __restrict__ out) {
  __shared__ GbStage<T> s;
  const int64_t t = xcd_tile(per);
  if (t >= T1) return;
  const int tid = threadIdx.x;
  const int64_t base = t * kGbTile;
  const int64_t c = t / kGbChunkTiles;
  if (tid < R1) {
    s.cnt[tid] = 0;
    s.goff[tid] = chunkbase[c * R1 + tid] + tilepref[t * R1 + tid];
  }
  // thread tid takes the tile's event quads q = j * 512 + tid (events
  // base + 4 q .. + 3), j = 0..3: every load instruction of a wave reads one
  // contiguous span (file / client ids 1 KiB, timestamps 2 x 1 KiB, op bytes
  // 256 B), so each cache line is used whole by the instruction that brings
  // it in.  (Lane-contiguous runs of 16 events left lines half-read between
  // instructions and, with the tile's working set over the L2, re-fetched:
  // 29.6 B read per 17-B event.)  The order of events inside a tile does not
  // matter to the partition.
  T val[kGbPer];
  unsigned dr[kGbPer];
  const bool full = base + kGbTile <= ne;
#pragma unroll
  for (int j = 0; j < kGbPer / 4; ++j) {
    const int64_t q = (int64_t)j * kGbThreads + tid;
    const int64_t eq = base + 4 * q;
    int fr[4], cv[4];
    long long tv[4];
    uint8_t ov[4];
    if (full) {
      const int4 a = reinterpret_cast<const int4*>(file + base)[q];
      const int4 b = reinterpret_cast<const int4*>(client + base)[q];
      const longlong2 t0 = reinterpret_cast<const longlong2*>(ts + base)[2 * q];
      const longlong2 t1 = reinterpret_cast<const longlong2*>(ts + base)[2 * q + 1];
      const unsigned o4 = reinterpret_cast<const unsigned*>(op + base)[q];
      fr[0] = a.x, fr[1] = a.y, fr[2] = a.z, fr[3] = a.w;
      cv[0] = b.x, cv[1] = b.y, cv[2] = b.z, cv[3] = b.w;
      tv[0] = t0.x, tv[1] = t0.y, tv[2] = t1.x, tv[3] = t1.y;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = (uint8_t)(o4 >> (8 * r));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t e = eq + r;
        const bool in = e < ne;
        fr[r] = in ? file[e] : -1;
        tv[r] = in ? ts[e] : 0;
        ov[r] = in ? op[e] : 0;
        cv[r] = in ? client[e] : -1;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * j + r;
      dr[o] = (fr[r] >= 0 && fr[r] < nf) ? (unsigned)fr[r] >> shift1 : ~0u;
      val[o] = gb_make<T>(p, (unsigned)((unsigned long long)(unsigned)fr[r] & p.low_mask), tv[r],
                          ov[r], cv[r]);
    }
  }
  __syncthreads();
  gb_place<T>(s, val, dr, R1, out);
}

__device__ __forceinline__ int find_digit(const int* __restrict__ start, int R1, int64_t t2) {
  int lo = 0, hi = R1;  // start[lo] <= t2 < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= t2) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(kGbThreads) void gb_hist2(const T* __restrict__ in,
                                                      const unsigned* __restrict__ binbase,
                                                      const int* __restrict__ tile2start, int R1,
                                                      int R2, int shift2,
                                                      unsigned* __restrict__ hist2) {
  __shared__ unsigned h[kGbMaxBins];
  const int64_t t2 = blockIdx.x;
  const int sd = find_digit(tile2start, R1, t2);
  const int64_t beg = binbase[sd] + (t2 - tile2start[sd]) * (int64_t)kGbTile;
  const int64_t end = min((int64_t)binbase[sd + 1], beg + kGbTile);
  if (threadIdx.x < R2) h[threadIdx.x] = 0;
  T v[kGbPer];
#pragma unroll
  for (int j = 0; j < kGbPer; ++j) {
    const int64_t i = beg + j * kGbThreads + threadIdx.x;
    v[j] = i < end ? in[i] : (T)0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kGbPer; ++j)
    if (beg + j * kGbThreads + threadIdx.x < end)
      atomicAdd(&h[(unsigned)((unsigned long long)v[j] >> shift2) & (R2 - 1)], 1u);
  __syncthreads();
  if (threadIdx.x < R2) hist2[t2 * R2 + threadIdx.x] = h[threadIdx.x];
}

// Pass 3 (large file counts): the R regions of pass 2 (bases bbase[0..R])
// become the regions pass 3 splits; tstart[r] = the 8192-event tiles before
// region r (exclusive scan of ceil(size / tile)), tstart[R] and *tot the
// total.  Two launches of kGbT3Per regions per workgroup, one region per
// thread: gb_tilecount3 sums each workgroup's tile counts, gb_tilestart3 adds
// the earlier workgroups' sums and scans its own regions.  (One workgroup
// walking all 2^18 regions of the 1B-event log took 0.43 ms per step.)
constexpr int kGbT3Per = 1024;
__device__ __forceinline__ unsigned gb_tiles_of(const unsigned* __restrict__ bbase, int r, int R) {
  return r < R ? (bbase[r + 1] - bbase[r] + kGbTile - 1) / kGbTile : 0u;
}
__global__ __launch_bounds__(kGbT3Per) void gb_tilecount3(const unsigned* __restrict__ bbase, int R,
                                                          unsigned* __restrict__ wsum) {
  __shared__ unsigned ws[kGbT3Per / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned c = gb_tiles_of(bbase, blockIdx.x * kGbT3Per + t, R);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) ws[w] = c;
  __syncthreads();
  if (t == 0) {
    unsigned s = 0;
    for (int i = 0; i < kGbT3Per / 64; ++i) s += ws[i];
    wsum[blockIdx.x] = s;
  }
}
__global__ __launch_bounds__(kGbT3Per) void gb_tilestart3(const unsigned* __restrict__ bbase, int R,
                                                          const unsigned* __restrict__ wsum,
                                                          int* __restrict__ tstart,
                                                          long long* __restrict__ tot) {
  __shared__ unsigned wb[kGbT3Per / 64], wi[kGbT3Per / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // this workgroup's base: the earlier workgroups' tile sums (a share per
  // wave, added up below)
  unsigned bs = 0;
  for (int i = t; i < (int)blockIdx.x; i += kGbT3Per) bs += wsum[i];
  for (int o = 32; o > 0; o >>= 1) bs += __shfl_xor(bs, o);
  // its regions' tile counts, scanned by waves and then across them
  const int r = blockIdx.x * kGbT3Per + t;
  const unsigned c = gb_tiles_of(bbase, r, R);
  unsigned inc = c;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 0) wb[w] = bs;
  if (lane == 63) wi[w] = inc;
  __syncthreads();
  unsigned run = inc - c;
  for (int i = 0; i < kGbT3Per / 64; ++i) {
    run += wb[i];             // the earlier workgroups' tiles
    if (i < w) run += wi[i];  // the earlier waves' regions
  }
  if (r < R) tstart[r] = (int)run;
  if (r == R - 1) {
    tstart[R] = (int)(run + c);
    *tot = (long long)(run + c);
  }
}

// Pass 3's scan with few bins (R3 <= 16): one thread per region sd (most
// regions span one or two tiles): running offsets over its tiles per bin,
// then its bucket bases bbase3[sd * R3 + r].
constexpr int kGbScan3Max = 16;
__global__ __launch_bounds__(256) void gb_scan3(unsigned* __restrict__ hist3,
                                                const int* __restrict__ tstart,
                                                const unsigned* __restrict__ bbase, int R12, int R3,
                                                unsigned* __restrict__ bbase3) {
  const int sd = blockIdx.x * 256 + threadIdx.x;
  if (sd >= R12) return;
  const int t0 = tstart[sd], t1 = tstart[sd + 1];
  unsigned base = bbase[sd];
  for (int r = 0; r < R3; ++r) {
    unsigned run = 0;
    for (int tb = t0; tb < t1; ++tb) {
      const unsigned v = hist3[(int64_t)tb * R3 + r];
      hist3[(int64_t)tb * R3 + r] = run;
      run += v;
    }
    bbase3[(int64_t)sd * R3 + r] = base;
    base += run;
  }
  if (sd == R12 - 1) bbase3[(int64_t)R12 * R3] = bbase[R12];
}

// One workgroup per pass-1 digit sd, thread r = pass-2 digit: running offsets
// over the digit's tiles, then the bucket bases bbase[sd * R2 + r].
__global__ __launch_bounds__(kGbMaxBins) void gb_scan2(unsigned* __restrict__ hist2,
                                                       const int* __restrict__ tile2start,
                                                       const unsigned* __restrict__ binbase,
                                                       int R1, int R2,
                                                       unsigned* __restrict__ bbase) {
  __shared__ unsigned cnt[kGbMaxBins], lp[kGbMaxBins], wsum[8];
  const int sd = blockIdx.x, r = threadIdx.x;
  const int t0 = tile2start[sd], t1 = tile2start[sd + 1];
  unsigned run = 0;
  if (r < R2) {
    for (int tb = t0; tb < t1; tb += 16) {
      unsigned v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tb + j < t1 ? hist2[(int64_t)(tb + j) * R2 + r] : 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (tb + j < t1) hist2[(int64_t)(tb + j) * R2 + r] = run;
        run += v[j];
      }
    }
    cnt[r] = run;
  }
  __syncthreads();
  lds_scan(cnt, lp, R2, wsum);
  if (r < R2) bbase[(int64_t)sd * R2 + r] = binbase[sd] + lp[r];
  if (sd == R1 - 1 && r == 0) bbase[(int64_t)R1 * R2] = binbase[R1];
}

template <typename T>
__global__ __launch_bounds__(kGbThreads) void gb_scatter2(
    const T* __restrict__ in, const unsigned* __restrict__ binbase,
    const int* __restrict__ tile2start, int R1, int R2, int shift2, int64_t T2, int64_t per,
    const unsigned* __restrict__ off2, const unsigned* __restrict__ bbase, T* __restrict__ out) {
  __shared__ GbStage<T> s;
  const int64_t t2 = xcd_tile(per);
  if (t2 >= T2) return;
  const int tid = threadIdx.x;
  const int sd = find_digit(tile2start, R1, t2);
  const int64_t beg = binbase[sd] + (t2 - tile2start[sd]) * (int64_t)kGbTile;
  const int64_t end = min((int64_t)binbase[sd + 1], beg + kGbTile);
  if (tid < R2) {
    s.cnt[tid] = 0;
    s.goff[tid] = bbase[(int64_t)sd * R2 + tid] + off2[t2 * R2 + tid];
  }
  T val[kGbPer];
  unsigned dr[kGbPer];
#pragma unroll
  for (int j = 0; j < kGbPer; ++j) {
    const int64_t i = beg + j * kGbThreads + tid;
    val[j] = i < end ? in[i] : (T)0;
  }
#pragma unroll
  for (int j = 0; j < kGbPer; ++j)
    dr[j] = beg + j * kGbThreads + tid < end
                ? (unsigned)((unsigned long long)val[j] >> shift2) & (R2 - 1)
                : ~0u;
  __syncthreads();
  gb_place<T>(s, val, dr, R2, out);
}

// One pass after the first: the NR regions of the pass before (bases rbase,
// NT tiles starting at tstart per region) are split by the R-valued digit at
// `shift`, from in to out; bbase = the NR R + 1 bases of what comes out.
template <typename T>
void gb_pass(Ctx& c, const unsigned* rbase, const int* tstart, int NR, int64_t NT, int R,
             int shift, const T* in, T* out, unsigned* bbase, bool scan3) {
  c.gb_hist2.ensure(sizeof(unsigned) * (size_t)std::max<int64_t>(NT, 1) * R);
  unsigned* hist = c.gb_hist2.as<unsigned>();
  if (NT > 0)
    hipLaunchKernelGGL(gb_hist2<T>, dim3((unsigned)NT), dim3(kGbThreads), 0, c.stream, in, rbase,
                       tstart, NR, R, shift, hist);
  if (scan3)
    hipLaunchKernelGGL(gb_scan3, dim3((NR + 255) / 256), dim3(256), 0, c.stream, hist, tstart,
                       rbase, NR, R, bbase);
  else
    hipLaunchKernelGGL(gb_scan2, dim3(NR), dim3(kGbMaxBins), 0, c.stream, hist, tstart, rbase, NR,
                       R, bbase);
  HIP_CHECK(hipGetLastError());
  if (NT > 0) {
    const int64_t per = ceil_div(NT, 8);
    hipLaunchKernelGGL(gb_scatter2<T>, dim3(8 * per), dim3(kGbThreads), 0, c.stream, in, rbase,
                       tstart, NR, R, shift, NT, per, hist, bbase, out);
    HIP_CHECK(hipGetLastError());
  }
}

template <typename T>
const void* gb_partition_t(Ctx& c, int64_t ne, int64_t nf, const GbLayout& lay,
                           const long long* res, const unsigned** bases) {
  const GbPay& p = lay.p;
  const int R1 = 1 << lay.B1, R2 = 1 << lay.B2;
  const int64_t T1 = std::max<int64_t>(1, ceil_div(ne, kGbTile));
  T* p1 = c.gb_p1.as<T>();
  unsigned* binbase = c.gb_small.as<unsigned>();
  if (res[4] > 0) {
    const int64_t per1 = ceil_div(T1, 8);
    hipLaunchKernelGGL(gb_scatter1<T>, dim3(8 * per1), dim3(kGbThreads), 0, c.stream,
                       c.ev_file.as<int32_t>(), c.ev_op.as<uint8_t>(), c.ev_client.as<int32_t>(),
                       c.ev_ts.as<long long>(), ne, nf, p, lay.fbits - lay.B1, R1, T1, per1,
                       c.gb_tilepref.as<unsigned>(), c.gb_chunk.as<unsigned>(), p1);
    HIP_CHECK(hipGetLastError());
  }
  const T* pb = p1;
  unsigned* bbase = binbase;  // one pass: the buckets are the pass-1 digits
  if (lay.B2 > 0) {
    // pass-2 tiles per digit were counted by S1 for the same tile size
    bbase = c.gb_bbase.as<unsigned>();
    gb_pass<T>(c, binbase, gb_tile2start(c), R1, res[3], R2, p.fshift + p.L + lay.B3, p1,
               c.gb_p2.as<T>(), bbase, false);
    pb = c.gb_p2.as<T>();
  }
  if (lay.B3 > 0) {
    // pass 3 within each of the R1 R2 pass-2 regions (the same kernels: its
    // regions take the place of pass 1's digits); output into p1's buffer
    const int R12 = R1 * R2, R3 = 1 << lay.B3;
    const int g3 = (R12 + kGbT3Per - 1) / kGbT3Per;
    c.gb_t3.ensure(sizeof(int) * ((size_t)R12 + 1 + g3) + 64);
    int* tstart3 = c.gb_t3.as<int>();
    unsigned* wsum3 = reinterpret_cast<unsigned*>(tstart3 + R12 + 1);  // (after the starts)
    long long* tot3 = c.gb_res.as<long long>() + 6;
    hipLaunchKernelGGL(gb_tilecount3, dim3(g3), dim3(kGbT3Per), 0, c.stream, bbase, R12, wsum3);
    hipLaunchKernelGGL(gb_tilestart3, dim3(g3), dim3(kGbT3Per), 0, c.stream, bbase, R12, wsum3,
                       tstart3, tot3);
    HIP_CHECK(hipGetLastError());
    long long T3 = 0;
    HIP_CHECK(hipMemcpyAsync(&T3, tot3, sizeof(T3), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    c.gb_bbase3.ensure(sizeof(unsigned) * ((size_t)R12 * R3 + 1) + 64);
    unsigned* bbase3 = c.gb_bbase3.as<unsigned>();
    gb_pass<T>(c, bbase, tstart3, R12, T3, R3, p.fshift + p.L, pb, p1, bbase3,
               R3 <= kGbScan3Max);
    pb = p1;
    bbase = bbase3;
  }
  *bases = bbase;
  return pb;
}

}  // namespace

void gb_count(Ctx& c, int64_t ne, int64_t nf, int fbits, int B1, long long res[5]) {
  const int R1 = 1 << B1;
  const int64_t T1 = std::max<int64_t>(1, ceil_div(ne, kGbTile));
  const int64_t C = ceil_div(T1, kGbChunkTiles);
  c.gb_tilepref.ensure(sizeof(unsigned) * (size_t)T1 * R1);
  c.gb_chunk.ensure(sizeof(unsigned) * (size_t)C * R1);
  c.gb_part.ensure(sizeof(long long) * 3 * (size_t)C + 64);
  c.gb_small.ensure(sizeof(int) * (3 * (kGbMaxBins + 1) + 8));
  c.gb_res.ensure(sizeof(long long) * 8);  // (res[6]: pass 3's tile total)
  c.gb_bbase.ensure(sizeof(unsigned) * ((size_t)R1 << kGbMaxDigit) + 64);
  // the producer's timestamp range, when it computed one for these events
  const bool tsr = c.ev_tsr_valid && c.ev_tsr_n == ne && !exp_env("CDR_GB_TSRANGE");
  hipLaunchKernelGGL(tsr ? gb_hist1<false> : gb_hist1<true>, dim3(C), dim3(kGbThreads), 0,
                     c.stream, c.ev_file.as<int32_t>(), c.ev_ts.as<long long>(), ne, nf,
                     fbits - B1, R1, c.gb_tilepref.as<unsigned>(), c.gb_chunk.as<unsigned>(),
                     c.gb_part.as<long long>());
  HIP_CHECK(hipGetLastError());
  unsigned* binbase = c.gb_small.as<unsigned>();
  const int64_t G = ceil_div(C, kGbRange);
  c.gb_rsum.ensure(sizeof(unsigned) * (size_t)G * R1);
  hipLaunchKernelGGL(gb_scan1a, dim3(G), dim3(kGbMaxBins), 0, c.stream, c.gb_chunk.as<unsigned>(),
                     C, R1, c.gb_rsum.as<unsigned>());
  hipLaunchKernelGGL(gb_scan1b, dim3(1), dim3(kGbMaxBins), 0, c.stream, c.gb_rsum.as<unsigned>(),
                     G, R1, c.gb_part.as<long long>(), C, binbase, gb_tile2start(c),
                     c.gb_res.as<long long>(), tsr ? c.ev_tsr.as<long long>() : nullptr);
  hipLaunchKernelGGL(gb_scan1c, dim3(G), dim3(kGbMaxBins), 0, c.stream, c.gb_chunk.as<unsigned>(),
                     C, R1, c.gb_rsum.as<unsigned>(), binbase);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(res, c.gb_res.p, 5 * sizeof(long long), hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

const void* gb_partition(Ctx& c, int64_t ne, int64_t nf, const GbLayout& lay,
                         const long long res[5], const unsigned** bbase) {
  const size_t bytes = (size_t)lay.pbytes * (ne > 0 ? (size_t)ne : 1);
  c.gb_p1.ensure(bytes);
  if (lay.B2 > 0) c.gb_p2.ensure(bytes);
  return lay.pbytes == 4 ? gb_partition_t<unsigned>(c, ne, nf, lay, res, bbase)
                         : gb_partition_t<unsigned long long>(c, ne, nf, lay, res, bbase);
}

// The resident events' timestamp range, computed once by their producer (the
// group-by's partition then reads 4 B per event in its histogram pass
// instead of 12).  Every writer of c.ev_ts calls this or clears
// c.ev_tsr_valid.
void events_ts_range(Ctx& c, int64_t ne) {
  c.ev_tsr.ensure(sizeof(long long) * 4);
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(2048, ceil_div(ne, 256 * 16)));
  c.gb_part.ensure(sizeof(long long) * 3 * (size_t)nb + 64);
  hipLaunchKernelGGL(gb_tsr_part, dim3(nb), dim3(256), 0, c.stream, c.ev_ts.as<long long>(), ne,
                     c.gb_part.as<long long>());
  hipLaunchKernelGGL(gb_tsr_fin, dim3(1), dim3(64), 0, c.stream, c.gb_part.as<long long>(), nb,
                     c.ev_tsr.as<long long>());
  HIP_CHECK(hipGetLastError());
  c.ev_tsr_valid = true;
  c.ev_tsr_n = ne;
}

}  // namespace cdr
