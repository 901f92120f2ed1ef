// place.hip — where each file's replicas go (an extension with no
// reference counterpart): per file the access count of every node, the nodes
// of its replicas (its primary first, then the nodes by descending count, ties
// to the lower id), and the accesses that are node-local before and after.
//
//   place_bucket<T>  the bucket form: one wave owns one bucket of 2^L files of
//                    the resident partition (groupby_pay.h's payload, 4 or 8 B
//                    per event), counts its events into a private LDS grid of
//                    2^L x (n_nodes + 1) uint32 (column 0: no node), then
//                    selects per file
//   place_count      the global form: one integer add per event into a zeroed
//                    uint32 [n_files][n_nodes + 1] table, straight from
//                    ev_file / ev_client
//   place_select     the global form's selection: one wave per 64 files
//
// Both forms run place_files over their rows: lane j holds cnt[f][j], `factor`
// rounds of a wave-wide arg-max over (count, -node id) choose the nodes.  The
// cluster and node sums are kept per workgroup in LDS (the node sums first in
// lane j's registers) and flushed once with global uint64 adds: integers, so
// the order does not matter.  A label outside [0, k), a factor outside [0, R]
// or a negative size raises a flag and is never used as an index; a client
// code above n_nodes counts in the file's total only; rows >= n_files are
// never read or written.
#include "cdr_internal.h"

#include <algorithm>

namespace cdr {

namespace {

constexpr int kPlWaves = 4;          // waves per workgroup
constexpr int kPlUnroll = 8;         // payload loads in flight per lane
constexpr int kPlSlice = 12288;      // bucket form: bytes of 2^L x n_nodes counters per wave
constexpr int kPlMaxNodes = 64;
constexpr int kPlMaxK = 1024;
constexpr int kPlMaxR = 8;
constexpr int kPlCountBlock = 256;
constexpr int kPlCountPerCu = 8;
constexpr int64_t kPlMaxCells = 1ll << 30;  // global form: n_files * n_nodes

struct PlaceArgs {
  const int32_t* primary;   // [nf], -2 = null
  const int32_t* labels;    // [nf] in [0, k)
  const int32_t* factors;   // [k] in [0, R]
  const long long* sizes;   // [nf] >= 0, or null
  int64_t nf;
  int n_nodes, k, R;
  int32_t* nodes;           // [nf][R]
  long long* per_file;      // [nf][3] or null
  long long* counts;        // [nf][n_nodes] or null
  unsigned long long* csum; // [k][3], zeroed
  unsigned long long* nsum; // [n_nodes][3], zeroed
  int* flag;
};

__device__ __forceinline__ unsigned wave_add(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}

// Lane j's sums of node j over everything its wave placed.
struct NodeAcc {
  unsigned long long rep = 0, lo = 0, hi = 0;
};

// The files f0 .. f0 + nfl of one wave: file i's row at rows + i * N1, [0] the
// events of no node, [1 + j] the events of node j.  Files go in chunks of 64
// (lane i loads file i's primary, label, factor, size) and, within a chunk, in
// groups of G = 64 / R: the group's R node ids per file sit in lanes
// [g R, g R + R) and leave as one contiguous run, its {total, before, after}
// in lane g.  Returns the lane's error bits (1 label, 2 size, 4 factor).
__device__ __forceinline__ int place_files(const unsigned* rows, int N1, int64_t f0, int nfl,
                                           const PlaceArgs& a, unsigned long long* lcs,
                                           NodeAcc& acc) {
  const int lane = threadIdx.x & 63;
  const int nn = a.n_nodes, R = a.R, G = 64 / R;
  int bad = 0;
  for (int c0 = 0; c0 < nfl; c0 += 64) {
    const int nc = min(64, nfl - c0);
    int pr = -2, lab = -1, fac = 0;
    long long sz = 0;
    if (lane < nc) {
      const int64_t f = f0 + c0 + lane;
      pr = a.primary[f];
      lab = a.labels[f];
      if ((unsigned)lab < (unsigned)a.k) {
        fac = a.factors[lab];
        if ((unsigned)fac > (unsigned)R) {
          bad |= 4;
          fac = 0;
        }
      } else {
        bad |= 1;
        lab = -1;
      }
      if (a.sizes) {
        sz = a.sizes[f];
        if (sz < 0) {
          bad |= 2;
          sz = 0;
        }
      }
    }
    for (int g0 = 0; g0 < nc; g0 += G) {
      const int ng = min(G, nc - g0);
      int ov = -1;
      unsigned t_ = 0, b_ = 0, a_ = 0;
      for (int g = 0; g < ng; ++g) {
        const int src = g0 + g;  // the file's lane in this chunk
        const int p = __shfl(pr, src);
        const int fc = __shfl(fac, src);
        const unsigned* row = rows + (size_t)(c0 + src) * N1;
        const unsigned cnt = lane < nn ? row[1 + lane] : 0u;
        const unsigned tot = wave_add(cnt + (lane == 0 ? row[0] : 0u));
        const bool pv = p >= 0 && p < nn;
        const unsigned lb = pv ? (unsigned)__shfl((int)cnt, p & 63) : 0u;
        const int m = min(fc, nn);
        bool avail = lane < nn;
        unsigned la = 0;
        for (int r = 0; r < m; ++r) {
          int pick;
          if (r == 0 && pv) {
            pick = p;
          } else {
            const unsigned mx = wave_umax(avail ? cnt : 0u);
            pick = __ffsll((long long)__ballot(avail && cnt == mx)) - 1;  // the lowest such id
          }
          la += (unsigned)__shfl((int)cnt, pick & 63);
          if (lane == pick) avail = false;
          if (lane == g * R + r) ov = pick;
        }
        if (lane == g) {
          t_ = tot;
          b_ = lb;
          a_ = la;
        }
        const unsigned long long s = (unsigned long long)__shfl(sz, src);
        if (lane < nn && !avail) {  // node `lane` holds a replica of this file
          acc.rep += 1;
          acc.lo += s & 0xFFFFFFFFull;
          acc.hi += s >> 32;
        }
        if (a.counts && lane < nn) a.counts[(f0 + c0 + src) * nn + lane] = (long long)cnt;
      }
      const int64_t fb = f0 + c0 + g0;
      if (lane < ng * R) a.nodes[fb * R + lane] = ov;
      const int lg = __shfl(lab, (g0 + lane) & 63);
      if (lane < ng) {
        if (a.per_file) {
          long long* o = a.per_file + (fb + lane) * 3;
          o[0] = t_;
          o[1] = b_;
          o[2] = a_;
        }
        if (lg >= 0) {
          if (t_) atomicAdd(&lcs[3 * lg], (unsigned long long)t_);
          if (b_) atomicAdd(&lcs[3 * lg + 1], (unsigned long long)b_);
          if (a_) atomicAdd(&lcs[3 * lg + 2], (unsigned long long)a_);
        }
      }
    }
  }
  return bad;
}

// LDS of both selection kernels: [k][3] cluster sums, [n_nodes][3] node sums.
__device__ __forceinline__ void sums_clear(unsigned long long* lds, int words) {
  for (int t = threadIdx.x; t < words; t += blockDim.x) lds[t] = 0ull;
  __syncthreads();
}

__device__ __forceinline__ void sums_flush(unsigned long long* lcs, unsigned long long* lns,
                                           const NodeAcc& acc, int bad, const PlaceArgs& a) {
  const int lane = threadIdx.x & 63;
  if (lane < a.n_nodes) {
    if (acc.rep) atomicAdd(&lns[3 * lane], acc.rep);
    if (acc.lo) atomicAdd(&lns[3 * lane + 1], acc.lo);
    if (acc.hi) atomicAdd(&lns[3 * lane + 2], acc.hi);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 3 * a.k; t += blockDim.x)
    if (lcs[t]) atomicAdd(&a.csum[t], lcs[t]);
  for (int t = threadIdx.x; t < 3 * a.n_nodes; t += blockDim.x)
    if (lns[t]) atomicAdd(&a.nsum[t], lns[t]);
  if (bad) atomicOr(a.flag, bad);
}

__host__ __device__ inline int pl_wave_words(int L, int n_nodes) {
  return (((n_nodes + 1) << L) + 3) & ~3;  // u32 words, 16-byte aligned slices
}
__host__ __device__ inline int pl_sum_words(int k, int n_nodes) {
  return (3 * (k + n_nodes) + 1) & ~1;  // u64 words, so that the slices start 16-byte aligned
}

// Persistent: wave w of the grid takes buckets w, w + W, ... (strided like
// gb_bucket_wave).  LDS instructions of one wave run in order, so the clear,
// the adds and the reads of its slice need no workgroup barrier.
template <typename T>
__global__ __launch_bounds__(64 * kPlWaves) void place_bucket(const T* __restrict__ pb,
                                                             const unsigned* __restrict__ bbase,
                                                             int64_t nbuckets, GbPay p,
                                                             PlaceArgs a) {
  extern __shared__ unsigned long long pl_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long* lcs = pl_lds;
  unsigned long long* lns = lcs + 3 * a.k;
  const int N1 = a.n_nodes + 1;
  const int F = 1 << p.L;
  const int KW = pl_wave_words(p.L, a.n_nodes);
  unsigned* grid =
      reinterpret_cast<unsigned*>(pl_lds + pl_sum_words(a.k, a.n_nodes)) + (size_t)wv * KW;
  sums_clear(pl_lds, 3 * (a.k + a.n_nodes));
  NodeAcc acc;
  int bad = 0;
  const int64_t nw = (int64_t)gridDim.x * kPlWaves;
  for (int64_t b = (int64_t)blockIdx.x * kPlWaves + wv; b < nbuckets; b += nw) {
    const int64_t s0 = bbase[b], n = (int64_t)bbase[b + 1] - s0;
    const int64_t f0 = b << p.L;
    const int nfl = (int)min((int64_t)F, a.nf - f0);
    if (nfl <= 0) continue;
    T v[kPlUnroll];
#pragma unroll
    for (int u = 0; u < kPlUnroll; ++u) {
      const int64_t i = u * 64 + lane;
      v[u] = i < n ? pb[s0 + i] : (T)0;
    }
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int i = lane * 4; i < KW; i += 256) *reinterpret_cast<uint4*>(grid + i) = z;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t i0 = 0; i0 < n; i0 += 64 * kPlUnroll) {
      if (i0 > 0) {
#pragma unroll
        for (int u = 0; u < kPlUnroll; ++u) {
          const int64_t i = i0 + u * 64 + lane;
          v[u] = i < n ? pb[s0 + i] : (T)0;
        }
      }
#pragma unroll
      for (int u = 0; u < kPlUnroll; ++u) {
        if (i0 + u * 64 >= n) break;  // (the same on every lane)
        if (i0 + u * 64 + lane < n) {
          const GbFields e = gb_decode((unsigned long long)v[u], p);
          const unsigned col = e.cc <= (unsigned)a.n_nodes ? e.cc : 0u;  // (code 0: no node)
          atomicAdd(&grid[e.fl * N1 + col], 1u);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bad |= place_files(grid, N1, f0, nfl, a, lcs, acc);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  sums_flush(lcs, lns, acc, bad, a);
}

__global__ __launch_bounds__(kPlCountBlock) void place_count(const int32_t* __restrict__ file,
                                                            const int32_t* __restrict__ client,
                                                            int64_t ne, int64_t nf, int n_nodes,
                                                            unsigned* __restrict__ table) {
  const int N1 = n_nodes + 1;
  for (int64_t e = (int64_t)blockIdx.x * kPlCountBlock + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * kPlCountBlock) {
    const int f = file[e];
    if (f < 0 || f >= nf) continue;
    const int cl = client[e];
    const int col = cl >= 0 && cl < n_nodes ? cl + 1 : 0;
    atomicAdd(&table[(int64_t)f * N1 + col], 1u);
  }
}

__global__ __launch_bounds__(64 * kPlWaves) void place_select(const unsigned* __restrict__ table,
                                                             PlaceArgs a) {
  extern __shared__ unsigned long long pl_lds[];
  const int wv = threadIdx.x >> 6;
  unsigned long long* lcs = pl_lds;
  unsigned long long* lns = lcs + 3 * a.k;
  const int N1 = a.n_nodes + 1;
  sums_clear(pl_lds, 3 * (a.k + a.n_nodes));
  NodeAcc acc;
  int bad = 0;
  const int64_t nw = (int64_t)gridDim.x * kPlWaves;
  const int64_t ngroups = (a.nf + 63) >> 6;
  for (int64_t g = (int64_t)blockIdx.x * kPlWaves + wv; g < ngroups; g += nw) {
    const int64_t f0 = g << 6;
    const int nfl = (int)min((int64_t)64, a.nf - f0);
    bad |= place_files(table + f0 * N1, N1, f0, nfl, a, lcs, acc);
  }
  sums_flush(lcs, lns, acc, bad, a);
}

struct PlaceEvents {
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~PlaceEvents() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

double pl_ms_between(hipEvent_t a, hipEvent_t b) {
  float v = 0.f;
  (void)hipEventElapsedTime(&v, a, b);
  return v;
}

template <typename T>
int launch_bucket(Ctx& c, const GbPartition& part, const PlaceArgs& a, size_t lds) {
  const void* fn = reinterpret_cast<const void*>(&place_bucket<T>);
  // beyond the default 64 KiB of dynamic LDS (set on every such launch)
  if (lds > 64 * 1024)
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * kPlWaves, lds));
  per_cu = std::max(1, per_cu);
  const int grid = (int)std::min<int64_t>(ceil_div(part.nb, (int64_t)kPlWaves),
                                          (int64_t)lloyd_num_cus(c.device) * per_cu);
  hipLaunchKernelGGL(place_bucket<T>, dim3(grid), dim3(64 * kPlWaves), lds, c.stream,
                     static_cast<const T*>(part.pay), part.bbase, part.nb, part.p, a);
  HIP_CHECK(hipGetLastError());
  return grid;
}

}  // namespace

void place_replicas(Ctx& c, int32_t n_nodes, const int64_t* labels, int64_t n_labels, int32_t k,
                    const int32_t* factors, int32_t R, const int64_t* sizes, int32_t* nodes_out,
                    int64_t* per_file_out, int64_t* counts_out, uint64_t* cluster_sums,
                    uint64_t* node_sums) {
  if (n_nodes < 1 || n_nodes > kPlMaxNodes)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "place: n_nodes outside [1, 64]");
  if (k < 1 || k > kPlMaxK) CDR_FAIL(CDR_ERR_UNSUPPORTED, "place: k outside [1, 1024]");
  if (R < 1 || R > kPlMaxR) CDR_FAIL(CDR_ERR_ARG, "place: R outside [1, 8]");
  if (c.ev_nf <= 0 || c.ev_foreign) CDR_FAIL(CDR_ERR_STATE, "place: no resident events");
  if (!nodes_out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  const int64_t ne = c.ev_n, nf = c.ev_nf;
  if (labels) {
    if (n_labels != nf) CDR_FAIL(CDR_ERR_ARG, "place: n_labels is not the events' n_files");
  } else {
    if (!c.have_labels)
      CDR_FAIL(CDR_ERR_STATE, "place: no labels on the device: run a Lloyd step or pass labels");
    if (c.n != nf) CDR_FAIL(CDR_ERR_ARG, "place: the resident labels' row count is not n_files");
    if (k < c.last_k) CDR_FAIL(CDR_ERR_ARG, "place: k smaller than the resident labels' k");
  }
  for (int j = 0; j < k; ++j)
    if (factors[j] < 0 || factors[j] > R) CDR_FAIL(CDR_ERR_ARG, "place: a factor outside [0, R]");
  if (sizes)
    for (int64_t i = 0; i < nf; ++i)
      if (sizes[i] < 0) CDR_FAIL(CDR_ERR_ARG, "place: negative size");
  if (labels) {
    c.pl_stage.ensure(sizeof(int32_t) * (size_t)nf);
    int32_t* h = c.pl_stage.as<int32_t>();
    for (int64_t i = 0; i < nf; ++i) {
      if (labels[i] < 0 || labels[i] >= k) CDR_FAIL(CDR_ERR_ARG, "place: a label outside [0, k)");
      h[i] = (int32_t)labels[i];
    }
  }
  for (int i = 0; i < 6; ++i) c.pl_info[i] = 0;
  c.pl_info[0] = -1;
  for (double& v : c.pl_ms) v = 0.0;
  PlaceEvents ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  // the form, decided before any launch
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  // (CDR_GROUPBY_SORT: the group-by does not take the shape, whatever is resident)
  bool bucket = !getenv("CDR_PLACE_GLOBAL") && !getenv("CDR_GROUPBY_SORT");
  bool reused = false;
  if (bucket) {
    reused = c.gb_part_rec.valid && c.gb_part_rec.ne == ne && c.gb_part_rec.nf == nf;
    if (!reused) {
      int64_t max_ts = 0;
      bucket = groupby_resident(c, ne, nf, nullptr, &max_ts);
    }
    if (bucket && ((int64_t)4 << c.gb_part_rec.p.L) * n_nodes > kPlSlice) bucket = false;
  }
  if (!bucket && nf * (int64_t)n_nodes > kPlMaxCells)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "place: n_files * n_nodes above 2^30 in the global form");
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  // uploads and zeroing
  if (labels) {
    c.pl_lab.ensure(sizeof(int32_t) * (size_t)nf);
    HIP_CHECK(hipMemcpyAsync(c.pl_lab.p, c.pl_stage.p, sizeof(int32_t) * (size_t)nf,
                             hipMemcpyHostToDevice, c.stream));
  }
  c.pl_fac.ensure(sizeof(int32_t) * (size_t)k);
  HIP_CHECK(hipMemcpyAsync(c.pl_fac.p, factors, sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice,
                           c.stream));
  if (sizes) {
    c.pl_sz.ensure(8 * (size_t)nf);
    HIP_CHECK(hipMemcpyAsync(c.pl_sz.p, sizes, 8 * (size_t)nf, hipMemcpyHostToDevice, c.stream));
  }
  c.pl_nodes.ensure(sizeof(int32_t) * (size_t)nf * R);
  if (per_file_out) c.pl_pf.ensure(8 * 3 * (size_t)nf);
  if (counts_out) c.pl_cnt.ensure(8 * (size_t)nf * n_nodes);
  const size_t words = 3 * (size_t)(k + n_nodes) + 1;  // cluster sums, node sums, the flag
  c.pl_sum.ensure(8 * words);
  c.pl_host.ensure(8 * words);
  HIP_CHECK(hipMemsetAsync(c.pl_sum.p, 0, 8 * words, c.stream));
  const int N1 = n_nodes + 1;
  if (!bucket) {
    c.pl_tab.ensure(sizeof(unsigned) * (size_t)nf * N1);
    HIP_CHECK(hipMemsetAsync(c.pl_tab.p, 0, sizeof(unsigned) * (size_t)nf * N1, c.stream));
  }
  HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
  PlaceArgs a;
  a.primary = c.ev_primary.as<int32_t>();
  a.labels = labels ? c.pl_lab.as<int32_t>() : c.labels.as<int32_t>();
  a.factors = c.pl_fac.as<int32_t>();
  a.sizes = sizes ? c.pl_sz.as<long long>() : nullptr;
  a.nf = nf;
  a.n_nodes = n_nodes;
  a.k = k;
  a.R = R;
  a.nodes = c.pl_nodes.as<int32_t>();
  a.per_file = per_file_out ? c.pl_pf.as<long long>() : nullptr;
  a.counts = counts_out ? c.pl_cnt.as<long long>() : nullptr;
  a.csum = c.pl_sum.as<unsigned long long>();
  a.nsum = a.csum + 3 * (size_t)k;
  a.flag = reinterpret_cast<int*>(a.csum + words - 1);
  const size_t sums_lds = 8 * (size_t)pl_sum_words(k, n_nodes);
  int grid = 0;
  if (bucket) {
    const GbPartition& part = c.gb_part_rec;
    const size_t lds = sums_lds + (size_t)kPlWaves * 4 * pl_wave_words(part.p.L, n_nodes);
    grid = part.pbytes == 4 ? launch_bucket<unsigned>(c, part, a, lds)
                            : launch_bucket<unsigned long long>(c, part, a, lds);
    c.pl_info[1] = part.p.L;
    c.pl_info[2] = part.nb;
    c.pl_info[4] = reused ? 1 : 0;
    c.pl_info[5] = part.pbytes;
  } else {
    const int cus = lloyd_num_cus(c.device);
    if (ne > 0) {
      const int cg = (int)std::min<int64_t>(ceil_div(ne, (int64_t)kPlCountBlock),
                                            (int64_t)kPlCountPerCu * cus);
      hipLaunchKernelGGL(place_count, dim3(cg), dim3(kPlCountBlock), 0, c.stream,
                         c.ev_file.as<int32_t>(), c.ev_client.as<int32_t>(), ne, nf, (int)n_nodes,
                         c.pl_tab.as<unsigned>());
      HIP_CHECK(hipGetLastError());
    }
    const void* fn = reinterpret_cast<const void*>(&place_select);
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * kPlWaves, sums_lds));
    per_cu = std::max(1, per_cu);
    grid = (int)std::min<int64_t>(ceil_div(ceil_div(nf, (int64_t)64), (int64_t)kPlWaves),
                                  (int64_t)cus * per_cu);
    hipLaunchKernelGGL(place_select, dim3(grid), dim3(64 * kPlWaves), sums_lds, c.stream,
                       c.pl_tab.as<unsigned>(), a);
    HIP_CHECK(hipGetLastError());
  }
  c.pl_info[0] = bucket ? 0 : 1;
  c.pl_info[3] = grid;
  HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
  HIP_CHECK(hipMemcpyAsync(c.pl_host.p, c.pl_sum.p, 8 * words, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipMemcpyAsync(nodes_out, c.pl_nodes.p, sizeof(int32_t) * (size_t)nf * R,
                           hipMemcpyDeviceToHost, c.stream));
  if (per_file_out)
    HIP_CHECK(hipMemcpyAsync(per_file_out, c.pl_pf.p, 8 * 3 * (size_t)nf, hipMemcpyDeviceToHost,
                             c.stream));
  if (counts_out)
    HIP_CHECK(hipMemcpyAsync(counts_out, c.pl_cnt.p, 8 * (size_t)nf * n_nodes,
                             hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[4], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  for (int i = 0; i < 4; ++i) c.pl_ms[i] = pl_ms_between(ev.e[i], ev.e[i + 1]);
  if (reused) c.pl_ms[0] = 0.0;
  const unsigned long long* h = c.pl_host.as<unsigned long long>();
  const unsigned flag = (unsigned)(h[words - 1] & 0xFFFFFFFFull);
  if (flag & 1u) CDR_FAIL(CDR_ERR_ARG, "place: a label outside [0, k)");
  if (flag & 2u) CDR_FAIL(CDR_ERR_ARG, "place: negative size");
  if (flag & 4u) CDR_FAIL(CDR_ERR_ARG, "place: a factor outside [0, R]");
  memcpy(cluster_sums, h, 8 * 3 * (size_t)k);
  memcpy(node_sums, h + 3 * (size_t)k, 8 * 3 * (size_t)n_nodes);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_place_replicas(cdr_ctx* h, int32_t n_nodes, const int64_t* labels, int64_t n_labels,
                       int32_t k, const int32_t* factors, int32_t R, const int64_t* sizes,
                       int32_t* nodes_out, int64_t* per_file_out, int64_t* counts_out,
                       uint64_t* cluster_sums, uint64_t* node_sums) {
  CDR_TRY
  if (!h || !factors || !cluster_sums || !node_sums)
    CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  place_replicas(h->c, n_nodes, labels, n_labels, k, factors, R, sizes, nodes_out, per_file_out,
                 counts_out, cluster_sums, node_sums);
  CDR_CATCH
}

int cdr_place_info(cdr_ctx* h, int64_t* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 6; ++i) out[i] = h->c.pl_info[i];
  CDR_CATCH
}

int cdr_place_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = h->c.pl_ms[i];
  CDR_CATCH
}

}  // extern "C"
