// quality.hip — cluster validity indices of the resident points: silhouette
// and the per-cluster scatter of Davies-Bouldin.  No reference counterpart
// (the reference fixes k = 4, src/main.py); the distance is the reference's
// own, np.linalg.norm(x - y) (src/kmeans_plusplus.py:33): the difference form
// sqrt(sum_f (x_f - y_f)^2) in fp64, never the Gram form (whose cancellation
// gives coincident points a distance of ~1e-8 instead of 0).
//
// Silhouette of m sample rows: the rows are gathered to fp64 row-major in
// label order (the labels are counted and ranked on the host: m <= 2^20
// integers), and the pair kernel gives every thread one or two of those rows,
// held in registers, and walks the column points in label order, kQColTile at
// a time staged in LDS (every lane reads the same address: a broadcast, no bank
// conflict).  Per row it keeps one running sum of sqrt(q) for the cluster
// segment the columns are in; at the segment's end the mean is folded into
// a_i (the row's own cluster, divided by c - 1: d(i, i) = 0 exactly is part of
// the sum) or min b_i, so no m x k table exists.  A column tile is read up to
// its count of real columns, never further: padding contributes nothing.  To
// fill the device at any m the columns are cut into parts of whole tiles
// (gridDim.y); a part leaves four numbers per row and q_combine folds the
// parts in part order.  No atomics; the order of every sum depends on the
// shape only, so the output is bit-identical on every run.
//
// Davies-Bouldin scatter: one pass over x32 / x64 with the labels; a workgroup
// takes chunks of kQsChunk points, leaves their distances to their own
// centroids in LDS, and thread j then adds the chunk's distances of cluster j
// (of its slice of the chunk) in point order into a register (its chunks come
// in a fixed order, the grid depends on n only); the per-workgroup partials are
// added in workgroup order.
#include <algorithm>
#include <cmath>

#include "cdr_internal.h"

namespace cdr {

constexpr int kQThreads = 128;   // threads of a pair workgroup
constexpr int kQColTile = 64;    // column points per LDS tile
constexpr int kQRowPad = 256;    // the largest row tile (kQThreads * 2)
constexpr int kQMaxD = 64;
constexpr int kQMaxK = 1024;
constexpr int64_t kQMaxM = 1ll << 20;
// Pairs (rows x m columns) of one pair-kernel launch: the row range is split
// so that no launch runs long on a shared device (DESIGN §11 has the time of
// one budget-sized launch).
constexpr int64_t kQPairBudget = 1ll << 33;

// Column parts per launch: enough for kQFillGroups workgroups (two waves on
// every SIMD of 256 CUs), at least kQMinPartTiles column tiles each, at most
// kQMaxParts.  A function of the shape only, so the sums' order is fixed.
constexpr int kQFillGroups = 1024;
constexpr int kQMinPartTiles = 4;
constexpr int kQMaxParts = 64;

constexpr int kQsChunk = 1024;  // points per scatter chunk (256 threads x 4)
constexpr int kQsGrid = 1024;   // most scatter workgroups (fixed: the order of the partials)
constexpr int kQsLdsC = 6144;   // centroids of up to this many doubles live in LDS

// rows of the sample in label order, fp64 row-major [m_pad][DP] (features
// >= d and rows >= m are zero)
template <typename V>
__global__ void q_gather(const V* __restrict__ X, int64_t n_pad, int d, int DP,
                         const int64_t* __restrict__ rows, int64_t m, int64_t m_pad,
                         double* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m_pad * DP;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = t / DP;
    const int f = (int)(t - p * DP);
    out[t] = (p < m && f < d) ? (double)X[xidx(X, f, rows[p], n_pad)] : 0.0;
  }
}

__global__ void q_gather_labels(const int32_t* __restrict__ labels,
                                const int64_t* __restrict__ idx, int64_t m,
                                int32_t* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m;
       t += (int64_t)gridDim.x * blockDim.x)
    out[t] = labels[idx ? idx[t] : t];
}

// Rows [row0 + blockIdx.x * kQThreads * R, ...) of the label-sorted sample
// against the columns of part blockIdx.y: column tiles [p nt / P, (p + 1) nt / P)
// of the nt tiles.  segoff[0 .. nseg] are the starts of the non-empty cluster
// segments (segoff[nseg] = m, segoff[nseg + 1] = never reached), rowseg[p] the
// segment of sorted row p, pinfo[2 p], pinfo[2 p + 1] the segments of the part's
// first and last column.  Per (row, part) four values go to `part`: the sum
// over the part's columns of its first segment, the same for its last segment
// (when that is another one), the smallest mean over the segments in between
// other than the row's own, and the sum over the row's own segment when it is
// one of those in between.  q_combine folds the parts in part order.
template <int DP, int R>
__global__ __launch_bounds__(kQThreads) void q_pairs(const double* __restrict__ Xs, int64_t m,
                                                     int64_t row0,
                                                     const int32_t* __restrict__ rowseg,
                                                     const int64_t* __restrict__ segoff,
                                                     const int32_t* __restrict__ pinfo,
                                                     double* __restrict__ part) {
  __shared__ double tile[kQColTile * DP];
  const int64_t rloc = (int64_t)blockIdx.x * (kQThreads * R) + threadIdx.x;
  const int P = gridDim.y, pi = blockIdx.y;
  const int64_t nt = (m + kQColTile - 1) / kQColTile;
  const int64_t c_begin = (nt * pi / P) * kQColTile;
  const int64_t c_end = min(m, (nt * (pi + 1) / P) * kQColTile);
  const int sf = pinfo[2 * pi], sl = pinfo[2 * pi + 1];
  double x[R][DP];
  int own[R];
  double acc[R], first[R], last[R], mid[R], osum[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const int64_t r = row0 + rloc + (int64_t)t * kQThreads;  // < m_pad: the buffer is padded
#pragma unroll
    for (int f = 0; f < DP; ++f) x[t][f] = Xs[r * DP + f];
    own[t] = r < m ? rowseg[r] : -1;
    acc[t] = 0.0;
    first[t] = 0.0;
    last[t] = 0.0;
    mid[t] = INFINITY;
    osum[t] = 0.0;
  }
  int s = sf;
  int64_t send = segoff[s + 1];
  for (int64_t c0 = c_begin; c0 < c_end; c0 += kQColTile) {
    const int nc = (int)min((int64_t)kQColTile, c_end - c0);  // real columns of this tile
    __syncthreads();
    for (int i = threadIdx.x; i < nc * DP; i += kQThreads) tile[i] = Xs[c0 * DP + i];
    __syncthreads();
    int j = 0;
    while (j < nc) {
      const int je = (int)min((int64_t)nc, send - c0);
#pragma unroll 2
      for (; j < je; ++j) {
        double q[R];
#pragma unroll
        for (int t = 0; t < R; ++t) q[t] = 0.0;
#pragma unroll
        for (int f = 0; f < DP; ++f) {
          const double y = tile[j * DP + f];
#pragma unroll
          for (int t = 0; t < R; ++t) {
            const double df = x[t][f] - y;
            q[t] = fma(df, df, q[t]);
          }
        }
#pragma unroll
        for (int t = 0; t < R; ++t) acc[t] += sqrt(q[t]);
      }
      const bool seg_done = c0 + j == send;
      if (seg_done || c0 + j == c_end) {  // the segment, or this part's share of it, is complete
        const double cnt = (double)(send - segoff[s]);
#pragma unroll
        for (int t = 0; t < R; ++t) {
          if (s == sf) {
            first[t] = acc[t];
          } else if (s == sl) {
            last[t] = acc[t];
          } else if (s == own[t]) {
            osum[t] = acc[t];
          } else {
            const double mean = acc[t] / cnt;
            mid[t] = mean < mid[t] ? mean : mid[t];
          }
          acc[t] = 0.0;
        }
        if (seg_done) {
          ++s;
          send = segoff[s + 1];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < R; ++t) {
    double* o = part + ((rloc + (int64_t)t * kQThreads) * P + pi) * 4;
    o[0] = first[t];
    o[1] = last[t];
    o[2] = mid[t];
    o[3] = osum[t];
  }
}

// s_i of rows [row0, row0 + nrows) from their P parts, in part order: the
// shares of a segment that spans parts are added left to right.
__global__ void q_combine(const double* __restrict__ part, int P, int64_t m, int64_t row0,
                          int64_t nrows, const int32_t* __restrict__ rowseg,
                          const int64_t* __restrict__ segoff, const int32_t* __restrict__ pinfo,
                          double* __restrict__ s_out) {
  const int64_t rl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (rl >= nrows || row0 + rl >= m) return;
  const int own = rowseg[row0 + rl];
  double a_sum = 0.0, b = INFINITY, carry = 0.0;
  int cseg = -1;
  auto close = [&](int seg, double sum) {
    if (seg == own) {
      a_sum = sum;
    } else {
      const double mean = sum / (double)(segoff[seg + 1] - segoff[seg]);
      b = mean < b ? mean : b;
    }
  };
  for (int p = 0; p < P; ++p) {
    const double* o = part + (rl * P + p) * 4;
    const int sf = pinfo[2 * p], sl = pinfo[2 * p + 1];
    if (sf != cseg) {
      if (cseg >= 0) close(cseg, carry);
      cseg = sf;
      carry = 0.0;
    }
    carry += o[0];
    if (sl != sf) {
      close(cseg, carry);
      b = o[2] < b ? o[2] : b;
      if (sf < own && own < sl) a_sum = o[3];
      cseg = sl;
      carry = o[1];
    }
  }
  close(cseg, carry);
  const int64_t cnt = segoff[own + 1] - segoff[own];
  const double a = cnt > 1 ? a_sum / (double)(cnt - 1) : 0.0;
  const double mx = a > b ? a : b;
  s_out[row0 + rl] = (cnt == 1 || !(mx > 0.0)) ? 0.0 : (b - a) / mx;
}

// ---- Davies-Bouldin scatter ------------------------------------------------
template <typename V, bool LDSC>
__global__ __launch_bounds__(256) void q_scatter(const V* __restrict__ X, int64_t n,
                                                 int64_t n_pad, int d,
                                                 const int32_t* __restrict__ labels,
                                                 const double* __restrict__ C, int k, int S,
                                                 double* __restrict__ psum,
                                                 long long* __restrict__ pcnt) {
  extern __shared__ double q_sh[];
  double* sd = q_sh;                                        // [kQsChunk] distances
  int* sl = reinterpret_cast<int*>(q_sh + kQsChunk);        // [kQsChunk] labels
  double* sC = q_sh + kQsChunk + kQsChunk / 2;              // [k * d] (LDSC)
  if (LDSC)
    for (int i = threadIdx.x; i < k * d; i += 256) sC[i] = C[i];
  double rs[4] = {0.0, 0.0, 0.0, 0.0};
  long long rc[4] = {0, 0, 0, 0};
  const int KP = 256 / S, len = kQsChunk / S;
  const int jq = threadIdx.x & (KP - 1), q = threadIdx.x / KP;
  const int64_t nchunks = (n + kQsChunk - 1) / kQsChunk;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    __syncthreads();
    const int64_t i0 = ch * kQsChunk;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int li = u * 256 + threadIdx.x;
      const int64_t i = i0 + li;
      double dist = 0.0;
      int lab = -1;
      if (i < n) {  // padding rows are skipped
        lab = labels[i];
        const double* cj = (LDSC ? sC : C) + (int64_t)lab * d;
        double qq = 0.0;
        if constexpr (sizeof(V) == 4) {
          for (int f0 = 0; f0 < d; f0 += 4) {
            const float4 v =
                *reinterpret_cast<const float4*>(&X[(((int64_t)(f0 >> 2) * n_pad) + i) * 4]);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (f0 + e < d) {
                const double df = (double)vv[e] - cj[f0 + e];
                qq = fma(df, df, qq);
              }
          }
        } else {
          for (int f = 0; f < d; ++f) {
            const double df = (double)X[xidx(X, f, i, n_pad)] - cj[f];
            qq = fma(df, df, qq);
          }
        }
        dist = sqrt(qq);
      }
      sd[li] = dist;
      sl[li] = lab;
    }
    __syncthreads();
    // cluster j's distances of this chunk, added in point order: for k <= 256
    // the chunk is cut into S = 256 / KP slices (KP = k rounded up to a power
    // of two) and thread (slice, j) adds its slice; for k > 256, S = 1 and a
    // thread has up to four clusters
    const int np = (int)min((int64_t)kQsChunk, n - i0);
    const int lo = q * len, hi = min(np, lo + len);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = u * 256 + jq;
      if (j < k) {
        double sacc = rs[u];
        long long cacc = rc[u];
#pragma unroll 4
        for (int i = lo; i < hi; ++i) {
          const bool hit = sl[i] == j;
          sacc += hit ? sd[i] : 0.0;  // + 0.0 leaves a non-negative sum as it is
          cacc += hit ? 1 : 0;
        }
        rs[u] = sacc;
        rc[u] = cacc;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = u * 256 + jq;
    if (j < k) {
      psum[((int64_t)blockIdx.x * S + q) * k + j] = rs[u];
      pcnt[((int64_t)blockIdx.x * S + q) * k + j] = rc[u];
    }
  }
}

__global__ void q_scatter_reduce(const double* __restrict__ psum,
                                 const long long* __restrict__ pcnt, int nparts, int k,
                                 double* __restrict__ sums, long long* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  long long c = 0;
  for (int b = 0; b < nparts; ++b) {  // workgroup order
    s += psum[(int64_t)b * k + j];
    c += pcnt[(int64_t)b * k + j];
  }
  sums[j] = s;
  counts[j] = c;
}

// ---- host side -------------------------------------------------------------
namespace {

struct Carve {  // sub-buffers of one device allocation, 256-byte aligned
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t at = total;
    total += (bytes + 255) & ~(size_t)255;
    return at;
  }
};

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
};

void check_state(const Ctx& c, bool resident_labels, int32_t k) {
  if (c.mode == 0 || c.n <= 0) CDR_FAIL(CDR_ERR_STATE, "quality: no points loaded");
  if (resident_labels && !c.have_labels)
    CDR_FAIL(CDR_ERR_STATE, "quality: no labels on the device: run a Lloyd step or pass labels");
  if (c.d < 1 || c.d > kQMaxD) CDR_FAIL(CDR_ERR_UNSUPPORTED, "quality: d outside [1, 64]");
  if (k > kQMaxK) CDR_FAIL(CDR_ERR_UNSUPPORTED, "quality: k > 1024");
  if (k < 1) CDR_FAIL(CDR_ERR_ARG, "quality: k < 1");
  if (resident_labels && k < c.last_k)
    CDR_FAIL(CDR_ERR_ARG, "quality: k smaller than the resident labels' k");
}

template <int DP, int R>
void launch_pairs(Ctx& c, const double* Xs, int64_t m, int64_t row0, int64_t nrows, int P,
                  const int32_t* rowseg, const int64_t* segoff, const int32_t* pinfo,
                  double* part) {
  const int64_t tile = (int64_t)kQThreads * R;
  hipLaunchKernelGGL((q_pairs<DP, R>), dim3((unsigned)ceil_div(nrows, tile), (unsigned)P),
                     dim3(kQThreads), 0, c.stream, Xs, m, row0, rowseg, segoff, pinfo, part);
}

}  // namespace

static int quality_dp(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }
static int quality_row_tile(int d) { return quality_dp(d) <= 32 ? kQThreads * 2 : kQThreads; }

void quality_silhouette(Ctx& c, const int64_t* idx, int64_t m, const int64_t* labels, int32_t k,
                        double* s, double* cluster_sum, int64_t* cluster_count) {
  check_state(c, labels == nullptr, k);
  if (m < 2 || m > kQMaxM) CDR_FAIL(CDR_ERR_ARG, "silhouette: m outside [2, 2^20]");
  if (!idx && m != c.n) CDR_FAIL(CDR_ERR_ARG, "silhouette: idx == NULL means all rows: m must be n");
  if (idx)
    for (int64_t i = 0; i < m; ++i)
      if (idx[i] < 0 || idx[i] >= c.n) CDR_FAIL(CDR_ERR_ARG, "silhouette: row index out of range");
  const int d = c.d, DP = quality_dp(d);
  const int64_t m_pad = ceil_div(m, kQRowPad) * kQRowPad;
  // the row range is split by the pair budget, the columns into P parts
  const int64_t tile = quality_row_tile(d);
  // (CDR_QUALITY_BUDGET: a smaller budget, for tests of the split at small m)
  int64_t budget = kQPairBudget;
  if (const char* e = std::getenv("CDR_QUALITY_BUDGET"))
    budget = std::min<int64_t>(kQPairBudget, std::max<int64_t>(1, std::atoll(e)));
  const int64_t rows_per = std::max<int64_t>(tile, budget / m / tile * tile);
  const int64_t nt = ceil_div(m, kQColTile);
  const int P = (int)std::max<int64_t>(
      1, std::min<int64_t>({ceil_div(kQFillGroups, ceil_div(std::min(rows_per, m), tile)),
                            nt / kQMinPartTiles, (int64_t)kQMaxParts}));

  Carve cv;
  const size_t o_rows = cv.take(sizeof(int64_t) * m);
  const size_t o_lab = cv.take(sizeof(int32_t) * m_pad);  // sample labels, then rowseg
  const size_t o_seg = cv.take(sizeof(int64_t) * (k + 2));
  const size_t o_s = cv.take(sizeof(double) * m_pad);
  const size_t o_x = cv.take(sizeof(double) * m_pad * DP);
  const size_t o_pinfo = cv.take(sizeof(int32_t) * 2 * P);
  const size_t o_part =
      cv.take(sizeof(double) * 4 * P * (size_t)(ceil_div(std::min(rows_per, m), tile) * tile));
  c.q_buf.ensure(cv.total);
  char* base = c.q_buf.as<char>();
  int64_t* d_rows = reinterpret_cast<int64_t*>(base + o_rows);
  int32_t* d_lab = reinterpret_cast<int32_t*>(base + o_lab);
  int64_t* d_seg = reinterpret_cast<int64_t*>(base + o_seg);
  double* d_s = reinterpret_cast<double*>(base + o_s);
  double* d_x = reinterpret_cast<double*>(base + o_x);
  int32_t* d_pinfo = reinterpret_cast<int32_t*>(base + o_pinfo);
  double* d_part = reinterpret_cast<double*>(base + o_part);

  // the sample's labels on the host
  std::vector<int32_t> lab(m);
  if (labels) {
    for (int64_t i = 0; i < m; ++i) {
      if (labels[i] < 0 || labels[i] >= k) CDR_FAIL(CDR_ERR_ARG, "silhouette: label outside [0, k)");
      lab[i] = (int32_t)labels[i];
    }
  } else {
    if (idx)
      HIP_CHECK(hipMemcpyAsync(d_rows, idx, sizeof(int64_t) * m, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(q_gather_labels, dim3((unsigned)std::min<int64_t>(ceil_div(m, 256), 4096)),
                       dim3(256), 0, c.stream, c.labels.as<int32_t>(), idx ? d_rows : nullptr, m,
                       d_lab);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(lab.data(), d_lab, sizeof(int32_t) * m, hipMemcpyDeviceToHost,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }

  // stable counting sort by label; the non-empty clusters become segments
  std::vector<int64_t> cnt(k, 0), start(k + 1, 0);
  for (int64_t i = 0; i < m; ++i) ++cnt[lab[i]];
  std::vector<int32_t> seg_of(k, -1);
  std::vector<int64_t> segoff;
  int nseg = 0;
  for (int j = 0; j < k; ++j) {
    start[j + 1] = start[j] + cnt[j];
    if (cnt[j] > 0) {
      seg_of[j] = nseg++;
      segoff.push_back(start[j]);
    }
  }
  if (nseg < 2 || nseg > m - 1)
    CDR_FAIL(CDR_ERR_ARG, "silhouette: the number of non-empty clusters is " +
                              std::to_string(nseg) + "; it must be in [2, m - 1]");
  segoff.push_back(m);
  segoff.push_back(INT64_MAX);
  std::vector<int64_t> perm(m), rows(m), cur(start.begin(), start.end() - 1);
  std::vector<int32_t> rowseg(m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t p = cur[lab[i]]++;
    perm[p] = i;
    rows[p] = idx ? idx[i] : i;
    rowseg[p] = seg_of[lab[i]];
  }
  HIP_CHECK(hipMemcpyAsync(d_rows, rows.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice,
                           c.stream));
  HIP_CHECK(hipMemcpyAsync(d_lab, rowseg.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice,
                           c.stream));
  HIP_CHECK(hipMemcpyAsync(d_seg, segoff.data(), sizeof(int64_t) * segoff.size(),
                           hipMemcpyHostToDevice, c.stream));
  std::vector<int32_t> pinfo(2 * P);  // segments of every part's first and last column
  for (int p = 0; p < P; ++p) {
    const int64_t cb = nt * p / P * kQColTile;
    const int64_t ce = std::min(m, nt * (p + 1) / P * kQColTile);
    pinfo[2 * p] = rowseg[cb];
    pinfo[2 * p + 1] = rowseg[ce - 1];
  }
  HIP_CHECK(hipMemcpyAsync(d_pinfo, pinfo.data(), sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice,
                           c.stream));
  const unsigned ggrid = (unsigned)std::min<int64_t>(ceil_div(m_pad * DP, 256), 8192);
  if (c.mode == CDR_MODE_F32X)
    hipLaunchKernelGGL(q_gather<float>, dim3(ggrid), dim3(256), 0, c.stream, c.x32.as<float>(),
                       c.n_pad, d, DP, d_rows, m, m_pad, d_x);
  else
    hipLaunchKernelGGL(q_gather<double>, dim3(ggrid), dim3(256), 0, c.stream, c.x64.as<double>(),
                       c.n_pad, d, DP, d_rows, m, m_pad, d_x);
  HIP_CHECK(hipGetLastError());

  std::vector<EventPair> evs;
  for (int64_t row0 = 0; row0 < m; row0 += rows_per) {
    const int64_t nrows = std::min(rows_per, m - row0);
    EventPair ev;
    HIP_CHECK(hipEventCreate(&ev.a));
    HIP_CHECK(hipEventCreate(&ev.b));
    evs.push_back(ev);
    HIP_CHECK(hipEventRecord(ev.a, c.stream));
    switch (DP) {
      case 4: launch_pairs<4, 2>(c, d_x, m, row0, nrows, P, d_lab, d_seg, d_pinfo, d_part); break;
      case 8: launch_pairs<8, 2>(c, d_x, m, row0, nrows, P, d_lab, d_seg, d_pinfo, d_part); break;
      case 16: launch_pairs<16, 2>(c, d_x, m, row0, nrows, P, d_lab, d_seg, d_pinfo, d_part); break;
      case 32: launch_pairs<32, 2>(c, d_x, m, row0, nrows, P, d_lab, d_seg, d_pinfo, d_part); break;
      default: launch_pairs<64, 1>(c, d_x, m, row0, nrows, P, d_lab, d_seg, d_pinfo, d_part); break;
    }
    hipLaunchKernelGGL(q_combine, dim3((unsigned)ceil_div(nrows, 256)), dim3(256), 0, c.stream,
                       d_part, P, m, row0, nrows, d_lab, d_seg, d_pinfo, d_s);
    HIP_CHECK(hipEventRecord(ev.b, c.stream));
  }
  hipError_t lerr = hipGetLastError();
  std::vector<double> ss(m);
  hipError_t cerr = hipMemcpyAsync(ss.data(), d_s, sizeof(double) * m, hipMemcpyDeviceToHost,
                                   c.stream);
  hipError_t serr = hipStreamSynchronize(c.stream);
  double total_ms = 0.0, max_ms = 0.0;
  for (EventPair& ev : evs) {
    float ms = 0.f;
    if (serr == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
      total_ms += ms;
      max_ms = std::max(max_ms, (double)ms);
    }
    (void)hipEventDestroy(ev.a);
    (void)hipEventDestroy(ev.b);
  }
  HIP_CHECK(lerr);
  HIP_CHECK(cerr);
  HIP_CHECK(serr);
  c.q_ms[0] = total_ms;
  c.q_ms[1] = max_ms;
  c.q_ms[2] = (double)evs.size();

  // caller's row order; per-cluster sums in sorted (= caller's, per cluster) order
  for (int j = 0; j < k; ++j) {
    double acc = 0.0;
    for (int64_t p = start[j]; p < start[j + 1]; ++p) acc += ss[p];
    if (cluster_sum) cluster_sum[j] = acc;
    if (cluster_count) cluster_count[j] = cnt[j];
  }
  for (int64_t p = 0; p < m; ++p) s[perm[p]] = ss[p];
}

void quality_scatter(Ctx& c, const double* C, int32_t k, const int64_t* labels, double* sums,
                     int64_t* counts) {
  check_state(c, labels == nullptr, k);
  const int d = c.d;
  const int64_t n = c.n;
  const int64_t nchunks = ceil_div(n, kQsChunk);
  const int grid = (int)std::min<int64_t>(nchunks, kQsGrid);
  int KP = 1;
  while (KP < k && KP < 256) KP <<= 1;
  const int S = 256 / KP;  // slices of a chunk (q_scatter)
  Carve cv;
  const size_t o_c = cv.take(sizeof(double) * (size_t)k * d);
  const size_t o_ps = cv.take(sizeof(double) * (size_t)grid * S * k);
  const size_t o_pc = cv.take(sizeof(long long) * (size_t)grid * S * k);
  const size_t o_out = cv.take(sizeof(double) * 2 * (size_t)k);
  const size_t o_lab = cv.take(labels ? sizeof(int32_t) * (size_t)n : 0);
  c.q_buf.ensure(cv.total);
  char* base = c.q_buf.as<char>();
  double* d_C = reinterpret_cast<double*>(base + o_c);
  double* d_ps = reinterpret_cast<double*>(base + o_ps);
  long long* d_pc = reinterpret_cast<long long*>(base + o_pc);
  double* d_sums = reinterpret_cast<double*>(base + o_out);
  long long* d_cnt = reinterpret_cast<long long*>(d_sums + k);
  const int32_t* d_lab = c.labels.as<int32_t>();
  std::vector<int32_t> lab;
  if (labels) {
    lab.resize(n);
    for (int64_t i = 0; i < n; ++i) {
      if (labels[i] < 0 || labels[i] >= k) CDR_FAIL(CDR_ERR_ARG, "scatter: label outside [0, k)");
      lab[i] = (int32_t)labels[i];
    }
    HIP_CHECK(hipMemcpyAsync(base + o_lab, lab.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice,
                             c.stream));
    d_lab = reinterpret_cast<const int32_t*>(base + o_lab);
  }
  HIP_CHECK(hipMemcpyAsync(d_C, C, sizeof(double) * (size_t)k * d, hipMemcpyHostToDevice,
                           c.stream));
  const bool ldsc = (int64_t)k * d <= kQsLdsC;
  const size_t lds = sizeof(double) * (kQsChunk + kQsChunk / 2 + (ldsc ? (size_t)k * d : 0));
  EventPair ev;
  HIP_CHECK(hipEventCreate(&ev.a));
  HIP_CHECK(hipEventCreate(&ev.b));
  (void)hipEventRecord(ev.a, c.stream);
  if (c.mode == CDR_MODE_F32X) {
    if (ldsc)
      hipLaunchKernelGGL((q_scatter<float, true>), dim3(grid), dim3(256), lds, c.stream,
                         c.x32.as<float>(), n, c.n_pad, d, d_lab, d_C, k, S, d_ps, d_pc);
    else
      hipLaunchKernelGGL((q_scatter<float, false>), dim3(grid), dim3(256), lds, c.stream,
                         c.x32.as<float>(), n, c.n_pad, d, d_lab, d_C, k, S, d_ps, d_pc);
  } else {
    if (ldsc)
      hipLaunchKernelGGL((q_scatter<double, true>), dim3(grid), dim3(256), lds, c.stream,
                         c.x64.as<double>(), n, c.n_pad, d, d_lab, d_C, k, S, d_ps, d_pc);
    else
      hipLaunchKernelGGL((q_scatter<double, false>), dim3(grid), dim3(256), lds, c.stream,
                         c.x64.as<double>(), n, c.n_pad, d, d_lab, d_C, k, S, d_ps, d_pc);
  }
  hipLaunchKernelGGL(q_scatter_reduce, dim3((unsigned)ceil_div(k, 256)), dim3(256), 0, c.stream,
                     d_ps, d_pc, grid * S, k, d_sums, d_cnt);
  hipError_t lerr = hipGetLastError();
  (void)hipEventRecord(ev.b, c.stream);
  hipError_t cerr = hipMemcpyAsync(sums, d_sums, sizeof(double) * k, hipMemcpyDeviceToHost,
                                   c.stream);
  if (cerr == hipSuccess)
    cerr = hipMemcpyAsync(counts, d_cnt, sizeof(long long) * k, hipMemcpyDeviceToHost, c.stream);
  hipError_t serr = hipStreamSynchronize(c.stream);
  float ms = 0.f;
  if (serr == hipSuccess) (void)hipEventElapsedTime(&ms, ev.a, ev.b);
  (void)hipEventDestroy(ev.a);
  (void)hipEventDestroy(ev.b);
  HIP_CHECK(lerr);
  HIP_CHECK(cerr);
  HIP_CHECK(serr);
  c.q_ms[3] = ms;
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_quality_silhouette(cdr_ctx* h, const int64_t* idx, int64_t m, const int64_t* labels,
                           int32_t k, double* s, double* cluster_sum, int64_t* cluster_count) {
  CDR_TRY
  if (!h || !s) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  quality_silhouette(h->c, idx, m, labels, k, s, cluster_sum, cluster_count);
  CDR_CATCH
}

int cdr_quality_scatter(cdr_ctx* h, const double* C, int32_t k, const int64_t* labels,
                        double* sums, int64_t* counts) {
  CDR_TRY
  if (!h || !C || !sums || !counts) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  quality_scatter(h->c, C, k, labels, sums, counts);
  CDR_CATCH
}

int cdr_quality_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = h->c.q_ms[i];
  CDR_CATCH
}

}  // extern "C"
