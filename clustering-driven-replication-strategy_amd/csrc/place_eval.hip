// place_eval.hip — how local a GIVEN placement is under the resident events,
// and what it costs (an extension with no reference
// counterpart).  The placement is a host table nodes[n_files][R] with entries
// in [-1, n_nodes); place.hip chooses one, this file judges any.
//
//   place_eval_files          one thread per file: the file's 16-byte record
//                             {mask (u64), first, label | copies << 16} from
//                             its row and label, and the replicas per node
//   place_eval_events<bool>   persistent: every lane reads ev_file, ev_client
//                             and ev_op with kPeUnroll loads in flight, gathers
//                             the file's record, forms `in` and adds into the
//                             workgroup's LDS tables [6 k] and [4 n_nodes] of
//                             uint64, flushed once with global uint64 adds;
//                             <true> also adds {total, local} into a zeroed
//                             uint32 [n_files][2] table (no-return atomics)
//
// With few nodes or clusters all 64 lanes of a wave add to a handful of LDS
// counters.  Keeping each table in up to 32 copies (lane l adding into copy
// l mod 32) was measured against the plain tables and changed nothing (DESIGN
// §13.4), so the tables are plain.  The counters are uint64 in LDS as in HBM,
// so no share of a column can overflow.  Integers only: the results do not
// depend on the order of the adds.
//
// A label outside [0, k) or a node entry outside [-1, n_nodes) raises a flag
// and is never used as an index or a shift count; a client code that is no
// node (negative, or >= n_nodes) is compared before it is shifted by; rows >=
// ev_n are never read.
#include "cdr_internal.h"

#include <algorithm>

namespace cdr {

namespace {

constexpr int kPeWaves = 4;           // waves per workgroup
constexpr int kPeUnroll = 8;          // events in flight per lane
constexpr int kPeWaveChunk = 64 * kPeUnroll;          // events of one wave and sweep
constexpr int kPeChunk = kPeWaves * kPeWaveChunk;     // of one workgroup and sweep
constexpr int kPeFileBlock = 256;
constexpr int kPeMaxNodes = 64;
constexpr int kPeMaxK = 1024;
constexpr int kPeMaxR = 8;
constexpr unsigned kPeNoLabel = 0xFFFFu;  // label field of a file whose label is out of range
constexpr int kOpWrite = 1, kOpRead = 2;

struct alignas(16) PeRec {
  unsigned long long mask;  // bit j: node j holds a replica
  int first;                // the first entry >= 0 of the row, -1 without one
  unsigned lc;              // label | copies << 16
};
static_assert(sizeof(PeRec) == 16, "one 16-byte gather per event");

__global__ __launch_bounds__(kPeFileBlock) void place_eval_files(
    const int32_t* __restrict__ nodes, const int32_t* __restrict__ labels, int64_t nf, int n_nodes,
    int R, int k, PeRec* __restrict__ rec, unsigned long long* __restrict__ nsum,
    int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  unsigned long long rep = 0;  // lane j: the files of this wave with node j
  int bad = 0;
  const int64_t stride = (int64_t)gridDim.x * kPeFileBlock;
  const int64_t nf_up = (nf + 63) & ~(int64_t)63;  // whole waves run the ballots
  for (int64_t f = (int64_t)blockIdx.x * kPeFileBlock + threadIdx.x; f < nf_up; f += stride) {
    unsigned long long mask = 0;
    if (f < nf) {
      int first = -1;
      for (int s = 0; s < R; ++s) {
        const int v = nodes[f * R + s];
        if (v >= 0 && v < n_nodes) {
          mask |= 1ull << v;
          if (first < 0) first = v;
        } else if (v != -1) {
          bad |= 2;
        }
      }
      unsigned lab = (unsigned)labels[f];
      if (lab >= (unsigned)k) {
        bad |= 1;
        lab = kPeNoLabel;
      }
      PeRec r;
      r.mask = mask;
      r.first = first;
      r.lc = lab | ((unsigned)__popcll(mask) << 16);
      rec[f] = r;
    }
    for (int j = 0; j < n_nodes; ++j) {
      const unsigned long long b = __ballot((mask >> j) & 1ull);
      if (lane == j) rep += (unsigned long long)__popcll(b);
    }
  }
  if (lane < n_nodes && rep) atomicAdd(&nsum[5 * lane + 4], rep);
  if (bad) atomicOr(flag, bad);
}

struct PeArgs {
  const int32_t* file;
  const int32_t* client;
  const uint8_t* op;
  const PeRec* rec;
  int64_t ne, nf;
  int n_nodes, k;
  unsigned* per_file;        // [nf][2], zeroed (kPerFile)
  unsigned long long* csum;  // [k][6], zeroed
  unsigned long long* nsum;  // [n_nodes][5]: columns 0..3 zeroed, 4 from the file pass
};

template <bool kPerFile>
__global__ __launch_bounds__(64 * kPeWaves) void place_eval_events(PeArgs a) {
  extern __shared__ unsigned long long pe_lds[];
  const int lane = threadIdx.x & 63;
  const int ncw = 6 * a.k, nnw = 4 * a.n_nodes;
  unsigned long long* lc = pe_lds;        // [k][6]
  unsigned long long* ln = pe_lds + ncw;  // [n_nodes][4]
  for (int t = threadIdx.x; t < ncw + nnw; t += blockDim.x) pe_lds[t] = 0ull;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kPeChunk;
  for (int64_t base = (int64_t)blockIdx.x * kPeChunk + (threadIdx.x >> 6) * kPeWaveChunk;
       base < a.ne; base += stride) {
    int f[kPeUnroll], cl[kPeUnroll], o[kPeUnroll];
#pragma unroll
    for (int u = 0; u < kPeUnroll; ++u) {
      const int64_t e = base + u * 64 + lane;
      const bool ok = e < a.ne;
      f[u] = ok ? a.file[e] : -1;
      cl[u] = ok ? a.client[e] : -1;
      o[u] = ok ? (int)a.op[e] : 0;
    }
    PeRec r[kPeUnroll];
#pragma unroll
    for (int u = 0; u < kPeUnroll; ++u) {
      const bool ok = f[u] >= 0 && f[u] < a.nf;  // (a row >= ev_n has f = -1)
      PeRec z;
      z.mask = 0ull;
      z.first = -1;
      z.lc = kPeNoLabel;
      r[u] = ok ? a.rec[f[u]] : z;
      if (!ok) f[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < kPeUnroll; ++u) {
      if (f[u] < 0) continue;
      const int c = cl[u];
      const bool node = c >= 0 && c < a.n_nodes;
      const bool in = node && ((r[u].mask >> (c & 63)) & 1ull);
      const bool rd = o[u] == kOpRead, wr = o[u] == kOpWrite;
      if (kPerFile) {
        atomicAdd(&a.per_file[2 * (int64_t)f[u]], 1u);
        if (in) atomicAdd(&a.per_file[2 * (int64_t)f[u] + 1], 1u);
      }
      const unsigned lab = r[u].lc & 0xFFFFu;
      if (lab < (unsigned)a.k) {
        unsigned long long* row = lc + 6 * lab;
        atomicAdd(&row[0], 1ull);
        if (in) atomicAdd(&row[1], 1ull);
        if (rd) {
          atomicAdd(&row[2], 1ull);
          if (in) atomicAdd(&row[3], 1ull);
        }
        if (wr) {
          atomicAdd(&row[4], 1ull);
          const unsigned copies = r[u].lc >> 16;
          if (copies) atomicAdd(&row[5], (unsigned long long)copies);
        }
      }
      if (node) {
        atomicAdd(&ln[4 * c], 1ull);
        if (in) atomicAdd(&ln[4 * c + 1], 1ull);
      }
      if (rd) {
        const int srv = in ? c : r[u].first;  // first is -1 or a checked node id
        if (srv >= 0) atomicAdd(&ln[4 * srv + 2], 1ull);
      }
      if (wr) {
        unsigned long long m = r[u].mask;  // only bits below n_nodes are ever set
        while (m) {
          const int j = __ffsll((long long)m) - 1;
          m &= m - 1;
          atomicAdd(&ln[4 * j + 3], 1ull);
        }
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < ncw; t += blockDim.x)
    if (lc[t]) atomicAdd(&a.csum[t], lc[t]);
  for (int t = threadIdx.x; t < nnw; t += blockDim.x)
    if (ln[t]) atomicAdd(&a.nsum[5 * (t >> 2) + (t & 3)], ln[t]);
}

struct PeEvents {
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~PeEvents() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

template <bool kPerFile>
int launch_events(Ctx& c, const PeArgs& a, size_t lds) {
  const void* fn = reinterpret_cast<const void*>(&place_eval_events<kPerFile>);
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * kPeWaves, lds));
  per_cu = std::max(1, per_cu);
  const int grid = (int)std::min<int64_t>(ceil_div(a.ne, (int64_t)kPeChunk),
                                          (int64_t)lloyd_num_cus(c.device) * per_cu);
  hipLaunchKernelGGL(place_eval_events<kPerFile>, dim3(grid), dim3(64 * kPeWaves), lds, c.stream,
                     a);
  HIP_CHECK(hipGetLastError());
  return grid;
}

}  // namespace

void place_evaluate(Ctx& c, int32_t n_nodes, const int32_t* nodes, int32_t R,
                    const int64_t* labels, int64_t n_labels, int32_t k, int64_t* per_file_out,
                    uint64_t* cluster_sums, uint64_t* node_sums) {
  if (n_nodes < 1 || n_nodes > kPeMaxNodes)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "place_evaluate: n_nodes outside [1, 64]");
  if (k < 1 || k > kPeMaxK) CDR_FAIL(CDR_ERR_UNSUPPORTED, "place_evaluate: k outside [1, 1024]");
  if (R < 1 || R > kPeMaxR) CDR_FAIL(CDR_ERR_ARG, "place_evaluate: R outside [1, 8]");
  if (c.ev_nf <= 0 || c.ev_foreign) CDR_FAIL(CDR_ERR_STATE, "place_evaluate: no resident events");
  const int64_t ne = c.ev_n, nf = c.ev_nf;
  if (ne >= (1ll << 32))
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "place_evaluate: 2^32 or more resident events");
  if (labels) {
    if (n_labels != nf)
      CDR_FAIL(CDR_ERR_ARG, "place_evaluate: n_labels is not the events' n_files");
  } else {
    if (!c.have_labels)
      CDR_FAIL(CDR_ERR_STATE,
               "place_evaluate: no labels on the device: run a Lloyd step or pass labels");
    if (c.n != nf)
      CDR_FAIL(CDR_ERR_ARG, "place_evaluate: the resident labels' row count is not n_files");
    if (k < c.last_k)
      CDR_FAIL(CDR_ERR_ARG, "place_evaluate: k smaller than the resident labels' k");
  }
  // pinned staging: the nodes table, then the labels as int32
  const size_t node_bytes = sizeof(int32_t) * (size_t)nf * R;
  c.pe_stage.ensure(node_bytes + sizeof(int32_t) * (size_t)nf);
  int32_t* hn = c.pe_stage.as<int32_t>();
  int32_t* hl = hn + (size_t)nf * R;
  for (int64_t i = 0; i < nf * R; ++i) {
    if (nodes[i] < -1 || nodes[i] >= n_nodes)
      CDR_FAIL(CDR_ERR_ARG, "place_evaluate: a node entry outside [-1, n_nodes)");
    hn[i] = nodes[i];
  }
  if (labels)
    for (int64_t i = 0; i < nf; ++i) {
      if (labels[i] < 0 || labels[i] >= k)
        CDR_FAIL(CDR_ERR_ARG, "place_evaluate: a label outside [0, k)");
      hl[i] = (int32_t)labels[i];
    }
  c.pe_info[0] = -1;
  c.pe_info[1] = c.pe_info[2] = 0;
  for (double& v : c.pe_ms) v = 0.0;
  PeEvents ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  // uploads and zeroing
  c.pe_nodes.ensure(node_bytes);
  HIP_CHECK(hipMemcpyAsync(c.pe_nodes.p, hn, node_bytes, hipMemcpyHostToDevice, c.stream));
  if (labels) {
    c.pe_lab.ensure(sizeof(int32_t) * (size_t)nf);
    HIP_CHECK(hipMemcpyAsync(c.pe_lab.p, hl, sizeof(int32_t) * (size_t)nf, hipMemcpyHostToDevice,
                             c.stream));
  }
  c.pe_rec.ensure(sizeof(PeRec) * (size_t)nf);
  const size_t words = 6 * (size_t)k + 5 * (size_t)n_nodes + 1;  // cluster sums, node sums, flag
  const size_t pf_bytes = per_file_out ? sizeof(unsigned) * 2 * (size_t)nf : 0;
  c.pe_sum.ensure(8 * words);
  c.pe_host.ensure(8 * words + pf_bytes);
  HIP_CHECK(hipMemsetAsync(c.pe_sum.p, 0, 8 * words, c.stream));
  if (per_file_out) {
    c.pe_pf.ensure(pf_bytes);
    HIP_CHECK(hipMemsetAsync(c.pe_pf.p, 0, pf_bytes, c.stream));
  }
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  unsigned long long* csum = c.pe_sum.as<unsigned long long>();
  unsigned long long* nsum = csum + 6 * (size_t)k;
  int* flag = reinterpret_cast<int*>(csum + words - 1);
  const int cus = lloyd_num_cus(c.device);
  {
    const int grid = (int)std::min<int64_t>(ceil_div(nf, (int64_t)kPeFileBlock), (int64_t)8 * cus);
    hipLaunchKernelGGL(place_eval_files, dim3(grid), dim3(kPeFileBlock), 0, c.stream,
                       c.pe_nodes.as<int32_t>(),
                       labels ? c.pe_lab.as<int32_t>() : c.labels.as<int32_t>(), nf, (int)n_nodes,
                       (int)R, (int)k, c.pe_rec.as<PeRec>(), nsum, flag);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
  PeArgs a;
  a.file = c.ev_file.as<int32_t>();
  a.client = c.ev_client.as<int32_t>();
  a.op = c.ev_op.as<uint8_t>();
  a.rec = c.pe_rec.as<PeRec>();
  a.ne = ne;
  a.nf = nf;
  a.n_nodes = n_nodes;
  a.k = k;
  a.per_file = per_file_out ? c.pe_pf.as<unsigned>() : nullptr;
  a.csum = csum;
  a.nsum = nsum;
  int grid = 0;
  if (ne > 0) {
    const size_t lds = 8 * ((size_t)6 * k + (size_t)4 * n_nodes);  // <= 50 KiB
    grid = per_file_out ? launch_events<true>(c, a, lds) : launch_events<false>(c, a, lds);
  }
  c.pe_info[1] = grid;
  c.pe_info[2] = kPeChunk;
  HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
  unsigned long long* h = c.pe_host.as<unsigned long long>();
  HIP_CHECK(hipMemcpyAsync(h, c.pe_sum.p, 8 * words, hipMemcpyDeviceToHost, c.stream));
  if (per_file_out)
    HIP_CHECK(hipMemcpyAsync(h + words, c.pe_pf.p, pf_bytes, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[4], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  for (int i = 0; i < 4; ++i) {
    float v = 0.f;
    (void)hipEventElapsedTime(&v, ev.e[i], ev.e[i + 1]);
    c.pe_ms[i] = v;
  }
  c.pe_info[0] = per_file_out ? 1 : 0;
  const unsigned flg = (unsigned)(h[words - 1] & 0xFFFFFFFFull);
  if (flg & 1u) CDR_FAIL(CDR_ERR_ARG, "place_evaluate: a label outside [0, k)");
  if (flg & 2u) CDR_FAIL(CDR_ERR_ARG, "place_evaluate: a node entry outside [-1, n_nodes)");
  memcpy(cluster_sums, h, 8 * 6 * (size_t)k);
  memcpy(node_sums, h + 6 * (size_t)k, 8 * 5 * (size_t)n_nodes);
  if (per_file_out) {
    const unsigned* pf = reinterpret_cast<const unsigned*>(h + words);
    for (int64_t i = 0; i < 2 * nf; ++i) per_file_out[i] = (int64_t)pf[i];
  }
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_place_evaluate(cdr_ctx* h, int32_t n_nodes, const int32_t* nodes, int32_t R,
                       const int64_t* labels, int64_t n_labels, int32_t k, int64_t* per_file_out,
                       uint64_t* cluster_sums, uint64_t* node_sums) {
  CDR_TRY
  if (!h || !nodes || !cluster_sums || !node_sums) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  place_evaluate(h->c, n_nodes, nodes, R, labels, n_labels, k, per_file_out, cluster_sums,
                 node_sums);
  CDR_CATCH
}

int cdr_place_evaluate_info(cdr_ctx* h, int64_t* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 3; ++i) out[i] = h->c.pe_info[i];
  CDR_CATCH
}

int cdr_place_evaluate_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = h->c.pe_ms[i];
  CDR_CATCH
}

}  // extern "C"
