// agree.hip — the contingency table of two labelings of the same rows (DESIGN
// §12): T[a][b] = number of rows i with lab_a[i] == a and lab_b[i] == b, and
// with sizes the per-cell sums of the sizes' low 32 and high 31 bits (uint64
// each, as plan_size_sums has them: neither can overflow below 2^31 rows).
//
//   agree_lds<SIZES>     small tables: a per-workgroup table in LDS (uint32 counts,
//                        uint64 {low, high} sums), grid-stride over the rows, one
//                        flush of the non-zero cells per workgroup with global
//                        uint64 adds into the zeroed table
//   agree_global<SIZES>  up to 2^20 cells: no-return global uint64 adds straight
//                        into the zeroed table
//
// Both read kAgreeUnroll groups of 64 consecutive rows per wave and iteration
// (the loads of all groups are issued before the first add), and both add a
// group whose rows all fall into one cell once, from one lane (two labelings
// that agree put most groups there, and same-address atomics serialise).
// A label outside its range (bit 0) or a negative size (bit 1) sets *flag and
// adds nothing; no such value is ever used as an index.  Rows >= n are never
// read.  Integer adds only: the result does not depend on their order.
#include "cdr_internal.h"

#include <algorithm>

namespace cdr {

namespace {

constexpr int kAgreeMaxK = 1024;
constexpr int kAgreeLdsBlock = 1024;    // threads of agree_lds (16 waves)
constexpr int kAgreeGlobalBlock = 256;  // threads of agree_global
constexpr int kAgreeUnroll = 4;         // 64-row groups per wave and iteration
// LDS caps in cells.  Counts alone: 4 B per cell, 16384 cells = 64 KiB, two
// workgroups (32 waves) per CU.  With sizes: 20 B per cell, 4096 cells (k = 64
// against itself) = 80 KiB, two workgroups fill the CU's 160 KiB exactly.
constexpr int kAgreeCapCounts = 16384;
constexpr int kAgreeCapSizes = 4096;
constexpr int kAgreeLdsPerCu = 2;     // agree_lds workgroups launched per CU
constexpr int kAgreeGlobalPerCu = 8;  // agree_global workgroups launched per CU (32 waves)
constexpr int kAgreeLdsGridMax = 1024;

struct AgreeArgs {
  const int32_t* la;       // n labels in [0, ka)
  const int32_t* lb;       // n labels in [0, kb)
  const long long* sizes;  // n sizes >= 0 (SIZES only)
  int64_t n;
  int ka, kb;
  unsigned long long* cnt;    // [ka * kb], zeroed
  unsigned long long* sum;    // [ka * kb][2], zeroed (SIZES only)
  int* flag;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One group of 64 rows: lane's row is in the table (ok) at `cell` with size
// halves lo, hi.  CT is the count cell's type (uint32 in LDS, uint64 global).
template <bool SIZES, typename CT>
__device__ __forceinline__ void add_group(bool ok, int cell, unsigned long long lo,
                                          unsigned long long hi, CT* cnt,
                                          unsigned long long* sum) {
  const unsigned long long act = __ballot(ok);
  if (act == 0ull) return;
  const int first = __ffsll(act) - 1;
  const int c0 = __shfl(cell, first);
  if (__ballot(ok && cell != c0) == 0ull) {  // (the same on every lane)
    if (SIZES) {
      lo = wave_sum(ok ? lo : 0ull);  // 64 values below 2^32
      hi = wave_sum(ok ? hi : 0ull);
    }
    if ((int)(threadIdx.x & 63) == first) {
      atomicAdd(&cnt[c0], (CT)__popcll(act));
      if (SIZES) {
        if (lo) atomicAdd(&sum[2 * c0], lo);
        if (hi) atomicAdd(&sum[2 * c0 + 1], hi);
      }
    }
    return;
  }
  if (!ok) return;
  atomicAdd(&cnt[cell], (CT)1);
  if (SIZES) {
    if (lo) atomicAdd(&sum[2 * cell], lo);
    if (hi) atomicAdd(&sum[2 * cell + 1], hi);
  }
}

// The rows of one wave iteration: kAgreeUnroll groups from row `base` (the
// same on every lane of the wave).  Returns 1 for a label out of range, 2 for a
// negative size, 3 for both among the lane's rows.
template <bool SIZES, typename CT>
__device__ __forceinline__ int add_rows(const AgreeArgs& g, int64_t base, CT* cnt,
                                        unsigned long long* sum) {
  const int lane = threadIdx.x & 63;
  int a[kAgreeUnroll], b[kAgreeUnroll];
  long long s[kAgreeUnroll];
#pragma unroll
  for (int u = 0; u < kAgreeUnroll; ++u) {
    const int64_t i = base + u * 64 + lane;
    const bool in = i < g.n;
    a[u] = in ? g.la[i] : 0;
    b[u] = in ? g.lb[i] : 0;
    s[u] = (SIZES && in) ? g.sizes[i] : 0;
  }
  int bad = 0;
#pragma unroll
  for (int u = 0; u < kAgreeUnroll; ++u) {
    if (base + u * 64 >= g.n) break;  // (the same on every lane)
    const bool in = base + u * 64 + lane < g.n;
    const bool lab_ok = (unsigned)a[u] < (unsigned)g.ka && (unsigned)b[u] < (unsigned)g.kb;
    if (in && !lab_ok) bad |= 1;
    if (in && s[u] < 0) bad |= 2;
    const bool ok = in && lab_ok && s[u] >= 0;
    add_group<SIZES, CT>(ok, ok ? a[u] * g.kb + b[u] : 0, (unsigned long long)s[u] & 0xFFFFFFFFull,
                         (unsigned long long)s[u] >> 32, cnt, sum);
  }
  return bad;
}

template <bool SIZES>
__global__ __launch_bounds__(kAgreeLdsBlock) void agree_lds(AgreeArgs g) {
  extern __shared__ unsigned long long agree_sh[];  // SIZES: [cells][2] sums, then the counts
  const int cells = g.ka * g.kb;
  unsigned long long* sum = agree_sh;
  unsigned int* cnt = reinterpret_cast<unsigned int*>(agree_sh + (SIZES ? 2 * cells : 0));
  for (int t = threadIdx.x; t < cells; t += kAgreeLdsBlock) {
    cnt[t] = 0u;
    if (SIZES) sum[2 * t] = sum[2 * t + 1] = 0ull;
  }
  __syncthreads();
  constexpr int64_t kRows = (int64_t)kAgreeLdsBlock * kAgreeUnroll;  // per workgroup and iteration
  int bad = 0;
  // a workgroup's share of the rows is below 2^32: its uint32 cells cannot overflow
  for (int64_t base = (int64_t)blockIdx.x * kRows + (threadIdx.x >> 6) * (64 * kAgreeUnroll);
       base < g.n; base += (int64_t)gridDim.x * kRows)
    bad |= add_rows<SIZES, unsigned int>(g, base, cnt, sum);
  __syncthreads();
  for (int t = threadIdx.x; t < cells; t += kAgreeLdsBlock) {
    const unsigned int c = cnt[t];
    if (c == 0u) continue;
    atomicAdd(&g.cnt[t], (unsigned long long)c);
    if (SIZES) {
      if (sum[2 * t]) atomicAdd(&g.sum[2 * t], sum[2 * t]);
      if (sum[2 * t + 1]) atomicAdd(&g.sum[2 * t + 1], sum[2 * t + 1]);
    }
  }
  if (bad) atomicOr(g.flag, bad);
}

template <bool SIZES>
__global__ __launch_bounds__(kAgreeGlobalBlock) void agree_global(AgreeArgs g) {
  constexpr int64_t kRows = (int64_t)kAgreeGlobalBlock * kAgreeUnroll;
  int bad = 0;
  for (int64_t base = (int64_t)blockIdx.x * kRows + (threadIdx.x >> 6) * (64 * kAgreeUnroll);
       base < g.n; base += (int64_t)gridDim.x * kRows)
    bad |= add_rows<SIZES, unsigned long long>(g, base, g.cnt, g.sum);
  if (bad) atomicOr(g.flag, bad);
}

struct AgreeEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~AgreeEvents() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

double ms_between(hipEvent_t a, hipEvent_t b) {
  float v = 0.f;
  (void)hipEventElapsedTime(&v, a, b);
  return v;
}

// The caller's labels as int32 in `dst`; a value outside [0, k) becomes -1 (the
// kernel flags it).
void upload_labels(Ctx& c, DevBuf& dst, const int64_t* labels, int64_t n, int32_t k) {
  c.agree_stage.ensure(sizeof(int32_t) * (size_t)n);
  int32_t* h = c.agree_stage.as<int32_t>();
  for (int64_t i = 0; i < n; ++i) h[i] = labels[i] < 0 || labels[i] >= k ? -1 : (int32_t)labels[i];
  dst.ensure(sizeof(int32_t) * (size_t)n);
  HIP_CHECK(hipMemcpyAsync(dst.p, h, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));  // the staging buffer serves both sides
}

template <bool SIZES>
void launch(Ctx& c, const AgreeArgs& g, bool lds, int grid) {
  if (lds) {
    const size_t shmem = (size_t)g.ka * g.kb * (SIZES ? 20 : 4);
    // beyond the default 64 KiB of dynamic LDS (the attribute may be per device:
    // set on every such launch, a host call of microseconds)
    if (shmem > 64 * 1024)
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&agree_lds<SIZES>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(agree_lds<SIZES>, dim3(grid), dim3(kAgreeLdsBlock), shmem, c.stream, g);
  } else {
    hipLaunchKernelGGL(agree_global<SIZES>, dim3(grid), dim3(kAgreeGlobalBlock), 0, c.stream, g);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void agree_keep(Ctx& c) {
  if (!c.have_labels || c.n <= 0)
    CDR_FAIL(CDR_ERR_STATE, "agree: no labels on the device: run a Lloyd step first");
  c.agree_kept.ensure(sizeof(int32_t) * (size_t)c.n);
  HIP_CHECK(hipMemcpyAsync(c.agree_kept.p, c.labels.p, sizeof(int32_t) * (size_t)c.n,
                           hipMemcpyDeviceToDevice, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  c.agree_kept_n = c.n;
  c.agree_kept_k = c.last_k;
}

void agree_table(Ctx& c, const int64_t* labels_a, int32_t ka, const int64_t* labels_b, int32_t kb,
                 int64_t n, const int64_t* sizes, uint64_t* counts, uint64_t* size_sums) {
  if (ka < 1 || kb < 1 || ka > kAgreeMaxK || kb > kAgreeMaxK)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "agree: ka or kb outside [1, 1024]");
  if (n < 0 || n >= (1ll << 31)) CDR_FAIL(CDR_ERR_ARG, "agree: n outside [0, 2^31)");
  if (!sizes && size_sums) CDR_FAIL(CDR_ERR_ARG, "agree: size_sums without sizes");
  if (sizes && !size_sums) CDR_FAIL(CDR_ERR_ARG, "agree: sizes without size_sums");
  if (!labels_a) {
    if (!c.have_labels)
      CDR_FAIL(CDR_ERR_STATE, "agree: no labels on the device: run a Lloyd step or pass labels_a");
    if (n != c.n) CDR_FAIL(CDR_ERR_ARG, "agree: n is not the resident labels' row count");
    if (ka < c.last_k) CDR_FAIL(CDR_ERR_ARG, "agree: ka smaller than the resident labels' k");
  }
  if (!labels_b) {
    if (c.agree_kept_n < 0)
      CDR_FAIL(CDR_ERR_STATE, "agree: no kept labels: call cdr_agree_keep or pass labels_b");
    if (n != c.agree_kept_n) CDR_FAIL(CDR_ERR_ARG, "agree: n is not the kept labels' row count");
    if (kb < c.agree_kept_k) CDR_FAIL(CDR_ERR_ARG, "agree: kb smaller than the kept labels' k");
  }
  const int64_t cells = (int64_t)ka * kb;
  const bool lds = cells <= (sizes ? kAgreeCapSizes : kAgreeCapCounts);
  for (double& v : c.agree_ms) v = 0.0;
  c.agree_form = lds ? 0 : 1;
  c.agree_wgs = 0;
  for (int64_t j = 0; j < cells; ++j) counts[j] = 0;
  if (size_sums)
    for (int64_t j = 0; j < 2 * cells; ++j) size_sums[j] = 0;
  if (n == 0) return;
  AgreeEvents ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  const size_t words = (size_t)cells * (sizes ? 3 : 1) + 1;  // counts, sums, the flag
  c.agree_tab.ensure(8 * words);
  c.agree_host.ensure(8 * words);
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  if (labels_a) upload_labels(c, c.agree_a, labels_a, n, ka);
  if (labels_b) upload_labels(c, c.agree_b, labels_b, n, kb);
  if (sizes) {
    c.agree_sz.ensure(8 * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(c.agree_sz.p, sizes, 8 * (size_t)n, hipMemcpyHostToDevice, c.stream));
  }
  HIP_CHECK(hipMemsetAsync(c.agree_tab.p, 0, 8 * words, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  AgreeArgs g;
  g.la = labels_a ? c.agree_a.as<int32_t>() : c.labels.as<int32_t>();
  g.lb = labels_b ? c.agree_b.as<int32_t>() : c.agree_kept.as<int32_t>();
  g.sizes = sizes ? c.agree_sz.as<long long>() : nullptr;
  g.n = n;
  g.ka = ka;
  g.kb = kb;
  g.cnt = c.agree_tab.as<unsigned long long>();
  g.sum = g.cnt + cells;
  g.flag = reinterpret_cast<int*>(g.cnt + words - 1);
  const int cus = lloyd_num_cus(c.device);
  int grid;
  if (lds)
    grid = (int)std::min<int64_t>(ceil_div(n, (int64_t)kAgreeLdsBlock * kAgreeUnroll),
                                  std::min(kAgreeLdsPerCu * cus, kAgreeLdsGridMax));
  else
    grid = (int)std::min<int64_t>(ceil_div(n, (int64_t)kAgreeGlobalBlock * kAgreeUnroll),
                                  (int64_t)kAgreeGlobalPerCu * cus);
  if (sizes) launch<true>(c, g, lds, grid);
  else launch<false>(c, g, lds, grid);
  c.agree_wgs = grid;
  HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
  HIP_CHECK(hipMemcpyAsync(c.agree_host.p, c.agree_tab.p, 8 * words, hipMemcpyDeviceToHost,
                           c.stream));
  HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  for (int i = 0; i < 3; ++i) c.agree_ms[i] = ms_between(ev.e[i], ev.e[i + 1]);
  const unsigned long long* h = c.agree_host.as<unsigned long long>();
  const unsigned flag = (unsigned)(h[words - 1] & 0xFFFFFFFFull);
  if (flag & 1u) CDR_FAIL(CDR_ERR_ARG, "agree: a label outside [0, ka) or [0, kb)");
  if (flag & 2u) CDR_FAIL(CDR_ERR_ARG, "agree: negative size");
  memcpy(counts, h, 8 * (size_t)cells);
  if (size_sums) memcpy(size_sums, h + cells, 16 * (size_t)cells);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_agree_keep(cdr_ctx* h) {
  CDR_TRY
  if (!h) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  agree_keep(h->c);
  CDR_CATCH
}

int cdr_agree_table(cdr_ctx* h, const int64_t* labels_a, int32_t ka, const int64_t* labels_b,
                    int32_t kb, int64_t n, const int64_t* sizes, uint64_t* counts,
                    uint64_t* size_sums) {
  CDR_TRY
  if (!h || !counts) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  agree_table(h->c, labels_a, ka, labels_b, kb, n, sizes, counts, size_sums);
  CDR_CATCH
}

int cdr_agree_info(cdr_ctx* h, int64_t* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  out[0] = h->c.agree_form;
  out[1] = kAgreeCapCounts;
  out[2] = kAgreeCapSizes;
  out[3] = h->c.agree_wgs;
  CDR_CATCH
}

int cdr_agree_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 3; ++i) out[i] = h->c.agree_ms[i];
  CDR_CATCH
}

}  // extern "C"
