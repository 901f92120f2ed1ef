// plan.hip — the per-file replication plan written on the device:
// one text row "path,cluster,category,replication\n" per record of the features
// CSV, the path copied as the bytes it has in that file, and the per-cluster
// sums of the files' sizes.
//
// The records are csvin.hip's (csv_index_count / csv_index_write: '\n' outside
// quotes, a '\r' before it dropped, empty lines skipped, a last line without
// '\n' kept), and the guard is the same (csv_guard.h, and a line of blanks).
//
//   plan_rows     one wave per 64 records, record after record: the wave reads
//                 the record 64 bytes at a time and ballots commas, quotes, NUL /
//                 CR and non-blanks; the path field's offset and length (-1: the
//                 row is deferred), the workgroup's (bytes, deferred) sums
//   csv_scan_top  one workgroup: exclusive scan of the workgroup sums (csv_scan.h)
//   plan_offsets  per row: its byte offset, the deferred list {row, offset,
//                 byte begin, byte end} in row order
//   plan_emit     one wave per 64 records, record after record: the lanes copy
//                 the field's bytes, then ',' + the decimal label + the
//                 cluster's tail ",<category>,<factor>\n" (formatted by the host)
//   plan_size_sums  per cluster the sums of the sizes' low 32 and high 31 bits
//
// A wave's 64 rows are adjacent in the output and each row is written as one
// contiguous run by consecutive lanes.  No floating point, vector stores only.
// The atomics are the guard's atomicMin (a well-formed file never reaches it)
// and plan_size_sums' integer adds (order-free).
#include <climits>

#include "cdr_internal.h"
#include "csv_guard.h"
#include "csv_scan.h"

#include <algorithm>

namespace cdr {

namespace {

constexpr int kPlanBlock = 256;        // rows per workgroup (4 waves x 64 rows)
constexpr int kPlanSlot = 64;          // bytes per tail slot: text[63], length at byte 63
constexpr int kPlanMaxTail = kPlanSlot - 1;
constexpr int kPlanMaxField = 65535;   // a longer path field is deferred
constexpr int kPlanMaxK = 1024;
constexpr int kPlanTile = 4096;        // csvin.hip's kTile: the body's zero padding
constexpr int kSumGrid = 1024;         // plan_size_sums workgroups at most

__device__ __forceinline__ int ndigits(unsigned v) {
  int n = 1;
  while (v >= 10u) {
    v /= 10u;
    ++n;
  }
  return n;
}

// bytes of row text after the path field: ',' + label + tail
__device__ __forceinline__ int suffix_len(const uint8_t* __restrict__ tails, int l) {
  return 1 + ndigits((unsigned)l) + tails[l * kPlanSlot + kPlanMaxTail];
}

// index of the i-th (0-based) set bit of m; m has more than i bits set
__device__ __forceinline__ int nth_bit(unsigned long long m, int i) {
  for (int j = 0; j < i; ++j) m &= m - 1;
  return __ffsll((unsigned long long)m) - 1;
}

struct RowArgs {
  const uint8_t* b;        // the body, a zero tile after the last
  const long long* ends;   // per record of the file: byte index of its terminator
  const int32_t* lab;      // per record of the file: its cluster
  const uint8_t* tails;    // k slots
  int64_t row0, nrows;     // the chunk: records [row0, row0 + nrows)
  int n_cols, path_col;
  long long* fstart;       // per row of the chunk: offset of the path field
  int32_t* flen;           // its length, -1: deferred
  long long* part;         // per workgroup: bytes, deferred rows
  long long* sc;           // sc[1]: first guard offset (atomicMin)
};

__global__ __launch_bounds__(kPlanBlock) void plan_rows(RowArgs a) {
  __shared__ long long sh[512];
  const int lane = threadIdx.x & 63;
  const int64_t i0 = (int64_t)blockIdx.x * kPlanBlock + (threadIdx.x & ~63);
  const int64_t i = i0 + lane;
  const int nw = (int)min<int64_t>(64, a.nrows - i0);  // (<= 0: a wave past the chunk)
  long long my_e = 0, my_p = 0;
  if (lane < nw) {
    const int64_t r = a.row0 + i;
    my_e = a.ends[r];
    my_p = r ? a.ends[r - 1] + 1 : 0;
  }
  long long my_fs = 0;
  int my_len = -1;
  for (int rr = 0; rr < nw; ++rr) {
    // everything in this loop is the same on every lane but `at` and `ch`
    int64_t s = __shfl(my_p, rr);
    int64_t e = __shfl(my_e, rr);
    for (;;) {  // the blank lines before the record ("\n", "\r\n")
      const uint8_t ch = a.b[s];
      if (ch == '\n') ++s;
      else if (ch == '\r' && a.b[s + 1] == '\n') s += 2;
      else break;
    }
    if (e > s && a.b[e - 1] == '\r') --e;
    int ncomma = 0;
    int64_t fs = a.path_col == 0 ? s : -1, fe = -1;
    bool quote = false, bad = false, nonblank = false;
    for (int64_t p = s; p < e; p += 64) {
      const int64_t at = p + lane;
      const bool in = at < e;
      const uint8_t ch = in ? a.b[at] : (uint8_t)'x';
      const unsigned long long mc = __ballot(in && ch == ',');
      quote |= __ballot(in && ch == '"') != 0;
      bad |= __ballot(in && (ch == 0 || ch == '\r')) != 0;
      nonblank |= __ballot(in && ch != ' ' && ch != '\t') != 0;
      const int cnt = __popcll(mc);
      // the field lies between comma path_col - 1 and comma path_col (0-based)
      if (fs < 0 && ncomma + cnt >= a.path_col) fs = p + nth_bit(mc, a.path_col - 1 - ncomma) + 1;
      if (fe < 0 && ncomma + cnt > a.path_col) fe = p + nth_bit(mc, a.path_col - ncomma);
      ncomma += cnt;
    }
    if (fs < 0) fs = fe = e;  // fewer fields than path_col: deferred below
    if (fe < 0) fe = e;
    const bool blank = e > s && !nonblank;  // pandas skips such a line
    const bool def = quote || bad || blank || ncomma + 1 != a.n_cols || fe - fs > kPlanMaxField;
    if (lane == 0 && (quote || blank)) {
      const int64_t g = blank ? s : guard_walk(a.b, s, e);
      if (g >= 0) atomicMin(&a.sc[1], (long long)g);
    }
    if (lane == rr) {
      my_fs = fs;
      my_len = def ? -1 : (int)(fe - fs);
    }
  }
  long long len = 0, ndef = 0;
  if (lane < nw) {
    a.fstart[i] = my_fs;
    a.flen[i] = my_len;
    if (my_len < 0) ndef = 1;
    else len = my_len + suffix_len(a.tails, a.lab[a.row0 + i]);
  }
  // the row's length is recomputed by plan_offsets from flen and the label
  block_sum2(len, ndef, sh);
  if (threadIdx.x == 0) {
    a.part[2 * blockIdx.x] = len;
    a.part[2 * blockIdx.x + 1] = ndef;
  }
}

__global__ __launch_bounds__(kPlanBlock) void plan_offsets(
    const int32_t* __restrict__ flen, const int32_t* __restrict__ lab,
    const uint8_t* __restrict__ tails, const long long* __restrict__ ends,
    const long long* __restrict__ part, int64_t row0, int64_t nrows, int64_t def_cap,
    long long* __restrict__ rowoff, long long* __restrict__ deferred) {
  __shared__ long long sh[512];
  const int64_t i = (int64_t)blockIdx.x * kPlanBlock + threadIdx.x;
  long long len = 0, def = 0;
  if (i < nrows) {
    const int32_t f = flen[i];
    if (f < 0) def = 1;
    else len = f + suffix_len(tails, lab[row0 + i]);
  }
  const bool is_def = def != 0;
  block_exscan2(len, def, sh);
  if (i >= nrows) return;
  const long long off = part[2 * blockIdx.x] + len;
  rowoff[i] = off;
  if (is_def) {
    const long long k = part[2 * blockIdx.x + 1] + def;
    if (k >= def_cap) return;
    const int64_t r = row0 + i;
    deferred[4 * k] = r;
    deferred[4 * k + 1] = off;
    deferred[4 * k + 2] = r ? ends[r - 1] + 1 : 0;
    deferred[4 * k + 3] = ends[r];
  }
}

__global__ __launch_bounds__(kPlanBlock) void plan_emit(
    const uint8_t* __restrict__ b, const long long* __restrict__ fstart,
    const int32_t* __restrict__ flen, const long long* __restrict__ rowoff,
    const int32_t* __restrict__ lab, const uint8_t* __restrict__ tails, int64_t row0,
    int64_t nrows, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i0 = (int64_t)blockIdx.x * kPlanBlock + (threadIdx.x & ~63);
  const int nw = (int)min<int64_t>(64, nrows - i0);
  long long my_fs = 0, my_off = 0;
  int my_len = -1, my_lab = 0;
  if (lane < nw) {
    my_fs = fstart[i0 + lane];
    my_len = flen[i0 + lane];
    my_off = rowoff[i0 + lane];
    my_lab = lab[row0 + i0 + lane];
  }
  for (int rr = 0; rr < nw; ++rr) {
    const int len = __shfl(my_len, rr);
    if (len < 0) continue;  // deferred: no bytes
    const uint8_t* src = b + __shfl(my_fs, rr);
    uint8_t* o = out + __shfl(my_off, rr);
    const int l = __shfl(my_lab, rr);
    for (int j = lane; j < len; j += 64) o[j] = src[j];
    o += len;
    const int nd = ndigits((unsigned)l);
    const uint8_t* tail = tails + l * kPlanSlot;
    const int sfx = 1 + nd + tail[kPlanMaxTail];
    for (int j = lane; j < sfx; j += 64) {
      uint8_t ch = ',';
      if (j > nd) {
        ch = tail[j - 1 - nd];
      } else if (j > 0) {
        unsigned v = (unsigned)l;
        for (int t = nd - j; t > 0; --t) v /= 10u;
        ch = (uint8_t)('0' + v % 10u);
      }
      o[j] = ch;
    }
  }
}

// out[2 j], out[2 j + 1] += the sums of (size & 0xFFFFFFFF) and (size >> 32)
// over the rows labelled j (sizes == nullptr: every size is 1); *flag |= 1 when a size is negative
__global__ __launch_bounds__(256) void plan_size_sums(const long long* __restrict__ sizes,
                                                      const int32_t* __restrict__ lab, int64_t n,
                                                      int k, unsigned long long* __restrict__ out,
                                                      int* __restrict__ flag) {
  __shared__ unsigned long long tab[2 * kPlanMaxK];
  for (int t = threadIdx.x; t < 2 * k; t += 256) tab[t] = 0ull;
  __syncthreads();
  bool neg = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const long long s = sizes ? sizes[i] : 1;  // no sizes: the rows are counted
    if (s < 0) {
      neg = true;
      continue;
    }
    const int l = lab[i];
    atomicAdd(&tab[2 * l], (unsigned long long)s & 0xFFFFFFFFull);
    atomicAdd(&tab[2 * l + 1], (unsigned long long)s >> 32);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * k; t += 256)
    if (tab[t]) atomicAdd(&out[t], tab[t]);
  if (neg) atomicOr(flag, 1);
}

int64_t plan_bound(int64_t n_rows, int64_t field_bytes) {
  // per row: the field, ',', at most 10 digits, the longest tail
  return field_bytes + n_rows * (1 + 10 + kPlanMaxTail);
}

struct Events {
  hipEvent_t e[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

float ms_between(hipEvent_t a, hipEvent_t b) {
  float v = 0.f;
  (void)hipEventElapsedTime(&v, a, b);
  return v;
}

void check_k(int32_t k) {
  if (k < 1) CDR_FAIL(CDR_ERR_ARG, "plan: k < 1");
  if (k > kPlanMaxK) CDR_FAIL(CDR_ERR_UNSUPPORTED, "plan: k > 1024");
}

void check_resident(const Ctx& c, int32_t k) {
  if (!c.have_labels)
    CDR_FAIL(CDR_ERR_STATE, "plan: no labels on the device: run a Lloyd step or pass labels");
  if (k < c.last_k) CDR_FAIL(CDR_ERR_ARG, "plan: k smaller than the resident labels' k");
}

// the caller's labels as int32 in c.plan_lab
void upload_labels(Ctx& c, const int64_t* labels, int64_t n, int32_t k) {
  std::vector<int32_t> lab((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (labels[i] < 0 || labels[i] >= k) CDR_FAIL(CDR_ERR_ARG, "plan: label outside [0, k)");
    lab[i] = (int32_t)labels[i];
  }
  c.plan_lab.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
  if (n > 0)
    HIP_CHECK(hipMemcpyAsync(c.plan_lab.p, lab.data(), sizeof(int32_t) * (size_t)n,
                             hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));  // lab goes out of scope
}

// Uploads the body, the labels and the tails and builds the record index.
void plan_open(Ctx& c, const char* bytes, int64_t nbytes, int64_t body_off,
               const int64_t* labels, int64_t n_labels, int32_t k, const char* tails,
               const int32_t* tail_len, Events& ev) {
  c.plan_rows = -1;
  for (double& v : c.plan_ms) v = 0.0;
  for (int j = 0; j < k; ++j)
    if (tail_len[j] < 0 || tail_len[j] > kPlanMaxTail)
      CDR_FAIL(CDR_ERR_ARG, "plan: a tail longer than 63 bytes");
  if (!labels) check_resident(c, k);
  c.h_small.ensure(64);
  const int64_t nb = nbytes - body_off;
  const int64_t ntiles = nb > 0 ? ceil_div(nb, kPlanTile) : 0;
  const size_t padded = (size_t)(ntiles + 1) * kPlanTile;  // a zero tile after the last
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  c.cin_bytes.ensure(padded);
  uint8_t* db = c.cin_bytes.as<uint8_t>();
  HIP_CHECK(hipMemsetAsync(db + nb, 0, padded - nb, c.stream));
  if (nb > 0) HIP_CHECK(hipMemcpyAsync(db, bytes + body_off, nb, hipMemcpyHostToDevice, c.stream));
  c.cin_sc.ensure(8 * 8 + 8 * 64);
  const long long init[8] = {0, LLONG_MAX, 0, 0, 0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(c.cin_sc.p, init, sizeof(init), hipMemcpyHostToDevice, c.stream));
  std::vector<uint8_t> slots((size_t)k * kPlanSlot, 0);
  for (int j = 0; j < k; ++j) {
    memcpy(&slots[(size_t)j * kPlanSlot], tails + (size_t)j * kPlanSlot, tail_len[j]);
    slots[(size_t)j * kPlanSlot + kPlanMaxTail] = (uint8_t)tail_len[j];
  }
  c.plan_tails.ensure(slots.size());
  HIP_CHECK(hipMemcpyAsync(c.plan_tails.p, slots.data(), slots.size(), hipMemcpyHostToDevice,
                           c.stream));
  if (labels) upload_labels(c, labels, n_labels, k);
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));  // init and slots go out of scope
  long long nrec = 0;
  if (ntiles > 0) {
    long long r8[8];
    csv_index_count(c, nb, r8);
    nrec = r8[0];
    if (nrec < 0 || nrec > nb) CDR_FAIL(CDR_ERR_STATE, "plan: inconsistent record count");
    if (nrec > 0) {
      c.cin_ends.ensure(8 * (size_t)nrec);
      csv_index_write(c, nb, nrec, r8[5] != 0);
    }
  }
  HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (nrec >= (1ll << 31)) CDR_FAIL(CDR_ERR_UNSUPPORTED, "plan: 2^31 rows or more");
  const int64_t have = labels ? n_labels : c.n;
  if (have != nrec)
    CDR_FAIL(CDR_ERR_ARG, "plan: " + std::to_string(have) + " labels, the file has " +
                              std::to_string(nrec) + " rows");
  c.plan_ms[0] = ms_between(ev.e[0], ev.e[1]);
  c.plan_ms[1] = ms_between(ev.e[1], ev.e[2]);
  c.plan_nb = nb;
  c.plan_k = k;
  c.plan_resident = labels == nullptr;
  c.plan_rows = nrec;
}

}  // namespace

void plan_format(Ctx& c, const char* bytes, int64_t nbytes, int64_t body_off, int32_t n_cols,
                 int32_t path_col, const int64_t* labels, int64_t n_labels, int32_t k,
                 const char* tails, const int32_t* tail_len, int64_t row_begin, int64_t row_count,
                 char* out, int64_t cap, int64_t* status, int64_t* deferred,
                 int64_t deferred_cap) {
  check_k(k);
  if (n_cols < 1 || n_cols > 32767)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "plan: n_cols outside [1, 32767]");
  if (path_col < 0 || path_col >= n_cols) CDR_FAIL(CDR_ERR_ARG, "plan: column outside the file");
  if (nbytes < 0 || body_off < 0 || body_off > nbytes || cap < 0 || deferred_cap < 0 ||
      row_begin < 0 || row_count < 0 || n_labels < 0)
    CDR_FAIL(CDR_ERR_ARG, "plan: bad size");
  Events ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  if (row_begin == 0) {
    plan_open(c, bytes, nbytes, body_off, labels, n_labels, k, tails, tail_len, ev);
  } else {
    if (c.plan_rows < 0 || c.plan_nb != nbytes - body_off || c.plan_k != k ||
        c.plan_resident != (labels == nullptr))
      CDR_FAIL(CDR_ERR_STATE, "plan: no index of this file on the device (start at row 0)");
    if (!labels) {  // the labels or the points may have been replaced since row 0
      check_resident(c, k);
      if (c.n != c.plan_rows) CDR_FAIL(CDR_ERR_ARG, "plan: the resident rows are not the file's");
    }
  }
  const int64_t nrec = c.plan_rows;
  if (row_begin > nrec) CDR_FAIL(CDR_ERR_ARG, "plan: row_begin past the last row");
  const int64_t rows = std::min(row_count, nrec - row_begin);
  status[0] = nrec;
  status[1] = status[2] = 0;
  status[3] = -1;
  long long* sc = c.cin_sc.as<long long>();
  long long* h8 = c.h_small.as<long long>();
  if (rows == 0) {
    HIP_CHECK(hipMemcpyAsync(h8, sc + 1, 8, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    status[3] = h8[0] == LLONG_MAX ? -1 : h8[0] + body_off;
    return;
  }
  bool cap_short = false;
  try {
    const int64_t n_parts = ceil_div(rows, kPlanBlock);
    const int64_t def_room = std::min(deferred_cap, rows);
    c.plan_fstart.ensure(8 * (size_t)rows);
    c.plan_flen.ensure(4 * (size_t)rows);
    c.plan_rowoff.ensure(8 * (size_t)rows);
    c.plan_part.ensure(8 * 2 * (size_t)(n_parts + 1));
    c.plan_def.ensure(32 * (size_t)std::max<int64_t>(def_room, 1));
    long long* d_part = c.plan_part.as<long long>();
    long long* d_total = d_part + 2 * n_parts;
    const int32_t* d_lab = labels ? c.plan_lab.as<int32_t>() : c.labels.as<int32_t>();
    const long long* d_ends = c.cin_ends.as<long long>();
    const uint8_t* d_tails = c.plan_tails.as<uint8_t>();
    RowArgs a;
    a.b = c.cin_bytes.as<uint8_t>();
    a.ends = d_ends;
    a.lab = d_lab;
    a.tails = d_tails;
    a.row0 = row_begin;
    a.nrows = rows;
    a.n_cols = n_cols;
    a.path_col = path_col;
    a.fstart = c.plan_fstart.as<long long>();
    a.flen = c.plan_flen.as<int32_t>();
    a.part = d_part;
    a.sc = sc;
    HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
    hipLaunchKernelGGL(plan_rows, dim3((unsigned)n_parts), dim3(kPlanBlock), 0, c.stream, a);
    hipLaunchKernelGGL(csv_scan_top, dim3(1), dim3(256), 0, c.stream, d_part, n_parts, d_total);
    hipLaunchKernelGGL(plan_offsets, dim3((unsigned)n_parts), dim3(kPlanBlock), 0, c.stream,
                       c.plan_flen.as<int32_t>(), d_lab, d_tails, d_ends, d_part, row_begin, rows,
                       def_room, c.plan_rowoff.as<long long>(), c.plan_def.as<long long>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[4], c.stream));
    HIP_CHECK(hipMemcpyAsync(h8, d_total, 16, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(h8 + 2, sc + 1, 8, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    const int64_t total = h8[0], ndef = h8[1], guard = h8[2];
    // every field lies inside the body, so the text is bounded by it
    if (total < 0 || total > plan_bound(rows, c.plan_nb) || ndef < 0 || ndef > rows)
      CDR_FAIL(CDR_ERR_STATE, "plan: inconsistent totals from the device");
    // nothing has been written to the caller's buffers yet
    if (total > cap) {
      status[1] = total;  // what a second call must offer; the index stays
      cap_short = true;
      CDR_FAIL(CDR_ERR_ARG, "plan: out holds " + std::to_string(cap) + " bytes, the rows need " +
                                std::to_string(total));
    }
    const int64_t take = std::min(ndef, def_room);
    if ((total > 0 && !out) || (take > 0 && !deferred)) CDR_FAIL(CDR_ERR_ARG, "null argument");
    c.plan_out.ensure((size_t)std::max<int64_t>(total, 1));
    HIP_CHECK(hipEventRecord(ev.e[5], c.stream));
    hipLaunchKernelGGL(plan_emit, dim3((unsigned)n_parts), dim3(kPlanBlock), 0, c.stream,
                       c.cin_bytes.as<uint8_t>(), c.plan_fstart.as<long long>(),
                       c.plan_flen.as<int32_t>(), c.plan_rowoff.as<long long>(), d_lab, d_tails,
                       row_begin, rows, c.plan_out.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[6], c.stream));
    c.plan_host.ensure((size_t)(total + 32 * take + 16));
    if (total > 0)
      HIP_CHECK(hipMemcpyAsync(c.plan_host.p, c.plan_out.p, total, hipMemcpyDeviceToHost, c.stream));
    char* h_def = c.plan_host.as<char>() + (total + 15) / 16 * 16;
    if (take > 0)
      HIP_CHECK(hipMemcpyAsync(h_def, c.plan_def.p, 32 * (size_t)take, hipMemcpyDeviceToHost,
                               c.stream));
    HIP_CHECK(hipEventRecord(ev.e[7], c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    if (total > 0) memcpy(out, c.plan_host.p, total);
    if (take > 0) memcpy(deferred, h_def, 32 * (size_t)take);
    for (int64_t j = 0; j < take; ++j) {  // byte offsets of the file, not of the body
      deferred[4 * j + 2] += body_off;
      deferred[4 * j + 3] += body_off;
    }
    status[1] = total;
    status[2] = ndef;
    status[3] = guard == LLONG_MAX ? -1 : guard + body_off;
    c.plan_ms[2] += ms_between(ev.e[3], ev.e[4]);
    c.plan_ms[3] += ms_between(ev.e[5], ev.e[6]);
    c.plan_ms[4] += ms_between(ev.e[6], ev.e[7]);
  } catch (...) {
    if (!cap_short) c.plan_rows = -1;
    throw;
  }
}

void plan_size_sums_run(Ctx& c, const int64_t* labels, int64_t n, int32_t k, const int64_t* sizes,
                        uint64_t* out) {
  check_k(k);
  if (n < 0 || n >= (1ll << 31)) CDR_FAIL(CDR_ERR_ARG, "plan: n outside [0, 2^31)");
  if (!labels) {
    check_resident(c, k);
    if (n != c.n) CDR_FAIL(CDR_ERR_ARG, "plan: one size per resident row");
  }
  for (int j = 0; j < 2 * k; ++j) out[j] = 0;
  if (n == 0) return;
  if (labels) {
    c.plan_rows = -1;  // plan_lab is rewritten
    upload_labels(c, labels, n, k);
  }
  if (sizes) c.plan_sz.ensure(8 * (size_t)n);
  c.plan_sum.ensure(8 * 2 * (size_t)k + 8);
  c.h_small.ensure(64);
  unsigned long long* d_sum = c.plan_sum.as<unsigned long long>();
  int* d_flag = reinterpret_cast<int*>(d_sum + 2 * k);
  if (sizes)
    HIP_CHECK(hipMemcpyAsync(c.plan_sz.p, sizes, 8 * (size_t)n, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemsetAsync(d_sum, 0, 8 * 2 * (size_t)k + 8, c.stream));
  const int grid = (int)std::min<int64_t>(ceil_div(n, 256), kSumGrid);
  hipLaunchKernelGGL(plan_size_sums, dim3(grid), dim3(256), 0, c.stream,
                     sizes ? c.plan_sz.as<long long>() : nullptr, labels ? c.plan_lab.as<int32_t>() : c.labels.as<int32_t>(),
                     n, (int)k, d_sum, d_flag);
  HIP_CHECK(hipGetLastError());
  std::vector<unsigned long long> h((size_t)2 * k + 1);
  HIP_CHECK(hipMemcpyAsync(h.data(), d_sum, 8 * h.size(), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (h[2 * k] & 0xFFFFFFFFull) CDR_FAIL(CDR_ERR_ARG, "plan: negative size");
  for (int j = 0; j < 2 * k; ++j) out[j] = h[j];
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_plan_format(cdr_ctx* h, const char* bytes, int64_t nbytes, int64_t body_off,
                    int32_t n_cols, int32_t path_col, const int64_t* labels, int64_t n_labels,
                    int32_t k, const char* tails, const int32_t* tail_len, int64_t row_begin,
                    int64_t row_count, char* out, int64_t cap, int64_t* status, int64_t* deferred,
                    int64_t deferred_cap) {
  CDR_TRY
  if (!h || !status || !tails || !tail_len || (nbytes > 0 && !bytes))
    CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  plan_format(h->c, bytes, nbytes, body_off, n_cols, path_col, labels, n_labels, k, tails,
              tail_len, row_begin, row_count, out, cap, status, deferred, deferred_cap);
  CDR_CATCH
}

int cdr_plan_bound(int64_t n_rows, int64_t field_bytes, int64_t* bytes) {
  CDR_TRY
  if (!bytes || n_rows < 0 || field_bytes < 0) CDR_FAIL(CDR_ERR_ARG, "plan: bad argument");
  *bytes = plan_bound(n_rows, field_bytes);
  CDR_CATCH
}

int cdr_plan_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 5; ++i) out[i] = h->c.plan_ms[i];
  CDR_CATCH
}

int cdr_plan_size_sums(cdr_ctx* h, const int64_t* labels, int64_t n, int32_t k,
                       const int64_t* sizes, uint64_t* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  plan_size_sums_run(h->c, labels, n, k, sizes, out);
  CDR_CATCH
}

}  // extern "C"
