// csvout.hip — the rows of the features CSV formatted on the device
// (src/compute_features.py:96).  The cell text is csv_digits.h's;
// the path is quoted as Python's csv.writer(lineterminator="\n") quotes it.
//
//   csv_cells    one thread per numeric cell: text and length into a 32-byte slot
//   csv_rowlen   one thread per row: quoted path length + cells + separators,
//                the deferred flag, and the workgroup's (bytes, deferred) sums
//   csv_scan_top one workgroup: exclusive scan of the workgroup sums (int64)
//   csv_offsets  per row: its byte offset (workgroup scan + base), the
//                deferred list {row, offset} in row order
//   csv_emit     one thread per field: the quoted path, or ',' + the slot's text
//
// No atomics: every sum is taken in a fixed order.  Vector stores only.
#include "cdr_internal.h"
#include "csv_digits.h"
#include "csv_scan.h"

#include <algorithm>

namespace cdr {

namespace {

constexpr int kCsvBlock = 256;        // rows per workgroup of the row kernels
constexpr int kCsvSlot = 32;          // bytes per cell slot: text[26], pad, length at byte 31
constexpr unsigned kCsvDeferred = 0xFF;  // slot length of a cell left to the host

__global__ __launch_bounds__(256) void csv_cells(const double* __restrict__ table, int64_t n_cells,
                                                 int n_cols, uint32_t long_mask,
                                                 ulonglong2* __restrict__ slots) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cells) return;
  const int col = (int)(i % n_cols);
  const double v = table[i];
  csvd::Text t;
  const int n = ((long_mask >> col) & 1u) ? csvd_long(v, t) : csvd_double(v, t);
  const uint64_t len = n > 0 ? (uint64_t)n : (uint64_t)kCsvDeferred;
  slots[2 * i] = make_ulonglong2(t.w0, t.w1);
  slots[2 * i + 1] = make_ulonglong2(t.w2, (t.w3 & 0x00FFFFFFFFFFFFFFull) | (len << 56));
}

// qlen[r] = the quoted path's length, or -1 for a row left to the host (a cell
// outside the device range, or a path with a NUL or CR byte); part[2 g],
// part[2 g + 1] = workgroup g's output bytes and deferred rows (a deferred row
// has no bytes).
__global__ __launch_bounds__(256) void csv_rowlen(const unsigned char* __restrict__ pbytes,
                                                  const long long* __restrict__ poff,
                                                  const unsigned char* __restrict__ slots,
                                                  int64_t n_rows, int n_cols,
                                                  int32_t* __restrict__ qlen,
                                                  long long* __restrict__ part) {
  __shared__ long long sh[512];
  const int64_t r = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
  long long len = 0, def = 0;
  if (r < n_rows) {
    const long long p0 = poff[r], p1 = poff[r + 1];
    int quotes = 0;
    bool need = false, bad = false;
    for (long long p = p0; p < p1; ++p) {
      const unsigned ch = pbytes[p];
      quotes += ch == '"';
      need |= ch == '"' || ch == ',' || ch == '\n';
      bad |= ch == 0 || ch == '\r';
    }
    long long cells = 0;
    for (int j = 0; j < n_cols; ++j) {
      const unsigned l = slots[(r * n_cols + j) * kCsvSlot + 31];
      bad |= l == kCsvDeferred;
      cells += 1 + l;
    }
    const long long q = (p1 - p0) + (need ? 2 + quotes : 0);
    if (bad) {
      qlen[r] = -1;
      def = 1;
    } else {
      qlen[r] = (int32_t)q;
      len = q + cells + 1;
    }
  }
  // the row's length is recomputed by csv_offsets from qlen and the slots
  block_sum2(len, def, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = len;
    part[2 * blockIdx.x + 1] = def;
  }
}

__device__ inline long long csv_row_bytes(const unsigned char* __restrict__ slots, int64_t r,
                                          int n_cols, int32_t q) {
  long long cells = 0;
  for (int j = 0; j < n_cols; ++j) cells += 1 + slots[(r * n_cols + j) * kCsvSlot + 31];
  return q + cells + 1;
}

__global__ __launch_bounds__(256) void csv_offsets(const unsigned char* __restrict__ slots,
                                                   const int32_t* __restrict__ qlen,
                                                   const long long* __restrict__ part,
                                                   int64_t n_rows, int n_cols,
                                                   long long* __restrict__ rowoff,
                                                   long long* __restrict__ deferred) {
  __shared__ long long sh[512];
  const int64_t r = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
  long long len = 0, def = 0;
  if (r < n_rows) {
    const int32_t q = qlen[r];
    if (q < 0)
      def = 1;
    else
      len = csv_row_bytes(slots, r, n_cols, q);
  }
  const bool is_def = def != 0;
  block_exscan2(len, def, sh);
  if (r >= n_rows) return;
  const long long off = part[2 * blockIdx.x] + len;
  rowoff[r] = off;
  if (is_def) {
    const long long k = part[2 * blockIdx.x + 1] + def;
    deferred[2 * k] = r;
    deferred[2 * k + 1] = off;
  }
}

__global__ __launch_bounds__(256) void csv_emit(const unsigned char* __restrict__ pbytes,
                                                const long long* __restrict__ poff,
                                                const unsigned char* __restrict__ slots,
                                                const int32_t* __restrict__ qlen,
                                                const long long* __restrict__ rowoff,
                                                int64_t n_items, int n_cols,
                                                unsigned char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const int64_t r = i / (n_cols + 1);
  const int f = (int)(i - r * (n_cols + 1));
  const int32_t q = qlen[r];
  if (q < 0) return;  // deferred: no bytes
  unsigned char* o = out + rowoff[r];
  if (f == 0) {
    const long long p0 = poff[r], p1 = poff[r + 1];
    if (q == p1 - p0) {
      for (long long p = p0; p < p1; ++p) *o++ = pbytes[p];
    } else {
      *o++ = '"';
      for (long long p = p0; p < p1; ++p) {
        const unsigned char ch = pbytes[p];
        if (ch == '"') *o++ = '"';
        *o++ = ch;
      }
      *o++ = '"';
    }
    return;
  }
  const int j = f - 1;
  o += q;
  for (int k = 0; k < j; ++k) o += 1 + slots[(r * n_cols + k) * kCsvSlot + 31];
  const ulonglong2* sl = reinterpret_cast<const ulonglong2*>(slots) + 2 * (r * n_cols + j);
  const ulonglong2 a = sl[0], b = sl[1];
  const int len = (int)(b.y >> 56);
  *o++ = ',';
#pragma unroll
  for (int k = 0; k < csvd::kMaxText; ++k) {
    const uint64_t w = k < 8 ? a.x : (k < 16 ? a.y : (k < 24 ? b.x : b.y));
    if (k < len) o[k] = (unsigned char)(w >> (8 * (k & 7)));
  }
  if (j == n_cols - 1) o[len] = '\n';
}

int64_t csv_bound(int64_t n_rows, int32_t n_cols, int64_t path_bytes_total) {
  // per row: every path byte doubled + two quotes, per cell ',' + 26 bytes, '\n'
  return 2 * path_bytes_total + n_rows * (3 + (int64_t)n_cols * (csvd::kMaxText + 1));
}

struct Events {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

}  // namespace

void csv_format(Ctx& c, int64_t n_rows, int32_t n_cols, uint32_t long_mask, const double* table,
                const char* pbytes, const int64_t* poff, char* out, int64_t cap,
                int64_t* written, int64_t* deferred, int64_t deferred_cap, int64_t* n_deferred) {
  if (n_cols < 1 || n_cols > 16) CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv: n_cols outside [1, 16]");
  if (n_rows < 0 || cap < 0 || deferred_cap < 0) CDR_FAIL(CDR_ERR_ARG, "csv: negative size");
  if (n_rows >= (1ll << 31)) CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv: 2^31 rows or more in one call");
  *written = 0;
  *n_deferred = 0;
  c.csv_ms[0] = c.csv_ms[1] = c.csv_ms[2] = 0.0;
  if (n_rows == 0) return;
  if (!table || !poff) CDR_FAIL(CDR_ERR_ARG, "null argument");
  const int64_t nb = poff[n_rows];
  if (poff[0] != 0 || nb < 0) CDR_FAIL(CDR_ERR_ARG, "csv: path offsets must start at 0");
  for (int64_t i = 0; i < n_rows; ++i) {
    if (poff[i + 1] < poff[i]) CDR_FAIL(CDR_ERR_ARG, "csv: path offsets must be non-decreasing");
    // (the quoted length, at most twice the path's + 2, is kept as an int32)
    if (poff[i + 1] - poff[i] >= (1 << 29))
      CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv: path of 512 MiB or more");
  }
  if (nb > 0 && !pbytes) CDR_FAIL(CDR_ERR_ARG, "null argument");
  const int64_t bound = csv_bound(n_rows, n_cols, nb);
  const int64_t n_cells = n_rows * n_cols, n_items = n_rows * (n_cols + 1);
  const int64_t n_parts = ceil_div(n_rows, kCsvBlock);

  c.csv_table.ensure(sizeof(double) * n_cells);
  c.csv_slots.ensure((size_t)kCsvSlot * n_cells);
  c.csv_pbytes.ensure(nb + 16);
  c.csv_poff.ensure(sizeof(int64_t) * (n_rows + 1));
  c.csv_qlen.ensure(sizeof(int32_t) * n_rows);
  c.csv_rowoff.ensure(sizeof(int64_t) * n_rows);
  c.csv_part.ensure(sizeof(int64_t) * 2 * (n_parts + 1));
  c.csv_def.ensure(sizeof(int64_t) * 2 * n_rows);
  c.csv_out.ensure(bound);
  c.h_small.ensure(64);
  long long* d_part = c.csv_part.as<long long>();
  long long* d_total = d_part + 2 * n_parts;
  const unsigned char* d_slots = c.csv_slots.as<unsigned char>();

  Events ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  HIP_CHECK(hipMemcpyAsync(c.csv_table.p, table, sizeof(double) * n_cells, hipMemcpyHostToDevice,
                           c.stream));
  if (nb > 0)
    HIP_CHECK(hipMemcpyAsync(c.csv_pbytes.p, pbytes, nb, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemcpyAsync(c.csv_poff.p, poff, sizeof(int64_t) * (n_rows + 1),
                           hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  hipLaunchKernelGGL(csv_cells, dim3((unsigned)ceil_div(n_cells, 256)), dim3(256), 0, c.stream,
                     c.csv_table.as<double>(), n_cells, (int)n_cols, long_mask,
                     c.csv_slots.as<ulonglong2>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
  hipLaunchKernelGGL(csv_rowlen, dim3((unsigned)n_parts), dim3(kCsvBlock), 0, c.stream,
                     c.csv_pbytes.as<unsigned char>(), c.csv_poff.as<long long>(), d_slots, n_rows,
                     (int)n_cols, c.csv_qlen.as<int32_t>(), d_part);
  hipLaunchKernelGGL(csv_scan_top, dim3(1), dim3(256), 0, c.stream, d_part, n_parts, d_total);
  hipLaunchKernelGGL(csv_offsets, dim3((unsigned)n_parts), dim3(kCsvBlock), 0, c.stream, d_slots,
                     c.csv_qlen.as<int32_t>(), d_part, n_rows, (int)n_cols,
                     c.csv_rowoff.as<long long>(), c.csv_def.as<long long>());
  hipLaunchKernelGGL(csv_emit, dim3((unsigned)ceil_div(n_items, 256)), dim3(256), 0, c.stream,
                     c.csv_pbytes.as<unsigned char>(), c.csv_poff.as<long long>(), d_slots,
                     c.csv_qlen.as<int32_t>(), c.csv_rowoff.as<long long>(), n_items, (int)n_cols,
                     c.csv_out.as<unsigned char>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
  long long* h_total = c.h_small.as<long long>();
  HIP_CHECK(hipMemcpyAsync(h_total, d_total, 16, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  const int64_t total = h_total[0], ndef = h_total[1];
  if (total < 0 || total > bound || ndef < 0 || ndef > n_rows)
    CDR_FAIL(CDR_ERR_STATE, "csv: inconsistent totals from the device");
  // nothing has been written to the caller's buffers yet
  if (total > cap)
    CDR_FAIL(CDR_ERR_ARG, "csv: out holds " + std::to_string(cap) + " bytes, the rows need " +
                              std::to_string(total));
  if (ndef > deferred_cap)
    CDR_FAIL(CDR_ERR_ARG, "csv: " + std::to_string(ndef) + " deferred rows, room for " +
                              std::to_string(deferred_cap));
  if ((total > 0 && !out) || (ndef > 0 && !deferred)) CDR_FAIL(CDR_ERR_ARG, "null argument");
  c.csv_host.ensure(total + 16 * ndef + 16);
  HIP_CHECK(hipEventRecord(ev.e[4], c.stream));
  if (total > 0)
    HIP_CHECK(hipMemcpyAsync(c.csv_host.p, c.csv_out.p, total, hipMemcpyDeviceToHost, c.stream));
  char* h_def = c.csv_host.as<char>() + (total + 15) / 16 * 16;
  if (ndef > 0)
    HIP_CHECK(hipMemcpyAsync(h_def, c.csv_def.p, 16 * ndef, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[5], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (total > 0) memcpy(out, c.csv_host.p, total);
  if (ndef > 0) memcpy(deferred, h_def, 16 * ndef);
  *written = total;
  *n_deferred = ndef;
  float up = 0.f, cells = 0.f, rest = 0.f, down = 0.f;
  (void)hipEventElapsedTime(&up, ev.e[0], ev.e[1]);
  (void)hipEventElapsedTime(&cells, ev.e[1], ev.e[2]);
  (void)hipEventElapsedTime(&rest, ev.e[2], ev.e[3]);
  (void)hipEventElapsedTime(&down, ev.e[4], ev.e[5]);
  c.csv_ms[0] = cells;
  c.csv_ms[1] = rest;
  c.csv_ms[2] = (double)up + down;
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_csv_format(cdr_ctx* h, int64_t n_rows, int32_t n_cols, uint32_t long_mask,
                   const double* table, const char* path_bytes, const int64_t* path_off, char* out,
                   int64_t cap, int64_t* written, int64_t* deferred, int64_t deferred_cap,
                   int64_t* n_deferred) {
  CDR_TRY
  if (!h || !written || !n_deferred) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  csv_format(h->c, n_rows, n_cols, long_mask, table, path_bytes, path_off, out, cap, written,
             deferred, deferred_cap, n_deferred);
  CDR_CATCH
}

int cdr_csv_bound(int64_t n_rows, int32_t n_cols, int64_t path_bytes_total, int64_t* bytes) {
  CDR_TRY
  if (!bytes || n_rows < 0 || path_bytes_total < 0) CDR_FAIL(CDR_ERR_ARG, "csv: bad argument");
  if (n_cols < 1 || n_cols > 16) CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv: n_cols outside [1, 16]");
  *bytes = csv_bound(n_rows, n_cols, path_bytes_total);
  CDR_CATCH
}

int cdr_csv_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 3; ++i) out[i] = h->c.csv_ms[i];
  CDR_CATCH
}

}  // extern "C"
