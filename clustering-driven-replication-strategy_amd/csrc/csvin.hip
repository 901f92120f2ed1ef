// csvin.hip — the features CSV read on the device into the resident points
// (the reference's main.py:75-81: pd.read_csv(path)[CLUSTERING_FEATURES].values;
// DESIGN §6.8).  The cell parser is csv_parse.h's restatement of pandas' float
// parser; this file finds the records as pandas' tokenizer does and splits them.
//
//   q_count    one uint4 per lane, 4 KiB tiles: the tile's quote parity and its
//              record terminators under both entering parities
//   qe_scan_*  one exclusive scan of (parity, count under parity 0, count under
//              parity 1) over the tiles: 4096 elements per workgroup, three kernels
//   q_total    record count, the last line without '\n', the final parity
//   q_write    q_count's per-lane masks under the tile's true parity, workgroup
//              scan, each record's end index
//   parse      64 records per workgroup iteration (one wave), their span staged
//              in LDS; one lane per record splits the fields and runs csvp_cell
//              on the selected columns, straight into the planar x64
//   def_write  the deferred rows {row, byte begin, byte end} in row order
//
// Record semantics (pandas' C tokenizer, default dialect): a record ends at a
// '\n' outside quotes; a '\r' right before it is dropped; an empty line (or
// only "\r") gives no record; a last line without '\n' is still a record.  A
// quote toggles the state wherever it stands, which is what pandas does as long
// as every opening quote is at a field start and every closing quote is
// followed by ',', '"', '\r', '\n' or the end; the parse kernel walks every row
// that holds a quote and reports the first byte where that fails (the guard),
// and with it a line of blanks and tabs only, which pandas skips.  The caller
// then takes the whole file to pandas.
//
// No floating-point atomics; the only atomic is the guard's atomicMin, which a
// well-formed file never reaches.  Counts are ballots summed in a fixed order.
#include <climits>

#include "cdr_internal.h"
#include "csv_guard.h"
#include "csv_parse.h"

namespace cdr {

namespace {

constexpr int kTile = 4096;    // bytes per q_count / q_write workgroup (256 lanes x 16)
constexpr int kRows = 64;      // records (lanes) per parse workgroup iteration
constexpr int kStage = 16384;  // LDS bytes staged per parse workgroup iteration
constexpr int kMaxSel = 16;    // selected columns (4 kinds x 16 = one counter per lane)
constexpr int kMaxCell = 4096; // a longer cell is deferred unread
constexpr int kScanPer = 16;               // elements per thread
constexpr int kScanPart = 256 * kScanPer;  // elements per workgroup
constexpr int kParseGrid = 8192;           // parse workgroups (each loops over its blocks)

// One step of the scan: the quote parity flips q times (mod 2) over the span,
// and it holds c0 (c1) record terminators when entered outside (inside) quotes.
struct QE {
  long long c0, c1;
  unsigned long long q;
};

__device__ __forceinline__ QE qe_make(long long c0, long long c1, unsigned q) {
  QE e;
  e.c0 = c0;
  e.c1 = c1;
  e.q = q;
  return e;
}

// a, then b (not commutative)
__device__ __forceinline__ QE qe_join(const QE& a, const QE& b) {
  return qe_make(a.c0 + (a.q ? b.c1 : b.c0), a.c1 + (a.q ? b.c0 : b.c1), (unsigned)(a.q ^ b.q));
}

// Exclusive scan of one element per thread over a 256-thread workgroup
// (Hillis-Steele through LDS, the left operand always the earlier span);
// *total = the workgroup's join.  Every thread of the workgroup calls it.
__device__ __forceinline__ QE wg256_exscan(QE v, QE* total) {
  __shared__ long long s0[256], s1[256];
  __shared__ unsigned sq[256];
  const int t = threadIdx.x;
  QE inc = v;
  for (int o = 1; o < 256; o <<= 1) {
    s0[t] = inc.c0;
    s1[t] = inc.c1;
    sq[t] = (unsigned)inc.q;
    __syncthreads();
    QE l = qe_make(0, 0, 0);
    if (t >= o) l = qe_make(s0[t - o], s1[t - o], sq[t - o]);
    __syncthreads();
    if (t >= o) inc = qe_join(l, inc);
  }
  s0[t] = inc.c0;
  s1[t] = inc.c1;
  sq[t] = (unsigned)inc.q;
  __syncthreads();
  *total = qe_make(s0[255], s1[255], sq[255]);
  const QE ex = t ? qe_make(s0[t - 1], s1[t - 1], sq[t - 1]) : qe_make(0, 0, 0);
  __syncthreads();  // the arrays are reused by the next call
  return ex;
}

__global__ __launch_bounds__(256) void qe_scan_part(const QE* __restrict__ el, int64_t n,
                                                    QE* __restrict__ part) {
  const int64_t lo = (int64_t)blockIdx.x * kScanPart + (int64_t)threadIdx.x * kScanPer;
  QE s = qe_make(0, 0, 0);
  for (int j = 0; j < kScanPer; ++j)
    if (lo + j < n) s = qe_join(s, el[lo + j]);
  QE tot;
  wg256_exscan(s, &tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void qe_scan_mid(QE* __restrict__ part, int64_t np) {
  const int64_t per = (np + 255) / 256;
  const int64_t lo = (int64_t)threadIdx.x * per;
  QE s = qe_make(0, 0, 0);
  for (int64_t i = lo; i < lo + per && i < np; ++i) s = qe_join(s, part[i]);
  QE tot;
  QE o = wg256_exscan(s, &tot);
  for (int64_t i = lo; i < lo + per && i < np; ++i) {
    const QE v = part[i];
    part[i] = o;
    o = qe_join(o, v);
  }
}

// pre[i] = the join of el[0, i); pre[n] = the join of all (written by the
// thread that holds the last element)
__global__ __launch_bounds__(256) void qe_scan_out(const QE* __restrict__ el, int64_t n,
                                                   const QE* __restrict__ part,
                                                   QE* __restrict__ pre) {
  const int64_t lo = (int64_t)blockIdx.x * kScanPart + (int64_t)threadIdx.x * kScanPer;
  QE s = qe_make(0, 0, 0);
  for (int j = 0; j < kScanPer; ++j)
    if (lo + j < n) s = qe_join(s, el[lo + j]);
  QE tot;
  QE o = qe_join(part[blockIdx.x], wg256_exscan(s, &tot));
  for (int j = 0; j < kScanPer; ++j) {
    if (lo + j < n) {
      pre[lo + j] = o;
      o = qe_join(o, el[lo + j]);
      if (lo + j == n - 1) pre[n] = o;
    }
  }
}

__device__ __forceinline__ bool is_rec_end(int64_t p, uint8_t c1, uint8_t c2) {
  // '\n' at p closes a non-blank line: c1 = b[p-1], c2 = b[p-2] (0 if absent)
  if (p == 0 || c1 == '\n') return false;
  if (c1 == '\r' && (p == 1 || c2 == '\n')) return false;
  return true;
}

// Per lane (16 bytes): the quote parity and the terminator bits for a lane
// entered outside (m0) and inside (m1) quotes.  A '\n' that is outside quotes
// has its one or two bytes before it in the same state (they are no quotes), so
// the blank-line rule needs no parity of its own.  masks[lane] = the bits under
// tile-entering parity 0 (low half) and 1 (high half).
__global__ __launch_bounds__(256) void q_count(const uint8_t* __restrict__ b,
                                               QE* __restrict__ tile,
                                               uint32_t* __restrict__ masks) {
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * 16;
  const uint4 v = *reinterpret_cast<const uint4*>(b + base);
  uint8_t by[16];
  memcpy(by, &v, 16);
  unsigned par = 0, m0 = 0, m1 = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint8_t ch = by[j];
    if (ch == '"') {
      par ^= 1u;
    } else if (ch == '\n') {
      const int64_t p = base + j;
      const uint8_t c1 = j >= 1 ? by[j - 1] : (p >= 1 ? b[p - 1] : 0);
      const uint8_t c2 = j >= 2 ? by[j - 2] : (p >= 2 ? b[p - 2] : 0);
      if (is_rec_end(p, c1, c2)) {
        if (par) m1 |= 1u << j;
        else m0 |= 1u << j;
      }
    }
  }
  QE tot;
  const QE ex = wg256_exscan(qe_make(__popc(m0), __popc(m1), par), &tot);
  const unsigned lo = ex.q ? m1 : m0, hi = ex.q ? m0 : m1;
  masks[(int64_t)blockIdx.x * 256 + threadIdx.x] = lo | (hi << 16);
  if (threadIdx.x == 0) tile[blockIdx.x] = tot;
}

// sc[0] = records (terminators + the tail record), sc[5] = 1 when the bytes
// after the last terminator are a record (a last line without '\n', or an open
// quote: its end index nbytes is then written last), sc[6] = the final parity.
__global__ void q_total(const QE* __restrict__ pre, int64_t ntiles,
                        const uint8_t* __restrict__ b, int64_t nbytes,
                        long long* __restrict__ sc) {
  const QE all = pre[ntiles];
  long long tail = 0;
  if (all.q) {
    tail = 1;
  } else if (nbytes > 0 && b[nbytes - 1] != '\n') {
    const uint8_t c1 = b[nbytes - 1], c2 = nbytes >= 2 ? b[nbytes - 2] : '\n';
    tail = !(c1 == '\r' && c2 == '\n');
  }
  sc[0] = all.c0 + tail;
  sc[5] = tail;
  sc[6] = (long long)all.q;
}

__global__ __launch_bounds__(256) void q_write(const uint32_t* __restrict__ masks,
                                               const QE* __restrict__ pre,
                                               long long* __restrict__ ends) {
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * 16;
  const uint32_t mm = masks[(int64_t)blockIdx.x * 256 + threadIdx.x];
  const QE p = pre[blockIdx.x];
  unsigned m = p.q ? mm >> 16 : mm & 0xFFFFu;
  QE tot;
  const int cnt = __popc(m);
  long long o = p.c0 + wg256_exscan(qe_make(cnt, cnt, 0), &tot).c0;
  while (m) {
    const int j = __ffs(m) - 1;
    m &= m - 1;
    ends[o++] = base + j;
  }
}

struct ParseArgs {
  const uint8_t* b;        // the body, 16-byte aligned, a zero tile after the last
  const long long* ends;   // per record: byte index of its terminator
  int64_t nrec, nblk, n_pad;
  const int16_t* colmap;   // per file column: its feature slot, or -1
  int n_cols, d;
  double* x;               // planar [d4][n_pad]
  QE* defel;               // per block: its deferred rows (as a scan element)
  unsigned long long* defmask;  // per block: which of its rows are deferred
  unsigned* wgcnt;         // per workgroup: 64 counters [slot][kind]
  long long* sc;           // sc[1]: first guard offset (atomicMin)
};

// One record: buf = the bytes from a0 on (LDS stage or global), st = position
// (relative to a0) just after the previous record, e0 = position of this
// record's terminator.  Returns bit 0: the row is deferred, bit 1: its cells were
// classified (kinds, 2 bits per slot).
__device__ __forceinline__ unsigned parse_row(const uint8_t* buf, int64_t st, int64_t e0,
                                              int64_t a0, int64_t r, const ParseArgs& a,
                                              unsigned* kinds_out) {
  int64_t s = st;  // skip the blank lines before the record ("\n", "\r\n")
  for (;;) {
    const uint8_t ch = buf[s];
    if (ch == '\n') ++s;
    else if (ch == '\r' && buf[s + 1] == '\n') s += 2;
    else break;
  }
  int64_t e = e0;
  if (e > s && buf[e - 1] == '\r') --e;
  // The wave walks field by field, not byte by byte: the field index and its
  // slot are the same for every lane, so the 64 lanes run csvp_cell on their
  // cell of a selected column together (a lane that met its comma earlier only
  // waits for the longest field of the wave).  Cells parsed one lane at a time,
  // wherever each lane's comma happened to stand, made the kernel three times
  // as slow.
  int nf = 0;
  int64_t k = s;
  unsigned kinds = 0;
  bool quote = false, bad = false, blank = e > s, celldef = false, ended = false;
  for (int f = 0; f < a.n_cols; ++f) {
    const int slot = a.colmap[f];
    const int64_t fs = k;
    if (!ended) {
      while (k < e) {
        const uint8_t ch = buf[k];
        quote |= ch == '"';
        bad |= ch == 0 || ch == '\r';
        blank &= ch == ' ' || ch == '\t';
        if (ch == ',') break;
        ++k;
      }
    }
    if (slot >= 0 && !ended) {
      double v = 0.0;
      const int64_t len = k - fs;
      const int kind = len <= kMaxCell ? csvp_cell(buf + fs, (int)len, &v) : (int)CSVP_DEFER;
      if (kind == CSVP_DEFER) celldef = true;
      else a.x[(int64_t)slot * a.n_pad + r] = v;
      kinds |= (unsigned)kind << (2 * slot);
    }
    if (!ended) {
      ++nf;
      if (k < e) ++k;  // past the comma: the next field starts (it may be empty)
      else ended = true;
    }
  }
  // a row that has not ended holds more fields than the header: its flags still count
  for (; !ended && k < e; ++k) {
    const uint8_t ch = buf[k];
    quote |= ch == '"';
    bad |= ch == 0 || ch == '\r';
    blank = false;
  }
  const bool shaped = ended && nf == a.n_cols && !quote && !bad && !blank;
  if (quote) {
    const int64_t g = guard_walk(buf, s, e);
    if (g >= 0) atomicMin(&a.sc[1], (long long)(a0 + g));
  }
  if (blank) atomicMin(&a.sc[1], (long long)(a0 + s));  // pandas skips such a line
  *kinds_out = kinds;
  return (shaped && !celldef ? 0u : 1u) | (shaped ? 2u : 0u);
}

__global__ __launch_bounds__(kRows) void parse(ParseArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStage + 16];
  const int lane = threadIdx.x;
  unsigned acc = 0;  // lane 4 j + kind: cells of that kind in slot j
  for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
    const int64_t r0 = blk * kRows;
    const int64_t r1 = min<int64_t>(a.nrec, r0 + kRows);
    const int64_t lo = r0 == 0 ? 0 : a.ends[r0 - 1] + 1;
    const int64_t hi = a.ends[r1 - 1];
    const int64_t a0 = lo & ~(int64_t)15;
    const int64_t r = r0 + lane;
    // byte positions are relative to a0
    const int64_t e0 = r < r1 ? a.ends[r] - a0 : 0;
    const int64_t st = r < r1 ? (r == r0 ? lo : a.ends[r - 1] + 1) - a0 : 0;
    unsigned flags = 0, kinds = 0;
    if (hi - a0 <= kStage) {
      const int nvec = (int)((hi - a0 + 16) >> 4);  // byte hi (the last terminator) included
      for (int v = lane; v < nvec; v += kRows)
        reinterpret_cast<uint4*>(stage)[v] = reinterpret_cast<const uint4*>(a.b + a0)[v];
      __syncthreads();
      if (r < r1) flags = parse_row(stage, st, e0, a0, r, a, &kinds);
    } else if (r < r1) {
      flags = parse_row(a.b + a0, st, e0, a0, r, a, &kinds);
    }
    const unsigned long long dm = __ballot((flags & 1u) != 0);
    if (lane == 0) {
      a.defmask[blk] = dm;
      const long long cnt = __popcll(dm);
      a.defel[blk] = qe_make(cnt, cnt, 0);
    }
    const bool shaped = (flags & 2u) != 0;
    for (int j = 0; j < a.d; ++j) {
      const unsigned kd = (kinds >> (2 * j)) & 3u;
#pragma unroll
      for (unsigned kk = 0; kk < 4; ++kk) {
        const unsigned cnt = (unsigned)__popcll(__ballot(shaped && kd == kk));
        if (lane == 4 * j + (int)kk) acc += cnt;
      }
    }
    __syncthreads();  // the stage is refilled by the next iteration
  }
  a.wgcnt[(int64_t)blockIdx.x * 64 + lane] = acc;
}

__global__ __launch_bounds__(64) void cnt_reduce(const unsigned* __restrict__ wgcnt, int nwg,
                                                 long long* __restrict__ out) {
  long long s = 0;
  for (int g = 0; g < nwg; ++g) s += wgcnt[(int64_t)g * 64 + threadIdx.x];
  out[threadIdx.x] = s;
}

__global__ __launch_bounds__(kRows) void def_write(const unsigned long long* __restrict__ defmask,
                                                   const QE* __restrict__ pre,
                                                   const long long* __restrict__ ends,
                                                   int64_t nblk, int64_t cap,
                                                   long long* __restrict__ list) {
  const int64_t blk = blockIdx.x;
  const unsigned long long m = defmask[blk];
  const int lane = threadIdx.x;
  if (!((m >> lane) & 1ull)) return;
  const long long idx = pre[blk].c0 + __popcll(m & ((1ull << lane) - 1ull));
  if (idx >= cap) return;
  const int64_t r = blk * kRows + lane;
  list[3 * idx] = r;
  list[3 * idx + 1] = r ? ends[r - 1] + 1 : 0;
  list[3 * idx + 2] = ends[r];
}

__global__ void scatter_rows(const long long* __restrict__ rows, const double* __restrict__ vals,
                             int64_t m, int d, int64_t n_pad, double* __restrict__ x) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m * d;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / d;
    const int f = (int)(t - i * d);
    x[(int64_t)f * n_pad + rows[i]] = vals[t];
  }
}

__global__ void planar_to_rowmajor(const double* __restrict__ x, int64_t row0, int64_t rows, int d,
                                   int64_t n_pad, double* __restrict__ dst) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * d;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / d;
    const int f = (int)(t - i * d);
    dst[t] = x[(int64_t)f * n_pad + row0 + i];
  }
}

int gsz(int64_t work, int threads, int cap) {
  const int64_t g = (work + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Exclusive scan of el[0, n) into pre[0, n] (pre[n] = the total); n >= 1.
void qe_scan(Ctx& c, const QE* el, int64_t n, QE* pre) {
  const int64_t nparts = ceil_div(n, kScanPart);
  c.cin_part.ensure(sizeof(QE) * nparts);
  QE* part = c.cin_part.as<QE>();
  hipLaunchKernelGGL(qe_scan_part, dim3(nparts), dim3(256), 0, c.stream, el, n, part);
  hipLaunchKernelGGL(qe_scan_mid, dim3(1), dim3(256), 0, c.stream, part, nparts);
  hipLaunchKernelGGL(qe_scan_out, dim3(nparts), dim3(256), 0, c.stream, el, n, part, pre);
  HIP_CHECK(hipGetLastError());
}

struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t& v : e)
      if (v) (void)hipEventDestroy(v);
  }
};

}  // namespace

// The record index of the body in c.cin_bytes (nb > 0 bytes, zero-padded to a
// whole tile and one more), for csv_read and plan.hip.  csv_index_count runs
// q_count, the scan and q_total and reads c.cin_sc back into r8 (r8[0] records,
// r8[5] the tail record, r8[6] the final parity); csv_index_write then fills
// c.cin_ends[0, nrec) (the caller has sized it).
void csv_index_count(Ctx& c, int64_t nb, long long* r8) {
  const int64_t ntiles = ceil_div(nb, kTile);
  const uint8_t* db = c.cin_bytes.as<uint8_t>();
  long long* sc = c.cin_sc.as<long long>();
  c.cin_tile.ensure(sizeof(QE) * (2 * ntiles + 1));
  QE* tile = c.cin_tile.as<QE>();
  QE* pre = tile + ntiles;
  c.cin_mask.ensure(4 * 256 * ntiles);
  hipLaunchKernelGGL(q_count, dim3(ntiles), dim3(256), 0, c.stream, db, tile,
                     c.cin_mask.as<uint32_t>());
  qe_scan(c, tile, ntiles, pre);
  hipLaunchKernelGGL(q_total, dim3(1), dim3(1), 0, c.stream, pre, ntiles, db, nb, sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(r8, sc, 8 * sizeof(long long), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

void csv_index_write(Ctx& c, int64_t nb, int64_t nrec, bool tail) {
  const int64_t ntiles = ceil_div(nb, kTile);
  hipLaunchKernelGGL(q_write, dim3(ntiles), dim3(256), 0, c.stream, c.cin_mask.as<uint32_t>(),
                     c.cin_tile.as<QE>() + ntiles, c.cin_ends.as<long long>());
  HIP_CHECK(hipGetLastError());
  if (tail) {  // the tail record's end goes last
    *c.h_small.as<long long>() = nb;
    HIP_CHECK(hipMemcpyAsync(c.cin_ends.as<long long>() + nrec - 1, c.h_small.p, 8,
                             hipMemcpyHostToDevice, c.stream));
  }
}

void csv_read(Ctx& c, const char* bytes, int64_t nbytes, int64_t body_off, int32_t n_cols,
              const int32_t* sel, int32_t d, int64_t* status, int64_t* col_kinds,
              int64_t* deferred, int64_t deferred_cap) {
  if (d < 1 || d > kMaxSel) CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv read: d outside [1, 16]");
  if (n_cols < 1 || n_cols > 32767)
    CDR_FAIL(CDR_ERR_UNSUPPORTED, "csv read: n_cols outside [1, 32767]");
  if (nbytes < 0 || body_off < 0 || body_off > nbytes || deferred_cap < 0)
    CDR_FAIL(CDR_ERR_ARG, "csv read: bad size");
  std::vector<int16_t> colmap(n_cols, (int16_t)-1);
  for (int j = 0; j < d; ++j) {
    if (sel[j] < 0 || sel[j] >= n_cols) CDR_FAIL(CDR_ERR_ARG, "csv read: column outside the file");
    if (colmap[sel[j]] >= 0) CDR_FAIL(CDR_ERR_ARG, "csv read: a column selected twice");
    colmap[sel[j]] = (int16_t)j;
  }
  c.cin_pending = false;
  c.plan_rows = -1;  // the index buffers are rewritten
  c.h_small.ensure(64);
  for (double& v : c.cin_ms) v = 0.0;
  const int64_t nb = nbytes - body_off;
  const int64_t ntiles = nb > 0 ? ceil_div(nb, kTile) : 0;
  const size_t padded = (size_t)(ntiles + 1) * kTile;  // a zero tile after the last
  Events ev;
  for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  c.cin_bytes.ensure(padded);
  uint8_t* db = c.cin_bytes.as<uint8_t>();
  HIP_CHECK(hipMemsetAsync(db + nb, 0, padded - nb, c.stream));
  if (nb > 0) HIP_CHECK(hipMemcpyAsync(db, bytes + body_off, nb, hipMemcpyHostToDevice, c.stream));
  c.cin_sc.ensure(8 * 8 + 8 * 64);
  long long* sc = c.cin_sc.as<long long>();
  long long* d_kinds = sc + 8;
  const long long init[8] = {0, LLONG_MAX, 0, 0, 0, 0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(sc, init, sizeof(init), hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemsetAsync(d_kinds, 0, 8 * 64, c.stream));
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  long long nrec = 0;
  bool tail = false;
  if (ntiles > 0) {
    long long r8[8];
    csv_index_count(c, nb, r8);
    nrec = r8[0];
    tail = r8[5] != 0;
    if (nrec < 0 || nrec > nb) CDR_FAIL(CDR_ERR_STATE, "csv read: inconsistent record count");
  }
  points_begin_resident(c, nrec, d);
  long long ndef = 0;
  if (nrec > 0) {
    const int64_t nblk = ceil_div(nrec, kRows);
    const int grid = (int)std::min<int64_t>(nblk, kParseGrid);
    c.cin_ends.ensure(8 * nrec);
    c.cin_blk.ensure(sizeof(QE) * (2 * nblk + 1) + 8 * nblk);
    QE* defel = c.cin_blk.as<QE>();
    QE* defpre = defel + nblk;
    unsigned long long* defmask = reinterpret_cast<unsigned long long*>(defpre + nblk + 1);
    c.cin_cnt.ensure(4 * 64 * (size_t)grid);
    c.cin_map.ensure(2 * (size_t)n_cols);
    HIP_CHECK(hipMemcpyAsync(c.cin_map.p, colmap.data(), 2 * (size_t)n_cols, hipMemcpyHostToDevice,
                             c.stream));
    csv_index_write(c, nb, nrec, tail);
    HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
    ParseArgs a;
    a.b = db;
    a.ends = c.cin_ends.as<long long>();
    a.nrec = nrec;
    a.nblk = nblk;
    a.n_pad = c.n_pad;
    a.colmap = c.cin_map.as<int16_t>();
    a.n_cols = n_cols;
    a.d = d;
    a.x = c.x64.as<double>();
    a.defel = defel;
    a.defmask = defmask;
    a.wgcnt = c.cin_cnt.as<unsigned>();
    a.sc = sc;
    hipLaunchKernelGGL(parse, dim3(grid), dim3(kRows), 0, c.stream, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
    hipLaunchKernelGGL(cnt_reduce, dim3(1), dim3(64), 0, c.stream, c.cin_cnt.as<unsigned>(), grid,
                       d_kinds);
    qe_scan(c, defel, nblk, defpre);
    HIP_CHECK(hipMemcpyAsync(c.h_small.p, defpre + nblk, sizeof(QE), hipMemcpyDeviceToHost,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    ndef = c.h_small.as<QE>()->c0;
    if (ndef < 0 || ndef > nrec) CDR_FAIL(CDR_ERR_STATE, "csv read: inconsistent deferred count");
    const int64_t take = std::min<int64_t>(ndef, deferred_cap);
    if (take > 0) {
      if (!deferred) CDR_FAIL(CDR_ERR_ARG, "null argument");
      c.cin_def.ensure(24 * (size_t)take);
      hipLaunchKernelGGL(def_write, dim3(nblk), dim3(kRows), 0, c.stream, defmask, defpre,
                         c.cin_ends.as<long long>(), nblk, take, c.cin_def.as<long long>());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(deferred, c.cin_def.p, 24 * (size_t)take, hipMemcpyDeviceToHost,
                               c.stream));
    }
  } else {
    HIP_CHECK(hipEventRecord(ev.e[2], c.stream));
    HIP_CHECK(hipEventRecord(ev.e[3], c.stream));
  }
  long long r[8 + 64];
  HIP_CHECK(hipMemcpyAsync(r, sc, sizeof(r), hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  const int64_t take = std::min<int64_t>(ndef, deferred_cap);
  for (int64_t i = 0; i < take; ++i) {  // byte offsets of the file, not of the body
    deferred[3 * i + 1] += body_off;
    deferred[3 * i + 2] += body_off;
  }
  status[0] = nrec;
  status[1] = ndef;
  status[2] = r[1] == LLONG_MAX ? -1 : r[1] + body_off;
  for (int j = 0; j < 4 * d; ++j) col_kinds[j] = r[8 + j];
  float up = 0.f, index = 0.f, prs = 0.f;
  (void)hipEventElapsedTime(&up, ev.e[0], ev.e[1]);
  (void)hipEventElapsedTime(&index, ev.e[1], ev.e[2]);
  (void)hipEventElapsedTime(&prs, ev.e[2], ev.e[3]);
  c.cin_ms[0] = up;
  c.cin_ms[1] = index;
  c.cin_ms[2] = prs;
  c.cin_pending = true;
}

void csv_read_finish(Ctx& c, const int64_t* rows, const double* values, int64_t m, double* X_out) {
  if (!c.cin_pending) CDR_FAIL(CDR_ERR_STATE, "csv read: no read to finish (cdr_csv_read)");
  if (m < 0 || m > c.n) CDR_FAIL(CDR_ERR_ARG, "csv read: more patched rows than rows");
  for (int64_t i = 0; i < m; ++i)
    if (rows[i] < 0 || rows[i] >= c.n) CDR_FAIL(CDR_ERR_ARG, "csv read: patched row out of range");
  c.cin_pending = false;  // whatever happens below, the read is over
  const int d = c.d;
  Events ev;
  HIP_CHECK(hipEventCreate(&ev.e[0]));
  HIP_CHECK(hipEventCreate(&ev.e[1]));
  HIP_CHECK(hipEventRecord(ev.e[0], c.stream));
  if (m > 0) {
    DevBuf dr, dv;
    dr.ensure(8 * (size_t)m);
    dv.ensure(8 * (size_t)m * d);
    HIP_CHECK(hipMemcpyAsync(dr.p, rows, 8 * (size_t)m, hipMemcpyHostToDevice, c.stream));
    HIP_CHECK(hipMemcpyAsync(dv.p, values, 8 * (size_t)m * d, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(scatter_rows, dim3(gsz(m * d, 256, 4096)), dim3(256), 0, c.stream,
                       dr.as<long long>(), dv.as<double>(), m, d, c.n_pad, c.x64.as<double>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    dr.release();
    dv.release();
    HIP_CHECK(e);
  }
  if (X_out && c.n > 0) {
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(32 << 20) / d);
    DevBuf stage;
    stage.ensure(8 * (size_t)std::min<int64_t>(chunk, c.n) * d);
    hipError_t e = hipSuccess;
    for (int64_t r0 = 0; r0 < c.n && e == hipSuccess; r0 += chunk) {
      const int64_t rows_now = std::min(chunk, c.n - r0);
      hipLaunchKernelGGL(planar_to_rowmajor, dim3(gsz(rows_now * d, 256, 4096)), dim3(256), 0,
                         c.stream, c.x64.as<double>(), r0, rows_now, d, c.n_pad,
                         stage.as<double>());
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(X_out + r0 * d, stage.p, 8 * (size_t)rows_now * d,
                           hipMemcpyDeviceToHost, c.stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    }
    stage.release();
    HIP_CHECK(e);
  }
  HIP_CHECK(hipEventRecord(ev.e[1], c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  float fin = 0.f;
  (void)hipEventElapsedTime(&fin, ev.e[0], ev.e[1]);
  c.cin_ms[3] = fin;
  points_finish_resident(c);
}

}  // namespace cdr

using namespace cdr;

extern "C" {

int cdr_csv_read(cdr_ctx* h, const char* bytes, int64_t nbytes, int64_t body_off, int32_t n_cols,
                 const int32_t* sel, int32_t d, int64_t* status, int64_t* col_kinds,
                 int64_t* deferred, int64_t deferred_cap) {
  CDR_TRY
  if (!h || !sel || !status || !col_kinds || (nbytes > 0 && !bytes))
    CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  csv_read(h->c, bytes, nbytes, body_off, n_cols, sel, d, status, col_kinds, deferred,
           deferred_cap);
  CDR_CATCH
}

int cdr_csv_read_finish(cdr_ctx* h, const int64_t* rows, const double* values, int64_t m,
                        double* X_out) {
  CDR_TRY
  if (!h || (m > 0 && (!rows || !values))) CDR_FAIL(CDR_ERR_ARG, "null argument");
  HIP_CHECK(hipSetDevice(h->c.device));
  csv_read_finish(h->c, rows, values, m, X_out);
  CDR_CATCH
}

int cdr_csv_read_timing(cdr_ctx* h, double* out) {
  CDR_TRY
  if (!h || !out) CDR_FAIL(CDR_ERR_ARG, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = h->c.cin_ms[i];
  CDR_CATCH
}

}  // extern "C"
