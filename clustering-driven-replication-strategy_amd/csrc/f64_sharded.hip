// f64_sharded.hip — the exact F64 sums of f64sum.hip over rows sharded on
// several ranks.
// ---------------------------------------------------------------------------
// Sharded F64 sums (include/cdr.h cdr_f64s_*).  Rows are sharded in rank
// order, so sums[j][f] is the sequential sum over shard 0's members, then
// shard 1's, ...: every shard but the first needs the exact running value the
// earlier shards leave, which is not known until they are done.  Instead of a
// rank chain, every shard describes its part of each sequence as a PROGRAM
// built from approximate quantities only, and every rank runs all programs in
// rank order from the exact start:
//   * each rank all-gathers its approximate per-sequence totals (any order)
//     and member counts; a shard's blocks get their binade predictions from
//     the earlier shards' approximate total + its own approximate prefix
//     (f64_predict_*, offset), and their transfers under them (f64_transfer);
//   * rank 0 starts from the exact start (nothing), so it walks (f64_walk)
//     and publishes the exact result: CONST {s, any};
//   * rank r > 0 publishes, per sequence, RUN {e, D0, D1} for every maximal
//     run of member blocks predicted in one binade e with no crossing inside
//     (the start and end predictions agree) and usable transfers, composed
//     (xc_compose; whole groups from f64_group with the end condition), and
//     ELEM {x} for every member of any other block (a binade crossing, a
//     flagged transfer, the sequence's first member, a negative addend);
//   * composing (f64s_compose): a RUN applies only when the exact running
//     value is in its binade and stays there (the transfer test: exact, as
//     in f64_walk); ELEM adds x in real fp64 (NumPy's first row starts the
//     reduce).  Every rank composes the same all-gathered programs, so the
//     sums and the verdict are the same on every rank; a failed test (a
//     prediction off by a binade) or an overfull program makes every rank
//     take the exact rank chain instead (f64s_chain: each shard walks from
//     the exact entry in turn).
// ---------------------------------------------------------------------------
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cdr_internal.h"
#include "f64sum.h"

namespace cdr {

namespace {

struct F64Item {
  long long a, b;  // RUN: D0, D1; ELEM / CONST: the value's bits
  int e, kind;     // RUN: binade; CONST: any
};
static_assert(sizeof(F64Item) == 24, "item layout (include/cdr.h)");
constexpr int kF64Run = 1, kF64Elem = 2, kF64Const = 3;

// per-sequence approximate totals [k d] then member counts [k] (as doubles,
// exact below 2^53): one wave per row
__global__ __launch_bounds__(256) void f64s_totals(const double* __restrict__ A,
                                                   const unsigned* __restrict__ cnt, int64_t nb,
                                                   int kd, int k, double* __restrict__ out) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (r >= kd + k) return;
  double v = 0.0;
  if (r < kd) {
    for (int64_t b = lane; b < nb; b += 64) v += A[(int64_t)r * nb + b];
  } else {
    unsigned long long c = 0;
    for (int64_t b = lane; b < nb; b += 64) c += cnt[(int64_t)(r - kd) * nb + b];
    v = (double)c;
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) out[r] = v;
}

// this rank's offsets (the earlier shards' approximate totals, added left to
// right) and the predicted binade at its end
__global__ __launch_bounds__(256) void f64s_offsets(const double* __restrict__ tot, int nranks,
                                                    int rank, int kd, int k,
                                                    double* __restrict__ off,
                                                    int* __restrict__ Eend) {
  const int stride = kd + k;
  for (int t = threadIdx.x; t < kd; t += blockDim.x) {
    double o = 0.0;
    for (int r = 0; r < rank; ++r) o += tot[(int64_t)r * stride + t];
    off[t] = o;
    Eend[t] = binade_e(o + tot[(int64_t)rank * stride + t]);
  }
}

// rank 0: the walk's exact result as one CONST item per sequence
__global__ __launch_bounds__(256) void f64s_const(const double* __restrict__ sums,
                                                  const double* __restrict__ tot, int kd, int d,
                                                  int k, int cap, F64Item* __restrict__ slot) {
  for (int t = threadIdx.x; t < kd; t += blockDim.x) {
    F64Item* it = slot + (int64_t)t * (cap + 1);
    const bool any = tot[kd + t / d] > 0.0;
    it[0] = F64Item{1, 0, 0, 0};
    it[1] = F64Item{__double_as_longlong(sums[t]), 0, any ? 1 : 0, kF64Const};
  }
}

// rank r > 0: one wave per (cluster, feature) sequence builds its program
// (header item: count, or -1 when it would exceed cap items)
template <typename TA>
__global__ __launch_bounds__(256) void f64s_program(const double* __restrict__ X, int64_t n,
                                                    int64_t n_pad, int d, int k, int64_t nb,
                                                    const int32_t* __restrict__ labels,
                                                    const unsigned* __restrict__ cnt,
                                                    const int* __restrict__ E,
                                                    const int* __restrict__ Eend,
                                                    const Xfer* __restrict__ T,
                                                    const GXfer* __restrict__ G, int64_t ng,
                                                    int cap, F64Item* __restrict__ slot) {
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (t >= k * d) return;
  const int j = t / d, f = t % d;
  F64Item* out = slot + (int64_t)t * (cap + 1);
  int nit = 0;  // items so far (wave-uniform)
  auto emit = [&](long long a, long long b, int e, int kind) {
    if (nit < cap && lane == 0) out[1 + nit] = F64Item{a, b, e, kind};
    ++nit;
  };
  bool run_on = false;
  int run_e = kENone;
  XferC run{0, 0, 2};
  auto add_run = [&](int e, long long d0, long long d1, int p) {
    const XferC x{d0, d1, p};
    if (run_on && run_e == e) {
      run = xc_compose(run, x);
    } else {
      if (run_on) emit(run.d0, run.d1, run_e, kF64Run);
      run = x;
      run_e = e;
      run_on = true;
    }
  };
  auto rd64 = [&](long long v, int l) {
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l)
                        << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)v, l));
  };
  const GXfer* Gt = G + (int64_t)t * ng;
  for (int64_t g0 = 0; g0 < ng; g0 += 64) {
    const GXfer gl = g0 + lane < ng ? Gt[g0 + lane] : GXfer{0, 0, kENone, 0};
    unsigned long long todo = __ballot((gl.p & 8) != 0);
    while (todo) {
      const int gi = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int gp = __builtin_amdgcn_readlane(gl.p, gi);
      if (gp & 4) {  // every member usable, one binade, no crossing inside
        add_run(__builtin_amdgcn_readlane(gl.e, gi), rd64(gl.d0, gi), rd64(gl.d1, gi), gp & 3);
        continue;
      }
      const int64_t b0 = (g0 + gi) * 64;
      const int64_t bl = b0 + lane;
      const bool in = bl < nb;
      const unsigned c = in ? cnt[(int64_t)j * nb + bl] : 0u;
      const int el = in ? E[(int64_t)t * nb + bl] : kENone;
      const int ea = in ? (bl + 1 < nb ? E[(int64_t)t * nb + bl + 1] : Eend[t]) : kENone;
      const Xfer xl = in ? T[(int64_t)t * nb + bl] : Xfer{0, 0, 4};
      const bool safe = c != 0 && !(xl.flags & 4) && el != kENone && ea == el;
      unsigned long long mem = __ballot(c != 0);
      const unsigned long long sm = __ballot(safe);
      while (mem) {
        const int i = __builtin_amdgcn_readfirstlane(__ffsll((long long)mem) - 1);
        mem &= mem - 1;
        if ((sm >> i) & 1ull) {
          const long long d0 = rd64(xl.d0, i);
          const int dd = __builtin_amdgcn_readlane(xl.dd, i);
          add_run(__builtin_amdgcn_readlane(el, i), d0, d0 + dd,
                  __builtin_amdgcn_readlane(xl.flags, i) & 3);
          continue;
        }
        // the block's members one by one (row order)
        if (run_on) emit(run.d0, run.d1, run_e, kF64Run);
        run_on = false;
        const int64_t r0 = (b0 + i) * kFB;
        int lj[4];
        double lx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t row = r0 + 64 * q + lane;
          lj[q] = row < n ? labels[row] : -1;
          lx[q] = row < n ? (double)X[xidx(X, f, row, n_pad)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned long long mk = __ballot(lj[q] == j);
          while (mk) {
            const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
            mk &= mk - 1;
            emit(rd64(__double_as_longlong(lx[q]), l), 0, 0, kF64Elem);
          }
        }
      }
    }
  }
  if (run_on) emit(run.d0, run.d1, run_e, kF64Run);
  if (lane == 0) out[0] = F64Item{nit <= cap ? nit : -1, 0, 0, 0};
}

// every rank: the programs of ranks 0 .. nranks-1 in order, one thread per
// sequence; sums[t], counts[j] (exact, from the gathered totals), and
// status |= 1 when a RUN's transfer test failed or a program overflowed
template <typename TA>
__global__ __launch_bounds__(256) void f64s_compose(const F64Item* __restrict__ progs,
                                                    int64_t slot_items, const double* __restrict__ tot,
                                                    int nranks, int kd, int k, int cap,
                                                    double* __restrict__ sums,
                                                    long long* __restrict__ counts,
                                                    int* __restrict__ status) {
  constexpr int MB = SumTraits<TA>::MB, kMinE = SumTraits<TA>::kMinE;
  constexpr long long kTop = 1ll << (MB + 1);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < k) {
    double c = 0.0;
    for (int r = 0; r < nranks; ++r) c += tot[(int64_t)r * (kd + k) + kd + t];
    counts[t] = (long long)c;
  }
  if (t >= kd) return;
  double s = 0.0;
  bool any = false, ok = true;
  for (int r = 0; r < nranks && ok; ++r) {
    const F64Item* it = progs + (int64_t)r * slot_items + (int64_t)t * (cap + 1);
    const long long m = it[0].a;
    if (m < 0 || m > cap) {
      ok = false;
      break;
    }
    for (long long i = 1; i <= m; ++i) {
      const F64Item x = it[i];
      if (x.kind == kF64Run) {
        ok = false;
        if (any && has_binade(s)) {
          int ex;
          frexp(s, &ex);
          if (ex - 1 == x.e && x.e >= kMinE) {
            const long long g = (long long)ldexp(s, MB - x.e);  // exact: s is on the grid
            const long long g2 = g + ((g & 1) ? x.b : x.a);
            if (g2 < kTop) {
              s = ldexp((double)g2, x.e - MB);
              ok = true;
            }
          }
        }
        if (!ok) break;
      } else if (x.kind == kF64Elem) {
        const double v = __longlong_as_double(x.a);
        s = any ? (double)((TA)s + (TA)v) : v;  // NumPy's reduce: the first row starts it
        any = true;
      } else if (x.kind == kF64Const) {
        s = __longlong_as_double(x.a);
        any = x.e != 0;
      }
    }
  }
  sums[t] = s;
  if (!ok) atomicOr(status, 1);
}

}  // namespace

int f64s_cap() {
  static const int cap = exp_env("CDR_F64S_CAP") ? std::max(1, std::atoi(exp_env("CDR_F64S_CAP"))) : 127;
  return cap;
}

// The step's assignment (labels, block sums and counts) and this shard's
// totals into tot_slot (k d + k doubles).  false: shape not covered.
bool f64s_assign_totals(Ctx& c, int k, const double* dC, double* tot_slot) {
  const int d = c.d;
  if (d < 2 || d > 16 || k < 1 || k > kFMaxK) return false;
  const size_t kd = (size_t)k * d;
  if (c.n > 0) {
    enqueue_f64_assign(c, k, dC, nullptr, nullptr);
    hipLaunchKernelGGL(f64s_totals, dim3((unsigned)ceil_div((int64_t)kd + k, 4)), dim3(256), 0,
                       c.stream, c.f64x_A.as<double>(), c.f64x_cnt.as<unsigned>(),
                       ceil_div(c.n, kFB), (int)kd, k, tot_slot);
  } else {
    HIP_CHECK(hipMemsetAsync(tot_slot, 0, sizeof(double) * (kd + k), c.stream));
  }
  HIP_CHECK(hipGetLastError());
  return true;
}

// This shard's program into its slot of prog_all ([nranks][k d][cap + 1]
// items) from the gathered totals tot_all ([nranks][k d + k]).
void f64s_build(Ctx& c, int k, int nranks, int rank, const double* tot_all, void* prog_all) {
  const int d = c.d, cap = f64s_cap();
  const int64_t n = c.n, nb = ceil_div(std::max<int64_t>(n, 1), kFB);
  const int kd = k * d;
  const int64_t slot_items = (int64_t)kd * (cap + 1);
  F64Item* slot = static_cast<F64Item*>(prog_all) + (size_t)rank * slot_items;
  c.f64s_off.ensure(sizeof(double) * kd + sizeof(int) * kd);
  double* off = c.f64s_off.as<double>();
  int* Eend = reinterpret_cast<int*>(off + kd);
  hipLaunchKernelGGL(f64s_offsets, dim3(1), dim3(256), 0, c.stream, tot_all, nranks, rank, kd, k,
                     off, Eend);
  HIP_CHECK(hipGetLastError());
  c.f64_sums.ensure(sizeof(double) * 2 * kd);
  if (n > 0) {
    F64Shard sh;
    sh.off = off;
    sh.Eend = rank > 0 ? Eend : nullptr;  // (rank 0 walks: no crossing condition needed)
    sh.walk = rank == 0;
    enqueue_f64_sums_after_block(c, k, c.f64_sums.as<double>(), sh, nullptr, nullptr);
  }
  if (rank == 0) {
    if (n == 0) HIP_CHECK(hipMemsetAsync(c.f64_sums.p, 0, sizeof(double) * kd, c.stream));
    hipLaunchKernelGGL(f64s_const, dim3(1), dim3(256), 0, c.stream, c.f64_sums.as<double>(),
                       tot_all, kd, d, k, cap, slot);
  } else if (n > 0) {
    const int64_t ng = ceil_div(nb, (int64_t)64);
    hipLaunchKernelGGL(f64s_program<double>, dim3((unsigned)ceil_div((int64_t)kd, 4)), dim3(256), 0,
                       c.stream, c.x64.as<double>(), n, c.n_pad, d, k, nb,
                       c.labels.as<int32_t>(), c.f64x_cnt.as<unsigned>(), c.f64x_E.as<int>(),
                       Eend, c.f64x_T.as<Xfer>(), c.f64x_G.as<GXfer>(), ng, cap, slot);
  } else {  // an empty shard: the identity (no items)
    std::vector<F64Item> z((size_t)slot_items, F64Item{0, 0, 0, 0});
    HIP_CHECK(hipMemcpyAsync(slot, z.data(), sizeof(F64Item) * z.size(), hipMemcpyHostToDevice,
                             c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }
  HIP_CHECK(hipGetLastError());
}

void f64s_compose_all(Ctx& c, int k, int nranks, const double* tot_all, const void* prog_all,
                      double* d_sums, long long* d_counts, int* d_status) {
  const int kd = k * c.d, cap = f64s_cap();
  const int64_t slot_items = (int64_t)kd * (cap + 1);
  HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int), c.stream));
  hipLaunchKernelGGL(f64s_compose<double>, dim3((unsigned)ceil_div(std::max(kd, k), 256)),
                     dim3(256), 0, c.stream, static_cast<const F64Item*>(prog_all), slot_items,
                     tot_all, nranks, kd, k, cap, d_sums, d_counts, d_status);
  HIP_CHECK(hipGetLastError());
}

// The exact rank chain (fallback): this shard walks from the exact entry
// chain[0, 2 k d) = {s, any} and leaves its exit there.
void f64s_chain_walk(Ctx& c, int k, double* chain) {
  const int kd = k * c.d;
  if (c.n == 0) return;  // nothing added: the entry is the exit
  F64Shard sh;
  sh.off = chain;  // the exact entry predicts every binade
  sh.entry = chain;
  sh.walk = true;
  c.f64s_off.ensure(sizeof(double) * kd + sizeof(int) * kd);
  enqueue_f64_sums_after_block(c, k, chain, sh, nullptr, nullptr);
}

}  // namespace cdr
