// seed_common.h — what the seeding files share: k-means++ D^2 seeding
// (reference src/kmeans_plusplus.py:3-22) in four translation units,
//   seed_update.hip  the D^2 update kernels and their dispatcher
//   seed_scan.hip    the exact cumsum scan: program, block walk, search
//   seed_run.hip     the device-resident run and the sharded phases
//   seed_f32r.hip    the reference's float32 seeding
// The library has no relocatable device code: a kernel is launched from the
// file that defines it, and another file reaches it through a host function
// declared at the end of this header.
//
// Per step i (one new centre c):
//   dist_sq = min(dist_sq, norm(X - c)**2)        :14-17  (running min is exact:
//                                                         min is order free)
//   total   = dist_sq.sum()                        :18     NumPy add.reduce: 8192-
//             element chunks, pairwise inside each chunk, chunks added left to right
//   idx     = rng.choice(n, p=dist_sq/total)       :19     = searchsorted(cumsum(p) /
//             cumsum(p)[-1], rng.random(), 'right') (one draw; u comes from host)
//
// The cumulative sum is where a parallel scan would change the rounding.  We
// emulate NumPy's strictly sequential fp64 accumulation exactly:
//   while the running value c stays inside one binade [2^e, 2^(e+1)), every
//   fl(c + p) lands on the grid g = 2^(e-52), so c/g = N is an integer and
//   N' = N + rne(p/g) — independent of N except for exact ties, where round-
//   half-even looks at the parity of N.  A run of elements is therefore a
//   *transfer* (D0, D1): the increment of N when N enters even / odd.  Two
//   transfers compose as D_q = L_q + R_{q ^ (L_q & 1)} (associative), so
//   blocks are reduced in parallel; a single wave then walks the blocks,
//   applying whole blocks inside a binade and walking element by element only
//   across the ~log2(c_last/c_first) binade crossings.
#pragma once

#include "cdr_internal.h"

namespace cdr {

// A block's transfer under the binade guessed for its start (xfer_kernel,
// applied by walk_kernel).
struct Xfer {
  long long d0, d1;
  int e;      // binade exponent the transfer was computed for
  int valid;  // 0: some element would leave the binade / overflow
  long long pad;
};

// Device-resident seeding (seed_run): the total S, the running value at the
// shard's end and the uniform of the draw live in device memory, written by
// the kernels before; a non-zero *gate (the program's success flag) turns the
// block-walk fallback kernels into no-ops.  Null pointers: the by-value
// arguments hold.
struct SeedDev {
  const double* S = nullptr;
  const double* gate = nullptr;
  const double* c_last = nullptr;
  const double* u = nullptr;
  const double* c_in = nullptr;  // (sharded device seeding: the shard's exact start)
};

// ---- the cumsum program (seed_scan.hip, "cumulative-sum programs") ----
// A run: the transfer of consecutive elements under one guessed binade.
struct Part {
  long long d0, d1;
  int e;   // binade exponent (kNoE when empty)
  int st;  // 0 empty (identity), 1 transfer, 2 broken (the guess cannot hold)
};
constexpr int kNoE = -100000;
constexpr long long kD52 = 1ll << 52;

// cdr_seed_item (include/cdr.h)
struct SeedItem {
  long long d0, d1;
  double p;
  int e;
  int kind;
};
static_assert(sizeof(SeedItem) == sizeof(cdr_seed_item), "cdr_seed_item layout");
enum : int {
  kItRun = CDR_SEED_RUN,
  kItCross = CDR_SEED_CROSS,
  kItConst = CDR_SEED_CONST,
  kItFine = CDR_SEED_FINE,
  kItMark = CDR_SEED_MARK,
  kItEnd = CDR_SEED_END,
  kItSkip = CDR_SEED_SKIP,
  kItBad = CDR_SEED_BAD
};

__host__ __device__ __forceinline__ Part part_empty() { return Part{0, 0, kNoE, 0}; }

// L then R
__host__ __device__ __forceinline__ Part part_compose(const Part& L, const Part& R) {
  if (L.st == 0) return R;
  if (R.st == 0) return L;
  if (L.st != 1 || R.st != 1 || L.e != R.e) return Part{0, 0, L.e, 2};
  Part o{L.d0 + ((L.d0 & 1) ? R.d1 : R.d0), L.d1 + ((L.d1 & 1) ? R.d0 : R.d1), L.e, 1};
  if (o.d0 >= kD52 || o.d1 >= kD52) o.st = 2;
  return o;
}

__host__ __device__ __forceinline__ bool sp_binade(double c, int& e, long long& N) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, c);
  const int ef = (int)((bits >> 52) & 0x7FF);
  if (ef == 0 || ef >= 2046 || (bits >> 63)) return false;
  e = ef - 1023;
  N = (long long)((bits & 0xFFFFFFFFFFFFFull) | (1ull << 52));
  return true;
}
__host__ __device__ __forceinline__ double sp_value(int e, long long N) {
  const unsigned long long bits =
      ((unsigned long long)(e + 1023) << 52) | ((unsigned long long)N & 0xFFFFFFFFFFFFFull);
  return __builtin_bit_cast(double, bits);
}

// One RUN / SKIP / BAD / CROSS / CONST item applied to the running value c
// (MARK and END leave it; FINE cannot be applied here).  False: the item does
// not hold for this c (the guessed binade was wrong).
__host__ __device__ __forceinline__ bool item_apply(const SeedItem& it, double& c) {
  switch (it.kind) {
    case kItRun: {
      int e;
      long long N;
      if (!sp_binade(c, e, N) || e != it.e) return false;
      const long long N2 = N + ((N & 1) ? it.d1 : it.d0);
      if (N2 >= (1ll << 53)) return false;
      c = sp_value(e, N2);
      return true;
    }
    case kItSkip:
    case kItMark:
    case kItEnd:
      return true;
    case kItCross:
      c = c + it.p;
      return true;
    case kItConst:
      c = it.p;
      return true;
    default:
      return false;
  }
}

__host__ __device__ __forceinline__ SeedItem run_item(const Part& P) {
  return SeedItem{P.d0, P.d1, 0.0, P.e, P.st == 0 ? kItSkip : (P.st == 1 ? kItRun : kItBad)};
}

// Element p joins run P under binade e (range_transfer_v's step).
__device__ __forceinline__ void part_add(Part& P, double p, int e) {
  if (P.st == 0) P = Part{0, 0, e, 1};
  if (P.st != 1) return;
  if (P.e != e) {
    P.st = 2;
    return;
  }
  const double f = ldexp(p, 52 - e);
  if (!(f < 4503599627370496.0)) {
    P.st = 2;
    return;
  }
  const double fl = floor(f);
  const double frac = f - fl;
  const long long k = (long long)fl;
  const long long up = frac > 0.5 ? 1 : 0;
  const bool tie = frac == 0.5;
  P.d0 += k + up + ((tie && ((P.d0 ^ k) & 1)) ? 1 : 0);
  P.d1 += k + up + ((tie && ((1 ^ P.d1 ^ k) & 1)) ? 1 : 0);
  if (P.d0 >= kD52 || P.d1 >= kD52) P.st = 2;
}

// part_add with the run's counts kept as fp64 integers (exact below 2^53; a
// run stops at 2^52) and their parities as bits: no fp64 -> int64 conversion
// per element (seg_block's loop is VALU-bound); to_part gives the Part that
// part_add would have built from the same elements.
struct PartD {
  double d0, d1;
  int p0, p1;  // parities of d0, d1
  int e, st;
};
__device__ __forceinline__ PartD partd_empty() { return PartD{0.0, 0.0, 0, 0, kNoE, 0}; }
__device__ __forceinline__ void partd_add(PartD& P, double p, int e) {
  if (P.st == 0) P = PartD{0.0, 0.0, 0, 0, e, 1};
  if (P.st != 1) return;
  if (P.e != e) {
    P.st = 2;
    return;
  }
  const double f = ldexp(p, 52 - e);
  if (!(f < 4503599627370496.0)) {
    P.st = 2;
    return;
  }
  const double fl = floor(f);
  const double frac = f - fl;
  // fl < 2^52: in fl + 2^52 the last significand bit is fl's parity
  const int kp = (int)(__double_as_longlong(fl + 4503599627370496.0) & 1);
  const int up = frac > 0.5 ? 1 : 0;
  const int tie = frac == 0.5 ? 1 : 0;
  const int i0 = up | (tie & (P.p0 ^ kp));
  const int i1 = up | (tie & (1 ^ P.p1 ^ kp));
  P.d0 = (P.d0 + fl) + (double)i0;
  P.d1 = (P.d1 + fl) + (double)i1;
  P.p0 ^= kp ^ i0;
  P.p1 ^= kp ^ i1;
  if (P.d0 >= 4503599627370496.0 || P.d1 >= 4503599627370496.0) P.st = 2;
}
__device__ __forceinline__ Part to_part(const PartD& P) {
  return Part{(long long)P.d0, (long long)P.d1, P.e, P.st};
}

constexpr int kKC = 32;  // crossings recorded per block
struct SegTail {
  Part t;      // the run after the block's last crossing (the whole block: none)
  int ncross;  // crossings in the block
  int opaque;  // walked element by element at evaluation
};
struct SegEnt {
  Part pre;  // the run before the crossing (from the block start or the previous crossing)
  double p;  // the crossing element
};
struct SegScan {
  Part s;        // transfer from the block's segment head (exclusive) through the block
  long long lh;  // segment head block (-1: the shard start)
};

// A wave-uniform 64-bit value into scalar registers (the program walks of
// seg_eval_kernel and shard_compose_kernel).
__device__ __forceinline__ long long sgpr64(long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// The left-to-right sum of v[0 .. n) in one wave (the value in every lane).
// The chain of n dependent fp64 (or fp32) adds is the whole cost, so each add
// takes its operand from LDS (a broadcast read, in order under lgkmcnt) and
// the values arrive in chunks: the wave loads chunk c + 1 into registers
// (coalesced, one value per lane per load) while the chain runs over chunk c,
// then writes it to the other LDS buffer.  (Round 5 read each value through
// two v_readlane into SGPRs: three VALU instructions and a hazard wait per
// add, ~2.5x slower.)  Padding past n adds +0.0, which leaves a sum of
// non-negative terms unchanged.
template <typename T>
__device__ __forceinline__ T wave_seq_sum(const T* __restrict__ v, int64_t n) {
  constexpr int kChunk = 1024;       // values per chunk
  constexpr int kPer = kChunk / 64;  // per lane
  __shared__ __attribute__((aligned(16))) T buf[2][kChunk];
  const int lane = threadIdx.x & 63;
  T r[kPer];
  // lane l holds values c0 + l + 64 j of the chunk at c0 (coalesced; no
  // branches: a clamped address and a select, so the loads stay in flight)
  auto load = [&](int64_t c0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t i = c0 + lane + 64 * j;
      r[j] = v[i < n ? i : n - 1];
    }
  };
  // (the select past n here, after the chain: not at the load, where it
  // would wait for the data)
  auto store = [&](T* dst, int64_t c0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) dst[lane + 64 * j] = c0 + lane + 64 * j < n ? r[j] : T(0);
  };
  T s = T(0);
  if (n <= 0) return s;
  load(0);
  store(buf[0], 0);
  int cb = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kChunk) {
    const bool more = c0 + kChunk < n;  // (uniform)
    if (more) load(c0 + kChunk);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const T* src = buf[cb];
    const int m = n - c0 < kChunk ? (int)(n - c0) : kChunk;
    if (m == kChunk) {
      // 16-byte reads kP ahead of the chain (the LDS latency covered by the
      // adds of the kP - 1 reads before)
      constexpr int kVec = 16 / sizeof(T);
      constexpr int kNV = kChunk / kVec;
      constexpr int kP = 8;
      typedef T tv __attribute__((ext_vector_type(kVec)));
      const tv* q = reinterpret_cast<const tv*>(src);
      tv pipe[kP];
#pragma unroll
      for (int i = 0; i < kP; ++i) pipe[i] = q[i];
#pragma unroll
      for (int i = 0; i < kNV; ++i) {
        const tv cur = pipe[i % kP];
        if (i + kP < kNV) pipe[i % kP] = q[i + kP];
#pragma unroll
        for (int e = 0; e < kVec; ++e) s = s + cur[e];
      }
    } else {
      for (int j = 0; j < m; ++j) s = s + src[j];
    }
    if (more) store(buf[cb ^ 1], c0 + kChunk);
    cb ^= 1;
  }
  return s;
}

inline void check_points(const Ctx& c) {
  if (c.mode == 0) CDR_FAIL(CDR_ERR_STATE, "no points loaded");
  if (c.d > 128) CDR_FAIL(CDR_ERR_UNSUPPORTED, "d > 128 is not supported yet");
}

// The program's result on the device: res[0] the running value after the
// shard, res[1] = 1 when every item held (seg_eval_kernel).
inline double* seed_res(Ctx& c) {
  return reinterpret_cast<double*>(c.seg_meta.as<long long>() + 4);
}

// The sharded phases (seed_run.hip)
constexpr int kShardProgCap = 1024;  // program items per rank (item 0: the header)
constexpr int kShardRed = 4;         // red buffer: row (d) | index + 1 | fail | nan | pad
enum : int { kSsS = 0, kSsGuess, kSsMine, kSsAfter, kSsLast, kSsFail, kSsNan, kSsNoHit, kSsWords };

// ---- seed_scan.hip, for the runs of seed_run.hip and seed_f32r.hip ----
// This shard's cumsum program under the guess c_guess of the running value at
// its first element, and its evaluation from the exact c_in (false: a guess
// failed).  Device-resident callers pass dv and c_out == nullptr: nothing is
// read back.
void seed_scan_program(Ctx& c, double total, double c_guess, const SeedDev& dv = SeedDev{});
bool seed_scan_finish(Ctx& c, double c_in, double* c_out, const SeedDev& dv = SeedDev{});
// search_kernel on the context's dmin and cend; the pick goes to out (device).
void seed_search_enqueue(Ctx& c, double total, double c_in, double c_last, double u,
                         int64_t* out, const SeedDev& dv);
// One step's draw with nothing read back, from dmin and the block sums: the
// program, its gated block-walk fallback (walk_only: the walk alone) and the
// search of u[0] * c_last into pick[0].  S: the total on the device, or
// nullptr for dmin already divided (S = 1).
void seed_step_resident(Ctx& c, const double* S, const double* u, int64_t* pick,
                        bool walk_only = false);

}  // namespace cdr
