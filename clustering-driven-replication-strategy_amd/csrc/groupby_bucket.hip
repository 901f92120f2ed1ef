// groupby_bucket.hip — the group-by's counting per bucket of 2^L consecutive
// files (K4 at the head of groupby.hip), from the partition's payloads in
// bucket order to the (files, 6) int64 rows.  Five kernels:
//   gb_bucket        LDS hash of (file, second) -> count, a workgroup per bucket
//   gb_bucket_dense  (file, second) grid of u16 counts, a workgroup per bucket
//                    (both are gb_block, over GbHashTable and GbDenseTable)
//   gb_bucket_wave   the same grid, a wave per bucket (L <= kGwMaxL)
//   gb_bucket_wave4  the same for <= 4 files per bucket, sums in registers
//   gb_bucket_big    buckets over the LDS capacity: the hash in global memory
#include <algorithm>

#include "groupby.h"

namespace cdr {

namespace {

constexpr int kGbBThreads = 256;                // bucket workgroups
constexpr int kGbSlots = 4096;                  // LDS hash slots per bucket
constexpr int kGbReg = kGbLdsCap / kGbBThreads; // payloads per bucket thread
constexpr unsigned long long kEmpty = ~0ull;

struct GbKey {
  int CB;                   // count bits of a hash slot (slot = key << CB | count)
  unsigned long long cmask;
};

GbKey gb_key(const GbPay& p) {
  GbKey k;
  k.CB = 64 - (p.L + p.sbits);
  k.cmask = k.CB >= 64 ? ~0ull : ((1ull << k.CB) - 1);
  return k;
}

__device__ __forceinline__ unsigned gb_hash(unsigned long long key) {
  return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32);
}

// Insert one event of (file-local fl, second code sc) into an open-addressing
// table; returns the pair's count after this event.
template <bool LDS>
__device__ __forceinline__ unsigned long long gb_insert(unsigned long long* slots, unsigned size,
                                                        bool pow2, unsigned long long key,
                                                        const GbKey& k) {
  unsigned h = gb_hash(key);
  h = pow2 ? (h & (size - 1)) : (h % size);
  const unsigned long long fresh = (key << k.CB) | 1ull;
  while (true) {
    // one CAS claims an empty slot (the common case: a new (file, second)
    // pair) or returns the occupant
    const unsigned long long v = atomicCAS(&slots[h], kEmpty, fresh);
    if (v == kEmpty) return 1;
    if ((v >> k.CB) == key) return (atomicAdd(&slots[h], 1ull) & k.cmask) + 1;
    h = h + 1 == size ? 0 : h + 1;
  }
}

// Per-file LDS state of a bucket (F = 2^L files), after the hash slots.
struct GbFiles {
  unsigned long long* cw;   // count | writes << 32
  unsigned long long* rl;   // reads | local << 32
  unsigned* conc;
  int* prim;
};

__device__ __forceinline__ GbFiles gb_files(unsigned long long* base, int F) {
  GbFiles g;
  g.cw = base;
  g.rl = base + F;
  g.conc = reinterpret_cast<unsigned*>(base + 2 * F);
  g.prim = reinterpret_cast<int*>(g.conc + F);
  return g;
}

// A wave's events (act: this lane holds one, of file-local fl, op code oc,
// loc: from its file's primary): count / writes / reads / local are added
// once per group of lanes of one file (ballots over the L file-local bits),
// so a bucket's few files do not serialise the LDS atomics.
__device__ __forceinline__ void gb_file_sums(GbFiles& g, bool act, unsigned fl, unsigned oc,
                                             bool loc, int L) {
  unsigned long long peers = __ballot(act);
  for (int b = 0; b < L; ++b) {
    const bool bit = (fl >> b) & 1u;
    const unsigned long long bb = __ballot(act && bit);
    peers &= bit ? bb : ~bb;
  }
  const unsigned long long mw = __ballot(act && oc == 1), mr = __ballot(act && oc == 2);
  const unsigned long long ml = __ballot(act && loc);
  const int lane = threadIdx.x & 63;
  if (act && lane == __ffsll((long long)peers) - 1) {
    atomicAdd(&g.cw[fl], (unsigned long long)__popcll(peers) |
                             ((unsigned long long)__popcll(peers & mw) << 32));
    atomicAdd(&g.rl[fl], (unsigned long long)__popcll(peers & mr) |
                             ((unsigned long long)__popcll(peers & ml) << 32));
  }
}

// The event of client cl (its code - 1) came from its file's primary node.
__device__ __forceinline__ bool gb_local(int cl, int prim) {
  return cl >= 0 && prim >= 0 && cl == prim;
}

// One event of the hash kernels: hash insert, concurrency maximum, file sums.
template <bool LDS>
__device__ __forceinline__ void gb_event(bool act, unsigned long long v, const GbPay& p,
                                         const GbKey& k, unsigned long long* slots,
                                         unsigned size, bool pow2, GbFiles& g) {
  const GbFields e = gb_decode(v, p);
  const int cl = gb_client(e.cc);
  bool loc = false;
  if (act) {
    const unsigned long long cnt =
        gb_insert<LDS>(slots, size, pow2, ((unsigned long long)e.fl << p.sbits) | e.sc, k);
    const unsigned c32 = (unsigned)min(cnt, 0xFFFFFFFFull);
    if (c32 > g.conc[e.fl]) atomicMax(&g.conc[e.fl], c32);
    loc = gb_local(cl, g.prim[e.fl]);
  }
  gb_file_sums(g, act, e.fl, e.oc, loc, p.L);
}

__device__ __forceinline__ void gb_write_files(const GbFiles& g, int nfl, int64_t f0,
                                               long long* __restrict__ out) {
  for (int f = threadIdx.x; f < nfl; f += kGbBThreads) {
    long long* o = out + (f0 + f) * 6;
    const unsigned long long cw = g.cw[f], rl = g.rl[f];
    o[0] = (long long)(cw & 0xFFFFFFFFull);
    o[1] = (long long)(cw >> 32);
    o[2] = (long long)(rl & 0xFFFFFFFFull);
    o[3] = (long long)(rl >> 32);
    o[4] = (long long)(cw & 0xFFFFFFFFull);
    o[5] = (long long)g.conc[f];
  }
}

// The persistent workgroup-per-bucket kernel, gb_bucket and gb_bucket_dense by
// the table B it counts a bucket in: workgroup w takes buckets w, w + G,
// w + 2G, ...; the next bucket's payloads and primaries are loaded while the
// current one is counted (a bucket holds ~1k events, so one global round trip
// per bucket would otherwise dominate).  A bucket of more than B::kCap events
// goes on big_list instead.  B is built from (lds, p, out, k...) and has
//   clear(n, nfl, prim)     empty, for n events of nfl files; prim: the files'
//                           primaries, kPrimReg per thread
//   add(act, x)             one event per lane (act: this lane holds one)
//   finish(ev, n, nfl, f0)  after the kGbReg events per thread that add() saw
//                           (all n of them are at ev): the files' rows
// The loop is the kernel's own body: as a function called from two kernels it
// cost both 4-byte instances an occupancy step.
constexpr int kPrimReg = (1 << kGbMaxL) / kGbBThreads;

template <typename T, typename B, typename... K>
__global__ __launch_bounds__(kGbBThreads) void gb_block(
    const T* __restrict__ pb, const unsigned* __restrict__ bbase, int64_t nbuckets, int64_t nf,
    GbPay p, const int32_t* __restrict__ primary, long long* __restrict__ out,
    int* __restrict__ big_list, int* __restrict__ big_count, K... k) {
  extern __shared__ unsigned long long lds[];
  B table(lds, p, out, k...);
  const int tid = threadIdx.x;
  const int F = 1 << p.L;
  const int64_t G = gridDim.x;
  int64_t b = blockIdx.x;
  if (b >= nbuckets) return;
  // bucket b's bounds, payloads (in registers) and primaries
  int64_t s0 = bbase[b], n = (int64_t)bbase[b + 1] - s0;
  T v[kGbReg];
  int pr[kPrimReg];
  auto fetch = [&](int64_t bb, int64_t ss, int64_t nn, T* vv, int* pp) {
    const bool ok = nn <= B::kCap;
#pragma unroll
    for (int j = 0; j < kGbReg; ++j) {
      const int64_t i = tid + j * kGbBThreads;
      vv[j] = ok && i < nn ? pb[ss + i] : (T)0;
    }
    const int64_t f0 = bb << p.L;
#pragma unroll
    for (int j = 0; j < kPrimReg; ++j) {
      const int64_t f = tid + j * kGbBThreads;
      pp[j] = f < F && f0 + f < nf ? primary[f0 + f] : -2;
    }
  };
  fetch(b, s0, n, v, pr);
  int64_t s0n = 0, nn = 0;
  if (b + G < nbuckets) {
    s0n = bbase[b + G];
    nn = (int64_t)bbase[b + G + 1] - s0n;
  }
  T v2[kGbReg];
  int pr2[kPrimReg];
  // One bucket: cur holds it (its loads are waited for at the empty asm,
  // before the next bucket's loads go out into nxt); ping-pong buffers
  // instead of copies, so no copy of an in-flight register forces a wait.
  auto step = [&](T (&cur)[kGbReg], int (&cpr)[kPrimReg], T (&nxt)[kGbReg],
                  int (&npr)[kPrimReg]) {
#pragma unroll
    for (int j = 0; j < kGbReg; ++j) asm volatile("" : "+v"(cur[j]));
#pragma unroll
    for (int j = 0; j < kPrimReg; ++j) asm volatile("" : "+v"(cpr[j]));
    const int64_t bn = b + G;
    const int64_t f0 = b << p.L;
    const int nfl = (int)min((int64_t)F, nf - f0);
    const bool over = n > B::kCap;
    if (!over) table.clear(n, nfl, cpr);
    __syncthreads();
    int64_t s0nn = 0, nnn = 0;
    if (bn < nbuckets) {
      fetch(bn, s0n, nn, nxt, npr);
      if (bn + G < nbuckets) {
        s0nn = bbase[bn + G];
        nnn = (int64_t)bbase[bn + G + 1] - s0nn;
      }
    }
    if (over) {
      if (tid == 0) big_list[atomicAdd(big_count, 1)] = (int)b;
    } else {
#pragma unroll
      for (int j = 0; j < kGbReg; ++j) {
        const bool act = tid + j * kGbBThreads < n;
        if (__ballot(act) == 0) break;
        table.add(act, (unsigned long long)cur[j]);
      }
      table.finish(pb + s0, n, nfl, f0);
    }
    __syncthreads();  // the LDS is cleared for the next bucket
    s0 = s0n;
    n = nn;
    s0n = s0nn;
    nn = nnn;
    b = bn;
  };
  while (true) {
    step(v, pr, v2, pr2);
    if (b >= nbuckets) break;
    step(v2, pr2, v, pr);
    if (b >= nbuckets) break;
  }
}

// gb_bucket's table: kGbSlots hash slots of (file, second) -> count in LDS,
// then the per-file state of F = 2^L files.
struct GbHashTable {
  static constexpr int kCap = kGbLdsCap;
  const GbPay& p;
  const GbKey& k;
  unsigned long long* slots;
  GbFiles g;
  long long* out;
  unsigned size = 64;  // slots in use for this bucket

  __device__ __forceinline__ GbHashTable(unsigned long long* lds, const GbPay& p_,
                                         long long* out_, const GbKey& k_)
      : p(p_), k(k_), slots(lds), g(gb_files(lds + kGbSlots, 1 << p_.L)), out(out_) {}
  __device__ __forceinline__ void clear(int64_t n, int nfl, const int (&prim)[kPrimReg]) {
    const int tid = threadIdx.x;
    size = 64;
    while (size < 2 * n && size < kGbSlots) size <<= 1;
    for (unsigned i = tid; i < size; i += kGbBThreads) slots[i] = kEmpty;
#pragma unroll
    for (int j = 0; j < kPrimReg; ++j) {
      const int f = tid + j * kGbBThreads;
      if (f < nfl) {
        g.cw[f] = 0;
        g.rl[f] = 0;
        g.conc[f] = 0;
        g.prim[f] = prim[j];
      }
    }
  }
  __device__ __forceinline__ void add(bool act, unsigned long long x) {
    gb_event<true>(act, x, p, k, slots, size, true, g);
  }
  template <typename T>
  __device__ __forceinline__ void finish(const T*, int64_t, int nfl, int64_t f0) {
    __syncthreads();
    gb_write_files(g, nfl, f0, out);
  }
};

template <typename T>
constexpr auto gb_bucket = gb_block<T, GbHashTable, GbKey>;

// gb_bucket_dense's table (2^(L + sbits) <= 2^kGbDenseBits): the bucket's
// (file, second) grid of u16 counts (two per u32 word; bucket events < 2^16,
// so no count overflows), one non-returning LDS add per event; count / writes
// / reads / local per file are added once per group of lanes of one file
// (gb_file_sums), and the concurrency maximum is a max over the file's row at
// the end.
struct GbDenseTable {
  static constexpr int kCap = kGbDenseCap;
  const GbPay& p;
  GbFiles g;
  unsigned* grid;
  long long* out;

  __device__ __forceinline__ GbDenseTable(unsigned long long* lds, const GbPay& p_, long long* out_)
      : p(p_), g(gb_files(lds, 1 << p_.L)),
        grid(reinterpret_cast<unsigned*>(g.prim + (1 << p_.L))), out(out_) {}
  __device__ __forceinline__ void clear(int64_t, int, const int (&prim)[kPrimReg]) {
    const int tid = threadIdx.x;
    const int F = 1 << p.L;
    const int KW = ((F << p.sbits) + 1) >> 1;  // u32 words of the count grid
    for (int i = tid; i < KW; i += kGbBThreads) grid[i] = 0;
#pragma unroll
    for (int j = 0; j < kPrimReg; ++j) {
      const int f = tid + j * kGbBThreads;
      if (f < F) {
        g.cw[f] = 0;
        g.rl[f] = 0;
        g.prim[f] = prim[j];
      }
    }
  }
  __device__ __forceinline__ void add(bool act, unsigned long long x) {
    unsigned fl = 0, oc = 0;
    int cl = -1;
    if (act) {
      const GbFields e = gb_decode(x, p);
      fl = e.fl, oc = e.oc, cl = gb_client(e.cc);
      const unsigned key = (fl << p.sbits) | (unsigned)e.sc;
      atomicAdd(&grid[key >> 1], 1u << ((key & 1u) << 4));
    }
    // (every lane reads a primary, so the read is not behind a branch and its
    // latency passes under the ballots; cl = -1 without an event)
    const int pf = g.prim[fl];
    gb_file_sums(g, act, fl, oc, gb_local(cl, pf), p.L);
  }
  template <typename T>
  __device__ __forceinline__ void finish(const T* ev, int64_t n, int nfl, int64_t f0) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int S = 1 << p.sbits;
    // the events beyond the registers
    for (int64_t i0 = kGbReg * kGbBThreads; i0 < n; i0 += kGbBThreads) {
      const int64_t i = i0 + tid;
      add(i < n, i < n ? (unsigned long long)ev[i] : 0ull);
    }
    __syncthreads();
    // one wave per file: the maximum count over the file's seconds
    for (int f = wv; f < nfl; f += kGbBThreads / 64) {
      const unsigned* row = grid + (((unsigned)f << p.sbits) >> 1);
      const int words = S >= 2 ? S >> 1 : 1;
      unsigned mx = 0;
      for (int w = lane; w < words; w += 64) {
        const unsigned e = row[w];
        const unsigned lo = S >= 2 ? (e & 0xFFFFu) : ((f & 1) ? (e >> 16) : (e & 0xFFFFu));
        const unsigned hi = S >= 2 ? (e >> 16) : 0u;
        mx = max(mx, max(lo, hi));
      }
      for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
      if (lane == 0) g.conc[f] = mx;
    }
    __syncthreads();
    gb_write_files(g, nfl, f0, out);
  }
};

template <typename T>
constexpr auto gb_bucket_dense = gb_block<T, GbDenseTable>;

// Dense variant, one WAVE per bucket (2^L <= 2^kGwMaxL files): each wave of
// the workgroup owns a private LDS slice [u16 grid of F x S counts | per-file
// state] and takes every (grid waves)-th bucket, so no workgroup barrier
// and no end-of-bucket row scan sits between two buckets: the wave clears
// its grid (ds_write_b128), adds each event with a RETURNING u16 add (the
// returned count + 1 is the pair's running count, so the concurrency
// maximum is tracked as it grows; counts of 1 need no atomic since every
// file with an event has concurrency >= 1), sums count / writes / reads /
// local per group of lanes of one file (ballots), and writes the bucket's
// (F, 6) int64 rows as one contiguous run.  LDS instructions of one wave run
// in order, so the clear, the adds and the reads need no barrier.
constexpr int kGwWaves = 4;   // waves per workgroup
constexpr int kGwUnroll = 8;  // payload loads in flight per lane

__host__ __device__ inline int gw_grid_words(int L, int sbits) {
  return ((((1 << (L + sbits)) + 1) >> 1) + 3) & ~3;  // u32 words, multiple of 4
}
__host__ __device__ inline int gw_wave_bytes(int L, int sbits) {
  return (4 * gw_grid_words(L, sbits) + 24 * (1 << L) + 15) & ~15;  // 16-byte aligned slices
}

template <typename T>
__global__ __launch_bounds__(64 * kGwWaves) void gb_bucket_wave(
    const T* __restrict__ pb, const unsigned* __restrict__ bbase, int64_t nbuckets, int64_t nf,
    GbPay p, const int32_t* __restrict__ primary, long long* __restrict__ out,
    int* __restrict__ big_list, int* __restrict__ big_count) {
  extern __shared__ unsigned long long lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int F = 1 << p.L;
  const int KW = gw_grid_words(p.L, p.sbits);
  unsigned char* mine =
      reinterpret_cast<unsigned char*>(lds) + (size_t)wv * gw_wave_bytes(p.L, p.sbits);
  unsigned* grid = reinterpret_cast<unsigned*>(mine);
  GbFiles g = gb_files(reinterpret_cast<unsigned long long*>(mine + 4 * KW), F);
  // buckets strided over the waves of the grid (a dynamic atomic counter
  // here miscompiled into a loop that never exits)
  const int64_t nw = (int64_t)gridDim.x * kGwWaves;
  for (int64_t b = (int64_t)blockIdx.x * kGwWaves + wv; b < nbuckets; b += nw) {
    const int b32 = (int)b;
    const int64_t s0 = bbase[b], n = (int64_t)bbase[b + 1] - s0;
    if (n > kGbDenseCap) {
      if (lane == 0) big_list[atomicAdd(big_count, 1)] = b32;
    } else {
      const int64_t f0 = b << p.L;
      const int nfl = (int)min((int64_t)F, nf - f0);
      // the first payloads go out before the clear
      T v[kGwUnroll];
  #pragma unroll
      for (int u = 0; u < kGwUnroll; ++u) {
        const int64_t i = u * 64 + lane;
        v[u] = i < n ? pb[s0 + i] : (T)0;
      }
      const uint4 z = {0u, 0u, 0u, 0u};
      for (int i = lane * 4; i < KW; i += 256) *reinterpret_cast<uint4*>(grid + i) = z;
      for (int f = lane; f < F; f += 64) {
        g.cw[f] = 0;
        g.rl[f] = 0;
        g.conc[f] = 0;
        g.prim[f] = f < nfl ? primary[f0 + f] : -2;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int64_t i0 = 0; i0 < n; i0 += 64 * kGwUnroll) {
        if (i0 > 0) {
  #pragma unroll
          for (int u = 0; u < kGwUnroll; ++u) {
            const int64_t i = i0 + u * 64 + lane;
            v[u] = i < n ? pb[s0 + i] : (T)0;
          }
        }
  #pragma unroll
        for (int u = 0; u < kGwUnroll; ++u) {
          const bool act = i0 + u * 64 + lane < n;
          if (__ballot(act) == 0) break;
          GbFields e = {0u, 0ull, 0u, 0u};
          bool loc = false;
          if (act) {
            e = gb_decode((unsigned long long)v[u], p);
            const unsigned key = (e.fl << p.sbits) | (unsigned)e.sc;
            const unsigned sh = (key & 1u) << 4;
            const unsigned old = atomicAdd(&grid[key >> 1], 1u << sh);
            const unsigned cnt = ((old >> sh) & 0xFFFFu) + 1u;
            if (cnt > 1u && cnt > g.conc[e.fl]) atomicMax(&g.conc[e.fl], cnt);
            loc = gb_local(gb_client(e.cc), g.prim[e.fl]);
          }
          gb_file_sums(g, act, e.fl, e.oc, loc, p.L);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // rows f0 .. f0 + nfl, six fields each: one contiguous run of the output
      long long* o = out + f0 * 6;
      for (int t = lane; t < 6 * nfl; t += 64) {
        const int f = t / 6, fld = t - 6 * f;
        const unsigned long long cw = g.cw[f], rl = g.rl[f];
        const long long cntf = (long long)(cw & 0xFFFFFFFFull);
        long long val;
        switch (fld) {
          case 0: val = cntf; break;
          case 1: val = (long long)(cw >> 32); break;
          case 2: val = (long long)(rl & 0xFFFFFFFFull); break;
          case 3: val = (long long)(rl >> 32); break;
          case 4: val = cntf; break;
          default: val = cntf > 0 ? (long long)max(g.conc[f], 1u) : 0; break;
        }
        o[t] = val;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// The same for buckets of at most 4 files (L <= 2, config 4's shape): the
// per-file count / writes / reads / local and the concurrency maximum are
// kept in each lane's registers (select by the event's file, no ballots and
// no per-file LDS atomics), a 4-byte payload is decoded with 32-bit field
// extracts (an 8-byte one from all its 64 bits: its client code takes up to
// 32), and the bucket's rows come from one wave reduction per value at
// the end.  The (file, second) counts stay in the wave's LDS grid.  The
// ballot kernel above spent ~165 instructions per 64 events here.
template <typename T>
__global__ __launch_bounds__(64 * kGwWaves) void gb_bucket_wave4(
    const T* __restrict__ pb, const unsigned* __restrict__ bbase, int64_t nbuckets, int64_t nf,
    GbPay p, const int32_t* __restrict__ primary, long long* __restrict__ out,
    int* __restrict__ big_list, int* __restrict__ big_count) {
  extern __shared__ unsigned long long lds[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int KW = gw_grid_words(p.L, p.sbits);
  unsigned* grid = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(lds) +
                                               (size_t)wv * gw_wave_bytes(p.L, p.sbits));
  const int F = 1 << p.L;
  const int sb = p.sbits;
  const int nw = gridDim.x * kGwWaves;
  for (int b = blockIdx.x * kGwWaves + wv; b < nbuckets; b += nw) {
    const int s0 = (int)bbase[b];
    const int n = (int)bbase[b + 1] - s0;
    if (n > kGbDenseCap) {
      if (lane == 0) big_list[atomicAdd(big_count, 1)] = b;
      continue;
    }
    const int64_t f0 = (int64_t)b << p.L;
    const int nfl = (int)min((int64_t)F, nf - f0);
    T v[kGwUnroll];
#pragma unroll
    for (int u = 0; u < kGwUnroll; ++u) {
      const int i = u * 64 + lane;
      v[u] = i < n ? pb[s0 + i] : (T)0;
    }
    const int pl = lane < nfl ? primary[f0 + lane] : -2;
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int i = lane * 4; i < KW; i += 256) *reinterpret_cast<uint4*>(grid + i) = z;
    // the bucket's primaries (client code = client + 1; -1: none)
    int pc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int q = __builtin_amdgcn_readlane(pl, f);
      // 8-byte payloads: client codes reach 2^31 (INT_MIN as an int), so the
      // codes compare as bit patterns and a primary below 0 takes code 0
      if constexpr (sizeof(T) == 4) pc[f] = q + 1;
      else pc[f] = q >= 0 ? (int)((unsigned)q + 1u) : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned A[4] = {0u, 0u, 0u, 0u}, B[4] = {0u, 0u, 0u, 0u}, M[4] = {0u, 0u, 0u, 0u};
    for (int i0 = 0; i0 < n; i0 += 64 * kGwUnroll) {
      if (i0 > 0) {
#pragma unroll
        for (int u = 0; u < kGwUnroll; ++u) {
          const int i = i0 + u * 64 + lane;
          v[u] = i < n ? pb[s0 + i] : (T)0;
        }
      }
#pragma unroll
      for (int u = 0; u < kGwUnroll; ++u) {
        if (i0 + u * 64 >= n) break;  // wave-uniform
        if (i0 + u * 64 + lane < n) {
          const unsigned long long x = (unsigned long long)v[u];
          const unsigned lo = (unsigned)x;  // op, client and (4-byte payloads) all fields
          const unsigned fl = (unsigned)(x >> p.fshift) & (unsigned)(F - 1);
          const unsigned sc = (unsigned)(x >> p.sshift) & ((1u << sb) - 1u);
          unsigned oc;
          int cc;
          if constexpr (sizeof(T) == 4) {  // 2 + cbits <= 32: both fields lie in lo
            oc = __builtin_amdgcn_ubfe(lo, p.cbits, 2);
            cc = (int)__builtin_amdgcn_ubfe(lo, 0, p.cbits);
          } else {  // cbits up to 32: the op, or both fields, may lie past lo
            oc = (unsigned)(x >> p.cbits) & 3u;
            cc = (int)(unsigned)(x & ((1ull << p.cbits) - 1));
          }
          const unsigned key = (fl << sb) | sc;
          const unsigned sh = (key & 1u) << 4;
          const unsigned old = atomicAdd(&grid[key >> 1], 1u << sh);
          const unsigned cnt = __builtin_amdgcn_ubfe(old, sh, 16) + 1u;
          const int pf = fl == 0 ? pc[0] : fl == 1 ? pc[1] : fl == 2 ? pc[2] : pc[3];
          unsigned loc;
          if constexpr (sizeof(T) == 4) loc = (cc != 0 && pf > 0 && cc == pf) ? 1u : 0u;
          else loc = (cc != 0 && cc == pf) ? 1u : 0u;
          const unsigned va = 1u | ((oc == 1u) ? 0x10000u : 0u);
          const unsigned vb = ((oc == 2u) ? 1u : 0u) | (loc << 16);
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            const bool m = fl == (unsigned)f;
            A[f] += m ? va : 0u;
            B[f] += m ? vb : 0u;
            M[f] = max(M[f], m ? cnt : 0u);
          }
        }
      }
    }
    // wave sums / maxima of the lanes' per-file values by halving exchanges:
    // at each xor step a lane keeps half of its values and adds the
    // partner's copy of that half (sums: A0..3 B0..3 over xor 32, 16, 8 ->
    // lane bits 5..3 name the value, then xor 4, 2, 1; maxima: M0..3 over
    // xor 32, 16 -> lane bits 5..4, then xor 8..1): 17 exchanges instead of
    // 72 (3 values x 4 files x 6 levels)
    const int h5 = (lane >> 5) & 1, h4 = (lane >> 4) & 1, h3 = (lane >> 3) & 1;
    unsigned s4[4], s2[2], s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned send = h5 ? A[i] : B[i];
      s4[i] = (h5 ? B[i] : A[i]) + (unsigned)__shfl_xor((int)send, 32);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned send = h4 ? s4[i] : s4[2 + i];
      s2[i] = (h4 ? s4[2 + i] : s4[i]) + (unsigned)__shfl_xor((int)send, 16);
    }
    {
      const unsigned send = h3 ? s2[0] : s2[1];
      s1 = (h3 ? s2[1] : s2[0]) + (unsigned)__shfl_xor((int)send, 8);
    }
    for (int o = 4; o > 0; o >>= 1) s1 += (unsigned)__shfl_xor((int)s1, o);
    unsigned m2[2], m1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned send = h5 ? M[i] : M[2 + i];
      m2[i] = max(h5 ? M[2 + i] : M[i], (unsigned)__shfl_xor((int)send, 32));
    }
    {
      const unsigned send = h4 ? m2[0] : m2[1];
      m1 = max(h4 ? m2[1] : m2[0], (unsigned)__shfl_xor((int)send, 16));
    }
    for (int o = 8; o > 0; o >>= 1) m1 = max(m1, (unsigned)__shfl_xor((int)m1, o));
    // lane 8 f holds A[f], lane 32 + 8 f B[f], lane 16 f M[f]
    const int fo = lane / 6;
    const unsigned a_f = (unsigned)__shfl((int)s1, (8 * fo) & 63);
    const unsigned b_f = (unsigned)__shfl((int)s1, (32 + 8 * fo) & 63);
    const unsigned m_f = (unsigned)__shfl((int)m1, (16 * fo) & 63);
    // rows f0 .. f0 + nfl, six fields each: one contiguous run of the output
    long long* o = out + f0 * 6;
    if (lane < 6 * nfl) {
      const int f = fo, fld = lane - 6 * f;
      const unsigned a = a_f;
      const unsigned bb = b_f;
      const unsigned mm = m_f;
      long long val;
      switch (fld) {
        case 0: val = a & 0xFFFFu; break;
        case 1: val = a >> 16; break;
        case 2: val = bb & 0xFFFFu; break;
        case 3: val = bb >> 16; break;
        case 4: val = a & 0xFFFFu; break;
        default: val = mm; break;
      }
      o[lane] = val;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// Buckets over the LDS capacity: the hash lives in global memory (2 n slots
// from gslots + 2 * s0, so buckets never overlap).
template <typename T>
__global__ __launch_bounds__(kGbBThreads) void gb_bucket_big(
    const T* __restrict__ pb, const unsigned* __restrict__ bbase, const int* __restrict__ list,
    int64_t nf, GbPay p, GbKey k, const int32_t* __restrict__ primary,
    unsigned long long* __restrict__ gslots, long long* __restrict__ out) {
  extern __shared__ unsigned long long lds[];
  const int64_t b = list[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t s0 = bbase[b], n = (int64_t)bbase[b + 1] - s0;
  const int F = 1 << p.L;
  const int64_t f0 = b << p.L;
  const int nfl = (int)min((int64_t)F, nf - f0);
  unsigned long long* slots = gslots + 2 * s0;
  const unsigned size = (unsigned)(2 * n);
  GbFiles g = gb_files(lds, F);
  for (unsigned i = tid; i < size; i += kGbBThreads) slots[i] = kEmpty;
  for (int f = tid; f < nfl; f += kGbBThreads) {
    g.cw[f] = 0;
    g.rl[f] = 0;
    g.conc[f] = 0;
    g.prim[f] = primary[f0 + f];
  }
  __syncthreads();
  for (int64_t i0 = 0; i0 < n; i0 += kGbBThreads) {
    const int64_t i = i0 + tid;
    const bool act = i < n;
    gb_event<false>(act, act ? (unsigned long long)pb[s0 + i] : 0ull, p, k, slots, size, false,
                    g);
  }
  __syncthreads();
  gb_write_files(g, nfl, f0, out);
}

// Persistent grids: exactly the workgroups that stay resident together (a
// second round of late workgroups would double the tail), at most `work`.
template <typename K>
int64_t gb_persistent_grid(Ctx& c, K kernel, int threads, size_t lds, int64_t work) {
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(kernel), threads, lds));
  return std::min<int64_t>(work, (int64_t)lloyd_num_cus(c.device) * std::max(1, per_cu));
}

template <typename T>
int gb_buckets_t(Ctx& c, const T* pb, const unsigned* bbase, int64_t nb, int64_t nf,
                 const GbLayout& lay, int64_t nvalid, int64_t* grid) {
  const GbPay& p = lay.p;
  const int L = p.L;
  int* big = gb_big_count(c);  // (the list itself: c.gb_list)
  HIP_CHECK(hipMemsetAsync(big, 0, 4, c.stream));
  c.gb_list.ensure(sizeof(int) * (size_t)std::max<int64_t>(nb, 1));
  const size_t files_lds = (size_t)24 << L;
  const int32_t* primary = c.ev_primary.as<int32_t>();
  long long* out = c.ev_out.as<long long>();
  if (lay.dense) {
    // the three dense kernels take the same arguments
    const bool wave = L <= kGwMaxL && !getenv("CDR_GB_BLOCK");
    auto kernel = wave ? gb_bucket_wave<T> : gb_bucket_dense<T>;
    const int threads = wave ? 64 * kGwWaves : kGbBThreads;
    const size_t lds = wave ? (size_t)kGwWaves * gw_wave_bytes(L, p.sbits)
                            : files_lds + ((size_t)4 << std::max(0, L + p.sbits - 1)) + 16;
    *grid = gb_persistent_grid(c, kernel, threads, lds,
                               wave ? ceil_div(nb, (int64_t)kGwWaves) : nb);
    // (the register kernel runs on the ballot kernel's grid)
    if (wave && L <= 2 && !getenv("CDR_GB_BALLOT")) kernel = gb_bucket_wave4<T>;
    hipLaunchKernelGGL(kernel, dim3(*grid), dim3(threads), lds, c.stream, pb, bbase, nb, nf, p,
                       primary, out, c.gb_list.as<int>(), big);
  } else {
    const size_t lds = 8 * kGbSlots + files_lds;
    *grid = gb_persistent_grid(c, gb_bucket<T>, kGbBThreads, lds, nb);
    hipLaunchKernelGGL(gb_bucket<T>, dim3(*grid), dim3(kGbBThreads), lds, c.stream, pb, bbase, nb,
                       nf, p, primary, out, c.gb_list.as<int>(), big, gb_key(p));
  }
  HIP_CHECK(hipGetLastError());
  prof_mark(c, 2);
  int nbig = 0;
  HIP_CHECK(hipMemcpyAsync(&nbig, big, 4, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
  if (nbig > 0) {
    c.gb_slots.ensure(sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(nvalid, 1));
    hipLaunchKernelGGL(gb_bucket_big<T>, dim3(nbig), dim3(kGbBThreads), files_lds, c.stream, pb,
                       bbase, c.gb_list.as<int>(), nf, p, gb_key(p), primary,
                       c.gb_slots.as<unsigned long long>(), out);
    HIP_CHECK(hipGetLastError());
    prof_mark(c, 2);
  }
  return nbig;
}

}  // namespace

int gb_buckets(Ctx& c, const void* pay, const unsigned* bbase, int64_t nb, int64_t nf,
               const GbLayout& lay, int64_t nvalid, int64_t* grid) {
  return lay.pbytes == 4
             ? gb_buckets_t(c, static_cast<const unsigned*>(pay), bbase, nb, nf, lay, nvalid, grid)
             : gb_buckets_t(c, static_cast<const unsigned long long*>(pay), bbase, nb, nf, lay,
                            nvalid, grid);
}

}  // namespace cdr
