// screen32b.hip — the bounded DELTA screen with 4-byte bound words (device
// loop; d <= 16, k <= 64: configs 2, 3): screen32b (LDS queue and fused fixup,
// CDR_S32B_SPLIT=0), screen32bz (the word stream of the two-launch form,
// CDR_S32BS_SPLIT=1, whose lists screen32bs.hip decides), and the kernels
// that reset and rebase the bound words of either width and build the 2-byte
// words' watch list (zh_watch_kernel).
//
// screen32p still reads every point's 32-byte hi copy every step.  After the
// first steps almost every point keeps its label by a wide margin and the
// centroids move little, so a point's distances can be bounded across steps
// instead of recomputed (Hamerly's bounds, SURVEY.md §7 hard parts (c): exact,
// the same labels, less work).  With t_j(s) = ||xhat - chat_j(s)|| (the
// reference's distance up to 2^sigma) and the centroid drifts
// delta_j(s) >= ||chat_j(s) - chat_j(s - 1)||, M(s) = max_j delta_j(s):
//   t_a(t) <= t_a(t0) + sum_{t0 < s <= t} delta_a(s),
//   min_{j != a} t_j(t) >= min_{j != a} t_j(t0) - sum_{t0 < s <= t} M(s).
// ll_finalize32 keeps the cumulative W_j(t) = sum_{s <= t} (M(s) + delta_j(s))
// as exact int64 multiples of 2^-40 (every increment rounded up) and hands
// this step W_j rounded up and down to fp32 (wup / wdn).  A point whose label
// a was decided at step t0 with rigorous bounds u0 >= t_a(t0) and
// l0 <= min_{j != a} t_j(t0) stores ONE word
//   Z = l0 (1 - 2^-20) - u0 + wdn_a(t0)     (rounded down; low 6 bits: a)
// and keeps a at step t when Z > wup_a(t): then
//   min_{j != a} t_j(t) > t_a(t) + 2^-20 l0 > t_a(t) (1 + 2^-22),
// far above the reference's fp64 rounding (< 2^-45), so np.argmin of the
// reference's norms is a (src/kmeans_plusplus.py:33-34) and the point's
// coordinates are not read at all.
//
// Per wave: phase 1 streams the bound words (4 per lane, 1 KiB per load, four
// chunks in flight) and lists the points that fail in LDS; phase 2 gathers
// those points' hi rows (AoS copy XH, one line per point) 64 at a time, one
// batch ahead, and decides them exactly as screen32p does (triangle test
// against c32_a, else the hi-only k-way screen and its certificate, else
// the exact fallback of the fused fixup), writing the point's new word:
//   triangle kept:  u0 = ub_a, l0 = h_a (1 - 2^-22) - ub_a;
//   k-way certified (label b, keys vb <= vs):
//     u0 = sqrt(vb (1 + 2^-16) + thr0 + ||h||^2_up - D_lo) (1 + 2^-19) + dn,
//     l0 = sqrt(vs - thr0 - D_hi + ||h||^2_lo) (1 - 2^-19) - dn
//     (|S_j - exact| <= E < thr0 / 2: thr0 also covers the fp32 rounding of
//     these sums; every other key is >= vs);
//   uncertified: "no bound" (kZbStale | old label; the fixup rewrites the
//     label if the exact decision moves the point).
// Moves and fallbacks go to the same per-wave lists as screen32p's, and the
// fused fixup finishes the step, so labels and int64 running sums are those
// of the full screen.
// ---------------------------------------------------------------------------
#include "screen32_common.h"
#include "screen32_fix.h"

namespace cdr {

template <int Q, int MT>
__global__ __launch_bounds__(256, 4) void screen32b(S32BArgs B) {
  const S32PArgs& a = B.p;
  constexpr int QH = FixDims<Q>::QH;
  if (a.gate && a.gate[0] == 0) return;
  constexpr bool H1 = QH == 1;
  constexpr int kTile = H1 ? 512 : 1024;  // bytes per 32-point tile of the queue
  constexpr int kHalf = kTile / 2;
  constexpr int kPB = H1 ? 8 : 16;        // bytes per (point, half)
  constexpr int NWH = kPB / 4;            // dwords per point half
  constexpr int kRow = 2 * kPB;           // bytes per point in XH
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float c32s[64 * kPrStr + 128];
  float* const eb = c32s + 64 * kPrStr;  // E_j
  float* const hc = eb + 64;             // h_j
  // per wave: the k-way queue (screen32p's ring) and, after the last drain,
  // the fused fixup's table (FixLds)
  constexpr size_t kQBytes = 4 * 2 * 2 * kTile + 4 * 128 * sizeof(int2);
  __shared__ __attribute__((aligned(16))) unsigned char qlds[kQBytes > kFixLdsBytes ? kQBytes : kFixLdsBytes];
  typedef unsigned char QRow[2][2 * kTile];
  QRow* qd = reinterpret_cast<QRow*>(qlds);
  int2 (*qm)[128] = reinterpret_cast<int2 (*)[128]>(qlds + 4 * 2 * 2 * kTile);
  // per wave: points whose bound failed, (chunk iteration << 14 | offset << 6 | label)
  __shared__ unsigned flist[4][kBList];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = t >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  const int nwaves = gridDim.x * 4;
  const int64_t nchunks = B.nchunks;

  // ---- phase 1 loads: the first chunks overlap the prologue ----
  // Ordinary loads (the compiler's s_waitcnt counts them): every iteration
  // issues exactly one, a chunk past the end reloads the last one, so the
  // counts are the same on every path and kBPD - 1 chunks stay in flight.
  auto zload = [&](u4v& z, int64_t ci) __attribute__((always_inline)) {
    const int64_t cc = ci < nchunks ? ci : nchunks - 1;  // past the end: reload the last
    z = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(B.zb + cc * kBChunk) + lane);
  };
  u4v zc[kBPD];
#pragma unroll
  for (int i = 0; i < kBPD - 1; ++i) zload(zc[i], wave + (int64_t)i * nwaves);

  // ---- the plan (screen32p's staging, one round trip) ----
  __shared__ h8 sA[MT * 2 * 64];
  __shared__ __attribute__((aligned(16))) float sC[MT * 4 * 2 * 4];
  constexpr int kPr4 = (64 * kPrStr + 128) / 4;
  static_assert(kPr4 <= 512 && MT * 2 * 64 <= 256, "prologue: two float4 per thread");
  const f4* prune4 = reinterpret_cast<const f4*>(a.prune);
  const f4 pv0 = prune4[t];
  const f4 pv1 = t + 256 < kPr4 ? prune4[t + 256] : f4{0.f, 0.f, 0.f, 0.f};
  h8 av = {};
  if (t < MT * 2 * 64) av = a.frag[t];
  float cv = 0.0f;
  const int cm = t >> 5, ci4 = (t >> 3) & 3, chh = (t >> 2) & 1, cc = t & 3;
  if (t < MT * 32) cv = a.cinit[(cm * 16 + ci4 * 4 + cc) * 64 + chh * 32];
  const float wup_l = B.wup[lane], wdn_l = B.wdn[lane];  // lane j: W_j (k <= 64)
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0, thr_rel = a.thr_rel;
  const float Dv = a.thr_dev ? a.thr_dev[1] : a.Dv;
  const float Dlo = Dv * (1.0f - 0x1p-19f), Dhi = Dv * (1.0f + 0x1p-19f);  // D_lo < D < D_hi
  reinterpret_cast<f4*>(c32s)[t] = pv0;
  if (t + 256 < kPr4) reinterpret_cast<f4*>(c32s)[t + 256] = pv1;
  if (t < MT * 2 * 64) sA[t] = av;
  if (t < MT * 32) sC[t] = cv;
  __syncthreads();

  int2* fb_region = a.fb_list + (size_t)wave * a.cap;
  int2* mv_region = a.mv_list + (size_t)wave * a.cap;
  int fb_used = 0, mv_used = 0;
  struct Row {
    unsigned w[2 * NWH];  // the point's hi row: half 0 then half 1 (packed fp16 pairs)
  };
  // q = ||h - c32_j||^2 (screen32p's dist2)
  auto dist2 = [&](const Row& b, int j) __attribute__((always_inline)) -> float {
    const f4* c4 = reinterpret_cast<const f4*>(c32s + j * kPrStr);
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < NWH; ++q) {
      const f4 cq = c4[q];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = 2 * q + u;
        const f2 df = {mix_sub_lo(b.w[i], cq[2 * u]), mix_sub_hi(b.w[i], cq[2 * u + 1])};
        acc = __builtin_elementwise_fma(df, df, acc);
      }
    }
    return acc.x + acc.y;
  };
  // (best, runner-up) keys of one 32-point tile of queued points (screen32p's tile)
  auto tile = [&](const u4v& v, unsigned& bk, unsigned& sk, float& hp) __attribute__((always_inline)) {
    const h8 BH = __builtin_bit_cast(h8, v);
    hp = 0.0f;
#pragma unroll
    for (int i = 0; i < (H1 ? 4 : 8); i += 2)
      hp = __builtin_amdgcn_fdot2(h2{BH[i], BH[i + 1]}, h2{BH[i], BH[i + 1]}, hp, false);
    unsigned b = 0xFFFFFFFFu, s = 0xFFFFFFFFu;
#pragma nounroll
    for (int m = 0; m < MT; ++m) {
      h8 A0 = sA[(m * 2 + 0) * 64 + lane];
      const h8 A1 = sA[(m * 2 + 1) * 64 + lane];
      if constexpr (H1)
#pragma unroll
        for (int i = 0; i < 4; ++i) A0[4 + i] = A1[i];
      f16v acc;
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const f4 c4v = *reinterpret_cast<const f4*>(sC + ((m * 4 + i4) * 2 + (lane >> 5)) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * i4 + i] = c4v[i];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, BH, acc, 0, 0, 0);
      if constexpr (!H1) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, BH, acc, 0, 0, 0);
      const unsigned rb = 32u * (unsigned)m;
      auto key = [&](int i) {
        return (__float_as_uint(acc[i]) & ~63u) | (rb + (unsigned)(8 * (i >> 2) + (i & 3)));
      };
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        const unsigned x = key(q), y = key(q + 1);
        unsigned tq;
        asm("v_med3_u32 %0, %1, %2, %3" : "=v"(tq) : "v"(b), "v"(x), "v"(y));
        asm("v_min3_u32 %0, %1, %2, %3" : "=v"(b) : "v"(b), "v"(x), "v"(y));
        s = min(s, tq);
      }
    }
    bk = b | ((unsigned)(lane >> 5) << 2);
    sk = s | ((unsigned)(lane >> 5) << 2);
  };
  // the k-way screen of queue block qb (nvalid entries), its lists and bound words
  auto drain = [&](int qb, int nvalid) __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's queue writes
    const unsigned char* src = qd[wv][qb];
    u4v v[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      if constexpr (H1) {
        const uint2 x = *reinterpret_cast<const uint2*>(src + tt * kTile + lane * kPB);
        v[tt] = u4v{x.x, x.y, x.x, x.y};
      } else {
        v[tt] = *reinterpret_cast<const u4v*>(src + tt * kTile + lane * kPB);
      }
    }
    const int2 meta = qm[wv][qb * 64 + lane];  // lane l owns entry l after the swap
    unsigned bA = 0, sA_ = 0, bB = 0, sB = 0;
    float hA = 0.0f, hB = 0.0f;
#pragma nounroll
    for (int tt = 0; tt < 2; ++tt) {
      unsigned bk, sk;
      float hp;
      tile(tt == 0 ? v[0] : v[1], bk, sk, hp);
      if (tt == 0) {
        bA = bk;
        sA_ = sk;
        hA = hp;
      } else {
        bB = bk;
        sB = sk;
        hB = hp;
      }
    }
    swap32(bA, bB);
    swap32(sA_, sB);
    merge_top2(bA, sA_, bB, sB);
    const int label = (int)(bA & 63u);
    const float vb = __uint_as_float(bA & ~63u);
    const float vs = __uint_as_float(sA_ & ~63u);
    float thr = fmaf(vb, thr_rel, thr0);
    unsigned ua = __float_as_uint(hA), ub = __float_as_uint(hB);
    swap32(ua, ub);
    const float hsum = __uint_as_float(ua) + __uint_as_float(ub);
    const float hh = fmaf(hsum, 1.0f + 0x1p-18f, 0x1p-20f);  // >= ||h||^2
    const float hl = hsum * (1.0f - 0x1p-18f);               // <= ||h||^2
    const float dn = fmaf(0x1p-11f * (1.0f + 0x1p-9f), __builtin_amdgcn_sqrtf(hh), 0x1p-23f);
    {  // the hi-only certificate (screen32_fix.h)
      const float K = thr0 + hh - Dlo;
      const float Gs = fmaxf(vs + K, 0x1p-100f), Gb = fmaxf(fmaf(vb, thr_rel, K), 0x1p-100f);
      thr += 2.0f * (1.0f + 0x1p-19f) * dn * (__builtin_amdgcn_sqrtf(Gs) + __builtin_amdgcn_sqrtf(Gb));
    }
    const bool valid = lane < nvalid;
    const bool cert = vs > thr;  // NaN: never certified
    const int pt = meta.x, ob = meta.y;
    const bool moved = valid && cert && label != ob;
    if (moved) {
      a.labels[pt] = label;
      a.lab8[pt] = (uint8_t)label;
    }
    // the point's bound word: from its best and runner-up keys, or "no bound"
    const float gb = fmaf(vb, thr_rel, thr0 + hh - Dlo);
    const float gs = vs - ((thr0 + Dhi) - hl);
    const float u0 = fmaf(__builtin_amdgcn_sqrtf(fmaxf(gb, 0.0f)), 1.0f + 0x1p-19f, dn);
    const float l0 = fmaf(__builtin_amdgcn_sqrtf(fmaxf(gs, 0.0f)), 1.0f - 0x1p-19f, -dn);
    const float wl = __shfl(wdn_l, label);
    if (valid) B.zb[pt] = cert ? zb_pack(l0, u0, wl, (unsigned)label) : (kZbStale | (unsigned)ob);
    const bool unc = valid && !cert;
    const unsigned long long mv = __ballot(moved);
    const unsigned long long need = __ballot(unc);
    const int rm = __builtin_amdgcn_mbcnt_hi((unsigned)(mv >> 32),
                                             __builtin_amdgcn_mbcnt_lo((unsigned)mv, 0u));
    const int rn = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                             __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
    if (moved) mv_region[mv_used + rm] = int2{pt, ob | (label << 16)};
    if (unc) fb_region[fb_used + rn] = int2{pt, ob};
    mv_used += __popcll(mv);
    fb_used += __popcll(need);
  };
  int qh = 0, qn = 0;  // k-way queue head (next slot, mod 128) and length: wave-uniform
  int qtot = 0, ttot = 0;
  // one gathered point per lane: the triangle test, else the k-way queue
  auto process = [&](const Row& b, bool valid, int pt, int ao) __attribute__((always_inline)) {
    const float qa = dist2(b, ao);
    const float uba = fmaf(__builtin_amdgcn_sqrtf(qa), 1.0f + 0x1p-18f, eb[ao]);
    const float l0 = fmaf(hc[ao], 1.0f - 0x1p-22f, -uba);
    const bool keep = l0 > uba * (1.0f + 0x1p-20f);
    if (valid && keep) B.zb[pt] = zb_pack(l0, uba, __shfl(wdn_l, ao), (unsigned)ao);
#ifdef CDR_EXPERIMENTS
    const bool q = valid && !keep && !(B.dbg & 8);  // (timing: no k-way screen)
#else
    const bool q = valid && !keep;
#endif
    const unsigned long long m = __ballot(q);
    if (m) {
      if (q) {
        const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        const int slot = (qh + r) & 127;
        const int e = slot & 63;
        unsigned char* dst = qd[wv][slot >> 6] + (e >> 5) * kTile + (e & 31) * kPB;
        if constexpr (H1) {
          *reinterpret_cast<uint2*>(dst) = uint2{b.w[0], b.w[1]};
          *reinterpret_cast<uint2*>(dst + kHalf) = uint2{b.w[2], b.w[3]};
        } else {
          *reinterpret_cast<uint4*>(dst) = uint4{b.w[0], b.w[1], b.w[2], b.w[3]};
          *reinterpret_cast<uint4*>(dst + kHalf) = uint4{b.w[4], b.w[5], b.w[6], b.w[7]};
        }
        qm[wv][slot] = int2{pt, ao};
      }
      const int c = __popcll(m);
      qh = (qh + c) & 127;
      qn += c;
      qtot += c;
      if (qn >= 64) {
        drain(((qh - qn) & 127) >> 6, 64);
        qn -= 64;
      }
    }
  };
  // ---- phase 2: the listed points, 64 per batch, the next batch's rows in flight ----
  // The gathers are ordinary loads too: a load issued from inline asm leaves
  // a register the allocator may copy (at a join, around a call-sized block)
  // before the data lands, which the compiler's own counts never do.
  unsigned* const fl = flist[wv];
  struct GB {
    Row r;
    int pt, ao;
    bool valid;
  };
  auto gload = [&](GB& g, int b, int cnt) __attribute__((always_inline)) {
    const int e = 64 * b + lane;
    g.valid = e < cnt;
    const unsigned ent = fl[g.valid ? e : 64 * b];  // (entry 64 b exists)
    const int64_t ci = wave + (int64_t)(ent >> 14) * nwaves;
    const int64_t pt = ci * kBChunk + ((ent >> 6) & 255);
    g.pt = (int)pt;
    g.ao = (int)(ent & 63);
    const u4v* src = reinterpret_cast<const u4v*>(B.XH + pt * kRow);
    const u4v q0 = __builtin_nontemporal_load(src);
    g.r.w[0] = q0.x; g.r.w[1] = q0.y; g.r.w[2] = q0.z; g.r.w[3] = q0.w;
    if constexpr (!H1) {
      const u4v q1 = __builtin_nontemporal_load(src + 1);
      g.r.w[4] = q1.x; g.r.w[5] = q1.y; g.r.w[6] = q1.z; g.r.w[7] = q1.w;
    }
  };
  // every full batch of the list (all of it when `last`); a partial batch
  // stays at the front for the next call
  auto phase2 = [&](int& cnt, bool last) __attribute__((always_inline)) {
    const int nb = last ? (cnt + 63) >> 6 : cnt >> 6;
    if (nb == 0) return;
    ttot += last ? cnt : nb * 64;
#ifdef CDR_EXPERIMENTS
    if (B.dbg & 4) {  // timing experiments only: the listed points are not decided
      cnt = 0;
      return;
    }
#endif
    // three batches in flight: every slot is reloaded unconditionally (past
    // the end: the last batch again, not processed), so the compiler's
    // counts let the two later batches stay in flight while one is decided
    GB g[3];
    gload(g[0], 0, cnt);
    gload(g[1], nb > 1 ? 1 : 0, cnt);
    for (int b = 0; b < nb; b += 3) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int nx = b + i + 2;
        gload(g[(i + 2) % 3], nx < nb ? nx : nb - 1, cnt);
        if (b + i < nb) process(g[i].r, g[i].valid, g[i].pt, g[i].ao);
      }
    }
    const int done = nb * 64;
    const int rem = last ? 0 : cnt - done;
    if (rem > 0) {
      const unsigned v = lane < rem ? fl[done + lane] : 0u;
      __builtin_amdgcn_wave_barrier();
      if (lane < rem) fl[lane] = v;
    }
    cnt = rem;
  };

  // ---- phase 1: the bound words, 4 points per lane per chunk ----
  int cnt = 0;  // listed points (wave-uniform)
  int64_t it = 0;
  for (int64_t C0 = wave; C0 < nchunks; C0 += (int64_t)kBPD * nwaves) {
#pragma unroll
    for (int i = 0; i < kBPD; ++i, ++it) {
      const int64_t Ci = C0 + (int64_t)i * nwaves;
      if (Ci >= nchunks) break;
      zload(zc[(i + kBPD - 1) % kBPD], Ci + (int64_t)(kBPD - 1) * nwaves);
      const u4v z = zc[i];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned w = z[u];
        const unsigned lab = w & 63u;
#ifdef CDR_EXPERIMENTS
        const bool fail = (!(__uint_as_float(w & ~63u) > __shfl(wup_l, (int)lab)) || (B.dbg & 1)) &&
                          !(B.dbg & 16);  // (timing: the stream alone)
#else
        const bool fail = !(__uint_as_float(w & ~63u) > __shfl(wup_l, (int)lab)) || (B.dbg & 1);
#endif
        const unsigned long long m = __ballot(fail);
        if (m) {
          if (fail) {
            const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            fl[cnt + r] = (unsigned)it << 14 | (unsigned)(4 * lane + u) << 6 | lab;
          }
          cnt += __popcll(m);
        }
      }
      if (cnt > kBList - kBChunk) phase2(cnt, false);
    }
  }
  phase2(cnt, true);
  if (qn > 0) drain(((qh - qn) & 127) >> 6, qn);  // the partial queue block
  if (lane == 0) {
    a.fb_count[wave] = fb_used;
    a.mv_count[wave] = mv_used;
    if (a.q_acc) a.q_acc[wave] += qtot;
    if (B.t_acc) B.t_acc[wave] += ttot;
  }
#ifdef CDR_EXPERIMENTS
  if (B.dbg & 2) return;  // (timing: no fused fixup)
#endif
  if (!a.fuse) return;
  __syncthreads();  // every queue drained (its LDS becomes the table); lists written
  const FixLds L(qlds);
  if (lane == 0) {
    L.s_mv[wv + 1] = mv_used;
    L.s_fb[wv + 1] = fb_used;
  }
  fixup_regions<Q, MT>(a.fx, blockIdx.x * 4, 4, blockIdx.x % kRunSlices, L, FixPlan{sA, sC});
}

// ---------------------------------------------------------------------------
// screen32bz: phase 1 of the bounded screen as its own launch (the split form,
// CDR_S32BS_SPLIT=1; the fused kernel is the default).  Streams every
// point's bound word (4 per lane per 1 KiB chunk, KPD chunks in flight per
// wave) and lists the points whose bound fails in the
// wave's region of B.zl, in screen32bs's entry format (chunk iteration << 14 |
// offset << 6 | label); screen32bs<Q, MT, true> then decides the lists with
// every wave of the chip on the gathers and the MFMA screen.  In the fused
// form a wave stops streaming while it decides a batch, so the stream and the
// decisions add up; split, the stream is a plain HBM-bound pass (no plan, no
// LDS beyond the list staging, low register count) and the decisions run at
// full occupancy.  Entries are staged in LDS and written 64 at a time (one
// 256-byte store), so stores rarely sit between a chunk load and its use.
// ---------------------------------------------------------------------------
template <int KPD>
__global__ __launch_bounds__(256) void screen32bz(S32BArgs B) {
  const S32PArgs& a = B.p;
  if (a.gate && a.gate[0] == 0) return;
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  constexpr int kZList = KPD * kBChunk + 64;
  __shared__ unsigned flist[4][kZList];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = t >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  const int64_t nchunks = B.nchunks;
  int64_t wbase, wend;
  int wstride;
  bs_range(B, wv, wbase, wstride, wend);
  auto zload = [&](u4v& z, int64_t ci) __attribute__((always_inline)) {
    const int64_t cc = ci < nchunks ? ci : nchunks - 1;
    z = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(B.zb + cc * kBChunk) + lane);
  };
  u4v zc[KPD];
#pragma unroll
  for (int i = 0; i < KPD - 1; ++i) zload(zc[i], wbase + (int64_t)i * wstride);
  const float wup_l = B.wup[lane];  // lane j: W_j rounded up (k <= 64)
  unsigned* const fl = flist[wv];
  uint32_t* const out = B.zl + (size_t)wave * B.zcap;
  int cnt = 0, total = 0;
  int it = 0;
  for (int64_t C0 = wbase; C0 < wend; C0 += (int64_t)KPD * wstride) {
#pragma unroll
    for (int i = 0; i < KPD; ++i, ++it) {
      const int64_t Ci = C0 + (int64_t)i * wstride;
      if (Ci >= wend) break;
      zload(zc[(i + KPD - 1) % KPD], Ci + (int64_t)(KPD - 1) * wstride);
      const u4v z = zc[i];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned w = z[u];
        const unsigned lab = w & 63u;
        const bool fail = !(__uint_as_float(w & ~63u) > __shfl(wup_l, (int)lab)) || (B.dbg & 1);
        const unsigned long long m = __ballot(fail);
        if (m) {
          if (fail) {
            const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            fl[cnt + r] = (unsigned)it << 14 | (unsigned)(4 * lane + u) << 6 | lab;
          }
          cnt += __popcll(m);
        }
      }
    }
    if (cnt >= 64) {  // whole 64-entry rows out, the rest to the front
      const int full = cnt & ~63;
      __builtin_amdgcn_wave_barrier();
      for (int o = 0; o < full; o += 64) out[total + o + lane] = fl[o + lane];
      const int rem = cnt - full;
      const unsigned v = lane < rem ? fl[full + lane] : 0u;
      __builtin_amdgcn_wave_barrier();
      if (lane < rem) fl[lane] = v;
      total += full;
      cnt = rem;
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < cnt) out[total + lane] = fl[lane];
  if (lane == 0) B.zn[wave] = total + cnt;
}

// Bound words before the first bounded step of a run of them: every real
// point "no bound" with its current label (lab8), padding rows "always keep".
__global__ void zb_reset_kernel(const uint8_t* __restrict__ lab8, uint32_t* __restrict__ zb,
                                int64_t n, int64_t n_pad, const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += (int64_t)gridDim.x * blockDim.x)
    zb[i] = i < n ? (kZbStale | lab8[i]) : 0x7F000000u;  // (2^127: above any W)
}

// 2-byte words before the first bounded step: every real point "no bound"
// (code 0) with its current label, padding rows "always keep" (code 1023).
__global__ void zh_reset_kernel(const uint8_t* __restrict__ lab8, uint16_t* __restrict__ zh,
                                int64_t n, int64_t n_pad, const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += (int64_t)gridDim.x * blockDim.x)
    zh[i] = i < n ? (uint16_t)lab8[i] : (uint16_t)kZ16Pad;
}

// A kept word carried to a new base (G_a grows by dg >= the exact step) and
// exponent: dec(code) - dg rounded down, then truncated; codes 0 and 1023 stay
__device__ __forceinline__ unsigned zb16_rebase(unsigned w, float dg, int e0o, int e0n) {
  const unsigned c = w >> 6;
  if (c == 0u || c == 1023u) return w;
  const float t = zb16_dec((int)c, e0o) - dg;  // |error| <= 2^-24 |t|
  int cn = t > 0.0f ? zb16_code(t * (1.0f - 0x1p-22f), e0n) : -1;
  cn = cn < 0 ? 0 : (cn > 1022 ? 1022 : cn);
  return (unsigned)cn << 6 | (w & 63u);
}

// A rebase of the 2-byte words (plan32.h; decided by ll_finalize32, run
// before the next screen at the steps the host allows, gated on the device):
// every kept word to the new base and exponent, 8 words per thread
// (dec(code) - dG rounded down, truncated; codes 0 and 1023 stay).
__global__ __launch_bounds__(256) void zh_rebase_kernel(uint16_t* __restrict__ zh, int64_t n_pad,
                                                        const unsigned char* __restrict__ bt,
                                                        const long long* __restrict__ gate) {
  if (gate && gate[0] == 0) return;
  const int* hd = reinterpret_cast<const int*>(bt + kBndHdr);
  if (hd[3] == 0) return;
  __shared__ float dgs[64];
  if (threadIdx.x < 64) dgs[threadIdx.x] = reinterpret_cast<const float*>(bt + kBndDG)[threadIdx.x];
  __syncthreads();
  const int e0o = hd[1], e0n = hd[2];
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  u4v* z4 = reinterpret_cast<u4v*>(zh);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad / 8;
       i += (int64_t)gridDim.x * blockDim.x) {
    u4v z = __builtin_nontemporal_load(z4 + i);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned lo = z[q] & 0xFFFFu, hi = z[q] >> 16;
      z[q] = zb16_rebase(lo, dgs[lo & 63u], e0o, e0n) | zb16_rebase(hi, dgs[hi & 63u], e0o, e0n) << 16;
    }
    __builtin_nontemporal_store(z, z4 + i);
  }
}

// The build slot of the watch list, in zh_rebase_kernel's
// place while the list path is on: a rebase carries the words as above, and
// when the finalize rebased or chose kWatchFull (no list, its budget spent, an
// overflow) the same pass over the words builds the list: wave w of the
// screen's grid appends offset << 16 | word for every point of [w wrange,
// (w + 1) wrange) with code <= H_label to its own region (no atomics) and
// writes its count.  Code 0 is always listed, a padding row (1023 > H) never.
// A region that overflows sets kWOvf: the screens then stream every word, and
// no list is built again before the next rebase (kWHold).
__global__ __launch_bounds__(256) void zh_watch_kernel(uint16_t* __restrict__ zh, int64_t n_pad,
                                                       unsigned char* __restrict__ bt,
                                                       const long long* __restrict__ gate,
                                                       uint32_t* __restrict__ wl,
                                                       int32_t* __restrict__ wn, int wcap,
                                                       int wrange) {
  if (gate && gate[0] == 0) return;
  const int* hd = reinterpret_cast<const int*>(bt + kBndHdr);
  int* wh = reinterpret_cast<int*>(bt + kBndWatch);
  const bool reb = hd[3] != 0;
  if (!reb && (wh[kWFin] == kWatchList || wh[kWHold])) return;  // the list stands, or none fits
  __shared__ float dgs[64];
  __shared__ unsigned hs[64];
  const int t = threadIdx.x, lane = t & 63;
  if (t < 64) {
    dgs[t] = reinterpret_cast<const float*>(bt + kBndDG)[t];
    hs[t] = reinterpret_cast<const unsigned*>(bt + kBndH)[t];
  }
  __syncthreads();
  if (blockIdx.x == 0) {  // (the other workgroups read kWFin and kBndH only)
    if (t < 64) reinterpret_cast<unsigned*>(bt + kBndHL)[t] = hs[t];
    if (t == 0) {
      wh[kWMode] = kWatchList;
      wh[kWValid] = 1;
      wh[kWEpochs] += 1;
      if (reb) wh[kWCarried] += 1;
    }
  }
  const int e0o = hd[1], e0n = hd[2];
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const int wave = blockIdx.x * 4 + (t >> 6);
  const int64_t p0 = (int64_t)wave * wrange;
  const int64_t p1 = p0 + wrange < n_pad ? p0 + wrange : n_pad;
  uint32_t* const out = wl + (size_t)wave * wcap;
  int cnt = 0;
  constexpr int kU = 4;  // chunks in flight
  for (int64_t c0 = p0; c0 < p1; c0 += kU * kZ16Chunk) {
    u4v z[kU];
#pragma unroll
    for (int i = 0; i < kU; ++i) {
      const int64_t ci = c0 + i * kZ16Chunk < p1 ? c0 + i * kZ16Chunk : c0;  // (past the end: again)
      z[i] = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(zh + ci) + lane);
    }
#pragma unroll
    for (int i = 0; i < kU; ++i) {
      const int64_t ci = c0 + i * kZ16Chunk;
      if (ci >= p1) break;
      if (reb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned lo = z[i][q] & 0xFFFFu, hi = z[i][q] >> 16;
          z[i][q] = zb16_rebase(lo, dgs[lo & 63u], e0o, e0n) |
                    zb16_rebase(hi, dgs[hi & 63u], e0o, e0n) << 16;
        }
        __builtin_nontemporal_store(z[i], reinterpret_cast<u4v*>(zh + ci) + lane);
      }
      const unsigned off = (unsigned)(ci - p0) + 8u * (unsigned)lane;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned w = (z[i][u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
        const bool listed = (w >> 6) <= hs[w & 63u];
        const unsigned long long m = __ballot(listed);
        if (m) {
          const int r = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (listed && r < wcap) out[r] = (off + (unsigned)u) << 16 | w;
          cnt += __popcll(m);
        }
      }
    }
  }
  if (lane == 0) {
    wn[wave] = cnt < wcap ? cnt : wcap;
    if (cnt > wcap) wh[kWOvf] = 1;
  }
}

void zh_rebase(Ctx& c, const long long* gate) {
  if (!c.zb_valid || c.zb_fmt != 16 || !c.bnd_ok) return;  // (no words to carry)
  if (c.watch_on)
    hipLaunchKernelGGL(zh_watch_kernel, dim3(c.watch_waves / 4), dim3(256), 0, c.stream,
                       c.zb.as<uint16_t>(), c.n_pad, static_cast<unsigned char*>(c.bnd.p), gate,
                       c.wl.as<uint32_t>(), c.wn.as<int32_t>(), c.watch_cap, c.watch_range);
  else
    hipLaunchKernelGGL(zh_rebase_kernel, dim3(2048), dim3(256), 0, c.stream, c.zb.as<uint16_t>(),
                       c.n_pad, reinterpret_cast<const unsigned char*>(c.bnd.p), gate);
  HIP_CHECK(hipGetLastError());
}

void bound_words_reset(bool z16, hipStream_t s, const uint8_t* lab8, void* zb, int64_t n,
                       int64_t n_pad, const long long* gate) {
  if (z16)
    hipLaunchKernelGGL(zh_reset_kernel, dim3(2048), dim3(256), 0, s, lab8,
                       static_cast<uint16_t*>(zb), n, n_pad, gate);
  else
    hipLaunchKernelGGL(zb_reset_kernel, dim3(2048), dim3(256), 0, s, lab8,
                       static_cast<uint32_t*>(zb), n, n_pad, gate);
}

int screen32b_blocks_per_cu(int Q, int MT) {
  static int cache[4][2] = {};
  int& nb = cache[Q - 1][MT - 1];
  if (!nb)
    dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
      nb = occupancy_blocks(screen32b<decltype(q)::value, decltype(m)::value>, 0);
    });
  return nb;
}

void screen32b_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32BArgs& p) {
  dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
    hipLaunchKernelGGL((screen32b<decltype(q)::value, decltype(m)::value>), grid, dim3(256), 0, s, p);
  });
}

// chunks in flight per wave of screen32bz (CDR_S32BZ_PD = 4 | 8 | 12)
void screen32bz_launch(dim3 grid, hipStream_t s, const S32BArgs& p) {
  static const int pd = exp_env("CDR_S32BZ_PD") ? std::atoi(exp_env("CDR_S32BZ_PD")) : 8;
  if (pd == 4) hipLaunchKernelGGL(screen32bz<4>, grid, dim3(256), 0, s, p);
  else if (pd == 12) hipLaunchKernelGGL(screen32bz<12>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(screen32bz<8>, grid, dim3(256), 0, s, p);
}

}  // namespace cdr
