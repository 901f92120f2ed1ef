// screen32p.hip — the pruned DELTA screen (d <= 16, k <= 64; configs 2 and 3):
// every DELTA step of the host-plan path, and the device loop's steps without
// bound words.
//
// A k-way screen of every point (64 MFMA values and a keyed top-2 per point,
// ~213 VALU per 64 points) is VALU-issue bound.  After the first step
// almost every point stays with its label a deep inside its cluster, where one
// distance decides it.  screen32p gives each lane ONE point and first tries
// the triangle inequality in distance space (t_j = ||xhat - chat_j|| =
// 2^sigma ||x - C_j||, the reference's distance up to a power of two):
//   t_j >= ||chat_a - chat_j|| - t_a >= h_a - t_a   for every j != a,
// h_a = min_j ||chat_a - chat_j||, so a is the argmin when 2 t_a < h_a (with
// margins).  t_a comes from the hi-only screen copy h = fp16(xhat) in fp32
// (16 v_fma_mix differences and packed fp32 squares against c32_a) and is
// bounded rigorously:
//   | ||h - c32_a|| - sqrt(q_a) | <= 2^-19 sqrt(q_a)   (q_a: 2 roundings + 9
//       along any summation path, every term >= 0; v_sqrt_f32 1 ulp),
//   ||h - xhat|| <= dn  (the fp16 rounding of the point, screen32_prune_dn),
//   ||c32_a - chat_a|| <= ec_a  (the fp32 rounding of the centroid),
// so ub_a = sqrt(q_a)(1 + 2^-18) + E_a with E_a >= (dn + ec_a)(1 + 2^-20)
// bounds t_a from above, and the point keeps a when
//   h_a (1 - 2^-22) - ub_a > ub_a (1 + 2^-20):
// every other exact distance then exceeds t_a by more than 2^-21 relative,
// far above the reference's own fp64 rounding (< 2^-45), so np.argmin of the
// reference's norms is a (src/kmeans_plusplus.py:33-34).
//
// The points this test cannot decide (near a second centroid, or of a
// centroid far from its points) are appended — their 32 (d <= 8: 16) bytes
// and {pt, a} — to a per-wave LDS queue laid out as the MFMA B operands.
// Whenever 64 are queued the wave runs the hi-only k-way screen and its
// certificate on them (screen32_fix.h; the step's plan, keys and bounds), so
// the MFMA work shrinks to the queued fraction; its moved points go to the
// wave's move region, its uncertified ones to its fallback region, and the
// fused fixup (fixup_regions) finishes the step in the workgroup's tail.
// Every point is still read and decided every step.
//
// c32, E and h come with the step's plan (the prune block, plan32.h: built by
// plan32_build on the device right after the centroids move, or by the host's
// build_plan32), so a workgroup only stages 5.6 KB of it into LDS.
// ---------------------------------------------------------------------------
#include "screen32_common.h"
#include "screen32_fix.h"

namespace cdr {

// QH: 2 for d = 9..16 (16 bytes per point half), 1 for d <= 8 (8 bytes);
// MT: 32-centroid tiles of the k-way screen; PD: groups in flight per wave.
template <int Q, int MT, int PD>
__global__ __launch_bounds__(256, 5) void screen32p(S32PArgs a) {
  constexpr int QH = FixDims<Q>::QH;
  if (a.gate && a.gate[0] == 0) return;
  constexpr bool H1 = QH == 1;
  constexpr int kTile = H1 ? 512 : 1024;  // bytes per 32-point tile
  constexpr int kHalf = kTile / 2;
  constexpr int kPB = H1 ? 8 : 16;        // bytes per (point, half)
  constexpr int NWH = kPB / 4;            // dwords per point half
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float c32s[64 * kPrStr + 128];
  float* const eb = c32s + 64 * kPrStr;  // E_j
  float* const hc = eb + 64;             // h_j
  // per wave: a ring of 2 blocks x 64 queued points (2 tiles each, B layout)
  // per wave: a ring of 2 blocks x 64 queued points (2 tiles each, B layout)
  // and their {pt, old label}; after the last drain the same LDS holds the
  // fused fixup's table (FixLds)
  constexpr size_t kQBytes = 4 * 2 * 2 * kTile + 4 * 128 * sizeof(int2);
  __shared__ __attribute__((aligned(16))) unsigned char qlds[kQBytes > kFixLdsBytes ? kQBytes : kFixLdsBytes];
  typedef unsigned char QRow[2][2 * kTile];
  QRow* qd = reinterpret_cast<QRow*>(qlds);
  int2 (*qm)[128] = reinterpret_cast<int2 (*)[128]>(qlds + 4 * 2 * 2 * kTile);
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = t >> 6;
  const int h = lane >> 5;
  const int p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  const int nwaves = gridDim.x * 4;
  const int64_t ngroups = a.n_pad >> 6;
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  struct Buf {
    u4v q0, q1;           // the loaded halves (QH = 2)
    u2v h0, h1;           // (QH = 1)
    unsigned w[2 * NWH];  // the lane's point: half 0 then half 1 (packed fp16 pairs)
    int ob;
  };
  // lane l: point 64 G + l = tile 2 G + (l >> 5), column l & 31
  unsigned loff = (unsigned)(h * kTile + p * kPB);
  unsigned lane4 = (unsigned)lane;
  // The group loads are issued from inline asm (SGPR base + lane offset) and
  // waited for with an explicit vmcnt: the compiler neither sees them nor
  // inserts waits of its own (its waits for conditional loads were vmcnt(0),
  // which drained the prefetch every few groups).  Vector-memory operations
  // complete in issue order, so before group i the wave waits until at most
  // 3 (PD - 1) of them are outstanding: the later groups' loads (and any
  // stores issued after them) may stay in flight.  A group past the end
  // reloads the last one (every iteration issues exactly 3 loads).
  auto load = [&](Buf& b, int64_t G) __attribute__((always_inline)) {
    const int64_t Gc = G < ngroups ? G : ngroups - 1;
    const unsigned char* base = a.XS + (size_t)Gc * (2 * kTile);  // wave-uniform
    const uint8_t* lbase = a.lab8 + Gc * 64;
    if constexpr (H1) {
      asm volatile("global_load_dwordx2 %0, %1, %2\n\t"
                   "global_load_dwordx2 %3, %1, %2 offset:256"
                   : "=&v"(b.h0), "+v"(loff), "+s"(base), "=&v"(b.h1));
    } else {
      asm volatile("global_load_dwordx4 %0, %1, %2\n\t"
                   "global_load_dwordx4 %3, %1, %2 offset:512"
                   : "=&v"(b.q0), "+v"(loff), "+s"(base), "=&v"(b.q1));
    }
    asm volatile("global_load_ubyte %0, %1, %2" : "=&v"(b.ob), "+v"(lane4), "+s"(lbase));
  };
  // wait for buffer b, `later` groups having been issued after it
  auto wait = [&](Buf& b, int later) __attribute__((always_inline)) {
    if constexpr (H1) {
      if (later >= 2) asm volatile("s_waitcnt vmcnt(6)" : "+v"(b.h0), "+v"(b.h1), "+v"(b.ob));
      else if (later == 1) asm volatile("s_waitcnt vmcnt(3)" : "+v"(b.h0), "+v"(b.h1), "+v"(b.ob));
      else asm volatile("s_waitcnt vmcnt(0)" : "+v"(b.h0), "+v"(b.h1), "+v"(b.ob));
      b.w[0] = b.h0.x; b.w[1] = b.h0.y; b.w[2] = b.h1.x; b.w[3] = b.h1.y;
    } else {
      if (later >= 2) asm volatile("s_waitcnt vmcnt(6)" : "+v"(b.q0), "+v"(b.q1), "+v"(b.ob));
      else if (later == 1) asm volatile("s_waitcnt vmcnt(3)" : "+v"(b.q0), "+v"(b.q1), "+v"(b.ob));
      else asm volatile("s_waitcnt vmcnt(0)" : "+v"(b.q0), "+v"(b.q1), "+v"(b.ob));
      b.w[0] = b.q0.x; b.w[1] = b.q0.y; b.w[2] = b.q0.z; b.w[3] = b.q0.w;
      b.w[4] = b.q1.x; b.w[5] = b.q1.y; b.w[6] = b.q1.z; b.w[7] = b.q1.w;
    }
  };
  const int64_t gs = nwaves;
  Buf buf[PD];
  // the first groups' loads overlap the prologue
#pragma unroll
  for (int i = 0; i < PD - 1; ++i) load(buf[i], wave + i * gs);

  // ---- k-way screen plan (the step's fragments and C operand), staged in LDS
  // and read by a wave only when it drains its queue (no VGPRs held):
  // fragments [MT][2][64] h8, C operand as [MT][4][2 halves][4] per 16 values
  __shared__ h8 sA[MT * 2 * 64];
  __shared__ __attribute__((aligned(16))) float sC[MT * 4 * 2 * 4];
  // Every global load of the staging is issued before the first LDS store
  // (one round trip for the whole prologue, not one per loop iteration).
  // cinit[(m * 16 + ii) * 64 + ln] belongs to row 32 m + 8 (ii >> 2) + 4 (ln >> 5)
  // + (ii & 3): one value per (m, ii, ln >> 5), kept as sC[m][ii >> 2][ln >> 5][ii & 3].
  constexpr int kPr4 = (64 * kPrStr + 128) / 4;  // prune block in float4
  static_assert(kPr4 <= 512 && MT * 2 * 64 <= 256, "prologue: two float4 per thread");
  const f4* prune4 = reinterpret_cast<const f4*>(a.prune);
  const f4 pv0 = prune4[t];
  const f4 pv1 = t + 256 < kPr4 ? prune4[t + 256] : f4{0.f, 0.f, 0.f, 0.f};
  h8 av = {};
  if (t < MT * 2 * 64) av = a.frag[t];
  float cv = 0.0f;
  const int cm = t >> 5, ci4 = (t >> 3) & 3, chh = (t >> 2) & 1, cc = t & 3;
  if (t < MT * 32) cv = a.cinit[(cm * 16 + ci4 * 4 + cc) * 64 + chh * 32];
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0, thr_rel = a.thr_rel;
  const float Dlo = (a.thr_dev ? a.thr_dev[1] : a.Dv) * (1.0f - 0x1p-19f);  // < D
  // the plan's fp32 centroids c32, their bounds E and nearest-centroid distances h
  // (contiguous in the plan and here: c32s | eb | hc)
  reinterpret_cast<f4*>(c32s)[t] = pv0;
  if (t + 256 < kPr4) reinterpret_cast<f4*>(c32s)[t + 256] = pv1;
  if (t < MT * 2 * 64) sA[t] = av;
  if (t < MT * 32) sC[t] = cv;
  __syncthreads();

  int2* fb_region = a.fb_list + (size_t)wave * a.cap;
  int2* mv_region = a.mv_list + (size_t)wave * a.cap;
  int fb_used = 0, mv_used = 0;
  // q = ||h - c32_j||^2: one fma_mix difference per feature, packed fp32 squares
  auto dist2 = [&](const Buf& b, int j) __attribute__((always_inline)) -> float {
    const f4* c4 = reinterpret_cast<const f4*>(c32s + j * kPrStr);  // 16-byte rows
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 acc = {0.0f, 0.0f};
    // dword i of the lane's point holds features 2i, 2i + 1 (half 0 then half 1)
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
  // (best, runner-up) keys of one 32-point tile of queued points (hi-only)
  // The centroid tiles m are screened one after another (a loop that is not
  // unrolled, fragments and C operand read from LDS inside it), so only one
  // tile's accumulators are ever live: 4 waves per SIMD instead of 3.
  auto tile = [&](const u4v& v, unsigned& bk, unsigned& sk, float& hp) __attribute__((always_inline)) {
    const h8 BH = __builtin_bit_cast(h8, v);
    hp = 0.0f;  // this lane's part of ||h||^2 (fp16 products are exact in fp32)
#pragma unroll
    for (int i = 0; i < (H1 ? 4 : 8); i += 2)
      hp = __builtin_amdgcn_fdot2(h2{BH[i], BH[i + 1]}, h2{BH[i], BH[i + 1]}, hp, false);
    unsigned b = 0xFFFFFFFFu, s = 0xFFFFFFFFu;
#pragma nounroll
    for (int m = 0; m < MT; ++m) {
      h8 A0 = sA[(m * 2 + 0) * 64 + lane];
      const h8 A1 = sA[(m * 2 + 1) * 64 + lane];
      if constexpr (H1)  // plan (QH = 1): A1 = [-2chi, -2chi], A3 = [-2clo, 0]
#pragma unroll
        for (int i = 0; i < 4; ++i) A0[4 + i] = A1[i];
      f16v acc;
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const f4 c4v = *reinterpret_cast<const f4*>(sC + ((m * 4 + i4) * 2 + h) * 4);
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
    bk = b | ((unsigned)h << 2);
    sk = s | ((unsigned)h << 2);
  };
  // the k-way screen of queue block qb (nvalid entries), then its lists
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
    unsigned bA = 0, sA = 0, bB = 0, sB = 0;
    float hA = 0.0f, hB = 0.0f;
    // one point tile at a time (a loop that is not unrolled)
#pragma nounroll
    for (int tt = 0; tt < 2; ++tt) {
      unsigned bk, sk;
      float hp;
      tile(tt == 0 ? v[0] : v[1], bk, sk, hp);
      if (tt == 0) {
        bA = bk;
        sA = sk;
        hA = hp;
      } else {
        bB = bk;
        sB = sk;
        hB = hp;
      }
    }
    swap32(bA, bB);
    swap32(sA, sB);
    merge_top2(bA, sA, bB, sB);
    const int label = (int)(bA & 63u);
    const float vb = __uint_as_float(bA & ~63u);
    const float vs = __uint_as_float(sA & ~63u);
    float thr = fmaf(vb, thr_rel, thr0);
    {  // the hi-only certificate (screen32_fix.h)
      unsigned ua = __float_as_uint(hA), ub = __float_as_uint(hB);
      swap32(ua, ub);
      const float hh = fmaf(__uint_as_float(ua) + __uint_as_float(ub), 1.0f + 0x1p-18f, 0x1p-20f);
      const float dn = fmaf(0x1p-11f * (1.0f + 0x1p-9f), __builtin_amdgcn_sqrtf(hh), 0x1p-23f);
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
    // both lists in straight-line code (two identical guarded blocks were
    // merged by the optimiser into one updating fb_used / mv_used through a
    // pointer, which put both counters in scratch memory)
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
  int qh = 0, qn = 0;  // queue head (next slot, mod 128) and length: wave-uniform
  int qtot = 0;        // points this wave queued (profiling)
  auto process = [&](const Buf& b, int64_t G) __attribute__((always_inline)) {
    const int64_t base = G << 6;
    if (base >= a.n) return;  // wave-uniform: padding groups have no real points
    const int64_t pt = base + lane;
    const bool real = pt < a.n;
    const int ao = b.ob;
    if (a.abl & 2) {  // timing experiments: streaming only
      if (b.w[0] == 0x7fffffffu && b.w[2 * NWH - 1] == 0x7fffffffu) fb_used += ao;
      return;
    }
    const float qa = dist2(b, ao);
    const float uba = fmaf(__builtin_amdgcn_sqrtf(qa), 1.0f + 0x1p-18f, eb[ao]);
    const bool keep = fmaf(hc[ao], 1.0f - 0x1p-22f, -uba) > uba * (1.0f + 0x1p-20f);
    const bool q = real && !keep;
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
        qm[wv][slot] = int2{(int)pt, ao};
      }
      const int c = __popcll(m);
      qh = (qh + c) & 127;
      qn += c;
      qtot += c;
      if (qn >= 64) {
        if (!(a.abl & 1)) drain(((qh - qn) & 127) >> 6, 64);
        qn -= 64;
      }
    }
  };
  for (int64_t G = wave; G < ngroups; G += PD * gs) {
#pragma unroll
    for (int i = 0; i < PD; ++i) {
      const int64_t Gi = G + i * gs;
      if (Gi >= ngroups) break;
      load(buf[(i + PD - 1) % PD], Gi + (PD - 1) * gs);
      wait(buf[i], PD - 1);
      process(buf[i], Gi);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the reloads past the end
  if (qn > 0) {  // the partial block (queue tail at a block start: 64 | qh - qn)
    drain(((qh - qn) & 127) >> 6, qn);
  }
  // per-wave counts only (their sum is the step's fallback total, formed by
  // the finalize): thousands of same-address atomics at the end of this
  // kernel serialised in L2 for tens of microseconds
  if (lane == 0) {
    a.fb_count[wave] = fb_used;
    a.mv_count[wave] = mv_used;
    if (a.q_acc) a.q_acc[wave] += qtot;  // (profiling) this wave's own slot
  }
  if (!a.fuse) return;
  // ---- the fixup of this workgroup's four waves (screen32_fix.h), fused: no extra
  // launch, and the tail of one workgroup overlaps the others' streaming ----
  __syncthreads();  // every queue drained (its LDS becomes the table); lists written
  const FixLds L(qlds);
  if (lane == 0) {
    L.s_mv[wv + 1] = mv_used;
    L.s_fb[wv + 1] = fb_used;
  }
  fixup_regions<Q, MT>(a.fx, blockIdx.x * 4, 4, blockIdx.x % kRunSlices, L, FixPlan{sA, sC});
}

// (3 groups in flight per wave)
int screen32p_blocks_per_cu(int Q, int MT) {
  static int cache[4][2] = {};
  int& nb = cache[Q - 1][MT - 1];
  if (!nb)
    dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
      nb = occupancy_blocks(screen32p<decltype(q)::value, decltype(m)::value, 3>, 0);
    });
  return nb;
}

void screen32p_launch(int Q, int MT, dim3 grid, hipStream_t s, const S32PArgs& p) {
  dispatch_q_mt<4>(Q, MT, [&](auto q, auto m) {
    hipLaunchKernelGGL((screen32p<decltype(q)::value, decltype(m)::value, 3>), grid, dim3(256), 0, s,
                       p);
  });
}

}  // namespace cdr
