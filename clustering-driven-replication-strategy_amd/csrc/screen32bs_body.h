// screen32bs_body.h - one form of screen32bs from its first statement to its
// last: included inside a kernel of screen32bs.hip (not a header of
// declarations), with the kernel's argument B, the constants Q, MT, SPLIT,
// WATCH and MERGED and the LDS arrays of S32BS_LDS in scope.  A body and not a
// device function: screen32bsw runs two forms on one set of LDS arrays, which
// each form names directly, and the default form's kernel keeps the code it
// had as the only body of its kernel (a force-inlined function template
// around the same text, with its arguments by reference or by value, changed
// the register allocation of every instantiation).
  static_assert(!(SPLIT && WATCH) && (!WATCH || CDR_S32BS_LAZY), "the WATCH form: 2-byte words, lazy phase 2");
  const S32PArgs& a = B.p;
  const FixArgs& F = a.fx;
#ifdef CDR_EXPERIMENTS
  unsigned long long tp[8] = {__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0, 0, 0};
#define CDR_TP(i) tp[i] = __builtin_amdgcn_s_memrealtime()
#else
#define CDR_TP(i)
#endif
  constexpr int QH = FixDims<Q>::QH;
  constexpr int DM = FixDims<Q>::DM;
  // near ties: the fused kernel lists them and resolves them after its last
  // batch (inlined in the streaming loop, the resolver costs registers and
  // code the stream needs); the split decide kernel resolves them at once
#ifndef CDR_S32BS_DEFER
#define CDR_S32BS_DEFER 1
#endif
  constexpr bool DEFER = !SPLIT && CDR_S32BS_DEFER;
  if constexpr (!MERGED) {  // (screen32bsw has done this)
  // the dynamic tail's counters for the next launch (the other parity; before
  // the gate, so a skipped launch leaves them zeroed too)
  if (!SPLIT && B.dyn && blockIdx.x == 0 && threadIdx.x < 32)
    B.dyn[((B.dyn_par ^ 1) * 32 + threadIdx.x) * 32] = 0u;
  if (a.gate && a.gate[0] == 0) return;
  // the watch list's mode word: with a list in the arguments
  // the default form runs only while the mode asks for no list
  if constexpr (!SPLIT) {
    if (B.watch) {
      const bool list = B.watch[kWMode] == kWatchList && B.watch[kWOvf] == 0;
      if (list != WATCH) return;
      if (blockIdx.x == 0 && threadIdx.x == 0) {  // (cdr_lloyd_watch_info)
        B.watch[WATCH ? kWListN : kWFullN] += 1;
        B.watch[kWLast] = WATCH ? kWatchList : kWatchFull;
      }
    }
  }
  }
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  float* const eb = c32s + 64 * kPrStr;  // E_j
  float* const hc = eb + 64;             // h_j
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = t >> 6;
  const int h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  const int64_t nchunks = B.nchunks;
  const int k = a.k, d = a.d, d1 = d + 1;
  // (screen32bsw: the host's Q is d4_of(d) / 4, so the features of the first
  // Q - 1 quads are all real; said here, the two bodies' per-feature tests fit
  // the scalar registers of one kernel.  The stand-alone kernels keep their code)
  if constexpr (MERGED) __builtin_assume(d > 4 * (Q - 1));
  // the WATCH form: this wave's entries (offset << 16 | word) of the points
  // from pbase on; the LDS list holds the failed entries and, kWL words on,
  // their slots
  uint32_t* const wlw = WATCH ? B.wl + (size_t)wave * B.wcap : nullptr;
  const int pbase = WATCH ? wave * B.wrange : 0;

  // ---- phase 1 loads: 2-byte words, 8 per lane per 1 KiB chunk (the split
  // form: screen32bz streamed 4-byte words) ----
  // points per chunk and the entry format's chunk-iteration shift
  constexpr int CH = SPLIT ? kBChunk : kZ16Chunk;
  constexpr int SH = SPLIT ? 14 : 15;
  auto zload = [&](u4v& z, int64_t ci) __attribute__((always_inline)) {
    const int64_t cc = ci < nchunks ? ci : nchunks - 1;
    z = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(B.zh + cc * kZ16Chunk) + lane);
  };
  // this wave's chunks: wbase + i wstride below wend
  int64_t wbase, wend;
  int wstride;
  int64_t rR0 = 0;
  int rsl = 0;
  bs_range(B, wv, wbase, wstride, wend, &rR0, &rsl);
  // the dynamic tail (B.dyn): this wave's static chunks end at swend, the
  // region's pool [P0, wend) goes out kBPD chunks at a time from dctr
  // (chunk indices: int, below 2^31 - the host's n_pad)
  const bool dyn = !SPLIT && !WATCH && B.dyn != nullptr && B.slot_wg > 0;
  // The pool is split over the 8 XCDs (workgroup b runs on XCD b % 8), one
  // counter each in its own 128-byte line: claims on one address serialise
  // (~10 ns apart, measured), so one counter per region holds the waves up
  int swend = (int)wend, P0 = (int)wend, P1 = (int)wend;
  if (dyn) {
    const int spw = (int)((wend - rR0) * B.dyn_pct / 100 / wstride);  // static chunks per wave
    swend = (int)rR0 + spw * wstride;
    const int xcd = blockIdx.x & 7;
    P0 = swend + (int)((wend - swend) * xcd / 8);
    P1 = swend + (int)((wend - swend) * (xcd + 1) / 8);
  }
  // the entries' chunk field: region-relative chunk (dynamic tail) or the
  // chunk ordinal in this wave's range
  const int ebase = dyn ? (int)rR0 : (int)wbase;
  const int estride = dyn ? 1 : wstride;
  u4v zc[kBPD];

  // ---- the plan ----
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
  // lane j: W_j (4-byte words: wup for the test, wdn for new words); 2-byte
  // words: W_j - G_j for new words (the thresholds T_j: LDS, below) and the
  // codes' exponent
  float wup_l = 0.0f, wnew_l;
  int e0n = 0;
  if constexpr (SPLIT) {
    wup_l = B.wup[lane];
    wnew_l = B.wdn[lane];
  } else {
    wnew_l = reinterpret_cast<const float*>(B.bt + kBndWdg)[lane];
    e0n = reinterpret_cast<const int*>(B.bt + kBndHdr)[2];
  }
  // a decided point's word (ok: bounds (l0, u0); w = __shfl(wnew_l, lab),
  // taken by every lane) or "no bound"; the WATCH form writes it to the
  // point's entry (slot sl) too: the two always agree, so the default form
  // can take over at any step
  auto zput = [&](int pt, int sl, bool ok, float l0, float u0, float w, unsigned lab) __attribute__((always_inline)) {
    if constexpr (SPLIT) {
      B.zb[pt] = ok ? zb_pack(l0, u0, w, lab) : (kZbStale | lab);
    } else {
      const unsigned short w16 = ok ? zb16_pack(l0, u0, w, e0n, lab) : (unsigned short)lab;
      B.zh[pt] = w16;
      if constexpr (WATCH) wlw[sl] = (unsigned)(pt - pbase) << 16 | w16;
    }
  };
  const float msv = lane < d ? F.ms[lane] : 0.0f;        // lane f: -mu_f 2^sigma
  const float thr0 = a.thr_dev ? a.thr_dev[0] : a.thr0, thr_rel = a.thr_rel;
  const float Dv = a.thr_dev ? a.thr_dev[1] : a.Dv;
  const float Dlo = Dv * (1.0f - 0x1p-19f), Dhi = Dv * (1.0f + 0x1p-19f);
  const float sig = F.sig;
  // The WATCH form: the list's count and its first group of kBPD entry loads
  // go out behind the plan's loads, so they return under the LDS set-up
  // instead of as two more dependent round trips after the barrier.  The loads
  // need no count: load i of the region, clamped to the region's last one
  // (regions are whole multiples of 256 entries; the last wave's ends the
  // buffer), and insertw ignores entries at or past the count.  The code
  // thresholds are loaded before them, so their LDS copy waits for no entry.
  // The count is read into a register here and made uniform only behind the
  // LDS set-up: asked for at once, it would be a round trip of its own ahead
  // of the entry loads.
  int wtotal = 0;
  unsigned tlv = 0;
  if constexpr (WATCH) {
    wtotal = B.wn[wave];
    if (t < 64) tlv = (B.dbg & 1) ? 1022u : reinterpret_cast<const unsigned*>(B.bt + kBndT)[t];
    const int lastl = (B.wcap >> 8) - 1;
    const u4v* const wl4 = reinterpret_cast<const u4v*>(wlw);
#pragma unroll
    for (int i = 0; i < kBPD; ++i) {
      __builtin_amdgcn_sched_barrier(0);  // (issued in order, after the plan's)
      zc[i] = wl4[(size_t)(i < lastl ? i : lastl) * 64 + lane];
    }
    __builtin_amdgcn_sched_barrier(0);
    // (the thresholds' LDS copy here, ahead of the loop that clears the move
    // table: behind it the compiler waits for every load in flight)
    if (t < 64) tls[t] = tlv;
  }
  reinterpret_cast<f4*>(c32s)[t] = pv0;
  if (t + 256 < kPr4) reinterpret_cast<f4*>(c32s)[t + 256] = pv1;
  if (t < MT * 2 * 64) sA[t] = av;
  if (t < MT * 32) sC[t] = cv;
  for (int e = t; e < 64 * 17; e += 256) mtab[e] = 0ull;
  if (t < 16) msl[t] = msv;
  if constexpr (!SPLIT && !WATCH) {
    // (CDR_BOUNDS_DBG=1, tests: every real point's bound fails)
    if (t < 64) tls[t] = (B.dbg & 1) ? 1022u : reinterpret_cast<const unsigned*>(B.bt + kBndT)[t];
  }
  if constexpr (WATCH) wtotal = __builtin_amdgcn_readfirstlane(wtotal);
  __syncthreads();
  CDR_TP(1);

  // (fb_used: the wave's tail records, fb_cert of them certified in the tail)
  int fb_used = 0, fb_cert = 0, mv_used = 0, qtot = 0, ttot = 0;
  const f4* XA4 = reinterpret_cast<const f4*>(F.XA);  // point i: XA4[i * Q + q]

  // (best, runner-up) keys of one 32-point tile of the split screen
  auto screen_m = [&](int m, const u4v (&v)[QH]) __attribute__((always_inline)) -> f16v {
    asm volatile("" ::: "memory");  // the plan is read here, not held in registers
    const h8 A0 = sA[(m * 2 + 0) * 64 + lane];
    const h8 A1 = sA[(m * 2 + 1) * 64 + lane];
    f16v acc;
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const f4 c4v = *reinterpret_cast<const f4*>(sC + ((m * 4 + i4) * 2 + h) * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[4 * i4 + i] = c4v[i];
    }
    const h8 BH = __builtin_bit_cast(h8, v[0]);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, BH, acc, 0, 0, 0);
    if constexpr (QH == 2) {
      const h8 BL = __builtin_bit_cast(h8, v[QH - 1]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, BL, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, BH, acc, 0, 0, 0);
  };
  auto tile = [&](const u4v (&v)[QH], unsigned& bk, unsigned& sk) __attribute__((always_inline)) {
    unsigned b = 0xFFFFFFFFu, s = 0xFFFFFFFFu;
#pragma nounroll
    for (int m = 0; m < MT; ++m) {
      const f16v acc = screen_m(m, v);
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
  // candidate rows of tile v for the point of this lane's column (threshold
  // tau of that point): bit 16 m + i = value i of centroid tile m in half h
  auto cmask = [&](const u4v (&v)[QH], float tau) __attribute__((always_inline)) -> unsigned {
    unsigned r = 0;
#pragma nounroll
    for (int m = 0; m < MT; ++m) {
      const f16v acc = screen_m(m, v);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float kv = __uint_as_float(__float_as_uint(acc[i]) & ~63u);
        if (!(kv > tau)) r |= 1u << (16 * m + i);  // (NaN: a candidate)
      }
    }
    return r;
  };
  // q = ||xhat32 - c32_j||^2 in fp32: one rounding per difference, two fma
  // chains of <= 8 and one add, every term >= 0, so |q - exact| <= 2^-20 q
  // and |sqrt(q) - ||xhat32 - c32_j||| <= 2^-19 sqrt(q) (v_sqrt_f32: 1 ulp)
  auto q32 = [&](const float (&xh)[DM], int j) __attribute__((always_inline)) -> float {
    const f4* c4 = reinterpret_cast<const f4*>(c32s + j * kPrStr);
    f2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const f4 cq = c4[q];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f2 df = {xh[4 * q + 2 * u] - cq[2 * u], xh[4 * q + 2 * u + 1] - cq[2 * u + 1]};
        acc = __builtin_elementwise_fma(df, df, acc);
      }
    }
    return acc.x + acc.y;
  };
  struct GB {
    f4 x[Q];  // the point's fp32 row
    int pt, ao;
    int sl;  // (WATCH) the entry's slot
    bool valid;
  };
  // the split screen operands of the wave's 64 rows (lane l: point l): the
  // hi / lo halves of xhat32; lanes 0-31 keep their own half 0 for tile 0 and
  // receive lane 32 + p's half 0 for tile 1, lanes 32-63 receive lane p's
  // half 1 for tile 0 and keep their own half 1 for tile 1
  auto split_tiles = [&](const float (&xh)[DM], u4v (&T0)[QH], u4v (&T1)[QH]) __attribute__((always_inline)) {
    unsigned hw[4 * QH], lw[4 * QH];
#pragma unroll
    for (int qq = 0; qq < 2 * QH; ++qq) {
      f4 xt = {0.f, 0.f, 0.f, 0.f};
      if (qq < Q) xt = f4{xh[4 * qq], xh[4 * qq + 1], xh[4 * qq + 2], xh[4 * qq + 3]};
      split4(xt, hw[2 * qq], hw[2 * qq + 1], lw[2 * qq], lw[2 * qq + 1]);
    }
    unsigned ad[4 * QH], bd[4 * QH];  // quads 0 .. QH-1 | quads QH .. 2QH-1
    if constexpr (QH == 1) {  // [hi(q), lo(q)]
      ad[0] = hw[0]; ad[1] = hw[1]; ad[2] = lw[0]; ad[3] = lw[1];
      bd[0] = hw[2]; bd[1] = hw[3]; bd[2] = lw[2]; bd[3] = lw[3];
    } else {  // [hi(q0), hi(q1)], [lo(q0), lo(q1)]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ad[i] = hw[i];
        ad[4 + i] = lw[i];
        bd[i] = hw[4 + i];
        bd[4 + i] = lw[4 + i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4 * QH; ++i) swap32(ad[i], bd[i]);
#pragma unroll
    for (int u = 0; u < QH; ++u) {
      T0[u] = u4v{ad[4 * u], ad[4 * u + 1], ad[4 * u + 2], ad[4 * u + 3]};
      T1[u] = u4v{bd[4 * u], bd[4 * u + 1], bd[4 * u + 2], bd[4 * u + 3]};
    }
  };
  // (best, runner-up) keys of this lane's point over both tiles and halves
  auto keys = [&](const u4v (&T0)[QH], const u4v (&T1)[QH], unsigned& b, unsigned& s) __attribute__((always_inline)) {
    unsigned bB, sB;
    tile(T0, b, s);
    tile(T1, bB, sB);
    swap32(b, bB);
    swap32(s, sB);
    merge_top2(b, s, bB, sB);
  };
  auto rowhat = [&](const f4 (&x)[Q], float (&xh)[DM]) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < DM; ++f) xh[f] = f < d ? fmaf(x[f >> 2][f & 3], sig, msl[f]) : 0.0f;
  };
  // a point leaving cluster ao for lab: labels and this workgroup's table
  // (row: the point's row when the caller holds it, else read again)
  auto move = [&](bool live, int pt, int ao, int lab, const f4* row) __attribute__((always_inline)) {
    const bool moved = live && lab != ao;
    const unsigned long long mm = __ballot(moved);
    if (!mm) return;
    if (moved) {
      a.labels[pt] = lab;
      a.lab8[pt] = (uint8_t)lab;
      f4 xr[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) xr[q] = row ? row[q] : XA4[(int64_t)pt * Q + q];
#pragma unroll
      for (int f = 0; f < DM; ++f) {
        if (f < d) {
          const long long v = __double2ll_rn((double)xr[f >> 2][f & 3] * F.fx);
          atomicAdd(&mtab[lab * d1 + f], (unsigned long long)v);
          atomicAdd(&mtab[ao * d1 + f], (unsigned long long)-v);
        }
      }
      atomicAdd(&mtab[lab * d1 + d], 1ull);
      atomicAdd(&mtab[ao * d1 + d], ~0ull);
    }
    mv_used += __popcll(mm);
  };
  int2* fb_region = a.fb_list + (size_t)wave * a.cap;
  // a tail record's first word: the point; the WATCH form: the point's offset
  // in the wave's range << 16 | its entry's slot (both below 2^16: a range is
  // at most kS32WatchMaxRange points and a region at most a range of entries),
  // so the tail needs no load of the entry between the record and the row
  auto rec_x = [&](int pt, int sl) __attribute__((always_inline)) -> int {
    return WATCH ? (int)((unsigned)(pt - pbase) << 16 | (unsigned)sl) : pt;
  };
  // A point the split screen could not certify (a near tie; best key bkey):
  // every centroid whose key is within the threshold of the best is a
  // candidate (|S_j - T_j| <= E: the reference's argmin is among them); the
  // candidates' direct fp32 distances from the LDS c32 copy decide with
  // rigorous intervals, and only an interval overlap falls to the exact fp64
  // NumPy-order evaluation (np.argmin of the reference's norms,
  // src/kmeans_plusplus.py:33-34).  Every lane of the wave calls it (the
  // screen values come from MFMAs over the wave's 64 points); lanes with
  // live = false return ao.  c2: decided by the direct distances, with the
  // bounds (u0, l0) of its new bound word; otherwise the point keeps "no
  // bound".
  auto near_tie = [&](bool live, int ao, unsigned bkey, const float (&xh)[DM],
                      const u4v (&T0)[QH], const u4v (&T1)[QH], const f4 (&xr)[Q], float xx,
                      bool& c2, float& u0, float& l0) __attribute__((always_inline)) -> int {
    const double* cs = F.cent;
    const float tau = fmaf(__uint_as_float(bkey & ~63u), thr_rel, thr0);
    // tile tt's column p is the point of lane 32 tt + p, which holds its tau
    unsigned mine[2], other[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const float tau_t = __shfl(tau, 32 * tt + p);
      const unsigned r = cmask(tt == 0 ? T0 : T1, tau_t);
      mine[tt] = r;
      other[tt] = (unsigned)__shfl_xor((int)r, 32);
    }
    int lab = ao;
    c2 = false;
    u0 = l0 = 0.0f;
    if (live) {
      unsigned long long cand = 0;
      const unsigned mh0 = h == 0 ? mine[0] : other[1], mh1 = h == 0 ? other[0] : mine[1];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        unsigned mmk = hh ? mh1 : mh0;  // rows of half hh of this lane's tile
        while (mmk) {
          const int bb = __builtin_ctz(mmk);
          mmk &= mmk - 1;
          const int m = bb >> 4, i = bb & 15;
          cand |= 1ull << (32 * m + 8 * (i >> 2) + 4 * hh + (i & 3));
        }
      }
      if (k < 64) cand &= (1ull << k) - 1;
      // the candidates' direct fp32 distances (c32 in LDS): t_j = ||xhat -
      // chat_j|| lies within sqrt(q_j) (1 -+ 2^-19) -+ (dn32 + ec_j), where
      // dn32 >= ||xhat32 - xhat|| and ec_j >= ||c32_j - chat_j||: c32 is
      // the fp32 rounding of chat_j in fp64, so ec_j <= (2^-24 + 2^-51)
      // ||chat_j|| <= 2^-24 (1 + 2^-18) ||c32_j||
      const float xu = fmaf(xx, 1.0f + 0x1p-19f, 0x1p-120f);
      const float xl = xx * (1.0f - 0x1p-19f);
      const float dn32 = fmaf(0x1p-24f * (1.0f + 0x1p-20f), __builtin_amdgcn_sqrtf(xu), 0x1p-120f);
      float ub = INFINITY, lo_other = INFINITY, lb_best = INFINITY, rbest = INFINITY;
      int jb = 0;
      bool bad = false;  // a NaN distance: the exact pass decides
      unsigned long long cm2 = cand;
      while (cm2) {  // increasing j
        const int j = __builtin_ctzll(cm2);
        cm2 &= cm2 - 1;
        float nc;
        {
          const float zr[DM] = {};
          nc = q32(zr, j);  // ||c32_j||^2 (the same rounding bound)
        }
        const float ec = fmaf(0x1p-24f * (1.0f + 0x1p-18f),
                              __builtin_amdgcn_sqrtf(nc * (1.0f + 0x1p-19f)), 0x1p-120f);
        const float e2 = (dn32 + ec) * (1.0f + 0x1p-20f);
        const float r = __builtin_amdgcn_sqrtf(q32(xh, j));
        const float U = fmaf(r, 1.0f + 0x1p-19f, e2), L = fmaf(r, 1.0f - 0x1p-19f, -e2);
        bad = bad || !(U == U) || !(L == L);
        if (r < rbest) {
          lo_other = fminf(lo_other, lb_best);
          rbest = r;
          ub = U;
          lb_best = L;
          jb = j;
        } else {
          lo_other = fminf(lo_other, L);
        }
      }
      // every other centroid's key is above tau: its distance is at least
      const float gs = tau - ((thr0 + Dhi) - xl);
      const float lnc = fmaf(__builtin_amdgcn_sqrtf(fmaxf(gs, 0.0f)), 1.0f - 0x1p-19f, -dn32);
      c2 = !bad && rbest < INFINITY && lo_other > ub * (1.0f + 0x1p-20f);
      if (c2) {
        lab = jb;
        u0 = ub;
        l0 = fminf(lo_other, lnc);
      } else {
        float x[16];  // fp32 data, converted exactly where used
#pragma unroll
        for (int f = 0; f < 16; ++f) x[f] = f < DM ? xr[f >> 2][f & 3] : 0.0f;
        double sb = INFINITY, rb = INFINITY;
        int jmin = 0x7fffffff;
        while (cand) {  // increasing j
          const int j = __builtin_ctzll(cand);
          cand &= cand - 1;
          const double sq = np_sqdist16(x, cs + j * d, d);
          if (sq < sb) {  // sqrt is monotone: only a smaller square gives a smaller root
            const double rt = sqrt(sq);
            sb = sq;
            if (rt < rb) {
              rb = rt;
              jmin = j;
            }
          }
        }
        lab = jmin >= k ? 0 : jmin;  // every root NaN: np.argmin of all-NaN is 0
      }
    }
    return lab;
  };
  // ||xhat32||^2 (fp32, 16 roundings at most: relative 2^-19 covers them)
  auto norm2 = [&](const float (&xh)[DM]) __attribute__((always_inline)) -> float {
    f2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int f = 0; f < DM; f += 2) {
      const f2 v = {xh[f], xh[f + 1]};
      acc = __builtin_elementwise_fma(v, v, acc);
    }
    return acc.x + acc.y;
  };
  // K-case: a certified point's bounds from its split keys (vb, vs)
  auto kcase = [&](float xx, float vb, float vs, float& u0, float& l0) __attribute__((always_inline)) {
    const float xu = fmaf(xx, 1.0f + 0x1p-19f, 0x1p-120f);  // >= ||xhat32||^2
    const float xl = xx * (1.0f - 0x1p-19f);               // <= ||xhat32||^2
    const float dn32 = fmaf(0x1p-24f * (1.0f + 0x1p-20f), __builtin_amdgcn_sqrtf(xu), 0x1p-120f);
    const float gb = fmaf(vb, thr_rel, thr0 + xu - Dlo);
    const float gs = vs - ((thr0 + Dhi) - xl);
    u0 = fmaf(__builtin_amdgcn_sqrtf(fmaxf(gb, 0.0f)), 1.0f + 0x1p-19f, dn32);
    l0 = fmaf(__builtin_amdgcn_sqrtf(fmaxf(gs, 0.0f)), 1.0f - 0x1p-19f, -dn32);
  };
  // one gathered batch: lane l decides point l
  auto decide = [&](const GB& g) __attribute__((always_inline)) {
    const bool valid = g.valid;
    const int pt = g.pt, ao = g.ao, sl = g.sl;
    float xh[DM];
    rowhat(g.x, xh);
    const float qa = q32(xh, ao);
    const float xx = norm2(xh);
    bool need;  // the lanes the k-way screen decides
    if (B.direct) {
      // The direct test: fp32 distances to c_ao and its two
      // nearest centroids n1, n2 with near_tie's intervals, t_j within
      // sqrt(q_j) (1 -+ 2^-19) -+ (dn32 + ec32_j); every other centroid j is
      // at least ||chat_ao - chat_j|| - t_ao >= h3_ao - U_ao away.  Decided:
      // the smallest root's upper end lies below every other lower end and
      // that rest bound (a NaN decides nothing)
      const f4 nv = reinterpret_cast<const f4*>(c32s + ao * kPrStr)[4];
      const int n1 = __float_as_int(nv[kPrN1 - 16]), n2 = __float_as_int(nv[kPrN2 - 16]);
      const float xu = fmaf(xx, 1.0f + 0x1p-19f, 0x1p-120f);
      const float dn32 = fmaf(0x1p-24f * (1.0f + 0x1p-20f), __builtin_amdgcn_sqrtf(xu), 0x1p-120f);
      int jb = ao;
      float rbest = 0.0f, ub = 0.0f, lb_best = 0.0f, lo = INFINITY, ua = 0.0f;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // ao, n1, n2 ("none": +inf away)
        const int jn = c == 0 ? ao : (c == 1 ? n1 : n2);
        const bool none = (unsigned)jn >= 64u;  // (-1; anything else out of range too)
        const int j = none ? ao : jn;
        const float q = c == 0 ? qa : (none ? INFINITY : q32(xh, j));
        const float ec = c == 0 ? nv[kPrEc - 16] : c32s[j * kPrStr + kPrEc];
        const float e2 = (dn32 + ec) * (1.0f + 0x1p-20f);
        const float r = __builtin_amdgcn_sqrtf(q);
        const float U = fmaf(r, 1.0f + 0x1p-19f, e2), L = fmaf(r, 1.0f - 0x1p-19f, -e2);
        bad = bad || !(U == U) || !(L == L);
        if (c == 0) {
          rbest = r;
          ub = ua = U;
          lb_best = L;
        } else if (r < rbest) {
          lo = fminf(lo, lb_best);
          rbest = r;
          ub = U;
          lb_best = L;
          jb = j;
        } else {
          lo = fminf(lo, L);
        }
      }
      const float l0 = fminf(lo, fmaf(nv[kPrH3 - 16], 1.0f - 0x1p-22f, -ua));
      const bool dec = !bad && l0 > ub * (1.0f + 0x1p-20f);
      const float w_b = __shfl(wnew_l, jb);
      if (valid && dec) zput(pt, sl, true, l0, ub, w_b, (unsigned)jb);
      move(valid && dec, pt, ao, jb, g.x);
      need = valid && !dec;
    } else {
      // (CDR_S32BS_DIRECT=0) the triangle test: q = ||xhat32 - c32_a||^2
      const float uba = fmaf(__builtin_amdgcn_sqrtf(qa), 1.0f + 0x1p-18f, eb[ao]);
      const float l0P = fmaf(hc[ao], 1.0f - 0x1p-22f, -uba);
      const bool keep = l0P > uba * (1.0f + 0x1p-20f);
      const float w_ao = __shfl(wnew_l, ao);
      if (valid && keep) zput(pt, sl, true, l0P, uba, w_ao, (unsigned)ao);
      need = valid && !keep;
    }
    const unsigned long long nm = __ballot(need);
    if (!nm) return;
    qtot += __popcll(nm);
#ifdef CDR_EXPERIMENTS
    if (B.dbg & 8) return;  // (timing: no k-way screen)
#endif
    if constexpr (DEFER) {
      // a few undecided lanes: "not screened" records (the old label in the
      // key's low bits), screened with the tail's batches
      if (B.direct && __popcll(nm) < kDirectDense) {
        if (need) {
          const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(nm >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((unsigned)nm, 0u));
          fb_region[fb_used + r] = int2{rec_x(pt, sl), (int)(kNotScreened | (unsigned)ao)};
        }
        // (readfirstlane: also keeps this update apart from the other counters',
        // which the compiler otherwise merges into one indexed stack slot)
        fb_used = __builtin_amdgcn_readfirstlane(fb_used + __popcll(nm));
        return;
      }
    }
    unsigned bA, sA_;
    u4v T0[QH], T1[QH];
    split_tiles(xh, T0, T1);
    keys(T0, T1, bA, sA_);
    const int label = (int)(bA & 63u);
    const float vb = __uint_as_float(bA & ~63u);
    const float vs = __uint_as_float(sA_ & ~63u);
    const bool cert = vs > fmaf(vb, thr_rel, thr0);  // NaN: never certified
    const bool unc = need && !cert;
    const float w_lab = __shfl(wnew_l, label);
    // K-case: the point's bound word from its split keys
    if (need && cert) {
      float u0, l0;
      kcase(xx, vb, vs, u0, l0);
      zput(pt, sl, true, l0, u0, w_lab, (unsigned)label);
    }
    const unsigned long long um = __ballot(unc);
    if constexpr (DEFER) {
    // uncertified (near ties): the wave's list {point, best key}, resolved
    // after the workgroup's last batch
    if (um) {
      if (unc) {
        const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(um >> 32),
                                                __builtin_amdgcn_mbcnt_lo((unsigned)um, 0u));
        // (the best key's label bits carry the old label: near_tie reads
        // the key's value only, and the tail needs no lab8 load)
        fb_region[fb_used + r] = int2{rec_x(pt, sl), (int)((bA & ~63u) | (unsigned)ao)};
      }
      fb_used += __popcll(um);
    }
    move(need && cert, pt, ao, label, nullptr);
    } else {
    // uncertified (near ties, ~1 in 5 re-read points at config 3) resolved
    // now, while the row, the split operands and the best key are in
    // registers: no list, no dependent re-gather of the row and label
    int labf = label;
    if (um) {
#ifdef CDR_EXPERIMENTS
      if (!(B.dbg & 2)) {  // (timing: no near-tie pass)
#endif
      bool c2;
      float u0, l0;
      const int lab = near_tie(unc, ao, bA, xh, T0, T1, g.x, xx, c2, u0, l0);
      const float wl = __shfl(wnew_l, lab);
      if (unc) {
        labf = lab;
        zput(pt, sl, c2, l0, u0, wl, (unsigned)lab);
      }
#ifdef CDR_EXPERIMENTS
      } else if (unc) {
        labf = ao;
      }
#endif
      fb_used += __popcll(um);
    }
    move(need, pt, ao, labf, g.x);
    }
  };

  // ---- phase 2: the listed points, 64 per batch, two batches in flight ----
  unsigned* const fl = flist[wv];
  constexpr int kWL = kSList / 2;             // (WATCH) entries the LDS list holds
  constexpr int LS = WATCH ? kWL : kSList;    // ... of either form
  constexpr int kRoom = WATCH ? 256 : CH;     // ... and one load's worth of them
  // listed entry e: its point, old label (and slot), the row's loads
  auto gfill = [&](GB& g, int e) __attribute__((always_inline)) {
    const unsigned ent = fl[e];
    int64_t pt;
    if constexpr (WATCH) {
      pt = pbase + (int)(ent >> 16);
      g.sl = (int)fl[kWL + e];
    } else {
      const int64_t ci = ebase + (int64_t)(ent >> SH) * estride;
      pt = ci * CH + ((ent >> 6) & (CH - 1));
      g.sl = 0;
    }
    g.pt = (int)pt;
    g.ao = (int)(ent & 63);
#pragma unroll
    for (int q = 0; q < Q; ++q) g.x[q] = __builtin_nontemporal_load(XA4 + pt * Q + q);
  };
  auto gload = [&](GB& g, int b, int cnt) __attribute__((always_inline)) {
    const int e = 64 * b + lane;
    g.valid = e < cnt;
    gfill(g, g.valid ? e : 64 * b);  // (entry 64 b exists)
  };
  auto phase2 = [&](int& cnt, bool last) __attribute__((always_inline)) {
    const int nb = last ? (cnt + 63) >> 6 : cnt >> 6;
    if (nb == 0) return;
    ttot += last ? cnt : nb * 64;
#ifdef CDR_EXPERIMENTS
    if (B.dbg & 4) {  // (timing: the listed points are not decided)
      cnt = 0;
      return;
    }
#endif
    // the next batch's rows load while one is decided (past the end: the
    // last batch again, not decided); the copy waits for them after it
#if CDR_S32BS_DEPTH >= 3
    GB cur, nxt, nx2;
    gload(cur, 0, cnt);
    gload(nxt, nb > 1 ? 1 : 0, cnt);
#pragma nounroll
    for (int b = 0; b < nb; ++b) {
      gload(nx2, b + 2 < nb ? b + 2 : nb - 1, cnt);
      decide(cur);
      cur = nxt;
      nxt = nx2;
    }
#else
    GB cur, nxt;
    gload(cur, 0, cnt);
#pragma nounroll
    for (int b = 0; b < nb; ++b) {
      gload(nxt, b + 1 < nb ? b + 1 : nb - 1, cnt);
      decide(cur);
      cur = nxt;
    }
#endif
    const int done = nb * 64;
    const int rem = last ? 0 : cnt - done;
    if (rem > 0) {
      const unsigned v = lane < rem ? fl[done + lane] : 0u;
      __builtin_amdgcn_wave_barrier();
      if (lane < rem) fl[lane] = v;
    }
    cnt = rem;
  };

  if constexpr (SPLIT) {
    // ---- the list screen32bz's wave `wave` wrote: 64 entries per batch ----
    const uint32_t* const L = B.zl + (size_t)wave * B.zcap;
    const int total = B.zn[wave];
    const int nb = (total + 63) >> 6;
    ttot = total;
    if (nb > 0) {
      auto eload = [&](int b) __attribute__((always_inline)) -> unsigned {
        const int e = 64 * b + lane;
        return L[e < total ? e : 64 * b];  // (entry 64 b exists: b < nb)
      };
      auto fill = [&](GB& g, unsigned ent, int b) __attribute__((always_inline)) {
        g.valid = 64 * b + lane < total;
        const int64_t ci = wbase + (int64_t)(ent >> 14) * wstride;
        const int64_t pt = ci * kBChunk + ((ent >> 6) & 255);
        g.pt = (int)pt;
        g.ao = (int)(ent & 63);
        g.sl = 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) g.x[q] = __builtin_nontemporal_load(XA4 + pt * Q + q);
      };
      GB cur, nxt;
      unsigned en = eload(0);
      fill(cur, en, 0);
      en = eload(nb > 1 ? 1 : 0);
#pragma nounroll
      for (int b = 0; b < nb; ++b) {
        // the next batch's rows and the one after's entries load while this
        // batch is decided (past the end: the last batch again, not decided)
        const int b1 = b + 1 < nb ? b + 1 : nb - 1;
        fill(nxt, en, b1);
        en = eload(b + 2 < nb ? b + 2 : nb - 1);
#ifdef CDR_EXPERIMENTS
        if (!(B.dbg & 4))  // (timing: the listed points are gathered, not decided)
#endif
        decide(cur);
        cur = nxt;
      }
    }
  } else {
#if CDR_S32BS_LAZY
  // Phase 2 interleaved with the stream: after every kBPD chunks the batch
  // whose rows were gathered one group of chunks earlier is decided and the
  // next 64 listed points' rows are gathered, so a batch's gather latency
  // hides behind the stream instead of stalling the wave.  Only when the
  // list would overflow (steps where most bounds fail) are batches decided
  // back to back.
  GB cur;
  bool pend = false;
  int head = 0;  // listed entries before head are gathered (wave-uniform)
  // (returns with room for one more chunk's entries: the stream breaks its
  // group early when a chunk would not fit, which only dense failures do)
  auto step2 = [&](int& cnt, bool last) __attribute__((always_inline)) {
    for (;;) {
      if (pend) {
#ifdef CDR_EXPERIMENTS
        const unsigned long long td0 = __builtin_amdgcn_s_memrealtime();
        if (!SPLIT) __builtin_amdgcn_s_waitcnt(0x0F70);  // (timing: the gathered rows' arrival)
        const unsigned long long td1 = __builtin_amdgcn_s_memrealtime();
#endif
        decide(cur);
        pend = false;
#ifdef CDR_EXPERIMENTS
        const unsigned long long td2 = __builtin_amdgcn_s_memrealtime();
        tp[5] += td2 - td1;  // decide
        tp[6] += 1;          // batches
        tp[7] += td1 - td0;  // waiting for the rows (and the stream's loads)
#endif
      }
      const int avail = cnt - head;
      if (avail >= 64 || (last && avail > 0)) {
        const int e = head + lane;
        cur.valid = e < cnt;
        gfill(cur, cur.valid ? e : head);
        const int take = avail < 64 ? avail : 64;
        head = __builtin_amdgcn_readfirstlane(head + take);
        ttot += take;
        pend = true;
      }
      if (head > 0 && !last && cnt + kRoom > LS) {  // compact [head, cnt) to the front
        const int m = cnt - head;
        for (int o = 0; o < m; o += 64) {  // (writes stay below the reads still to come)
          const int e2 = o + lane;
          const unsigned v = e2 < m ? fl[head + e2] : 0u;
          unsigned vs = 0u;
          if constexpr (WATCH) vs = e2 < m ? fl[kWL + head + e2] : 0u;
          __builtin_amdgcn_wave_barrier();
          if (e2 < m) fl[e2] = v;
          if constexpr (WATCH)
            if (e2 < m) fl[kWL + e2] = vs;
          __builtin_amdgcn_wave_barrier();
        }
        cnt = m;
        head = 0;
      }
      const bool again = last ? (pend || cnt > head) : (cnt - head + kRoom > LS);
      if (!again) break;
    }
  };
#else
  constexpr int head = 0;  // (phase 2 in bursts compacts the list itself)
#endif

  if constexpr (WATCH) {
  // ---- phase 1, the WATCH form: this wave's entries, 4 per lane per 16-byte
  // load, kBPD loads issued together and phase 2 between the groups, as
  // below.  An entry fails as its point's word does (code <= T_label); its
  // copy and its slot go on the LDS list.  A load whose entries might not fit
  // the list is left for the next group, which step2 makes room for.
  // The first group's loads went out with the plan's (above).
  const u4v* const wl4 = reinterpret_cast<const u4v*>(wlw);
  const int total = wtotal;
  const int ng = (total + 255) >> 8;
  int cnt = 0;
  auto insertw = [&](const u4v& z, int gi) __attribute__((always_inline)) {
    const int e0 = 256 * gi + 4 * lane;
    unsigned fm = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned w = z[u] & 0xFFFFu;
      fm |= (unsigned)(e0 + u < total && (w >> 6) <= tls[w & 63u]) << u;
    }
    if (__ballot(fm != 0u)) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool fail = (fm >> u) & 1u;
        const unsigned long long m = __ballot(fail);
        if (m) {
          if (fail) {
            const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            fl[cnt + r] = z[u];
            fl[kWL + cnt + r] = (unsigned)(e0 + u);
          }
          cnt = __builtin_amdgcn_readfirstlane(cnt + __popcll(m));
        }
      }
    }
  };
  int g0 = 0;
  for (bool first = true;; first = false) {
    const bool more = g0 < ng;  // (wave-uniform)
    if (!first) step2(cnt, !more);
    if (!more) break;
    if (!first) {
#pragma unroll
      for (int i = 0; i < kBPD; ++i) {
        zc[i] = wl4[(size_t)(g0 + i < ng ? g0 + i : ng - 1) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);  // (issued in order)
      }
    }
    int adv = 0;
#pragma unroll
    for (int i = 0; i < kBPD; ++i) {
      // insertw writes at the absolute index cnt, so the room is counted from
      // there, not from head: step2 returns with cnt + kRoom <= LS (it compacts
      // whenever head > 0 and that fails), so the group's first load always
      // fits, and a later one that might not waits for the next group
      if (g0 + i >= ng || cnt + kRoom > LS) break;
      insertw(zc[i], g0 + i);
      adv = i + 1;
    }
    g0 += adv;
  }
  } else {
  // ---- phase 1: the bound words, 8 points per lane per chunk ----
  // Groups of kBPD chunks issued together, phase 2 between groups.  The waits
  // must stay exact: vmcnt counts stores too and is in order, so a store or a
  // reload between a chunk's load and its use made the compiler wait for
  // every load in flight (a rebase is zh_rebase_kernel's).  A chunk whose
  // entries would not fit the list (dense failures: the first bounded step)
  // hands the rest of the wave's range to a plain loop, one chunk at a time,
  // phase 2 draining the list whenever it must.
  int cnt = 0;
  int it = 0;  // chunk ordinal within this wave's range (the entries' high bits)
  auto insert = [&](const u4v& z, int ci) __attribute__((always_inline)) {
    const unsigned enc = dyn ? (unsigned)(ci - ebase) : (unsigned)it;
    // the 8 thresholds from LDS (independent reads, one wait), then the
    // tests; entries only from chunks with a failed point
    unsigned fm = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned w = (z[u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
      fm |= (unsigned)((w >> 6) <= tls[w & 63u]) << u;
    }
#ifdef CDR_EXPERIMENTS
    if (B.dbg & 16) fm = 0;  // (timing: the stream alone)
#endif
    if (__ballot(fm != 0u)) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool fail = (fm >> u) & 1u;
        const unsigned long long m = __ballot(fail);
        if (m) {
          if (fail) {
            const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            fl[cnt + r] = enc << 15 | (unsigned)(8 * lane + u) << 6 |
                          ((z[u >> 1] >> (16 * (u & 1))) & 63u);
          }
          // (readfirstlane: uniform to the compiler, so the loops branch on
          // scalars and the waits stay exact)
          cnt = __builtin_amdgcn_readfirstlane(cnt + __popcll(m));
        }
      }
    }
    ++it;
  };
  // the group walk: chunks gC + i gS below gEnd (static: this wave's range;
  // then, with the dynamic tail, groups claimed from the region's pool)
  int gC = (int)wbase, gEnd = swend;
  bool dynph = false;
#define gS (dynph ? 1 : wstride)
  int ncl = -1;  // a claim made ahead: its pool offset (-1: none)
  // a wave claims while its near-tie region (a.cap points) holds the chunks
  // it may yet stream: the one in hand and the one claimed (the host sizes
  // the regions so the waves' budgets cover the pool)
#define budget (a.cap / CH - 2 * kBPD)
  auto claim = [&]() __attribute__((always_inline)) -> unsigned {
    unsigned v = 0;
    if (lane == 0)
      v = atomicAdd(B.dyn + ((B.dyn_par * 4 + rsl) * 8 + (blockIdx.x & 7)) * 32, (unsigned)kBPD);
    return v;
  };
  // the next group when the current phase is spent (uniform)
  auto next_group = [&]() __attribute__((always_inline)) -> bool {
    if (gC < gEnd) return true;
    if (!dyn) return false;
    dynph = true;
    if (ncl < 0) {
      if (it > budget) return false;
      ncl = (int)__builtin_amdgcn_readfirstlane(claim());
    }
    gC = P0 + ncl;
    ncl = -1;
    gEnd = gC + kBPD < P1 ? gC + kBPD : P1;
    return gC < gEnd;
  };
  int C0 = gC;
  bool dense = false;  // (wave-uniform) the plain loop takes over at chunk C0
  for (bool first = true;; first = false) {
    const bool more = next_group();  // (wave-uniform)
    // phase 2 first: the rows it gathers load under this group's stream, and
    // this group's loads are the youngest, so each chunk waits for itself
    // only (vmcnt(kBPD - 1 - i)) whatever phase 2 issued
#if CDR_S32BS_LAZY
    if (!first) step2(cnt, !more);
#else
    if (!first && (!more || cnt - head + CH > kSList - (kBPD - 1) * CH)) phase2(cnt, !more);
#endif
    if (!more) break;
#pragma unroll
    for (int i = 0; i < kBPD; ++i) {
      zload(zc[i], gC + i * gS);
      __builtin_amdgcn_sched_barrier(0);  // (issued in chunk order)
    }
    // the next dynamic group's claim, ahead of its use (returned under this
    // group's tests)
    const bool ahead = dyn && it <= budget && (dynph || gC + kBPD * gS >= gEnd);
    unsigned clv = 0;
    if (ahead) clv = claim();
#pragma unroll
    for (int i = 0; i < kBPD; ++i) {
      const int Ci = gC + i * gS;
      if (Ci >= gEnd) break;
      if (cnt - head + CH > kSList) {  // (dense failures only)
        dense = true;
        C0 = Ci;
        break;
      }
      insert(zc[i], Ci);
    }
    if (ahead) ncl = (int)__builtin_amdgcn_readfirstlane(clv);
    if (dense) break;
    gC = dynph ? gEnd : gC + kBPD * gS;
  }
  if (dense) {
    // the rest of the current group / phase one chunk at a time, then (the
    // dynamic tail) further claimed groups
    gC = C0;
    for (;;) {
      const bool more = next_group();
#if CDR_S32BS_LAZY
      if (!more || cnt - head + CH > kSList) step2(cnt, !more);  // (returns with room)
#else
      if (!more || cnt - head + CH > kSList) phase2(cnt, !more);
#endif
      if (!more) break;
      u4v z;
      zload(z, gC);
      insert(z, gC);
      gC += gS;
    }
  }
#undef gS
#undef budget
  }  // (!WATCH)
  }  // (!SPLIT)
  // ---- the uncertified points: the same split screen again (the same values),
  // every centroid whose key is within the threshold of the best is a
  // candidate (|S_j - T_j| <= E: the reference's argmin is among them), and
  // the candidates in exact fp64 NumPy order (fixup_regions' decision) from
  // an LDS copy of the step's centroids (the lists' LDS, free now) ----
  CDR_TP(2);
#ifdef CDR_EXPERIMENTS
  if (B.dbg & 2) fb_used = 0;  // (timing: no exact pass)
#endif
  if constexpr (DEFER) {
  // the next batch's records and rows load while one is decided
  // (Q >= 3: the records only - the rows ahead too spill registers)
  // (the WATCH form's records carry the entry's slot and the point's offset,
  // rec_x; its rows load with the record's batch, not ahead)
  constexpr int QA = Q < 3 && !WATCH ? Q : 0;
  auto tload = [&](int e0, int2& rec, f4 (&xr)[Q]) __attribute__((always_inline)) {
    const int e = e0 + lane;
    rec = fb_region[e < fb_used ? e : e0];
#pragma unroll
    for (int q = 0; q < QA; ++q) xr[q] = XA4[(int64_t)rec.x * Q + q];
  };
  int2 rec_n = {0, 0};
  f4 xr_n[Q];
  if (fb_used > 0) tload(0, rec_n, xr_n);
  for (int e0 = 0; e0 < fb_used; e0 += 64) {
    const int e = e0 + lane;
    const bool live = e < fb_used;
    const int2 rec = rec_n;
    f4 xr[Q];
#pragma unroll
    for (int q = 0; q < QA; ++q) xr[q] = xr_n[q];
    int pt = rec.x, sl = 0;
    if constexpr (WATCH) {  // (rec_x: unsigned halves)
      sl = (int)((unsigned)rec.x & 0xFFFFu);
      pt = pbase + (int)((unsigned)rec.x >> 16);
    }
#pragma unroll
    for (int q = QA; q < Q; ++q) xr[q] = XA4[(int64_t)pt * Q + q];
    if (e0 + 64 < fb_used) tload(e0 + 64, rec_n, xr_n);
    const int ao = rec.y & 63;  // (the record's: unchanged until this pass decides the point)
    float xh[DM];
    rowhat(xr, xh);
    u4v T0[QH], T1[QH];
    split_tiles(xh, T0, T1);
    const float xx = norm2(xh);
    // "not screened" records (the direct test's few undecided lanes): the
    // split screen and its certificate now, the K-case word for the
    // certified; the others join the near ties with their best key
    unsigned bkey = (unsigned)rec.y;
    const bool uns = live && (bkey & ~63u) == kNotScreened;
    bool tie = live;
    int lab = ao;
    if (__ballot(uns)) {
      unsigned bA, sA_;
      keys(T0, T1, bA, sA_);
      const float vb = __uint_as_float(bA & ~63u);
      const float vs = __uint_as_float(sA_ & ~63u);
      const bool cert = uns && vs > fmaf(vb, thr_rel, thr0);  // NaN: never certified
      const float w_c = __shfl(wnew_l, (int)(bA & 63u));
      if (uns) bkey = bA;
      if (cert) {
        float u0, l0;
        kcase(xx, vb, vs, u0, l0);
        lab = (int)(bA & 63u);
        zput(pt, sl, true, l0, u0, w_c, (unsigned)lab);
        tie = false;
      }
      fb_cert += __popcll(__ballot(cert));
    }
    const unsigned long long tm = __ballot(tie);
    if (tm) {
      bool c2;
      float u0, l0;
      const int lt = near_tie(tie, ao, bkey, xh, T0, T1, xr, xx, c2, u0, l0);
      const float w_lab = __shfl(wnew_l, lt);
      if (tie) {
        lab = lt;
        zput(pt, sl, c2, l0, u0, w_lab, (unsigned)lab);  // the direct bounds, or none
      }
    }
    move(live, pt, ao, lab, xr);
  }
  }  // DEFER
  CDR_TP(3);
  if (lane == 0) {
    a.fb_count[wave] = fb_used - fb_cert;  // the points no certificate decided
    a.mv_count[wave] = mv_used;
    if (a.q_acc) a.q_acc[wave] += qtot;
    if (B.t_acc) B.t_acc[wave] += ttot;
    if constexpr (!SPLIT)
      if (B.wf) B.wf[wave] = ttot;  // (cdr_lloyd_watch_info: the entries or words that failed)
  }
  // this workgroup's moves into one run_sums slice (nothing to do: no atomics)
  if (__syncthreads_or(mv_used)) {
    const int cells = k * d1;
    unsigned long long* out = F.run_sums + (size_t)(blockIdx.x % kRunSlices) * cells;
    for (int e = t; e < cells; e += 256) {
      const unsigned long long v = mtab[e];
      if (v) atomicAdd(&out[e], v);
    }
  }
#ifdef CDR_EXPERIMENTS
  CDR_TP(4);
  if (B.tprof && lane == 0)
    for (int q = 0; q < 8; ++q) B.tprof[(size_t)wave * 8 + q] = tp[q];
#endif
#undef CDR_TP
