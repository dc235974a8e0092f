// The similarity scan (included by ip_topk.hip after ip_prepare.hpp): ScanArgs, the row filter, the epilogues of the five
// modes (FULL, TOP2, EMIT, BAND, MARK), the two persistent scan kernels on the MFMA main loops of gemm_nt.hpp, and the
// launchers -- launch_scan<MODE>, launch_scan_band, launch_scan_mark -- every host pipeline calls.
#pragma once

namespace convdr {

// ------------------------------------------------------------------------------------------
// The scan GEMM.  A = passages (rows -> accumulator rows), B = queries (-> accumulator columns,
// one query per lane), so the per-query threshold lives in one VGPR per 32-column MFMA tile.
// Grid: 1-D, nPt * nQt blocks, XCD-remapped so the nQt query tiles of one passage tile run
// back-to-back on one XCD (the passage tile is fetched from HBM once, then hits that XCD's L2).
// ------------------------------------------------------------------------------------------
// One hit counter per 128-byte line.  The returning atomics that reserve candidate slots execute at the memory side and
// serialise per LINE: with the counters packed 32 to a line, 1,000 queries shared 32 lines and the ~1.6 M reservations of
// a 1 M-passage scan were 30 % of its time; one line per query spreads them over every channel.
constexpr int IP_COUNT_STRIDE = 32;

struct ScanArgs {
  const bf16_t* P;   // [n, d]
  const bf16_t* Qb;  // [nq_pad, d] (rows >= nq are zero)
  const bf16_t* Plo; // split-bf16 scan: remainders (nullptr = plain bf16 scan)
  const bf16_t* Qlo;
  int64_t n;
  int nq, nq_pad, d;
  int nPt, nQt;      // tiles actually visited / query tiles
  int pt_stride;     // visited passage tile t -> tile t * pt_stride
  const float* tau;  // EMIT: [nq_pad]
  uint32_t* counts;  // EMIT: [nq_pad * IP_COUNT_STRIDE], counter of query q at q * IP_COUNT_STRIDE
  uint32_t* cand_id; // EMIT: [nq, cap]
  float* cand_s;     // EMIT: [nq, cap]
  int cap;
  float* T;          // FULL: [nPt*128, nq_pad]; TOP2: [nPt*8, nq_pad]
  int two_pass;      // half store (fp16 only): S~ = P Qh + P Ql, the passage operand is exact and has no remainder copy
  const uint32_t* bits;  // row filter (FILT kernels only): row r is allowed iff bit r & 31 of word r >> 5 is set; padded with
                         // zero bits to whole TR-row tiles, word 0 = row 0 of P (a sub-block's pointer advances with its P)
  const float* tau_hi;   // BAND: [nq_pad], tau <= tau_hi: rows with S~ >= tau_hi are counted, not listed (tau is the band's lower end)
  uint32_t* above;       // BAND: [nq_pad * IP_COUNT_STRIDE], the count of query q at q * IP_COUNT_STRIDE, like counts
  const uint32_t* ord;   // MARK: [n], the dense document number of every row (convdr_doc_ordinals); >= ndocs: no document
  uint32_t* marks;       // MARK: [nq, mark_words], one bit per document and query: some row of it scored S~ >= tau_hi
  int64_t mark_words;    // MARK: words of one query's bitmap (>= ceil(ndocs / 32))
  int64_t ndocs;
  // Trace library only (trace_knobs.hpp; empty in the product).  prelanded: timing experiment, a tile's first K chunks are not
  // waited for (garbage results)
  [[no_unique_address]] TraceKnobs knobs;
};

// The row filter in the scan epilogues.  A wave's accumulator tile mt covers the 32 rows (wr * MT + mt) * 32 .. + 31 of the
// passage tile -- exactly ONE bitmap word, wave-uniform -- and register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5)
// of them.  filter_lane_words clears the bits of rows past the block's end (the caller's padding is not trusted: a set bit
// there would name a row that does not exist) and shifts by the lane's 4 * hi, so that the bit sits at a compile-time
// position.  THE RULE, in every mode: a row whose bit is clear never reserves a list slot, whatever tau is, and contributes
// -inf to a threshold sample.  filter_acc applies it to the accumulators in place, before the epilogue proper: a masked
// score becomes NaN in the emitting scan (NaN >= tau is false for EVERY tau; -inf would pass the no-threshold plans'
// tau = -inf and fill the list with masked rows) and -inf in the sampling modes.  Two VALU operations per accumulator (sign-
// extended bit field, bit select), no compare: the sweeps that follow are the unfiltered ones and hold no extra masks.
template <class T>
__device__ __forceinline__ void filter_lane_words(const uint32_t (&fw)[T::MT], const WavePos<T>& w, int rows_left,
                                                  uint32_t (&out)[T::MT]) {
#pragma unroll
  for (int mt = 0; mt < T::MT; ++mt) {
    const int left = rows_left - (w.wr * T::MT + mt) * 32;
    const uint32_t valid = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << left) - 1u : 0u);
    out[mt] = (fw[mt] & valid) >> (4 * w.hi);
  }
}
template <class T>
__device__ __forceinline__ void filter_acc(GemmAcc<T>& acc, const uint32_t (&fw)[T::MT], const WavePos<T>& w, int64_t rows_after_m0,
                                           uint32_t masked_bits) {
  uint32_t fl[T::MT];
  filter_lane_words<T>(fw, w, (int)(rows_after_m0 < (int64_t)T::TR ? rows_after_m0 : (int64_t)T::TR), fl);
#pragma unroll
  for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t m = (uint32_t)((int32_t)(fl[mt] << (31 - ((r & 3) + 8 * (r >> 2)))) >> 31);   // all ones iff allowed
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt)
        acc.c[mt][nt][r] = __uint_as_float((__float_as_uint(acc.c[mt][nt][r]) & m) | (masked_bits & ~m));
    }
}
constexpr uint32_t IP_MASKED_EMIT = 0xffffffffu;     // a NaN
constexpr uint32_t IP_MASKED_SAMPLE = 0xff800000u;   // -inf

template <int MODE, class T, bool FILT>
__device__ __forceinline__ void scan_epilogue(const ScanArgs& a, GemmAcc<T>& acc, const WavePos<T>& w, int ts, int64_t m0,
                                              int64_t n0, const float (&tau_lane)[T::NT], const uint32_t (&fw)[T::MT],
                                              const float (&tau_hi_lane)[T::NT]) {   // (tau_hi_lane: BAND only)
  constexpr bool MARK = MODE == IP_MODE_MARK;     // BAND plus one bit per document with a row above tau_hi (ip_docrank.hpp)
  constexpr bool LISTS = MODE == IP_MODE_EMIT || MODE == IP_MODE_BAND || MARK;
  if constexpr (FILT) filter_acc<T>(acc, fw, w, a.n - m0, LISTS ? IP_MASKED_EMIT : IP_MASKED_SAMPLE);
  if constexpr (MODE == IP_MODE_BAND || MARK) {
    // Two thresholds per query column, tau <= tau_hi.  S~ >= tau_hi: the row is COUNTED into the query's "above" counter and
    // nothing else -- no slot, no id.  tau <= S~ < tau_hi: the row is listed exactly as EMIT lists it (one returning atomic per
    // lane reserves the slots, the hits are written once it has retired, the hit counter counts past cap).  A masked score is
    // NaN and fails both compares; the rows past n of the last tile score -inf, and tau is never below -FLT_MAX.
    // How the above count leaves the registers: lanes l and l + 32 hold the same query column (the two halves of the 32 rows
    // of an accumulator tile), so the pair is folded in registers first (a cross-lane move: no LDS is allocated, the R3 main
    // loop owns all of it); then lanes 0..31 issue ONE non-returning 32-bit add per query tile into the query's counter, which
    // has a 128-byte line of its own.  Integer sums do not depend on the order of arrival: the count is the same in every run.
    const int rows_left = (int)(a.n - m0 < (int64_t)T::TR ? a.n - m0 : (int64_t)T::TR);
    if (!FILT && rows_left < T::TR) {
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (w.r_index(mt, r) >= rows_left) acc.c[mt][nt][r] = -INFINITY;
    }
    uint32_t cnt[T::NT], slot[T::NT];
    uint32_t mine_above[MARK ? T::NT : 1] = {};      // MARK: this lane's own share of the above count, per query column
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      uint32_t c = 0, ca = 0;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          c += acc.c[mt][nt][r] >= tau_lane[nt] ? 1u : 0u;
          ca += acc.c[mt][nt][r] >= tau_hi_lane[nt] ? 1u : 0u;
        }
      cnt[nt] = c - ca;          // (tau <= tau_hi: every row counted above also passed tau)
      if constexpr (MARK) mine_above[nt] = ca;
      const uint32_t pair = ca + (uint32_t)__shfl_xor((int)ca, 32, 64);
      const int q = (int)n0 + w.l_index(nt);
      if (w.hi == 0 && pair) __hip_atomic_fetch_add(&a.above[(int64_t)q * IP_COUNT_STRIDE], pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0 + w.l_index(nt);
      slot[nt] = cnt[nt] ? atomicAdd(&a.counts[(int64_t)q * IP_COUNT_STRIDE], cnt[nt]) : 0u;
    }
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(slot[nt]));   // hipcc: the reservations retire HERE, once (see EMIT)
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      if (cnt[nt] == 0) continue;
      const int q = (int)n0 + w.l_index(nt);
      const float tau = tau_lane[nt], tau_hi = tau_hi_lane[nt];
      uint32_t* ids = a.cand_id + (int64_t)q * a.cap;
      float* sc = a.cand_s + (int64_t)q * a.cap;
      uint32_t sl = slot[nt];
      const uint32_t row0 = (uint32_t)m0;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt) {
        const f32x16 v = acc.c[mt][nt];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (v[r] >= tau && !(v[r] >= tau_hi)) {
            if (sl < (uint32_t)a.cap) {
              ids[sl] = row0 + (uint32_t)w.r_index(mt, r);
              sc[sl] = v[r];
            }
            ++sl;
          }
        }
      }
    }
    if constexpr (MARK) {
      // The rows above tau_hi precede the target for certain: each ORs the bit of its DOCUMENT into the query's bitmap -- no
      // slot, no id, no re-score.  One dependent load (the row's ordinal) and one non-returning atomic per such row; lanes
      // that counted none skip the walk.  Nothing is stored for a row past the block's end, an ordinal that names no
      // document or a padding query column, whatever the thresholds are.  An OR is idempotent and commutative: the bitmap
      // is the same in every run.  No LDS (the R3 main loop owns all of it).
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt) {
        if (mine_above[nt] == 0) continue;
        const int q = (int)n0 + w.l_index(nt);
        if (q >= a.nq) continue;
        const float tau_hi = tau_hi_lane[nt];
        uint32_t* mk = a.marks + (int64_t)q * a.mark_words;
#pragma unroll
        for (int mt = 0; mt < T::MT; ++mt) {
          const f32x16 v = acc.c[mt][nt];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (v[r] >= tau_hi) {
              const int64_t row = m0 + w.r_index(mt, r);
              if (row < a.n) {
                const uint32_t o = a.ord[row];
                if ((int64_t)o < a.ndocs && (int64_t)(o >> 5) < a.mark_words)
                  __hip_atomic_fetch_or(&mk[o >> 5], 1u << (o & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
          }
        }
      }
    }
  } else if constexpr (MODE == IP_MODE_EMIT) {
    // A lane owns one query per 32-column tile and MT*16 of the tile's passages.  It counts its hits, reserves that
    // many slots of the query's candidate list with ONE atomic (a device-scope returning atomic is a ~1-2 us round
    // trip to the memory side; one per hit -- ~100 per tile, serialised by the branches around them -- was 30 % of
    // the scan), then writes the hits into consecutive slots.  The list order differs from run to run either way;
    // the downstream kernels do not depend on it.
    const int rows_left = (int)(a.n - m0 < (int64_t)T::TR ? a.n - m0 : (int64_t)T::TR);
    // the last passage tile: rows past n scored 0 (zero-filled operand) and must never hit (FILT: masked with the rest)
    if (!FILT && rows_left < T::TR) {
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (w.r_index(mt, r) >= rows_left) acc.c[mt][nt][r] = -INFINITY;
    }
    uint32_t cnt[T::NT], slot[T::NT];
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      uint32_t c = 0;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) c += acc.c[mt][nt][r] >= tau_lane[nt] ? 1u : 0u;
      cnt[nt] = c;
    }
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0 + w.l_index(nt);
      slot[nt] = cnt[nt] ? atomicAdd(&a.counts[(int64_t)q * IP_COUNT_STRIDE], cnt[nt]) : 0u;
    }
    // hipcc: retire the reservations HERE, once.  Left to the compiler, every hit below starts with s_waitcnt vmcnt(0)
    // (the slot might still be pending on the path that skipped the previous hit), which on gfx9 also waits for the
    // previous hit's STORES: a dozen serialised write round trips per wave per tile.
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(slot[nt]));
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      if (cnt[nt] == 0) continue;
      const int q = (int)n0 + w.l_index(nt);
      const float tau = tau_lane[nt];
      uint32_t* ids = a.cand_id + (int64_t)q * a.cap;
      float* sc = a.cand_s + (int64_t)q * a.cap;
      uint32_t sl = slot[nt];
      const uint32_t row0 = (uint32_t)m0;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt) {
        const f32x16 v = acc.c[mt][nt];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (v[r] >= tau) {
            if (sl < (uint32_t)a.cap) {
              ids[sl] = row0 + (uint32_t)w.r_index(mt, r);
              sc[sl] = v[r];
            }
            ++sl;
          }
        }
      }
    }
  } else if constexpr (MODE == IP_MODE_FULL) {
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0 + w.l_index(nt);
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = m0 + w.r_index(mt, r);
          a.T[row * a.nq_pad + q] = (FILT || row < a.n) ? acc.c[mt][nt][r] : -INFINITY;
        }
    }
  } else {  // TOP2: best two of this lane's MT*16 scores (one query, MT*16 of the tile's passages)
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0 + w.l_index(nt);
      float b0 = -INFINITY, b1 = -INFINITY;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = m0 + w.r_index(mt, r);
          const float s = (FILT || row < a.n) ? acc.c[mt][nt][r] : -INFINITY;
          const float lo = fminf(b0, s);
          b0 = fmaxf(b0, s);
          b1 = fmaxf(b1, lo);
        }
      const int64_t slot = (((int64_t)ts * T::WR + w.wr) * 2 + w.hi) * 2;
      a.T[slot * a.nq_pad + q] = b0;
      a.T[(slot + 1) * a.nq_pad + q] = b1;
    }
  }
}

// Persistent: one workgroup per resident slot walks a strided sequence of tiles (XCD x owns a contiguous chunk of the
// tile order, query tile fastest); the first K chunk of the next tile streams into the idle operand stage while the
// epilogue of this one runs, so neither the workgroup dispatch gap nor the cold HBM round trip for a fresh passage
// tile is exposed (they were ~40 % of a 12-step tile).
// PASSES: 1 = S~ = Ph Qh; 3 = the split scan Ph Qh + Ph Ql + Pl Qh; 2 = the half store's second rung P Qh + P Ql (the
// stored halves ARE the passages: there is no Pl).
// FILT: the row filter (a.bits).  A compile-time parameter, not a test on the pointer: the unfiltered instantiations are
// instruction for instruction the kernels they were before the filter existed.
template <int MODE, class T, int PASSES, bool F16, bool FILT>
__global__ void __launch_bounds__(T::THREADS, 2) k_ip_scan(const ScanArgs a) {
  static_assert(MODE != IP_MODE_BAND && MODE != IP_MODE_MARK, "the band-count scan is single pass: k_ip_scan_r3<..., IP_MODE_BAND>");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t ntiles = (uint32_t)a.nPt * (uint32_t)a.nQt;
  const uint32_t xcd = blockIdx.x & 7u, q8 = ntiles >> 3, r8 = ntiles & 7u;
  const uint32_t chunk_base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const uint32_t chunk_len = q8 + (xcd < r8 ? 1u : 0u);
  const uint32_t stride = (gridDim.x + 7u) >> 3;
  uint32_t idx = blockIdx.x >> 3;
  if (idx >= chunk_len) return;
  const WavePos<T> w;
  auto coords = [&](uint32_t i, int& ts, int64_t& m0, int64_t& n0) {
    const uint32_t logical = chunk_base + i;
    ts = (int)(logical / a.nQt);
    const int qt = (int)(logical - (uint32_t)ts * a.nQt);
    m0 = (int64_t)ts * a.pt_stride * T::TR;
    n0 = (int64_t)qt * T::TL;
  };
  int ts;
  int64_t m0, n0;
  coords(idx, ts, m0, n0);
  TileSrc<T> src(a.P, a.d, a.n, a.Qb, a.d, a.nq_pad, m0, n0, w);
  int buf = 0;
  gemm_issue_stage<T>(src, 0, smem + buf * T::STAGE_BYTES, w);
  // A tile's thresholds are loaded one tile ahead (loop-carried, so the load cannot be sunk to its use after the main
  // loop, where its full latency would be exposed) and are retired by the main loop's own waits; an ordinary load used
  // while the next tile's LDS-DMA is in flight would drain that too.
  float tau_next[T::NT];
  auto load_tau = [&](int64_t n0_) {
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0_ + w.l_index(nt);
      tau_next[nt] = (MODE == IP_MODE_EMIT && q < a.nq) ? a.tau[q] : INFINITY;
    }
  };
  load_tau(n0);
  // FILT: the tile's bitmap words -- the MT consecutive words of this wave's rows, one 16-byte load at a wave-uniform,
  // 16-byte aligned address (m0 is a multiple of TR) -- travel with the thresholds: loaded one tile ahead, retired by the
  // main loop's waits.  Strided TOP2 tiles index the bitmap by their own m0.
  uint32_t fw_next[T::MT] = {};
  auto load_bits = [&](int64_t m0_) {
    if constexpr (FILT) {
      static_assert(T::MT == 4, "one uint4 of bitmap words per wave");
      const uint4 v = *(const uint4*)(a.bits + (m0_ >> 5) + w.wr * T::MT);
      fw_next[0] = v.x; fw_next[1] = v.y; fw_next[2] = v.z; fw_next[3] = v.w;
    }
  };
  load_bits(m0);
  for (;;) {
    GemmAcc<T> acc;
    acc.zero();
    float tau_lane[T::NT];
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) tau_lane[nt] = tau_next[nt];
    uint32_t fw[T::MT];
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt) fw[mt] = fw_next[mt];
    int idle = gemm_nt_mainloop<T, F16>(src, a.d, smem, acc, w, buf, true);
    if constexpr (PASSES >= 2) {  // S~ = Ph Qh + Ph Ql + Pl Qh: fp32-class scores from three bf16 passes into the same accumulators
      __syncthreads();
      const TileSrc<T> s2(a.P, a.d, a.n, a.Qlo, a.d, a.nq_pad, m0, n0, w);
      idle = gemm_nt_mainloop<T, F16>(s2, a.d, smem, acc, w, idle);
      if constexpr (PASSES == 3) {
        __syncthreads();
        const TileSrc<T> s3(a.Plo, a.d, a.n, a.Qb, a.d, a.nq_pad, m0, n0, w);
        idle = gemm_nt_mainloop<T, F16>(s3, a.d, smem, acc, w, idle);
      }
    }
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(tau_lane[nt]));   // hipcc: the loads are retired HERE
    if constexpr (FILT) {
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt) asm volatile("" : "+v"(fw[mt]));
    }
    const uint32_t next = idx + stride;
    const bool has_next = next < chunk_len;
    const int ts_cur = ts;
    const int64_t m0_cur = m0, n0_cur = n0;
    if (has_next) {
      coords(next, ts, m0, n0);
      load_tau(n0);
      load_bits(m0);
      src = TileSrc<T>(a.P, a.d, a.n, a.Qb, a.d, a.nq_pad, m0, n0, w);
      gemm_issue_stage<T>(src, 0, smem + idle * T::STAGE_BYTES, w);
    }
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));   // opaque: the epilogue's lane-dependent addresses stay out of the main loop's registers
    const WavePos<T> we(tid_e);
    scan_epilogue<MODE, T, FILT>(a, acc, we, ts_cur, m0_cur, n0_cur, tau_lane, fw, tau_lane);
    if (!has_next) break;
    idx = next;
    buf = idle;
  }
}

// Emission with the slot reservation off the critical path (k_ip_scan_r3).  scan_epilogue<EMIT> counts a lane's hits,
// reserves their list slots with a returning atomic and has to WAIT for it (~1.5 us of a ~20 us tile, plus the counting
// sweep) before it can write them.  Here one sweep both counts and keeps a lane's first two hits in registers (hits
// are ~0.2 per lane and tile; a lane with more than two -- one in several thousand -- takes the old reserve-and-wait
// route for the rest), the reservation is issued and NOT waited for, and the two hits are written after the NEXT
// tile's main loop, by which time it has long returned.
template <class T>
struct EmitPending {
  uint32_t cnt[T::NT], slot[T::NT], id0[T::NT], id1[T::NT];
  float s0[T::NT], s1[T::NT];
  int64_t n0;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) { cnt[nt] = 0; slot[nt] = 0; id0[nt] = id1[nt] = 0; s0[nt] = s1[nt] = 0.f; }
    n0 = 0;
  }
};

template <class T, bool FILT>
__device__ __forceinline__ void scan_emit_capture(const ScanArgs& a, GemmAcc<T>& acc, const WavePos<T>& w, int64_t m0, int64_t n0,
                                                  const float (&tau_lane)[T::NT], EmitPending<T>& pd,
                                                  const uint32_t (&fw)[T::MT]) {
  const int rows_left = (int)(a.n - m0 < (int64_t)T::TR ? a.n - m0 : (int64_t)T::TR);
  if constexpr (FILT) filter_acc<T>(acc, fw, w, a.n - m0, IP_MASKED_EMIT);   // masked rows and rows past n: NaN, never a hit
  if (!FILT && rows_left < T::TR) {   // the last passage tile: rows past n scored 0 (zero-filled operand) and must never hit
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (w.r_index(mt, r) >= rows_left) acc.c[mt][nt][r] = -INFINITY;
  }
  const uint32_t row0 = (uint32_t)m0;
  pd.n0 = n0;
  // per accumulator register: one compare and one wave-uniform branch when no lane hits (9 registers in 10); the
  // capture itself is predicated, not branched (nested divergent branches cost hipcc an exec-mask stack in SGPR spills)
#pragma unroll
  for (int nt = 0; nt < T::NT; ++nt) {
    const float tau = tau_lane[nt];
    uint32_t c = 0, i0 = 0, i1 = 0;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt) {
      const f32x16 v = acc.c[mt][nt];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool hit = v[r] >= tau;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit) != 0ull, 0)) {
          const uint32_t id = row0 + (uint32_t)w.r_index(mt, r);
          const bool f0 = hit && c == 0, f1 = hit && c == 1;
          s0 = f0 ? v[r] : s0; i0 = f0 ? id : i0;
          s1 = f1 ? v[r] : s1; i1 = f1 ? id : i1;
          c += hit ? 1u : 0u;
        }
      }
    }
    pd.cnt[nt] = c; pd.id0[nt] = i0; pd.id1[nt] = i1; pd.s0[nt] = s0; pd.s1[nt] = s1;
  }
#pragma unroll
  for (int nt = 0; nt < T::NT; ++nt) {
    const int q = (int)n0 + w.l_index(nt);
    pd.slot[nt] = pd.cnt[nt] ? atomicAdd(&a.counts[(int64_t)q * IP_COUNT_STRIDE], pd.cnt[nt]) : 0u;
  }
#pragma unroll
  for (int nt = 0; nt < T::NT; ++nt) {
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(pd.cnt[nt] > 2) == 0ull, 1)) continue;   // no lane of the wave overflowed
    asm volatile("" : "+v"(pd.slot[nt]));   // hipcc: wait for the reservation once, not in front of every store
    const int q = (int)n0 + w.l_index(nt);
    float tau = tau_lane[nt];
    asm volatile("" : "+v"(tau));   // opaque copy: or hipcc keeps all 128 compare masks of the sweep above alive (in spilled SGPRs) for this one
    uint32_t* ids = a.cand_id + (int64_t)q * a.cap;
    float* sc = a.cand_s + (int64_t)q * a.cap;
    uint32_t k = 0;
    const uint32_t base = pd.slot[nt];
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt) {
      const f32x16 v = acc.c[mt][nt];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool hit = v[r] >= tau;
        if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
          if (hit && k >= 2 && base + k < (uint32_t)a.cap) {
            ids[base + k] = row0 + (uint32_t)w.r_index(mt, r);
            sc[base + k] = v[r];
          }
          k += hit ? 1u : 0u;
        }
      }
    }
  }
}

template <class T>
__device__ __forceinline__ void scan_emit_flush(const ScanArgs& a, const WavePos<T>& w, EmitPending<T>& pd) {
  // hipcc: retire the reservations HERE, once (nothing else is in flight at the two call sites)
#pragma unroll
  for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(pd.slot[nt]));
#pragma unroll
  for (int nt = 0; nt < T::NT; ++nt) {
    if (pd.cnt[nt] == 0) continue;
    const int q = (int)pd.n0 + w.l_index(nt);
    uint32_t* ids = a.cand_id + (int64_t)q * a.cap;
    float* sc = a.cand_s + (int64_t)q * a.cap;
    const uint32_t sl = pd.slot[nt];
    if (sl < (uint32_t)a.cap) { ids[sl] = pd.id0[nt]; sc[sl] = pd.s0[nt]; }
    if (pd.cnt[nt] > 1 && sl + 1 < (uint32_t)a.cap) { ids[sl + 1] = pd.id1[nt]; sc[sl + 1] = pd.s1[nt]; }
    pd.cnt[nt] = 0;
  }
}

// The emitting scan of 256 x 256 tiles on the 3 R-slot / 2 L-slot main loop (gemm_nt_mainloop_r3); same persistent walk,
// next-tile prologue under the epilogue and one-tile-ahead thresholds as k_ip_scan.  (The split-bf16 scan and the
// sampling modes stay on the two-stage loop.)
// MODE: IP_MODE_EMIT (the default: every caller before the band-count scan), or IP_MODE_BAND -- the same walk with
// scan_epilogue<IP_MODE_BAND> in the place of capture / flush: the band's slots are reserved and waited for in the epilogue
// (the list holds the few rows in doubt; the rows above are counted, not listed), and tau_hi travels with tau.  IP_MODE_MARK
// is BAND with scan_epilogue<IP_MODE_MARK>: the rows above also mark their document (document rank, ip_docrank.hpp).
template <class T, bool F16, bool FILT, int MODE = IP_MODE_EMIT>
__global__ void __launch_bounds__(T::THREADS, 2) k_ip_scan_r3(const ScanArgs a) {
  static_assert(MODE == IP_MODE_EMIT || MODE == IP_MODE_BAND || MODE == IP_MODE_MARK, "the R3 scan lists: EMIT, BAND or MARK");
  constexpr bool BAND = MODE == IP_MODE_BAND || MODE == IP_MODE_MARK;      // two thresholds, the epilogue of the band
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the 256 x 128 tile serves scans with ONE query tile (at most 128 queries): every passage chunk is read exactly once,
  // so its DMA is non-temporal -- the block streams past L2 instead of through it
  constexpr int P_AUX = T::TL <= 128 ? 2 : 0;
  const uint32_t ntiles = (uint32_t)a.nPt * (uint32_t)a.nQt;
  const uint32_t xcd = blockIdx.x & 7u, q8 = ntiles >> 3, r8 = ntiles & 7u;
  const uint32_t chunk_base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const uint32_t chunk_len = q8 + (xcd < r8 ? 1u : 0u);
  const uint32_t stride = (gridDim.x + 7u) >> 3;
  uint32_t idx = blockIdx.x >> 3;
  if (idx >= chunk_len) return;
  const WavePos<T> w;
  auto coords = [&](uint32_t i, int& ts, int64_t& m0, int64_t& n0) {
    const uint32_t logical = chunk_base + i;
    ts = (int)(logical / a.nQt);
    const int qt = (int)(logical - (uint32_t)ts * a.nQt);
    m0 = (int64_t)ts * a.pt_stride * T::TR;
    n0 = (int64_t)qt * T::TL;
  };
  int ts;
  int64_t m0, n0;
  coords(idx, ts, m0, n0);
  TileSrcAll<T> src(a.P, a.d, a.n, a.Qb, a.d, a.nq_pad, m0, n0, w);
  R3Slots slots{0, 0};
  gemm_r3_prologue<T, P_AUX>(src, a.d, smem, w, slots);
  float tau_next[T::NT];
  float tau_hi_next[BAND ? T::NT : 1] = {};   // BAND: the upper thresholds, one tile ahead like tau
  auto load_tau = [&](int64_t n0_) {
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) {
      const int q = (int)n0_ + w.l_index(nt);
      tau_next[nt] = q < a.nq ? a.tau[q] : INFINITY;
      if constexpr (BAND) tau_hi_next[nt] = q < a.nq ? a.tau_hi[q] : INFINITY;
    }
  };
  load_tau(n0);
  uint32_t fw_next[T::MT] = {};   // FILT: the tile's bitmap words, one tile ahead like the thresholds (see k_ip_scan)
  auto load_bits = [&](int64_t m0_) {
    if constexpr (FILT) {
      static_assert(T::MT == 4, "one uint4 of bitmap words per wave");
      const uint4 v = *(const uint4*)(a.bits + (m0_ >> 5) + w.wr * T::MT);
      fw_next[0] = v.x; fw_next[1] = v.y; fw_next[2] = v.z; fw_next[3] = v.w;
    }
  };
  load_bits(m0);
  EmitPending<T> pend;
  if constexpr (!BAND) pend.clear();
  for (;;) {
    GemmAcc<T> acc;
    acc.zero();
    float tau_lane[T::NT];
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) tau_lane[nt] = tau_next[nt];
    float tau_hi_lane[T::NT] = {};
    if constexpr (BAND) {
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt) tau_hi_lane[nt] = tau_hi_next[nt];
    }
    uint32_t fw[T::MT];
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt) fw[mt] = fw_next[mt];
    slots = gemm_nt_mainloop_r3<T, F16, P_AUX>(src, a.d, smem, acc, w, slots, true, false, a.knobs.prelanded() != 0);
#pragma unroll
    for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(tau_lane[nt]));
    if constexpr (BAND) {
#pragma unroll
      for (int nt = 0; nt < T::NT; ++nt) asm volatile("" : "+v"(tau_hi_lane[nt]));
    }
    if constexpr (FILT) {
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt) asm volatile("" : "+v"(fw[mt]));
    }
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const WavePos<T> we(tid_e);
    if constexpr (!BAND) scan_emit_flush<T>(a, we, pend);   // the previous tile's hits: their reservations came back under this main loop
    const uint32_t next = idx + stride;
    const bool has_next = next < chunk_len;
    const int64_t m0_cur = m0, n0_cur = n0;
    if (has_next) {
      coords(next, ts, m0, n0);
      load_tau(n0);
      load_bits(m0);
      src = TileSrcAll<T>(a.P, a.d, a.n, a.Qb, a.d, a.nq_pad, m0, n0, w);
      gemm_r3_prologue<T, P_AUX>(src, a.d, smem, w, slots);
    }
    if constexpr (BAND) scan_epilogue<MODE, T, FILT>(a, acc, we, 0, m0_cur, n0_cur, tau_lane, fw, tau_hi_lane);
    else scan_emit_capture<T, FILT>(a, acc, we, m0_cur, n0_cur, tau_lane, pend, fw);
    if (!has_next) break;
    idx = next;
  }
  if constexpr (!BAND) scan_emit_flush<T>(a, w, pend);
}

// ------------------------------------------------------------------------------------------
// the scan launcher: one entry, launch_scan<MODE>, for every caller (the host pipelines follow in ip_host.hpp)
// ------------------------------------------------------------------------------------------
constexpr int IP_TILE_256 = 1, IP_TILE_TALL = 2;   // scan tile classes (IpPlanHead::big)

template <int MODE, class T, int PASSES, bool F16, bool FILT>
static int launch_scan_x(const ScanArgs& a, hipStream_t st) {
  const unsigned tiles = (unsigned)a.nPt * (unsigned)a.nQt;
  if constexpr (MODE == IP_MODE_EMIT && PASSES == 1) {   // the two-stage loop
    constexpr int R3_SMEM = 3 * T::R_BYTES + 2 * T::L_BYTES;
    static DeviceOnce attr3;  // > 48 KB dynamic LDS needs the opt-in once per kernel and device
    if (attr3.first())
      CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_scan_r3<T, F16, FILT>, hipFuncAttributeMaxDynamicSharedMemorySize, R3_SMEM));
    ScanArgs b = a;
#ifdef CONVDR_ENABLE_TRACE   // timing only (every threshold = +inf: results are garbage): `make TRACE=1` library only
    if (getenv("CONVDR_DBG_SCAN_NOEMIT")) b.nq = 0;
    if (getenv("CONVDR_DBG_PRELANDED")) b.knobs.v_prelanded = 1;
#endif
    ProfScope prof("ip_scan_emit", st);
    hipLaunchKernelGGL((k_ip_scan_r3<T, F16, FILT>), dim3(std::min(tiles, (unsigned)device_cu_count())), dim3(T::THREADS), R3_SMEM, st, b);
    CONVDR_CHECK_LAUNCH("k_ip_scan_r3");
  } else {
    static DeviceOnce attr_done;
    if (attr_done.first())
      CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_scan<MODE, T, PASSES, F16, FILT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           T::SMEM_BYTES));
    const unsigned slots = (unsigned)device_cu_count() * (T::SMEM_BYTES > 80 * 1024 ? 1u : 2u);
    const unsigned grid = std::min(tiles, slots);
    ProfScope prof(MODE == IP_MODE_EMIT ? "ip_scan_emit" : "ip_scan_sample", st);
    ScanArgs b = a;
#ifdef CONVDR_ENABLE_TRACE
    static const bool no_emit = getenv("CONVDR_DBG_SCAN_NOEMIT") != nullptr;   // timing only: every threshold = +inf
    if (no_emit) b.nq = 0;
#endif
    hipLaunchKernelGGL((k_ip_scan<MODE, T, PASSES, F16, FILT>), dim3(grid), dim3(T::THREADS), T::SMEM_BYTES, st, b);
    CONVDR_CHECK_LAUNCH("k_ip_scan");
  }
  return 0;
}

template <int MODE, class T, bool F16, bool FILT>
static int launch_scan_t(const ScanArgs& a, hipStream_t st) {
  if (a.two_pass) {
    if constexpr (F16) return launch_scan_x<MODE, T, 2, F16, FILT>(a, st);
    CONVDR_REQUIRE(false, "convdr_ip_search: the two-pass scan exists for fp16 only");
  }
  return a.Plo ? launch_scan_x<MODE, T, 3, F16, FILT>(a, st) : launch_scan_x<MODE, T, 1, F16, FILT>(a, st);
}

template <int MODE, bool F16, bool FILT>
static int launch_scan_k(const ScanArgs& a, int tile, hipStream_t st) {
  if (tile == IP_TILE_256) return launch_scan_t<MODE, Tile256, F16, FILT>(a, st);
  return launch_scan_t<MODE, TileTall, F16, FILT>(a, st);
}
template <int MODE, bool FILT>
static int launch_scan_f(const ScanArgs& a, int tile, int kind, hipStream_t st) {
  return kind == IP_KIND_F16 ? launch_scan_k<MODE, true, FILT>(a, tile, st) : launch_scan_k<MODE, false, FILT>(a, tile, st);
}
template <int MODE>
static int launch_scan_q8(const ScanArgs& a, hipStream_t st);   // the 8-bit store's integer scan (ip_scan_q8.hpp)
template <int MODE>
static int launch_scan(const ScanArgs& a, int tile, int kind, hipStream_t st) {   // a.bits selects the filtered kernels
  if (kind == IP_KIND_I8) return launch_scan_q8<MODE>(a, st);
  return a.bits ? launch_scan_f<MODE, true>(a, tile, kind, st) : launch_scan_f<MODE, false>(a, tile, kind, st);
}

// The band-count scan (IP_MODE_BAND): the single-pass shapes of launch_scan<IP_MODE_EMIT> -- both tiles, both kinds (the half
// store scans with the fp16 kernels), with and without the row filter -- on the R3 kernel.  There is no split BAND scan.
// MODE: IP_MODE_BAND, or IP_MODE_MARK -- the same eight shapes with the marking epilogue (launch_scan_mark).
template <class T, bool F16, bool FILT, int MODE>
static int launch_band_x(const ScanArgs& a, hipStream_t st) {
  constexpr int R3_SMEM = 3 * T::R_BYTES + 2 * T::L_BYTES;
  static DeviceOnce attr3;
  if (attr3.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_scan_r3<T, F16, FILT, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         R3_SMEM));
  const unsigned tiles = (unsigned)a.nPt * (unsigned)a.nQt;
  ProfScope prof(MODE == IP_MODE_MARK ? "ip_scan_mark" : "ip_scan_band", st);
  hipLaunchKernelGGL((k_ip_scan_r3<T, F16, FILT, MODE>), dim3(std::min(tiles, (unsigned)device_cu_count())), dim3(T::THREADS),
                     R3_SMEM, st, a);
  if constexpr (MODE == IP_MODE_MARK) CONVDR_CHECK_LAUNCH("k_ip_scan_r3<MARK>");
  else CONVDR_CHECK_LAUNCH("k_ip_scan_r3<BAND>");
  return 0;
}
template <bool F16, bool FILT, int MODE>
static int launch_band_k(const ScanArgs& a, int tile, hipStream_t st) {
  return tile == IP_TILE_256 ? launch_band_x<Tile256, F16, FILT, MODE>(a, st) : launch_band_x<TileTall, F16, FILT, MODE>(a, st);
}
template <int MODE>
static int launch_band_m(const ScanArgs& a, int tile, int kind, hipStream_t st) {   // a.bits selects the filtered kernels
  if (kind == IP_KIND_F16) return a.bits ? launch_band_k<true, true, MODE>(a, tile, st) : launch_band_k<true, false, MODE>(a, tile, st);
  return a.bits ? launch_band_k<false, true, MODE>(a, tile, st) : launch_band_k<false, false, MODE>(a, tile, st);
}
static int launch_scan_band(const ScanArgs& a, int tile, int kind, hipStream_t st) {
  CONVDR_REQUIRE(!a.two_pass && !a.Plo && a.tau_hi && a.above, "band scan: one pass, tau_hi and above set");
  return launch_band_m<IP_MODE_BAND>(a, tile, kind, st);
}
// The marking scan (IP_MODE_MARK): the band scan whose rows above tau_hi also OR their document's bit into a.marks.
static int launch_scan_mark(const ScanArgs& a, int tile, int kind, hipStream_t st) {
  CONVDR_REQUIRE(!a.two_pass && !a.Plo && a.tau_hi && a.above, "mark scan: one pass, tau_hi and above set");
  CONVDR_REQUIRE(a.ord && a.ndocs >= 0 && a.ndocs <= a.n && a.mark_words * 32 >= a.ndocs && (a.marks || a.ndocs == 0),
                 "mark scan: ord, marks and mark_words must cover ndocs=%lld documents", (long long)a.ndocs);
  return launch_band_m<IP_MODE_MARK>(a, tile, kind, st);
}

}  // namespace convdr
