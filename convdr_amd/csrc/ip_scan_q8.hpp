// The scan of the 8-bit store (included by ip_topk.hip after ip_scan.hpp): int8 code rows against int8 query operands on
// v_mfma_i32_32x32x32_i8, through the R3 K step of gemm_nt.hpp with integer accumulators, into the UNCHANGED epilogues of
// ip_scan.hpp (FULL, TOP2, EMIT; the row filter).
//
// One geometry serves every query count.  A query is two int8 operands, Qi = 128 hi + lo (k_q8_queries), and the MFMA tile is
// Tile256: 256 code rows x 256 operand rows = 128 QUERIES x {hi, lo}, interleaved so that the two 32-column tiles of a wave
// (nt = 0, 1) are hi and lo of the same 32 queries.  A passage K chunk is therefore staged ONCE for both operands -- with at
// most 128 queries the scan streams every code byte exactly once, non-temporal, as TileTall does for 16-bit rows -- and a
// lane holds S_hi and S_lo of its query side by side.  After the main loop
//     S = 128 S_hi + S_lo,   S~ = (float)S
// is formed in registers, and what remains is a 256 x 128 accumulator tile with TileTall's element map (same WR, WL, MT; NT = 1),
// which scan_epilogue / scan_emit_capture / scan_emit_flush take as they are.  More than 128 queries are further query tiles
// of 128 (the L2 -> LDS bytes per query-passage pair are those of a two-pass 256 x 256 tile: P once + 256 operand rows per
// 128 queries, against P twice + 512 per 256).
//
// Integer range, d <= 1024 (IP_Q8_MAX_D; the entries check it): |c| <= 127, |hi| <= 127, |lo| <= 64, |Qi| <= 16256, so
//     |S_hi| <= 1024 x 127 x 127 = 16,516,096,   128 |S_hi| <= 2,114,060,288 < 2^31,   |S_lo| <= 1024 x 127 x 64 = 8,323,072,
// and 128 S_hi + S_lo = sum_j Qi_j c_ij has |S| <= 1024 x 127 x 16256 = 2,114,060,288 < 2^31 = 2,147,483,648: the MFMA's int32
// accumulators, the multiplication by 128 and the final sum are all exact.  The conversion to float rounds above 2^24; the
// band carries it (IP_Q8_COEF, ip_topk.hip).
#pragma once

namespace convdr {

// MODE: IP_MODE_EMIT (capture / flush, as k_ip_scan_r3), IP_MODE_FULL or IP_MODE_TOP2 (scan_epilogue).  STREAM: one query
// tile -- the code rows are read once, their DMA is non-temporal.  a.d is the row length in 16-bit words (d / 2), a.Qb the
// interleaved operand [2 nq_pad, d] int8, a.nQt the query tiles of 128; everything else as for k_ip_scan_r3.
template <int MODE, bool FILT, bool STREAM>
__global__ void __launch_bounds__(Tile256::THREADS, 2) k_ip_scan_q8(const ScanArgs a) {
  static_assert(MODE == IP_MODE_EMIT || MODE == IP_MODE_FULL || MODE == IP_MODE_TOP2, "the 8-bit scan emits or samples");
  using G = Tile256;     // the MFMA tile
  using E = TileTall;    // the tile the epilogues see
  static_assert(G::WR == E::WR && G::WL == E::WL && G::MT == E::MT && G::NT == 2 && E::NT == 1 && G::TL == 2 * E::TL,
                "hi / lo column tiles of one wave fold into one TileTall column tile");
  constexpr bool EMIT = MODE == IP_MODE_EMIT;
  constexpr int P_AUX = STREAM ? 2 : 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t ntiles = (uint32_t)a.nPt * (uint32_t)a.nQt;
  const uint32_t xcd = blockIdx.x & 7u, q8 = ntiles >> 3, r8 = ntiles & 7u;
  const uint32_t chunk_base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const uint32_t chunk_len = q8 + (xcd < r8 ? 1u : 0u);
  const uint32_t stride = (gridDim.x + 7u) >> 3;
  uint32_t idx = blockIdx.x >> 3;
  if (idx >= chunk_len) return;
  const WavePos<G> w;
  const int64_t nL = 2 * (int64_t)a.nq_pad;      // operand rows
  auto coords = [&](uint32_t i, int& ts, int64_t& m0, int64_t& n0) {
    const uint32_t logical = chunk_base + i;
    ts = (int)(logical / a.nQt);
    const int qt = (int)(logical - (uint32_t)ts * a.nQt);
    m0 = (int64_t)ts * a.pt_stride * G::TR;
    n0 = (int64_t)qt * E::TL;                    // first QUERY of the tile; its operand rows begin at 2 n0
  };
  int ts;
  int64_t m0, n0;
  coords(idx, ts, m0, n0);
  TileSrcAll<G> src(a.P, a.d, a.n, a.Qb, a.d, nL, m0, 2 * n0, w);
  R3Slots slots{0, 0};
  gemm_r3_prologue<G, P_AUX>(src, a.d, smem, w, slots);
  // thresholds and bitmap words one tile ahead, retired by the main loop's waits (see k_ip_scan)
  float tau_next[E::NT];
  auto load_tau = [&](int64_t n0_) {
    const int q = (int)n0_ + w.wl * 32 + w.li;   // = WavePos<E>::l_index(0)
    tau_next[0] = (EMIT && q < a.nq) ? a.tau[q] : INFINITY;
  };
  load_tau(n0);
  uint32_t fw_next[E::MT] = {};
  auto load_bits = [&](int64_t m0_) {
    if constexpr (FILT) {
      static_assert(E::MT == 4, "one uint4 of bitmap words per wave");
      const uint4 v = *(const uint4*)(a.bits + (m0_ >> 5) + w.wr * E::MT);
      fw_next[0] = v.x; fw_next[1] = v.y; fw_next[2] = v.z; fw_next[3] = v.w;
    }
  };
  load_bits(m0);
  EmitPending<E> pend;
  if constexpr (EMIT) pend.clear();
  for (;;) {
    GemmAccI8<G> acc;
    acc.zero();
    float tau_lane[E::NT] = {tau_next[0]};
    uint32_t fw[E::MT];
#pragma unroll
    for (int mt = 0; mt < E::MT; ++mt) fw[mt] = fw_next[mt];
    slots = gemm_nt_mainloop_r3<G, false, P_AUX>(src, a.d, smem, acc, w, slots, true);
    asm volatile("" : "+v"(tau_lane[0]));   // hipcc: the loads are retired HERE
    if constexpr (FILT) {
#pragma unroll
      for (int mt = 0; mt < E::MT; ++mt) asm volatile("" : "+v"(fw[mt]));
    }
    // S~ = (float)(128 S_hi + S_lo): exact integers (range: head of this file), one rounding in the conversion
    GemmAcc<E> f;
#pragma unroll
    for (int mt = 0; mt < E::MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) f.c[mt][0][r] = (float)(acc.c[mt][0][r] * 128 + acc.c[mt][1][r]);
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const WavePos<E> we(tid_e);
    if constexpr (EMIT) scan_emit_flush<E>(a, we, pend);
    const uint32_t next = idx + stride;
    const bool has_next = next < chunk_len;
    const int ts_cur = ts;
    const int64_t m0_cur = m0, n0_cur = n0;
    if (has_next) {
      coords(next, ts, m0, n0);
      load_tau(n0);
      load_bits(m0);
      src = TileSrcAll<G>(a.P, a.d, a.n, a.Qb, a.d, nL, m0, 2 * n0, w);
      gemm_r3_prologue<G, P_AUX>(src, a.d, smem, w, slots);
    }
    if constexpr (EMIT) scan_emit_capture<E, FILT>(a, f, we, m0_cur, n0_cur, tau_lane, pend, fw);
    else scan_epilogue<MODE, E, FILT>(a, f, we, ts_cur, m0_cur, n0_cur, tau_lane, fw, tau_lane);
    if (!has_next) break;
    idx = next;
  }
  if constexpr (EMIT) {
    const WavePos<E> we;
    scan_emit_flush<E>(a, we, pend);
  }
}

template <int MODE, bool FILT, bool STREAM>
static int launch_scan_q8_x(const ScanArgs& a, hipStream_t st) {
  constexpr int R3_SMEM = 3 * Tile256::R_BYTES + 2 * Tile256::L_BYTES;
  static DeviceOnce attr;  // > 48 KB dynamic LDS needs the opt-in once per kernel and device
  if (attr.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_scan_q8<MODE, FILT, STREAM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         R3_SMEM));
  const unsigned tiles = (unsigned)a.nPt * (unsigned)a.nQt;
  ProfScope prof(MODE == IP_MODE_EMIT ? "ip_scan_emit" : "ip_scan_sample", st);
  hipLaunchKernelGGL((k_ip_scan_q8<MODE, FILT, STREAM>), dim3(std::min(tiles, (unsigned)device_cu_count())), dim3(Tile256::THREADS),
                     R3_SMEM, st, a);
  CONVDR_CHECK_LAUNCH("k_ip_scan_q8");
  return 0;
}

template <int MODE>
static int launch_scan_q8(const ScanArgs& a, hipStream_t st) {   // a.bits selects the filtered kernels
  CONVDR_REQUIRE(!a.Plo && !a.Qlo && !a.two_pass && a.d % 64 == 0 && a.nQt * 128 <= a.nq_pad,
                 "8-bit scan: rows of d %% 128 == 0 codes, one operand of interleaved hi / lo rows");
  if (a.nPt <= 0 || a.nQt <= 0) return 0;
  if (a.bits) return a.nQt == 1 ? launch_scan_q8_x<MODE, true, true>(a, st) : launch_scan_q8_x<MODE, true, false>(a, st);
  return a.nQt == 1 ? launch_scan_q8_x<MODE, false, true>(a, st) : launch_scan_q8_x<MODE, false, false>(a, st);
}

}  // namespace convdr
