// Deep candidate lists: exact top-k for 4,096 < k <= 65,536 (included by ip_topk.hip, after the kernels it mirrors).
//
// The shallow finish (k_ip_cut / k_ip_select / k_ip_finish) holds a query's candidate list and its re-scored band in LDS,
// which ends at 8,192 entries.  Here the same three phases run through global memory, one workgroup per query:
//   k_ip_cut_deep     radix select of S~(k) with the list left in global memory (four passes over it), the eps and the
//                     verdict of k_ip_cut (ip_certify.hpp), the band compacted into a SECOND pair of arrays
//   k_ip_rescore      unchanged (it always worked on a band in global memory, for any cap)
//   k_ip_select_deep  radix select of the k-th exact score on the high key word, survivors compacted into a third
//                     array, ordered by a tiled bitonic network, D / I written with FAISS padding
// and the threshold comes from COMPLETE scores of a row sample (k_tau_select_deep), because the TOP2 sample of the shallow
// plan keeps two scores per 64 rows and cannot represent a rank above n / 128.
// The certificate is k_ip_cut's (the proof is above that kernel): it never depended on where the list lives.
#pragma once

namespace convdr {

constexpr int IP_DEEP_THREADS = 1024;
constexpr int IP_DEEP_TILE = 4096;             // pairs ordered in LDS at a time: 4096 x (8 + 4) bytes = 48 KB
constexpr int IP_DEEP_SAMPLE_RANK = 512;       // expected rank of the threshold inside the row sample (see ip_deep_plan)
constexpr int IP_DEEP_SAMPLE_SEGMENTS = 16;    // the sample is this many evenly spaced runs of whole passage tiles

// Appends the lanes with `hit` to a list whose length lives in LDS: one atomic per wave (ballot + prefix), not one per
// element.  Every lane of the wave must call it.  The slots differ from run to run; nothing downstream depends on them.
__device__ __forceinline__ uint32_t wave_append_slot(bool hit, uint32_t* counter) {
  const uint64_t mask = __ballot(hit);
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == 0 && mask) base = atomicAdd(counter, (uint32_t)__popcll(mask));
  base = __shfl(base, 0, 64);
  return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// tau[q] = r-th largest of column q of T[0..nvals) -- k_tau_select with the column left in global memory (its LDS form
// ends at 32,768 values): four histogram passes over the column.
__global__ void __launch_bounds__(IP_DEEP_THREADS) k_tau_select_deep(const float* __restrict__ T, int nvals, int nq_pad, int r,
                                                                     float* __restrict__ tau) {
  __shared__ SelectScratch sc;
  const int q = blockIdx.x;
  if (r < 1 || r > nvals) {
    if (threadIdx.x == 0) tau[q] = -INFINITY;
    return;
  }
  const uint32_t kk = (uint32_t)block_kth_largest<32>(
      [&](int i) { return (uint64_t)f32_order_key(T[(int64_t)i * nq_pad + q]); }, nvals, (uint32_t)r, sc);
  if (threadIdx.x == 0) tau[q] = f32_from_order_key(kk);
}

// k_ip_cut over a list in global memory.  list_* [nq, cap] is what the emitting scan wrote (read only here), band_id
// [nq, cap] receives the ids of {S~ >= cut} in no particular order, m_out[q] their number.
__global__ void __launch_bounds__(IP_DEEP_THREADS) k_ip_cut_deep(int64_t n, int k, int cap, const uint32_t* __restrict__ counts,
                                                                 uint32_t* __restrict__ counts_packed,
                                                                 const uint32_t* __restrict__ list_id,
                                                                 const float* __restrict__ list_s,
                                                                 uint32_t* __restrict__ band_id,
                                                                 const float* __restrict__ tau, const IpBand band,
                                                                 uint32_t* __restrict__ m_out, int32_t* __restrict__ status,
                                                                 float* __restrict__ tau_retry) {
  __shared__ SelectScratch sc;
  __shared__ uint32_t sh_m;
  const int q = blockIdx.x;
  const uint32_t cnt = ip_hits(counts, q);
  if (threadIdx.x == 0) counts_packed[q] = cnt;
  const int c = cnt < (uint32_t)cap ? (int)cnt : cap;
  const float* ls = list_s + (int64_t)q * cap;
  const uint32_t* li = list_id + (int64_t)q * cap;
  uint32_t* bi = band_id + (int64_t)q * cap;
  if (threadIdx.x == 0) sh_m = 0;
  __syncthreads();
  const int need = (int64_t)k < n ? k : (int)n;
  const float t = tau[q];
  const float eps = band.eps(q);
  const bool out_of_range = band.out_of_range(q);
  const bool have_k = need > 0 && c >= need;
  float cut = -INFINITY;
  if (have_k)
    cut = f32_from_order_key((uint32_t)block_kth_largest<32>([&](int i) { return (uint64_t)f32_order_key(ls[i]); }, c,
                                                             (uint32_t)need, sc)) -
          2.f * eps;
  for (int i0 = 0; i0 < c; i0 += IP_DEEP_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    const bool hit = i < c && ls[i] >= cut;
    const uint32_t slot = wave_append_slot(hit, &sh_m);
    if (hit) bi[slot] = li[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const IpVerdict v = ip_topk_verdict(cnt, cap, c, need, t, cut, eps, out_of_range);
    m_out[q] = sh_m;
    status[q] = v.status;
    tau_retry[q] = v.retry;
  }
}

// Sub-stages j0, j0 / 2, .., 1 of merge step k2 of the bitonic network, for the LDS tile that holds elements
// [base, base + nt) of the sequence (nt a power of two, j0 < nt).  One compare-exchange per thread and pair.
__device__ __forceinline__ void deep_tile_steps(double* s, uint32_t* id, int nt, int base, int k2, int j0) {
  for (int j = j0; j > 0; j >>= 1) {
    for (int t = threadIdx.x; t < (nt >> 1); t += IP_DEEP_THREADS) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
      const double x = s[i], y = s[p];
      const uint32_t ix = id[i], iy = id[p];
      const bool fwd = ((base + i) & k2) == 0;
      const bool sw = fwd ? cand_before(y, iy, x, ix) : cand_before(x, ix, y, iy);
      if (sw) { s[i] = y; s[p] = x; id[i] = iy; id[p] = ix; }
    }
    __syncthreads();
  }
}

// Orders gx / gi [0, np2) (global memory, np2 a power of two) by (score desc, id asc): the bitonic network of
// bitonic_cand, tiled.  A sub-stage whose partner distance is at least one tile is a sweep through global memory; as soon
// as the distance is inside a tile, the tile is loaded into LDS, all remaining sub-stages of the merge step finish there
// and the tile is written back.  At np2 = 131,072 that is 15 global sweeps and 6 tile passes instead of 153 sweeps.
// Every element is read and written by threads of this one workgroup only, with a barrier between sub-stages.
__device__ void deep_bitonic(double* gx, uint32_t* gi, int np2, double* s, uint32_t* id) {
  const int tile = np2 < IP_DEEP_TILE ? np2 : IP_DEEP_TILE;
  auto load = [&](int base) {
    for (int i = threadIdx.x; i < tile; i += IP_DEEP_THREADS) { s[i] = gx[base + i]; id[i] = gi[base + i]; }
    __syncthreads();
  };
  auto store = [&](int base) {
    for (int i = threadIdx.x; i < tile; i += IP_DEEP_THREADS) { gx[base + i] = s[i]; gi[base + i] = id[i]; }
    __syncthreads();
  };
  for (int base = 0; base < np2; base += tile) {
    load(base);
    for (int k2 = 2; k2 <= tile; k2 <<= 1) deep_tile_steps(s, id, tile, base, k2, k2 >> 1);
    store(base);
  }
  for (int k2 = tile << 1; k2 <= np2; k2 <<= 1) {
    for (int j = k2 >> 1; j >= tile; j >>= 1) {
      for (int t = threadIdx.x; t < (np2 >> 1); t += IP_DEEP_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const double x = gx[i], y = gx[p];
        const uint32_t ix = gi[i], iy = gi[p];
        const bool fwd = (i & k2) == 0;
        const bool sw = fwd ? cand_before(y, iy, x, ix) : cand_before(x, ix, y, iy);
        if (sw) { gx[i] = y; gx[p] = x; gi[i] = iy; gi[p] = ix; }
      }
      __syncthreads();
    }
    for (int base = 0; base < np2; base += tile) {
      load(base);
      deep_tile_steps(s, id, tile, base, k2, tile >> 1);
      store(base);
    }
  }
}

// k_ip_select over a band in global memory.  band_* [nq, cap]: the re-scored band (read only); sort_x / sort_id [nq, cap]:
// the survivors {high key word >= that of the k-th exact score} -- more than k only for ties at the boundary word --,
// ordered in place; D / I [nq, k].
__global__ void __launch_bounds__(IP_DEEP_THREADS) k_ip_select_deep(int k, int cap, const uint32_t* __restrict__ m_in,
                                                                    const uint32_t* __restrict__ band_id,
                                                                    const double* __restrict__ band_x, uint32_t* sort_id,
                                                                    double* sort_x, float* __restrict__ D,
                                                                    int64_t* __restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ SelectScratch sc;
  __shared__ uint32_t sh_g;
  const int q = blockIdx.x;
  const uint32_t mq = m_in[q];
  const int c = mq < (uint32_t)cap ? (int)mq : cap;
  const double* bx = band_x + (int64_t)q * cap;
  const uint32_t* bi = band_id + (int64_t)q * cap;
  double* gx = sort_x + (int64_t)q * cap;
  uint32_t* gi = sort_id + (int64_t)q * cap;
  double* s = (double*)smem;
  uint32_t* id = (uint32_t*)(smem + (size_t)IP_DEEP_TILE * 8);
  if (threadIdx.x == 0) sh_g = 0;
  __syncthreads();
  uint64_t kth = 0;   // c <= k: everything survives
  if (c > k) kth = block_kth_largest<32>([&](int i) { return f64_order_key(bx[i]) >> 32; }, c, (uint32_t)k, sc);
  for (int i0 = 0; i0 < c; i0 += IP_DEEP_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    const double x = i < c ? bx[i] : 0.0;
    const bool hit = i < c && (f64_order_key(x) >> 32) >= kth;
    const uint32_t slot = wave_append_slot(hit, &sh_g);
    if (hit) { gx[slot] = x; gi[slot] = bi[i]; }
  }
  __syncthreads();
  const int g = (int)sh_g;
  int np2 = 2;
  while (np2 < g) np2 <<= 1;   // g <= c <= cap, cap a power of two: np2 <= cap
  for (int i = g + threadIdx.x; i < np2; i += IP_DEEP_THREADS) { gx[i] = -INFINITY; gi[i] = 0xffffffffu; }
  __syncthreads();
  deep_bitonic(gx, gi, np2, s, id);
  for (int j = threadIdx.x; j < k; j += IP_DEEP_THREADS) {
    D[(int64_t)q * k + j] = j < g ? (float)gx[j] : -FLT_MAX;
    I[(int64_t)q * k + j] = j < g ? (int64_t)gi[j] : -1;
  }
}

// ------------------------------------------------------------------------------------------
// host-side plan of the deep search
// ------------------------------------------------------------------------------------------
struct IpDeepPlan : IpPlanHead {
  int mode;            // -1: n <= cap, every row is a candidate; IP_MODE_FULL: threshold from a row sample
  int R;               // rank the threshold aims at in the whole block
  int nSeg, segTiles;  // the sample: nSeg runs of segTiles passage tiles, run g starting at tile g * nPt / nSeg
  int64_t sampled_rows, t_rows;   // rows of the block in the sample / rows of T the sample fills
  int r;               // rank selected inside the sample
  size_t o_qlo, o_counts_packed, o_T, o_bid, o_bx, o_sx;
};

// Threshold rule.  The list has `cap` slots, the cut needs the k best scan scores in it and the band below them.  The
// threshold aims at rank R = cap / 2 of the whole block (k + (cap - k) / 2 where that leaves less than 1.5x above k), so
// that the list may come out a third shorter or longer than planned and still hold k without overflowing.  R is
// estimated from the COMPLETE scan scores of S sampled rows: with f = S / n the rank-round(R f) score of the sample sits
// at a whole-block rank whose relative standard deviation is 1 / sqrt(R f) (the number of the block's R best rows that
// fall into the sample is hypergeometric, variance <= R f).  S is chosen for R f >= IP_DEEP_SAMPLE_RANK = 512: 4.4 %, so
// even six deviations (27 %) stay inside the 1.33x .. 1.5x headroom on either side.  S is at least IP_SAMPLE_MIN rows
// (as the shallow plan) and at most IP_SAMPLE_MAX (the sample's score matrix is S x nq_pad floats: 1 GB at 1,024
// queries); beyond n = R / 512 * IP_SAMPLE_MAX rows the expected sample rank falls below 512 and misses get likelier.
// A miss -- or rows that are not exchangeable, e.g. a block sorted by topic -- costs one retry with the threshold the
// cut proposes, never correctness: the certificate decides.
// The scan kernel writes a tile's scores at the tile's own row, so a strided sample would need a score matrix as tall
// as the block; the sample is therefore IP_DEEP_SAMPLE_SEGMENTS evenly spaced runs of whole tiles, each scanned by one
// launch over a sub-block (its own P pointer and row count), writing its rows of T contiguously.
static IpDeepPlan ip_deep_plan(int nq, int64_t n, int d, int k, int cap, int rank_target) {
  IpDeepPlan p{ip_plan_head(nq, n)};
  int R = rank_target > 0 ? rank_target : cap / 2;
  if (2 * (int64_t)R < 3 * (int64_t)k) R = k + (cap - k) / 2;
  if (R > cap) R = cap;
  p.R = R;
  p.nSeg = 0; p.segTiles = 0; p.sampled_rows = 0; p.t_rows = 0; p.r = 0;
  if (n <= cap) {
    p.mode = -1;
  } else {
    p.mode = IP_MODE_FULL;
    int64_t S = ceil_div64((int64_t)IP_DEEP_SAMPLE_RANK * n, R);
    if (S < IP_SAMPLE_MIN) S = IP_SAMPLE_MIN;
    if (S > IP_SAMPLE_MAX) S = IP_SAMPLE_MAX;
    const int64_t nSt = ceil_div64(S, p.tr);
    p.nSeg = nSt < IP_DEEP_SAMPLE_SEGMENTS ? (int)nSt : IP_DEEP_SAMPLE_SEGMENTS;
    p.segTiles = (int)ceil_div64(nSt, p.nSeg);
    if ((int64_t)p.nSeg * p.segTiles >= p.nPt) { p.nSeg = 1; p.segTiles = p.nPt; }   // the whole block is the sample
    p.t_rows = (int64_t)p.nSeg * p.segTiles * p.tr;
    const int64_t last_end = ((int64_t)(p.nSeg - 1) * p.nPt / p.nSeg + p.segTiles) * p.tr;
    p.sampled_rows = p.t_rows - (last_end > n ? last_end - n : 0);
    int64_t r = llrint((double)R * (double)p.sampled_rows / (double)n);
    if (r < 1) r = 1;
    if (r > p.sampled_rows) r = p.sampled_rows;
    p.r = (int)r;
  }
  // Layout as before the shared head: qb|qlo|qnorm|tau|counts|counts_packed|m|T|id|s|bid|bx|sx, same sizes (no accessors).
  WsCursor ws;
  p.o_qb = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qlo = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qnorm = ws.take((size_t)p.nq_pad * 4);
  p.o_tau = ws.take((size_t)p.nq_pad * 4);
  p.o_counts = ws.take((size_t)p.nq_pad * IP_COUNT_STRIDE * 4);
  p.o_counts_packed = ws.take((size_t)p.nq_pad * 4);
  p.o_m = ws.take((size_t)p.nq_pad * 4);
  // T is sized for the tallest sample any threshold rank allows (R >= 1.5 k), whether or not this call samples: the size
  // then depends on neither rank_target nor the plan's branch, and never shrinks when cap grows
  int64_t s_max = ceil_div64((int64_t)2 * IP_DEEP_SAMPLE_RANK * n, (int64_t)3 * k);
  if (s_max < IP_SAMPLE_MIN) s_max = IP_SAMPLE_MIN;
  if (s_max > IP_SAMPLE_MAX) s_max = IP_SAMPLE_MAX;
  int64_t t_tiles = ceil_div64(s_max, p.tr) + IP_DEEP_SAMPLE_SEGMENTS;
  if (t_tiles > p.nPt) t_tiles = p.nPt;
  if (t_tiles * p.tr < p.t_rows) t_tiles = p.t_rows / p.tr;
  p.o_T = ws.take((size_t)t_tiles * p.tr * p.nq_pad * 4);
  p.o_id = ws.take((size_t)nq * cap * 4);     // the scan's list: ids; after the cut: the survivors' ids (k_ip_select_deep)
  p.o_s = ws.take((size_t)nq * cap * 4);      // the scan's list: scan scores
  p.o_bid = ws.take((size_t)nq * cap * 4);    // the band: ids
  p.o_bx = ws.take((size_t)nq * cap * 8);     // the band: canonical fp64 scores
  p.o_sx = ws.take((size_t)nq * cap * 8);     // the survivors' scores, ordered in place
  p.total = ws.at;
  return p;
}

// The deep pipeline.  p plans the arguments ip_topk validated; the row filter as in ip_search (ip_host.hpp).
static int ip_search_deep(const char* name, const IpBlock& b, const IpTopkArgs& c, const IpDeepPlan& p) {
  if (int e = ip_check_workspace(name, c.workspace_bytes, p.total)) return e;
  const int nq = c.nq, k = c.k, cap = c.cap;
  const int64_t n = b.n;
  hipStream_t st = c.st;
  char* ws = (char*)c.workspace;
  float* qnorm = (float*)(ws + p.o_qnorm);
  float* tau = (float*)(ws + p.o_tau);
  uint32_t* counts = (uint32_t*)(ws + p.o_counts);
  uint32_t* counts_packed = (uint32_t*)(ws + p.o_counts_packed);
  float* T = (float*)(ws + p.o_T);
  uint32_t* list_id = (uint32_t*)(ws + p.o_id);
  float* list_s = (float*)(ws + p.o_s);
  uint32_t* band_id = (uint32_t*)(ws + p.o_bid);
  double* band_x = (double*)(ws + p.o_bx);
  double* sort_x = (double*)(ws + p.o_sx);
  uint32_t* band_m = (uint32_t*)(ws + p.o_m);
  bf16_t* qlo = b.split() ? (bf16_t*)(ws + p.o_qlo) : nullptr;
  const bool all_candidates = p.mode < 0 || (b.row_bits && b.n_allowed <= cap);

  if (int e = ip_prepare_queries(b, p, ws, c.q_f32, nq, qlo, st)) return e;
  const ScanArgs emit = ip_scan_args(b, p, ws, nq, cap, qlo, T);
  if (n == 0 || c.tau_in || all_candidates) {   // (an empty block is not scanned: -inf, whatever tau_in is)
    if (int e = ip_given_tau(p, ws, n > 0 ? c.tau_in : nullptr, nq, st)) return e;
  } else {
    for (int g = 0; g < p.nSeg; ++g) {
      const int64_t row0 = (int64_t)g * p.nPt / p.nSeg * p.tr;
      const int64_t rows = std::min<int64_t>((int64_t)p.segTiles * p.tr, n - row0);
      ScanArgs a = emit;
      a.P = emit.P + row0 * emit.d;             // (emit.d: the row's 16-bit words -- b.d, or b.d / 2 for rows of int8 codes)
      if (emit.Plo) a.Plo = emit.Plo + row0 * emit.d;
      if (emit.bits) a.bits = emit.bits + row0 / 32;   // (row0 is a multiple of the tile height: whole words)
      a.n = rows;
      a.nPt = (int)ceil_div64(rows, p.tr);   // = segTiles: only the block's last tile is ragged
      a.T = T + (int64_t)g * p.segTiles * p.tr * p.nq_pad;
      if (int e = launch_scan<IP_MODE_FULL>(a, p.big, b.kind(), st)) return e;
    }
    ProfScope prof("ip_tau_deep", st);
    hipLaunchKernelGGL(k_tau_select_deep, dim3(nq), dim3(IP_DEEP_THREADS), 0, st, T, (int)p.t_rows, p.nq_pad, p.r, tau);
    CONVDR_CHECK_LAUNCH("k_tau_select_deep");
  }
  if (n > 0)
    if (int e = launch_scan<IP_MODE_EMIT>(emit, p.big, b.kind(), st)) return e;
  {
    ProfScope prof("ip_cut_deep", st);
    hipLaunchKernelGGL(k_ip_cut_deep, dim3(nq), dim3(IP_DEEP_THREADS), 0, st, b.n_need(), k, cap, counts, counts_packed, list_id, list_s,
                       band_id, tau, b.band(qnorm), band_m, c.status, c.tau_retry);
    CONVDR_CHECK_LAUNCH("k_ip_cut_deep");
  }
  if (n > 0) {
    // (bands are thousands of rows per query here: more waves per query than the shallow call's 64 when queries are few)
    ProfScope prof("ip_rescore_deep", st);
    if (int e = ip_rescore(b, c.q_f32, nq, nq < 64 ? 128 : 16, cap, band_m, band_id, band_x, st)) return e;
  }
  static DeviceOnce attr_done;
  if (attr_done.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_select_deep, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         IP_DEEP_TILE * 12));
  ProfScope prof("ip_select_deep", st);
  hipLaunchKernelGGL(k_ip_select_deep, dim3(nq), dim3(IP_DEEP_THREADS), (size_t)IP_DEEP_TILE * 12, st, k, cap, band_m, band_id, band_x,
                     list_id, sort_x, c.D, c.I);
  CONVDR_CHECK_LAUNCH("k_ip_select_deep");
  return 0;
}

}  // namespace convdr

extern "C" size_t convdr_ip_deep_workspace_bytes(int nq, int64_t n, int d, int k, int cap) {
  using namespace convdr;
  if (ip_check_sizes(IP_DEEP, nq, n, d, k, cap)) return 0;
  return ip_deep_plan(nq, n, d, k, cap, 0).total;
}
