// Exact range search: every row whose canonical fp64 score exceeds a per-query radius (included by ip_topk.hip, after the
// kernels it reuses; contract in include/convdr_hip.h, "Range search").
//
//   k_rows_to_half       the queries' 16-bit operands and norms, counters zeroed            (unchanged)
//   k_ip_range_tau       radius[q] -> the scan threshold tau[q], every rounding pushed DOWN
//   k_ip_scan*<EMIT>     one single-pass scan: the list of {S~ >= tau}, all hits counted     (unchanged; filtered variants)
//   k_ip_range_clamp     m[q] = min(hits, cap)
//   k_ip_rescore         canonical fp64 score of all m list entries: the whole list is the band (unchanged)
//   k_ip_range_select    predicate x > (double)radius, survivors compacted and ordered by (score desc, id asc), status
//   k_ip_range_lims      exclusive scan of the survivor counts -> lims
//   k_ip_range_pack      (convdr_ip_range_pack) the ordered runs -> D + lims[q], I + lims[q], X + lims[q]
//
// The certificate is simpler than top-k's: nothing depends on an unknown k-th score.  With eps the band of k_ip_cut
// (|S~ - exact scaled score| <= eps for every row of the block) and tau <= scaled(radius) - eps, a row with exact score
// > radius has S~ >= tau and is in the list unless the list overflowed; the list's entries are re-scored and decided on
// the canonical fp64 value.  So a query fails only by OVERFLOW (re-run with a list as long as the reported hit count) or
// by RANGE (the fp16 scale no longer fits the block).  The split scans would only narrow the band of wasted re-scores;
// they are left out.
#pragma once

namespace convdr {

constexpr int IP_RANGE_THREADS = 1024;
constexpr int IP_RANGE_LDS_SORT = 8192;        // survivors ordered by the LDS network; more take deep_bitonic

// tau[q] = round_down(qs[q] * p_scale * (radius[q] - q . centre)) - eps[q].   One wave per query.
//
// CLAIM: every row p of the block whose canonical score X(q, p) exceeds radius[q] has S~(q, p) >= tau[q].
//   Let x = q . p in real arithmetic, c the centre (0 when there is none), v = p - c, and g = (d + 8) 2^-52.
//   1. The canonical score is an fp64 sum of exact products, at most d / 64 + 6 roundings deep: |X - x| <= g |q| |p| <=
//      g |q| (|c| + |v|) =: e_x.  So X > radius implies q . v > radius - q . c - e_x.
//   2. q . c is summed in fp64 here, same depth: |fl(q . c) - q . c| <= g sum |q_i c_i| =: e_c.  t below is
//      radius - fl(q . c) - e_c - e_x with every operation's rounding (relative 2^-53) charged by the final
//      t -= 2^-50 (|radius| + |fl(q . c)| + e_c + e_x) (IpCentreTerms::bound): t <= radius - q . c - e_x, hence q . v > t.
//   3. The scan operands are qs q and p_scale fl32(v): powers of two scale exactly, so qs p_scale q . v > qs p_scale t
//      =: s (exact in fp64: a power-of-two factor; overflow to +-inf keeps the order).  f = s rounded to fp32 toward -inf.
//   4. |S~ - qs p_scale q . v| <= eps: the band of k_ip_cut (IpBand::eps).  (It bounds the error against the
//      fp32-rounded v; the rounding of the subtraction itself, <= 2^-24 |q| |v|, sits inside the 1.0001 and 1.001
//      factors the band already carries: the smallest coefficient, fp16 one pass, is 2^-11 + d 2^-23 > 4.8e-4, and
//      1.1e-3 of it exceeds 2^-24.)  Hence S~ > f - eps.
//   5. tau = fp32(f - eps) moved one ulp down: tau <= f - eps.  So S~ > tau.
// radius = +inf gives tau = +inf (no score exceeds it, and no finite S~ reaches it).  radius = -inf -- every row -- gives
// tau = -FLT_MAX, and no tau is ever lower: the scan scores the rows past the block's end in its last tile -inf, and they
// must not be listed (the whole list is re-scored here; top-k drops them with the band).  Every real row has a finite S~
// unless an operand holds inf, which is the RANGE status.
// per_row_scale: the queries were scaled row by row (k_rows_to_half<F16, true>): qnorm holds the SCALED norm, and qs, a
// power of two, is recovered from its ratio to the unscaled norm summed here (the ratio is 2^k (1 +- 1e-6); a zero or
// non-finite query was left unscaled: qs = 1).
__global__ void __launch_bounds__(256) k_ip_range_tau(const float* __restrict__ Q, int nq, int d, const float* __restrict__ centre,
                                                      const float* __restrict__ radius, const IpBand band, int per_row_scale,
                                                      float* __restrict__ tau) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= nq) return;
  const IpCentreSums sums = ip_centre_sums(Q + (int64_t)q * d, centre, d, lane);
  if (lane != 0) return;
  const double r = (double)radius[q];
  float t32;
  if (r == (double)INFINITY) {
    t32 = INFINITY;
  } else if (r == -(double)INFINITY) {
    t32 = -FLT_MAX;
  } else {
    const IpCentreTerms ct(sums, d, band.qnorm[q], band.p_max_norm[0], per_row_scale);
    const float f = ip_scan_units<false>(ct.bound<false>(r), ct.qs, band.p_scale);   // steps 2 and 3
    t32 = nextafterf(f - band.eps(q), -INFINITY);
    if (!(t32 >= -FLT_MAX)) t32 = -FLT_MAX;  // (NaN from a non-finite norm or query -- RANGE reports it --, or -inf: see above)
  }
  tau[q] = t32;
}

__global__ void k_ip_range_clamp(const uint32_t* __restrict__ counts, int nq, int cap, uint32_t* __restrict__ m_out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint32_t c = ip_hits(counts, q);
  m_out[q] = c < (uint32_t)cap ? c : (uint32_t)cap;
}

// One workgroup per query.  list_id / list_x [nq, cap]: the scan's list and its canonical scores (read only); sort_id /
// sort_x [nq, cap]: the survivors {x > radius}, ordered in place by (x desc, id asc); nsurv[q]: their number (0 unless the
// status is OK: lims then gives a failed query an empty run).  counts_out[q]: the survivors, or the scan's hit count when
// the list overflowed.  COUNT_ONLY: predicate and count, nothing else is written to the workspace.
// Everything read here was written by this call's scan (the first min(hits, cap) list entries) or re-score.
template <bool COUNT_ONLY>
__global__ void __launch_bounds__(IP_RANGE_THREADS) k_ip_range_select(int cap, const uint32_t* __restrict__ counts,
                                                                      const uint32_t* __restrict__ list_id,
                                                                      const double* __restrict__ list_x,
                                                                      const float* __restrict__ radius, const IpBand band,
                                                                      uint32_t* sort_id, double* sort_x,
                                                                      uint32_t* __restrict__ nsurv, int64_t* __restrict__ counts_out,
                                                                      int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ uint32_t sh_g;
  const int q = blockIdx.x;
  const uint32_t cnt = ip_hits(counts, q);
  const int m = cnt < (uint32_t)cap ? (int)cnt : cap;
  const double r = (double)radius[q];
  const uint32_t* li = list_id + (int64_t)q * cap;
  const double* lx = list_x + (int64_t)q * cap;
  double* gx = sort_x + (int64_t)q * cap;
  uint32_t* gi = sort_id + (int64_t)q * cap;
  const int st = ip_list_verdict(cnt, cap, 0u, band.out_of_range(q));
  if (threadIdx.x == 0) sh_g = 0;
  __syncthreads();
  for (int i0 = 0; i0 < m; i0 += IP_RANGE_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    const double x = i < m ? lx[i] : 0.0;
    const bool hit = i < m && x > r;
    const uint32_t slot = wave_append_slot(hit, &sh_g);
    if (!COUNT_ONLY && st == CONVDR_IP_OK && hit) { gx[slot] = x; gi[slot] = li[i]; }
  }
  __syncthreads();
  const int g = (int)sh_g;
  if (threadIdx.x == 0) {
    status[q] = st;
    counts_out[q] = st == CONVDR_IP_OVERFLOW ? (int64_t)cnt : (int64_t)g;
    nsurv[q] = st == CONVDR_IP_OK ? (uint32_t)g : 0u;
  }
  if (COUNT_ONLY || st != CONVDR_IP_OK || g < 2) return;
  int np2 = 2;
  while (np2 < g) np2 <<= 1;      // g <= m <= cap, cap a power of two: np2 <= cap
  double* s = (double*)smem;
  if (np2 <= IP_RANGE_LDS_SORT) {
    uint32_t* id = (uint32_t*)(smem + (size_t)np2 * 8);
    for (int i = threadIdx.x; i < np2; i += IP_RANGE_THREADS) {
      s[i] = i < g ? gx[i] : -INFINITY;
      id[i] = i < g ? gi[i] : 0xffffffffu;
    }
    __syncthreads();
    bitonic_cand(s, id, np2);
    for (int i = threadIdx.x; i < g; i += IP_RANGE_THREADS) { gx[i] = s[i]; gi[i] = id[i]; }
  } else {
    uint32_t* id = (uint32_t*)(smem + (size_t)IP_DEEP_TILE * 8);
    for (int i = g + threadIdx.x; i < np2; i += IP_RANGE_THREADS) { gx[i] = -INFINITY; gi[i] = 0xffffffffu; }
    __syncthreads();
    deep_bitonic(gx, gi, np2, s, id);
  }
}

// lims[0] = 0, lims[q + 1] = nsurv[0] + .. + nsurv[q].  One workgroup: a thread sums a contiguous run of queries, the 1024
// run totals are scanned in LDS, the thread writes its run.
__global__ void __launch_bounds__(IP_RANGE_THREADS) k_ip_range_lims(const uint32_t* __restrict__ nsurv, int nq,
                                                                    int64_t* __restrict__ lims) {
  __shared__ int64_t part[IP_RANGE_THREADS];
  const int per = (nq + IP_RANGE_THREADS - 1) / IP_RANGE_THREADS;
  const int a = (int)threadIdx.x * per, b = a + per < nq ? a + per : nq;
  int64_t sum = 0;
  for (int i = a; i < b; ++i) sum += nsurv[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < IP_RANGE_THREADS; o <<= 1) {
    const int64_t v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = part[threadIdx.x] - sum;    // exclusive
  if (threadIdx.x == 0) lims[0] = 0;
  for (int i = a; i < b; ++i) {
    run += nsurv[i];
    lims[i + 1] = run;
  }
}

__global__ void k_ip_range_zero(int nq, int64_t* __restrict__ counts, int64_t* __restrict__ lims, int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq) { counts[i] = 0; status[i] = CONVDR_IP_OK; }
  if (lims && i <= nq) lims[i] = 0;
}

// grid (nq, chunks): query q's ordered run of lims[q + 1] - lims[q] entries -> D / I / X + lims[q]
__global__ void __launch_bounds__(256) k_ip_range_pack(int cap, const uint32_t* __restrict__ sort_id, const double* __restrict__ sort_x,
                                                       const int64_t* __restrict__ lims, float* __restrict__ D,
                                                       int64_t* __restrict__ I, double* __restrict__ X) {
  const int q = blockIdx.x;
  const int64_t at = lims[q], g = lims[q + 1] - at;
  const double* gx = sort_x + (int64_t)q * cap;
  const uint32_t* gi = sort_id + (int64_t)q * cap;
  for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < g && i < cap; i += (int64_t)gridDim.y * 256) {
    const double x = gx[i];
    D[at + i] = (float)x;
    I[at + i] = (int64_t)gi[i];
    if (X) X[at + i] = x;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct IpRangePlan : IpPlanHead {
  size_t o_nsurv, o_x, o_sx;
};

// Workspace layout: the regions of the contract (include/convdr_hip.h, "Range search": workspace), order and sizes as before
// the shared head.  Only the total has an accessor; convdr_ip_range_pack finds o_s (after the scan: the survivors' ids) and o_sx.
static IpRangePlan ip_range_plan(int nq, int64_t n, int d, int cap) {
  IpRangePlan p{ip_plan_head(nq, n)};
  WsCursor ws;
  p.o_qb = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qnorm = ws.take((size_t)p.nq_pad * 4);
  p.o_tau = ws.take((size_t)p.nq_pad * 4);
  p.o_counts = ws.take((size_t)p.nq_pad * IP_COUNT_STRIDE * 4);
  p.o_m = ws.take((size_t)p.nq_pad * 4);
  p.o_nsurv = ws.take((size_t)p.nq_pad * 4);
  p.o_id = ws.take((size_t)nq * cap * 4);
  p.o_s = ws.take((size_t)nq * cap * 4);
  p.o_x = ws.take((size_t)nq * cap * 8);
  p.o_sx = ws.take((size_t)nq * cap * 8);
  p.total = ws.at;
  return p;
}

// The range pipeline behind convdr_ip_range_search: every check of its arguments, then the launches.  b.store is in range.
static int ip_range_search(const IpBlock& b, const float* q_f32, int nq, const float* centre, const float* radius, int cap,
                           int count_only, void* workspace, size_t workspace_bytes, int64_t* counts, int64_t* lims,
                           int32_t* status, hipStream_t st) {
  const char* name = "convdr_ip_range_search";
  if (int e = ip_check_sizes(IP_RANGE, nq, b.n, b.d, 0, cap)) return e;
  CONVDR_REQUIRE(count_only == 0 || count_only == 1, "%s: count_only=%d (0 or 1)", name, count_only);
  CONVDR_REQUIRE(!b.rows_f16() || centre == nullptr, "%s: the half store has no centre", name);
  CONVDR_REQUIRE(b.row_bits != nullptr || b.row_bits_words == 0, "%s: row_bits is NULL but row_bits_words=%lld", name,
                 (long long)b.row_bits_words);
  if (int e = ip_check_block(name, b)) return e;
  const IpRangePlan p = ip_range_plan(nq, b.n, b.d, cap);
  if (int e = ip_check_workspace(name, workspace_bytes, p.total)) return e;
  CONVDR_REQUIRE(q_f32 && radius && counts && status && (lims || count_only) && workspace,
                 "%s: a NULL argument (q_f32, radius, workspace, counts, status; lims unless count_only)", name);
  CONVDR_REQUIRE(b.n == 0 || (b.p_half && b.p_max_norm && (b.rows_f16() || b.p_f32)),
                 "%s: a NULL block pointer (p_half, p_max_norm; p_f32 unless store = 2)", name);
  if (b.n == 0) {
    hipLaunchKernelGGL(k_ip_range_zero, dim3((nq + 256) / 256), dim3(256), 0, st, nq, counts, lims, status);
    CONVDR_CHECK_LAUNCH("k_ip_range_zero");
    return 0;
  }
  char* ws = (char*)workspace;
  float* qnorm = (float*)(ws + p.o_qnorm);
  float* tau = (float*)(ws + p.o_tau);
  uint32_t* hits = (uint32_t*)(ws + p.o_counts);
  uint32_t* m = (uint32_t*)(ws + p.o_m);
  uint32_t* nsurv = (uint32_t*)(ws + p.o_nsurv);
  uint32_t* list_id = (uint32_t*)(ws + p.o_id);
  uint32_t* sort_id = (uint32_t*)(ws + p.o_s);     // (the scan scores are dead once the scan has ended)
  double* list_x = (double*)(ws + p.o_x);
  double* sort_x = (double*)(ws + p.o_sx);

  if (int e = ip_prepare_queries(b, p, ws, q_f32, nq, nullptr, st)) return e;   // (one pass: no remainders)
  hipLaunchKernelGGL(k_ip_range_tau, dim3((nq + 3) / 4), dim3(256), 0, st, q_f32, nq, b.d, centre, radius, b.band(qnorm),
                     b.kind() == IP_KIND_F16 ? 1 : 0, tau);
  CONVDR_CHECK_LAUNCH("k_ip_range_tau");
  if (int e = launch_scan<IP_MODE_EMIT>(ip_scan_args(b, p, ws, nq, cap, nullptr, nullptr), p.big, b.kind(), st)) return e;
  hipLaunchKernelGGL(k_ip_range_clamp, dim3((nq + 255) / 256), dim3(256), 0, st, hits, nq, cap, m);
  CONVDR_CHECK_LAUNCH("k_ip_range_clamp");
  {
    ProfScope prof("ip_range_rescore", st);
    if (int e = ip_rescore(b, q_f32, nq, nq < 64 ? 128 : 16, cap, m, list_id, list_x, st)) return e;
  }
  {
    ProfScope prof("ip_range_select", st);
    if (count_only) {
      hipLaunchKernelGGL(k_ip_range_select<true>, dim3(nq), dim3(IP_RANGE_THREADS), 0, st, cap, hits, list_id, list_x, radius,
                         b.band(qnorm), sort_id, sort_x, nsurv, counts, status);
    } else {
      const int lds_n = cap < IP_RANGE_LDS_SORT ? cap : IP_RANGE_LDS_SORT;     // (>= IP_DEEP_TILE whenever deep_bitonic can run)
      static DeviceOnce attr_done;
      if (attr_done.first())
        CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_range_select<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             IP_RANGE_LDS_SORT * 12));
      hipLaunchKernelGGL(k_ip_range_select<false>, dim3(nq), dim3(IP_RANGE_THREADS), (size_t)lds_n * 12, st, cap, hits, list_id,
                         list_x, radius, b.band(qnorm), sort_id, sort_x, nsurv, counts, status);
    }
    CONVDR_CHECK_LAUNCH("k_ip_range_select");
  }
  if (lims) {
    hipLaunchKernelGGL(k_ip_range_lims, dim3(1), dim3(IP_RANGE_THREADS), 0, st, nsurv, nq, lims);
    CONVDR_CHECK_LAUNCH("k_ip_range_lims");
  }
  return 0;
}

}  // namespace convdr

extern "C" size_t convdr_ip_range_workspace_bytes(int nq, int64_t n, int d, int cap) {
  using namespace convdr;
  if (ip_check_sizes(IP_RANGE, nq, n, d, 0, cap)) return 0;
  return ip_range_plan(nq, n, d, cap).total;
}

extern "C" int convdr_ip_range_search(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale,
                                      const float* centre, int64_t n, int d, const float* p_max_norm, const float* radius,
                                      int cap, int count_only, const uint32_t* row_bits, int64_t row_bits_words, void* workspace,
                                      size_t workspace_bytes, int64_t* counts, int64_t* lims, int32_t* status,
                                      convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(store >= 0 && store <= 2, "convdr_ip_range_search: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) "
                 "(got %d)", store);
  // (one pass: no remainder copy; n_allowed is top-k's)
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, p_max_norm, row_bits, row_bits_words, 0};
  return ip_range_search(b, q_f32, nq, centre, radius, cap, count_only, workspace, workspace_bytes, counts, lims, status,
                         (hipStream_t)stream);
}

extern "C" int convdr_ip_range_pack(const void* workspace, int nq, int64_t n, int d, int cap, const int64_t* lims, float* D,
                                    int64_t* I, double* X, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(ip_check_sizes(IP_RANGE, nq, n, d, 0, cap) == 0,
                 "convdr_ip_range_pack: sizes outside the contract of convdr_ip_range_search (nq=%d n=%lld d=%d cap=%d)", nq,
                 (long long)n, d, cap);
  CONVDR_REQUIRE(workspace && lims && D && I, "convdr_ip_range_pack: a NULL argument (workspace, lims, D, I)");
  if (n == 0) return 0;     // every run is empty
  const IpRangePlan p = ip_range_plan(nq, n, d, cap);
  const char* ws = (const char*)workspace;
  const int chunks = cap / 1024 < 32 ? cap / 1024 : 32;
  hipLaunchKernelGGL(k_ip_range_pack, dim3(nq, chunks), dim3(256), 0, (hipStream_t)stream, cap, (const uint32_t*)(ws + p.o_s),
                     (const double*)(ws + p.o_sx), lims, D, I, X);
  CONVDR_CHECK_LAUNCH("k_ip_range_pack");
  return 0;
}
