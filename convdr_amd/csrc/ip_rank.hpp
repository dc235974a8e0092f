// Exact score and exact rank of GIVEN rows (included by ip_topk.hip after ip_range.hpp; contract in include/convdr_hip.h,
// "Score and rank of given rows").
//
//   k_ip_score_rows      canonical fp64 score of (query, row) pairs named by int64 ids; ids outside [0, n) are not dereferenced
//   k_rows_to_half       the queries' 16-bit operands and norms, both counter arrays zeroed      (unchanged)
//   k_ip_band_tau        X_t[q] -> two scan thresholds: tau_lo (every rounding DOWN) and tau_hi (every rounding UP)
//   k_ip_scan_r3<BAND>   one single-pass scan: rows with S~ >= tau_hi are COUNTED, rows in [tau_lo, tau_hi) are listed
//   k_ip_range_clamp     m[q] = min(band hits, cap)                                               (unchanged)
//   k_ip_rescore         canonical fp64 score of the m band entries                               (unchanged)
//   k_ip_rank_finish     rank = above + #{band entries that precede the target in (score desc, row asc)}, status
//
// The certificate is two-sided.  With X_t the canonical score of the query's target row t, the rank of t -- the number of rows
// that precede it in the canonical order -- is #{r : X_r > X_t} + #{r < t : X_r == X_t}.  The scan cannot decide X_r > X_t for
// rows whose scan score lies within the error band of X_t, but it can for all the others: S~ >= tau_hi PROVES X_r > X_t (such
// a row only needs counting) and S~ < tau_lo PROVES X_r < X_t (such a row is nothing).  Only the rows between the two are
// listed and re-scored, so the cost follows the width of the error band, not the rank.  A query fails only by OVERFLOW of the
// band list (re-run with a list as long as the reported band count: same thresholds, cannot overflow again) or by RANGE.
// convdr_ip_rank_docs (ip_docrank.hpp) runs the same pipeline with the marking scan and its own finish: ip_rank_rows below.
#pragma once

namespace convdr {

constexpr int IP_RANK_THREADS = 1024;

// One wave per (query, row) pair (ip_row_score: the value k_ip_rescore gives it); grid (nq, chunks).  rows / X / D share the
// pitch ld; the query of pair (q, j) is row q of Q.
// An id outside [0, n) yields the score FAISS pads with and P is not touched for it.
template <class PT>
__global__ void __launch_bounds__(256) k_ip_score_rows(const float* __restrict__ Q, typename IpRows<PT>::type P, int64_t n, int d,
                                                       const int64_t* __restrict__ rows, int m, int64_t ld,
                                                       double* __restrict__ X, float* __restrict__ D, double unscale) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* qv = Q + (int64_t)q * d;
  for (int j = blockIdx.y * 4 + wave; j < m; j += gridDim.y * 4) {
    const int64_t id = rows[(int64_t)q * ld + j];
    double acc = -(double)FLT_MAX;
    if (id >= 0 && id < n) acc = ip_row_score<PT>(qv, ip_row_at(P, id, d), d, lane, unscale);        // (wave-uniform)
    if (lane == 0) {
      if (X) X[(int64_t)q * ld + j] = acc;
      if (D) D[(int64_t)q * ld + j] = (float)acc;
    }
  }
}

// tau_lo[q], tau_hi[q] from the fp64 canonical score X_t = xt[q] of the query's target.  One wave per query, on the pieces
// k_ip_range_tau uses (ip_certify.hpp: the sums, the error terms, the eps); the radius is an fp64 value here.
//
// Notation: x = q . p in real arithmetic, c the centre (0 when there is none), v = p - c, g = (d + 8) 2^-52, qs the query's
// power-of-two scale, and
//   e_x = g |q| (|c| + max|v|)   bounds |X(q, p) - x| for every row (an fp64 sum of exact products, at most d / 64 + 6
//                                roundings deep; |p| <= |c| + |v|),
//   e_c = g sum |q_i c_i|        bounds |fl(q . c) - q . c| for the fp64 sum made here (same depth),
//   eps                          the band of k_ip_cut: |S~(p) - qs p_scale q . v| <= eps for every row.  (It bounds the error
//                                against the fp32-rounded v; the rounding of the subtraction itself, <= 2^-24 |q| |v|, sits
//                                inside the 1.0001 and 1.001 factors the band already carries: see k_ip_range_tau, step 4.)
//
// CLAIM LO: X(q, r) >= X_t  implies  S~(r) >= tau_lo.
//   1. X >= X_t and |X - x| <= e_x give x >= X_t - e_x, i.e. q . v >= X_t - q . c - e_x.
//   2. q . c <= fl(q . c) + e_c, so q . v >= X_t - fl(q . c) - e_c - e_x.  t_lo is that expression evaluated in fp64 with
//      every operation's rounding (relative 2^-53) charged by t_lo -= 2^-50 (|X_t| + |fl(q . c)| + e_c + e_x): t_lo is not
//      above the real value, hence q . v >= t_lo.
//   3. Powers of two scale exactly: qs p_scale q . v >= qs p_scale t_lo =: s_lo.  f_lo = s_lo rounded to fp32 toward -inf.
//   4. S~ >= qs p_scale q . v - eps >= f_lo - eps.
//   5. tau_lo = fp32(f_lo - eps) moved one ulp down: tau_lo <= f_lo - eps <= S~.                                        QED
// CLAIM HI: S~(r) >= tau_hi  implies  X(q, r) > X_t, strictly.
//   1. tau_hi = fp32(f_hi + eps) moved one ulp UP.  The fp32 sum is within half an ulp of f_hi + eps and the step adds a
//      whole one, so tau_hi > f_hi + eps (or tau_hi = +inf, which no score reaches).
//   2. S~ >= tau_hi and qs p_scale q . v >= S~ - eps give qs p_scale q . v > f_hi.
//   3. f_hi = s_hi rounded to fp32 toward +inf, s_hi = qs p_scale t_hi (exact): q . v > t_hi.
//   4. t_hi is X_t - fl(q . c) + e_c + e_x evaluated in fp64 with t_hi += 2^-50 (|X_t| + |fl(q . c)| + e_c + e_x): not below
//      the real value, and q . c >= fl(q . c) - e_c, so t_hi >= X_t - q . c + e_x.  Hence x = q . v + q . c > X_t + e_x.
//   5. X >= x - e_x > X_t.                                                                                              QED
// Consequences: tau_lo <= tau_hi; the target row itself has S~ >= tau_lo (LO with r = t) and S~ < tau_hi (HI would give
// X_t > X_t), so it is always in the band -- where the finishing predicate excludes it -- unless the row filter masks it.
// tau_lo is never below -FLT_MAX: the scan scores the rows past the block's end -inf, and they must reach neither branch.
// A target outside [0, n) (tgt[q]) gets tau_lo = tau_hi = +inf: no row of that column is counted or listed.  A non-finite
// intermediate (a non-finite query, norm or score: an operand may hold inf) raises bad[q] and gets the same thresholds:
// k_ip_rank_finish reports CONVDR_IP_RANGE for it, never a count.
__global__ void __launch_bounds__(256) k_ip_band_tau(const float* __restrict__ Q, int nq, int d, const float* __restrict__ centre,
                                                     const double* __restrict__ xt, const int64_t* __restrict__ tgt, int64_t n,
                                                     const IpBand band, int per_row_scale, float* __restrict__ tau_lo,
                                                     float* __restrict__ tau_hi, uint32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= nq) return;
  const IpCentreSums sums = ip_centre_sums(Q + (int64_t)q * d, centre, d, lane);
  if (lane != 0) return;
  float lo = INFINITY, hi = INFINITY;
  uint32_t flag = 0;
  const int64_t t = tgt[q];
  if (t >= 0 && t < n) {
    const double r = xt[q];
    const IpCentreTerms ct(sums, d, band.qnorm[q], band.p_max_norm[0], per_row_scale);
    double s_lo, s_hi;
    const float f_lo = ip_scan_units<false>(ct.bound<false>(r), ct.qs, band.p_scale, &s_lo);   // LO steps 2 and 3
    const float f_hi = ip_scan_units<true>(ct.bound<true>(r), ct.qs, band.p_scale, &s_hi);     // HI steps 4 and 3
    const float eps = band.eps(q);
    const bool finite = fabs(s_lo) < (double)INFINITY && fabs(s_hi) < (double)INFINITY && eps < INFINITY;   // (false for NaN)
    if (finite) {
      lo = nextafterf(f_lo - eps, -INFINITY);
      hi = nextafterf(f_hi + eps, INFINITY);
      if (!(lo >= -FLT_MAX)) lo = -FLT_MAX;
    } else {
      flag = 1u;
    }
  }
  tau_lo[q] = lo;
  tau_hi[q] = hi;
  bad[q] = flag;
}

// One workgroup per query, over the re-scored band list (the first min(hits, cap) entries, all written by this call's scan
// and re-score).  rank = above + #{band entries r : X_r > X_t or (X_r == X_t and r < t)}: the rows that precede t in the
// canonical order.  The target itself is in the band and fails the predicate; no case is needed for it.
__global__ void __launch_bounds__(IP_RANK_THREADS) k_ip_rank_finish(int cap, int64_t n, const uint32_t* __restrict__ hits,
                                                                    const uint32_t* __restrict__ above_in,
                                                                    const uint32_t* __restrict__ bad,
                                                                    const uint32_t* __restrict__ list_id,
                                                                    const double* __restrict__ list_x,
                                                                    const int64_t* __restrict__ tgt, double* __restrict__ xt,
                                                                    const IpBand band, int64_t* __restrict__ rank,
                                                                    int64_t* __restrict__ counts, int64_t* __restrict__ above,
                                                                    int32_t* __restrict__ status) {
  __shared__ uint32_t sh_g;
  const int q = blockIdx.x;
  const int64_t t = tgt[q];
  if (!(t >= 0 && t < n)) {         // (uniform) padding or an id outside the block: rank -1, nothing was scanned for it
    if (threadIdx.x == 0) { rank[q] = -1; counts[q] = 0; above[q] = 0; status[q] = CONVDR_IP_OK; }
    return;
  }
  const uint32_t cnt = ip_hits(hits, q);
  const int m = cnt < (uint32_t)cap ? (int)cnt : cap;
  const double x_t = xt[q];
  const uint32_t* li = list_id + (int64_t)q * cap;
  const double* lx = list_x + (int64_t)q * cap;
  if (threadIdx.x == 0) sh_g = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (int i = threadIdx.x; i < m; i += IP_RANK_THREADS) {
    const double x = lx[i];
    mine += (x > x_t || (x == x_t && (int64_t)li[i] < t)) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&sh_g, mine);     // (a sum of integers: the order of arrival does not show)
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t ab = ip_hits(above_in, q);
    const int st = ip_list_verdict(cnt, cap, bad[q], band.out_of_range(q));
    rank[q] = st == CONVDR_IP_OK ? (int64_t)ab + (int64_t)sh_g : -1;
    counts[q] = (int64_t)cnt;
    above[q] = (int64_t)ab;
    status[q] = st;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct IpRankPlan : IpPlanHead {
  size_t o_tau_hi, o_above, o_bad, o_x;
};

// Workspace layout (include/convdr_hip.h, "Score and rank of given rows": workspace; tests/golden/ip_rank_workspace_layout.json
// pins the totals).  The above counters follow the hit counters directly: k_rows_to_half zeroes both as one array.
static IpRankPlan ip_rank_plan(int np, int64_t n, int d, int cap) {
  IpRankPlan p{ip_plan_head(np, n)};
  WsCursor ws;
  p.o_qb = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qnorm = ws.take((size_t)p.nq_pad * 4);
  p.o_tau = ws.take((size_t)p.nq_pad * 4);
  p.o_tau_hi = ws.take((size_t)p.nq_pad * 4);
  p.o_counts = ws.take((size_t)p.nq_pad * IP_COUNT_STRIDE * 4);     // (nq_pad is a multiple of 128: no padding after it)
  p.o_above = ws.take((size_t)p.nq_pad * IP_COUNT_STRIDE * 4);
  p.o_m = ws.take((size_t)p.nq_pad * 4);
  p.o_bad = ws.take((size_t)p.nq_pad * 4);
  p.o_id = ws.take((size_t)np * cap * 4);
  p.o_s = ws.take((size_t)np * cap * 4);
  p.o_x = ws.take((size_t)np * cap * 8);
  p.total = ws.at;
  return p;
}

static int ip_score_rows_launch(const IpBlock& b, const float* q_f32, int nq, const int64_t* rows, int m, int64_t ld, double* X,
                                float* D, hipStream_t st) {
  const int chunks = m < 4 ? 1 : (m / 4 < 1024 ? m / 4 : 1024);
  if (b.rows_q8())
    hipLaunchKernelGGL(k_ip_score_rows<int8_t>, dim3(nq, chunks), dim3(256), 0, st, q_f32, b.q8_rows(), b.n, b.d, rows, m, ld, X, D,
                       b.unscale());
  else if (b.rows_f16())
    hipLaunchKernelGGL(k_ip_score_rows<_Float16>, dim3(nq, chunks), dim3(256), 0, st, q_f32, (const _Float16*)b.p_half, b.n, b.d, rows,
                       m, ld, X, D, b.unscale());
  else
    hipLaunchKernelGGL(k_ip_score_rows<float>, dim3(nq, chunks), dim3(256), 0, st, q_f32, b.p_f32, b.n, b.d, rows, m, ld, X, D,
                       b.unscale());
  CONVDR_CHECK_LAUNCH("k_ip_score_rows");
  return 0;
}

// Document rank (ip_docrank.hpp, convdr_ip_rank_docs): the same pipeline with the marking scan and its own finish.
struct RankDocs {
  const uint32_t* ord;       // [n] the rows' document ordinals (convdr_doc_ordinals)
  int64_t ndocs;
};
constexpr IpDepth IP_RANK_DOCS = {"convdr_ip_rank_docs", 1024, 131072, false};
static inline int64_t docrank_mark_words(int64_t ndocs) { return ceil_div64(ndocs, 32 * 32) * 32; }   // whole 128-byte lines
static inline size_t docrank_mark_bytes(int np, int64_t ndocs) { return align_up((size_t)np * docrank_mark_words(ndocs) * 4, 256); }
struct DocRankFinish {       // what the two finishing launches read and write (ip_docrank.hpp)
  int np, cap;
  int64_t n;
  const uint32_t *hits, *above_u, *bad, *list_id;
  const double* list_x;
  const int64_t* target;
  const double* xt;
  IpBand band;
  const uint32_t* ord;
  int64_t ndocs, mark_words;
  uint32_t* marks;
  int64_t *rank, *counts, *above;
  int32_t* status;
};
static int ip_docrank_finish(const DocRankFinish& f, hipStream_t st);

// The pipeline behind convdr_ip_rank_rows (depth = IP_RANK, docs = NULL) and convdr_ip_rank_docs (IP_RANK_DOCS, the ordinals):
// every check of its arguments, then the launches.  b.store is in range.
static int ip_rank_rows(const IpDepth& depth, const IpBlock& b, const float* q_f32, int np, const int64_t* target, const float* centre,
                        int cap, void* workspace, size_t workspace_bytes, int64_t* rank, double* X, int64_t* counts, int64_t* above,
                        int32_t* status, const RankDocs* docs, hipStream_t st) {
  const char* name = depth.entry;
  if (int e = ip_check_sizes(depth, np, b.n, b.d, 0, cap)) return e;
  CONVDR_REQUIRE(!docs || (docs->ndocs >= 0 && docs->ndocs <= b.n), "%s: ndocs=%lld outside [0, n=%lld]", name,
                 docs ? (long long)docs->ndocs : 0ll, (long long)b.n);
  CONVDR_REQUIRE(!b.rows_f16() || centre == nullptr, "%s: the half store has no centre", name);
  CONVDR_REQUIRE(b.row_bits != nullptr || b.row_bits_words == 0, "%s: row_bits is NULL but row_bits_words=%lld", name,
                 (long long)b.row_bits_words);
  CONVDR_REQUIRE(!b.row_bits || (b.n_allowed >= 0 && b.n_allowed <= b.n), "%s: n_allowed=%lld outside [0, n=%lld]", name,
                 (long long)b.n_allowed, (long long)b.n);
  if (int e = ip_check_block(name, b)) return e;
  const IpRankPlan p = ip_rank_plan(np, b.n, b.d, cap);
  const size_t mark_bytes = docs ? docrank_mark_bytes(np, docs->ndocs) : 0;       // the bitmap follows the rank plan's regions
  if (int e = ip_check_workspace(name, workspace_bytes, p.total + mark_bytes)) return e;
  CONVDR_REQUIRE(q_f32 && target && workspace && rank && X && counts && above && status,
                 "%s: a NULL argument (q_f32, target, workspace, rank, X, counts, above, status)", name);
  CONVDR_REQUIRE(!docs || docs->ord || b.n == 0, "%s: ord is NULL (the rows' document ordinals: convdr_doc_ordinals)", name);
  CONVDR_REQUIRE(b.n == 0 || (b.p_half && b.p_max_norm && (b.rows_f16() || b.p_f32)),
                 "%s: a NULL block pointer (p_half, p_max_norm; p_f32 unless store = 2)", name);
  char* ws = (char*)workspace;
  float* qnorm = (float*)(ws + p.o_qnorm);
  float* tau_lo = (float*)(ws + p.o_tau);
  float* tau_hi = (float*)(ws + p.o_tau_hi);
  uint32_t* hits = (uint32_t*)(ws + p.o_counts);
  uint32_t* above_u = (uint32_t*)(ws + p.o_above);
  uint32_t* m = (uint32_t*)(ws + p.o_m);
  uint32_t* bad = (uint32_t*)(ws + p.o_bad);
  uint32_t* list_id = (uint32_t*)(ws + p.o_id);
  double* list_x = (double*)(ws + p.o_x);
  CONVDR_REQUIRE(p.o_above == p.o_counts + (size_t)p.nq_pad * IP_COUNT_STRIDE * 4, "%s: counter arrays not adjacent", name);

  if (int e = ip_prepare_queries(b, p, ws, q_f32, np, nullptr, st, 2)) return e;   // (one pass: no remainders; hits and above zeroed)
  // the targets' canonical scores, straight into the caller's X (an id outside [0, n): the padding score, nothing read)
  if (int e = ip_score_rows_launch(b, q_f32, np, target, 1, 1, X, nullptr, st)) return e;
  // (n == 0: every target is outside the block and p_max_norm may be NULL -- the kernel reads it for valid targets only)
  hipLaunchKernelGGL(k_ip_band_tau, dim3((np + 3) / 4), dim3(256), 0, st, q_f32, np, b.d, centre, X, target, b.n, b.band(qnorm),
                     b.kind() == IP_KIND_F16 ? 1 : 0, tau_lo, tau_hi, bad);
  CONVDR_CHECK_LAUNCH("k_ip_band_tau");
  const bool scan = b.n > 0 && !(b.row_bits && b.n_allowed == 0);     // (no allowed row: nothing precedes any target)
  uint32_t* marks = (uint32_t*)(ws + p.total);
  const int64_t mark_words = docs ? docrank_mark_words(docs->ndocs) : 0;
  if (mark_bytes) CONVDR_CHECK_HIP(hipMemsetAsync(marks, 0, mark_bytes, st));       // zeroed in the call, on the stream
  if (scan) {
    ScanArgs a = ip_scan_args(b, p, ws, np, cap, nullptr, nullptr);
    a.tau_hi = tau_hi;
    a.above = above_u;
    if (docs) {
      a.ord = docs->ord;  a.ndocs = docs->ndocs;  a.marks = marks;  a.mark_words = mark_words;
      if (int e = launch_scan_mark(a, p.big, b.kind(), st)) return e;
    } else {
      if (int e = launch_scan_band(a, p.big, b.kind(), st)) return e;
    }
  }
  hipLaunchKernelGGL(k_ip_range_clamp, dim3((np + 255) / 256), dim3(256), 0, st, hits, np, cap, m);
  CONVDR_CHECK_LAUNCH("k_ip_range_clamp");
  if (scan) {
    ProfScope prof("ip_rank_rescore", st);
    if (int e = ip_rescore(b, q_f32, np, np < 64 ? 128 : 16, cap, m, list_id, list_x, st)) return e;
  }
  if (docs) {
    ProfScope prof("ip_docrank_finish", st);
    const DocRankFinish f = {np, cap, b.n, hits, above_u, bad, list_id, list_x, target, X, b.band(qnorm), docs->ord, docs->ndocs,
                             mark_words, marks, rank, counts, above, status};
    if (int e = ip_docrank_finish(f, st)) return e;
  } else {
    ProfScope prof("ip_rank_finish", st);
    hipLaunchKernelGGL(k_ip_rank_finish, dim3(np), dim3(IP_RANK_THREADS), 0, st, cap, b.n, hits, above_u, bad, list_id, list_x, target,
                       X, b.band(qnorm), rank, counts, above, status);
    CONVDR_CHECK_LAUNCH("k_ip_rank_finish");
  }
  return 0;
}

}  // namespace convdr

extern "C" int convdr_ip_score_rows(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale,
                                    int64_t n, int d, const int64_t* rows, int m, int64_t ld, double* X, float* D,
                                    convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_score_rows";
  CONVDR_REQUIRE(store >= 0 && store <= 2, "%s: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) (got %d)", name, store);
  CONVDR_REQUIRE(nq >= 0 && m >= 0 && ld >= m, "%s: bad sizes nq=%d m=%d ld=%lld (ld >= m)", name, nq, m, (long long)ld);
  CONVDR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: bad block size n=%lld (0 <= n < 2^31)", name, (long long)n);
  CONVDR_REQUIRE(d > 0 && d % 64 == 0 && d <= 4096, "%s: need d %% 64 == 0 and d <= 4096 (got %d)", name, d);
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, nullptr, nullptr, 0, 0};
  if (int e = ip_check_block(name, b)) return e;
  if (nq == 0 || m == 0) return 0;
  CONVDR_REQUIRE(q_f32 && rows, "%s: a NULL argument (q_f32, rows)", name);
  CONVDR_REQUIRE(n == 0 || (b.rows_f16() ? p_half != nullptr : p_f32 != nullptr),
                 "%s: a NULL block pointer (p_f32; p_half for store = 2)", name);
  if (!X && !D) return 0;
  return ip_score_rows_launch(b, q_f32, nq, rows, m, ld, X, D, (hipStream_t)stream);
}

extern "C" size_t convdr_ip_rank_workspace_bytes(int np, int64_t n, int d, int cap) {
  using namespace convdr;
  if (ip_check_sizes(IP_RANK, np, n, d, 0, cap)) return 0;
  return ip_rank_plan(np, n, d, cap).total;
}

extern "C" int convdr_ip_rank_rows(int store, const float* q_f32, int np, const int64_t* target, const float* p_f32,
                                   const void* p_half, float p_scale, const float* centre, int64_t n, int d,
                                   const float* p_max_norm, const uint32_t* row_bits, int64_t row_bits_words, int64_t n_allowed,
                                   int cap, void* workspace, size_t workspace_bytes, int64_t* rank, double* X, int64_t* counts,
                                   int64_t* above, int32_t* status, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(store >= 0 && store <= 2, "convdr_ip_rank_rows: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) "
                 "(got %d)", store);
  // (one pass: no remainder copy)
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, p_max_norm, row_bits, row_bits_words,
                     row_bits ? n_allowed : n};
  return ip_rank_rows(IP_RANK, b, q_f32, np, target, centre, cap, workspace, workspace_bytes, rank, X, counts, above, status, nullptr,
                      (hipStream_t)stream);
}
