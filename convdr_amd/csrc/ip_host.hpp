// Host side of the search entries, included by ip_topk.hip after the kernel headers (ip_scan.hpp, ip_select.hpp); ip_deep.hpp and
// ip_range.hpp follow with their pipelines.  The map of all three: DESIGN.md section 4, "Host side of the search entries".
#pragma once

namespace convdr {

// ---- the block a call searches (fields in the order of the entries' arguments: they initialise it positionally) ----------
struct IpBlock {
  int store;                  // 0: bf16 scan copy, 1: fp16 scan copy, 2: half store (the halves are corpus and scan operand),
                              // 3: 8-bit store (p_half: rows of d int8 codes, corpus and scan operand; q8_centre, q8_step)
  const float* p_f32;         // [n, d] fp32 rows the re-score reads; not read for the half store
  const void* p_half;         // [n, d] 16-bit scan operand; the half store: the stored rows 2^s v
  const void* p_half_lo;      // [n, d] remainder copy (the three-pass split scan), or NULL
  float p_scale;              // power of two the fp16 operand was scaled by; 1 for the bf16 copy
  bool two_pass;              // half store: S~ = P Qh + P Ql, no remainder copy
  int64_t n;
  int d;
  const float* p_max_norm;    // device: largest UNSCALED row norm
  const uint32_t* row_bits;   // row filter (NULL: every row), one bit per row, whole 256-row tiles
  int64_t row_bits_words;     // words the caller says the bitmap holds (checked against n, then not read)
  int64_t n_allowed;          // set bits among rows 0..n-1 (top-k only; read only with row_bits)
  const float* q8_centre = nullptr;   // 8-bit store: [d] each; p_max_norm is then the largest row L1 norm of the codes
  const float* q8_step = nullptr;

  int kind() const { return store == 3 ? IP_KIND_I8 : (store == 0 ? IP_KIND_BF16 : IP_KIND_F16); }
  bool rows_q8() const { return store == 3; }                             // the re-score reads codes, centre and step
  IpQ8Rows q8_rows() const { return {(const int8_t*)p_half, q8_centre, q8_step}; }
  bool rows_f16() const { return store == 2; }                            // the re-score reads p_half
  bool split() const { return p_half_lo != nullptr || two_pass; }         // the query's remainder is an operand: the tighter band
  float scan_scale() const { return kind() == IP_KIND_F16 ? p_scale : 1.f; }   // units of the scan scores and thresholds
  float norm_limit() const { return kind() == IP_KIND_F16 ? IP_F16_NORM_LIMIT : (kind() == IP_KIND_I8 ? FLT_MAX : INFINITY); }   // above it: CONVDR_IP_RANGE
  float norm_floor() const { return kind() == IP_KIND_BF16 ? IP_BF16_NORM_FLOOR : 0.f; }       // non-zero and below it: CONVDR_IP_RANGE
  double unscale() const { return rows_f16() ? 1.0 / (double)p_scale : 1.0; }  // one factor on the fp64 sum over scaled rows
  int64_t n_need() const { return row_bits ? n_allowed : n; }   // TOP-K ONLY (range search sets no n_allowed): need = min(k, n_need)
  float eps_coef() const { return ip_eps_coef(d, split(), kind()); }
  float eps_abs() const { return ip_eps_abs(d, split(), kind()); }
  // the error band of this block's scan scores for queries whose norms are at qnorm (device, [nq]): what every finishing kernel takes
  // (8-bit store: qnorm holds A(q), +inf for a query out of range, and the coefficient of the L1 norm replaces the other two)
  IpBand band(const float* qnorm) const {
    if (rows_q8()) return {qnorm, p_max_norm, 0.f, 0.f, 1.f, norm_limit(), 0.f, IP_Q8_COEF};
    return {qnorm, p_max_norm, eps_coef(), eps_abs(), scan_scale(), norm_limit(), norm_floor()};
  }
};

// per-call arguments of the seven top-k entries, in the entries' order
struct IpTopkArgs {
  const float* q_f32;
  int nq, k;
  const float* tau_in;
  int cap, rank_target;
  void* workspace;
  size_t workspace_bytes;
  float* D; int64_t* I; int32_t* status; float* tau_retry;   // outputs: D, I [nq, k]; status, tau_retry [nq]
  hipStream_t st;
};

// ---- argument checks, one copy each.  Size messages carry the depth's base entry, all others the called entry's name ----
struct IpDepth { const char* entry; int min_cap, max_cap; bool top_k; };    // top_k: k is an argument, 1 <= k <= cap / 2
constexpr IpDepth IP_SHALLOW = {"convdr_ip_search", 1024, 8192, true};              // lists and bands in LDS
constexpr IpDepth IP_DEEP = {"convdr_ip_search_deep", 16384, 131072, true};         // lists in global memory (ip_deep.hpp)
constexpr IpDepth IP_RANGE = {"convdr_ip_range_search", 1024, 131072, false};       // range search: no k (ip_range.hpp)
constexpr IpDepth IP_RANK = {"convdr_ip_rank_rows", 1024, 131072, false};           // rank of given rows: no k (ip_rank.hpp)

static int ip_check_sizes(const IpDepth& depth, int nq, int64_t n, int d, int k, int cap) {
  CONVDR_REQUIRE(nq > 0, "%s: bad sizes nq=%d", depth.entry, nq);
  CONVDR_REQUIRE(k > 0 || !depth.top_k, "%s: bad sizes k=%d", depth.entry, k);
  CONVDR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: bad block size n=%lld (0 <= n < 2^31)", depth.entry, (long long)n);
  CONVDR_REQUIRE(d > 0 && d % 64 == 0 && d <= 4096, "%s: need d %% 64 == 0 and d <= 4096 (got %d)", depth.entry, d);
  CONVDR_REQUIRE(cap >= depth.min_cap && cap <= depth.max_cap && (cap & (cap - 1)) == 0,
                 "%s: cap must be a power of two in [%d, %d] (got %d)", depth.entry, depth.min_cap, depth.max_cap, cap);
  CONVDR_REQUIRE(!depth.top_k || k <= cap / 2, "%s: k=%d too large for cap=%d", depth.entry, k, cap);
  return 0;
}

static bool ip_pow2_scale_ok(float s) {   // a finite power of two
  int ex = 0;
  return s > 0.f && s < INFINITY && frexpf(s, &ex) == 0.5f;
}

// The block's own arguments.  Scale: 1 for the bf16 copy (the entries pass it); the half store's copy is 2^s v with s >= 0.
// Bitmap: one that is there -- whether it may be absent is the entry's rule (filtered top-k: no; range search: NULL, 0).
static int ip_check_block(const char* name, const IpBlock& b) {
  CONVDR_REQUIRE(b.store != 3 || (b.d % 128 == 0 && b.d <= IP_Q8_MAX_D),
                 "%s: the 8-bit store needs d %% 128 == 0 and d <= %d (got %d): one K step is 128 codes, and the integer scan's "
                 "range is proven up to that width", name, IP_Q8_MAX_D, b.d);
  CONVDR_REQUIRE(b.store != 3 || b.n == 0 || (b.p_half && b.q8_centre && b.q8_step && b.p_max_norm),
                 "%s: a NULL block pointer (codes, centre, step, max_l1)", name);
  CONVDR_REQUIRE(ip_pow2_scale_ok(b.p_scale) && (b.store != 2 || b.p_scale >= 1.f), "%s: p_scale must be a power of two%s (got %g)",
                 name, b.store == 2 ? " >= 1" : "", (double)b.p_scale);
  if (!b.row_bits) return 0;
  CONVDR_REQUIRE(((uintptr_t)b.row_bits & 15u) == 0, "%s: row_bits must be 16-byte aligned (the scan reads four words at a time)",
                 name);
  const int64_t words = ceil_div64(b.n, 256) * 8;
  CONVDR_REQUIRE(b.row_bits_words >= words, "%s: the bitmap holds %lld words, n=%lld rows need %lld (whole 256-row tiles, zero padded)",
                 name, (long long)b.row_bits_words, (long long)b.n, (long long)words);
  return 0;
}

static int ip_check_workspace(const char* name, size_t have, size_t need) {
  CONVDR_REQUIRE(have >= need, "%s: workspace too small (%zu < %zu)", name, have, need);
  return 0;
}

// ---- workspace plans: the head the three plans share and the cursor that lays regions out.  Each plan takes its regions
// itself, in its own order (tests/golden/ip_workspace_layout.json pins the sizes and the offsets that have an accessor).
struct IpPlanHead {
  int big;           // scan tile class: IP_TILE_256 (more than 128 queries), IP_TILE_TALL (256 passages x 128 queries: the
                     // HBM-bound regime)
  int tr, tl;        // tile extent over passages / queries
  int nq_pad, nQt, nPt;
  size_t o_qb, o_qnorm, o_tau, o_counts, o_m, o_id, o_s, total;
};

static IpPlanHead ip_plan_head(int nq, int64_t n) {   // the tiling; the offsets are the plan's to fill
  IpPlanHead p{};
  p.big = nq > 128 ? IP_TILE_256 : IP_TILE_TALL;
  p.tr = Tile256::TR;   // = TileTall::TR
  p.tl = p.big == IP_TILE_256 ? Tile256::TL : TileTall::TL;
  p.nq_pad = (nq + p.tl - 1) / p.tl * p.tl;
  p.nQt = p.nq_pad / p.tl;
  p.nPt = (int)ceil_div64(n, p.tr);
  return p;
}

// Regions in the order they are taken, each starting on a 256-byte boundary; `at` ends as the plan's total.
struct WsCursor {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t start = at; at = align_up(at + bytes, 256); return start; }
};

struct IpPlan : IpPlanHead {
  int mode;          // -1: no threshold pass (n <= cap), else IP_MODE_FULL / IP_MODE_TOP2
  int nSt, stride;   // sampled passage tiles / tile stride
  int64_t nvals;     // values per query handed to k_tau_select
  int npow2;
  size_t o_qlo, o_counts_packed, o_T, o_x;
};

// Layout as before the shared head: qb|qlo|qnorm|tau|counts|counts_packed|m|T|id|s|x, same sizes (T, id, s: convdr_ip_debug_sample /
// convdr_ip_debug_list; x: no accessor).
static IpPlan ip_plan(int nq, int64_t n, int d, int cap) {
  IpPlan p{ip_plan_head(nq, n)};
  p.nSt = 0; p.stride = 1; p.nvals = 0; p.npow2 = 2;
  if (n <= cap) {
    p.mode = -1;
  } else if (n <= IP_FULL_MAX_N) {
    p.mode = IP_MODE_FULL; p.nSt = p.nPt; p.nvals = n;
  } else {
    p.mode = IP_MODE_TOP2;
    int64_t S = n / 32;
    if (S < IP_SAMPLE_MIN) S = IP_SAMPLE_MIN;
    if (S > IP_SAMPLE_MAX) S = IP_SAMPLE_MAX;
    p.nSt = (int)(S / p.tr);
    if (p.nSt > p.nPt) p.nSt = p.nPt;
    p.stride = p.nPt / p.nSt;
    p.nvals = (int64_t)p.nSt * 8;   // WR * 2 halves * 2 values per tile, WR = 2 for both tile shapes
  }
  while (p.npow2 < p.nvals) p.npow2 <<= 1;
  WsCursor ws;
  p.o_qb = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qlo = ws.take((size_t)p.nq_pad * d * 2);
  p.o_qnorm = ws.take((size_t)p.nq_pad * 4);
  p.o_tau = ws.take((size_t)p.nq_pad * 4);
  p.o_counts = ws.take((size_t)p.nq_pad * IP_COUNT_STRIDE * 4);
  p.o_counts_packed = ws.take((size_t)p.nq_pad * 4);
  p.o_m = ws.take((size_t)p.nq_pad * 4);
  const size_t t_rows = p.mode == IP_MODE_FULL ? (size_t)p.nPt * p.tr : (size_t)p.nvals;
  p.o_T = ws.take(t_rows * p.nq_pad * 4);
  p.o_id = ws.take((size_t)nq * cap * 4);
  p.o_s = ws.take((size_t)nq * cap * 4);
  p.o_x = ws.take((size_t)nq * cap * 8);
  p.total = ws.at;
  return p;
}

// ---- steps every pipeline runs -------------------------------------------------------------------------------------------
// Queries -> 16-bit operands and norms (fp16: scaled row by row); the kernel also zeroes the padding rows and the hit
// counters.  qlo: where the remainders go, NULL when the scan has no use for them.
// counter_sets: how many [nq_pad x IP_COUNT_STRIDE] counter arrays follow each other at o_counts (the rank plan: hits, above).
static int ip_prepare_queries(const IpBlock& b, const IpPlanHead& p, char* ws, const float* q_f32, int nq, bf16_t* qlo,
                              hipStream_t st, int counter_sets = 1) {
  bf16_t* qb = (bf16_t*)(ws + p.o_qb);
  float* qnorm = (float*)(ws + p.o_qnorm);
  uint32_t* counts = (uint32_t*)(ws + p.o_counts);
  const int64_t n_count = (int64_t)p.nq_pad * IP_COUNT_STRIDE * counter_sets;
  if (b.kind() == IP_KIND_I8) {   // hi / lo int8 operands, interleaved, in the place of qb (2 nq_pad rows of d bytes); A(q) for the norm
    hipLaunchKernelGGL(k_q8_queries, dim3((p.nq_pad + 3) / 4), dim3(256), 0, st, q_f32, (int64_t)nq, b.d, b.q8_centre, b.q8_step,
                       (int8_t*)qb, qnorm, (int64_t)p.nq_pad, counts, n_count);
    CONVDR_CHECK_LAUNCH("k_q8_queries");
    return 0;
  }
  if (b.kind() == IP_KIND_F16)
    hipLaunchKernelGGL((k_rows_to_half<IP_KIND_F16, true>), dim3((p.nq_pad + 3) / 4), dim3(256), 0, st, q_f32, (int64_t)nq, b.d,
                       (const float*)nullptr, 1.f, qb, qlo, qnorm, (float*)nullptr, (int64_t)p.nq_pad, counts, n_count);
  else
    hipLaunchKernelGGL((k_rows_to_half<IP_KIND_BF16, false>), dim3((p.nq_pad + 3) / 4), dim3(256), 0, st, q_f32, (int64_t)nq, b.d,
                       (const float*)nullptr, 1.f, qb, qlo, qnorm, (float*)nullptr, (int64_t)p.nq_pad, counts, n_count);
  CONVDR_CHECK_LAUNCH("k_rows_to_half(Q)");
  return 0;
}

// A threshold that needs no estimate: the caller's tau_in [nq] (a retry), or -inf -- every row is a candidate.
static int ip_given_tau(const IpPlanHead& p, char* ws, const float* tau_in, int nq, hipStream_t st) {
  float* tau = (float*)(ws + p.o_tau);
  if (tau_in) {
    CONVDR_CHECK_HIP(hipMemcpyAsync(tau, tau_in, (size_t)nq * 4, hipMemcpyDeviceToDevice, st));
  } else {
    hipLaunchKernelGGL(k_fill_f32, dim3((p.nq_pad + 255) / 256), dim3(256), 0, st, tau, p.nq_pad, -INFINITY);
    CONVDR_CHECK_LAUNCH("k_fill_f32");
  }
  return 0;
}

// The emitting scan of the whole block.  The sampling scans start from a copy and narrow P, n, nPt, pt_stride and T.
static ScanArgs ip_scan_args(const IpBlock& b, const IpPlanHead& p, char* ws, int nq, int cap, const bf16_t* qlo, float* T) {
  ScanArgs a{};
  a.P = (const bf16_t*)b.p_half;        a.Plo = (const bf16_t*)b.p_half_lo;     // passage operands, [n, d]
  a.Qb = (const bf16_t*)(ws + p.o_qb);  a.Qlo = qlo;                            // query operands, [nq_pad, d]
  a.n = b.n;  a.d = b.d;  a.nq = nq;  a.nq_pad = p.nq_pad;
  a.nQt = p.nQt;  a.nPt = p.nPt;  a.pt_stride = 1;                              // every tile of the block
  a.tau = (const float*)(ws + p.o_tau);  a.counts = (uint32_t*)(ws + p.o_counts);         // thresholds in, hit counters out
  a.cand_id = (uint32_t*)(ws + p.o_id);  a.cand_s = (float*)(ws + p.o_s);  a.cap = cap;   // the list: [nq, cap] each
  a.T = T;                                                                      // the sample's scores (the sampling scans)
  a.two_pass = b.two_pass ? 1 : 0;
  a.bits = b.row_bits;
  if (b.kind() == IP_KIND_I8) {   // rows of d int8 are rows of d / 2 16-bit words to the staging; query tiles of 128 (ip_scan_q8.hpp)
    a.d = b.d / 2;  a.nQt = (nq + 127) / 128;  a.Plo = nullptr;  a.Qlo = nullptr;  a.two_pass = 0;
  }
  return a;
}

// Canonical fp64 scores of the first m[q] ids of every query's list -> x.  The half store's rows are its halves, and the sum
// over the scaled rows is multiplied by 1 / p_scale once.  waves: the grid's second dimension, the caller's choice.
static int ip_rescore(const IpBlock& b, const float* q_f32, int nq, int waves, int cap, const uint32_t* m, const uint32_t* ids,
                      double* x, hipStream_t st) {
  if (b.rows_q8())
    hipLaunchKernelGGL(k_ip_rescore<int8_t>, dim3(nq, waves), dim3(256), 0, st, q_f32, b.q8_rows(), b.d, cap, m, ids, x, b.unscale());
  else if (b.rows_f16())
    hipLaunchKernelGGL(k_ip_rescore<_Float16>, dim3(nq, waves), dim3(256), 0, st, q_f32, (const _Float16*)b.p_half, b.d, cap, m, ids,
                       x, b.unscale());
  else
    hipLaunchKernelGGL(k_ip_rescore<float>, dim3(nq, waves), dim3(256), 0, st, q_f32, b.p_f32, b.d, cap, m, ids, x, b.unscale());
  CONVDR_CHECK_LAUNCH("k_ip_rescore");
  return 0;
}

// ---- the shallow pipeline: k <= 4,096, lists and bands in LDS.  p plans the arguments ip_topk validated. ----------------
// The row filter: the scan emits allowed rows only and samples -inf for the others; the finishing kernels take n_allowed where
// they took n; n_allowed <= cap: every allowed row is a candidate -- no threshold pass, tau = -inf.
static int ip_search(const char* name, const IpBlock& b, const IpTopkArgs& c, const IpPlan& p) {
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
  uint32_t* cand_id = (uint32_t*)(ws + p.o_id);
  float* cand_s = (float*)(ws + p.o_s);
  double* cand_x = (double*)(ws + p.o_x);
  uint32_t* band_m = (uint32_t*)(ws + p.o_m);
  bf16_t* qlo = b.split() ? (bf16_t*)(ws + p.o_qlo) : nullptr;
  const bool all_candidates = p.mode < 0 || (b.row_bits && b.n_allowed <= cap);

  if (int e = ip_prepare_queries(b, p, ws, c.q_f32, nq, qlo, st)) return e;
  const ScanArgs emit = ip_scan_args(b, p, ws, nq, cap, qlo, T);
  if (n == 0 || c.tau_in || all_candidates) {   // (an empty block is not scanned: -inf, whatever tau_in is)
    if (int e = ip_given_tau(p, ws, n > 0 ? c.tau_in : nullptr, nq, st)) return e;
  } else {
    int R = c.rank_target > 0 ? c.rank_target : 16 * k;
    if (R > cap / 2) R = cap / 2;
    if (R < k) R = k;
    int r;
    ScanArgs a = emit;   // the sample: every stride-th tile
    a.nPt = p.nSt;
    a.pt_stride = p.stride;
    if (p.mode == IP_MODE_FULL) {
      r = (int64_t)R < n ? R : (int)n;
      if (int e = launch_scan<IP_MODE_FULL>(a, p.big, b.kind(), st)) return e;
    } else {
      // The sample keeps the two best scores of every 64 sampled passages, so it can only represent a rank whose expected
      // hits per 64 passages stay well below 2: R <= n / 128 (half a hit per 64).  Blocks of 32 k .. 200 k passages
      // therefore aim at a lower rank than 16 k (n = 47,104 asked for rank 1,113 of a 1,024-value sample: no threshold,
      // every passage emitted, every query overflowed and was re-run); a band that then reaches below the threshold
      // comes back UNCERTAIN with the threshold to retry, as for any clustered block.
      if ((int64_t)R > n / 128) R = (int)(n / 128 > k ? n / 128 : k);
      const double frac = (double)p.nSt * p.tr / (double)n;
      r = (int)lrint(R * frac);
      if (r < 8) r = 8;
      if (r > p.nvals / 4) r = (int)(p.nvals / 4);
      if (int e = launch_scan<IP_MODE_TOP2>(a, p.big, b.kind(), st)) return e;
    }
    static DeviceOnce attr_done;
    if (attr_done.first())
      CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_tau_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           IP_FULL_MAX_N * 4));
    hipLaunchKernelGGL(k_tau_select, dim3(nq), dim3(1024), (size_t)p.npow2 * 4, st, T, p.nvals, p.nq_pad, r, tau);
    CONVDR_CHECK_LAUNCH("k_tau_select");
  }
  if (n > 0)
    if (int e = launch_scan<IP_MODE_EMIT>(emit, p.big, b.kind(), st)) return e;
  static DeviceOnce attr_done2;
  if (attr_done2.first()) {
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_cut, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8));
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_select, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 12));
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_finish<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 16));
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_finish<_Float16>, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 16));
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_ip_finish<int8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 16));
  }
  if (g_ip_fused_finish && n > 0) {
    ProfScope prof("ip_finish", st);
    if (b.rows_q8())
      hipLaunchKernelGGL(k_ip_finish<int8_t>, dim3(nq), dim3(IP_SELECT_THREADS), (size_t)cap * 16, st, b.n_need(), k, cap, counts, counts_packed,
                         cand_id, cand_s, tau, b.band(qnorm), c.q_f32, b.q8_rows(), b.d, band_m, c.status, c.tau_retry, c.D, c.I,
                         b.unscale());
    else if (b.rows_f16())
      hipLaunchKernelGGL(k_ip_finish<_Float16>, dim3(nq), dim3(IP_SELECT_THREADS), (size_t)cap * 16, st, b.n_need(), k, cap, counts, counts_packed,
                         cand_id, cand_s, tau, b.band(qnorm), c.q_f32, (const _Float16*)b.p_half, b.d, band_m, c.status, c.tau_retry,
                         c.D, c.I, b.unscale());
    else
      hipLaunchKernelGGL(k_ip_finish<float>, dim3(nq), dim3(IP_SELECT_THREADS), (size_t)cap * 16, st, b.n_need(), k, cap, counts, counts_packed,
                         cand_id, cand_s, tau, b.band(qnorm), c.q_f32, b.p_f32, b.d, band_m, c.status, c.tau_retry, c.D, c.I, b.unscale());
    CONVDR_CHECK_LAUNCH("k_ip_finish");
    return 0;
  }
  {
    ProfScope prof("ip_cut", st);
    hipLaunchKernelGGL(k_ip_cut, dim3(nq), dim3(1024), (size_t)cap * 8, st, b.n_need(), k, cap, counts, counts_packed, cand_id, cand_s,
                       tau, b.band(qnorm), band_m, c.status, c.tau_retry);
    CONVDR_CHECK_LAUNCH("k_ip_cut");
  }
  if (n > 0) {
    ProfScope prof("ip_rescore", st);
    if (int e = ip_rescore(b, c.q_f32, nq, 16, cap, band_m, cand_id, cand_x, st)) return e;
  }
  ProfScope prof("ip_select", st);
  hipLaunchKernelGGL(k_ip_select, dim3(nq), dim3(IP_SELECT_THREADS), (size_t)cap * 12, st, k, cap, band_m, cand_id, cand_x, c.D, c.I);
  CONVDR_CHECK_LAUNCH("k_ip_select");
  return 0;
}

}  // namespace convdr
