// Exact brute-force inner-product top-k over a resident passage-embedding block (gfx950).
//
// Replaces faiss.IndexFlatIP.add/.search as driven by the reference at
//   /root/reference/drivers/run_convdr_inference.py:180-182  (gpu_index.add(block); D, I = gpu_index.search(Q, topN))
//
// Design (see DESIGN.md §"IP scan"): never materialise [nq, n].
//   prepare   fp32 block -> bf16 scan copy + max row norm                      (HBM-bound, once per .add)
//   sample    bf16 MFMA GEMM over ~1/32 of the block, epilogue keeps per-(query, 32 passages) top-2,
//             per-query radix select in LDS -> tau[q] ~ score of rank `rank_target` in the whole block
//   scan      persistent bf16 MFMA GEMM  P_bf16[n,d] * Q_bf16[nq,d]^T  (gemm_nt.hpp); epilogue: each lane (= query)
//             counts the accumulators >= tau[q], reserves that many slots of the query's candidate list with one
//             atomic and writes (index, score) of its hits
//   cut       per query: k-th largest scan score by radix select, band {S~ >= S~(k) - 2 eps} moved to the front,
//             certificate OK iff the list is complete down to the cut (cut >= tau, no overflow),
//             eps = 0.0079 * |q| * max|p - centre|   (bf16 rounding bound)
//   rescore   one wave per band candidate: fp64 dot of the fp32 originals, canonical order (oracle/search.py)
//   select    per query: the k best exact scores (radix select + bitonic sort of the survivors by
//             (exact score desc, index asc))
#include "gemm_nt.hpp"

#include <float.h>
#include <math.h>

#include "../../include/convdr_hip.h"

namespace convdr {

constexpr int IP_MODE_FULL = 0, IP_MODE_TOP2 = 1, IP_MODE_EMIT = 2, IP_MODE_BAND = 3, IP_MODE_MARK = 4;
constexpr int IP_FULL_MAX_N = 32768;      // <= this many passages: "sample" = all scores, exact rank select
constexpr int IP_SAMPLE_MIN = 32768;      // sampled passages (>= 1/32 of the block)
constexpr int IP_SAMPLE_MAX = 262144;
// Error-band coefficients: |scan score - exact score| <= coef * |q| * max|p - centre| for every passage of the block.
// u = 2^-8 bounds the relative error of a bf16 rounding, the accumulation term charges 2^-23 per accumulated product
// (gamma_K of an fp32 sum whose per-step rounding is at worst truncation: the MFMA's internal rounding is not
// documented; it sums 8-16 products per step, so this over-counts) relative to sum |q_i p_i| <= |q| |p|.  Computed from d
// (round 1 used constants that only covered d <= 1024 with the 2^-24 model).
//   bf16 scan:        (1 + u)^2 - 1 = 2u + u^2          + d * 2^-23
//   split-bf16 scan:  hi*hi + hi*lo + lo*hi leaves out lo*lo and the two second-rounding remainders,
//                     each <= u^2 (1 + u) |q| |p|         + 3 d * 2^-23 (one accumulator chain over the three passes)
//   fp16 scan:        same forms with u = 2^-11 (8x tighter: 1.07e-3 at d = 768 in one pass, 2.8e-4 split) PLUS an absolute
//                     term: below 2^-14 a half has no relative precision.  Both operands are scaled by powers of two
//                     (exact; per block / per query) so that their norms sit near 2^12, and an element is charged
//                     eta = 2^-14 of absolute error -- which also covers hardware that flushes subnormal MFMA inputs:
//                     |fl(q) fl(p) - q p| summed over d  <=  rel |q||p| + eta (1 + u) sqrt(d) (|q| + |p|) + d eta^2
//                     (ip_eps_abs; ~1e-6 of |q||p| at these scales).  The scan then works entirely in scaled units:
//                     thresholds, candidate scores and eps; the results come from the fp64 re-scoring of the originals.
//   half store:      (the passages ARE halves, the resident copy 2^s v is exact: the passage operand has no error)
//                     one pass:   only the query rounds: u + d * 2^-23, and eta sqrt(d) |p| -- every term is one of the
//                                 fp16 scan's above, which is used unchanged (a superset, incl. flushed subnormal inputs)
//                     two passes: P Qh + P Ql leaves out the query's second-rounding remainder, <= u^2 (1 + u) |q| |p|, and
//                                 runs two accumulation chains, 2 d * 2^-23; Qh and Ql each carry eta.  Term by term below
//                                 the split scan's 3 u^2 (1 + 2u) + 3 d 2^-23 and 2 eta (1 + u) sqrt(d): used unchanged
constexpr int IP_KIND_BF16 = 0, IP_KIND_F16 = 1;
static inline float ip_eps_coef(int d, bool x3, int kind = IP_KIND_BF16) {
  const double u = kind == IP_KIND_F16 ? 1.0 / 2048.0 : 1.0 / 256.0, acc = (double)d / 8388608.0;
  const double c = x3 ? 3.0 * u * u * (1.0 + 2.0 * u) + 3.0 * acc : 2.0 * u + u * u + acc;
  return (float)(c * 1.0001);
}
constexpr double IP_F16_ETA = 1.0 / 16384.0;
static inline float ip_eps_abs(int d, bool x3, int kind) {   // multiplies (|q| + max|p|), scaled units
  if (kind != IP_KIND_F16) return 0.f;
  // split scan: hi and lo are both halfs; the remainder x - hi - lo carries at most eta as well
  return (float)((x3 ? 2.0 : 1.0) * IP_F16_ETA * (1.0 + 1.0 / 2048.0) * sqrt((double)d) * 1.0001);
}
constexpr float IP_F16_TARGET_EXP = 12.f;    // the block's scale puts its (first) max norm into [2^12, 2^13) (convdr_ip_f16_scale),
                                             // a query's own scale puts its norm into [2^11, 2^12) (k_rows_to_half<F16, true>)
constexpr float IP_F16_NORM_LIMIT = 60000.f; // scaled norms above this may hold elements that round to inf: CONVDR_IP_RANGE
// The bf16 scan does not rescale, and its bound has relative terms only.  k_rows_to_half<IP_KIND_BF16> rounds elements below
// 2^-126 to bf16 SUBNORMALS (quantum 2^-133, no relative precision), and products below 2^-126 lose bits in the fp32
// accumulator: in the operand-rounding model rows of elements ~2^-129 / 2^-131 / 2^-132 against a query of 2^40 whose signs
// follow their rounding errors miss the bound by 1.2x / 5.5x / 10x, and exact operands of ~3e-23 on both sides by 30x through
// the roundings of their products alone (tests/test_scan_error_cpu.py, family `tiny`).  So the bf16 kinds refuse a NON-ZERO
// norm below a floor -- IpBand::out_of_range, CONVDR_IP_RANGE:
//   operands   a subnormal rounding adds at most 2^-134 per element, sqrt(d) 2^-134 |q| per score (an MFMA that flushed
//              subnormal inputs: 2^-126, sqrt(d) 2^-126 |q|); that is negligible against u |q| pm when pm >> sqrt(d) 2^-127.
//   products   each product below 2^-126 loses at most 2^-150: d 2^-150 per score, negligible against the band when
//              |q| pm >> d 2^-143.  (An accumulator that flushed such products or partial sums loses less than d 2^-126 <=
//              2^-114: the + 1e-30f of IpBand::eps covers that at any norm.)
// With d <= 4096, a floor of 2^-60 on each norm gives pm >= 2^-60 = 2^61 sqrt(d) 2^-127 and |q| pm >= 2^-120 = 2^11 d 2^-143:
// more than 2^50 of margin on the operand term even if subnormal inputs were flushed, 2^11 on the product term.  2^-60 is 18
// orders of magnitude below any real embedding norm.  A zero norm stays in range: every score is exactly 0.  The fp16 kinds
// rescale both operands and are not affected (precision="auto" / "fp16" take such data).
constexpr float IP_BF16_NORM_FLOOR = 0x1p-60f;

// The 8-bit store (store 3, IP_KIND_I8): rows of int8 codes c_ij, |c_ij| <= 127; the corpus is v_ij = fl(centre_j + fl(step_j c_ij)).
// The scan is integer and exact: S_i = sum_j Qi_j c_ij with Qi_j = rint(fl(q_j step_j) / t) (k_q8_queries), handed on as the float
// S~_i = fl(S_i).  Its target is the exact scaled score E_i = (1 / t) sum_j q_j (v_ij - centre_j), which orders the rows of a
// query as q . v_i does (t > 0, q . centre the same for every row).  With u = 2^-24 and every step_j zero or a normal number
// (k_colstep_finish), so that each fp32 product below has relative error <= u:
//   rows      fl(step c) = step c (1 + d1), v = (centre + fl(step c)) (1 + d2), |d1|, |d2| <= u (an fp32 sum is exact in the
//             subnormal range), hence |v_ij - centre_j - step_j c_ij| <= u (|centre_j| + 127 (2 + u) step_j) =: u rho_j and
//             |E_i - (1 / t) sum_j q_j step_j c_ij| <= (u / t) sum_j |q_j| rho_j =: A(q)            (k_q8_queries, per query)
//   query     |Qi_j - q_j step_j / t| <= 1/2 + u (1 + 2u) 16256 + 2^-36: the rint, the rounding of q_j step_j relative to
//             |fl(q_j step_j)| / t <= 16256, and 2^-150 / t for a product in the subnormal range (t >= 2^-114: queries with
//             max |fl(q_j step_j)| below 2^-100 are CONVDR_IP_RANGE); times |c_ij| and summed: (1/2 + r0) ||c_i||_1
//   convert   |fl(S_i) - S_i| <= u |S_i| <= u 16256 ||c_i||_1
// Together |S~_i - E_i| <= (1/2 + r) max_i ||c_i||_1 + A(q),  r = u 16256 (2 + 2u) + 2^-36 = 0.00193787...; IpBand::eps adds its
// 1.001.  The largest row L1 norm is kept at add (only ever growing); nothing here depends on d.
// No integer overflows for d <= 1024 (ip_scan_q8.hpp): |S_i| <= 1024 x 127 x 16256 = 2,114,060,288 < 2^31.
constexpr int IP_KIND_I8 = 2;
constexpr int IP_Q8_MAX_D = 1024;
constexpr float IP_Q8_COEF = (float)((0.5 + (16256.0 * (2.0 + 0x1p-23) * 0x1p-24 + 0x1p-36)) * (1.0 + 1e-6));

}  // namespace convdr

// rows to 16-bit scan operands and norms, the half store, the column mean
#include "ip_prepare.hpp"
// the scan: arguments, row filter, epilogues, the two persistent kernels, launch_scan<MODE>
#include "ip_scan.hpp"
// the 8-bit store's scan: int8 codes against hi / lo int8 queries on the i8 MFMA, the same epilogues
#include "ip_scan_q8.hpp"
// order statistics, threshold select, cut / re-score / select / finish; the certificate (ip_certify.hpp)
#include "ip_select.hpp"
// the host side: block descriptor, argument checks, plan head, shared steps and the shallow pipeline (k <= 4096)
#include "ip_host.hpp"
// k > 4096: the same cut / re-score / select through global memory
#include "ip_deep.hpp"
// range search: every row scoring above a per-query radius (convdr_ip_range_*)
#include "ip_range.hpp"
// rank and score of given rows: the band-count scan (convdr_ip_score_rows, convdr_ip_rank_*)
#include "ip_rank.hpp"
// removing rows: stable in-place compaction of the resident buffers (convdr_ip_compact_*)
#include "ip_compact.hpp"
// row ids: a hash set of the listed keys, probed by every row of the id column (convdr_keyset_*, convdr_keys_*)
#include "ip_keys.hpp"
// documents by id: all rows of the listed keys as a CSR, the MaxP score of (query, document) pairs (convdr_keys_rows_*, convdr_ip_score_docs)
#include "ip_docs.hpp"
// per-query exclusion lists: the canonical rows, the drop from certified lists, the count of excluded rows ahead (convdr_excl_*, convdr_ip_excl_count_ahead)
#include "ip_exclude.hpp"
// document rank: dense document numbers of the id column, the marking band scan's finish (convdr_doc_ordinals, convdr_ip_rank_docs)
#include "ip_docrank.hpp"
// the digest a snapshot file is checked against, on the device and on the host (convdr_digest_rows, convdr_digest_host)
#include "ip_digest.hpp"
// judging a run against the qrels: labels, rank measures, negatives (convdr_run_*)
#include "run_judge.hpp"

using namespace convdr;

// two-way merge, W-way merge and distinct of lists in LDS (convdr_topk_merge*, convdr_topk_distinct)
#include "topk_lists.hpp"
// lists of up to 65,536 entries: the same two contracts through global memory (convdr_topk_distinct_deep, convdr_topk_merge_deep*)
#include "topk_deep.hpp"

extern "C" int convdr_ip_column_mean(const float* p_f32, int64_t n, int d, float* scratch /* >= 1024 * d floats */,
                                     float* mean, convdr_stream_t stream) {
  CONVDR_REQUIRE(n > 0 && d > 0, "convdr_ip_column_mean: empty block");
  // (64 row chunks x 3 column blocks = 192 workgroups streamed a 3 GB block at 0.5 TB/s: 5.8 ms of every first add();
  //  1024 chunks fill the chip)
  const int chunks = n >= 262144 ? 1024 : (n >= 4096 ? 64 : 1);
  hipLaunchKernelGGL(k_colsum_f32, dim3((d + 255) / 256, chunks), dim3(256), 0, (hipStream_t)stream, p_f32, n, d, scratch);
  hipLaunchKernelGGL(k_colmean_finish, dim3((d + 255) / 256), dim3(256), 0, (hipStream_t)stream, scratch, chunks, d, n, mean);
  CONVDR_CHECK_LAUNCH("k_colsum_f32");
  return 0;
}

static int ip_prepare_block(int kind, const float* p_f32, int64_t n, int d, const float* centre, float scale, void* p_half,
                            void* p_half_lo, float* max_norm, hipStream_t st) {
  CONVDR_REQUIRE(n >= 0 && d > 0 && d % 64 == 0, "convdr_ip_prepare_block: need d %% 64 == 0 (got n=%lld d=%d)",
                 (long long)n, d);
  if (n == 0) return 0;
  const int64_t blocks = ceil_div64(n, 4);
  const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
  if (kind == IP_KIND_F16) {
    int ex = 0;
    CONVDR_REQUIRE(scale > 0.f && frexpf(scale, &ex) == 0.5f, "convdr_ip_prepare_block_f16: scale must be a power of two (got %g)",
                   (double)scale);
    hipLaunchKernelGGL((k_rows_to_half<IP_KIND_F16, false>), dim3(grid), dim3(256), 0, st, p_f32, n, d, centre, scale,
                       (bf16_t*)p_half, (bf16_t*)p_half_lo, (float*)nullptr, max_norm);
  } else {
    hipLaunchKernelGGL((k_rows_to_half<IP_KIND_BF16, false>), dim3(grid), dim3(256), 0, st, p_f32, n, d, centre, 1.f,
                       (bf16_t*)p_half, (bf16_t*)p_half_lo, (float*)nullptr, max_norm);
  }
  CONVDR_CHECK_LAUNCH("k_rows_to_half");
  return 0;
}

extern "C" int convdr_ip_prepare_block(const float* p_f32, int64_t n, int d, const float* centre, void* p_bf16,
                                       void* p_bf16_lo, float* max_norm, convdr_stream_t stream) {
  return ip_prepare_block(IP_KIND_BF16, p_f32, n, d, centre, 1.f, p_bf16, p_bf16_lo, max_norm, (hipStream_t)stream);
}

extern "C" int convdr_ip_prepare_block_f16(const float* p_f32, int64_t n, int d, const float* centre, float scale, void* p_f16,
                                           void* p_f16_lo, float* max_norm, convdr_stream_t stream) {
  return ip_prepare_block(IP_KIND_F16, p_f32, n, d, centre, scale, p_f16, p_f16_lo, max_norm, (hipStream_t)stream);
}

extern "C" float convdr_ip_f16_scale(float max_norm) {
  // power of two that puts max_norm into [2^12, 2^13): elements stay below 2^13 (fp16 max 65504 leaves a factor 7 for
  // blocks added later), typical elements (norm / sqrt(d)) far above the 2^-14 end of the normal range
  if (!(max_norm > 0.f) || max_norm == INFINITY) return 1.f;
  int ex = 0;
  (void)frexpf(max_norm, &ex);
  int sh = (int)IP_F16_TARGET_EXP + 1 - ex;
  sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
  return ldexpf(1.f, sh);
}

// The shallow plan's size for any nq, n, d it can be computed for: k and cap are not checked here (the search entries do).
extern "C" size_t convdr_ip_workspace_bytes(int nq, int64_t n, int d, int k, int cap) {
  if (nq <= 0 || n < 0 || d <= 0) return 0;
  return ip_plan(nq, n, d, cap).total;
}

extern "C" const uint32_t* convdr_ip_debug_counts(const void* workspace, int nq, int64_t n, int d, int k, int cap) {
  return (const uint32_t*)((const char*)workspace + ip_plan(nq, n, d, cap).o_counts_packed);
}

extern "C" const uint32_t* convdr_ip_debug_band(const void* workspace, int nq, int64_t n, int d, int k, int cap) {
  return (const uint32_t*)((const char*)workspace + ip_plan(nq, n, d, cap).o_m);
}

// Test aids: where the last search on this workspace left its raw scan scores (include/convdr_hip.h says when they are whole).
extern "C" int convdr_ip_debug_list(const void* workspace, int nq, int64_t n, int d, int k, int cap, const uint32_t** id,
                                    const float** s) {
  CONVDR_REQUIRE(workspace && id && s && nq > 0 && n >= 0 && d > 0 && cap > 0, "convdr_ip_debug_list: bad arguments");
  const IpPlan p = ip_plan(nq, n, d, cap);
  *id = (const uint32_t*)((const char*)workspace + p.o_id);
  *s = (const float*)((const char*)workspace + p.o_s);
  return 0;
}

extern "C" int convdr_ip_debug_sample(const void* workspace, int nq, int64_t n, int d, int k, int cap, const float** T,
                                      int64_t* ld) {
  CONVDR_REQUIRE(workspace && T && ld && nq > 0 && n >= 0 && d > 0 && cap > 0, "convdr_ip_debug_sample: bad arguments");
  const IpPlan p = ip_plan(nq, n, d, cap);
  *T = p.mode < 0 ? nullptr : (const float*)((const char*)workspace + p.o_T);
  *ld = p.nq_pad;
  return 0;
}

// ---- the half store ------------------------------------------------------------------------------------------------
extern "C" int convdr_ip_store_rows_f16(const void* src, int src_is_f32, int64_t n, int d, float scale, void* store,
                                        float* max_norm, int32_t* flags, convdr_stream_t stream) {
  CONVDR_REQUIRE(n >= 0 && d > 0 && d % 64 == 0, "convdr_ip_store_rows_f16: need d %% 64 == 0 (got n=%lld d=%d)", (long long)n, d);
  CONVDR_REQUIRE(ip_pow2_scale_ok(scale), "convdr_ip_store_rows_f16: scale must be a power of two (got %g)", (double)scale);
  CONVDR_REQUIRE(scale >= 1.f || (!src_is_f32 && src == store && src != nullptr),
                 "convdr_ip_store_rows_f16: scale must be >= 1 (got %g); only the in-place rescale of a half store takes a "
                 "factor below 1", (double)scale);
  CONVDR_REQUIRE(flags != nullptr || n == 0, "convdr_ip_store_rows_f16: flags is NULL");
  if (n == 0) return 0;
  const int64_t blocks = ceil_div64(n, 4);
  const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
  if (src_is_f32)
    hipLaunchKernelGGL(k_store_rows_f16<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, n, d, scale, 1.f / scale,
                       (_Float16*)store, max_norm, flags);
  else
    hipLaunchKernelGGL(k_store_rows_f16<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, n, d, scale, 1.f / scale,
                       (_Float16*)store, max_norm, flags);
  CONVDR_CHECK_LAUNCH("k_store_rows_f16");
  return 0;
}

// ---- exact top-k: seven entries, one validated call ------------------------------------------------------------------
// Every top-k entry ends here, the direct ones with a block that has no bitmap: the checks, then the depth's plan and pipeline
// (which checks the workspace against its plan first).  `name`: the entry that was called.
static int ip_topk(const char* name, bool deep, IpBlock b, const IpTopkArgs& c) {
  if (int e = ip_check_sizes(deep ? IP_DEEP : IP_SHALLOW, c.nq, b.n, b.d, c.k, c.cap)) return e;
  CONVDR_REQUIRE(!deep || c.rank_target >= 0, "%s: rank_target=%d", name, c.rank_target);
  if (int e = ip_check_block(name, b)) return e;
  // no allowed row: the empty block's path (no scan; the finishing kernels pad every row of D / I)
  if (b.row_bits && b.n_allowed == 0) b.n = 0;
  if (deep) return ip_search_deep(name, b, c, ip_deep_plan(c.nq, b.n, b.d, c.k, c.cap, c.rank_target));
  return ip_search(name, b, c, ip_plan(c.nq, b.n, b.d, c.cap));
}

// the per-call arguments, which the seven entries name alike (as include/convdr_hip.h does)
#define IP_TOPK_ARGS {q_f32, nq, k, tau_in, cap, rank_target, workspace, workspace_bytes, D, I, status, tau_retry, (hipStream_t)stream}

extern "C" int convdr_ip_search(const float* q_f32, int nq, const float* p_f32, const void* p_bf16, const void* p_bf16_lo,
                                int64_t n, int d, int k, const float* p_max_norm, const float* tau_in, int cap,
                                int rank_target, void* workspace, size_t workspace_bytes, float* D, int64_t* I,
                                int32_t* status, float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search", false, {0, p_f32, p_bf16, p_bf16_lo, 1.f, false, n, d, p_max_norm}, IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_f16(const float* q_f32, int nq, const float* p_f32, const void* p_f16, const void* p_f16_lo,
                                    float p_scale, int64_t n, int d, int k, const float* p_max_norm, const float* tau_in,
                                    int cap, int rank_target, void* workspace, size_t workspace_bytes, float* D,
                                    int64_t* I, int32_t* status, float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_f16", false, {1, p_f32, p_f16, p_f16_lo, p_scale, false, n, d, p_max_norm}, IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_h16(const float* q_f32, int nq, const void* store_f16, float p_scale, int two_pass, int64_t n, int d,
                                    int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target, void* workspace,
                                    size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry,
                                    convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_h16", false,
                 {2, nullptr, store_f16, nullptr, p_scale, two_pass != 0, n, d, p_max_norm}, IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_deep(const float* q_f32, int nq, const float* p_f32, const void* p_bf16, const void* p_bf16_lo,
                                     int64_t n, int d, int k, const float* p_max_norm, const float* tau_in, int cap,
                                     int rank_target, void* workspace, size_t workspace_bytes, float* D, int64_t* I,
                                     int32_t* status, float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_deep", true, {0, p_f32, p_bf16, p_bf16_lo, 1.f, false, n, d, p_max_norm}, IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_deep_f16(const float* q_f32, int nq, const float* p_f32, const void* p_f16, const void* p_f16_lo,
                                         float p_scale, int64_t n, int d, int k, const float* p_max_norm, const float* tau_in,
                                         int cap, int rank_target, void* workspace, size_t workspace_bytes, float* D,
                                         int64_t* I, int32_t* status, float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_deep_f16", true, {1, p_f32, p_f16, p_f16_lo, p_scale, false, n, d, p_max_norm}, IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_deep_h16(const float* q_f32, int nq, const void* store_f16, float p_scale, int two_pass, int64_t n,
                                         int d, int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target,
                                         void* workspace, size_t workspace_bytes, float* D, int64_t* I, int32_t* status,
                                         float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_deep_h16", true,
                 {2, nullptr, store_f16, nullptr, p_scale, two_pass != 0, n, d, p_max_norm}, IP_TOPK_ARGS);
}

// Row-filtered search: the six entries above restricted to the rows whose bit is set; its own arguments are checked here.
extern "C" int convdr_ip_search_filtered(int store, int deep, const float* q_f32, int nq, const float* p_f32, const void* p_half,
                                         const void* p_half_lo, float p_scale, int two_pass, int64_t n, int d, int k,
                                         const float* p_max_norm, const float* tau_in, int cap, int rank_target, void* workspace,
                                         size_t workspace_bytes, const uint32_t* row_bits, int64_t row_bits_words,
                                         int64_t n_allowed, float* D, int64_t* I, int32_t* status, float* tau_retry,
                                         convdr_stream_t stream) {
  const char* name = "convdr_ip_search_filtered";
  CONVDR_REQUIRE(store >= 0 && store <= 2 && (deep == 0 || deep == 1),
                 "%s: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) and deep 0 or 1 (got store=%d deep=%d)", name, store,
                 deep);
  CONVDR_REQUIRE(row_bits != nullptr, "%s: row_bits is NULL", name);
  CONVDR_REQUIRE(n_allowed >= 0 && n_allowed <= n, "%s: n_allowed=%lld outside [0, n=%lld]", name, (long long)n_allowed, (long long)n);
  CONVDR_REQUIRE(two_pass == 0 || (two_pass == 1 && store == 2), "%s: two_pass=%d (0, or 1 with the half store)", name, two_pass);
  CONVDR_REQUIRE(store != 2 || p_half_lo == nullptr, "%s: the half store has no remainder copy", name);
  return ip_topk(name, deep != 0, {store, p_f32, p_half, p_half_lo, store == 0 ? 1.f : p_scale, two_pass != 0, n, d, p_max_norm,
                                   row_bits, row_bits_words, n_allowed}, IP_TOPK_ARGS);
}

// ---- the 8-bit store -------------------------------------------------------------------------------------------------
static int q8_check_width(const char* name, int64_t n, int d) {
  CONVDR_REQUIRE(n >= 0 && d > 0 && d % 128 == 0 && d <= IP_Q8_MAX_D, "%s: need n >= 0, d %% 128 == 0 and d <= %d (got n=%lld d=%d)", name,
                 IP_Q8_MAX_D, (long long)n, d);
  return 0;
}

extern "C" int convdr_ip_column_absdev(const float* p_f32, int64_t n, int d, const float* centre, float* scratch /* >= 1024 * d floats */,
                                       float* step, convdr_stream_t stream) {
  CONVDR_REQUIRE(n > 0 && d > 0, "convdr_ip_column_absdev: empty block");
  CONVDR_REQUIRE(p_f32 && centre && scratch && step, "convdr_ip_column_absdev: a NULL argument (p_f32, centre, scratch, step)");
  const int chunks = n >= 262144 ? 1024 : (n >= 4096 ? 64 : 1);   // (as convdr_ip_column_mean)
  hipLaunchKernelGGL(k_colabsdev_f32, dim3((d + 255) / 256, chunks), dim3(256), 0, (hipStream_t)stream, p_f32, n, d, centre, scratch);
  CONVDR_CHECK_LAUNCH("k_colabsdev_f32");
  hipLaunchKernelGGL(k_colstep_finish, dim3((d + 255) / 256), dim3(256), 0, (hipStream_t)stream, scratch, chunks, d, step);
  CONVDR_CHECK_LAUNCH("k_colstep_finish");
  return 0;
}

extern "C" int convdr_ip_store_rows_q8(const float* src, int64_t n, int d, const float* centre, const float* step, void* codes,
                                       float* max_l1, int32_t* flags, uint32_t* saturated, convdr_stream_t stream) {
  const char* name = "convdr_ip_store_rows_q8";
  if (int e = q8_check_width(name, n, d)) return e;
  if (n == 0) return 0;
  CONVDR_REQUIRE(src && centre && step && codes && max_l1 && flags && saturated,
                 "%s: a NULL argument (src, centre, step, codes, max_l1, flags, saturated)", name);
  const int64_t blocks = ceil_div64(n, 4);
  hipLaunchKernelGGL(k_store_rows_q8, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, src, n, d, centre,
                     step, (int8_t*)codes, max_l1, flags, saturated);
  CONVDR_CHECK_LAUNCH("k_store_rows_q8");
  return 0;
}

static IpBlock q8_block(const void* codes, const float* centre, const float* step, int64_t n, int d, const float* p_max_l1,
                        const uint32_t* row_bits = nullptr, int64_t row_bits_words = 0, int64_t n_allowed = 0) {
  IpBlock b = {3, nullptr, codes, nullptr, 1.f, false, n, d, p_max_l1, row_bits, row_bits_words, n_allowed};
  b.q8_centre = centre;
  b.q8_step = step;
  return b;
}

extern "C" int convdr_ip_search_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step, int64_t n,
                                   int d, int k, const float* p_max_l1, const float* tau_in, int cap, int rank_target,
                                   void* workspace, size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry,
                                   convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_q8", false, q8_block(codes, centre, step, n, d, p_max_l1), IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_deep_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step,
                                        int64_t n, int d, int k, const float* p_max_l1, const float* tau_in, int cap,
                                        int rank_target, void* workspace, size_t workspace_bytes, float* D, int64_t* I,
                                        int32_t* status, float* tau_retry, convdr_stream_t stream) {
  return ip_topk("convdr_ip_search_deep_q8", true, q8_block(codes, centre, step, n, d, p_max_l1), IP_TOPK_ARGS);
}

extern "C" int convdr_ip_search_filtered_q8(int deep, const float* q_f32, int nq, const void* codes, const float* centre,
                                            const float* step, int64_t n, int d, int k, const float* p_max_l1, const float* tau_in,
                                            int cap, int rank_target, void* workspace, size_t workspace_bytes,
                                            const uint32_t* row_bits, int64_t row_bits_words, int64_t n_allowed, float* D,
                                            int64_t* I, int32_t* status, float* tau_retry, convdr_stream_t stream) {
  const char* name = "convdr_ip_search_filtered_q8";
  CONVDR_REQUIRE(deep == 0 || deep == 1, "%s: deep must be 0 or 1 (got %d)", name, deep);
  CONVDR_REQUIRE(row_bits != nullptr, "%s: row_bits is NULL", name);
  CONVDR_REQUIRE(n_allowed >= 0 && n_allowed <= n, "%s: n_allowed=%lld outside [0, n=%lld]", name, (long long)n_allowed, (long long)n);
  return ip_topk(name, deep != 0, q8_block(codes, centre, step, n, d, p_max_l1, row_bits, row_bits_words, n_allowed), IP_TOPK_ARGS);
}

extern "C" int convdr_ip_score_rows_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step,
                                       int64_t n, int d, const int64_t* rows, int m, int64_t ld, double* X, float* D,
                                       convdr_stream_t stream) {
  const char* name = "convdr_ip_score_rows_q8";
  CONVDR_REQUIRE(nq >= 0 && m >= 0 && ld >= m, "%s: bad sizes nq=%d m=%d ld=%lld (ld >= m)", name, nq, m, (long long)ld);
  CONVDR_REQUIRE(n < ((int64_t)1 << 31), "%s: bad block size n=%lld (0 <= n < 2^31)", name, (long long)n);
  if (int e = q8_check_width(name, n, d)) return e;
  if (nq == 0 || m == 0) return 0;
  CONVDR_REQUIRE(q_f32 && rows, "%s: a NULL argument (q_f32, rows)", name);
  CONVDR_REQUIRE(n == 0 || (codes && centre && step), "%s: a NULL block pointer (codes, centre, step)", name);
  if (!X && !D) return 0;
  return ip_score_rows_launch(q8_block(codes, centre, step, n, d, nullptr), q_f32, nq, rows, m, ld, X, D, (hipStream_t)stream);
}
