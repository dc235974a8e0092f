/*
 * libconvdr_hip.so -- C ABI of the MI355X (gfx950) kernels behind ConvDR's hot path.
 *
 * The reference (thunlp/ConvDR) is pure Python; it has no FFI of its own.  Every entry point
 * below replaces a *third-party arithmetic call site* of the reference and is
 * what a ctypes binding on the reference side would bind (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (tensor.data_ptr()) unless the name says host;
 *   - plain C types only, row-major contiguous arrays, explicit sizes;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - no allocation and no synchronisation inside: the caller owns outputs and workspace;
 *   - return 0 on success, negative on error; convdr_last_error() gives the message
 *     (thread-local).  Kernels are enqueued asynchronously.
 */
#ifndef CONVDR_HIP_H
#define CONVDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* convdr_stream_t;

int convdr_version(void);
/* "domain:bus:device.function" of HIP device `device` (hipDeviceGetPCIBusId through the runtime this library is bound
 * to): the host side looks up the GPU's NUMA node with it and places its pinned staging buffers there. */
int convdr_device_pci_bus_id(int device, char* out, int len);
const char* convdr_last_error(void);

/* Optional per-kernel timing with hipEvents recorded on the launch stream (bench.py's roofline
 * leg).  enable(1) clears the recorded spans; collect() synchronises on the spans named `name`
 * ("ip_scan_emit", "ip_scan_sample", "ip_rescore", ...) and returns their summed duration. */
int convdr_prof_enable(int on);
int convdr_prof_collect(const char* name, float* total_ms, int* launches);

/* ------------------------------------------------------------------------------------------
 * Flat inner-product index: replaces faiss.IndexFlatIP(768) as driven by
 *   /root/reference/drivers/run_convdr_inference.py:353 (ctor), :180 (.add), :182 (.search), :202 (.reset)
 * ------------------------------------------------------------------------------------------ */

/* Column mean of an fp32 block [n, d] (the centring vector of the scan copies).  scratch: >= 1024 * d floats. */
int convdr_ip_column_mean(const float* p_f32, int64_t n, int d, float* scratch, float* mean, convdr_stream_t stream);

/* .add(block): build the bf16 scan copy of an fp32 block [n, d]:  p_bf16 = bf16(p - centre)  (centre: device fp32 [d]
 * or NULL).  Subtracting a fixed vector from every passage shifts all scores of a query by the same constant, so the
 * ranking is unchanged while the rounding-error bound of the scan shrinks from |q| max|p| to |q| max|p - centre|
 * (embeddings of one encoder share a large common component).  p_bf16_lo (nullable): bf16 of the rounding remainder
 * (p - centre) - hi, needed by the split-bf16 scan.  max_i ||p_i - centre||_2 is folded into *max_norm (device float,
 * caller zero-initialises it on reset).  d % 64 == 0. */
int convdr_ip_prepare_block(const float* p_f32, int64_t n, int d, const float* centre, void* p_bf16, void* p_bf16_lo,
                            float* max_norm, convdr_stream_t stream);

/* The same for the fp16 scan (the default first rung: v_mfma_f32_32x32x16_f16 runs at the bf16 rate with 11 significand
 * bits instead of 8, i.e. an 8x tighter error band per pass):  p_f16 = half(scale * (p - centre)),  p_f16_lo (nullable)
 * = half of the remainder.  `scale` is a power of two (exact) that moves the block's norms to ~2^12, away from both
 * ends of the half range; convdr_ip_f16_scale(max norm seen so far) proposes it.  *max_norm stays UNSCALED.
 * p_f16 == NULL: only fold the norms into *max_norm (the pass that finds the scale of a first block). */
int convdr_ip_prepare_block_f16(const float* p_f32, int64_t n, int d, const float* centre, float scale, void* p_f16,
                                void* p_f16_lo, float* max_norm, convdr_stream_t stream);
float convdr_ip_f16_scale(float max_norm);

/* Bytes of device workspace convdr_ip_search needs for these sizes. */
size_t convdr_ip_workspace_bytes(int nq, int64_t n, int d, int k, int cap);

/* per-query status written by convdr_ip_search */
#define CONVDR_IP_OK 0        /* result is the exact top-k (certified)                                  */
#define CONVDR_IP_OVERFLOW 1  /* more than `cap` candidates passed tau: retry with tau_retry (raise cap
                                 when tau_retry does not exceed the tau that was used)                    */
#define CONVDR_IP_TOO_FEW 2   /* fewer than min(k, n) candidates passed tau: retry with tau_retry         */
#define CONVDR_IP_UNCERTAIN 3 /* the re-score band reaches below tau: retry with tau_retry               */
#define CONVDR_IP_RANGE 4     /* fp16 scan only: scale * max norm > 60000, elements of the half copy may be
                                 inf -- rebuild the copy with convdr_ip_f16_scale(current max norm), search again */

/* .search(Q, k): exact inner-product top-k of nq fp32 queries against one resident block.
 *   scan     bf16 MFMA GEMM  S~ = P_bf16 * Q_bf16^T  with a fused per-query threshold test: passages with
 *            S~ >= tau[q] are appended to a candidate list (a [nq, n] score matrix is never written);
 *            tau comes from a bf16 scan of a 1/32 sample of the block, aimed at `rank_target` hits per
 *            query (or tau_in when given);
 *   cut      with eps = (2u + u^2 + d 2^-23) * ||q|| * max||p||, u = 2^-8 (rigorous bound on |S~ - exact|; 0.00792 at d = 768): the band
 *            {S~ >= S~(k) - 2 eps} provably contains the exact top-k;
 *   rescore  the band is re-scored from the fp32 originals in fp64 with the canonical summation order
 *            documented in oracle/search.py, and sorted by (score desc, index asc).
 * status is OK only if the candidate list is complete over the band (cut >= tau, no overflow), so an
 * OK result equals the exhaustive exact top-k; otherwise tau_retry[q] is the threshold to pass as
 * tau_in for that query.
 * Outputs (device): D [nq, k] fp32 scores (descending), I [nq, k] int64 row indices into the block
 * (-1 / -FLT_MAX padding when n < k, as FAISS does), status [nq] int32, tau_retry [nq] fp32.
 * tau_in: NULL, or device [nq] thresholds (retry path).  cap: candidate capacity per query
 * (power of two, 1024..8192).  rank_target: expected candidates per query (0 -> 16*k, at most cap/2).
 * p_bf16_lo: NULL = plain bf16 scan (eps = 0.00792 |q| max|p'| at d = 768); non-NULL = split-bf16 scan S~ = Ph Qh + Ph Ql + Pl Qh
 * (three MFMA passes, eps = (3 u^2 + 3 d 2^-23) |q| max|p'| = 3.2e-4 at d = 768): the second rung for clustered embeddings whose top scores are closer
 * together than the bf16 error band. */
int convdr_ip_search(const float* q_f32, int nq, const float* p_f32, const void* p_bf16, const void* p_bf16_lo, int64_t n, int d,
                     int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target,
                     void* workspace, size_t workspace_bytes, float* D, int64_t* I, int32_t* status,
                     float* tau_retry, convdr_stream_t stream);

/* convdr_ip_search over the fp16 scan copy built by convdr_ip_prepare_block_f16 with the same p_scale.  Queries are
 * scaled per row by a power of two inside (norm -> [2^11, 2^12)); thresholds (tau_in / tau_retry) are in those scaled
 * units and are only meaningful for a retry of the same query against the same copy.
 *   eps = (2u + u^2 + d 2^-23) |q| max|p'| + eta (1 + u) sqrt(d) (|q| + max|p'|) + d eta^2,  u = 2^-11, eta = 2^-14
 *   (1.07e-3 |q| max|p'| at d = 768; the absolute term ~1e-6 of it);  p_f16_lo non-NULL: the split scan
 *   S~ = Ph Qh + Ph Ql + Pl Qh with 3 u^2 + 3 d 2^-23 = 2.8e-4.
 * status may also be CONVDR_IP_RANGE (see above).  D / I are defined exactly as for convdr_ip_search -- the rung only
 * decides which candidates are re-scored, never the result. */
int convdr_ip_search_f16(const float* q_f32, int nq, const float* p_f32, const void* p_f16, const void* p_f16_lo, float p_scale,
                         int64_t n, int d, int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target,
                         void* workspace, size_t workspace_bytes, float* D, int64_t* I, int32_t* status,
                         float* tau_retry, convdr_stream_t stream);

/* Deep candidate lists: convdr_ip_search[_f16] for 4,096 < k <= 65,536 (any k >= 1 is accepted).  Same arguments, same
 * outputs, same status words and tau_retry, same certificate; the differences:
 *   cap          a power of two in [16384, 131072], 1 <= k <= cap / 2 (so k <= 65,536); n < 2^31, d % 64 == 0, d <= 4096.
 *   n <= cap     every row is a candidate (no threshold pass), as in the shallow call.
 *   threshold    n > cap: from the COMPLETE scan scores of a row sample (16 evenly spaced runs of whole 256-row tiles,
 *                >= 32,768 and <= 262,144 rows, sized so that the target rank is ~512 inside the sample); aimed at rank
 *                rank_target of the block (0 -> cap / 2, or k + (cap - k) / 2 where cap / 2 < 1.5 k).
 *   finish       three launches through global memory, one workgroup per query: cut (list -> band), the canonical fp64
 *                re-score (the shallow call's kernel), select (radix select + tiled bitonic ordering of the survivors).
 * Workspace (convdr_ip_deep_workspace_bytes; every part 256-byte aligned, nq_pad = nq rounded up to the scan's query tile,
 * 128 or 256): the 16-bit queries and their remainders 2 x [nq_pad, d] x 2, norms / thresholds / band sizes / packed counts
 * 4 x [nq_pad] x 4, hit counters [nq_pad] x 128, the sample's scores [rows, nq_pad] x 4 (rows: the tallest sample k allows, reserved for every n), then per query and list
 * slot 28 bytes: list id 4 + list scan score 4 + band id 4 + band fp64 score 8 + ordered fp64 score 8 (the ordered ids
 * reuse the list ids) = nq * cap * 28.  Arguments are validated before anything touches a device. */
size_t convdr_ip_deep_workspace_bytes(int nq, int64_t n, int d, int k, int cap);   /* 0 outside the contract: convdr_last_error says why */
int convdr_ip_search_deep(const float* q_f32, int nq, const float* p_f32, const void* p_bf16, const void* p_bf16_lo, int64_t n,
                          int d, int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target,
                          void* workspace, size_t workspace_bytes, float* D, int64_t* I, int32_t* status,
                          float* tau_retry, convdr_stream_t stream);
int convdr_ip_search_deep_f16(const float* q_f32, int nq, const float* p_f32, const void* p_f16, const void* p_f16_lo,
                              float p_scale, int64_t n, int d, int k, const float* p_max_norm, const float* tau_in, int cap,
                              int rank_target, void* workspace, size_t workspace_bytes, float* D, int64_t* I,
                              int32_t* status, float* tau_retry, convdr_stream_t stream);

/* Half-precision passage store: the passage is stored ONCE, in 16 bits, and that copy is both the corpus and the scan
 * operand (1,536 bytes per passage at d = 768 instead of 3,072 fp32 + 1,536 scan copy, + 1,536 for the split rung).
 *   corpus    THE STORED HALVES.  Built from float16 rows (kept bit for bit) or from fp32 rows rounded to nearest even once
 *             (numpy.astype(float16), torch.half()); from then on the corpus is those halves widened exactly to fp32.
 *   result    what the fp32 entries return for that widened corpus, bit for bit: canonical fp64 summation order, ranking by
 *             (score desc, index asc), D = the fp64 score rounded to fp32, padding -FLT_MAX / -1.
 *   scaling   the resident copy is 2^s v for the stored half v, s >= 0 (p_scale = 2^s >= 1; convdr_ip_f16_scale of the
 *             first rows' largest norm, clamped to >= 1).  Scaling a half up by a power of two is exact, subnormals included,
 *             unless it overflows, so the copy is literally an un-centred fp16 scan copy and scan, thresholds (scaled
 *             units) and certificate are those of convdr_ip_search_f16 with this p_scale.  The re-score sums
 *             q . (2^s v) in fp64 and multiplies once by 2^-s: every fp64 step scales exactly, the value is the oracle's.
 *   no centre the store is what it is: eps carries max|p|, not max|p - centre|.
 *
 * convdr_ip_store_rows_f16: src = n rows of halves (src_is_f32 = 0) or of fp32 (rounded here); store[i] = half * scale;
 * the rows' UNSCALED norms are folded into *max_norm (nullable).  *flags (device int32, the caller zeroes it) is OR-ed with
 *   1  a value is not finite (after rounding to half)
 *   2  a scaled value overflowed, or store / scale != half
 * store == NULL: norms and flag 1 only.  store == src (halves): the in-place rescale after CONVDR_IP_RANGE by the factor
 * scale = 2^(s_new - s_old) <= 1 with s_new >= 0 -- the only form that takes a scale below 1.  d % 64 == 0, scale a power
 * of two; arguments are validated before anything touches a device. */
int convdr_ip_store_rows_f16(const void* src, int src_is_f32, int64_t n, int d, float scale, void* store, float* max_norm,
                             int32_t* flags, convdr_stream_t stream);
/* convdr_ip_search_f16 over a half store (workspace: convdr_ip_workspace_bytes).  two_pass = 0: the single-pass fp16 scan
 * with today's fp16 eps (it bounds a superset of the errors: the passage operand carries none).  two_pass = 1: the second
 * rung S~ = P Qh + P Ql -- two MFMA passes, no remainder copy -- with the split scan's eps (3 u^2 (1 + 2u) + 3 d 2^-23,
 * u = 2^-11; every term of the two-pass error is majorised by the corresponding term of the three-pass bound).
 * p_scale: a power of two >= 1, the scale the store was built with.  Status words, tau_retry and convdr_ip_debug_* as for
 * convdr_ip_search_f16; both settings of the option ip_fused_finish work. */
int convdr_ip_search_h16(const float* q_f32, int nq, const void* store_f16, float p_scale, int two_pass, int64_t n, int d,
                         int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target, void* workspace,
                         size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry, convdr_stream_t stream);
/* The same with deep candidate lists: the contract of convdr_ip_search_deep_f16 (workspace: convdr_ip_deep_workspace_bytes,
 * cap a power of two in [16384, 131072], k <= cap / 2, n < 2^31). */
int convdr_ip_search_deep_h16(const float* q_f32, int nq, const void* store_f16, float p_scale, int two_pass, int64_t n, int d,
                              int k, const float* p_max_norm, const float* tau_in, int cap, int rank_target, void* workspace,
                              size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry,
                              convdr_stream_t stream);

/* Row-filtered search: any of the six entries above restricted to an allowed subset of the block's rows (what FAISS calls an
 * IDSelector: deleted rows, a sub-collection, a top-k that must not contain known positives).
 *   bitmap       row_bits: device uint32 words, 16-BYTE ALIGNED (the scan reads a wave's four words as one 16-byte load; any
 *                hipMalloc pointer is); row r is allowed iff bit (r & 31) of word (r >> 5) is set.  The bitmap covers
 *                whole 256-row scan tiles, zero padded: row_bits_words >= ceil(n / 256) * 8, and the bits of the rows past n are
 *                zero (the scan does not trust them: a set bit past n is ignored).
 *   n_allowed    the number of set bits among rows 0..n-1, a HOST value the library cannot check (it would cost a device round
 *                trip per search): it takes n's place in need = min(k, n_allowed) -- padding with -FLT_MAX / -1 begins there,
 *                TOO_FEW means fewer than that many candidates -- and n_allowed <= cap selects the one-pass plan: every allowed
 *                row is a candidate, no threshold sample, tau = -inf.  A wrong n_allowed gives wrong padding or a status that
 *                never clears, never an out-of-bounds access: the list is bounded by cap and only rows < n are ever named.
 *                n_allowed == 0: no scan, D / I are all padding.
 *   scan         a row whose bit is clear never becomes a candidate, whatever the threshold is, and counts as -inf in the
 *                threshold samples (which therefore estimate ranks among the allowed rows).
 *   certificate  unchanged, over the allowed rows: the list holds every ALLOWED row with S~ >= tau, cut = S~(k) - 2 eps is taken
 *                over allowed rows, and OK means the list is complete down to the cut -- the result is the exhaustive exact
 *                top-k of the allowed rows, canonical fp64 scores, (score desc, index asc); I holds row indices of the block.
 *   store, deep  store = 0: the bf16 scan copy (convdr_ip_search[_deep]; p_scale and two_pass are not read / must be 0);
 *                store = 1: the fp16 scan copy (.._f16; p_scale a power of two); store = 2: the half store (.._h16; p_half is
 *                the store, p_f32 is not read, p_half_lo must be NULL, p_scale a power of two >= 1, two_pass 0 or 1).
 *                deep = 0 / 1: the shallow or the deep entry, with that entry's contract for cap and k and its workspace size
 *                (convdr_ip_workspace_bytes / convdr_ip_deep_workspace_bytes, planned by n, not by n_allowed).
 * Every other argument, output and status word is the matching entry's; both settings of the option ip_fused_finish work.
 * Arguments are validated before anything touches a device. */
int convdr_ip_search_filtered(int store, int deep, const float* q_f32, int nq, const float* p_f32, const void* p_half,
                              const void* p_half_lo, float p_scale, int two_pass, int64_t n, int d, int k, const float* p_max_norm,
                              const float* tau_in, int cap, int rank_target, void* workspace, size_t workspace_bytes,
                              const uint32_t* row_bits, int64_t row_bits_words, int64_t n_allowed, float* D, int64_t* I,
                              int32_t* status, float* tau_retry, convdr_stream_t stream);

/* 8-bit store: the passage is stored ONCE, as d int8 codes, and that buffer is both the corpus and the scan operand (768
 * bytes per passage at d = 768).  A scalar quantiser with one centre and one step per column (FAISS IndexScalarQuantizer,
 * QT_8bit), and an EXACT search over what it stores.
 *   corpus    THE RECONSTRUCTED ROWS  v[i, j] = fl32(centre[j] + fl32(step[j] * c[i, j])): one fp32 multiplication rounded, one
 *             fp32 addition rounded, never contracted (numpy's float32 arithmetic gives the same bits).
 *   codes     c = clamp(rint((p - centre) / step), -127, 127) in fp32 (subtraction, IEEE division, round half to even); a
 *             column with step 0 has code 0; -128 is never stored.  centre: convdr_ip_column_mean of the first rows; step:
 *             convdr_ip_column_absdev of the same rows.  Both are fixed then; later rows outside the range saturate.
 *   result    what the fp32 entries return for the corpus v, bit for bit: canonical fp64 summation order, ranking by
 *             (score desc, index asc), D = the fp64 score rounded to fp32, padding -FLT_MAX / -1.
 *   scan      integer and exact: per query q'[j] = fl32(q[j] * step[j]), t the power of two with max |q'| / t in (8128, 16256],
 *             Qi = rint(q' / t) = 128 hi + lo with hi in [-127, 127], lo in [-64, 63]; S = 128 sum hi c + sum lo c on
 *             v_mfma_i32_32x32x32_i8 (no int32 overflows for d <= 1024), S~ = (float)S.  Thresholds, tau_retry and the lists of
 *             convdr_ip_debug_* are in these units.
 *   band      |S~ - E| <= (1/2 + r) max_i ||c_i||_1 + A(q) for E = (1 / t) sum_j q[j] (v[i, j] - centre[j]), r = 0.001938, A(q) =
 *             (2^-24 / t) sum_j |q[j]| (|centre[j]| + 254 step[j]): the query's rounding, the two fp32 roundings of v, the
 *             int-to-float conversion (derivation: csrc/ip_topk.hip, IP_Q8_COEF).  max_l1: device float, the largest row sum of
 *             |c| (an upper bound is enough).
 *   status    as for convdr_ip_search; CONVDR_IP_RANGE: the query holds a value that is not finite, or its largest |q'| is non-zero
 *             and below 2^-100 -- no threshold helps.
 *   sizes     d % 128 == 0 (one K step is 128 codes) and d <= 1024 (the int32 range above); otherwise those of the matching
 *             fp32 entry, whose workspace size (convdr_ip_workspace_bytes / convdr_ip_deep_workspace_bytes) and layout serve as
 *             they are: the two int8 query operands take the place of the 16-bit one.
 * Arguments are validated before anything touches a device.
 *
 * convdr_ip_column_absdev: step[j] = max_i |p[i, j] - centre[j]| / 127 as fp32 (a quotient below FLT_MIN counts as 0: a constant
 * column).  scratch: >= 1024 * d floats, as for convdr_ip_column_mean. */
int convdr_ip_column_absdev(const float* p_f32, int64_t n, int d, const float* centre, float* scratch, float* step,
                            convdr_stream_t stream);
/* codes[i] = the codes of the fp32 row src[i] (n rows of d int8).  *max_l1 (device float, atomic max: the caller zeroes it once
 * per index) takes the largest row sum of |c|; *flags (device int32, the caller zeroes it) |= 1 for a value that is not finite;
 * *saturated (device uint32, the caller zeroes it) counts the values the clamp moved. */
int convdr_ip_store_rows_q8(const float* src, int64_t n, int d, const float* centre, const float* step, void* codes, float* max_l1,
                            int32_t* flags, uint32_t* saturated, convdr_stream_t stream);
/* convdr_ip_search / convdr_ip_search_deep over an 8-bit store. */
int convdr_ip_search_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step, int64_t n, int d,
                        int k, const float* p_max_l1, const float* tau_in, int cap, int rank_target, void* workspace,
                        size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry, convdr_stream_t stream);
int convdr_ip_search_deep_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step, int64_t n,
                             int d, int k, const float* p_max_l1, const float* tau_in, int cap, int rank_target, void* workspace,
                             size_t workspace_bytes, float* D, int64_t* I, int32_t* status, float* tau_retry,
                             convdr_stream_t stream);
/* The two above restricted to the rows of a bitmap: row_bits, row_bits_words, n_allowed and deep as for
 * convdr_ip_search_filtered. */
int convdr_ip_search_filtered_q8(int deep, const float* q_f32, int nq, const void* codes, const float* centre, const float* step,
                                 int64_t n, int d, int k, const float* p_max_l1, const float* tau_in, int cap, int rank_target,
                                 void* workspace, size_t workspace_bytes, const uint32_t* row_bits, int64_t row_bits_words,
                                 int64_t n_allowed, float* D, int64_t* I, int32_t* status, float* tau_retry,
                                 convdr_stream_t stream);
/* convdr_ip_score_rows over an 8-bit store: the canonical score of (query, reconstructed row), one device function with the
 * search's re-score. */
int convdr_ip_score_rows_q8(const float* q_f32, int nq, const void* codes, const float* centre, const float* step, int64_t n, int d,
                            const int64_t* rows, int m, int64_t ld, double* X, float* D, convdr_stream_t stream);

/* Range search: every row of the block whose score EXCEEDS a per-query radius (IndexFlatIP.range_search, with one radius
 * per query), exact and ragged.
 *   result       with X the canonical fp64 score of the search entries (same summation order, same corpus per store: the
 *                fp32 block, or the stored halves widened -- the centre and the scale are the scan's private business and do
 *                not show), row i belongs to query q iff X[q, i] > (double)radius[q]: STRICT, as FAISS's inner-product
 *                range search.  Per query the rows are ordered by (X desc, index asc).  D is X rounded to fp32 -- so a
 *                reported D may EQUAL the radius, for a score above it by less than half an ulp --, I the int64 row number,
 *                lims int64 [nq + 1] with lims[0] = 0: query q owns D / I [lims[q], lims[q + 1]).  With a bitmap (the
 *                contract of convdr_ip_search_filtered: 16-byte aligned, whole 256-row tiles, bits past n ignored; NULL, 0:
 *                no filter) the result is the same set intersected with the allowed rows.
 *   radius       device fp32 [nq].  -inf: every row; +inf: no row.  NaN is the caller's to refuse (never true: no row).
 *   threshold    one single-pass scan (the index's kind: store 0 bf16, 1 / 2 fp16; the half store one pass) lists the rows with
 *                S~ >= tau[q] = round_down(qs[q] * p_scale * (radius[q] - q . centre)) - eps[q], where qs is the query's
 *                power-of-two scale (1 for bf16), q . centre is summed in fp64 (centre may be NULL; must be for store 2), eps
 *                is the error band of the top-k certificate, and every rounding -- the fp64 sums' own error bounds, the
 *                conversion to fp32, the subtraction -- pushes tau DOWN.  Claim: every row with X > radius has S~ >= tau
 *                (proof beside k_ip_range_tau), so a list that did not overflow holds every result row; all its entries are
 *                re-scored canonically and the predicate is decided on X.  There is no sample, no k-th score, no TOO_FEW or
 *                UNCERTAIN.  The split scans would only narrow the band of wasted re-scores and are not used.
 *   status       CONVDR_IP_OK: the query's run is exact and complete, counts[q] = its length.  CONVDR_IP_OVERFLOW: the scan
 *                hit more than cap rows; counts[q] = the scan's total hit count (>= the result's length): re-run with
 *                cap >= counts[q], which cannot overflow again.  CONVDR_IP_RANGE (fp16 kinds): the scale no longer fits the
 *                block's norms (or the query is astronomically long): rebuild the scan copy.  A query that is not OK has an
 *                empty run in lims.
 *   cap          a power of two in [1024, 131072]: entries of a query's list, which lives in global memory at every cap.
 *   count_only   1: re-score, predicate and count only -- counts and status are written, lims too unless it is NULL (it
 *                may be), nothing is ordered and convdr_ip_range_pack must not follow.
 *   workspace    convdr_ip_range_workspace_bytes(nq, n, d, cap) bytes (0 outside the contract: convdr_last_error says why), 256-byte aligned
 *                regions in this order: query operands [nq_pad, d] x 2 | query norms [nq_pad] | tau [nq_pad] | hit counters
 *                [nq_pad x 32] | min(hits, cap) [nq_pad] | survivor counts [nq_pad] | list ids [nq, cap] u32 | list scan
 *                scores [nq, cap] f32 (then: the survivors' ids) | list canonical scores [nq, cap] f64 | survivors' scores
 *                [nq, cap] f64 -- about 24 bytes per list entry.  Nothing of it is read before this call wrote it.
 *   two calls    the caller sizes D and I from lims[nq] -- one host read -- and calls convdr_ip_range_pack with the same
 *                workspace, nq, n, d, cap and lims: it copies every query's ordered run to D + lims[q], I + lims[q] and, when X
 *                is not NULL, the fp64 scores to X + lims[q] (a host-side merge of row slices orders by them).  Exactly
 *                lims[nq] entries of each are written.
 * nq > 0, 0 <= n < 2^31, d % 64 == 0, d <= 4096; store and p_scale as for convdr_ip_search_filtered.  n == 0: counts and lims
 * are zero, status OK, no scan.  Arguments are validated before anything touches a device; no allocation, no sync. */
size_t convdr_ip_range_workspace_bytes(int nq, int64_t n, int d, int cap);
int convdr_ip_range_search(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale,
                           const float* centre, int64_t n, int d, const float* p_max_norm, const float* radius, int cap,
                           int count_only, const uint32_t* row_bits, int64_t row_bits_words, void* workspace,
                           size_t workspace_bytes, int64_t* counts, int64_t* lims, int32_t* status, convdr_stream_t stream);
int convdr_ip_range_pack(const void* workspace, int nq, int64_t n, int d, int cap, const int64_t* lims, float* D, int64_t* I,
                         double* X, convdr_stream_t stream);

/* Score and rank of given rows: where does a KNOWN row stand, and what does it score?  (FAISS: compute_distance_subset; the
 * rank has no FAISS counterpart.)  X is the canonical fp64 score of the search entries throughout.
 *
 * convdr_ip_score_rows: X[q, j] = the canonical score of query q and row rows[q, j], j < m; rows, X and D share the pitch ld
 * (>= m).  The fp32 block is re-scored for store 0 / 1 (p_half is not read), the stored halves for store 2 (p_f32 is not read;
 * the sum over the resident 2^s v is multiplied by 2^-s once, exactly).  D is X rounded to fp32.  Either output may be NULL.
 * An id outside [0, n) -- the -1 that pads a result list -- is never dereferenced and yields the score FAISS pads with,
 * -3.4028235e38.  No workspace, no centre, no scan.  nq, m >= 0, 0 <= n < 2^31, d % 64 == 0, d <= 4096.
 *
 * convdr_ip_rank_rows: one target row per query row (the caller expands (query, target) pairs: np pairs, q_f32 [np, d]).
 *   result       rank[p] = the number of rows r of the block (with a bitmap: of the ALLOWED rows) that precede the target t in
 *                the canonical order of the search entries: X_r > X_t, or X_r == X_t and r < t.  0-based: when rank < k,
 *                row rank of the top-k of the same query is t.  The target need not be allowed itself ("rank among the rows
 *                that are not known positives").  X[p] = X_t.  A target outside [0, n): rank -1, X the padding score,
 *                counts = above = 0, status OK, and no scan work for that column.
 *   thresholds   from X_t, two per query: tau_lo with every rounding pushed DOWN, so that X_r >= X_t implies S~(r) >= tau_lo,
 *                and tau_hi with every rounding pushed UP, so that S~(r) >= tau_hi implies X_r > X_t strictly (proofs beside
 *                k_ip_band_tau; the error terms and eps are those of the range search).  One single-pass scan then COUNTS the
 *                rows with S~ >= tau_hi (above[p]: they certainly precede t) and LISTS the rows with tau_lo <= S~ < tau_hi
 *                (the band: at most 2 eps of scan score wide); only the band is re-scored canonically, and
 *                rank = above + #{band rows that precede t}.  The cost follows the band, not the rank.
 *   status       CONVDR_IP_OK: rank[p] is exact.  CONVDR_IP_OVERFLOW: the band holds more than cap rows; counts[p] = the
 *                scan's exact band count: re-run with cap >= counts[p] -- the thresholds are the same, it cannot overflow
 *                again.  CONVDR_IP_RANGE: as for range search, or an intermediate of the thresholds was not finite.  A pair
 *                that is not OK has rank -1.  counts[p] is the band count and above[p] the counted rows for every status.
 *   cap          a power of two in [1024, 131072]: entries of a pair's band list (global memory).
 *   bitmap       row_bits / row_bits_words: the contract of convdr_ip_search_filtered (NULL, 0: no filter); n_allowed: set bits
 *                among rows 0..n-1, read only with a bitmap -- 0 skips the scan (every rank is 0).
 *   workspace    convdr_ip_rank_workspace_bytes(np, n, d, cap) bytes (0 outside the contract: convdr_last_error says why),
 *                256-byte aligned regions in this order: query operands [nq_pad, d] x 2 | query norms [nq_pad] | tau_lo
 *                [nq_pad] | tau_hi [nq_pad] | band hit counters [nq_pad x 32] | above counters [nq_pad x 32] | min(hits, cap)
 *                [nq_pad] | threshold flags [nq_pad] | band ids [np, cap] u32 | band scan scores [np, cap] f32 | band
 *                canonical scores [np, cap] f64 -- 16 bytes per list entry.  Nothing of it is read before this call wrote it.
 * np > 0, 0 <= n < 2^31, d % 64 == 0, d <= 4096; store, p_scale and centre as for convdr_ip_range_search.  Every output (rank,
 * X, counts, above int64 / fp64 [np], status int32 [np]) must be given.  Arguments are validated before anything touches a
 * device; no allocation, no sync. */
int convdr_ip_score_rows(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale, int64_t n,
                         int d, const int64_t* rows, int m, int64_t ld, double* X, float* D, convdr_stream_t stream);
size_t convdr_ip_rank_workspace_bytes(int np, int64_t n, int d, int cap);
int convdr_ip_rank_rows(int store, const float* q_f32, int np, const int64_t* target, const float* p_f32, const void* p_half,
                        float p_scale, const float* centre, int64_t n, int d, const float* p_max_norm, const uint32_t* row_bits,
                        int64_t row_bits_words, int64_t n_allowed, int cap, void* workspace, size_t workspace_bytes,
                        int64_t* rank, double* X, int64_t* counts, int64_t* above, int32_t* status, convdr_stream_t stream);

/* Removing rows: stable IN-PLACE compaction of a resident row buffer (FAISS: remove_ids).  The buffer is never copied; the
 * extra memory is the workspace, bounded by one window of rows.
 *   keep set     keep_bits / keep_bits_words: the bitmap contract of convdr_ip_search_filtered (16-byte aligned, bit (r & 31) of
 *                word (r >> 5) set = row r is KEPT, whole 256-row tiles zero padded: keep_bits_words >= ceil(n / 256) * 8, bits
 *                past n ignored).  NULL, 0: every row is kept.
 *   result       a kept row r ends at row dest(r) = the number of kept rows before r: the order is preserved, dest(r) <= r,
 *                rows [0, n_kept) of the buffer are the kept rows in order, bit for bit, and rows [n_kept, n) are unspecified.
 *   two calls    convdr_ip_compact_plan, once: per-tile kept counts and their exclusive prefix, written to the workspace, and
 *                the device scalar *n_kept (int64).  Then convdr_ip_compact_rows once per buffer that shares the row numbering
 *                (the fp32 block, the scan copy, the remainder copy), with the same n, bitmap and workspace; the workspace is
 *                sized for the widest row_bytes.  Everything is enqueued on `stream`; the calls between them need no host read.
 *   windows      the buffer is processed in windows of window_rows consecutive source rows, one after the other in stream
 *                order.  Window [a, b) with kept_w kept rows writes [dest(a), dest(a) + kept_w), which ends at or before b and
 *                can overlap only the window's own sources and rows of earlier, finished windows.  Per window, decided on the
 *                device: SKIP (dest(a) == a and kept_w == b - a: nothing removed so far), DIRECT (dest(a) + kept_w <= a: the
 *                destination cannot touch the window's sources) or BOUNCE (one launch packs the kept rows into the bounce
 *                buffer, the next copies them to the destination).  Two launches per window are always enqueued; the one with
 *                nothing to do returns at once.  Ordering is stream order alone: no workgroup waits for another.
 *                window_rows: a multiple of 256 in [256, 1048576].
 *   row_bytes    a multiple of 16 in [16, 65536]; rows are moved as 16-byte pieces with streaming loads and stores.  The
 *                buffer must be 16-byte aligned.
 *   workspace    convdr_ip_compact_workspace_bytes(n, row_bytes, window_rows) bytes (0 outside the contract: convdr_last_error
 *                says why), 256-byte aligned regions in this order: tile prefix u32 [ceil(n / 256) + 1] (the last entry is
 *                n_kept) | chunk sums u32 [ceil((ceil(n / 256) + 1) / 8192)] | bounce buffer window_rows x row_bytes bytes.
 *                convdr_ip_compact_plan writes the first two regions and needs no more than them; convdr_ip_compact_rows
 *                reads the prefix and uses the bounce buffer.  Nothing of it is read before these calls wrote it.
 * 0 <= n < 2^31.  n == 0, or a bitmap that keeps every row: nothing moves, *n_kept is still written.  Arguments are validated
 * before anything touches a device; no allocation, no sync. */
size_t convdr_ip_compact_workspace_bytes(int64_t n, int64_t row_bytes, int64_t window_rows);
int convdr_ip_compact_plan(const uint32_t* keep_bits, int64_t keep_bits_words, int64_t n, void* workspace, size_t workspace_bytes,
                           int64_t* n_kept, convdr_stream_t stream);
int convdr_ip_compact_rows(void* rows, int64_t row_bytes, int64_t n, const uint32_t* keep_bits, int64_t keep_bits_words,
                           int64_t window_rows, void* workspace, size_t workspace_bytes, convdr_stream_t stream);

/* Row ids: which rows of an int64 key column hold a key of a given list, and where (FAISS: IndexIDMap2 -- remove_ids by id, an
 * IDSelector of ids, reconstruct by id).  No table is kept between calls: convdr_keyset_build makes a hash set of the m listed
 * keys in the workspace, and a row pass streams the n row keys (8 bytes per row) and probes it.
 *   the set      open addressing with linear probing; S = the smallest power of two >= max(64, 2 m) slots (load factor <= 1/2);
 *                home slot of key x = mix(x) & (S - 1) with, on uint64,
 *                  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31.
 *                Repeats within the list collapse into one slot, which remembers the smallest list position of its key.
 *   reserved     INT64_MIN marks a free slot and is no legal key: a list that holds it sets bit 0 of *status, a column that
 *                holds it bit 2 of the head's status word; such a list entry is in no slot and such a row never hits.
 *   bounded      every probe loop runs at most S steps; one that ends there sets bit 1 (of *status in the build, of the
 *                head's status word in a row pass) and leaves.  With at most S / 2 slots taken this cannot happen; the bound
 *                is what makes a defect a status bit and not a workgroup that spins.
 *   workspace    convdr_keyset_workspace_bytes(m) bytes (0 outside the contract), 256-byte aligned regions in this order:
 *                head 256 bytes (u32 word 0: status of the last row pass -- bit 1 probe bound, bit 2 reserved key in the
 *                column, bit 3 the workspace holds no set that fits workspace_bytes; u32 word 1: log2 S) | slot keys int64 [S] |
 *                smallest list position u32 [S] | smallest row u32 [S] | row count u32 [S]: 256 + 20 S bytes.
 *                convdr_keyset_build writes all of it; the row passes reset what they accumulate (the last two regions and
 *                word 0) themselves, so one build serves any number of them.  They take S from word 1 and refuse (bit 3; the
 *                outputs are then an all-zero bitmap / (-1, 0, j)) a value whose layout does not fit workspace_bytes.
 *                Nothing of the workspace is read before these calls wrote it.
 * convdr_keyset_build   *status (device int32) = 0 | bit 0 | bit 1.  Two launches (one when m == 0).
 * convdr_keys_member    bits = the row bitmap of convdr_ip_search_filtered / convdr_ip_compact_*: bit (r & 31) of word (r >> 5)
 *                set iff r < n and ((row_keys[r] is in the set) != (invert != 0)); exactly ceil(n / 256) * 8 words are written,
 *                whole 256-row tiles, zero past n (invert applies to rows < n only), with plain stores: every wave ballots its
 *                64 rows into two words.  bits 16-byte aligned, bits_words >= ceil(n / 256) * 8.  counts int64 [2] = (bits
 *                set, distinct list keys found on no row); integer sums, the same in every run.  Three launches.
 * convdr_keys_locate    per list position j < m: first_row[j] (int64) = the smallest row holding keys[j] or -1, count[j]
 *                (int32) = the rows holding it, dup_of[j] (int32, nullable) = the smallest list position with the same key
 *                (j itself for a key that is not repeated, and for INT64_MIN).  keys / m: the list the set was built from.
 *                Three launches: reset, rows (atomicMin / atomicAdd per hit), answers.
 * convdr_ip_compact_ids the id column's share of a removal (convdr_ip_compact_rows moves rows of 16 bytes and more): dst[dest(r)]
 *                = src[r] for every kept row, stable, OUT OF PLACE (src != dst, dst holds n entries), 8 bytes per row.  Reads
 *                the tile prefix convdr_ip_compact_plan wrote to plan_workspace for the same n and bitmap; workspace_bytes
 *                covers the plan's regions.  keep_bits NULL, 0: every row kept (a copy).
 * 0 <= n < 2^31, 0 <= m <= 2^27; n == 0 and m == 0 are legal and write their outputs (row_keys / keys / bits / the per-position
 * outputs may then be NULL).  Arguments are validated before anything touches a device: a refusal is a negative code and a
 * convdr_last_error message; no allocation, no sync. */
size_t convdr_keyset_workspace_bytes(int64_t m);
int convdr_keyset_build(const int64_t* keys, int64_t m, void* workspace, size_t workspace_bytes, int32_t* status,
                        convdr_stream_t stream);
int convdr_keys_member(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, int invert, uint32_t* bits,
                       int64_t bits_words, int64_t* counts, convdr_stream_t stream);
int convdr_keys_locate(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, const int64_t* keys, int64_t m,
                       int64_t* first_row, int32_t* count, int32_t* dup_of, convdr_stream_t stream);
int convdr_ip_compact_ids(const int64_t* src, int64_t* dst, int64_t n, const uint32_t* keep_bits, int64_t keep_bits_words,
                          const void* plan_workspace, size_t workspace_bytes, convdr_stream_t stream);

/* Documents by id: a DOCUMENT is the set of rows that carry one key (the chunk rows of a MaxP block share theirs).  Two
 * primitives: every row of every listed key as a CSR, and the MaxP score -- the best row -- of (query, document) pairs.
 *   the set      convdr_keyset_build of keys[m], into the FRONT of the workspace described below (it needs no more than its
 *                own convdr_keyset_workspace_bytes(m) and may be given the whole size).  The calls below take m again and
 *                refuse on the device (bit 3 of the head's status word; start = count = total = 0, rows[] not written) a set
 *                whose slot count is not the one of m.  Reserved key, probe bound, status words: as under "Row ids".
 * convdr_keys_rows_count   per list position j < m: start[j] (int64), count[j] (int32), dup_of[j] (int32, nullable); *total
 *                (device int64).  The rows that hold keys[j] are rows[start[j] : start[j] + count[j]] of the list the fill
 *                writes.  Segments follow the LIST: the segment of the first occurrence of a key begins where the segments of
 *                the earlier distinct keys end (an exclusive scan over the owning positions), a repeated key shares the
 *                segment of its first occurrence, dup_of[j], and *total counts every distinct key's rows once (total <= n).
 *                A key on no row has count 0 (and the start its segment would have); INT64_MIN has (0, 0, j).
 *                Six launches: reset, rows (convdr_keys_locate's row pass: atomicAdd per hit), block sums, scan of the block
 *                sums (one workgroup), starts, answers.  m == 0: *total = 0.
 * convdr_keys_rows_fill    rows[0 : total] (int64), every segment in ASCENDING row order -- the same bits in every run.  After a
 *                count with the same workspace, m, column and n.  total > rows_cap: NOTHING is written to rows[] and bit 4 of
 *                the head's status word is set; re-run with rows_cap >= total (the count need not be repeated).  A second
 *                pass over the column: every row that hits draws a place in its segment from a per-slot cursor (atomicAdd;
 *                the order inside a segment is then the order of arrival), into a list of (slot, row) entries; the lists are
 *                then ordered: every 256-entry chunk of a segment by rank (at most 256 steps per entry), then runs of width
 *                256, 512, ... merged by binary search in the sibling run (at most 32 steps per entry and pass), one launch
 *                per width below min(n, rows_cap): a segment of any length comes out sorted, n log^2 n work at worst, every
 *                loop bounded, no workgroup waits for another.  3 + ceil(log2(min(n, rows_cap) / 256)) launches (one when
 *                n == 0 or rows_cap == 0); plain vector stores.  For a column other than the count's the result is
 *                unspecified but every access stays inside the workspace and rows[0 : rows_cap].
 *   workspace    convdr_keys_rows_workspace_bytes(m, rows_cap) bytes (0 outside the contract: convdr_last_error says why),
 *                256-byte aligned regions in this order: the key set's regions (256 + 20 S bytes, "Row ids") | head 256 bytes
 *                (u32 word 0: total) | segment start u32 [S] | cursor u32 [S] | block sums u32 [ceil(m / 256)] | list A
 *                u64 [rows_cap] | list B u64 [rows_cap] (entry = slot << 32 | row).  The count needs the size for
 *                rows_cap = 0 and writes head, starts (of the slots in use) and block sums; the fill zeroes the cursors and
 *                writes the lists.  Nothing is read before these calls wrote it.  convdr_keyset_workspace_bytes is unchanged.
 * convdr_ip_score_docs     (query q, segment (start[q, j], count[q, j])) for j < m; start (int64), count (int32), X, D and R share
 *                the pitch ld (>= m).  X[q, j] (fp64, nullable) = the maximum over the segment's rows r = rows[start + i] of the
 *                canonical score of (q, r): for every row the value convdr_ip_score_rows gives, bit for bit (one device
 *                function serves both); D[q, j] (fp32, nullable) = (float)X; R[q, j] (int64, nullable) = the row that attains
 *                it, the LOWEST such row on equal fp64 scores, whatever the order of the list.  The maximum starts below
 *                every score (the first row is taken unconditionally): all-negative scores are ordinary.  An empty segment,
 *                one that does not lie inside rows[0 : rows_len], or one whose entries are all outside [0, n) gives
 *                (-3.4028235e38, -1); an entry outside [0, n) is skipped and never dereferenced.  One wave per pair walks its
 *                segment; one launch, no workspace.  store / p_f32 / p_half / p_scale as for convdr_ip_score_rows.
 *                nq, m >= 0, rows_len >= 0, 0 <= n < 2^31, d % 64 == 0, d <= 4096.
 * 0 <= n < 2^31, 0 <= m <= 2^27, 0 <= rows_cap < 2^31; n == 0 and m == 0 are legal and write their outputs (row_keys / keys /
 * rows / the per-position outputs may then be NULL).  Arguments are validated before anything touches a device: a refusal is a
 * negative code and a convdr_last_error message; no allocation, no sync. */
size_t convdr_keys_rows_workspace_bytes(int64_t m, int64_t rows_cap);
int convdr_keys_rows_count(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, const int64_t* keys, int64_t m,
                           int64_t* start, int32_t* count, int32_t* dup_of, int64_t* total, convdr_stream_t stream);
int convdr_keys_rows_fill(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, int64_t m, int64_t* rows,
                          int64_t rows_cap, convdr_stream_t stream);
int convdr_ip_score_docs(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale, int64_t n,
                         int d, const int64_t* rows, int64_t rows_len, const int64_t* start, const int32_t* count, int m, int64_t ld,
                         double* X, float* D, int64_t* R, convdr_stream_t stream);

/* Document rank: how many DOCUMENTS precede a known row?  A document is the set of rows that carry one key ("Documents by id")
 * and stands where its best row stands -- largest canonical score, lowest row on equal scores --, so document D precedes a
 * target row t iff at least one (allowed) row of D precedes t in the canonical row order, and
 *     doc_rank(q, t) = #{ distinct keys among the allowed rows r that precede t (X_r > X_t, or X_r == X_t and r < t),
 *                         other than the key of row t }.
 * With t the best row of a document this is that document's 0-based position among the documents of the same query.
 * convdr_doc_ordinals   query independent, one pass over the key column: ord[r] (u32 [n]) = the number of distinct keys whose
 *                first row lies below the first row of row_keys[r] -- the documents numbered 0 .. ndocs - 1 in the order of first
 *                appearance --, *ndocs (device int64) = the distinct keys.  The same bits in every run.  A row that holds
 *                INT64_MIN is in no document: ord = 0xffffffff, and bit 2 of the head's status word is set (bit 1: a probe hit
 *                its bound; bit 3: no set -- as under "Row ids").  The key set of "Row ids" is built over the column itself (its
 *                smallest list position is the first row), the rows that own their key are scanned exclusively (block sums, one
 *                workgroup over the block sums, the scan inside each block), a last pass writes ord.  Six launches (two when
 *                n == 0); plain vector stores, the only atomics are the key set's and the status bits.  0 <= n <= 2^27.
 *   workspace    convdr_doc_ordinals_workspace_bytes(n) bytes (0 outside the contract), 256-byte aligned regions in this order:
 *                the key set's regions for a list of n keys (256 + 20 S bytes, S = the smallest power of two >= max(64, 2 n)) |
 *                head 256 bytes (u32 word 0: ndocs, word 1: the build's status) | document number per slot u32 [S] | block sums
 *                u32 [ceil(n / 256)].  Nothing of it is read before this call wrote it.
 * convdr_ip_rank_docs   the arguments of convdr_ip_rank_rows plus ord [n] and ndocs (of the SAME column and n).  target names
 *                rows.  Thresholds, certificate, statuses, cap, bitmap and n_allowed: "Score and rank of given rows", unchanged.
 *                A row with S~ >= tau_hi precedes t for certain: it is counted (above) and ORs its document's bit into the
 *                pair's bitmap -- no slot, no id, no re-score; the band [tau_lo, tau_hi) is listed and re-scored as there, and
 *                the entries that precede t OR their bit afterwards; a last launch counts the set bits with the bit of ord[t]
 *                cleared.  A row whose ordinal is >= ndocs marks nothing.
 *   outputs      rank[p] = doc_rank (-1 unless status is OK; a target outside [0, n): -1, status OK, counts = above = 0);
 *                X[p] = X_t; counts[p] = the band's exact row count (re-run with cap >= counts[p] on CONVDR_IP_OVERFLOW);
 *                above[p] = the ROWS the scan marked without a re-score (above <= the row rank of t); status as there.
 *   workspace    convdr_ip_rank_docs_workspace_bytes(np, n, d, cap, ndocs) bytes (0 outside the contract): the regions of
 *                convdr_ip_rank_workspace_bytes(np, n, d, cap) in their order, then the bitmap u32 [np, mark_words],
 *                mark_words = ceil(ndocs / 32) rounded up to a multiple of 32 (np x ndocs / 8 bytes, whole 128-byte lines per
 *                pair).  The bitmap is zeroed on the stream inside the call; nothing is read before this call wrote it.
 * np > 0, 0 <= n < 2^31, 0 <= ndocs <= n, ord not NULL unless n == 0; everything else as for convdr_ip_rank_rows.  Arguments are
 * validated before anything touches a device: a refusal is a negative code and a convdr_last_error message that names the
 * entry; no allocation, no sync. */
size_t convdr_doc_ordinals_workspace_bytes(int64_t n);
int convdr_doc_ordinals(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, uint32_t* ord, int64_t* ndocs,
                        convdr_stream_t stream);
size_t convdr_ip_rank_docs_workspace_bytes(int np, int64_t n, int d, int cap, int64_t ndocs);
int convdr_ip_rank_docs(int store, const float* q_f32, int np, const int64_t* target, const float* p_f32, const void* p_half,
                        float p_scale, const float* centre, int64_t n, int d, const float* p_max_norm, const uint32_t* row_bits,
                        int64_t row_bits_words, int64_t n_allowed, const uint32_t* ord, int64_t ndocs, int cap, void* workspace,
                        size_t workspace_bytes, int64_t* rank, double* X, int64_t* counts, int64_t* above, int32_t* status,
                        convdr_stream_t stream);

/* Per-query exclusions: every query of a call leaves out ITS OWN rows (its known positives, the passages of its earlier turns,
 * itself).  Nothing here scans: the exclusion is applied to certified results.  With A the allowed rows (all rows without a
 * bitmap) and E_q the excluded rows of query q, the canonical order of A \ E_q is the canonical order of A with E_q removed, so
 *   top-k        = the first k entries of the certified top-(k + |E_q|) of A whose row is not in E_q        (the drop)
 *   rank(q, t)   = rank_A(q, t) - #{x in E_q and A : X_x > X_t, or X_x == X_t and x < t}                     (the count ahead)
 *   range count  = count_A(q) - #{x in E_q and A : X_x > (double)radius_q}               (the count ahead with row_thr = -1)
 * the operand    ex_rows (u32 [nq, ex_ld]) and ex_count (int32 [nq]): row q holds the query's excluded rows ASCENDING and DISTINCT
 *                in its first ex_count[q] words, then 0xffffffff.  ex_ld is a multiple of 4, 4 <= ex_ld <= 16,384.  Membership is
 *                a binary search in the row (at most 15 steps).  A count outside [0, ex_ld] is clamped into it.
 * convdr_excl_build_rows   rows (int64 [nq, e], pitch ld >= e; any order, repeats allowed, negative = padding), e <= 16,384 and
 *                ex_ld >= e.  One workgroup per query: the entries go to LDS, a bitonic network sorts them (the next power of
 *                two >= max(e, 64) words), the first of every run of equal rows is written.  *status (device int32, zeroed on the
 *                stream inside the call) gets bit 0 when a row >= n was met (it is left out).
 * convdr_excl_build_docs   the same from the CSR of convdr_keys_rows_count / convdr_keys_rows_fill: query q excludes every row of its
 *                m segments (start, count)[q, 0 .. m) (pitch ld >= m, m <= 16,384) of csr_rows[0 : rows_len]; a segment that does not
 *                lie inside the list, or is empty, excludes nothing.  The sort always runs over 16,384 words.  Bit 1 of *status:
 *                a query's segments hold more than 16,384 entries (repeats counted): its row is then incomplete.  A query's
 *                distinct rows beyond ex_ld are not written and ex_count is clamped to ex_ld: size ex_ld to min(16,384, rows_len)
 *                rounded up to a multiple of 4 and that cannot happen.
 * convdr_excl_drop_topk    (D, I) [nq, m], pitch ld >= m: a canonical list, padding I = -1 (at the tail; anywhere, it is skipped).
 *                (D_out, I_out) [nq, k], contiguous: the first k entries whose row is not in the query's canonical row, in order,
 *                then (-3.4028235e38, -1); kept[q] (int32) = the survivors BEFORE the cut.  Out of place: the outputs must not
 *                overlap the inputs.  One workgroup per query walks the list in 256-entry chunks: a ballot per wave and a running
 *                base give every survivor its place.  1 <= m <= 2^30 (the searches produce up to 131,072), 1 <= k <= 2^30.
 * convdr_excl_count_ragged / convdr_excl_pack_ragged   the same over a ragged result: query q owns I[lims[q] : lims[q + 1]] (lims
 *                int64 [nq + 1], clamped to [0, total]).  count: kept[q] (int64) = the entries whose row is not excluded.  pack:
 *                those entries, in order, to [lims_out[q] : lims_out[q + 1]] of (D_out, I_out) [total_out] -- never past the run's
 *                end nor past total_out.  lims_out is the exclusive scan of kept, which the caller makes (total_out <= total).
 * convdr_ip_excl_count_ahead   per pair p < np of query pairq[p] (int32; outside [0, nq): ahead = 0) with the threshold (x_thr[p]
 *                fp64, row_thr[p] int64): ahead[p] (int64) = #{x in the query's canonical row : x < n, x allowed, X_x > x_thr or
 *                (X_x == x_thr and x < row_thr)}.  X_x is the value convdr_ip_score_rows gives for (query, x), bit for bit (one
 *                device function serves both).  Allowed: row_bits (NULL, 0: every row), the bitmap of convdr_ip_search_filtered
 *                under that entry's contract (16-byte aligned, whole 256-row tiles).  A rank passes (X_t, t): t itself never
 *                counts.  A range count passes ((double)radius, -1).  One wave per (pair, slice of the list); ahead is zeroed on
 *                the stream inside the call and summed with integer atomic adds.  store / p_f32 / p_half / p_scale as for
 *                convdr_ip_score_rows; nq, np >= 0, 0 <= n < 2^31, d % 64 == 0, d <= 4096.
 * Plain C++ and vector stores only; every loop is bounded by an argument; no workgroup waits for another.  Arguments are validated
 * before anything touches a device: a refusal is a negative code and a convdr_last_error message that names the entry; no
 * allocation, no sync. */
int convdr_excl_build_rows(const int64_t* rows, int nq, int e, int64_t ld, int64_t n, uint32_t* ex_rows, int64_t ex_ld,
                           int32_t* ex_count, int32_t* status, convdr_stream_t stream);
int convdr_excl_build_docs(const int64_t* csr_rows, int64_t rows_len, const int64_t* start, const int32_t* count, int nq, int m,
                           int64_t ld, int64_t n, uint32_t* ex_rows, int64_t ex_ld, int32_t* ex_count, int32_t* status,
                           convdr_stream_t stream);
int convdr_excl_drop_topk(const float* D, const int64_t* I, int nq, int m, int64_t ld, const uint32_t* ex_rows, int64_t ex_ld,
                          const int32_t* ex_count, int k, float* D_out, int64_t* I_out, int32_t* kept, convdr_stream_t stream);
int convdr_excl_count_ragged(const int64_t* lims, const int64_t* I, int64_t total, int nq, const uint32_t* ex_rows, int64_t ex_ld,
                             const int32_t* ex_count, int64_t* kept, convdr_stream_t stream);
int convdr_excl_pack_ragged(const int64_t* lims, const float* D, const int64_t* I, int64_t total, int nq, const uint32_t* ex_rows,
                            int64_t ex_ld, const int32_t* ex_count, const int64_t* lims_out, float* D_out, int64_t* I_out,
                            int64_t total_out, convdr_stream_t stream);
int convdr_ip_excl_count_ahead(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale,
                               int64_t n, int d, const uint32_t* row_bits, int64_t row_bits_words, const uint32_t* ex_rows,
                               int64_t ex_ld, const int32_t* ex_count, int np, const int32_t* pairq, const double* x_thr,
                               const int64_t* row_thr, int64_t* ahead, convdr_stream_t stream);

/* Digest and snapshot file: a resident index (rows in their compacted order, id column, centre, scale, max norm) written to ONE
 * file and read back (FAISS: write_index / read_index), every byte covered by a digest that is checked where the bytes land.
 *   the digest   a buffer is m little-endian 64-bit words w[0 .. m) with a starting word index word0.  With g_i = word0 + i + 1,
 *                mix = the mixer of "Row ids" above, K1 = 0x9e3779b97f4a7c15, K2 = 0xd6e8feb86659fd93, all arithmetic mod 2^64:
 *                  A = sum_i mix(w_i ^ (g_i * K1)),   B = sum_i mix(rotl(w_i, 29) ^ (g_i * K2)).
 *                The digest is (A, B); the empty buffer gives (0, 0).  POSITION-DEPENDENT: swapped, shifted or stale rows show
 *                up, and so does a window of zeros at the wrong place.  ADDITIVE: the digest of a concatenation is the wrapping
 *                sum of the parts' digests taken at their own word0, so any split into windows, chunks or workgroups gives the
 *                same bits; the device sums with integer atomics and is deterministic.  NOT cryptographic: it catches
 *                accidents, not an adversary.
 * convdr_digest_rows   buf: device memory, 8-byte aligned (it need not be 16-byte aligned), n_rows rows of row_bytes bytes,
 *                row_bytes > 0 and a multiple of 8 (at most 2^20; n_rows at most 2^40).  Window j covers rows [j * window_rows,
 *                min(n_rows, (j + 1) * window_rows)), window_rows >= 1 (at most 2^30 windows); its first word has index word0 +
 *                j * window_rows * row_bytes / 8.  out: device uint64 [ceil(n_rows / window_rows)][2] = (A, B) per window; the
 *                entry zeroes it on `stream` and overwrites it, nothing is read from it.  One launch: 16-byte streaming loads
 *                with an 8-byte head / tail where a window starts or ends on an odd word, two 64-bit sums per lane, one pair of
 *                64-bit atomic adds per workgroup.  n_rows == 0: returns 0, launches nothing, writes nothing (buf, out may be NULL).
 * convdr_digest_host   the same function of n_bytes bytes of HOST memory (n_bytes % 8 == 0, any alignment), out[2] = (A, B) on
 *                the host.  No GPU is touched; it may be called from several threads at once.
 * Arguments are validated before anything touches a device: a refusal is a negative code and a convdr_last_error message that
 * names the entry; no allocation, no sync.
 *
 * The snapshot file (one file, little-endian; convdr_amd/snapshot.py writes and reads it):
 *   bytes 0-63   "CONVDRIX" | u32 version = 1 | u32 0 | u64 JSON length | u64 A | u64 B = the digest (word0 = 0) of the JSON bytes
 *                zero padded to a multiple of 8 | 24 zero bytes
 *   from byte 64 the JSON object: d_in, d (the resident width: d_in rounded up to a multiple of 64), storage ("fp32" | "fp16"),
 *                precision, center, n, scale and max_norm (fp32 bit patterns as 8 hex digits), x3_first, has_ids, window_rows,
 *                sections = {name: {offset, bytes, row_bytes, digests}}; digests = one [A, B] per window of window_rows rows as
 *                16-digit hex strings, window j of a section taken at word0 = j * window_rows * row_bytes / 8
 *   sections     each at an offset that is a multiple of 4,096: "rows" n x d elements of the re-score rows at the resident width
 *                (fp32 store: the fp32 block; half store: the resident halves, i.e. already multiplied by the saved scale),
 *                "ids" n x 8 bytes (int64) when has_ids, "centre" ONE row of d x 4 bytes (one window) when centred
 *   not stored   the scan copy and the remainder copy: a pure function of (row, centre, scale), rebuilt by the loader
 * A writer writes the sections first and the header last into a temporary file and renames it; a reader refuses a bad magic,
 * an unknown version, a header digest mismatch, a section that runs past the end of the file and a truncated file. */
int convdr_digest_rows(const void* buf, int64_t n_rows, int64_t row_bytes, uint64_t word0, int64_t window_rows, uint64_t* out,
                       convdr_stream_t stream);
int convdr_digest_host(const void* buf, int64_t n_bytes, uint64_t word0, uint64_t* out);

/* Instrumentation of the last convdr_ip_search on this workspace (device uint32 [nq] each):
 * candidates emitted by the scan / size of the exactly re-scored band. */
const uint32_t* convdr_ip_debug_counts(const void* workspace, int nq, int64_t n, int d, int k, int cap);
const uint32_t* convdr_ip_debug_band(const void* workspace, int nq, int64_t n, int d, int k, int cap);

/* Test aids: the RAW scan scores S~ of the last shallow search (convdr_ip_search, _f16, _h16, _filtered with deep = 0) on this
 * workspace, in scan units (fp16 kinds: query scale x p_scale x q . (p - centre)), before any re-score.  Same arguments as the two
 * accessors above plus out-pointers; both return 0, or a negative code for a NULL pointer or sizes no plan exists for.  The
 * pointers are device pointers into `workspace`, valid until its next search.
 * convdr_ip_debug_list    *id / *s: the candidate list [nq, cap], row ids (uint32) and their scan scores (float); query q's
 *                entries start at q * cap.  The cut REWRITES the list: it compacts the band {S~ >= S~(k) - 2 eps} to the front
 *                and the rest is left in no defined state.  The list therefore holds the scan score of EVERY row exactly when
 *                the band is the whole list: k >= n (the cut is -inf), n <= cap (no threshold pass: every row is a candidate)
 *                and the three-launch chain (convdr_set_option("ip_fused_finish", 0)) -- the plan the exhaustive rung runs.
 *                Its first convdr_ip_debug_band entries per query are then all n rows, each once, in no particular order (the
 *                rows past n of the last 256-row tile, which the scan lists with -inf, are dropped by the cut).  With a row
 *                filter: the allowed rows.  In any other plan only the first convdr_ip_debug_band entries mean anything: the
 *                band's rows and scores.
 * convdr_ip_debug_sample  *T: the threshold sample, *ld its pitch (the padded query count): the score of sampled row i for
 *                query q is T[i * ld + q].  *T is NULL when the plan has no sample (n <= cap).  For cap < n <= 32,768 the
 *                sample is the whole block (every row's scan score, rows n .. the end of the last 256-row tile -inf) -- provided
 *                the call estimated its threshold: tau_in == NULL and no row filter that admits at most cap rows; otherwise
 *                the region is not written.  Above 32,768 rows it holds the two best scores per 64 sampled rows, which steer
 *                the threshold and prove nothing. */
int convdr_ip_debug_list(const void* workspace, int nq, int64_t n, int d, int k, int cap, const uint32_t** id, const float** s);
int convdr_ip_debug_sample(const void* workspace, int nq, int64_t n, int d, int k, int cap, const float** T, int64_t* ld);

/* Two-way merge of per-query result lists: replaces the Python pointer walk of
 *   /root/reference/drivers/run_convdr_inference.py:213-229
 * Da/Ia [nq, na] is the running result (earlier blocks), Db/Ib [nq, nb] the new block's, every row sorted by score
 * descending.  Writes the first n_out (<= na + nb) entries of the complete merge; on equal scores the entry of list
 * A comes first (`>=`, :218) and each list keeps its own order -- the permutation a stable descending sort of the
 * concatenation [A, B] produces.  lda / ldb / ldo: row pitches in elements.  na, nb <= 4096. */
int convdr_topk_merge(const float* Da, const int64_t* Ia, int na, int64_t lda, const float* Db, const int64_t* Ib, int nb,
                      int64_t ldb, int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo, convdr_stream_t stream);

/* W-way merge in ONE launch: the exchange step of the sharded search (every rank's top-k list of every query, all-gathered).
 * nlists lists of n entries per query, every row sorted by score descending; writes the first n_out entries of the
 * complete merge.  On equal scores the entry of the EARLIER list comes first and each list keeps its own order: the
 * permutation a stable descending sort of the concatenation [list 0, ..., list nlists - 1] produces, i.e. what
 * chaining convdr_topk_merge over lists 0 .. nlists - 1 gives.  FAISS padding (-3.4028235e38, -1) sorts like any score;
 * NaN scores are out of contract.  Nothing but the n_out entries of each output row is written.
 *   1 <= nlists, 0 <= n <= 4096, nlists * min(n, n_out) <= 32768, 0 <= n_out <= nlists * n, nq >= 0;
 *   nq == 0 or n_out == 0: returns 0 without a launch; nlists == 1: a copy of the first n_out entries.
 * convdr_topk_merge_multi  list w of query q at D / I + w * list_stride + q * ld (elements; ld >= n), ldo >= n_out.
 * convdr_topk_merge_packed `lists` is the all-gathered exchange buffer [nlists][nq][n] of 12-byte records (score bits,
 *                          offset low word, offset high word), as the ranks put it on the wire. */
int convdr_topk_merge_multi(const float* D, const int64_t* I, int nlists, int n, int64_t list_stride, int64_t ld, int nq,
                            int n_out, float* Dout, int64_t* Iout, int64_t ldo, convdr_stream_t stream);
int convdr_topk_merge_packed(const void* lists, int nlists, int n, int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo,
                             convdr_stream_t stream);

/* Document-level cut of a row-level result: the first entry per key of every query's ranked list, i.e. the `seen_pid` walk of
 *   /root/reference/drivers/run_convdr_inference.py:58-69
 * on the device.  D / I [nq, n] (row pitch ld) is a ranked list per query.  Per query, in position order 0 .. n - 1:
 *   - an entry with I < 0 (FAISS padding) is dropped wherever it stands;
 *   - key = key_map ? key_map[I] : I   (key_map: device int64 [key_map_len], e.g. offset2pid; NULL, 0: the id is the key);
 *   - an I >= key_map_len is never dereferenced: the entry is dropped and the query's n_distinct is reported as -1;
 *   - an entry is kept iff no earlier non-dropped entry has the same 64-bit key.
 * The first n_out kept entries go out in their original order: Dout = score bits unchanged, Iout = the entry's own I (the best
 * row of its key), Kout (nullable) = the key; the remaining slots of the n_out get (-3.4028235e38, -1, -1).  Nothing beyond
 * n_out entries per row is written (row pitch ldo).  counts (nullable, int32 [nq, 2]) = (n_distinct, n_valid): ALL kept
 * entries, before the cut to n_out, and all non-dropped entries.  With them a caller certifies a document-level top-k taken
 * from an exact row-level top-n: it is the exhaustive answer iff n_distinct >= k, or n_valid < n, or n is the whole corpus
 * (DESIGN.md section 4).  Bitwise repeatable; no workspace, no host synchronisation.
 *   0 <= n <= 4096, 0 <= n_out <= 4096, ld >= n, ldo >= n_out, nq >= 0; nq == 0 or n_out == 0: returns 0 without a launch
 *   (counts is then not written). */
int convdr_topk_distinct(const float* D, const int64_t* I, int n, int64_t ld, int nq, const int64_t* key_map, int64_t key_map_len,
                         int n_out, float* Dout, int64_t* Iout, int64_t* Kout, int64_t ldo, int32_t* counts,
                         convdr_stream_t stream);

/* Deep lists: the two list kernels above for lists of up to 65,536 entries, what a row search beyond k = 4,096
 * (convdr_ip_search_deep) hands on.  Same contracts, same bytes wherever the shallow entry accepts the shape; the lists stay
 * in global memory.  Arguments are validated before anything touches a device.
 *
 * convdr_topk_distinct_deep   convdr_topk_distinct, word for word: padding ids dropped, key_map / key_map_len, n_distinct = -1
 *   for an id >= key_map_len, an entry kept iff it is the first of its 64-bit key, score bits / I / K out with the
 *   (-3.4028235e38, -1, -1) tail, counts = (n_distinct, n_valid), nothing past n_out written, bitwise repeatable, no host
 *   synchronisation.  0 <= n <= 65536, 0 <= n_out <= 65536, ld >= n, ldo >= n_out, nq >= 0, Kout and counts nullable;
 *   nq == 0 or n_out == 0: returns 0 without a launch (counts is then not written).  One 1,024-thread workgroup per query.
 *   workspace (device, workspace_bytes >= convdr_topk_distinct_deep_workspace_bytes(nq, n)): the staged keys int64 [nq][n],
 *   rounded up to 256 bytes, then the open-addressing tables uint32 [nq][2^hbits], 2^hbits the smallest power of two >= 2n
 *   and >= 64 -- at most 512 KB + 512 KB per query.  The kernel initialises what it reads: no result depends on what the
 *   workspace or the outputs held before.
 * convdr_topk_distinct_deep_workspace_bytes   0 for sizes outside the contract (nq < 0, n < 0, n > 65536).
 *
 * convdr_topk_merge_deep / convdr_topk_merge_deep_packed   convdr_topk_merge_multi / convdr_topk_merge_packed with the same
 *   arguments (plain pitches / the [nlists][nq][n] 12-byte records of the exchange, read in place) and the same permutation:
 *   the stable descending sort of [list 0, ..., list nlists - 1], earlier lists first on equal scores, FAISS padding sorted
 *   like a score, NaN out of contract.  Nothing but the n_out entries of each output row is written; no workspace.
 *   1 <= nlists <= 64, 0 <= n <= 65536, 0 <= n_out <= nlists * n, nlists * min(n, n_out) < 2^31, nq >= 0, ld >= n,
 *   ldo >= n_out, list_stride >= n where nlists > 1; nq == 0 or n_out == 0: returns 0 without a launch.  A query's
 *   nlists * min(n, n_out) elements are cut into chunks of 1,024 over grid.y (at most 4,096 chunks), queries on grid.x. */
size_t convdr_topk_distinct_deep_workspace_bytes(int nq, int n);
int convdr_topk_distinct_deep(const float* D, const int64_t* I, int n, int64_t ld, int nq, const int64_t* key_map,
                              int64_t key_map_len, int n_out, float* Dout, int64_t* Iout, int64_t* Kout, int64_t ldo,
                              int32_t* counts, void* workspace, size_t workspace_bytes, convdr_stream_t stream);
int convdr_topk_merge_deep(const float* D, const int64_t* I, int nlists, int n, int64_t list_stride, int64_t ld, int nq,
                           int n_out, float* Dout, int64_t* Iout, int64_t ldo, convdr_stream_t stream);
int convdr_topk_merge_deep_packed(const void* lists, int nlists, int n, int nq, int n_out, float* Dout, int64_t* Iout,
                                  int64_t ldo, convdr_stream_t stream);

/* Judging a run: join a ranked key list per query with that query's judged set (the qrels) on the device.  Replaces the
 * per-entry dict lookup of the reference's drivers/run_convdr_inference.py:98-99, the trec_eval step that follows its .trec
 * file, and the two walks over a text run file of its data/gen_ranking_data.py:539-567.
 *   run          K int64 [nq, n], row pitch ld >= n: per query a ranked list of DISTINCT keys (what convdr_topk_distinct[_deep]
 *                writes as Kout); a negative entry is padding wherever it stands.  0 <= n <= 65536, nq >= 0.
 *   qrels        a CSR over the SAME query order: off int64 [nq + 1] (off[0] = 0, monotone, off[nq] = nnz), and per query q in
 *                [off[q], off[q + 1]): key int64 strictly ascending, grade int32 (<= 0: judged non-relevant; the two sentinel
 *                values below are not grades), ideal int32 = the segment's positive grades sorted descending, then zeros.
 *                The library cannot check these on the device (convdr_amd/judge.py checks them when it packs); a segment is
 *                clamped to [0, nnz] before use, so a wrong off gives wrong answers, never an access outside the arrays.
 *   labels       int32 [nq, n] (dense): the grade of K[q, r] in q's segment, found by binary search on the full 64-bit key,
 *                CONVDR_LABEL_UNJUDGED for a key that is not there, CONVDR_LABEL_PAD for padding.
 *
 * convdr_run_measures: out fp64 [nq, 4 + 3 nc].  An entry is RELEVANT iff label >= rel_level (>= 1); its GAIN is
 * max(label, 0) whatever rel_level is; sentinels are neither.  Ranks r start at 1; c runs over the nc cutoffs (a HOST array,
 * each >= 1, strictly ascending, nc <= 16).  Columns:
 *   0            num_rel      qrels entries of the query with grade >= rel_level
 *   1            num_rel_ret  relevant entries of the list
 *   2            recip_rank   1 / r of the first relevant entry, else 0
 *   3            map          (sum over relevant ranks r of #relevant in 1..r / r) / num_rel; 0 when num_rel = 0
 *   4 + i        ndcg_cut_c   DCG_c / IDCG_c; DCG_c = sum over r <= min(c, n) of gain_r / log2(r + 1), IDCG_c the same sum over
 *                             the first c values of ideal; 0 when IDCG_c = 0
 *   4 + nc + i   recall_c     #relevant in 1..min(c, n) / num_rel; 0 when num_rel = 0
 *   4 + 2nc + i  P_c          #relevant in 1..min(c, n) / c
 * All in fp64; the counts and the single divisions are exact / correctly rounded, the two sums (map, DCG) are made in a fixed
 * order that is not the ascending-rank order (at most 65,536 non-negative terms: relative error below 1e-11), and a call
 * repeats bit for bit.  These are the usual trec_eval per-query definitions restated; agreement is claimed with THESE FORMULAS
 * (tests/judge_cases.py), not with the trec_eval binary, which nothing here runs.  Averaging over queries is the caller's.
 *
 * convdr_run_negatives: the negative list of gen_ranking_data.py:539-567 for one ranked list per query.  out_keys (and out_rows,
 * with I = the row ids of the same entries, pitch ld; both or neither) int64 [nq, W], W = max(n, fill_to), -1 padded; counts
 * int32 [nq].  A query with no qrels entry of grade > 0 gets count 0 (the reference's `positive_ids != {}`).  Otherwise A then B:
 *   A            every entry whose label is a judged grade <= 0, in list order, uncapped;
 *   B            the first max(0, fill_to - |A|) entries, in list order, that are not positives (label <= 0 or not judged;
 *                padding skipped).  B REPEATS members of A: the reference's second pass appends without looking at the first's.
 * fill_to in [0, 65536] (the reference: 20).  Sampling num_negs of the list stays with the caller.
 *
 * Every array but cutoffs is a device pointer; key, grade, ideal may be NULL when nnz = 0, K / I / labels when n = 0.  nq = 0
 * (and n = 0 for convdr_run_label): returns 0 without a launch.  Arguments are validated before anything touches a device; no
 * allocation, no sync, no workspace.  One 1,024-thread workgroup per query walks the list 1,024 ranks at a time. */
#define CONVDR_LABEL_PAD (-2147483647 - 1)  /* the entry is padding                       */
#define CONVDR_LABEL_UNJUDGED (-2147483647) /* the key is not in the query's qrels segment */
int convdr_run_label(const int64_t* K, int n, int64_t ld, int nq, const int64_t* off, const int64_t* key, const int32_t* grade,
                     int64_t nnz, int32_t* labels, convdr_stream_t stream);
int convdr_run_measures(const int32_t* labels, int n, int nq, const int64_t* off, const int32_t* grade, const int32_t* ideal,
                        int64_t nnz, int rel_level, const int32_t* cutoffs, int n_cutoffs, double* out, convdr_stream_t stream);
int convdr_run_negatives(const int64_t* K, const int64_t* I, int n, int64_t ld, int nq, const int32_t* labels, const int64_t* off,
                         const int32_t* grade, int64_t nnz, int fill_to, int64_t* out_keys, int64_t* out_rows, int32_t* counts,
                         convdr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dual-encoder forward: replaces the HuggingFace RobertaModel / BertModel forward + pooling + head
 * behind  /root/reference/model/models.py:140-148 (RobertaDot_NLL_LN.query_emb / body_emb) and
 * :205-211, :227-235 (HFBertEncoder.forward, BiEncoder.query_emb / body_emb).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t kind;        /* 0 = RoBERTa position ids (cumsum(ids != pad_idx) * (ids != pad_idx) + pad_idx), 1 = BERT (0..L-1) */
  int32_t hidden, heads, layers, intermediate;   /* head_dim = hidden / heads must be 64 */
  int32_t vocab, max_pos, pad_idx;
  int32_t out_dim;     /* 768 for rdot_nll (embeddingHead + norm, models.py:136-137); 0 = raw CLS (dpr, models.py:210) */
  float ln_eps;        /* encoder LayerNorms (1e-5 RoBERTa, 1e-12 BERT) */
  float head_ln_eps;   /* nn.LayerNorm(768) default 1e-5 */
  int32_t pool_mean;   /* 0 = CLS pooling emb_all[0][:, 0] (every registered config, models.py:43); 1 = masked mean over the
                        * sequence's tokens (EmbeddingMixin.masked_mean, models.py:32-35, use_mean = True) */
} convdr_encoder_config;

typedef struct {       /* device pointers; w* are bf16 [out, in] row-major (nn.Linear layout), the rest fp32 */
  const void* wqkv;    /* [3H, H] = rows of attention.self.{query,key,value}.weight stacked */
  const float* bqkv;   /* [3H] */
  const void* wo;      /* attention.output.dense.weight [H, H] */
  const float* bo;
  const float *ln1_g, *ln1_b; /* attention.output.LayerNorm */
  const void* w1;      /* intermediate.dense.weight [I, H] */
  const float* b1;
  const void* w2;      /* output.dense.weight [H, I] */
  const float* b2;
  const float *ln2_g, *ln2_b; /* output.LayerNorm */
  /* Optional (NULL = absent): wo / w2 again in K-slice-major order [in / 32][H][32] (convdr_pack_kslice), read by the
   * fused projection + residual + LayerNorm kernel of the inference forward (hidden == 768, >= 24576 packed rows):
   * a 32-wide K slice of all H output rows is then one contiguous 48 KB run of whole cache lines.  Ignored by the
   * training entry points. */
  const void* wo_ks;
  const void* w2_ks;
} convdr_layer_weights;

typedef struct {
  const float *word_emb, *pos_emb, *type_emb; /* fp32 [vocab, H], [max_pos, H], [>=1, H] (row 0 used) */
  const float *emb_ln_g, *emb_ln_b;
  const convdr_layer_weights* layers;         /* HOST array of `layers` entries */
  const void* head_w;                         /* bf16 [out_dim, H] (out_dim > 0) */
  const float *head_b, *head_ln_g, *head_ln_b;
} convdr_encoder_weights;

/* fp32 -> bf16 (round to nearest even); n % 4 == 0.  Used to pack weights at load time / after an optimizer step. */
int convdr_cast_f32_bf16(const float* x, void* y, int64_t n, convdr_stream_t stream);

/* bf16 [n, k] row-major -> K-slice-major bf16 [k / 32][n][32]  (out[(s * n + r) * 32 + c] = w[r * k + 32 s + c]);
 * k % 32 == 0.  See convdr_layer_weights.wo_ks / w2_ks. */
int convdr_pack_kslice(const void* w_bf16, int n, int k, void* out, convdr_stream_t stream);

size_t convdr_encoder_workspace_bytes(const convdr_encoder_config* cfg, int64_t rows, int B);

/* Status word of an encoder forward: the first int32 of `workspace` (inference and training forward alike), zeroed at
 * the start of the call and OR-ed by the packing kernel.  The reference raises IndexError from nn.Embedding for a token
 * id outside the table (model/models.py:141-142); a kernel cannot raise, so the id is clamped to 0 (no out-of-bounds
 * read, no out-of-bounds atomic in the backward), the flag is set, and the host raises when it next reads the word
 * (the outputs of a flagged batch are meaningless). */
#define CONVDR_ENC_STATUS_BAD_TOKEN 1  /* a token id < 0 or >= cfg->vocab under the mask                       */
#define CONVDR_ENC_STATUS_BAD_LENS 2   /* seq_lens[b] != number of unmasked tokens of row b (or > L)          */
#define CONVDR_ENC_STATUS_BAD_MASK 4   /* attention_mask[b, 0] == 0: the CLS position must be a real token    */

/* out[b, :] = embedding of sequence b.  input_ids / attention_mask: device int64 [B, L] exactly as the reference
 * drivers pass them (gen_passage_embeddings.py:105-112); with ids_are_int32 != 0 input_ids is int32 [B, L] (token-cache
 * records, data/tokenizing.py:116) and attention_mask may be NULL = "l < seq_lens[b]" (what GetProcessingFn builds,
 * data/tokenizing.py:138-140).  Only mask == 1 tokens are computed ("packed rows"):
 * cu_seqlens (device int32 [B+1]) gives each sequence's first row, multiples of 8, cu[B] == rows;
 * seq_lens (device int32 [B]) = mask.sum(1) >= 1; mask[b, 0] must be 1 (the CLS position).  max_len = max(seq_lens).
 * max_len sizes the attention grid and is a host value the library cannot check against the device array: it must be
 * >= max(seq_lens) (a smaller one leaves the query rows past it without attention output; a larger one only costs idle
 * workgroups).
 * out: device fp32 [B, out_dim or hidden]. */
int convdr_encoder_forward(const convdr_encoder_config* cfg, const convdr_encoder_weights* w,
                           const void* input_ids, int ids_are_int32, const int64_t* attention_mask, int B, int L,
                           const int32_t* cu_seqlens, const int32_t* seq_lens, int64_t rows, int max_len,
                           void* workspace, size_t workspace_bytes, float* out, convdr_stream_t stream);

/* The same forward for RAGGED input: instead of a padded [B, L] matrix and its mask, `tokens` (device int32 [n_tokens])
 * holds the unmasked tokens of all B sequences back to back with no padding, and tok_offsets (device int32 [B+1]) where
 * each begins: sequence b is tokens[tok_offsets[b] .. tok_offsets[b+1]), tok_offsets[b+1] - tok_offsets[b] == seq_lens[b],
 * tok_offsets[B] <= n_tokens.  This is what a right-padded ("prefix") mask keeps; a mask with holes is not representable
 * and stays with convdr_encoder_forward.  So sequences that arrive in batches of different widths run in one forward
 * without being re-padded to the widest.  cu_seqlens, seq_lens, rows, max_len (>= max(seq_lens), as above), workspace
 * (convdr_encoder_workspace_bytes), the status word, convdr_encoder_debug_layout and `out` are those of
 * convdr_encoder_forward, and for the same sequences, cu_seqlens and B the result is bit-identical to it.
 * Requires B > 0, n_tokens >= B, rows % 8 == 0, rows >= n_tokens, 0 < max_len <= n_tokens.  A sequence whose offsets are
 * not as stated (or do not fit its rows cu[b+1] - cu[b]) is not read: CONVDR_ENC_STATUS_BAD_LENS is set and its rows are
 * computed as empty; no read ever goes past tokens + n_tokens. */
int convdr_encoder_forward_ragged(const convdr_encoder_config* cfg, const convdr_encoder_weights* w,
                                  const int32_t* tokens, int64_t n_tokens, const int32_t* tok_offsets, int B,
                                  const int32_t* cu_seqlens, const int32_t* seq_lens, int64_t rows, int max_len,
                                  void* workspace, size_t workspace_bytes, float* out, convdr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training step of the student encoder: replaces, for /root/reference/drivers/run_convdr_train.py:109-191,
 *   embs = model(concat_ids, concat_id_mask)          -> convdr_encoder_train_forward (keeps activations)
 *   loss_fn(embs, teacher_embs)           :115, :460   -> convdr_mse_fwd_bwd
 *   logits / loss_fn_2(logits, labels)    :160-170     -> convdr_rank_ce_fwd_bwd
 *   loss.backward()                       :178         -> convdr_encoder_backward
 *   clip_grad_norm_(.., max_grad_norm)    :188-189     -> convdr_grad_norm_clip
 *   optimizer.step()  (HF AdamW, utils/dpr_utils.py:80-87) -> convdr_adamw_step
 * Dropout (run_convdr_train.py:107 model.train(): hidden / attention-probability dropout inside the HF encoder): torch's
 * RNG stream cannot be matched, so the mask is a documented counter-based function of (seed, site, layer, element)
 * (csrc/dropout.hpp, restated in oracle/dropout.py); the backward regenerates it.  NULL / p = 0: identity.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  float p_hidden;      /* config.hidden_dropout_prob: embeddings output, attention-output dense, FFN-output dense */
  float p_attention;   /* config.attention_probs_dropout_prob: softmax probabilities */
  uint32_t seed;       /* the SAME value for a forward and its backward */
} convdr_dropout;

typedef struct {   /* bf16 transposed weights for the data-gradient GEMMs (device pointers) */
  const void* wqkv_t;  /* [H, 3H] */
  const void* wo_t;    /* [H, H]  */
  const void* w1_t;    /* [H, I]  */
  const void* w2_t;    /* [I, H]  */
} convdr_layer_weights_t;

typedef struct {   /* fp32 gradient buffers, ACCUMULATED into (+=); same shapes as the parameters */
  float *wqkv, *bqkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
} convdr_layer_grads;

typedef struct {
  float *word_emb, *pos_emb, *type_emb;   /* only row 0 of type_emb receives gradient */
  float *emb_ln_g, *emb_ln_b;
  const convdr_layer_grads* layers;       /* HOST array */
  float *head_w, *head_b, *head_ln_g, *head_ln_b;
} convdr_encoder_grads;

size_t convdr_encoder_train_workspace_bytes(const convdr_encoder_config* cfg, int64_t rows, int B);

/* Same contract as convdr_encoder_forward; additionally leaves every activation the backward needs in `workspace`
 * (which must stay untouched until convdr_encoder_backward has been enqueued). */
int convdr_encoder_train_forward(const convdr_encoder_config* cfg, const convdr_encoder_weights* w,
                                 const void* input_ids, int ids_are_int32, const int64_t* attention_mask, int B, int L,
                                 const int32_t* cu_seqlens, const int32_t* seq_lens, int64_t rows, int max_len,
                                 void* workspace, size_t workspace_bytes, float* out, const convdr_dropout* dropout,
                                 convdr_stream_t stream);

/* d_out: fp32 [B, out_dim or hidden] gradient of the loss w.r.t. the embeddings.  wt: HOST array of `layers`
 * entries; head_w_t: bf16 [hidden, out_dim] (NULL when out_dim == 0). */
int convdr_encoder_backward(const convdr_encoder_config* cfg, const convdr_encoder_weights* w,
                            const convdr_layer_weights_t* wt, const int32_t* cu_seqlens, const int32_t* seq_lens,
                            const void* head_w_t, int B, int64_t rows, int max_len, void* workspace,
                            size_t workspace_bytes, const float* d_out, const convdr_encoder_grads* grads,
                            const convdr_dropout* dropout, convdr_stream_t stream);

/* The same backward for gradient buffers NOBODY HAS WRITTEN YET (what autograd hands loss.backward() on the first backward after
 * zero_grad(): /root/reference/drivers/run_convdr_train.py:178,190): every gradient except the embedding tables is STORED by the one
 * kernel that completes it (weight-gradient tiles, the partial-sum reductions) instead of added to the buffer's contents, so
 * only grads->word_emb / pos_emb / type_emb / emb_ln_g / emb_ln_b must be zero on entry (the tables are scatter-added: token rows
 * repeat) and the other buffers may hold anything.  Bit-identical to convdr_encoder_backward on all-zero buffers; saves the
 * fill of, and one read of, every weight gradient (0.7 GB per step for roberta-base). */
int convdr_encoder_backward_fresh(const convdr_encoder_config* cfg, const convdr_encoder_weights* w,
                                  const convdr_layer_weights_t* wt, const int32_t* cu_seqlens, const int32_t* seq_lens,
                                  const void* head_w_t, int B, int64_t rows, int max_len, void* workspace,
                                  size_t workspace_bytes, const float* d_out, const convdr_encoder_grads* grads,
                                  const convdr_dropout* dropout, convdr_stream_t stream);

/* One weight gradient of the backward above, exposed for parity tests at arbitrary shapes:
 *   dW[n, k] += sum_t dy[t, n] * x[t, k]     (what autograd's Linear backward computes for
 *   /root/reference/drivers/run_convdr_train.py:178; dy / x bf16 row-major with row strides ld_dy / ld_x, fp32 out)
 * straight from the token-major operands (TN MFMA engine, csrc/gemm_tn.hpp).  N, K and the strides are multiples of 8.
 * slab: fp32 scratch of slab_elems >= N * K elements (more lets the contraction be split across more workgroups; the
 * slices are summed in a fixed order: deterministic). */
int convdr_wgrad(const void* dy, int N, int64_t ld_dy, const void* x, int K, int64_t ld_x, int64_t rows, float* slab,
                 size_t slab_elems, float* dW, convdr_stream_t stream);

/* Gradient all-reduce under the backward (replaces what DistributedDataParallel's bucket hooks do for
 * /root/reference/drivers/run_convdr_train.py:52,178): makes `stream` wait until every gradient of encoder layer
 * `layer` written by the most recent convdr_encoder_backward on the current device is complete (the layers finish in
 * the order layers-1 .. 0; embeddings and head only with the whole call).  The caller then enqueues the collective for
 * that layer's slice of the gradient arena on `stream` while the backward of the layers below is still running.
 * layer = -1: the embedding tables and the embedding LayerNorm -- written by the call's last kernels on its own stream,
 * while the last weight-gradient branch may still be running (the call's stream only joins it afterwards). */
int convdr_backward_wait_layer(int layer, convdr_stream_t stream);

/* fp32 [n, k] row-major -> bf16 [k, n] (packing of the transposed weights) */
int convdr_transpose_f32_bf16(const float* x, int n, int k, void* y, convdr_stream_t stream);

/* Batched form: for i < count, fp32 [n[i], k[i]] at base + src_off[i] -> bf16 [k[i], n[i]] at out + dst_off[i]
 * (offsets in elements; src_off / n / k / dst_off are HOST arrays). */
int convdr_pack_transposed(const float* base, int count, const int64_t* src_off, const int32_t* n, const int32_t* k,
                           const int64_t* dst_off, void* out, convdr_stream_t stream);

/* The same from a bf16 source: bf16 [n[i], k[i]] at (bf16*)base + src_off[i] -> bf16 [k[i], n[i]].  For hosts that keep a bf16 copy
 * of the weights current (convdr_adamw_step_packed does): a third less traffic per training step than re-rounding the fp32 master
 * weights, same bits. */
int convdr_pack_transposed_bf16(const void* base, int count, const int64_t* src_off, const int32_t* n, const int32_t* k,
                                const int64_t* dst_off, void* out, convdr_stream_t stream);

/* loss[0] = mean((s - t)^2) over n elements (nn.MSELoss); ds (nullable) = grad_scale * 2 (s - t) / n */
int convdr_mse_fwd_bwd(const float* s, const float* t, int64_t n, float grad_scale, float* loss, float* ds,
                       convdr_stream_t stream);

/* logits[b, k] = <embs[b], docs[b, k]>, k = 0 is the positive; loss_per_query[b] = -log_softmax(logits[b])[0]
 * (nn.CrossEntropyLoss = their mean); d_embs (nullable) (+)= grad_scale / B * sum_k (softmax - onehot0) docs[b, k].
 * embs [B, E], docs [B, K, E] fp32, K <= 64. */
int convdr_rank_ce_fwd_bwd(const float* embs, const float* docs, int B, int K, int E, float grad_scale,
                           float* loss_per_query, float* d_embs, int accumulate, convdr_stream_t stream);

/* In-batch-negative form of the ranking loss (BASELINE configs[4]: the B x K teacher document embeddings of every rank
 * are all-gathered; NOT in the reference, whose formula above stays the default -- defined by
 * oracle/train.py:inbatch_rank_loss): logits[b, n] = <embs[b], docs[n]> over ALL N gathered documents,
 * loss_per_query[b] = -log_softmax(logits[b])[pos[b]] with pos[b] the row of query b's own positive document;
 * d_embs (nullable) (+)= grad_scale / B * sum_n (softmax - onehot(pos[b])) docs[n].  embs [B, E], docs [N, E] fp32,
 * pos device int32 [B], N <= 16384. */
/* The pairwise NLL of the model surface -- NLL.forward(q, a, b) (/root/reference/model/models.py:66-75; BiEncoder.forward
 * :254-262) and its MaxP form NLL_MultiChunk.forward (:92-126) -- with gradients for ALL three inputs (a and b are student
 * outputs here, not frozen teacher embeddings):  s_x[i] = max_c(<q[i], x[i, c]> + bias_x[i, c]) for x in {a, b} (C chunks per
 * document; C = 1 and NULL biases: the plain pairwise form; the first maximal chunk wins, like torch.max),
 * loss_per_query[i] = -log_softmax([s_a, s_b])[0]; d_q / d_a / d_b (each nullable) = grad_scale / B * d(sum_i loss_i) / d(.),
 * overwritten (non-selected chunks get zeros).  q [B, E], a / b [B, C, E], biases [B, C] fp32; C <= 32. */
int convdr_pair_nll_fwd_bwd(const float* q, const float* a, const float* b, const float* bias_a, const float* bias_b, int B,
                            int C, int E, float grad_scale, float* loss_per_query, float* d_q, float* d_a, float* d_b,
                            convdr_stream_t stream);

int convdr_inbatch_ce_fwd_bwd(const float* embs, const float* docs, int B, int N, int E, const int32_t* pos,
                              float grad_scale, float* loss_per_query, float* d_embs, int accumulate,
                              convdr_stream_t stream);

/* torch.nn.utils.clip_grad_norm_ over one flat fp32 gradient buffer whose entries still have to be multiplied by
 * pre_scale (1 / world size after a SUM all-reduce; 1 otherwise):  norm_and_coef[0] = ||pre_scale * g||_2,
 * norm_and_coef[1] = pre_scale * min(1, max_norm / (norm + 1e-6)) = the factor the stored gradients are multiplied by;
 * apply != 0 does that in place, otherwise the caller hands norm_and_coef + 1 to convdr_adamw_step (grad_scale).
 * scratch: >= 1024 floats. */
int convdr_grad_norm_clip(float* grads, int64_t n, float max_norm, float pre_scale, float* scratch, float* norm_and_coef,
                          int apply, convdr_stream_t stream);

/* The two halves of convdr_grad_norm_clip, for callers that sum a gradient arena piece by piece -- e.g. every encoder
 * layer's slice on a side stream as soon as convdr_backward_wait_layer says it is complete, under the backward of the
 * layers below, so that only the last pieces are summed after the backward:
 *   convdr_grad_sumsq:       partials[b] = sum of squares of block b's share of x[0, n), b < nblocks (<= 1024)
 *   convdr_grad_norm_finish: norm_and_coef as convdr_grad_norm_clip, from `count` partial sums (any order of pieces: the
 *                            finish folds them in index order in fp64 -- deterministic for a fixed layout) */
int convdr_grad_sumsq(const float* x, int64_t n, float* partials, int nblocks, convdr_stream_t stream);
int convdr_grad_norm_finish(const float* partials, int count, float max_norm, float pre_scale, float* norm_and_coef,
                            convdr_stream_t stream);

/* The stream convdr_encoder_backward runs its weight-gradient branches on (default: one it creates itself).  HIP multiplexes
 * streams onto GPU_MAX_HW_QUEUES hardware queues in order of first use; a caller that has verified that `stream` runs
 * concurrently with its compute stream hands it in here.  Per device (the stream must belong to the CURRENT device, else
 * an error is returned); may be called again between two backward calls to move the branch to another stream (every
 * backward ends with the caller's stream waiting for the branch, so nothing is pending in between). */
int convdr_train_set_side_stream(convdr_stream_t stream);

/* x[i] *= scale[0] (device scalar), e.g. the clip coefficient */
int convdr_scale_f32(float* x, int64_t n, const float* scale, convdr_stream_t stream);

/* transformers==2.3.0 AdamW on flat fp32 buffers (NOT torch.optim.AdamW: eps is added to sqrt(v) before the bias
 * correction, decoupled weight decay is applied after the update).  grad_scale: optional device scalar multiplied
 * into g first (the clip coefficient).  step >= 1. */
int convdr_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int step, int correct_bias, const float* grad_scale,
                      convdr_stream_t stream);
/* The same update, also refreshing the packed bf16 copy of the weights that the encoder GEMMs read (what
 * convdr_cast_f32_bf16 over p[bf16_first, n) would produce afterwards): bf16_copy[i - bf16_first] = bf16(p[i]) for
 * i >= bf16_first, written from the registers that hold the new weight -- the training step then has no cast pass over
 * the parameter arena.  bf16_copy == NULL: exactly convdr_adamw_step.  bf16_first % 4 == 0. */
int convdr_adamw_step_packed(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int step, int correct_bias, const float* grad_scale,
                             void* bf16_copy, int64_t bf16_first, convdr_stream_t stream);

/* Tuning / test knobs: "fused_ln_min_rows" = minimum packed rows for the fused GEMM + residual + LayerNorm kernel
 * (default 24576; tests lower it to exercise that kernel on small inputs); "fused_ln_max_k" = largest contraction
 * length it is used for; "hm_blocked" = 0 / 1: row-major / blocked layout of the FFN activation between FFN1 and the
 * fused FFN2 + LayerNorm kernel (default 1; a workspace-internal choice, results are identical); "cls_fold" = 1 / 0: the last
 * layer of the inference forward with CLS pooling folds Wk and Wv through the CLS query and reads the layer input once (K and
 * V are never formed) / projects K and V of every token and runs the CLS-query attention (default 1; rounding-level
 * differences; "cls_fold_min_rows" = packed rows from which the first form is taken, default 16,384: below, the second is
 * faster; batches averaging under hidden / 32 packed rows per sequence take the second form either way); "attn_bwd_fused" = 1 / 0:
 * training backward of the attention in one workgroup per (sequence, head) for sequences of at most 256 tokens / always the
 * dQ kernel + the dK, dV kernel (default 1); "gelu_gp" = 1 / 0: gelu' evaluated in the training forward's FFN1 epilogue / the
 * pre-activation saved and a separate pass in the backward; "ip_fused_finish" = 1 / 0: one / three launches behind a scan;
 * "ffn2_splitk" = 1 / 0: the K = 3072 projection of at most 5,376 packed rows as 4 / 2 contraction slices + a finishing row
 * kernel / as whole-contraction tiles (default 1; fp32 summation order differs);
 * "ln_rows", "ln_bwd_rows" = straight-line LayerNorm forward (1 / 0) and backward (2 / 1 / 0) kernels for hidden size 768 against
 * the general ones (same formulas, rounding-level differences); "train_bwd_stop_layer" = test aid, default -1 (off): with value
 * l >= 0 convdr_encoder_backward[_fresh] enqueues the head and the layers down to and including l (data gradients, parameter
 * gradients, the layer's events) and skips the layers below and the embedding backward (l >= layers: no layer at all), so the
 * buffers every layer rewrites still hold layer l's values; the events of convdr_backward_wait_layer and the final join are
 * recorded as usual; "gemm_trace" / "gemm_trace_ln" = device buffer for the s_memtime phase stamps of a
 * `make TRACE=1` build (tools/gemm_trace*.py; 0 = off). */
int convdr_set_option(const char* name, int64_t value);

/* Test aid: byte offsets of the activation buffers inside the encoder workspace, in the order tok_id, tok_pos, X, Q, K,
 * Vt, ctx, Hm, Y, cls_b, cls_y, cls_f, head_y; out[13] = leading dimension of Vt. */
int convdr_encoder_debug_layout(const convdr_encoder_config* cfg, int64_t rows, int B, int64_t* out);

/* Test aid: byte offsets of the regions of the TRAINING workspace (convdr_encoder_train_workspace_bytes), as the training
 * forward and backward themselves plan them, -1 for a region this configuration does not have.  Order:
 *   tok_id, tok_pos, order;
 *   for each layer: Xin, QKV, ctx, LSE, Mbits, X1, Hpre, Hm, Y1, Y2   (X1 .. Y2 = -1 for the last layer under CLS pooling, whose
 *                   tail lives in the compact c_* regions);
 *   for each layer: dYb, dHpre, dYb2, dQKV;
 *   Xout, cls_b, cls_y, cls_f, head_y, G0, G1, Drow, dcls_y, dcls_f, dhead_y, dhead_yb, dXb1, dXb2, dctx,
 *   c_ctx, c_xin, c_X1, c_Hpre, c_Hm, c_Y1, c_ctx32, c_dYb, c_dHpre, c_dYb2, c_dctx, c_dX1f, c_dY1;
 *   ldt (row stride of LSE / Mbits / Drow), Tp
 * = 3 + 14 * layers + 30 entries.  Returns that count, or -1 (convdr_last_error) when out_len is smaller. */
int convdr_encoder_train_debug_layout(const convdr_encoder_config* cfg, int64_t rows, int B, int64_t* out, int out_len);

/* ------------------------------------------------------------------------------------------
 * Collectives of the N > 1 paths for hosts that are not Python: thin wrappers over RCCL (xGMI).
 * The reference's own interface for these exchanges is torch.distributed (gen_passage_embeddings.py:314, DDP /
 * nn.DataParallel run_convdr_train.py:77-78, faiss IndexShards run_convdr_inference.py:355-368), which
 * convdr_amd/parallel.py keeps using; a torch-free host gets the same three steps here:
 *   query all-gather            convdr_comm_allgather(comm, Q_local, Q_all, nq_local * d * 4, stream)
 *   per-rank top-k all-gather   convdr_comm_allgather(comm, packed (score, offset) lists, all lists, nq * k * 12, stream)
 *                               followed by ONE convdr_topk_merge_packed call on the gathered buffer
 *   gradient all-reduce (sum)   convdr_comm_allreduce_f32(comm, arena slice, arena slice, count, stream) behind
 *                               convdr_backward_wait_layer; 1 / W rides on convdr_grad_norm_clip(pre_scale)
 * One communicator per process and device (one process per GPU).  librccl.so is looked up at the first call (the copy
 * the process has already loaded, e.g. torch's; else the system one): it is not a link-time dependency.
 * convdr_comm_unique_id fills CONVDR_COMM_ID_BYTES HOST bytes on one rank; the host distributes them out of band (file, MPI,
 * socket) and every rank calls convdr_comm_init with them.  send / recv are device pointers; in-place use
 * (recv + rank * bytes == send, or recv == send for the all-reduce) is allowed as in RCCL.
 * ------------------------------------------------------------------------------------------ */
#define CONVDR_COMM_ID_BYTES 128
typedef struct convdr_comm_opaque* convdr_comm_t;
int convdr_comm_unique_id(void* id_out_host);
int convdr_comm_init(convdr_comm_t* comm, int nranks, int rank, const void* unique_id_host);
int convdr_comm_ranks(convdr_comm_t comm, int* nranks, int* rank);
int convdr_comm_allgather(convdr_comm_t comm, const void* send, void* recv, size_t bytes_per_rank, convdr_stream_t stream);
int convdr_comm_allreduce_f32(convdr_comm_t comm, const float* send, float* recv, size_t count, convdr_stream_t stream);
int convdr_comm_destroy(convdr_comm_t comm);

#ifdef __cplusplus
}
#endif
#endif /* CONVDR_HIP_H */
