// Per-query exclusion lists (included by ip_topk.hip after ip_docs.hpp; contract in include/convdr_hip.h, "Per-query
// exclusions").  Nothing here scans: the exclusion is applied to CERTIFIED results ("Per-query exclusions").
//
//   k_excl_build<DOCS>      one workgroup per query: the query's entries -> LDS, bitonic sort, de-duplicate, the canonical row
//   k_excl_drop_topk        one workgroup per query: the first k entries of a canonical list whose row is not excluded
//   k_excl_ragged<PACK>     the same over a lims-indexed result: the kept count per query, or the pack into the new lims
//   k_ip_excl_count_ahead   one wave per (pair, slice of the list): the excluded, allowed rows that precede a threshold
//
// The canonical row of a query: its excluded rows ascending and distinct, then 0xffffffff.  Membership is a binary search in
// it (at most 15 steps: a row holds at most 16,384 entries).  Every loop is bounded by an argument, no workgroup waits for
// another, all stores are plain vector stores; the only atomics are integer adds / ors (the order of arrival does not show).
#pragma once

namespace convdr {

constexpr int EXCL_MAX_ENTRIES = 16384;            // entries per query, before de-duplication: 64 KB of LDS
constexpr uint32_t EXCL_PAD = 0xffffffffu;
constexpr int EXCL_ST_ROW = 1, EXCL_ST_LONG = 2;   // status bits of the builds: a row >= n; more than EXCL_MAX_ENTRIES entries
constexpr int EXCL_BUILD_THREADS = 1024, EXCL_THREADS = 256;
constexpr int EXCL_AUX_WORDS = 32;                 // behind the sort buffer: wave sums [16], cursor [16], flags [17]

// Stable ranks inside one workgroup pass: the number of kept entries of the threads below this one, and the pass's total.
// wsum: LDS [THREADS / 64].  The whole workgroup calls it; it ends behind a barrier, so the next pass may write wsum again.
template <int THREADS>
__device__ __forceinline__ uint32_t excl_block_rank(bool keep, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ballot = __ballot(keep);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const uint32_t c = wsum[w];
    before += w < wave ? c : 0u;
    all += c;
  }
  __syncthreads();
  *total = all;
  return before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

// entries of query q's canonical row, clamped to the pitch (a count the builds did not write cannot lead outside the row)
__device__ __forceinline__ int excl_count_of(const int32_t* __restrict__ ex_count, int q, int64_t ex_ld) {
  const int c = ex_count[q];
  return c < 0 ? 0 : ((int64_t)c > ex_ld ? (int)ex_ld : c);
}

__device__ __forceinline__ bool excl_member(const uint32_t* __restrict__ list, int cnt, uint32_t row) {
  int lo = 0, hi = cnt;
  for (int s = 0; s < 16 && lo < hi; ++s) {        // (cnt <= 16,384: 15 halvings empty the interval)
    const int mid = (lo + hi) >> 1;
    if (list[mid] < row) lo = mid + 1; else hi = mid;
  }
  return lo < cnt && list[lo] == row;
}

// One workgroup per query.  DOCS = false: src is the int64 list [nq, e] with pitch ld_in (negative: padding).  DOCS = true: src is
// the row list of a CSR (convdr_keys_rows_fill), the query owns the e segments (start, count)[q, 0 .. e) with pitch ld_in; a
// segment that does not lie inside src[0, rows_len) is skipped, as convdr_ip_score_docs skips it.  p2: the sort's length, a power
// of two >= the entries a query can hold (DOCS: EXCL_MAX_ENTRIES).  LDS: p2 + EXCL_AUX_WORDS words.
template <bool DOCS>
__global__ void __launch_bounds__(EXCL_BUILD_THREADS) k_excl_build(const int64_t* __restrict__ src, int64_t rows_len,
                                                                   const int64_t* __restrict__ start,
                                                                   const int32_t* __restrict__ count_in, int e, int64_t ld_in,
                                                                   int64_t n, int p2, uint32_t* __restrict__ rows_out,
                                                                   int64_t ld_out, int32_t* __restrict__ count,
                                                                   int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* sh = (uint32_t*)smem;
  uint32_t* aux = sh + p2;
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < p2; i += EXCL_BUILD_THREADS) sh[i] = EXCL_PAD;
  if (tid < EXCL_AUX_WORDS) aux[tid] = 0;
  __syncthreads();
  uint32_t flags = 0;
  if (!DOCS) {
    for (int i = tid; i < e; i += EXCL_BUILD_THREADS) {
      const int64_t v = src[(int64_t)q * ld_in + i];
      if (v >= n) flags |= EXCL_ST_ROW;
      else if (v >= 0) sh[i] = (uint32_t)v;
    }
  } else {
    for (int j = tid; j < e; j += EXCL_BUILD_THREADS) {
      const int64_t at = (int64_t)q * ld_in + j;
      const int64_t s0 = start[at], c = (int64_t)count_in[at];
      if (!(c > 0 && s0 >= 0 && s0 <= rows_len - c)) continue;
      // the segments may land in any order: the sort follows.  A clamped length keeps the cursor inside 32 bits
      const uint32_t cc = c > EXCL_MAX_ENTRIES ? (uint32_t)EXCL_MAX_ENTRIES + 1u : (uint32_t)c;
      const uint32_t base = atomicAdd(&aux[16], cc);
      if (base + cc > (uint32_t)EXCL_MAX_ENTRIES) { flags |= EXCL_ST_LONG; continue; }
      for (uint32_t i = 0; i < cc; ++i) {
        const int64_t v = src[s0 + i];
        if (v >= n) flags |= EXCL_ST_ROW;
        else if (v >= 0) sh[base + i] = (uint32_t)v;
      }
    }
  }
  if (flags) atomicOr(&aux[17], flags);
  __syncthreads();
  // bitonic network, ascending: the padding (the largest word) gathers at the end
  for (int kk = 2; kk <= p2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < p2; i += EXCL_BUILD_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const uint32_t a = sh[i], b = sh[o];
          if ((a > b) == ((i & kk) == 0)) { sh[i] = b; sh[o] = a; }
        }
      }
      __syncthreads();
    }
  }
  // the first of every run of equal rows is kept, in order
  uint32_t* out = rows_out + (int64_t)q * ld_out;
  uint32_t kept = 0;
  for (int c0 = 0; c0 < p2; c0 += EXCL_BUILD_THREADS) {
    const int i = c0 + tid;
    const uint32_t v = i < p2 ? sh[i] : EXCL_PAD;
    const bool keep = v != EXCL_PAD && (i == 0 || sh[i - 1] != v);
    uint32_t total;
    const uint32_t pos = kept + excl_block_rank<EXCL_BUILD_THREADS>(keep, aux, &total);
    if (keep && (int64_t)pos < ld_out) out[pos] = v;
    kept += total;
  }
  const int64_t filled = (int64_t)kept < ld_out ? (int64_t)kept : ld_out;
  for (int64_t i = filled + tid; i < ld_out; i += EXCL_BUILD_THREADS) out[i] = EXCL_PAD;
  if (tid == 0) {
    count[q] = (int32_t)filled;
    if (aux[17]) atomicOr(status, (int32_t)aux[17]);
  }
}

// One workgroup per query over a canonical list (D, I)[q, 0 .. m), pitch ld, padding I = -1 at the tail: the first k entries whose
// row is not in the query's canonical row, in order, then (-3.4028235e38, -1); kept[q] = the survivors before the cut.
__global__ void __launch_bounds__(EXCL_THREADS) k_excl_drop_topk(const float* __restrict__ D, const int64_t* __restrict__ I, int m,
                                                                 int64_t ld, const uint32_t* __restrict__ ex_rows, int64_t ex_ld,
                                                                 const int32_t* __restrict__ ex_count, int k,
                                                                 float* __restrict__ D_out, int64_t* __restrict__ I_out,
                                                                 int32_t* __restrict__ kept) {
  __shared__ uint32_t wsum[EXCL_THREADS / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const uint32_t* list = ex_rows + (int64_t)q * ex_ld;
  const int cnt = excl_count_of(ex_count, q, ex_ld);
  const float* d_in = D + (int64_t)q * ld;
  const int64_t* i_in = I + (int64_t)q * ld;
  float* d_out = D_out + (int64_t)q * k;
  int64_t* i_out = I_out + (int64_t)q * k;
  uint32_t base = 0;
  for (int c0 = 0; c0 < m; c0 += EXCL_THREADS) {
    const int i = c0 + tid;
    const int64_t row = i < m ? i_in[i] : -1;
    const bool keep = row >= 0 && !excl_member(list, cnt, (uint32_t)row);
    uint32_t total;
    const uint32_t pos = base + excl_block_rank<EXCL_THREADS>(keep, wsum, &total);
    if (keep && pos < (uint32_t)k) { d_out[pos] = d_in[i]; i_out[pos] = row; }
    base += total;
  }
  for (int64_t i = (int64_t)(base < (uint32_t)k ? base : (uint32_t)k) + tid; i < k; i += EXCL_THREADS) {
    d_out[i] = -FLT_MAX;
    i_out[i] = -1;
  }
  if (tid == 0) kept[q] = (int32_t)base;
}

// One workgroup per query over its run [lims[q], lims[q + 1]) of a ragged result (clamped to [0, total]).  PACK = false:
// kept[q] = the entries whose row is not excluded.  PACK = true: those entries, in order, to [lims_out[q], lims_out[q + 1]) of
// (D_out, I_out) -- never past that run's end nor past total_out.
template <bool PACK>
__global__ void __launch_bounds__(EXCL_THREADS) k_excl_ragged(const int64_t* __restrict__ lims, const float* __restrict__ D,
                                                              const int64_t* __restrict__ I, int64_t total,
                                                              const uint32_t* __restrict__ ex_rows, int64_t ex_ld,
                                                              const int32_t* __restrict__ ex_count, int64_t* __restrict__ kept,
                                                              const int64_t* __restrict__ lims_out, float* __restrict__ D_out,
                                                              int64_t* __restrict__ I_out, int64_t total_out) {
  __shared__ uint32_t wsum[EXCL_THREADS / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const uint32_t* list = ex_rows + (int64_t)q * ex_ld;
  const int cnt = excl_count_of(ex_count, q, ex_ld);
  int64_t a = lims[q], b = lims[q + 1];
  a = a < 0 ? 0 : (a > total ? total : a);
  b = b < a ? a : (b > total ? total : b);
  int64_t oa = 0, ob = 0;
  if (PACK) {
    oa = lims_out[q];
    ob = lims_out[q + 1];
    oa = oa < 0 ? 0 : (oa > total_out ? total_out : oa);
    ob = ob < oa ? oa : (ob > total_out ? total_out : ob);
  }
  int64_t base = 0;
  for (int64_t c0 = a; c0 < b; c0 += EXCL_THREADS) {
    const int64_t i = c0 + tid;
    const int64_t row = i < b ? I[i] : -1;
    const bool keep = row >= 0 && !excl_member(list, cnt, (uint32_t)row);
    uint32_t chunk;
    const int64_t pos = base + excl_block_rank<EXCL_THREADS>(keep, wsum, &chunk);
    if (PACK && keep && oa + pos < ob) { D_out[oa + pos] = D[i]; I_out[oa + pos] = row; }
    base += chunk;
  }
  if (!PACK && tid == 0) kept[q] = base;
}

// One wave per (pair, slice of the list); grid (np, slices).  Pair p = (query pairq[p], threshold (x_thr[p], row_thr[p])):
// ahead[p] += #{x in the query's canonical row : x < n, x allowed, X_x > x_thr or (X_x == x_thr and x < row_thr)}, X_x the value
// k_ip_score_rows gives (ip_row_score).  ahead is zeroed on the stream before the launch; a pair whose query is outside
// [0, nq) adds nothing.
template <class PT>
__global__ void __launch_bounds__(EXCL_THREADS) k_ip_excl_count_ahead(const float* __restrict__ Q, int nq, const PT* __restrict__ P,
                                                                      int64_t n, int d, double unscale,
                                                                      const uint32_t* __restrict__ row_bits,
                                                                      const uint32_t* __restrict__ ex_rows, int64_t ex_ld,
                                                                      const int32_t* __restrict__ ex_count,
                                                                      const int32_t* __restrict__ pairq,
                                                                      const double* __restrict__ x_thr,
                                                                      const int64_t* __restrict__ row_thr,
                                                                      int64_t* __restrict__ ahead) {
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = pairq[p];
  if (q < 0 || q >= nq) return;                     // (uniform)
  const uint32_t* list = ex_rows + (int64_t)q * ex_ld;
  const int cnt = excl_count_of(ex_count, q, ex_ld);
  const float* qv = Q + (int64_t)q * d;
  const double xt = x_thr[p];
  const int64_t rt = row_thr[p];
  uint32_t mine = 0;
  for (int j = blockIdx.y * 4 + wave; j < cnt; j += gridDim.y * 4) {
    const uint32_t x = list[j];                     // (wave-uniform, as everything below)
    if ((int64_t)x >= n) continue;
    if (row_bits && !((row_bits[x >> 5] >> (x & 31u)) & 1u)) continue;
    const double s = ip_row_score<PT>(qv, P + (int64_t)x * d, d, lane, unscale);
    mine += (s > xt || (s == xt && (int64_t)x < rt)) ? 1u : 0u;
  }
  if (lane == 0 && mine) atomicAdd((unsigned long long*)(ahead + p), (unsigned long long)mine);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// the canonical rows an entry reads: [nq, ex_ld] words and [nq] counts
static int excl_check_operand(const char* name, const uint32_t* ex_rows, int64_t ex_ld, const int32_t* ex_count) {
  CONVDR_REQUIRE(ex_ld >= 4 && ex_ld <= EXCL_MAX_ENTRIES && ex_ld % 4 == 0,
                 "%s: ex_ld=%lld must be a multiple of 4 in [4, %d] (at most %d entries per query)", name, (long long)ex_ld,
                 EXCL_MAX_ENTRIES, EXCL_MAX_ENTRIES);
  CONVDR_REQUIRE(ex_rows && ex_count, "%s: a NULL argument (ex_rows, ex_count)", name);
  return 0;
}

static int excl_build_launch(bool docs, const int64_t* src, int64_t rows_len, const int64_t* start, const int32_t* count_in, int nq,
                             int e, int64_t ld_in, int64_t n, uint32_t* ex_rows, int64_t ex_ld, int32_t* ex_count, int32_t* status,
                             hipStream_t st) {
  CONVDR_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (nq == 0) return 0;
  int p2 = 64;
  while (p2 < (docs ? EXCL_MAX_ENTRIES : e)) p2 <<= 1;
  const size_t lds = ((size_t)p2 + EXCL_AUX_WORDS) * 4;
  static DeviceOnce attr_done;
  if (attr_done.first()) {
    const int most = (EXCL_MAX_ENTRIES + EXCL_AUX_WORDS) * 4;
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_excl_build<false>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_excl_build<true>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
  }
  ProfScope prof("excl_build", st);
  if (docs)
    hipLaunchKernelGGL(k_excl_build<true>, dim3(nq), dim3(EXCL_BUILD_THREADS), lds, st, src, rows_len, start, count_in, e, ld_in, n, p2,
                       ex_rows, ex_ld, ex_count, status);
  else
    hipLaunchKernelGGL(k_excl_build<false>, dim3(nq), dim3(EXCL_BUILD_THREADS), lds, st, src, rows_len, start, count_in, e, ld_in, n,
                       p2, ex_rows, ex_ld, ex_count, status);
  CONVDR_CHECK_LAUNCH("k_excl_build");
  return 0;
}

}  // namespace convdr

extern "C" int convdr_excl_build_rows(const int64_t* rows, int nq, int e, int64_t ld, int64_t n, uint32_t* ex_rows, int64_t ex_ld,
                                      int32_t* ex_count, int32_t* status, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_excl_build_rows";
  CONVDR_REQUIRE(nq >= 0 && e >= 0 && ld >= e, "%s: bad sizes nq=%d e=%d ld=%lld (ld >= e)", name, nq, e, (long long)ld);
  CONVDR_REQUIRE(e <= EXCL_MAX_ENTRIES, "%s: e=%d entries per query, at most %d", name, e, EXCL_MAX_ENTRIES);
  if (int err = compact_check_n(name, n)) return err;
  CONVDR_REQUIRE(status != nullptr, "%s: status is NULL", name);
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE(ex_ld >= e, "%s: ex_ld=%lld cannot hold e=%d entries", name, (long long)ex_ld, e);
  CONVDR_REQUIRE(rows || e == 0 || nq == 0, "%s: rows is NULL", name);
  return excl_build_launch(false, rows, 0, nullptr, nullptr, nq, e, ld, n, ex_rows, ex_ld, ex_count, status, (hipStream_t)stream);
}

extern "C" int convdr_excl_build_docs(const int64_t* csr_rows, int64_t rows_len, const int64_t* start, const int32_t* count, int nq,
                                      int m, int64_t ld, int64_t n, uint32_t* ex_rows, int64_t ex_ld, int32_t* ex_count,
                                      int32_t* status, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_excl_build_docs";
  CONVDR_REQUIRE(nq >= 0 && m >= 0 && ld >= m, "%s: bad sizes nq=%d m=%d ld=%lld (ld >= m)", name, nq, m, (long long)ld);
  CONVDR_REQUIRE(m <= EXCL_MAX_ENTRIES, "%s: m=%d documents per query, at most %d entries", name, m, EXCL_MAX_ENTRIES);
  CONVDR_REQUIRE(rows_len >= 0 && rows_len < ((int64_t)1 << 31), "%s: bad list length rows_len=%lld (0 <= rows_len < 2^31)", name,
                 (long long)rows_len);
  if (int err = compact_check_n(name, n)) return err;
  CONVDR_REQUIRE(status != nullptr, "%s: status is NULL", name);
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE((start && count) || m == 0 || nq == 0, "%s: a NULL argument (start, count)", name);
  CONVDR_REQUIRE(csr_rows || rows_len == 0, "%s: csr_rows is NULL", name);
  return excl_build_launch(true, csr_rows, rows_len, start, count, nq, m, ld, n, ex_rows, ex_ld, ex_count, status,
                           (hipStream_t)stream);
}

extern "C" int convdr_excl_drop_topk(const float* D, const int64_t* I, int nq, int m, int64_t ld, const uint32_t* ex_rows,
                                     int64_t ex_ld, const int32_t* ex_count, int k, float* D_out, int64_t* I_out, int32_t* kept,
                                     convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_excl_drop_topk";
  CONVDR_REQUIRE(nq >= 0 && m >= 1 && m <= (1 << 30) && ld >= m, "%s: bad sizes nq=%d m=%d ld=%lld (1 <= m <= 2^30, ld >= m)", name,
                 nq, m, (long long)ld);
  CONVDR_REQUIRE(k >= 1 && k <= (1 << 30), "%s: bad sizes k=%d (1 <= k <= 2^30)", name, k);
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE(D && I && D_out && I_out && kept, "%s: a NULL argument (D, I, D_out, I_out, kept)", name);
  if (nq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("excl_drop_topk", st);
  hipLaunchKernelGGL(k_excl_drop_topk, dim3(nq), dim3(EXCL_THREADS), 0, st, D, I, m, ld, ex_rows, ex_ld, ex_count, k, D_out, I_out, kept);
  CONVDR_CHECK_LAUNCH("k_excl_drop_topk");
  return 0;
}

extern "C" int convdr_excl_count_ragged(const int64_t* lims, const int64_t* I, int64_t total, int nq, const uint32_t* ex_rows,
                                        int64_t ex_ld, const int32_t* ex_count, int64_t* kept, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_excl_count_ragged";
  CONVDR_REQUIRE(nq >= 0 && total >= 0, "%s: bad sizes nq=%d total=%lld", name, nq, (long long)total);
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE(lims && kept && (I || total == 0), "%s: a NULL argument (lims, kept, I)", name);
  if (nq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("excl_count_ragged", st);
  hipLaunchKernelGGL(k_excl_ragged<false>, dim3(nq), dim3(EXCL_THREADS), 0, st, lims, (const float*)nullptr, I, total, ex_rows, ex_ld,
                     ex_count, kept, (const int64_t*)nullptr, (float*)nullptr, (int64_t*)nullptr, (int64_t)0);
  CONVDR_CHECK_LAUNCH("k_excl_ragged<count>");
  return 0;
}

extern "C" int convdr_excl_pack_ragged(const int64_t* lims, const float* D, const int64_t* I, int64_t total, int nq,
                                       const uint32_t* ex_rows, int64_t ex_ld, const int32_t* ex_count, const int64_t* lims_out,
                                       float* D_out, int64_t* I_out, int64_t total_out, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_excl_pack_ragged";
  CONVDR_REQUIRE(nq >= 0 && total >= 0 && total_out >= 0 && total_out <= total, "%s: bad sizes nq=%d total=%lld total_out=%lld "
                 "(0 <= total_out <= total)", name, nq, (long long)total, (long long)total_out);
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE(lims && lims_out && ((D && I) || total == 0) && ((D_out && I_out) || total_out == 0),
                 "%s: a NULL argument (lims, lims_out, D, I, D_out, I_out)", name);
  if (nq == 0 || total_out == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("excl_pack_ragged", st);
  hipLaunchKernelGGL(k_excl_ragged<true>, dim3(nq), dim3(EXCL_THREADS), 0, st, lims, D, I, total, ex_rows, ex_ld, ex_count,
                     (int64_t*)nullptr, lims_out, D_out, I_out, total_out);
  CONVDR_CHECK_LAUNCH("k_excl_ragged<pack>");
  return 0;
}

extern "C" int convdr_ip_excl_count_ahead(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half,
                                          float p_scale, int64_t n, int d, const uint32_t* row_bits, int64_t row_bits_words,
                                          const uint32_t* ex_rows, int64_t ex_ld, const int32_t* ex_count, int np,
                                          const int32_t* pairq, const double* x_thr, const int64_t* row_thr, int64_t* ahead,
                                          convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_excl_count_ahead";
  CONVDR_REQUIRE(store >= 0 && store <= 2, "%s: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) (got %d)", name, store);
  CONVDR_REQUIRE(nq >= 0 && np >= 0, "%s: bad sizes nq=%d np=%d", name, nq, np);
  if (int err = compact_check_n(name, n)) return err;
  CONVDR_REQUIRE(d > 0 && d % 64 == 0 && d <= 4096, "%s: need d %% 64 == 0 and d <= 4096 (got %d)", name, d);
  CONVDR_REQUIRE(row_bits != nullptr || row_bits_words == 0, "%s: row_bits is NULL but row_bits_words=%lld", name,
                 (long long)row_bits_words);
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, nullptr, row_bits, row_bits_words, 0};
  if (int err = ip_check_block(name, b)) return err;
  if (int err = excl_check_operand(name, ex_rows, ex_ld, ex_count)) return err;
  CONVDR_REQUIRE(ahead != nullptr || np == 0, "%s: ahead is NULL", name);
  if (np == 0) return 0;
  CONVDR_REQUIRE(q_f32 && pairq && x_thr && row_thr, "%s: a NULL argument (q_f32, pairq, x_thr, row_thr)", name);
  CONVDR_REQUIRE(n == 0 || (b.rows_f16() ? p_half != nullptr : p_f32 != nullptr),
                 "%s: a NULL block pointer (p_f32; p_half for store = 2)", name);
  hipStream_t st = (hipStream_t)stream;
  CONVDR_CHECK_HIP(hipMemsetAsync(ahead, 0, (size_t)np * sizeof(int64_t), st));
  if (n == 0 || nq == 0) return 0;                  // (no row can be ahead / no query a pair could name)
  const int slices = ex_ld < 64 ? 1 : (ex_ld / 64 < 64 ? (int)(ex_ld / 64) : 64);
  ProfScope prof("ip_excl_count_ahead", st);
  if (b.rows_f16())
    hipLaunchKernelGGL(k_ip_excl_count_ahead<_Float16>, dim3(np, slices), dim3(EXCL_THREADS), 0, st, q_f32, nq, (const _Float16*)p_half,
                       n, d, b.unscale(), row_bits, ex_rows, ex_ld, ex_count, pairq, x_thr, row_thr, ahead);
  else
    hipLaunchKernelGGL(k_ip_excl_count_ahead<float>, dim3(np, slices), dim3(EXCL_THREADS), 0, st, q_f32, nq, p_f32, n, d, b.unscale(),
                       row_bits, ex_rows, ex_ld, ex_count, pairq, x_thr, row_thr, ahead);
  CONVDR_CHECK_LAUNCH("k_ip_excl_count_ahead");
  return 0;
}
