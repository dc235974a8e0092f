// Judging a run against the qrels (included by ip_topk.hip after ip_compact.hpp; contract in include/convdr_hip.h,
// "Judging a run").
//
//   k_run_label       labels[q, r] = the grade of key K[q, r] in query q's qrels segment (binary search on the 64-bit key),
//                     or one of the two sentinels: not judged / padding
//   k_run_measures    one workgroup per query: num_rel, num_rel_ret, recip_rank, map and ndcg_cut / recall / P at the cutoffs
//   k_run_negatives   one workgroup per query: the two-pass negative list of data/gen_ranking_data.py:539-567
//
// The qrels are a CSR: off int64 [nq + 1], and per query the judged keys (strictly ascending), their grades, and `ideal`, the
// positive grades sorted descending and zero filled -- the ideal DCG is a prefix sum of it and nothing is sorted here.  The
// kernels never trust `off`: a segment is clamped to [0, nnz] before anything is read through it.
//
// Both workgroup kernels walk a list in PIECES of RUN_THREADS consecutive ranks, one rank per thread, and carry the count of
// flagged entries from piece to piece: a wave ballot gives a lane its count inside the wave, 16 wave totals in LDS give the
// rest.  Sums of fp64 terms are made in a fixed order (a thread's own ranks ascending, the wave's butterfly, the 16 waves
// ascending), so a call repeats bit for bit.
#pragma once

namespace convdr {

constexpr int RUN_THREADS = 1024;           // = the piece: ranks walked per step of the two workgroup kernels
constexpr int RUN_WAVES = RUN_THREADS / 64;
constexpr int RUN_MAX_N = 65536;            // FlatIPIndex.DEEP_MAX_K
constexpr int RUN_MAX_CUTOFFS = 16;

struct RunCuts {
  int nc;
  int c[RUN_MAX_CUTOFFS];
};

// query q's segment [lo, hi) of the qrels arrays, whatever off holds
__device__ __forceinline__ void run_segment(const int64_t* __restrict__ off, int q, int64_t nnz, int64_t& lo, int64_t& hi) {
  lo = off[q];
  hi = off[q + 1];
  lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
  hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
}

// grid (nq, chunks), 256 threads: one entry per thread and step.  A negative key is padding.
__global__ void __launch_bounds__(256) k_run_label(const int64_t* __restrict__ K, int n, int64_t ld, const int64_t* __restrict__ off,
                                                   const int64_t* __restrict__ key, const int32_t* __restrict__ grade, int64_t nnz,
                                                   int32_t* __restrict__ labels) {
  const int q = blockIdx.x;
  int64_t lo, hi;
  run_segment(off, q, nnz, lo, hi);
  for (int r = blockIdx.y * 256 + threadIdx.x; r < n; r += gridDim.y * 256) {
    const int64_t k = K[(int64_t)q * ld + r];
    int32_t lab = CONVDR_LABEL_PAD;
    if (k >= 0) {
      int64_t a = lo, b = hi;             // the first position in [lo, hi) whose key is >= k
      while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (key[m] < k) a = m + 1; else b = m;
      }
      lab = (a < hi && key[a] == k) ? grade[a] : CONVDR_LABEL_UNJUDGED;
    }
    labels[(int64_t)q * n + r] = lab;
  }
}

// Exclusive count of the flagged threads before this one in the workgroup, and the workgroup's total.  Two barriers: every
// thread of the workgroup calls it, the same number of times.
__device__ __forceinline__ uint32_t run_block_scan(bool flag, uint32_t* sh_w, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) sh_w[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RUN_WAVES; ++w) {
    const uint32_t v = sh_w[w];
    base += w < wave ? v : 0u;
    tot += v;
  }
  __syncthreads();
  total = tot;
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Sum over the workgroup in a fixed order; every thread gets it.  Two barriers.
__device__ __forceinline__ double run_block_sum(double v, double* sh_d) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh_d[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < RUN_WAVES; ++w) s += sh_d[w];
  __syncthreads();
  return s;
}

// out[q] = num_rel, num_rel_ret, recip_rank, map, ndcg_cut x nc, recall x nc, P x nc.  The ranks are walked in nc + 1
// stretches that end at min(cutoff, n) and at n, so the DCG and the relevant count "up to the cutoff" are what the walk
// holds when a stretch ends; the ideal list is walked the same way up to min(last cutoff, its length).
__global__ void __launch_bounds__(RUN_THREADS) k_run_measures(const int32_t* __restrict__ labels, int n, const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ grade, const int32_t* __restrict__ ideal,
                                                              int64_t nnz, int rel_level, RunCuts cuts, double* __restrict__ out) {
  __shared__ uint32_t sh_w[RUN_WAVES];
  __shared__ double sh_d[RUN_WAVES];
  __shared__ double sh_dcg[RUN_MAX_CUTOFFS], sh_idcg[RUN_MAX_CUTOFFS];
  __shared__ uint32_t sh_cnt[RUN_MAX_CUTOFFS];
  __shared__ uint32_t sh_first;
  const int q = blockIdx.x, tid = threadIdx.x, nc = cuts.nc;
  const int32_t* L = labels + (int64_t)q * n;
  int64_t lo, hi;
  run_segment(off, q, nnz, lo, hi);
  if (tid == 0) sh_first = 0;

  // num_rel: the query's qrels entries at or above the relevance level
  uint32_t mine = 0;
  for (int64_t i = lo + tid; i < hi; i += RUN_THREADS) mine += grade[i] >= rel_level ? 1u : 0u;
  const double num_rel = run_block_sum((double)mine, sh_d);      // (integers below 2^53: exact in any order)

  // the ideal DCG at every cutoff
  {
    const int64_t len = hi - lo;
    double run = 0.0;
    int a = 0;
    for (int i = 0; i < nc; ++i) {
      const int b = (int64_t)cuts.c[i] < len ? cuts.c[i] : (int)len;     // (len < c <= INT_MAX there)
      double acc = 0.0;
      for (int r = a + tid; r < b; r += RUN_THREADS) {
        const int32_t g = ideal[lo + r];
        if (g > 0) acc += (double)g / log2((double)r + 2.0);
      }
      run += run_block_sum(acc, sh_d);
      if (tid == 0) sh_idcg[i] = run;
      a = b > a ? b : a;
    }
  }

  // the list
  uint32_t carry = 0;          // relevant entries in the pieces walked so far (uniform)
  double map_acc = 0.0, dcg_run = 0.0;
  int a = 0;
  for (int i = 0; i <= nc; ++i) {
    const int b = i < nc ? (cuts.c[i] < n ? cuts.c[i] : n) : n;
    double dcg = 0.0;
    for (int r0 = a; r0 < b; r0 += RUN_THREADS) {
      const int r = r0 + tid;
      const int32_t lab = r < b ? L[r] : CONVDR_LABEL_PAD;
      const bool rel = lab >= rel_level;                 // (rel_level >= 1: never a sentinel)
      uint32_t total;
      const uint32_t before = run_block_scan(rel, sh_w, total);
      if (rel) {
        const uint32_t cnt = carry + before + 1u;
        map_acc += (double)cnt / (double)(r + 1);
        if (cnt == 1u) sh_first = (uint32_t)(r + 1);     // (one writer)
      }
      if (lab > 0) dcg += (double)lab / log2((double)r + 2.0);
      carry += total;
    }
    if (i < nc) {
      dcg_run += run_block_sum(dcg, sh_d);
      if (tid == 0) { sh_dcg[i] = dcg_run; sh_cnt[i] = carry; }
    }
    a = b > a ? b : a;
  }
  const double map_sum = run_block_sum(map_acc, sh_d);   // (its barriers publish sh_first, sh_dcg, sh_idcg, sh_cnt)
  if (tid != 0) return;
  double* o = out + (int64_t)q * (4 + 3 * nc);
  o[0] = num_rel;
  o[1] = (double)carry;
  o[2] = sh_first ? 1.0 / (double)sh_first : 0.0;
  o[3] = num_rel > 0.0 ? map_sum / num_rel : 0.0;
  for (int i = 0; i < nc; ++i) {
    o[4 + i] = sh_idcg[i] > 0.0 ? sh_dcg[i] / sh_idcg[i] : 0.0;
    o[4 + nc + i] = num_rel > 0.0 ? (double)sh_cnt[i] / num_rel : 0.0;
    o[4 + 2 * nc + i] = (double)sh_cnt[i] / (double)cuts.c[i];
  }
}

// out_keys / out_rows [q, 0 .. W), W = max(n, fill_to): list A, then list B, then -1.
//   A  every entry with a judged grade <= 0, in list order;
//   B  the first max(0, fill_to - |A|) entries that are not positives (grade <= 0, or not judged), in list order -- members of
//      A among them once more, as the reference's second pass appends without looking at what the first pass found.
// A query without a qrels entry of grade > 0 gets nothing.  I (nullable) shares K's pitch.
__global__ void __launch_bounds__(RUN_THREADS) k_run_negatives(const int64_t* __restrict__ K, const int64_t* __restrict__ I, int n,
                                                               int64_t ld, const int32_t* __restrict__ labels,
                                                               const int64_t* __restrict__ off, const int32_t* __restrict__ grade,
                                                               int64_t nnz, int fill_to, int W, int64_t* __restrict__ out_keys,
                                                               int64_t* __restrict__ out_rows, int32_t* __restrict__ counts) {
  __shared__ uint32_t sh_w[RUN_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int32_t* L = labels + (int64_t)q * n;
  const int64_t* Kq = K + (int64_t)q * ld;
  const int64_t* Iq = I ? I + (int64_t)q * ld : nullptr;
  int64_t* ok = out_keys + (int64_t)q * W;
  int64_t* orow = out_rows ? out_rows + (int64_t)q * W : nullptr;
  int64_t lo, hi;
  run_segment(off, q, nnz, lo, hi);
  bool pos = false;
  for (int64_t i = lo + tid; i < hi; i += RUN_THREADS) pos |= grade[i] > 0;
  uint32_t total;
  run_block_scan(pos, sh_w, total);
  uint32_t na = 0, nb = 0;
  if (total) {             // (uniform)
    for (int r0 = 0; r0 < n; r0 += RUN_THREADS) {
      const int r = r0 + tid;
      const int32_t lab = r < n ? L[r] : CONVDR_LABEL_PAD;
      const bool f = lab > CONVDR_LABEL_UNJUDGED && lab <= 0;
      const uint32_t before = run_block_scan(f, sh_w, total);
      if (f) {
        ok[na + before] = Kq[r];
        if (orow) orow[na + before] = Iq[r];
      }
      na += total;
    }
    const uint32_t want = (uint32_t)fill_to > na ? (uint32_t)fill_to - na : 0u;
    for (int r0 = 0; r0 < n && nb < want; r0 += RUN_THREADS) {
      const int r = r0 + tid;
      const int32_t lab = r < n ? L[r] : CONVDR_LABEL_PAD;
      const bool f = lab != CONVDR_LABEL_PAD && lab <= 0;
      const uint32_t before = run_block_scan(f, sh_w, total);
      if (f && nb + before < want) {
        ok[na + nb + before] = Kq[r];
        if (orow) orow[na + nb + before] = Iq[r];
      }
      nb = nb + total < want ? nb + total : want;
    }
  }
  const int cnt = (int)(na + nb);          // <= W: na <= n, and na + nb <= fill_to where nb > 0
  for (int i = cnt + tid; i < W; i += RUN_THREADS) {
    ok[i] = -1;
    if (orow) orow[i] = -1;
  }
  if (tid == 0) counts[q] = cnt;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int run_check_sizes(const char* name, int n, int nq, int64_t nnz) {
  CONVDR_REQUIRE(n >= 0 && n <= RUN_MAX_N && nq >= 0 && nnz >= 0, "%s: bad sizes n=%d nq=%d nnz=%lld (0 <= n <= %d, nq >= 0, nnz >= 0)",
                 name, n, nq, (long long)nnz, RUN_MAX_N);
  return 0;
}

}  // namespace convdr

extern "C" int convdr_run_label(const int64_t* K, int n, int64_t ld, int nq, const int64_t* off, const int64_t* key,
                                const int32_t* grade, int64_t nnz, int32_t* labels, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_run_label";
  if (int e = run_check_sizes(name, n, nq, nnz)) return e;
  CONVDR_REQUIRE(ld >= n, "%s: pitch smaller than the row (ld=%lld n=%d)", name, (long long)ld, n);
  if (nq == 0 || n == 0) return 0;
  CONVDR_REQUIRE(K && off && labels && (nnz == 0 || (key && grade)), "%s: a NULL argument (K, off, labels; key, grade unless nnz = 0)",
                 name);
  const int chunks = (n + 255) / 256 < 64 ? (n + 255) / 256 : 64;
  hipLaunchKernelGGL(k_run_label, dim3(nq, chunks), dim3(256), 0, (hipStream_t)stream, K, n, ld, off, key, grade, nnz, labels);
  CONVDR_CHECK_LAUNCH("k_run_label");
  return 0;
}

extern "C" int convdr_run_measures(const int32_t* labels, int n, int nq, const int64_t* off, const int32_t* grade,
                                   const int32_t* ideal, int64_t nnz, int rel_level, const int32_t* cutoffs, int n_cutoffs,
                                   double* out, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_run_measures";
  if (int e = run_check_sizes(name, n, nq, nnz)) return e;
  CONVDR_REQUIRE(rel_level >= 1, "%s: rel_level must be >= 1 (got %d)", name, rel_level);
  CONVDR_REQUIRE(n_cutoffs >= 0 && n_cutoffs <= RUN_MAX_CUTOFFS, "%s: at most %d cutoffs (got %d)", name, RUN_MAX_CUTOFFS, n_cutoffs);
  CONVDR_REQUIRE(n_cutoffs == 0 || cutoffs, "%s: cutoffs is NULL (a HOST array of %d values)", name, n_cutoffs);
  RunCuts cuts = {};
  cuts.nc = n_cutoffs;
  for (int i = 0; i < n_cutoffs; ++i) {
    CONVDR_REQUIRE(cutoffs[i] >= 1 && (i == 0 || cutoffs[i] > cutoffs[i - 1]),
                   "%s: cutoffs must be >= 1 and strictly ascending (cutoffs[%d] = %d)", name, i, cutoffs[i]);
    cuts.c[i] = cutoffs[i];
  }
  if (nq == 0) return 0;
  CONVDR_REQUIRE(off && out && (n == 0 || labels) && (nnz == 0 || (grade && ideal)),
                 "%s: a NULL argument (off, out; labels unless n = 0; grade, ideal unless nnz = 0)", name);
  hipLaunchKernelGGL(k_run_measures, dim3(nq), dim3(RUN_THREADS), 0, (hipStream_t)stream, labels, n, off, grade, ideal, nnz, rel_level,
                     cuts, out);
  CONVDR_CHECK_LAUNCH("k_run_measures");
  return 0;
}

extern "C" int convdr_run_negatives(const int64_t* K, const int64_t* I, int n, int64_t ld, int nq, const int32_t* labels,
                                    const int64_t* off, const int32_t* grade, int64_t nnz, int fill_to, int64_t* out_keys,
                                    int64_t* out_rows, int32_t* counts, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_run_negatives";
  if (int e = run_check_sizes(name, n, nq, nnz)) return e;
  CONVDR_REQUIRE(fill_to >= 0 && fill_to <= RUN_MAX_N, "%s: fill_to=%d outside [0, %d]", name, fill_to, RUN_MAX_N);
  CONVDR_REQUIRE(ld >= n, "%s: pitch smaller than the row (ld=%lld n=%d)", name, (long long)ld, n);
  CONVDR_REQUIRE(out_rows || !I, "%s: I is given but out_rows is NULL", name);
  CONVDR_REQUIRE(!out_rows || I || n == 0 || nq == 0, "%s: out_rows is given but I is NULL", name);
  if (nq == 0) return 0;
  const int W = n > fill_to ? n : fill_to;
  CONVDR_REQUIRE(off && counts && (W == 0 || out_keys) && (n == 0 || (K && labels)) && (nnz == 0 || grade),
                 "%s: a NULL argument (off, counts; out_keys unless max(n, fill_to) = 0; K, labels unless n = 0; grade unless nnz = 0)",
                 name);
  hipLaunchKernelGGL(k_run_negatives, dim3(nq), dim3(RUN_THREADS), 0, (hipStream_t)stream, K, I, n, ld, labels, off, grade, nnz,
                     fill_to, W, out_keys, out_rows, counts);
  CONVDR_CHECK_LAUNCH("k_run_negatives");
  return 0;
}
