// Merging and de-duplicating ranked lists of up to 4,096 entries in LDS (included by ip_topk.hip after the search headers):
// the two-way merge, the W-way merge, the first occurrence per key, each with its entry (convdr_topk_merge,
// convdr_topk_merge_multi, convdr_topk_merge_packed, convdr_topk_distinct).  Longer lists: topk_deep.hpp.
#pragma once

// ---- two-way merge of sorted per-query lists (run_convdr_inference.py:213-229) -------------------------------------
// One workgroup per query.  Every element computes its own output slot: its index in its list + the number of
// elements of the other list that precede it (binary search on the descending scores held in LDS) -- A before B on
// ties, so for a in A the B elements strictly greater count, for b in B the A elements greater or equal.
namespace convdr {
__global__ void __launch_bounds__(256) k_topk_merge(const float* __restrict__ Da, const int64_t* __restrict__ Ia, int na,
                                                    int64_t lda, const float* __restrict__ Db,
                                                    const int64_t* __restrict__ Ib, int nb, int64_t ldb, int n_out,
                                                    float* __restrict__ Dout, int64_t* __restrict__ Iout, int64_t ldo) {
  extern __shared__ float sm[];
  float* sa = sm;
  float* sb = sm + na;
  const int q = blockIdx.x;
  Da += q * lda; Ia += q * lda; Db += q * ldb; Ib += q * ldb; Dout += q * ldo; Iout += q * ldo;
  for (int i = threadIdx.x; i < na; i += 256) sa[i] = Da[i];
  for (int i = threadIdx.x; i < nb; i += 256) sb[i] = Db[i];
  __syncthreads();
  for (int i = threadIdx.x; i < na + nb; i += 256) {
    const bool from_a = i < na;
    const int j = from_a ? i : i - na;
    const float v = from_a ? sa[j] : sb[j];
    const float* other = from_a ? sb : sa;
    int lo = 0, hi = from_a ? nb : na;       // first index of `other` that does NOT precede v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const bool precedes = from_a ? (other[mid] > v) : (other[mid] >= v);
      if (precedes) lo = mid + 1; else hi = mid;
    }
    const int pos = j + lo;
    if (pos < n_out) {
      Dout[pos] = v;
      Iout[pos] = from_a ? Ia[j] : Ib[j];
    }
  }
}
}  // namespace convdr

extern "C" int convdr_topk_merge(const float* Da, const int64_t* Ia, int na, int64_t lda, const float* Db, const int64_t* Ib,
                                 int nb, int64_t ldb, int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo,
                                 convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(na >= 0 && nb >= 0 && na <= 4096 && nb <= 4096 && n_out >= 0 && n_out <= na + nb && nq >= 0,
                 "convdr_topk_merge: bad sizes na=%d nb=%d n_out=%d nq=%d", na, nb, n_out, nq);
  if (nq == 0 || n_out == 0) return 0;
  hipLaunchKernelGGL(k_topk_merge, dim3(nq), dim3(256), (size_t)(na + nb) * 4, (hipStream_t)stream, Da, Ia, na, lda, Db, Ib,
                     nb, ldb, n_out, Dout, Iout, ldo);
  CONVDR_CHECK_LAUNCH("k_topk_merge");
  return 0;
}

// ---- W-way merge of sorted per-query lists in one launch (the exchange step of the sharded search) ------------------
// k_topk_merge taken from 2 lists to W.  One workgroup per query; the first m = min(n, n_out) scores of every list are
// staged in LDS list after list (an entry past position n_out of its own list can never be output, and a count cut at
// m >= n_out still pushes its element past the output).  Element j of list w goes to slot
//   j + sum_{u < w} #{x in list u : x >= v} + sum_{u > w} #{x in list u : x > v}         (earlier lists win ties)
// -- the stable descending sort of [list 0, ..., list W-1], i.e. the reference's `>=` merge chained over blocks 0..W-1 --
// each count a binary search; the walk over u stops as soon as the slot has left the output, and elements below a
// score that n_out others certainly reach are not searched for at all.  The lanes' searches diverge, so LDS bank
// conflicts are the rule here (at most W * m * (W - 1) * log2 m dword reads per query: 39 k at 8 x 100).
namespace convdr {
struct MergeListsPlain {     // D / I + w * list_stride + q * ld
  const float* D;
  const int64_t* I;
  int64_t list_stride, ld;
  __device__ float score(int w, int q, int j) const { return D[w * list_stride + q * ld + j]; }
  __device__ int64_t id(int w, int q, int j) const { return I[w * list_stride + q * ld + j]; }
};
struct MergeListsPacked {    // [nlists][nq][n] records of 3 dwords: score bits, offset low word, offset high word
  const uint32_t* rec;
  int64_t nq, n;
  __device__ const uint32_t* at(int w, int q, int j) const { return rec + ((w * nq + q) * n + j) * 3; }
  __device__ float score(int w, int q, int j) const { return __uint_as_float(at(w, q, j)[0]); }
  __device__ int64_t id(int w, int q, int j) const {
    const uint32_t* r = at(w, q, j);
    return (int64_t)(((uint64_t)r[2] << 32) | (uint64_t)r[1]);
  }
};

template <class Lists, int THREADS>
__global__ void __launch_bounds__(THREADS) k_topk_merge_multi(Lists in, int nlists, int m, int n_out,
                                                              float* __restrict__ Dout, int64_t* __restrict__ Iout,
                                                              int64_t ldo) {
  extern __shared__ float sm[];
  const int q = blockIdx.x;
  const int total = nlists * m;
  Dout += q * ldo; Iout += q * ldo;
  for (int e = threadIdx.x; e < total; e += THREADS) {
    const int w = e / m;
    sm[e] = in.score(w, q, e - w * m);
  }
  __syncthreads();
  // Entry p = ceil(n_out / W) - 1 exists in every list (n_out <= W * n), and at least W * (p + 1) >= n_out entries are
  // >= the smallest of those W scores: anything strictly below it cannot be output, whatever the tie rule.  With W
  // like lists that leaves about n_out of the W * m elements to search for (all of them when one list is padding only).
  const int p = (n_out + nlists - 1) / nlists - 1;
  float floor_v = sm[p];
  for (int u = 1; u < nlists; ++u) floor_v = fminf(floor_v, sm[u * m + p]);
  for (int e = threadIdx.x; e < total; e += THREADS) {
    const float v = sm[e];
    if (v < floor_v) continue;
    const int w = e / m, j = e - w * m;
    int pos = j;
    for (int u = 0; u < nlists && pos < n_out; ++u) {
      if (u == w) continue;
      const float* other = sm + u * m;
      const bool earlier = u < w;
      // first index of list u that does NOT precede v, looked for among the first `hi` entries only: a count of
      // n_out - pos already puts the element past the output.  The last of them is probed first: an element that is
      // out leaves after ONE read instead of a whole search (8 x 4096 lists, 100 queries: 133 -> 110 us).
      int lo = 0, hi = m < n_out - pos ? m : n_out - pos;
      const float last = other[hi - 1];
      if (earlier ? (last >= v) : (last > v)) {
        lo = hi;
      } else {
        --hi;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const bool precedes = earlier ? (other[mid] >= v) : (other[mid] > v);
          if (precedes) lo = mid + 1; else hi = mid;
        }
      }
      pos += lo;
    }
    if (pos < n_out) {
      Dout[pos] = v;
      Iout[pos] = in.id(w, q, j);
    }
  }
}

constexpr int64_t TOPK_MERGE_MULTI_MAX = 32768;      // staged scores: 128 KB of the CU's 160 KB LDS

template <class Lists, int THREADS>
static int launch_topk_merge_multi(const Lists& in, int nlists, int m, int nq, int n_out, float* Dout, int64_t* Iout,
                                   int64_t ldo, hipStream_t st) {
  static DeviceOnce attr_done;
  if (attr_done.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_topk_merge_multi<Lists, THREADS>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)(TOPK_MERGE_MULTI_MAX * 4)));
  hipLaunchKernelGGL((k_topk_merge_multi<Lists, THREADS>), dim3(nq), dim3(THREADS), (size_t)nlists * m * 4, st, in, nlists, m,
                     n_out, Dout, Iout, ldo);
  CONVDR_CHECK_LAUNCH("k_topk_merge_multi");
  return 0;
}

// 256 threads up to 4096 staged elements (k = 100 at W = 8: 800, three or four per thread); 1024 beyond (32 k elements)
template <class Lists>
static int topk_merge_multi(const Lists& in, int nlists, int n, int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo,
                            hipStream_t st) {
  const int m = n < n_out ? n : n_out;
  if ((int64_t)nlists * m <= 4096) return launch_topk_merge_multi<Lists, 256>(in, nlists, m, nq, n_out, Dout, Iout, ldo, st);
  return launch_topk_merge_multi<Lists, 1024>(in, nlists, m, nq, n_out, Dout, Iout, ldo, st);
}

static bool topk_merge_multi_sizes_ok(int nlists, int n, int nq, int n_out) {
  return nlists >= 1 && n >= 0 && n <= 4096 && nq >= 0 && n_out >= 0 && (int64_t)n_out <= (int64_t)nlists * n &&
         (int64_t)nlists * (n < n_out ? n : n_out) <= TOPK_MERGE_MULTI_MAX;
}
}  // namespace convdr

extern "C" int convdr_topk_merge_multi(const float* D, const int64_t* I, int nlists, int n, int64_t list_stride, int64_t ld,
                                       int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(topk_merge_multi_sizes_ok(nlists, n, nq, n_out),
                 "convdr_topk_merge_multi: bad sizes nlists=%d n=%d n_out=%d nq=%d (n <= 4096, nlists * min(n, n_out) <= %d, "
                 "n_out <= nlists * n)", nlists, n, n_out, nq, (int)TOPK_MERGE_MULTI_MAX);
  CONVDR_REQUIRE(ld >= n && ldo >= n_out && (nlists == 1 || nq == 0 || list_stride >= n),
                 "convdr_topk_merge_multi: pitch smaller than the row (ld=%lld list_stride=%lld n=%d, ldo=%lld n_out=%d)",
                 (long long)ld, (long long)list_stride, n, (long long)ldo, n_out);
  if (nq == 0 || n_out == 0) return 0;
  return topk_merge_multi(MergeListsPlain{D, I, list_stride, ld}, nlists, n, nq, n_out, Dout, Iout, ldo, (hipStream_t)stream);
}

extern "C" int convdr_topk_merge_packed(const void* lists, int nlists, int n, int nq, int n_out, float* Dout, int64_t* Iout,
                                        int64_t ldo, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(topk_merge_multi_sizes_ok(nlists, n, nq, n_out),
                 "convdr_topk_merge_packed: bad sizes nlists=%d n=%d n_out=%d nq=%d (n <= 4096, nlists * min(n, n_out) <= %d, "
                 "n_out <= nlists * n)", nlists, n, n_out, nq, (int)TOPK_MERGE_MULTI_MAX);
  CONVDR_REQUIRE(ldo >= n_out, "convdr_topk_merge_packed: pitch smaller than the row (ldo=%lld n_out=%d)", (long long)ldo, n_out);
  if (nq == 0 || n_out == 0) return 0;
  return topk_merge_multi(MergeListsPacked{(const uint32_t*)lists, (int64_t)nq, (int64_t)n}, nlists, n, nq, n_out, Dout, Iout,
                          ldo, (hipStream_t)stream);
}

// ---- first occurrence per key of a ranked list: the document-level cut of a row-level result -----------------------
// The reference's `seen_pid` walk (run_convdr_inference.py:58-69) for all queries at once, one workgroup per query.
//   stage    keys (key_map[I] or I) of the n entries into LDS; entries with I < 0 or I >= key_map_len are dropped
//   claim    an open-addressing table of 2n..4n slots holds, per distinct key, the SMALLEST position that carries it:
//            an element takes an empty slot with a compare-and-swap of its own position, or -- when the slot's holder
//            has its key -- lowers the slot with atomicMin, or moves on to the next slot.  Which slot a key ends up in
//            depends on the arrival order; the minimum it holds does not.
//   compact  an element is kept iff its key's slot names it.  Positions are walked in chunks of THREADS, in order:
//            ballot + popcount inside a wave, the waves' totals through LDS, a running base across chunks.
// Nothing is ordered by an atomic's arrival: two runs write the same bytes.
namespace convdr {
constexpr uint32_t DISTINCT_EMPTY = 0xffffffffu;
constexpr uint32_t DISTINCT_PAD_SCORE_BITS = 0xff7fffffu;   // -3.4028235e38, the score FAISS pads with

__device__ __forceinline__ uint32_t distinct_hash(int64_t key) {   // murmur3's 64-bit finaliser
  uint64_t x = (uint64_t)key;
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return (uint32_t)x;
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_topk_distinct(const float* __restrict__ D, const int64_t* __restrict__ I, int n,
                                                           int64_t ld, const int64_t* __restrict__ key_map, int64_t key_map_len,
                                                           int n_out, float* __restrict__ Dout, int64_t* __restrict__ Iout,
                                                           int64_t* __restrict__ Kout, int64_t ldo, int32_t* __restrict__ counts,
                                                           int hbits) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WAVES = THREADS / 64;
  __shared__ uint32_t wave_tot[WAVES];
  __shared__ uint32_t sh_valid, sh_oob;
  int64_t* key = (int64_t*)smem;                              // [n]
  uint32_t* table = (uint32_t*)(smem + (size_t)n * 8);        // [1 << hbits]
  const uint32_t hmask = (1u << hbits) - 1u;
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  D += q * ld; I += q * ld; Dout += q * ldo; Iout += q * ldo;
  if (Kout) Kout += q * ldo;
  auto valid_id = [&](int64_t id) { return id >= 0 && (key_map == nullptr || id < key_map_len); };

  for (uint32_t h = threadIdx.x; h <= hmask; h += THREADS) table[h] = DISTINCT_EMPTY;
  if (threadIdx.x == 0) { sh_valid = 0; sh_oob = 0; }
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const int64_t id = I[i];
    key[i] = valid_id(id) ? (key_map ? key_map[id] : id) : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const int64_t id = I[i];
    if (!valid_id(id)) continue;
    const int64_t k = key[i];
    uint32_t h = distinct_hash(k) & hmask;
    for (uint32_t step = 0; step <= hmask; ++step, h = (h + 1u) & hmask) {   // ends early: the table has more slots than keys
      const uint32_t o = atomicCAS(&table[h], DISTINCT_EMPTY, (uint32_t)i);
      if (o == DISTINCT_EMPTY) break;
      if (key[o] == k) { atomicMin(&table[h], (uint32_t)i); break; }
    }
  }
  __syncthreads();
  uint32_t base = 0;                                          // kept entries before this chunk (the same in every thread)
  uint32_t wave_valid = 0;                                    // non-dropped entries of this wave's lanes
  bool oob = false;
  for (int i0 = 0; i0 < n; i0 += THREADS) {
    const int i = i0 + threadIdx.x;
    bool kept = false, valid = false;
    int64_t id = -1, k = 0;
    if (i < n) {
      id = I[i];
      valid = valid_id(id);
      oob = oob || (id >= 0 && !valid);
      if (valid) {
        k = key[i];
        uint32_t h = distinct_hash(k) & hmask, o = DISTINCT_EMPTY;
        for (uint32_t step = 0; step <= hmask; ++step, h = (h + 1u) & hmask) {   // the key is in the table, no empty slot before it
          o = table[h];
          if (o == DISTINCT_EMPTY || key[o] == k) break;
        }
        kept = o == (uint32_t)i;
      }
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(kept);
    wave_valid += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid));
    if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t t = wave_tot[w];
      before += w < wave ? t : 0u;
      total += t;
    }
    const uint32_t pos = base + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (kept && pos < (uint32_t)n_out) {
      ((uint32_t*)Dout)[pos] = ((const uint32_t*)D)[i];       // score bits unchanged
      Iout[pos] = id;
      if (Kout) Kout[pos] = k;
    }
    base += total;
    __syncthreads();                                          // wave_tot is rewritten by the next chunk
  }
  for (uint32_t p = base + threadIdx.x; p < (uint32_t)n_out; p += THREADS) {
    ((uint32_t*)Dout)[p] = DISTINCT_PAD_SCORE_BITS;
    Iout[p] = -1;
    if (Kout) Kout[p] = -1;
  }
  if (lane == 0) atomicAdd(&sh_valid, wave_valid);            // (a sum of integers: the order of arrival does not show)
  if (oob) sh_oob = 1u;                                       // (every writer writes the same value)
  __syncthreads();
  if (counts && threadIdx.x == 0) {
    counts[2 * q] = sh_oob ? -1 : (int32_t)base;
    counts[2 * q + 1] = (int32_t)sh_valid;
  }
}

constexpr int TOPK_DISTINCT_MAX_N = 4096;
constexpr int TOPK_DISTINCT_MAX_LDS = TOPK_DISTINCT_MAX_N * 8 + 2 * TOPK_DISTINCT_MAX_N * 4;   // keys + table: 64 KB

template <int THREADS>
static int launch_topk_distinct(const float* D, const int64_t* I, int n, int64_t ld, int nq, const int64_t* key_map,
                                int64_t key_map_len, int n_out, float* Dout, int64_t* Iout, int64_t* Kout, int64_t ldo,
                                int32_t* counts, hipStream_t st) {
  static DeviceOnce attr_done;
  if (attr_done.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_topk_distinct<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         TOPK_DISTINCT_MAX_LDS));
  int hbits = 6;                                              // at least 2n slots (load <= 1/2), at least 64
  while ((1 << hbits) < 2 * n) ++hbits;
  hipLaunchKernelGGL((k_topk_distinct<THREADS>), dim3(nq), dim3(THREADS), (size_t)n * 8 + ((size_t)4 << hbits), st, D, I, n, ld,
                     key_map, key_map_len, n_out, Dout, Iout, Kout, ldo, counts, hbits);
  CONVDR_CHECK_LAUNCH("k_topk_distinct");
  return 0;
}
}  // namespace convdr

extern "C" int convdr_topk_distinct(const float* D, const int64_t* I, int n, int64_t ld, int nq, const int64_t* key_map,
                                    int64_t key_map_len, int n_out, float* Dout, int64_t* Iout, int64_t* Kout, int64_t ldo,
                                    int32_t* counts, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(n >= 0 && n <= TOPK_DISTINCT_MAX_N && n_out >= 0 && n_out <= TOPK_DISTINCT_MAX_N && nq >= 0 &&
                     key_map_len >= 0 && (key_map != nullptr || key_map_len == 0),
                 "convdr_topk_distinct: bad sizes n=%d n_out=%d nq=%d key_map_len=%lld (n, n_out <= %d; key_map_len = 0 "
                 "without a key_map)", n, n_out, nq, (long long)key_map_len, TOPK_DISTINCT_MAX_N);
  CONVDR_REQUIRE(ld >= n && ldo >= n_out, "convdr_topk_distinct: pitch smaller than the row (ld=%lld n=%d, ldo=%lld n_out=%d)",
                 (long long)ld, n, (long long)ldo, n_out);
  if (nq == 0 || n_out == 0) return 0;
  // 256 threads up to 1024 entries (four chunks of the ordered compaction), 1024 beyond
  if (n <= 1024)
    return launch_topk_distinct<256>(D, I, n, ld, nq, key_map, key_map_len, n_out, Dout, Iout, Kout, ldo, counts, (hipStream_t)stream);
  return launch_topk_distinct<1024>(D, I, n, ld, nq, key_map, key_map_len, n_out, Dout, Iout, Kout, ldo, counts, (hipStream_t)stream);
}
