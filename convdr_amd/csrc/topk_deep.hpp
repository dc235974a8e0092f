// Deep lists for the two list kernels that follow a deep search: the first occurrence per key (convdr_topk_distinct_deep)
// and the W-way merge (convdr_topk_merge_deep[_packed]) for lists of up to 65,536 entries.  Included by ip_topk.hip after
// the kernels it mirrors (k_topk_distinct, k_topk_merge_multi): same contracts, same bytes, the lists left in global memory.
#pragma once

namespace convdr {

constexpr int TOPK_DEEP_MAX_N = 65536;
constexpr int TOPK_DISTINCT_DEEP_THREADS = 1024;

// ---- first occurrence per key, keys and table in global memory -----------------------------------------------------
// k_topk_distinct with its two LDS arrays moved into the workspace (at n = 65,536: 512 KB of keys and a 512 KB table per
// query).  One workgroup per query, the phases and their barriers are the shallow kernel's:
//   stage    key[i] -> workspace, the table filled with DISTINCT_EMPTY by the kernel itself
//   claim    as k_topk_distinct, the atomics now 32-bit global ones (performed at L2).  Before any atomic the slot is READ:
//            a holder with the element's key and a smaller position settles the element without one.  The read may be stale
//            (it is served by this CU's L1, which the atomics pass by): a claimed slot never changes its key and its position
//            only falls, so an old value can only send the element to the atomic it would have issued anyway.  Without the
//            read a list that carries ONE key sends n atomics to one address.
//   compact  as k_topk_distinct.  The table is read with agent-scope loads (they are served by L2): the claim phase's reads
//            may have left older copies of these lines in L1.  The keys are written once, before the first barrier, and are
//            read plainly.
// No result depends on what the workspace held before, and two runs write the same bytes.
__global__ void __launch_bounds__(TOPK_DISTINCT_DEEP_THREADS)
k_topk_distinct_deep(const float* __restrict__ D, const int64_t* __restrict__ I, int n, int64_t ld,
                     const int64_t* __restrict__ key_map, int64_t key_map_len, int n_out, float* __restrict__ Dout,
                     int64_t* __restrict__ Iout, int64_t* __restrict__ Kout, int64_t ldo, int32_t* __restrict__ counts,
                     int64_t* __restrict__ keys, uint32_t* tables, int hbits) {
  constexpr int THREADS = TOPK_DISTINCT_DEEP_THREADS, WAVES = THREADS / 64;
  __shared__ uint32_t wave_tot[WAVES];
  __shared__ uint32_t sh_valid, sh_oob;
  const uint32_t hmask = (1u << hbits) - 1u;
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t* key = keys + (int64_t)q * n;                       // [n]
  uint32_t* table = tables + ((size_t)q << hbits);            // [1 << hbits]
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
      // (a relaxed workgroup-scope load is a plain load to the hardware and keeps the race with the atomics defined)
      uint32_t o = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (o != DISTINCT_EMPTY) {
        if (o >= (uint32_t)n || key[o] != k) continue;        // another key holds this slot, for good
        if (o > (uint32_t)i) atomicMin(&table[h], (uint32_t)i);
        break;
      }
      o = atomicCAS(&table[h], DISTINCT_EMPTY, (uint32_t)i);
      if (o == DISTINCT_EMPTY) break;
      if (key[o] == k) {
        if (o > (uint32_t)i) atomicMin(&table[h], (uint32_t)i);
        break;
      }
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
          o = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (o >= (uint32_t)n || key[o] == k) break;         // (EMPTY is >= n)
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

struct DistinctDeepPlan {
  int hbits;                 // table slots = 1 << hbits: >= 2n (load <= 1/2), at least 64
  size_t o_keys, o_tables, total;
};

static bool topk_distinct_deep_sizes_ok(int nq, int n) { return nq >= 0 && n >= 0 && n <= TOPK_DEEP_MAX_N; }

static DistinctDeepPlan topk_distinct_deep_plan(int nq, int n) {
  DistinctDeepPlan p;
  p.hbits = 6;
  while (((int64_t)1 << p.hbits) < 2 * (int64_t)n) ++p.hbits;
  p.o_keys = 0;
  p.o_tables = align_up((size_t)nq * n * 8, 256);
  p.total = p.o_tables + (size_t)nq * ((size_t)4 << p.hbits);    // (a table is a multiple of 256 bytes)
  return p;
}

// ---- W-way merge, lists in global memory ----------------------------------------------------------------------------
// k_topk_merge_multi without the LDS staging, for lists of up to 65,536 entries: every element's slot is independent of
// every other's, so a query's nlists * m elements (m = min(n, n_out)) are cut into chunks of TOPK_MERGE_DEEP_CHUNK over
// grid.y.  The slot formula, the score floor, the search cut to n_out - slot entries with its last entry probed first
// and the early end of the walk are k_topk_merge_multi's; each workgroup takes the floor from W loads of its own.
// Every output slot is written by exactly one element of one workgroup.
constexpr int TOPK_MERGE_DEEP_THREADS = 256;
constexpr int TOPK_MERGE_DEEP_CHUNK = 1024;      // elements per workgroup: grid.y <= 64 * 65536 / 1024 = 4096
constexpr int TOPK_MERGE_DEEP_MAX_LISTS = 64;

template <class Lists>
__global__ void __launch_bounds__(TOPK_MERGE_DEEP_THREADS) k_topk_merge_deep(Lists in, int nlists, int m, int n_out,
                                                                             float* __restrict__ Dout,
                                                                             int64_t* __restrict__ Iout, int64_t ldo) {
  __shared__ float sh_floor[TOPK_MERGE_DEEP_MAX_LISTS];
  const int q = blockIdx.x;
  const int total = nlists * m;
  Dout += q * ldo; Iout += q * ldo;
  const int p = (n_out + nlists - 1) / nlists - 1;            // exists in every list: see k_topk_merge_multi
  if ((int)threadIdx.x < nlists) sh_floor[threadIdx.x] = in.score(threadIdx.x, q, p);
  __syncthreads();
  float floor_v = sh_floor[0];
  for (int u = 1; u < nlists; ++u) floor_v = fminf(floor_v, sh_floor[u]);
  const int e0 = blockIdx.y * TOPK_MERGE_DEEP_CHUNK;
  const int e1 = total - e0 < TOPK_MERGE_DEEP_CHUNK ? total : e0 + TOPK_MERGE_DEEP_CHUNK;
  for (int e = e0 + threadIdx.x; e < e1; e += TOPK_MERGE_DEEP_THREADS) {
    const int w = e / m, j = e - w * m;
    const float v = in.score(w, q, j);
    if (v < floor_v) continue;
    int pos = j;
    for (int u = 0; u < nlists && pos < n_out; ++u) {
      if (u == w) continue;
      const bool earlier = u < w;
      int lo = 0, hi = m < n_out - pos ? m : n_out - pos;
      const float last = in.score(u, q, hi - 1);
      if (earlier ? (last >= v) : (last > v)) {
        lo = hi;
      } else {
        --hi;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const float x = in.score(u, q, mid);
          const bool precedes = earlier ? (x >= v) : (x > v);
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

static bool topk_merge_deep_sizes_ok(int nlists, int n, int nq, int n_out) {
  return nlists >= 1 && nlists <= TOPK_MERGE_DEEP_MAX_LISTS && n >= 0 && n <= TOPK_DEEP_MAX_N && nq >= 0 && n_out >= 0 &&
         (int64_t)n_out <= (int64_t)nlists * n && (int64_t)nlists * (n < n_out ? n : n_out) < ((int64_t)1 << 31);
}

template <class Lists>
static int topk_merge_deep(const Lists& in, int nlists, int n, int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo,
                           hipStream_t st) {
  const int m = n < n_out ? n : n_out;
  const int chunks = (int)ceil_div64((int64_t)nlists * m, TOPK_MERGE_DEEP_CHUNK);
  hipLaunchKernelGGL((k_topk_merge_deep<Lists>), dim3(nq, chunks), dim3(TOPK_MERGE_DEEP_THREADS), 0, st, in, nlists, m, n_out,
                     Dout, Iout, ldo);
  CONVDR_CHECK_LAUNCH("k_topk_merge_deep");
  return 0;
}

}  // namespace convdr

extern "C" size_t convdr_topk_distinct_deep_workspace_bytes(int nq, int n) {
  using namespace convdr;
  if (!topk_distinct_deep_sizes_ok(nq, n)) return 0;
  return topk_distinct_deep_plan(nq, n).total;
}

extern "C" int convdr_topk_distinct_deep(const float* D, const int64_t* I, int n, int64_t ld, int nq, const int64_t* key_map,
                                         int64_t key_map_len, int n_out, float* Dout, int64_t* Iout, int64_t* Kout,
                                         int64_t ldo, int32_t* counts, void* workspace, size_t workspace_bytes,
                                         convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(topk_distinct_deep_sizes_ok(nq, n) && n_out >= 0 && n_out <= TOPK_DEEP_MAX_N && key_map_len >= 0 &&
                     (key_map != nullptr || key_map_len == 0),
                 "convdr_topk_distinct_deep: bad sizes n=%d n_out=%d nq=%d key_map_len=%lld (n, n_out <= %d; key_map_len = 0 "
                 "without a key_map)", n, n_out, nq, (long long)key_map_len, TOPK_DEEP_MAX_N);
  CONVDR_REQUIRE(ld >= n && ldo >= n_out, "convdr_topk_distinct_deep: pitch smaller than the row (ld=%lld n=%d, ldo=%lld n_out=%d)",
                 (long long)ld, n, (long long)ldo, n_out);
  const DistinctDeepPlan p = topk_distinct_deep_plan(nq, n);
  CONVDR_REQUIRE(workspace_bytes >= p.total, "convdr_topk_distinct_deep: workspace too small (%zu < %zu)", workspace_bytes, p.total);
  if (nq == 0 || n_out == 0) return 0;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(k_topk_distinct_deep, dim3(nq), dim3(TOPK_DISTINCT_DEEP_THREADS), 0, (hipStream_t)stream, D, I, n, ld, key_map,
                     key_map_len, n_out, Dout, Iout, Kout, ldo, counts, (int64_t*)(ws + p.o_keys), (uint32_t*)(ws + p.o_tables),
                     p.hbits);
  CONVDR_CHECK_LAUNCH("k_topk_distinct_deep");
  return 0;
}

extern "C" int convdr_topk_merge_deep(const float* D, const int64_t* I, int nlists, int n, int64_t list_stride, int64_t ld,
                                      int nq, int n_out, float* Dout, int64_t* Iout, int64_t ldo, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(topk_merge_deep_sizes_ok(nlists, n, nq, n_out),
                 "convdr_topk_merge_deep: bad sizes nlists=%d n=%d n_out=%d nq=%d (1 <= nlists <= %d, n <= %d, n_out <= nlists * n)",
                 nlists, n, n_out, nq, TOPK_MERGE_DEEP_MAX_LISTS, TOPK_DEEP_MAX_N);
  CONVDR_REQUIRE(ld >= n && ldo >= n_out && (nlists == 1 || nq == 0 || list_stride >= n),
                 "convdr_topk_merge_deep: pitch smaller than the row (ld=%lld list_stride=%lld n=%d, ldo=%lld n_out=%d)",
                 (long long)ld, (long long)list_stride, n, (long long)ldo, n_out);
  if (nq == 0 || n_out == 0) return 0;
  return topk_merge_deep(MergeListsPlain{D, I, list_stride, ld}, nlists, n, nq, n_out, Dout, Iout, ldo, (hipStream_t)stream);
}

extern "C" int convdr_topk_merge_deep_packed(const void* lists, int nlists, int n, int nq, int n_out, float* Dout,
                                             int64_t* Iout, int64_t ldo, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(topk_merge_deep_sizes_ok(nlists, n, nq, n_out),
                 "convdr_topk_merge_deep_packed: bad sizes nlists=%d n=%d n_out=%d nq=%d (1 <= nlists <= %d, n <= %d, n_out <= "
                 "nlists * n)", nlists, n, n_out, nq, TOPK_MERGE_DEEP_MAX_LISTS, TOPK_DEEP_MAX_N);
  CONVDR_REQUIRE(ldo >= n_out, "convdr_topk_merge_deep_packed: pitch smaller than the row (ldo=%lld n_out=%d)", (long long)ldo,
                 n_out);
  if (nq == 0 || n_out == 0) return 0;
  return topk_merge_deep(MergeListsPacked{(const uint32_t*)lists, (int64_t)nq, (int64_t)n}, nlists, n, nq, n_out, Dout, Iout,
                         ldo, (hipStream_t)stream);
}
