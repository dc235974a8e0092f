// Documents by id: ALL rows of every listed key as a CSR, and the MaxP score of (query, document) pairs (included by
// ip_topk.hip after ip_keys.hpp; contract in include/convdr_hip.h, "Documents by id").  A document is the set of rows that
// carry one key; the key set, its probes and the per-slot row counts are those of ip_keys.hpp.
//
//   k_keyset_reset, k_keys_rows   per slot: the rows that hold its key (ip_keys.hpp, unchanged)           count, launches 1-2
//   k_docs_block_sums   per 256 list positions: the rows of the positions that OWN their key (smallest
//                       position of the key), summed                                                        count, launch 3
//   k_docs_scan_blocks  exclusive scan of the block sums, one workgroup; total                             count, launch 4
//   k_docs_starts       the scan inside each block; every owner writes its segment start into its slot     count, launch 5
//   k_docs_answer       per list position: start and count of its key's slot, smallest position            count, launch 6
//   k_docs_fill_reset   per-slot cursors zeroed; total > rows_cap: the status bit                          fill, launch 1
//   k_docs_fill         every row that hits draws a place in its segment (atomic cursor) -> list A         fill, launch 2
//   k_docs_chunk_sort   every 256-entry chunk of every segment rank-sorted: A -> B, and -> rows[] when the
//                       segment is one chunk                                                                fill, launch 3
//   k_docs_merge        pairs of sorted runs of width w merged, w = 256, 512, ... < min(n, rows_cap):
//                       B -> A -> B ..., the pass that finishes a segment writes rows[]                     fill, launches 4 ...
//   k_ip_score_docs     one wave per (query, segment): max of the canonical scores, lowest row on ties
//
// Order.  The segments follow the LIST (exclusive scan over owning positions), not the slots: which slot a key lands in
// depends on the order in which colliding inserts arrive, list positions do not.  Inside a segment the atomic cursors place
// the rows in the order the waves arrive; the sort makes that order irrelevant: rows are distinct integers, so ascending order
// is one permutation.  A chunk is rank-sorted (rank = entries of the chunk below mine: at most 256 steps), runs are merged by
// binary search in the sibling run (at most 32 steps): n log^2 work for a segment of any length, no loop without a bound, and
// no thread waits for another -- ordering between the passes is stream order.
// All stores are plain vector stores; the only atomics are the cursors (atomicAdd on u32) and the status bits (atomicOr).
// Everything the fill reads in the lists it wrote itself: every entry e < total is written exactly once when the column is the
// one the count saw; for another column the range checks of docs_segment keep every access inside the lists.
#pragma once

namespace convdr {

constexpr uint32_t KEYSET_ST_ROWS_CAP = 16u; // total > rows_cap: rows[] was not written
constexpr int DOCS_HEAD_BYTES = 256;         // u32 word 0: total (rows of all distinct listed keys)
constexpr int DOCS_CHUNK = 256;              // entries of a rank-sorted chunk; the first merge width
constexpr int DOCS_SCAN_THREADS = 1024;

struct DocsPlan {
  int lg;
  int64_t blocks;            // ceil(m / 256)
  size_t o_head, o_seg, o_cur, o_bsum, o_list_a, o_list_b, total;
};

// Workspace layout (include/convdr_hip.h, "Documents by id": workspace): the key set's regions first, where
// convdr_keyset_build puts them for the same m.
static DocsPlan docs_plan(int64_t m, int64_t rows_cap) {
  DocsPlan p;
  p.lg = keyset_lg(m);
  p.blocks = ceil_div64(m, 256);
  const size_t S = (size_t)1 << p.lg;
  WsCursor ws;
  ws.take(keyset_bytes(p.lg));
  p.o_head = ws.take(DOCS_HEAD_BYTES);
  p.o_seg = ws.take(4 * S);
  p.o_cur = ws.take(4 * S);
  p.o_bsum = ws.take(4 * (size_t)p.blocks);
  p.o_list_a = ws.take(8 * (size_t)rows_cap);
  p.o_list_b = ws.take(8 * (size_t)rows_cap);
  p.total = ws.at;
  return p;
}

struct Docs {                // the regions behind the key set, as device pointers
  uint32_t* head;            // [64]  word 0: total
  uint32_t* seg;             // [S]   first entry of the slot's segment in rows[] (owners' slots only)
  uint32_t* cur;             // [S]   entries of the segment handed out so far                     -- the fill
  uint32_t* bsum;            // [blocks]  rows owned by 256 list positions, then their exclusive prefix
  uint64_t* list_a;          // [rows_cap]  (slot << 32 | row) per entry                           -- the fill
  uint64_t* list_b;          // [rows_cap]
};

static Docs docs_at(void* workspace, const DocsPlan& p) {
  char* ws = (char*)workspace;
  return Docs{(uint32_t*)(ws + p.o_head), (uint32_t*)(ws + p.o_seg), (uint32_t*)(ws + p.o_cur), (uint32_t*)(ws + p.o_bsum),
              (uint64_t*)(ws + p.o_list_a), (uint64_t*)(ws + p.o_list_b)};
}

// the set of exactly 2^lg slots the build left in the workspace (the regions behind it were laid out for that slot count)
__device__ __forceinline__ bool docs_open(void* workspace, int lg, KeySet* ks) {
  if (((const uint32_t*)workspace)[1] != (uint32_t)lg) return false;
  *ks = keyset_at(workspace, lg);
  return true;
}

// rows of keys[j] if j is the smallest list position of its key (the OWNER of the key's segment), else 0; *slot: its slot
__device__ __forceinline__ uint32_t docs_own(const KeySet& ks, bool open, const long long* __restrict__ keys, int64_t j, int64_t m,
                                             uint32_t* slot, bool* exhausted) {
  *slot = KEYSET_NONE;
  if (!open || j >= m) return 0u;
  const long long key = keys[j];
  if (key == KEYSET_EMPTY) return 0u;
  const uint32_t s = keyset_find(ks, key, exhausted);
  if (s == KEYSET_NONE || ks.pos[s] != (uint32_t)j) return 0u;
  *slot = s;
  return ks.cnt[s];
}

// inclusive scan of one value per thread over the workgroup (WAVES waves); *sum: the workgroup's total.  sh: WAVES words.
template <int WAVES>
__device__ __forceinline__ uint32_t docs_block_scan(uint32_t v, uint32_t* sh, uint32_t* sum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wave] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const uint32_t t = sh[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  __syncthreads();           // (sh is free again)
  *sum = all;
  return before + x;
}

__global__ void __launch_bounds__(256) k_docs_block_sums(void* workspace, int lg, const long long* __restrict__ keys, int64_t m,
                                                         uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  uint32_t slot, sum;
  bool exhausted = false;
  const uint32_t own = docs_own(ks, open, keys, (int64_t)blockIdx.x * 256 + threadIdx.x, m, &slot, &exhausted);
  docs_block_scan<4>(own, sh, &sum);
  if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
  if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
}

// One workgroup: bsum -> its exclusive prefix, DOCS_SCAN_THREADS entries per step with a carry; total.  Every sum is at most
// n < 2^31 (a row holds one key, and a key's rows are counted at one position): u32 cannot wrap.
__global__ void __launch_bounds__(DOCS_SCAN_THREADS) k_docs_scan_blocks(void* workspace, int lg, uint32_t* __restrict__ bsum,
                                                                        int64_t blocks, uint32_t* __restrict__ dhead,
                                                                        int64_t* __restrict__ total) {
  __shared__ uint32_t sh[DOCS_SCAN_THREADS / 64];
  uint32_t carry = 0;
  for (int64_t base = 0; base < blocks; base += DOCS_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < blocks ? bsum[i] : 0u;
    uint32_t sum;
    const uint32_t incl = docs_block_scan<DOCS_SCAN_THREADS / 64>(v, sh, &sum);
    if (i < blocks) bsum[i] = carry + incl - v;
    carry += sum;
  }
  if (threadIdx.x == 0) {
    dhead[0] = carry;
    *total = (int64_t)carry;
    KeySet ks;
    if (!docs_open(workspace, lg, &ks)) atomicOr((uint32_t*)workspace, KEYSET_ST_NOSET);     // (the set is not the list's)
  }
}

__global__ void __launch_bounds__(256) k_docs_starts(void* workspace, int lg, const long long* __restrict__ keys, int64_t m,
                                                     const uint32_t* __restrict__ bsum, uint32_t* __restrict__ seg) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  uint32_t slot, sum;
  bool exhausted = false;
  const uint32_t own = docs_own(ks, open, keys, (int64_t)blockIdx.x * 256 + threadIdx.x, m, &slot, &exhausted);
  const uint32_t incl = docs_block_scan<4>(own, sh, &sum);
  if (slot != KEYSET_NONE) seg[slot] = bsum[blockIdx.x] + incl - own;
}

// no set: (0, 0, j) for every position.  A key the set does not hold (INT64_MIN) has start 0, count 0 and stands for itself.
__global__ void __launch_bounds__(256) k_docs_answer(void* workspace, int lg, const long long* __restrict__ keys, int64_t m,
                                                     const uint32_t* __restrict__ seg, int64_t* __restrict__ start,
                                                     int32_t* __restrict__ count, int32_t* __restrict__ dup_of) {
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const long long key = keys[j];
  bool exhausted = false;
  const uint32_t s = (!open || key == KEYSET_EMPTY) ? KEYSET_NONE : keyset_find(ks, key, &exhausted);
  int64_t st = 0;
  int32_t c = 0, dup = (int32_t)j;
  if (s != KEYSET_NONE) {
    st = (int64_t)seg[s];
    c = (int32_t)ks.cnt[s];
    dup = (int32_t)ks.pos[s];
  }
  start[j] = st;
  count[j] = c;
  if (dup_of) dup_of[j] = dup;
}

__global__ void __launch_bounds__(256) k_docs_fill_reset(void* workspace, int lg, const uint32_t* __restrict__ dhead,
                                                         uint32_t* __restrict__ cur, int64_t rows_cap) {
  KeySet ks;
  if (!docs_open(workspace, lg, &ks)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((uint32_t*)workspace, KEYSET_ST_NOSET);
    return;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ks.S; i += (uint64_t)gridDim.x * 256) cur[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (int64_t)dhead[0] > rows_cap) atomicOr(&ks.head[0], KEYSET_ST_ROWS_CAP);
}

__global__ void __launch_bounds__(256) k_docs_fill(void* workspace, int lg, const long long* __restrict__ row_keys, int64_t n,
                                                   const uint32_t* __restrict__ dhead, const uint32_t* __restrict__ seg,
                                                   uint32_t* __restrict__ cur, uint64_t* __restrict__ list, int64_t rows_cap) {
  KeySet ks;
  if (!docs_open(workspace, lg, &ks)) return;
  const uint32_t total = dhead[0];
  if ((int64_t)total > rows_cap) return;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const long long key = __builtin_nontemporal_load(row_keys + r);
  if (key == KEYSET_EMPTY) return;                   // (the count's row pass has set the status bit)
  bool exhausted = false;
  const uint32_t s = keyset_find(ks, key, &exhausted);
  if (s != KEYSET_NONE) {
    const uint32_t c = atomicAdd(&cur[s], 1u);
    const uint32_t at = seg[s] + c;
    // (both hold for the column the count saw; another column must not send the store past the segment or the list)
    if (c < ks.cnt[s] && at < total) list[at] = (uint64_t)s << 32 | (uint64_t)(uint32_t)r;
  }
  if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
}

// the segment [*start, *start + *len) that entry e of a list belongs to; false: the entry names none that holds e inside
// [0, total) -- it was not written by this fill
__device__ __forceinline__ bool docs_segment(const KeySet& ks, const uint32_t* __restrict__ seg, uint64_t v, uint32_t e, uint32_t total,
                                             uint32_t* start, uint32_t* len) {
  const uint64_t s = v >> 32;
  if (s >= ks.S) return false;
  const uint32_t st = seg[s], L = ks.cnt[s];
  if (st > e || L > total || st > total - L || e - st >= L) return false;
  *start = st;
  *len = L;
  return true;
}

// one thread per entry: its rank inside its 256-entry chunk of its segment; a segment of one chunk is finished here
__global__ void __launch_bounds__(256) k_docs_chunk_sort(void* workspace, int lg, const uint32_t* __restrict__ dhead,
                                                         const uint32_t* __restrict__ seg, const uint64_t* __restrict__ src,
                                                         uint64_t* __restrict__ dst, int64_t* __restrict__ rows, int64_t rows_cap) {
  KeySet ks;
  if (!docs_open(workspace, lg, &ks)) return;
  const uint32_t total = dhead[0];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((int64_t)total > rows_cap || e >= (int64_t)total) return;
  const uint64_t v = src[e];
  uint32_t start, L;
  if (!docs_segment(ks, seg, v, (uint32_t)e, total, &start, &L)) return;
  const uint32_t i = (uint32_t)e - start, c0 = i / DOCS_CHUNK * DOCS_CHUNK;
  const uint32_t c1 = c0 + DOCS_CHUNK < L ? c0 + DOCS_CHUNK : L;
  uint32_t rank = 0;
  for (uint32_t k = c0; k < c1; ++k) rank += src[start + k] < v ? 1u : 0u;
  const uint32_t out = start + c0 + rank;
  dst[out] = v;              // (every entry, finished or not: from here on BOTH lists name the right segment at every position)
  if (L <= (uint32_t)DOCS_CHUNK) rows[out] = (int64_t)(uint32_t)v;
}

// one thread per entry of the segments longer than w: its place among the two sorted runs of width w it belongs to
__global__ void __launch_bounds__(256) k_docs_merge(void* workspace, int lg, const uint32_t* __restrict__ dhead,
                                                    const uint32_t* __restrict__ seg, const uint64_t* __restrict__ src,
                                                    uint64_t* __restrict__ dst, int64_t* __restrict__ rows, int64_t rows_cap, uint32_t w) {
  KeySet ks;
  if (!docs_open(workspace, lg, &ks)) return;
  const uint32_t total = dhead[0];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((int64_t)total > rows_cap || e >= (int64_t)total) return;
  // (position e of either list holds an entry of e's segment: the fill wrote list A, the chunk sort list B, and a pass writes
  //  only entries of a segment into places of that segment -- so a finished segment is recognised and left alone)
  const uint64_t v = src[e];
  uint32_t start, L;
  if (!docs_segment(ks, seg, v, (uint32_t)e, total, &start, &L) || L <= w) return;
  const uint32_t i = (uint32_t)e - start, run = i / w, mine = run * w, sib = (run ^ 1u) * w;
  uint32_t less = 0;
  if (sib < L) {
    uint32_t lo = sib, hi = sib + w < L ? sib + w : L;             // entries of the sibling run below v: [sib, lo)
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (src[start + mid] < v) lo = mid + 1; else hi = mid;
    }
    less = lo - sib;
  }
  const uint32_t out = start + (mine < sib ? mine : sib) + (i - mine) + less;
  if (L <= 2 * w) rows[out] = (int64_t)(uint32_t)v;
  else dst[out] = v;
}

// One wave per (query, segment) pair; grid (nq, chunks).  start / count / X / D / R share the pitch ld.  The wave walks the
// rows of its segment and keeps the largest canonical score (ip_row_score: the value k_ip_score_rows gives for that pair) and
// the row that attains it, the lowest row on equal scores whatever the order of the list.  The first row is taken
// unconditionally: the maximum starts below every score.  A list entry outside [0, n) is skipped and P not touched for it;
// a segment that does not lie inside rows[0, rows_len), or has no valid row, gives the padding pair.
template <class PT>
__global__ void __launch_bounds__(256) k_ip_score_docs(const float* __restrict__ Q, const PT* __restrict__ P, int64_t n, int d,
                                                       const int64_t* __restrict__ rows, int64_t rows_len,
                                                       const int64_t* __restrict__ start, const int32_t* __restrict__ count, int m,
                                                       int64_t ld, double* __restrict__ X, float* __restrict__ D,
                                                       int64_t* __restrict__ R, double unscale) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* qv = Q + (int64_t)q * d;
  for (int j = blockIdx.y * 4 + wave; j < m; j += gridDim.y * 4) {
    const int64_t at = (int64_t)q * ld + j;
    const int64_t s0 = start[at], c = (int64_t)count[at];
    double best = -(double)FLT_MAX;
    int64_t best_row = -1;
    if (c > 0 && s0 >= 0 && s0 <= rows_len - c) {        // (wave-uniform, as everything below)
      for (int64_t i = 0; i < c; ++i) {
        const int64_t id = rows[s0 + i];
        if (id < 0 || id >= n) continue;
        const double x = ip_row_score<PT>(qv, P + id * d, d, lane, unscale);
        if (best_row < 0 || x > best || (x == best && id < best_row)) { best = x; best_row = id; }
      }
    }
    if (lane == 0) {
      if (X) X[at] = best;
      if (D) D[at] = (float)best;
      if (R) R[at] = best_row;
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int docs_check_cap(const char* name, int64_t rows_cap) {
  CONVDR_REQUIRE(rows_cap >= 0 && rows_cap < ((int64_t)1 << 31), "%s: bad list capacity rows_cap=%lld (0 <= rows_cap < 2^31)", name,
                 (long long)rows_cap);
  return 0;
}

}  // namespace convdr

extern "C" size_t convdr_keys_rows_workspace_bytes(int64_t m, int64_t rows_cap) {
  using namespace convdr;
  const char* name = "convdr_keys_rows_workspace_bytes";
  if (keyset_check_m(name, m)) return 0;
  if (docs_check_cap(name, rows_cap)) return 0;
  return docs_plan(m, rows_cap).total;
}

extern "C" int convdr_keys_rows_count(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, const int64_t* keys,
                                      int64_t m, int64_t* start, int32_t* count, int32_t* dup_of, int64_t* total,
                                      convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_keys_rows_count";
  if (int e = keyset_check_m(name, m)) return e;
  if (int e = compact_check_n(name, n)) return e;
  CONVDR_REQUIRE((row_keys || n == 0) && workspace && total && ((keys && start && count) || m == 0),
                 "%s: a NULL argument (row_keys, workspace, total, keys, start, count)", name);
  const DocsPlan p = docs_plan(m, 0);
  if (int e = ip_check_workspace(name, workspace_bytes, p.total)) return e;
  hipStream_t st = (hipStream_t)stream;
  const Docs dc = docs_at(workspace, p);
  const long long* lk = (const long long*)keys;
  ProfScope prof("keys_rows_count", st);
  hipLaunchKernelGGL(k_keyset_reset, dim3(keyset_pass_blocks(p.lg)), dim3(256), 0, st, workspace, p.lg, (unsigned long long*)nullptr);
  CONVDR_CHECK_LAUNCH("k_keyset_reset");
  if (n > 0) {
    hipLaunchKernelGGL(k_keys_rows, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, workspace, p.lg, (const long long*)row_keys, n);
    CONVDR_CHECK_LAUNCH("k_keys_rows");
  }
  if (m > 0) {
    hipLaunchKernelGGL(k_docs_block_sums, dim3((unsigned)p.blocks), dim3(256), 0, st, workspace, p.lg, lk, m, dc.bsum);
    CONVDR_CHECK_LAUNCH("k_docs_block_sums");
  }
  hipLaunchKernelGGL(k_docs_scan_blocks, dim3(1), dim3(DOCS_SCAN_THREADS), 0, st, workspace, p.lg, dc.bsum, p.blocks, dc.head, total);
  CONVDR_CHECK_LAUNCH("k_docs_scan_blocks");
  if (m > 0) {
    hipLaunchKernelGGL(k_docs_starts, dim3((unsigned)p.blocks), dim3(256), 0, st, workspace, p.lg, lk, m, dc.bsum, dc.seg);
    CONVDR_CHECK_LAUNCH("k_docs_starts");
    hipLaunchKernelGGL(k_docs_answer, dim3((unsigned)p.blocks), dim3(256), 0, st, workspace, p.lg, lk, m, dc.seg, start, count, dup_of);
    CONVDR_CHECK_LAUNCH("k_docs_answer");
  }
  return 0;
}

extern "C" int convdr_keys_rows_fill(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, int64_t m,
                                     int64_t* rows, int64_t rows_cap, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_keys_rows_fill";
  if (int e = keyset_check_m(name, m)) return e;
  if (int e = compact_check_n(name, n)) return e;
  if (int e = docs_check_cap(name, rows_cap)) return e;
  CONVDR_REQUIRE((row_keys || n == 0) && workspace && (rows || rows_cap == 0), "%s: a NULL argument (row_keys, workspace, rows)", name);
  const DocsPlan p = docs_plan(m, rows_cap);
  if (int e = ip_check_workspace(name, workspace_bytes, p.total)) return e;
  hipStream_t st = (hipStream_t)stream;
  const Docs dc = docs_at(workspace, p);
  ProfScope prof("keys_rows_fill", st);
  hipLaunchKernelGGL(k_docs_fill_reset, dim3(keyset_pass_blocks(p.lg)), dim3(256), 0, st, workspace, p.lg, dc.head, dc.cur, rows_cap);
  CONVDR_CHECK_LAUNCH("k_docs_fill_reset");
  if (n == 0 || rows_cap == 0) return 0;                 // (no row can hit / no entry may be written)
  hipLaunchKernelGGL(k_docs_fill, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, workspace, p.lg, (const long long*)row_keys, n,
                     dc.head, dc.seg, dc.cur, dc.list_a, rows_cap);
  CONVDR_CHECK_LAUNCH("k_docs_fill");
  const dim3 grid((unsigned)ceil_div64(rows_cap, 256));
  hipLaunchKernelGGL(k_docs_chunk_sort, grid, dim3(256), 0, st, workspace, p.lg, dc.head, dc.seg, dc.list_a, dc.list_b, rows, rows_cap);
  CONVDR_CHECK_LAUNCH("k_docs_chunk_sort");
  // a segment holds at most min(n, rows_cap) entries; the pass of width w finishes the segments of up to 2 w
  const int64_t longest = n < rows_cap ? n : rows_cap;
  uint64_t* src = dc.list_b;
  uint64_t* dst = dc.list_a;
  for (int64_t w = DOCS_CHUNK; w < longest; w *= 2) {
    hipLaunchKernelGGL(k_docs_merge, grid, dim3(256), 0, st, workspace, p.lg, dc.head, dc.seg, src, dst, rows, rows_cap, (uint32_t)w);
    CONVDR_CHECK_LAUNCH("k_docs_merge");
    uint64_t* t = src; src = dst; dst = t;
  }
  return 0;
}

extern "C" int convdr_ip_score_docs(int store, const float* q_f32, int nq, const float* p_f32, const void* p_half, float p_scale,
                                    int64_t n, int d, const int64_t* rows, int64_t rows_len, const int64_t* start,
                                    const int32_t* count, int m, int64_t ld, double* X, float* D, int64_t* R,
                                    convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_score_docs";
  CONVDR_REQUIRE(store >= 0 && store <= 2, "%s: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) (got %d)", name, store);
  CONVDR_REQUIRE(nq >= 0 && m >= 0 && ld >= m, "%s: bad sizes nq=%d m=%d ld=%lld (ld >= m)", name, nq, m, (long long)ld);
  CONVDR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: bad block size n=%lld (0 <= n < 2^31)", name, (long long)n);
  CONVDR_REQUIRE(d > 0 && d % 64 == 0 && d <= 4096, "%s: need d %% 64 == 0 and d <= 4096 (got %d)", name, d);
  CONVDR_REQUIRE(rows_len >= 0, "%s: bad list length rows_len=%lld", name, (long long)rows_len);
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, nullptr, nullptr, 0, 0};
  if (int e = ip_check_block(name, b)) return e;
  if (nq == 0 || m == 0) return 0;
  CONVDR_REQUIRE(q_f32 && start && count && (rows || rows_len == 0), "%s: a NULL argument (q_f32, start, count, rows)", name);
  CONVDR_REQUIRE(n == 0 || (b.rows_f16() ? p_half != nullptr : p_f32 != nullptr),
                 "%s: a NULL block pointer (p_f32; p_half for store = 2)", name);
  if (!X && !D && !R) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = m < 4 ? 1 : (m / 4 < 1024 ? m / 4 : 1024);
  ProfScope prof("ip_score_docs", st);
  if (b.rows_f16())
    hipLaunchKernelGGL(k_ip_score_docs<_Float16>, dim3(nq, chunks), dim3(256), 0, st, q_f32, (const _Float16*)p_half, n, d, rows,
                       rows_len, start, count, m, ld, X, D, R, b.unscale());
  else
    hipLaunchKernelGGL(k_ip_score_docs<float>, dim3(nq, chunks), dim3(256), 0, st, q_f32, p_f32, n, d, rows, rows_len, start, count, m,
                       ld, X, D, R, b.unscale());
  CONVDR_CHECK_LAUNCH("k_ip_score_docs");
  return 0;
}
