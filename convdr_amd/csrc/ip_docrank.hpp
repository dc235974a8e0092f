// Document rank: how many DOCUMENTS precede a given row (included by ip_topk.hip after ip_docs.hpp; contract in
// include/convdr_hip.h, "Document rank").  A document is the set of rows that carry one key; it stands where its best row
// stands, so document D precedes a target row t iff at least ONE row of D precedes t -- and "precedes t" is what the band-count
// scan of ip_rank.hpp already decides per row.  Distinct documents are counted in a bitmap, one bit per document and pair.
//
//   k_keyset_init, k_keyset_insert   the key set of ip_keys.hpp over the COLUMN as a list of n keys: pos[slot] is the smallest
//                       list position of the key, i.e. the document's first row                          ordinals, launches 1-2
//   k_ord_block_sums    per 256 rows: the rows that OWN their document (pos[slot] == row), counted         ordinals, launch 3
//   k_docs_scan_blocks  exclusive scan of the block sums, one workgroup; the total is ndocs (ip_docs.hpp)  ordinals, launch 4
//   k_ord_starts        the scan inside each block; every owner writes its document's number into its slot ordinals, launch 5
//   k_ord_write         ord[r] = the number in the slot of row_keys[r]                                     ordinals, launch 6
//   k_ip_scan_r3<MARK>  the band-count scan; a row with S~ >= tau_hi also ORs its document's bit (ip_scan.hpp)
//   k_ip_docrank_mark_band   the re-scored band entries that precede the target OR their document's bit    rank, after the re-score
//   k_ip_docrank_count  popcount of the pair's bitmap with the target's own document cleared; status       rank, last launch
//
// Ordinals.  ord[r] = #{distinct keys whose first row lies below the first row of row_keys[r]}: 0 .. ndocs - 1 in the order of
// first appearance.  Which slot a key lands in depends on the order colliding inserts arrive in; first rows do not, so the
// values are the same bits in every run.  A row that holds INT64_MIN is in no document: ord = 0xffffffff (never a bit) and
// bit 2 of the head's status word.  Plain vector stores; the only atomics are the key set's own and the status bits.
// The bitmap.  Both marking steps use non-returning relaxed agent-scope ORs; the count is a SEPARATE launch, so the words it
// reads were completed by the launches before it in stream order -- no fence, no flag, no workgroup waits for another.
#pragma once

namespace convdr {

constexpr int ORD_HEAD_BYTES = 256;          // u32 word 0: ndocs, word 1: the build's status (convdr_keyset_build's *status)
constexpr uint32_t ORD_NONE = 0xffffffffu;   // the row is in no document

struct OrdPlan {
  int lg;
  int64_t blocks;            // ceil(n / 256)
  size_t o_head, o_num, o_bsum, total;
};

// Workspace layout (include/convdr_hip.h, "Document rank": workspace): the key set's regions first.
static OrdPlan ord_plan(int64_t n) {
  OrdPlan p;
  p.lg = keyset_lg(n);
  p.blocks = ceil_div64(n, 256);
  WsCursor ws;
  ws.take(keyset_bytes(p.lg));
  p.o_head = ws.take(ORD_HEAD_BYTES);
  p.o_num = ws.take(4 * ((size_t)1 << p.lg));
  p.o_bsum = ws.take(4 * (size_t)p.blocks);
  p.total = ws.at;
  return p;
}

// 1 if row r is the first row of its key (its slot: *slot), else 0 and KEYSET_NONE
__device__ __forceinline__ uint32_t ord_own(const KeySet& ks, bool open, const long long* __restrict__ row_keys, int64_t r, int64_t n,
                                            uint32_t* slot, bool* exhausted) {
  docs_own(ks, open, row_keys, r, n, slot, exhausted);       // (the row count it returns is not ours: no row pass has run)
  return *slot != KEYSET_NONE ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_ord_block_sums(void* workspace, int lg, const long long* __restrict__ row_keys, int64_t n,
                                                        uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  uint32_t slot, sum;
  bool exhausted = false;
  const uint32_t own = ord_own(ks, open, row_keys, (int64_t)blockIdx.x * 256 + threadIdx.x, n, &slot, &exhausted);
  docs_block_scan<4>(own, sh, &sum);
  if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
  if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
}

__global__ void __launch_bounds__(256) k_ord_starts(void* workspace, int lg, const long long* __restrict__ row_keys, int64_t n,
                                                    const uint32_t* __restrict__ bsum, uint32_t* __restrict__ num) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  uint32_t slot, sum;
  bool exhausted = false;
  const uint32_t own = ord_own(ks, open, row_keys, (int64_t)blockIdx.x * 256 + threadIdx.x, n, &slot, &exhausted);
  const uint32_t incl = docs_block_scan<4>(own, sh, &sum);
  if (slot != KEYSET_NONE) num[slot] = bsum[blockIdx.x] + incl - own;
}

// no set: every row ORD_NONE (k_docs_scan_blocks has set NOSET).  dhead[1]: what the build reported; its probe bit is folded
// into the head's status word, its list bit is the column bit here (the list IS the column), raised by the rows that hold it.
__global__ void __launch_bounds__(256) k_ord_write(void* workspace, int lg, const long long* __restrict__ row_keys, int64_t n,
                                                   const uint32_t* __restrict__ num, const uint32_t* __restrict__ dhead,
                                                   uint32_t* __restrict__ ord) {
  KeySet ks;
  const bool open = docs_open(workspace, lg, &ks);
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (open && r == 0 && (dhead[1] & KEYSET_ST_PROBE)) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
  if (r >= n) return;
  uint32_t o = ORD_NONE;
  if (open) {
    const long long key = __builtin_nontemporal_load(row_keys + r);
    if (key == KEYSET_EMPTY) {
      atomicOr(&ks.head[0], KEYSET_ST_COLUMN);
    } else {
      bool exhausted = false;
      const uint32_t s = keyset_find(ks, key, &exhausted);
      if (s != KEYSET_NONE) o = num[s];
      if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
    }
  }
  ord[r] = o;
}

// One workgroup per pair, over the re-scored band list (the first min(hits, cap) entries, written by this call's scan and
// re-score).  An entry that precedes the target -- the predicate of k_ip_rank_finish -- ORs its document's bit.  An entry
// outside [0, n) or an ordinal that names no document stores nothing.
__global__ void __launch_bounds__(IP_RANK_THREADS) k_ip_docrank_mark_band(int cap, int64_t n, const uint32_t* __restrict__ hits,
                                                                          const uint32_t* __restrict__ list_id,
                                                                          const double* __restrict__ list_x,
                                                                          const int64_t* __restrict__ tgt, const double* __restrict__ xt,
                                                                          const uint32_t* __restrict__ ord, int64_t ndocs,
                                                                          int64_t mark_words, uint32_t* __restrict__ marks) {
  const int q = blockIdx.x;
  const int64_t t = tgt[q];
  if (!(t >= 0 && t < n)) return;                                    // (uniform) nothing was scanned for it
  const uint32_t cnt = ip_hits(hits, q);
  const int m = cnt < (uint32_t)cap ? (int)cnt : cap;
  const double x_t = xt[q];
  const uint32_t* li = list_id + (int64_t)q * cap;
  const double* lx = list_x + (int64_t)q * cap;
  uint32_t* mk = marks + (int64_t)q * mark_words;
  for (int i = threadIdx.x; i < m; i += IP_RANK_THREADS) {
    const double x = lx[i];
    const int64_t r = (int64_t)li[i];
    if (!(x > x_t || (x == x_t && r < t)) || r >= n) continue;
    const uint32_t o = ord[r];
    if ((int64_t)o < ndocs && (int64_t)(o >> 5) < mark_words)
      __hip_atomic_fetch_or(&mk[o >> 5], 1u << (o & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup per pair: rank = the set bits of the pair's bitmap, the bit of the target's own document cleared in
// registers.  counts / above / status: the rules of k_ip_rank_finish.
__global__ void __launch_bounds__(IP_RANK_THREADS) k_ip_docrank_count(int cap, int64_t n, const uint32_t* __restrict__ hits,
                                                                      const uint32_t* __restrict__ above_in,
                                                                      const uint32_t* __restrict__ bad, const int64_t* __restrict__ tgt,
                                                                      const IpBand band, const uint32_t* __restrict__ ord, int64_t ndocs,
                                                                      int64_t mark_words, const uint32_t* __restrict__ marks,
                                                                      int64_t* __restrict__ rank, int64_t* __restrict__ counts,
                                                                      int64_t* __restrict__ above, int32_t* __restrict__ status) {
  __shared__ uint32_t sh_g;
  const int q = blockIdx.x;
  const int64_t t = tgt[q];
  if (!(t >= 0 && t < n)) {         // (uniform) padding or an id outside the block: rank -1, nothing was scanned for it
    if (threadIdx.x == 0) { rank[q] = -1; counts[q] = 0; above[q] = 0; status[q] = CONVDR_IP_OK; }
    return;
  }
  if (threadIdx.x == 0) sh_g = 0;
  __syncthreads();
  const uint32_t own = ord[t];                                       // (ORD_NONE: the target is in no document, nothing cleared)
  const int64_t used = (ndocs + 31) / 32;                            // (the words past them hold no document's bit)
  const int64_t words = used < mark_words ? used : mark_words;
  const uint32_t* mk = marks + (int64_t)q * mark_words;
  uint32_t mine = 0;
  for (int64_t wd = threadIdx.x; wd < words; wd += IP_RANK_THREADS) {
    uint32_t v = mk[wd];
    if ((int64_t)(own >> 5) == wd) v &= ~(1u << (own & 31));
    mine += (uint32_t)__popc(v);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&sh_g, mine);       // (a sum of integers: the order of arrival does not show)
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t cnt = ip_hits(hits, q);
    const int st = ip_list_verdict(cnt, cap, bad[q], band.out_of_range(q));
    rank[q] = st == CONVDR_IP_OK ? (int64_t)sh_g : -1;
    counts[q] = (int64_t)cnt;
    above[q] = (int64_t)ip_hits(above_in, q);
    status[q] = st;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Two launches, on purpose: the count reads words the marking launches OR'ed, and stream order is what completes them.
static int ip_docrank_finish(const DocRankFinish& f, hipStream_t st) {
  if (f.n > 0 && f.ndocs > 0) {
    hipLaunchKernelGGL(k_ip_docrank_mark_band, dim3(f.np), dim3(IP_RANK_THREADS), 0, st, f.cap, f.n, f.hits, f.list_id, f.list_x, f.target,
                       f.xt, f.ord, f.ndocs, f.mark_words, f.marks);
    CONVDR_CHECK_LAUNCH("k_ip_docrank_mark_band");
  }
  hipLaunchKernelGGL(k_ip_docrank_count, dim3(f.np), dim3(IP_RANK_THREADS), 0, st, f.cap, f.n, f.hits, f.above_u, f.bad, f.target, f.band,
                     f.ord, f.ndocs, f.mark_words, f.marks, f.rank, f.counts, f.above, f.status);
  CONVDR_CHECK_LAUNCH("k_ip_docrank_count");
  return 0;
}

}  // namespace convdr

extern "C" size_t convdr_doc_ordinals_workspace_bytes(int64_t n) {
  using namespace convdr;
  if (keyset_check_m("convdr_doc_ordinals", n)) return 0;
  return ord_plan(n).total;
}

extern "C" int convdr_doc_ordinals(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, uint32_t* ord,
                                   int64_t* ndocs, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_doc_ordinals";
  if (int e = keyset_check_m(name, n)) return e;
  CONVDR_REQUIRE(((row_keys && ord) || n == 0) && workspace && ndocs, "%s: a NULL argument (row_keys, workspace, ord, ndocs)", name);
  const OrdPlan p = ord_plan(n);
  if (int e = ip_check_workspace(name, workspace_bytes, p.total)) return e;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const KeySet ks = keyset_at(workspace, p.lg);
  uint32_t* dhead = (uint32_t*)(ws + p.o_head);
  uint32_t* num = (uint32_t*)(ws + p.o_num);
  uint32_t* bsum = (uint32_t*)(ws + p.o_bsum);
  const long long* col = (const long long*)row_keys;
  const dim3 grid((unsigned)p.blocks);
  ProfScope prof("doc_ordinals", st);
  hipLaunchKernelGGL(k_keyset_init, dim3(keyset_pass_blocks(p.lg)), dim3(256), 0, st, ks, p.lg, (int32_t*)(dhead + 1));
  CONVDR_CHECK_LAUNCH("k_keyset_init");
  if (n > 0) {
    hipLaunchKernelGGL(k_keyset_insert, grid, dim3(256), 0, st, ks, col, n, (int32_t*)(dhead + 1));
    CONVDR_CHECK_LAUNCH("k_keyset_insert");
    hipLaunchKernelGGL(k_ord_block_sums, grid, dim3(256), 0, st, workspace, p.lg, col, n, bsum);
    CONVDR_CHECK_LAUNCH("k_ord_block_sums");
  }
  hipLaunchKernelGGL(k_docs_scan_blocks, dim3(1), dim3(DOCS_SCAN_THREADS), 0, st, workspace, p.lg, bsum, p.blocks, dhead, ndocs);
  CONVDR_CHECK_LAUNCH("k_docs_scan_blocks");
  if (n > 0) {
    hipLaunchKernelGGL(k_ord_starts, grid, dim3(256), 0, st, workspace, p.lg, col, n, bsum, num);
    CONVDR_CHECK_LAUNCH("k_ord_starts");
    hipLaunchKernelGGL(k_ord_write, grid, dim3(256), 0, st, workspace, p.lg, col, n, num, dhead, ord);
    CONVDR_CHECK_LAUNCH("k_ord_write");
  }
  return 0;
}

extern "C" size_t convdr_ip_rank_docs_workspace_bytes(int np, int64_t n, int d, int cap, int64_t ndocs) {
  using namespace convdr;
  if (ip_check_sizes(IP_RANK_DOCS, np, n, d, 0, cap)) return 0;
  if (!(ndocs >= 0 && ndocs <= n)) {
    set_error("%s: ndocs=%lld outside [0, n=%lld]", IP_RANK_DOCS.entry, (long long)ndocs, (long long)n);
    return 0;
  }
  return ip_rank_plan(np, n, d, cap).total + docrank_mark_bytes(np, ndocs);
}

extern "C" int convdr_ip_rank_docs(int store, const float* q_f32, int np, const int64_t* target, const float* p_f32,
                                   const void* p_half, float p_scale, const float* centre, int64_t n, int d,
                                   const float* p_max_norm, const uint32_t* row_bits, int64_t row_bits_words, int64_t n_allowed,
                                   const uint32_t* ord, int64_t ndocs, int cap, void* workspace, size_t workspace_bytes,
                                   int64_t* rank, double* X, int64_t* counts, int64_t* above, int32_t* status, convdr_stream_t stream) {
  using namespace convdr;
  CONVDR_REQUIRE(store >= 0 && store <= 2, "convdr_ip_rank_docs: store must be 0 (bf16 copy), 1 (fp16 copy) or 2 (half store) "
                 "(got %d)", store);
  const IpBlock b = {store, p_f32, p_half, nullptr, store == 0 ? 1.f : p_scale, false, n, d, p_max_norm, row_bits, row_bits_words,
                     row_bits ? n_allowed : n};
  const RankDocs docs = {ord, ndocs};
  return ip_rank_rows(IP_RANK_DOCS, b, q_f32, np, target, centre, cap, workspace, workspace_bytes, rank, X, counts, above, status, &docs,
                      (hipStream_t)stream);
}
