// Row ids: membership and location of a list of 64-bit keys in a column of row keys (included by ip_topk.hip after
// ip_compact.hpp; contract in include/convdr_hip.h, "Row ids").  No table outlives a call: every operation builds a hash set
// from the m keys of its list -- small, L2 resident -- and the n rows probe it in one streaming pass over the column.
//
//   k_keyset_init      head written (status 0, log2 S), every slot empty, the caller's status word zero         build, launch 1
//   k_keyset_insert    list position j claims the slot of keys[j] (64-bit CAS) and folds j into its min position build, launch 2
//   k_keyset_reset     per-slot min row / row count, the head's status and counts[2] back to "no row" member / locate, launch 1
//   k_keys_member      256 rows per workgroup probe the set; every wave ballots its 64 rows into two words  member, launch 2
//   k_keys_missing     slots that hold a key no row had                                                    member, launch 3
//   k_keys_rows        every row that hits folds itself into its slot's min row and count                  locate, launch 2
//   k_keys_answer      per list position: first row, count, smallest position with the same key            locate, launch 3
//   k_compact_ids      src -> dst by the tile prefix of convdr_ip_compact_plan, 8 bytes per row            compact_ids
//
// The set.  Open addressing, linear probing, S = the smallest power of two >= max(64, 2 m) slots: load factor <= 1/2.  The home
// slot of key k is keyset_mix(k) & (S - 1), keyset_mix the 64-bit finaliser below (every input bit reaches every output bit, so
// keys that differ only above bit 20, or by a stride, do not share low hash bits).  KEYSET_EMPTY = INT64_MIN marks a free slot
// and is therefore no legal key: a list or a column that holds it sets a status bit, and such a row never hits.
// Every probe loop runs at most S steps.  With at most m <= S / 2 slots taken a probe always meets its key or a free slot
// first; the bound is there so that a defect ends in a status bit (KEYSET_ST_PROBE), not in a workgroup that spins.
// The row passes are not told m: they read log2 S from the head the build wrote and refuse (KEYSET_ST_NOSET, nothing else
// read or written beyond the head) a value that is no slot count or whose layout would not fit the workspace they were given.
// Atomics: device-scope 64-bit atomicCAS claims a slot, atomicMin / atomicAdd / atomicOr fold results; the row bitmap is
// written with plain stores, one lane per wave, no atomics.  All sums are integers: the outputs are the same in every run.
#pragma once

namespace convdr {

constexpr long long KEYSET_EMPTY = (long long)0x8000000000000000ull;     // INT64_MIN
constexpr int64_t KEYSET_MAX_M = (int64_t)1 << 27;
constexpr int KEYSET_MIN_LG = 6, KEYSET_MAX_LG = 28;                     // 64 <= S <= 2^28
constexpr uint32_t KEYSET_NONE = 0xffffffffu;                            // no list position / no row / no slot
constexpr uint32_t KEYSET_ST_LIST = 1u;      // the list holds INT64_MIN
constexpr uint32_t KEYSET_ST_PROBE = 2u;     // a probe ran S steps without meeting its key or a free slot
constexpr uint32_t KEYSET_ST_COLUMN = 4u;    // the column holds INT64_MIN
constexpr uint32_t KEYSET_ST_NOSET = 8u;     // the workspace holds no set that fits workspace_bytes
constexpr int KEYSET_HEAD_BYTES = 256;       // the head region: word 0 = status of the row passes, word 1 = log2 S
constexpr int KEYSET_PASS_BLOCKS = 2048;     // grid of the per-slot passes (they stride over the S slots)

// The fixed mixer (the finaliser of splitmix64).
__host__ __device__ __forceinline__ uint64_t keyset_mix(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

struct KeySet {              // the regions of the workspace, as device pointers
  uint32_t* head;            // [64]
  long long* key;            // [S]   KEYSET_EMPTY or the slot's key
  uint32_t* pos;             // [S]   smallest list position that holds the key
  uint32_t* row;             // [S]   smallest row that holds the key (KEYSET_NONE: none)          -- the row passes
  uint32_t* cnt;             // [S]   rows that hold the key (member: 0 / 1)                       -- the row passes
  uint64_t S;
};

// every region starts on a 256-byte boundary: S >= 64
__host__ __device__ __forceinline__ KeySet keyset_at(void* workspace, int lg) {
  char* ws = (char*)workspace;
  const uint64_t S = (uint64_t)1 << lg;
  return KeySet{(uint32_t*)ws, (long long*)(ws + KEYSET_HEAD_BYTES), (uint32_t*)(ws + KEYSET_HEAD_BYTES + 8 * S),
                (uint32_t*)(ws + KEYSET_HEAD_BYTES + 12 * S), (uint32_t*)(ws + KEYSET_HEAD_BYTES + 16 * S), S};
}
static inline size_t keyset_bytes(int lg) { return (size_t)KEYSET_HEAD_BYTES + 20 * ((size_t)1 << lg); }

// the set the build left in the workspace; false: the head names no slot count in [2^6, 2^max_lg]
__device__ __forceinline__ bool keyset_open(void* workspace, int max_lg, KeySet* ks) {
  const uint32_t lg = ((const uint32_t*)workspace)[1];
  if (lg < (uint32_t)KEYSET_MIN_LG || lg > (uint32_t)max_lg) return false;
  *ks = keyset_at(workspace, (int)lg);
  return true;
}

// slot of `key` or KEYSET_NONE (not in the set); sets *exhausted when the bound ended the loop.  key != KEYSET_EMPTY.
__device__ __forceinline__ uint32_t keyset_find(const KeySet& ks, long long key, bool* exhausted) {
  const uint64_t mask = ks.S - 1;
  uint64_t s = keyset_mix((uint64_t)key) & mask;
  for (uint64_t i = 0; i < ks.S; ++i, s = (s + 1) & mask) {
    const long long have = ks.key[s];
    if (have == key) return (uint32_t)s;
    if (have == KEYSET_EMPTY) return KEYSET_NONE;
  }
  *exhausted = true;
  return KEYSET_NONE;
}

__global__ void __launch_bounds__(256) k_keyset_init(KeySet ks, int lg, int32_t* __restrict__ status) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ks.S; i += (uint64_t)gridDim.x * 256) {
    ks.key[i] = KEYSET_EMPTY; ks.pos[i] = KEYSET_NONE; ks.row[i] = KEYSET_NONE; ks.cnt[i] = 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x < KEYSET_HEAD_BYTES / 4) ks.head[threadIdx.x] = threadIdx.x == 1 ? (uint32_t)lg : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
}

__global__ void __launch_bounds__(256) k_keyset_insert(KeySet ks, const long long* __restrict__ keys, int64_t m,
                                                       int32_t* __restrict__ status) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const long long key = keys[j];
  if (key == KEYSET_EMPTY) { atomicOr((unsigned int*)status, KEYSET_ST_LIST); return; }
  const uint64_t mask = ks.S - 1;
  uint64_t s = keyset_mix((uint64_t)key) & mask;
  for (uint64_t i = 0; i < ks.S; ++i, s = (s + 1) & mask) {
    const unsigned long long was = atomicCAS((unsigned long long*)&ks.key[s], (unsigned long long)KEYSET_EMPTY, (unsigned long long)key);
    if (was == (unsigned long long)KEYSET_EMPTY || was == (unsigned long long)key) {
      atomicMin(&ks.pos[s], (uint32_t)j);
      return;
    }
  }
  atomicOr((unsigned int*)status, KEYSET_ST_PROBE);
}

// The state of the row passes: a set serves any number of member / locate calls after one build.  The first launch of both:
// it alone decides whether the head names a set, and says so in the head's status word.
__global__ void __launch_bounds__(256) k_keyset_reset(void* workspace, int max_lg, unsigned long long* __restrict__ counts) {
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (first && counts) { counts[0] = 0ull; counts[1] = 0ull; }
  KeySet ks;
  if (!keyset_open(workspace, max_lg, &ks)) {
    if (first) ((uint32_t*)workspace)[0] = KEYSET_ST_NOSET;
    return;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ks.S; i += (uint64_t)gridDim.x * 256) {
    ks.row[i] = KEYSET_NONE; ks.cnt[i] = 0u;
  }
  if (first) ks.head[0] = 0u;
}

// One workgroup per 256-row tile, one row per thread.  bit = (row < n) and ((its key is in the set) != invert).
__global__ void __launch_bounds__(256) k_keys_member(void* workspace, int max_lg, const long long* __restrict__ row_keys, int64_t n,
                                                     int invert, uint32_t* __restrict__ bits, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  const bool open = keyset_open(workspace, max_lg, &ks);     // (workgroup uniform; no set: an all-zero bitmap, NOSET is set)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool hit = false, exhausted = false;
  if (open && r < n) {
    const long long key = __builtin_nontemporal_load(row_keys + r);
    if (key == KEYSET_EMPTY) {
      atomicOr(&ks.head[0], KEYSET_ST_COLUMN);
    } else {
      const uint32_t s = keyset_find(ks, key, &exhausted);
      if (s != KEYSET_NONE) {
        hit = true;
        if (ks.cnt[s] == 0u) ks.cnt[s] = 1u;       // every writer stores the same word: "some row holds this key"
      }
    }
    if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
  }
  const bool bit = open && r < n && (hit != (invert != 0));
  const unsigned long long b = __ballot(bit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    uint32_t* w = bits + (int64_t)blockIdx.x * 8 + wave * 2;
    w[0] = (uint32_t)b;
    w[1] = (uint32_t)(b >> 32);
    sh[wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t c = sh[0] + sh[1] + sh[2] + sh[3];
    if (c) atomicAdd(&counts[0], (unsigned long long)c);
  }
}

// counts[1] += slots whose key no row held
__global__ void __launch_bounds__(256) k_keys_missing(void* workspace, int max_lg, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t sh[4];
  KeySet ks;
  if (!keyset_open(workspace, max_lg, &ks)) return;
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ks.S; i += (uint64_t)gridDim.x * 256)
    mine += (ks.key[i] != KEYSET_EMPTY && ks.cnt[i] == 0u) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t c = sh[0] + sh[1] + sh[2] + sh[3];
    if (c) atomicAdd(&counts[1], (unsigned long long)c);
  }
}

__global__ void __launch_bounds__(256) k_keys_rows(void* workspace, int max_lg, const long long* __restrict__ row_keys, int64_t n) {
  KeySet ks;
  if (!keyset_open(workspace, max_lg, &ks)) return;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const long long key = __builtin_nontemporal_load(row_keys + r);
  if (key == KEYSET_EMPTY) { atomicOr(&ks.head[0], KEYSET_ST_COLUMN); return; }
  bool exhausted = false;
  const uint32_t s = keyset_find(ks, key, &exhausted);
  if (s != KEYSET_NONE) {
    atomicMin(&ks.row[s], (uint32_t)r);
    atomicAdd(&ks.cnt[s], 1u);
  }
  if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
}

// no set: (-1, 0, j) for every position, NOSET is set
__global__ void __launch_bounds__(256) k_keys_answer(void* workspace, int max_lg, const long long* __restrict__ keys, int64_t m,
                                                     int64_t* __restrict__ first_row, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ dup_of) {
  KeySet ks;
  const bool open = keyset_open(workspace, max_lg, &ks);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const long long key = keys[j];
  bool exhausted = false;
  const uint32_t s = (!open || key == KEYSET_EMPTY) ? KEYSET_NONE : keyset_find(ks, key, &exhausted);
  int64_t fr = -1;
  int32_t c = 0, dup = (int32_t)j;                   // (a key the set does not hold -- INT64_MIN -- stands for itself)
  if (s != KEYSET_NONE) {
    const uint32_t row = ks.row[s];
    fr = row == KEYSET_NONE ? -1 : (int64_t)row;
    c = (int32_t)ks.cnt[s];
    dup = (int32_t)ks.pos[s];
  }
  first_row[j] = fr;
  count[j] = c;
  if (dup_of) dup_of[j] = dup;
  if (exhausted) atomicOr(&ks.head[0], KEYSET_ST_PROBE);
}

// dst[tile_base[t] + rank of r among its tile's kept rows] = src[r]: out of place, stable; bits == NULL: every row kept
__global__ void __launch_bounds__(256) k_compact_ids(const long long* __restrict__ src, long long* __restrict__ dst, int64_t n,
                                                     const uint32_t* __restrict__ bits, const uint32_t* __restrict__ tile_base) {
  const int64_t t = blockIdx.x;
  const int r = threadIdx.x, wd = r >> 5, bit = r & 31;
  const int64_t row = t * COMPACT_TILE + r;
  if (row >= n) return;
  uint32_t rank = 32u * wd, word = 0xffffffffu;
  if (bits) {
    const uint32_t* tw = bits + t * 8;
    rank = 0;
    for (int i = 0; i < wd; ++i) rank += __popc(tw[i]);
    word = tw[wd];
  }
  rank += __popc(word & ((1u << bit) - 1u));
  const int64_t at = (int64_t)tile_base[t] + rank;       // (< n for the plan of this bitmap; a plan of another one must not
  if (((word >> bit) & 1u) && at < n) dst[at] = __builtin_nontemporal_load(src + row);      //  send the store past dst)
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int keyset_lg(int64_t m) {            // log2 of the slot count for a list of m keys
  int lg = KEYSET_MIN_LG;
  while (((int64_t)1 << lg) < 2 * m) ++lg;
  return lg;
}

static int keyset_check_m(const char* name, int64_t m) {
  CONVDR_REQUIRE(m >= 0 && m <= KEYSET_MAX_M, "%s: bad list length m=%lld (0 <= m <= 2^27)", name, (long long)m);
  return 0;
}

// a row pass: the largest log2 S whose layout fits the workspace it was given (the device holds the set's own)
static int keyset_max_lg(const char* name, size_t workspace_bytes, int* max_lg) {
  if (int e = ip_check_workspace(name, workspace_bytes, keyset_bytes(KEYSET_MIN_LG))) return e;
  int lg = KEYSET_MIN_LG;
  while (lg < KEYSET_MAX_LG && keyset_bytes(lg + 1) <= workspace_bytes) ++lg;
  *max_lg = lg;
  return 0;
}

static int keyset_pass_blocks(int lg) {
  const uint64_t b = (((uint64_t)1 << lg) + 255) / 256;
  return b < (uint64_t)KEYSET_PASS_BLOCKS ? (int)b : KEYSET_PASS_BLOCKS;
}

}  // namespace convdr

extern "C" size_t convdr_keyset_workspace_bytes(int64_t m) {
  using namespace convdr;
  if (keyset_check_m("convdr_keyset_build", m)) return 0;
  return keyset_bytes(keyset_lg(m));
}

extern "C" int convdr_keyset_build(const int64_t* keys, int64_t m, void* workspace, size_t workspace_bytes, int32_t* status,
                                   convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_keyset_build";
  if (int e = keyset_check_m(name, m)) return e;
  CONVDR_REQUIRE((keys || m == 0) && workspace && status, "%s: a NULL argument (keys, workspace, status)", name);
  const int lg = keyset_lg(m);
  if (int e = ip_check_workspace(name, workspace_bytes, keyset_bytes(lg))) return e;
  hipStream_t st = (hipStream_t)stream;
  const KeySet ks = keyset_at(workspace, lg);
  ProfScope prof("keyset_build", st);
  hipLaunchKernelGGL(k_keyset_init, dim3(keyset_pass_blocks(lg)), dim3(256), 0, st, ks, lg, status);
  CONVDR_CHECK_LAUNCH("k_keyset_init");
  if (m > 0) {
    hipLaunchKernelGGL(k_keyset_insert, dim3((unsigned)ceil_div64(m, 256)), dim3(256), 0, st, ks, (const long long*)keys, m, status);
    CONVDR_CHECK_LAUNCH("k_keyset_insert");
  }
  return 0;
}

extern "C" int convdr_keys_member(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, int invert,
                                  uint32_t* bits, int64_t bits_words, int64_t* counts, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_keys_member";
  if (int e = compact_check_n(name, n)) return e;
  CONVDR_REQUIRE((row_keys || n == 0) && workspace && (bits || n == 0) && counts,
                 "%s: a NULL argument (row_keys, workspace, bits, counts)", name);
  if (n > 0)
    if (int e = compact_check_bits(name, bits, bits_words, n)) return e;
  int max_lg = 0;
  if (int e = keyset_max_lg(name, workspace_bytes, &max_lg)) return e;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* c = (unsigned long long*)counts;
  ProfScope prof("keys_member", st);
  hipLaunchKernelGGL(k_keyset_reset, dim3(keyset_pass_blocks(max_lg)), dim3(256), 0, st, workspace, max_lg, c);
  CONVDR_CHECK_LAUNCH("k_keyset_reset");
  if (n > 0) {
    hipLaunchKernelGGL(k_keys_member, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, workspace, max_lg, (const long long*)row_keys,
                       n, invert, bits, c);
    CONVDR_CHECK_LAUNCH("k_keys_member");
  }
  hipLaunchKernelGGL(k_keys_missing, dim3(keyset_pass_blocks(max_lg)), dim3(256), 0, st, workspace, max_lg, c);
  CONVDR_CHECK_LAUNCH("k_keys_missing");
  return 0;
}

extern "C" int convdr_keys_locate(const int64_t* row_keys, int64_t n, void* workspace, size_t workspace_bytes, const int64_t* keys,
                                  int64_t m, int64_t* first_row, int32_t* count, int32_t* dup_of, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_keys_locate";
  if (int e = keyset_check_m(name, m)) return e;
  if (int e = compact_check_n(name, n)) return e;
  CONVDR_REQUIRE((row_keys || n == 0) && workspace && ((keys && first_row && count) || m == 0),
                 "%s: a NULL argument (row_keys, workspace, keys, first_row, count)", name);
  if (int e = ip_check_workspace(name, workspace_bytes, keyset_bytes(keyset_lg(m)))) return e;
  int max_lg = 0;
  if (int e = keyset_max_lg(name, workspace_bytes, &max_lg)) return e;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof("keys_locate", st);
  hipLaunchKernelGGL(k_keyset_reset, dim3(keyset_pass_blocks(max_lg)), dim3(256), 0, st, workspace, max_lg, (unsigned long long*)nullptr);
  CONVDR_CHECK_LAUNCH("k_keyset_reset");
  if (n > 0) {
    hipLaunchKernelGGL(k_keys_rows, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, workspace, max_lg, (const long long*)row_keys, n);
    CONVDR_CHECK_LAUNCH("k_keys_rows");
  }
  if (m > 0) {
    hipLaunchKernelGGL(k_keys_answer, dim3((unsigned)ceil_div64(m, 256)), dim3(256), 0, st, workspace, max_lg, (const long long*)keys, m,
                       first_row, count, dup_of);
    CONVDR_CHECK_LAUNCH("k_keys_answer");
  }
  return 0;
}

extern "C" int convdr_ip_compact_ids(const int64_t* src, int64_t* dst, int64_t n, const uint32_t* keep_bits, int64_t keep_bits_words,
                                     const void* plan_workspace, size_t workspace_bytes, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_compact_ids";
  if (int e = compact_check_n(name, n)) return e;
  if (int e = compact_check_bits(name, keep_bits, keep_bits_words, n)) return e;
  const CompactPlan p = compact_plan(n, 16, COMPACT_TILE);
  if (int e = ip_check_workspace(name, workspace_bytes, p.o_bounce)) return e;       // (the plan's regions)
  if (n == 0) return 0;
  CONVDR_REQUIRE(src && dst && plan_workspace, "%s: a NULL argument (src, dst, plan_workspace)", name);
  CONVDR_REQUIRE(src != dst, "%s: src and dst are the same buffer (the ids are compacted out of place)", name);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t* tile_base = (const uint32_t*)((const char*)plan_workspace + p.o_tile_base);
  ProfScope prof("ip_compact_ids", st);
  hipLaunchKernelGGL(k_compact_ids, dim3((unsigned)p.T), dim3(256), 0, st, (const long long*)src, (long long*)dst, n, keep_bits, tile_base);
  CONVDR_CHECK_LAUNCH("k_compact_ids");
  return 0;
}
