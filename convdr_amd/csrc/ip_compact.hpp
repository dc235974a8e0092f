// Stable in-place compaction of a row buffer (included by ip_topk.hip after ip_rank.hpp; contract in include/convdr_hip.h,
// "Removing rows").  The keep set is the row bitmap of convdr_ip_search_filtered; a kept row r ends at
//   dest(r) = #{kept rows before r} = tile_base[r >> 8] + popcount of its tile's bits before r.
//
//   k_compact_block_sums   kept rows of every chunk of 8,192 tiles (bits past n masked)                       plan, launch 1
//   k_compact_prefix       tile_base[0 .. T]: the exclusive prefix over the T tiles, tile_base[T] = n_kept    plan, launch 2
//   k_compact_gather       one window's kept rows -> their destination (direct form) or the bounce buffer     per window, 1
//   k_compact_unbounce     the bounce buffer -> the window's destination (bounce form only)                   per window, 2
//
// The in-place hazard.  A kept row's destination may be the source of another kept row that has not been read yet, and
// nothing inside one launch orders the two.  The buffer is therefore processed in windows of window_rows consecutive source
// rows, one after the other in STREAM ORDER -- the only ordering used: no flag, no look-back, no workgroup waits for another.
// Window [a, b) with kept_w kept rows writes [dest(a), dest(a) + kept_w).  dest(a) <= a, and dest(a) + kept_w = dest(b) <= b:
// the range can overlap only the window's own sources and rows of earlier windows, which have been moved by earlier
// launches; never a later window's.  Per window, decided on the device from tile_base (workgroup uniform):
//   skip      dest(a) == a and kept_w == b - a: nothing was removed before or inside the window; both launches return.
//   direct    dest(a) + kept_w <= a: the destination lies wholly before the window's sources; the gather writes it.
//   bounce    otherwise: the gather packs the kept rows into the bounce buffer (sources only read), the next launch -- after
//             every read of the window in stream order -- copies them to the destination.
// Both launches are enqueued for every window; the one with nothing to do returns at once.  Sources are always rows no
// launch has written: a destination lies before every later window's sources.
#pragma once

namespace convdr {

constexpr int COMPACT_TILE = 256;                 // rows per bitmap tile (8 words): the scan's tile
constexpr int COMPACT_CHUNK_TILES = 8192;         // tile positions per workgroup of the plan kernels: 1,024 threads x 8
constexpr int64_t COMPACT_MAX_ROW_BYTES = 65536;
constexpr int64_t COMPACT_MAX_WINDOW = 1 << 20;

typedef uint32_t compact_u32x4 __attribute__((ext_vector_type(4)));

// kept rows of tile t (rows [256 t, 256 t + 256) cut at n); bits == NULL: every row is kept.  t >= T: 0.
__device__ __forceinline__ uint32_t compact_tile_count(const uint32_t* __restrict__ bits, int64_t t, int64_t T, int64_t n) {
  if (t >= T) return 0u;
  const int64_t left = n - t * COMPACT_TILE;
  const int valid = left < COMPACT_TILE ? (int)left : COMPACT_TILE;
  if (!bits) return (uint32_t)valid;
  const compact_u32x4 lo = *(const compact_u32x4*)(bits + t * 8), hi = *(const compact_u32x4*)(bits + t * 8 + 4);
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int v = valid - 32 * i;      // rows of this word inside the block
    const uint32_t mask = v >= 32 ? 0xffffffffu : (v <= 0 ? 0u : ((1u << v) - 1u));
    c += __popc(w[i] & mask);
  }
  return c;
}

// sum over the workgroup's 1,024 threads, returned to all; sh: 16 words
__device__ __forceinline__ uint32_t compact_block_sum(uint32_t v, uint32_t* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                   // (sh may still be read from an earlier use)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += sh[i];
  return s;
}

// chunk_sum[c] = kept rows of tile positions [8192 c, 8192 c + 8192)
__global__ void __launch_bounds__(1024) k_compact_block_sums(const uint32_t* __restrict__ bits, int64_t n, int64_t T,
                                                             uint32_t* __restrict__ chunk_sum) {
  __shared__ uint32_t sh[16];
  const int64_t t0 = (int64_t)blockIdx.x * COMPACT_CHUNK_TILES + (int64_t)threadIdx.x * 8;
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) mine += compact_tile_count(bits, t0 + i, T, n);
  const uint32_t s = compact_block_sum(mine, sh);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = s;
}

// tile_base[p] = kept rows before tile p, for the T + 1 positions 0 .. T (position T counts nothing: tile_base[T] is the
// total, also written to *n_kept).  Every workgroup sums the chunk sums before its own (at most 1,025 values).
__global__ void __launch_bounds__(1024) k_compact_prefix(const uint32_t* __restrict__ bits, int64_t n, int64_t T,
                                                         const uint32_t* __restrict__ chunk_sum, uint32_t* __restrict__ tile_base,
                                                         int64_t* __restrict__ n_kept) {
  __shared__ uint32_t sh[16];
  __shared__ uint32_t sh_wave[16];
  uint32_t before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 1024) before += chunk_sum[i];
  const uint32_t base = compact_block_sum(before, sh);
  const int64_t t0 = (int64_t)blockIdx.x * COMPACT_CHUNK_TILES + (int64_t)threadIdx.x * 8;
  uint32_t c[8], mine = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) { c[i] = compact_tile_count(bits, t0 + i, T, n); mine += c[i]; }
  // exclusive scan of `mine` over the workgroup: inclusive within the wave, then the waves before it
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  uint32_t run = base + incl - mine;
  for (int i = 0; i < wave; ++i) run += sh_wave[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (t0 + i <= T) tile_base[t0 + i] = run;
    if (t0 + i == T) *n_kept = (int64_t)run;
    run += c[i];
  }
}

// what a window does, from the prefix (uniform over the launch: one window per launch)
struct CompactWindow {
  int64_t a, b;           // source rows [a, b)
  int64_t dest;           // dest(a)
  int64_t kept;           // kept rows of the window
  int form;               // 0 skip, 1 direct, 2 bounce
};
__device__ __forceinline__ CompactWindow compact_window(const uint32_t* __restrict__ tile_base, int64_t n, int64_t T, int64_t window,
                                                        int64_t window_rows) {
  CompactWindow w;
  w.a = window * window_rows;
  w.b = w.a + window_rows < n ? w.a + window_rows : n;
  const int64_t ta = w.a / COMPACT_TILE, tb = (w.a + window_rows) / COMPACT_TILE;     // (window_rows % 256 == 0)
  w.dest = (int64_t)tile_base[ta];
  w.kept = (int64_t)tile_base[tb < T ? tb : T] - w.dest;
  w.form = (w.dest == w.a && w.kept == w.b - w.a) ? 0 : (w.dest + w.kept <= w.a ? 1 : 2);
  return w;
}

// 16-byte streaming accessors: every byte here is touched once
__device__ __forceinline__ compact_u32x4 compact_load16(const char* p) { return __builtin_nontemporal_load((const compact_u32x4*)p); }

// grid (tiles of the window, parts); 256 threads.  Workgroup (t, part) moves the 16-byte pieces part, part + parts, ... of
// the (kept row, piece) list of tile t, 256 pieces at a time, four loads in flight per thread.
__global__ void __launch_bounds__(256) k_compact_gather(char* __restrict__ rows, int64_t row_bytes, int64_t n, int64_t T,
                                                        const uint32_t* __restrict__ bits, const uint32_t* __restrict__ tile_base,
                                                        int64_t window, int64_t window_rows, char* __restrict__ bounce) {
  __shared__ uint16_t sh_src[COMPACT_TILE];      // sh_src[j] = the tile's j-th kept row
  const CompactWindow w = compact_window(tile_base, n, T, window, window_rows);
  if (w.form == 0 || w.kept == 0) return;
  const int64_t t = w.a / COMPACT_TILE + blockIdx.x;
  if (t >= T) return;
  const uint32_t first = tile_base[t], kept_t = tile_base[t + 1] - first;
  if (kept_t == 0) return;
  {
    const int r = threadIdx.x, wd = r >> 5, bit = r & 31;
    const uint32_t* tw = bits + t * 8;
    uint32_t rank = 0;
    for (int i = 0; i < wd; ++i) rank += __popc(tw[i]);
    const uint32_t word = tw[wd];
    rank += __popc(word & ((1u << bit) - 1u));
    if (((word >> bit) & 1u) && t * COMPACT_TILE + r < n) sh_src[rank] = (uint16_t)r;     // (bits past n are ignored)
  }
  __syncthreads();
  // direct: row j of the tile goes to row first + j of the buffer; bounce: to row first - dest(a) + j of the bounce buffer
  char* dst = w.form == 1 ? rows + (int64_t)first * row_bytes : bounce + ((int64_t)first - w.dest) * row_bytes;
  const char* src = rows + t * COMPACT_TILE * row_bytes;
  const uint32_t ppr = (uint32_t)(row_bytes >> 4);                       // pieces per row
  const uint32_t total = kept_t * ppr;                                   // (<= 256 * 4,096)
  const uint32_t step = 256u * gridDim.y;
  for (uint32_t i0 = blockIdx.y * 256u + threadIdx.x; i0 < total; i0 += 4u * step) {
    compact_u32x4 v[4];
    uint32_t at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t i = i0 + u * step;
      at[u] = i;
      if (i < total) {
        const uint32_t j = i / ppr, c = i - j * ppr;
        v[u] = compact_load16(src + (int64_t)sh_src[j] * row_bytes + ((int64_t)c << 4));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (at[u] < total) store16<true>(dst + ((int64_t)at[u] << 4), v[u]);      // (piece i of the list is piece i of the packed rows)
  }
}

// bounce form only: kept * row_bytes contiguous bytes, bounce -> rows + dest(a) * row_bytes.  A fixed grid strides over them.
__global__ void __launch_bounds__(256) k_compact_unbounce(char* __restrict__ rows, int64_t row_bytes, int64_t n, int64_t T,
                                                          const uint32_t* __restrict__ tile_base, int64_t window,
                                                          int64_t window_rows, const char* __restrict__ bounce) {
  const CompactWindow w = compact_window(tile_base, n, T, window, window_rows);
  if (w.form != 2) return;
  char* dst = rows + w.dest * row_bytes;
  const int64_t total = w.kept * (row_bytes >> 4);
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * step) {
    compact_u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * step < total) v[u] = compact_load16(bounce + ((i0 + u * step) << 4));
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * step < total) store16<true>(dst + ((i0 + u * step) << 4), v[u]);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct CompactPlan {
  int64_t T;                  // tiles
  int chunks;                 // workgroups of the plan kernels: ceil((T + 1) / 8192)
  size_t o_tile_base, o_chunk_sum, o_bounce, total;
};

// Workspace layout (include/convdr_hip.h, "Removing rows": workspace).  The bounce buffer comes last: the regions of the plan
// sit where they sit whatever row_bytes and window_rows are.
static CompactPlan compact_plan(int64_t n, int64_t row_bytes, int64_t window_rows) {
  CompactPlan p{};
  p.T = ceil_div64(n, COMPACT_TILE);
  p.chunks = (int)ceil_div64(p.T + 1, COMPACT_CHUNK_TILES);
  WsCursor ws;
  p.o_tile_base = ws.take((size_t)(p.T + 1) * 4);
  p.o_chunk_sum = ws.take((size_t)p.chunks * 4);
  p.o_bounce = ws.take((size_t)window_rows * (size_t)row_bytes);
  p.total = ws.at;
  return p;
}

static int compact_check_n(const char* name, int64_t n) {
  CONVDR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: bad block size n=%lld (0 <= n < 2^31)", name, (long long)n);
  return 0;
}

static int compact_check_shape(const char* name, int64_t row_bytes, int64_t window_rows) {
  CONVDR_REQUIRE(row_bytes >= 16 && row_bytes <= COMPACT_MAX_ROW_BYTES && row_bytes % 16 == 0,
                 "%s: need row_bytes %% 16 == 0 and 16 <= row_bytes <= %lld (got %lld)", name, (long long)COMPACT_MAX_ROW_BYTES,
                 (long long)row_bytes);
  CONVDR_REQUIRE(window_rows >= COMPACT_TILE && window_rows <= COMPACT_MAX_WINDOW && window_rows % COMPACT_TILE == 0,
                 "%s: window_rows must be a multiple of 256 in [256, %lld] (got %lld)", name, (long long)COMPACT_MAX_WINDOW,
                 (long long)window_rows);
  return 0;
}

static int compact_check_bits(const char* name, const uint32_t* keep_bits, int64_t keep_bits_words, int64_t n) {
  CONVDR_REQUIRE(keep_bits != nullptr || keep_bits_words == 0, "%s: keep_bits is NULL but keep_bits_words=%lld", name,
                 (long long)keep_bits_words);
  const IpBlock b = {0, nullptr, nullptr, nullptr, 1.f, false, n, 64, nullptr, keep_bits, keep_bits_words, 0};
  return ip_check_block(name, b);                  // alignment and length: the bitmap contract of the filtered search
}

}  // namespace convdr

extern "C" size_t convdr_ip_compact_workspace_bytes(int64_t n, int64_t row_bytes, int64_t window_rows) {
  using namespace convdr;
  const char* name = "convdr_ip_compact_rows";
  if (compact_check_shape(name, row_bytes, window_rows) || compact_check_n(name, n)) return 0;
  return compact_plan(n, row_bytes, window_rows).total;
}

extern "C" int convdr_ip_compact_plan(const uint32_t* keep_bits, int64_t keep_bits_words, int64_t n, void* workspace,
                                      size_t workspace_bytes, int64_t* n_kept, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_compact_plan";
  if (int e = compact_check_n(name, n)) return e;
  if (int e = compact_check_bits(name, keep_bits, keep_bits_words, n)) return e;
  const CompactPlan p = compact_plan(n, 16, COMPACT_TILE);
  if (int e = ip_check_workspace(name, workspace_bytes, p.o_bounce)) return e;       // (the plan's regions: all but the bounce buffer)
  CONVDR_REQUIRE(workspace && n_kept, "%s: a NULL argument (workspace, n_kept)", name);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* tile_base = (uint32_t*)(ws + p.o_tile_base);
  uint32_t* chunk_sum = (uint32_t*)(ws + p.o_chunk_sum);
  ProfScope prof("ip_compact_plan", st);
  hipLaunchKernelGGL(k_compact_block_sums, dim3(p.chunks), dim3(1024), 0, st, keep_bits, n, p.T, chunk_sum);
  CONVDR_CHECK_LAUNCH("k_compact_block_sums");
  hipLaunchKernelGGL(k_compact_prefix, dim3(p.chunks), dim3(1024), 0, st, keep_bits, n, p.T, chunk_sum, tile_base, n_kept);
  CONVDR_CHECK_LAUNCH("k_compact_prefix");
  return 0;
}

extern "C" int convdr_ip_compact_rows(void* rows, int64_t row_bytes, int64_t n, const uint32_t* keep_bits, int64_t keep_bits_words,
                                      int64_t window_rows, void* workspace, size_t workspace_bytes, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_ip_compact_rows";
  if (int e = compact_check_shape(name, row_bytes, window_rows)) return e;
  if (int e = compact_check_n(name, n)) return e;
  if (int e = compact_check_bits(name, keep_bits, keep_bits_words, n)) return e;
  const CompactPlan p = compact_plan(n, row_bytes, window_rows);
  if (int e = ip_check_workspace(name, workspace_bytes, p.total)) return e;
  if (n == 0 || !keep_bits) return 0;              // nothing to move: an empty block, or every row kept
  CONVDR_REQUIRE(rows && workspace, "%s: a NULL argument (rows, workspace)", name);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const uint32_t* tile_base = (const uint32_t*)(ws + p.o_tile_base);
  char* bounce = ws + p.o_bounce;
  const int64_t windows = ceil_div64(n, window_rows);
  const int tiles_w = (int)(window_rows / COMPACT_TILE);
  // workgroups per tile: about 2,048 per launch, each with at least four rounds of pieces to move
  int parts = 2048 / tiles_w;
  const int most = (int)(row_bytes / 64);            // 256 rows x row_bytes / 16 pieces over 256 threads x 4 rounds
  if (parts > most) parts = most;
  if (parts > 64) parts = 64;
  if (parts < 1) parts = 1;
  ProfScope prof("ip_compact_rows", st);
  for (int64_t w = 0; w < windows; ++w) {
    const int64_t left = ceil_div64(n - w * window_rows, COMPACT_TILE);
    const int tiles = left < tiles_w ? (int)left : tiles_w;
    hipLaunchKernelGGL(k_compact_gather, dim3(tiles, parts), dim3(256), 0, st, (char*)rows, row_bytes, n, p.T, keep_bits, tile_base, w,
                       window_rows, bounce);
    CONVDR_CHECK_LAUNCH("k_compact_gather");
    hipLaunchKernelGGL(k_compact_unbounce, dim3(2048), dim3(256), 0, st, (char*)rows, row_bytes, n, p.T, tile_base, w, window_rows,
                       (const char*)bounce);
    CONVDR_CHECK_LAUNCH("k_compact_unbounce");
  }
  return 0;
}
