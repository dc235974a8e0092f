// A streaming, position-dependent digest of rows (included by ip_topk.hip after ip_keys.hpp, whose mixer it uses; contract in
// include/convdr_hip.h, "Digest and snapshot file").  It is what a snapshot file's bytes are checked against where they land:
// in HBM after a load (k_digest_rows), on the host over the file (convdr_digest_host).
//
// Definition.  A buffer is m little-endian 64-bit words w[0 .. m) with a starting word index word0.  With g_i = word0 + i + 1,
// mix = keyset_mix (the splitmix64 finaliser), K1 = 0x9e3779b97f4a7c15, K2 = 0xd6e8feb86659fd93, everything mod 2^64:
//   A = sum_i mix(w_i ^ (g_i * K1))
//   B = sum_i mix(rotl(w_i, 29) ^ (g_i * K2))
// The digest is (A, B); the empty buffer gives (0, 0).
//   position-dependent   a word's term depends on its index: rows that were swapped, shifted or left stale change both sums,
//                        and so does a window of zeros at the wrong place (mix(g K) differs per g; g >= 1, so no term is mix(0)).
//   additive             the digest of a concatenation is the wrapping sum of the parts' digests, each taken at its own word0.
//                        Any split into windows, chunks, workgroups or lanes gives the same bits: the device result is
//                        deterministic although it is summed with atomics (integer adds commute), and host == device.
//   NOT cryptographic    it detects accidents (a torn copy, a stale buffer, a flipped bit), not an adversary: both sums are
//                        linear in per-word terms anyone can compute.
//
//   k_digest_rows   grid = windows x blocks-per-window, 256 threads.  A workgroup grid-strides over its window's 16-byte
//                   pieces (non-temporal loads, four in flight per lane); a window that starts or ends on an odd word of a
//                   16-byte line has an 8-byte head / tail word, taken by one lane of the window's first workgroup.  Each lane
//                   keeps two 64-bit sums and forms g K incrementally (one add per step).  Wave64 shuffle reduction, the four
//                   waves through 64 bytes of LDS, then ONE pair of 64-bit atomic adds per workgroup into the window's slot.
//                   The entry zeroes the slots on the same stream first.  Every loop is bounded by the sizes passed.
#pragma once

namespace convdr {

constexpr uint64_t DIGEST_K1 = 0x9e3779b97f4a7c15ull, DIGEST_K2 = 0xd6e8feb86659fd93ull;
constexpr int DIGEST_THREADS = 256;
constexpr int DIGEST_UNROLL = 4;                      // 16-byte loads in flight per lane
constexpr int64_t DIGEST_GRID_BLOCKS = 4096;          // workgroups of a launch, about (16 per CU): windows x blocks-per-window
constexpr int64_t DIGEST_MAX_ROWS = (int64_t)1 << 40, DIGEST_MAX_ROW_BYTES = (int64_t)1 << 20;
constexpr int64_t DIGEST_MAX_WINDOWS = (int64_t)1 << 30;

// one word's two terms: gk1 = g K1, gk2 = g K2 of its index
__host__ __device__ __forceinline__ void digest_word(uint64_t w, uint64_t gk1, uint64_t gk2, uint64_t& A, uint64_t& B) {
  A += keyset_mix(w ^ gk1);
  B += keyset_mix(((w << 29) | (w >> 35)) ^ gk2);
}

// the host form: m words at `p` (any alignment), the first with index word0
static void digest_words_host(const unsigned char* p, int64_t m, uint64_t word0, uint64_t out[2]) {
  uint64_t A = 0, B = 0, gk1 = (word0 + 1) * DIGEST_K1, gk2 = (word0 + 1) * DIGEST_K2;
  for (int64_t i = 0; i < m; ++i, gk1 += DIGEST_K1, gk2 += DIGEST_K2) {
    uint64_t w;
    memcpy(&w, p + 8 * i, 8);
    digest_word(w, gk1, gk2, A, B);
  }
  out[0] = A;
  out[1] = B;
}

__device__ __forceinline__ uint64_t digest_wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// Window j = blockIdx.x / bpw covers words [j * window_words, min(m, (j + 1) * window_words)) of `buf`; workgroup part =
// blockIdx.x % bpw of it takes the pieces part * 256 + lane, + bpw * 256, ...
__global__ void __launch_bounds__(DIGEST_THREADS) k_digest_rows(const char* __restrict__ buf, int64_t m, int64_t window_words,
                                                                uint64_t word0, uint32_t bpw, unsigned long long* __restrict__ out) {
  __shared__ uint64_t sh[2 * DIGEST_THREADS / 64];
  const int64_t win = blockIdx.x / bpw;
  const uint32_t part = blockIdx.x - (uint32_t)win * bpw;
  const int64_t a = win * window_words;                                   // (< m: the grid has ceil(m / window_words) windows)
  const int64_t b = a + window_words < m ? a + window_words : m;
  // the window's words: an 8-byte head when its first word is the upper half of a 16-byte line, whole lines, an 8-byte tail
  const int64_t head = (int64_t)((((uintptr_t)buf >> 3) + (uint64_t)a) & 1u);
  const int64_t first = a + head < b ? a + head : b;                      // first word of the first whole line
  const int64_t pieces = (b - first) >> 1;
  const int64_t tail = first + 2 * pieces;                                // (== b, or the one word left)
  uint64_t A = 0, B = 0;
  if (part == 0 && threadIdx.x == 0) {
    if (head && a < b) {
      const uint64_t g = word0 + (uint64_t)a + 1;
      digest_word(__builtin_nontemporal_load((const uint64_t*)(buf + 8 * a)), g * DIGEST_K1, g * DIGEST_K2, A, B);
    }
    if (tail < b) {
      const uint64_t g = word0 + (uint64_t)tail + 1;
      digest_word(__builtin_nontemporal_load((const uint64_t*)(buf + 8 * tail)), g * DIGEST_K1, g * DIGEST_K2, A, B);
    }
  }
  const int64_t step = (int64_t)bpw * DIGEST_THREADS;                     // pieces between a lane's consecutive loads
  const char* src = buf + 8 * first;
  int64_t i0 = (int64_t)part * DIGEST_THREADS + threadIdx.x;
  // g K of the first word of piece i0, then one add per piece: a piece is two words, a step 2 * step words
  uint64_t gk1 = (word0 + (uint64_t)first + 2 * (uint64_t)i0 + 1) * DIGEST_K1;
  uint64_t gk2 = (word0 + (uint64_t)first + 2 * (uint64_t)i0 + 1) * DIGEST_K2;
  const uint64_t s1 = 2 * (uint64_t)step * DIGEST_K1, s2 = 2 * (uint64_t)step * DIGEST_K2;
  for (; i0 < pieces; i0 += DIGEST_UNROLL * step) {
    compact_u32x4 v[DIGEST_UNROLL];
#pragma unroll
    for (int u = 0; u < DIGEST_UNROLL; ++u)
      if (i0 + u * step < pieces) v[u] = compact_load16(src + ((i0 + u * step) << 4));
#pragma unroll
    for (int u = 0; u < DIGEST_UNROLL; ++u) {
      if (i0 + u * step < pieces) {
        digest_word((uint64_t)v[u].x | ((uint64_t)v[u].y << 32), gk1, gk2, A, B);
        digest_word((uint64_t)v[u].z | ((uint64_t)v[u].w << 32), gk1 + DIGEST_K1, gk2 + DIGEST_K2, A, B);
      }
      gk1 += s1;
      gk2 += s2;
    }
  }
  A = digest_wave_sum(A);
  B = digest_wave_sum(B);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[2 * wave] = A; sh[2 * wave + 1] = B; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < DIGEST_THREADS / 64; ++i) { A += sh[2 * i]; B += sh[2 * i + 1]; }
    atomicAdd(out + 2 * win, (unsigned long long)A);
    atomicAdd(out + 2 * win + 1, (unsigned long long)B);
  }
}

}  // namespace convdr

extern "C" int convdr_digest_rows(const void* buf, int64_t n_rows, int64_t row_bytes, uint64_t word0, int64_t window_rows,
                                  uint64_t* out, convdr_stream_t stream) {
  using namespace convdr;
  const char* name = "convdr_digest_rows";
  CONVDR_REQUIRE(n_rows >= 0 && n_rows <= DIGEST_MAX_ROWS, "%s: bad row count n_rows=%lld (0 <= n_rows <= 2^40)", name,
                 (long long)n_rows);
  CONVDR_REQUIRE(row_bytes > 0 && row_bytes <= DIGEST_MAX_ROW_BYTES && row_bytes % 8 == 0,
                 "%s: need row_bytes %% 8 == 0 and 8 <= row_bytes <= %lld (got %lld)", name, (long long)DIGEST_MAX_ROW_BYTES,
                 (long long)row_bytes);
  CONVDR_REQUIRE(window_rows >= 1, "%s: window_rows must be >= 1 (got %lld)", name, (long long)window_rows);
  CONVDR_REQUIRE(((uintptr_t)buf & 7u) == 0, "%s: buf must be 8-byte aligned", name);
  if (window_rows > n_rows) window_rows = n_rows > 0 ? n_rows : 1;        // (one window; keeps window_rows * row_bytes small)
  const int64_t windows = ceil_div64(n_rows, window_rows);
  CONVDR_REQUIRE(windows <= DIGEST_MAX_WINDOWS, "%s: %lld windows (n_rows=%lld, window_rows=%lld), at most 2^30", name,
                 (long long)windows, (long long)n_rows, (long long)window_rows);
  if (n_rows == 0) return 0;
  CONVDR_REQUIRE(buf && out, "%s: a NULL argument (buf, out)", name);
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_words = row_bytes >> 3, window_words = window_rows * row_words;
  // workgroups per window: one per 256 x 4 pieces, as many as keep the launch near DIGEST_GRID_BLOCKS in all
  int64_t bpw = ceil_div64(window_words >> 1, (int64_t)DIGEST_THREADS * DIGEST_UNROLL);
  const int64_t most = DIGEST_GRID_BLOCKS / windows;
  if (bpw > most) bpw = most;
  if (bpw < 1) bpw = 1;
  ProfScope prof("digest_rows", st);
  CONVDR_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)windows * 16, st));
  hipLaunchKernelGGL(k_digest_rows, dim3((unsigned)(windows * bpw)), dim3(DIGEST_THREADS), 0, st, (const char*)buf, n_rows * row_words,
                     window_words, word0, (uint32_t)bpw, (unsigned long long*)out);
  CONVDR_CHECK_LAUNCH("k_digest_rows");
  return 0;
}

extern "C" int convdr_digest_host(const void* buf, int64_t n_bytes, uint64_t word0, uint64_t out[2]) {
  using namespace convdr;
  const char* name = "convdr_digest_host";
  CONVDR_REQUIRE(n_bytes >= 0 && n_bytes % 8 == 0, "%s: need n_bytes %% 8 == 0 and n_bytes >= 0 (got %lld)", name, (long long)n_bytes);
  CONVDR_REQUIRE(out && (buf || n_bytes == 0), "%s: a NULL argument (buf, out)", name);
  digest_words_host((const unsigned char*)buf, n_bytes >> 3, word0, out);
  return 0;
}
