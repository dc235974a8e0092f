// From a query's candidate list to its exact top-k (included by ip_topk.hip after ip_scan.hpp): block-wide order statistics
// in LDS, the threshold select (k_tau_select), and the finishing kernels of the shallow search -- k_ip_cut, k_ip_rescore,
// k_ip_select, and k_ip_finish, which is the three in one launch.  The certificate they draw is in ip_certify.hpp, included
// below, after the order statistics it builds on.
#pragma once

namespace convdr {

// ------------------------------------------------------------------------------------------
// Block-wide order statistics in LDS.  The search needs three of them per query -- the r-th largest sample score (the
// threshold), the k-th largest candidate score (the band cut) and the k best re-scored candidates -- and none needs
// the whole list ordered: an MSB-first radix select (one 256-bin histogram per key byte) finds the k-th largest key
// in a handful of barriers where the full bitonic sorts these replaced took 55-78 barrier-separated stages.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f32_order_key(float f) {   // a > b  <=>  key(a) > key(b)   (-0 orders below +0)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_order_key(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
__device__ __forceinline__ uint64_t f64_order_key(double f) {
  const uint64_t u = (uint64_t)__double_as_longlong(f);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

struct SelectScratch {   // static LDS of a selecting kernel
  uint32_t hist[256];
  uint32_t wave_sum[4];
  uint32_t bin, rem;
};

// kth-largest (kth = 1: the maximum; 1 <= kth <= c) of key_at(0..c-1); NBITS = significant key bits (32 or 64).
// Every thread returns the key.  blockDim.x >= 256.
template <int NBITS, class KeyAt>
__device__ uint64_t block_kth_largest(KeyAt key_at, int c, uint32_t kth, SelectScratch& sc) {
  uint64_t prefix = 0, mask = 0;
  uint32_t rem = kth;
  for (int shift = NBITS - 8; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) sc.hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < c; i += blockDim.x) {
      const uint64_t x = key_at(i);
      if ((x & mask) == prefix) atomicAdd(&sc.hist[(uint32_t)(x >> shift) & 255u], 1u);
    }
    __syncthreads();
    // the bin holding the rem-th largest of the keys that match the prefix: suffix sums of the histogram, one bin
    // per thread of the first four waves (shuffle scan inside a wave, the four wave totals through LDS)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t here = 0, incl = 0;
    if (threadIdx.x < 256) {
      here = incl = sc.hist[threadIdx.x];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += v;
      }
      if (lane == 0) sc.wave_sum[wave] = incl;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
      uint32_t above = incl - here;
      for (int v = wave + 1; v < 4; ++v) above += sc.wave_sum[v];
      if (above < rem && rem <= above + here) { sc.bin = threadIdx.x; sc.rem = rem - above; }
    }
    __syncthreads();
    prefix |= (uint64_t)sc.bin << shift;
    mask |= (uint64_t)255 << shift;
    rem = sc.rem;
  }
  return prefix;
}

__device__ __forceinline__ bool cand_before(double sa, uint32_t ia, double sb, uint32_t ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// LDS bitonic sort by (score desc, index asc); n a power of two
__device__ void bitonic_cand(double* s, uint32_t* id, int n) {
  for (int k2 = 2; k2 <= n; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int p = i ^ j;
        if (p > i) {
          const double x = s[i], y = s[p];
          const uint32_t ix = id[i], iy = id[p];
          const bool fwd = (i & k2) == 0;
          const bool sw = fwd ? cand_before(y, iy, x, ix) : cand_before(x, ix, y, iy);
          if (sw) { s[i] = y; s[p] = x; id[i] = iy; id[p] = ix; }
        }
      }
      __syncthreads();
    }
}

// tau[q] = r-th largest of T[0..nvals) for query q (column q of T, leading dim nq_pad)
__global__ void __launch_bounds__(1024) k_tau_select(const float* __restrict__ T, int64_t nvals, int nq_pad, int r,
                                                     float* __restrict__ tau) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ SelectScratch sc;
  uint32_t* key = (uint32_t*)smem;
  const int q = blockIdx.x;
  for (int i = threadIdx.x; i < nvals; i += blockDim.x) key[i] = f32_order_key(T[(int64_t)i * nq_pad + q]);
  __syncthreads();
  if (r < 1 || r > nvals) {
    if (threadIdx.x == 0) tau[q] = -INFINITY;
    return;
  }
  const uint32_t kk = (uint32_t)block_kth_largest<32>([&](int i) { return (uint64_t)key[i]; }, (int)nvals, (uint32_t)r, sc);
  if (threadIdx.x == 0) tau[q] = f32_from_order_key(kk);
}

}  // namespace convdr

// the certificate, one copy of each piece: error band, verdicts, canonical fp64 score, exact top-k of a band in LDS
#include "ip_certify.hpp"

namespace convdr {

// ------------------------------------------------------------------------------------------
// band cut: which candidates must be re-scored exactly?
// Let s~(k) be the k-th best bf16-pass score of the query and eps its error bound
// (|s~ - exact| <= eps for every passage of the block).  The k best by s~ all have exact >= s~(k) - eps,
// so the true k-th exact score t_k >= s~(k) - eps.  A passage with s~ < cut := s~(k) - 2 eps has
// exact < s~(k) - eps <= t_k and cannot be in the true top-k.  Hence re-scoring exactly the band
// {s~ >= cut} yields the exact top-k, PROVIDED the candidate list is complete down to cut, i.e.
// cut >= tau and the list did not overflow.  Otherwise the query is flagged for a retry with a
// threshold that makes the next pass complete.
// Moves the band to the front of the query's candidate list (in no particular order: k_ip_select orders the
// re-scored band by (exact score, index), which does not depend on it) and writes m[q] = band size.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_ip_cut(int64_t n, int k, int cap, const uint32_t* __restrict__ counts,
                                                uint32_t* __restrict__ counts_packed,
                                                uint32_t* __restrict__ cand_id, float* __restrict__ cand_s,
                                                const float* __restrict__ tau, const IpBand band,
                                                uint32_t* __restrict__ m_out, int32_t* __restrict__ status,
                                                float* __restrict__ tau_retry) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ SelectScratch sc;
  __shared__ uint32_t sh_m;
  const int q = blockIdx.x;
  const uint32_t cnt = ip_hits(counts, q);
  if (threadIdx.x == 0) counts_packed[q] = cnt;   // [nq] copy for convdr_ip_debug_counts
  const int c = cnt < (uint32_t)cap ? (int)cnt : cap;
  uint32_t* key = (uint32_t*)smem;
  uint32_t* id = (uint32_t*)(smem + (size_t)cap * 4);
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    key[i] = f32_order_key(cand_s[(int64_t)q * cap + i]);
    id[i] = cand_id[(int64_t)q * cap + i];
  }
  if (threadIdx.x == 0) sh_m = 0;
  __syncthreads();
  const int need = (int64_t)k < n ? k : (int)n;
  const float t = tau[q];
  const float eps = band.eps(q);
  const bool out_of_range = band.out_of_range(q);
  const bool have_k = need > 0 && c >= need;
  float cut = -INFINITY;
  if (have_k)
    cut = f32_from_order_key((uint32_t)block_kth_largest<32>([&](int i) { return (uint64_t)key[i]; }, c, (uint32_t)need, sc)) -
          2.f * eps;
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    const float v = f32_from_order_key(key[i]);
    if (v >= cut) {
      const uint32_t slot = atomicAdd(&sh_m, 1u);
      cand_id[(int64_t)q * cap + slot] = id[i];
      cand_s[(int64_t)q * cap + slot] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const IpVerdict v = ip_topk_verdict(cnt, cap, c, need, t, cut, eps, out_of_range);
    m_out[q] = sh_m;
    status[q] = v.status;
    tau_retry[q] = v.retry;
  }
}

// exact rescoring of a band in global memory: one wave per candidate, the canonical fp64 score (ip_row_score)
template <class PT>
__global__ void __launch_bounds__(256) k_ip_rescore(const float* __restrict__ Q, typename IpRows<PT>::type P, int d,
                                                    int cap, const uint32_t* __restrict__ m_in,
                                                    const uint32_t* __restrict__ cand_id,
                                                    double* __restrict__ cand_x, double unscale) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t c = m_in[q];
  const float* qv = Q + (int64_t)q * d;
  for (uint32_t slot = blockIdx.y * 4 + wave; slot < c; slot += gridDim.y * 4) {
    const uint32_t id = cand_id[(int64_t)q * cap + slot];
    const double acc = ip_row_score<PT>(qv, ip_row_at(P, (int64_t)id, d), d, lane, unscale);
    if (lane == 0) cand_x[(int64_t)q * cap + slot] = acc;
  }
}

// per-query top-k of the re-scored band in global memory, cap <= 8192: staged into LDS, then ip_band_topk_lds
__global__ void __launch_bounds__(IP_SELECT_THREADS) k_ip_select(int k, int cap, const uint32_t* __restrict__ m_in,
                                                                 const uint32_t* __restrict__ cand_id,
                                                                 const double* __restrict__ cand_x,
                                                                 float* __restrict__ D, int64_t* __restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ SelectScratch sc;
  __shared__ uint32_t sh_g;
  const int q = blockIdx.x;
  const int c = (int)m_in[q];
  double* s = (double*)smem;
  uint32_t* id = (uint32_t*)(smem + (size_t)cap * 8);
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    s[i] = cand_x[(int64_t)q * cap + i];
    id[i] = cand_id[(int64_t)q * cap + i];
  }
  if (threadIdx.x == 0) sh_g = 0;
  __syncthreads();
  ip_band_topk_lds(s, id, c, k, q, sc, sh_g, D, I);
}

// ------------------------------------------------------------------------------------------
// Round 5: cut + re-score + select of ONE query in ONE workgroup (k_ip_cut, k_ip_rescore and k_ip_select chained three
// launches per search with the band making a round trip through HBM between them; at 100 queries the three were 39 us of
// kernel time plus their boundaries around a 290 us scan).  Same arithmetic, phase by phase:
//   1. the query's candidate list into LDS, radix select of S~(k), cut = S~(k) - 2 eps, certificate (status, retry
//      threshold), the band compacted IN LDS (ids);
//   2. canonical fp64 re-score of the band: one wave per candidate, sixteen waves per query, each wave's next candidate's
//      loads in flight while it folds the current one (the same lane / butterfly order as k_ip_rescore: bit-identical);
//   3. radix select of the k-th exact score on the high key word, bitonic sort of the survivors, D / I written.
// LDS: cap x (4 id + 4 key) for phase 1, the key half reused with the id half's neighbour as cap x 8 scores from phase 2 on
// -> cap x 16 bytes (64 KB at the default cap of 4096: two workgroups per CU).  The per-query band size and packed candidate
// count are still written (convdr_ip_debug_*).  convdr_set_option("ip_fused_finish", 0) gives the three launches back.
// ------------------------------------------------------------------------------------------
template <class PT>
__global__ void __launch_bounds__(IP_SELECT_THREADS) k_ip_finish(int64_t n, int k, int cap, const uint32_t* __restrict__ counts,
                                                   uint32_t* __restrict__ counts_packed,
                                                   const uint32_t* __restrict__ cand_id, const float* __restrict__ cand_s,
                                                   const float* __restrict__ tau, const IpBand band,
                                                   const float* __restrict__ Q, typename IpRows<PT>::type P, int d,
                                                   uint32_t* __restrict__ m_out, int32_t* __restrict__ status, float* __restrict__ tau_retry,
                                                   float* __restrict__ D, int64_t* __restrict__ I, double unscale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ SelectScratch sc;
  __shared__ uint32_t sh_m, sh_g;
  const int q = blockIdx.x;
  const uint32_t cnt = ip_hits(counts, q);
  if (threadIdx.x == 0) counts_packed[q] = cnt;
  const int c = cnt < (uint32_t)cap ? (int)cnt : cap;
  double* sx = (double*)smem;                                   // [cap] exact scores (phases 2, 3)
  uint32_t* key = (uint32_t*)smem;                              // [cap] order keys of the scan scores (phase 1; dead before sx is written)
  uint32_t* id = (uint32_t*)(smem + (size_t)cap * 8);           // [cap] candidate ids, then the band's ids
  uint32_t* bid = (uint32_t*)(smem + (size_t)cap * 12);         // [cap] the band, compacted
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    key[i] = f32_order_key(cand_s[(int64_t)q * cap + i]);
    id[i] = cand_id[(int64_t)q * cap + i];
  }
  if (threadIdx.x == 0) { sh_m = 0; sh_g = 0; }
  __syncthreads();
  // ---- phase 1: cut (k_ip_cut: the proof is above it) ----
  const int need = (int64_t)k < n ? k : (int)n;
  const float t = tau[q];
  const float eps = band.eps(q);
  const bool out_of_range = band.out_of_range(q);
  const bool have_k = need > 0 && c >= need;
  float cut = -INFINITY;
  if (have_k)
    cut = f32_from_order_key((uint32_t)block_kth_largest<32>([&](int i) { return (uint64_t)key[i]; }, c, (uint32_t)need, sc)) -
          2.f * eps;
  for (int i = threadIdx.x; i < c; i += blockDim.x)
    if (f32_from_order_key(key[i]) >= cut) bid[atomicAdd(&sh_m, 1u)] = id[i];
  __syncthreads();
  const int m = (int)sh_m;
  if (threadIdx.x == 0) {
    const IpVerdict v = ip_topk_verdict(cnt, cap, c, need, t, cut, eps, out_of_range);
    m_out[q] = (uint32_t)m;
    status[q] = v.status;
    tau_retry[q] = v.retry;
  }
  // ---- phase 2: canonical fp64 re-score (k_ip_rescore), one wave per band candidate ----
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float* qv = Q + (int64_t)q * d;
    for (int slot = wave; slot < m; slot += nw) {
      const double acc = ip_row_score<PT>(qv, ip_row_at(P, (int64_t)bid[slot], d), d, lane, unscale);
      if (lane == 0) sx[slot] = acc;     // (key[] is dead: every thread passed the barrier after the compaction)
    }
  }
  __syncthreads();
  // ---- phase 3: exact top-k of the band (k_ip_select); id[] now holds the band ----
  for (int i = threadIdx.x; i < m; i += blockDim.x) id[i] = bid[i];
  __syncthreads();
  ip_band_topk_lds(sx, id, m, k, q, sc, sh_g, D, I);
}

int64_t g_ip_fused_finish = 1;   // convdr_set_option("ip_fused_finish"): 1 = k_ip_finish, 0 = k_ip_cut + k_ip_rescore + k_ip_select

}  // namespace convdr
