// Prototype (NOT product): the product R3 K step of a 256 x 256 tile (3 R slots + 2 L slots, LDS-DMA by role, counted vmcnt,
// one barrier per step: gemm_nt_mainloop_r3 itself, called as k_gemm calls it) against the SAME staging with the wave's
// 128 x 64 tile computed by v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_32x32x16_bf16, at the FFN1 shape
// (262,144 x 768 x 3,072), persistent over 256 workgroups in k_gemm's tile order, next tile's prologue issued when the main
// loop returns, no epilogue.  Question: the chip runs these GEMMs power-capped at ~1.7 GHz of 2.4; does it hold a higher
// clock on the 16x16x32 shape at the same output tile per wave and the same LDS bytes, and does that show as wall time?
//
// The LDS image is unchanged.  A 16x16x32 operand fragment is row (lane & 15), 16-byte k-chunk 4 s2 + (lane >> 4) of the
// K = 32 sub-step s2; with the image's chunk swizzle c ^ ((row >> 1) & 7) sixteen lanes cover sixteen distinct 16-byte slots
// of 256 B.  Per sub-step: 8 R fragments, 4 L fragments, 32 MFMAs walked i-major; an R fragment is re-read for the next
// sub-step as soon as its 4 MFMAs have issued (one register set of R fragments, two of L: 64 fragment VGPRs).  That loop is
// gemm_nt_mainloop_r3_m16 of gemm_nt.hpp: it was written here, measured (profiles/mfma16_proto.txt: GO) and moved there.
//
// Both bodies run as interleaved rounds in ONE process on random operands; wall per K step (hipEvent) and the in-kernel
// clock (s_memtime / s_memrealtime stamps of every workgroup, written to a buffer nothing else reads) are reported per
// round, then median / min / spread per body.  `verify` first checks both bodies against each other and a host reference
// on a small ragged problem.
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I convdr_amd/csrc tools/proto/mfma16_proto.hip -o tools/proto/bin/mfma16_proto
// Run:    tools/proto/bin/mfma16_proto [rounds = 8] [launches per round = 300]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gemm_nt.hpp"

using namespace convdr;

struct Args {
  const bf16_t* W; const bf16_t* X;
  float* Y;                     // [workgroups * 512] sink
  float* C;                     // VERIFY: [rows, N] fp32
  int64_t rows; int N, K; int tilesN, tilesT;
  unsigned long long* stamps;   // [workgroups][4]: s_memtime, s_memrealtime at the start and the end of the workgroup
};

using T = Tile256;

// SHAPE 0: 32x32x16 (gemm_nt_mainloop_r3, the product loop), 1: 16x16x32
template <int SHAPE, bool VERIFY>
__global__ void __launch_bounds__(T::THREADS, 2) k_proto(const Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WavePos<T> w;
  // k_gemm's tile walk
  const uint32_t ntiles = (uint32_t)a.tilesN * a.tilesT;
  const uint32_t xcd = blockIdx.x & 7u, q8 = ntiles >> 3, r8 = ntiles & 7u;
  const uint32_t chunk_base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const uint32_t chunk_len = q8 + (xcd < r8 ? 1u : 0u);
  const uint32_t stride = (gridDim.x + 7u) >> 3;
  uint32_t idx = blockIdx.x >> 3;
  if (idx >= chunk_len) return;
  if (threadIdx.x == 0) {
    a.stamps[blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime();
    a.stamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime();
  }
  struct Coord { int64_t t0; int n0; };
  auto decode = [&](uint32_t i) {
    const uint32_t logical = chunk_base + i;
    const int tt = logical / a.tilesN, tn = logical - tt * a.tilesN;
    return Coord{(int64_t)tt * T::TL, tn * T::TR};
  };
  auto src_of = [&](const Coord& c) { return TileSrcAll<T>(a.W, a.K, a.N, a.X, a.K, a.rows, c.n0, c.t0, w); };
  R3Slots st{0, 0};
  Coord c = decode(idx);
  TileSrcAll<T> src = src_of(c);
  gemm_r3_prologue<T>(src, a.K, smem, w, st, false);
  __syncthreads();
  float sink = 0.f;
  for (;;) {
    const uint32_t next = idx + stride;
    const bool has_next = next < chunk_len;
    const Coord cn = has_next ? decode(next) : c;
    if constexpr (SHAPE == 0) {
      GemmAcc<T> acc;
      acc.zero();
      st = gemm_nt_mainloop_r3<T>(src, a.K, smem, acc, w, st, true, true, false);
      if (has_next) { src = src_of(cn); gemm_r3_prologue<T>(src, a.K, smem, w, st, false); }
#pragma unroll
      for (int i = 0; i < T::MT; ++i)
#pragma unroll
        for (int j = 0; j < T::NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (VERIFY) {
              const int64_t t = c.t0 + w.l_index(j);
              const int f = c.n0 + w.r_index(i, r);
              if (t < a.rows && f < a.N) a.C[t * a.N + f] = acc.c[i][j][r];
            } else sink += acc.c[i][j][r];
          }
    } else {
      GemmAcc16<T> acc;
      acc.zero();
      st = gemm_nt_mainloop_r3_m16<T>(src, a.K, smem, acc, w, st, true, true, false);
      if (has_next) { src = src_of(cn); gemm_r3_prologue<T>(src, a.K, smem, w, st, false); }
#pragma unroll
      for (int i = 0; i < 2 * T::MT; ++i)
#pragma unroll
        for (int j = 0; j < 2 * T::NT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (VERIFY) {
              const int64_t t = c.t0 + w.wl * T::NT * 32 + 16 * j + (w.lane & 15);
              const int f = c.n0 + w.wr * T::MT * 32 + 16 * i + 4 * (w.lane >> 4) + r;
              if (t < a.rows && f < a.N) a.C[t * a.N + f] = acc.c[i][j][r];
            } else sink += acc.c[i][j][r];
          }
    }
    if (!has_next) break;
    idx = next;
    c = cn;
  }
  if (threadIdx.x == 0) {
    a.stamps[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memtime();
    a.stamps[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
  }
  if constexpr (!VERIFY) a.Y[(size_t)blockIdx.x * T::THREADS + threadIdx.x] = sink;
}

#define CHECK(e)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (e);                                                               \
    if (e_ != hipSuccess) {                                                            \
      printf("%s failed: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__);        \
      exit(2);                                                                         \
    }                                                                                  \
  } while (0)

constexpr int SMEM = 3 * T::R_BYTES + 2 * T::L_BYTES;
static int g_grid = 256;

template <class F>
static void launch(F fn, const Args& a) { hipLaunchKernelGGL(fn, dim3(g_grid), dim3(T::THREADS), SMEM, 0, a); }

static float bf16_host(bf16_t v) { uint32_t u = (uint32_t)v << 16; float f; memcpy(&f, &u, 4); return f; }

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.size() & 1 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]); }

struct Round { double ms, ticks_per_step, clock_mhz; };

template <class F>
static Round timed_round(F fn, const Args& a, int launches, int steps_per_wg) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < launches; ++i) launch(fn, a);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  float ms = 0;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0); hipEventDestroy(e1);
  std::vector<unsigned long long> s((size_t)g_grid * 4);
  CHECK(hipMemcpy(s.data(), a.stamps, s.size() * 8, hipMemcpyDeviceToHost));   // the round's last launch
  std::vector<double> ticks, mhz;
  for (int b = 0; b < g_grid; ++b) {
    const double dt = (double)(s[b * 4 + 2] - s[b * 4 + 0]), dr = (double)(s[b * 4 + 3] - s[b * 4 + 1]);
    ticks.push_back(dt / steps_per_wg);
    if (dr > 0) mhz.push_back(dt / dr * 100.0);
  }
  return Round{ms / launches, median(ticks), median(mhz)};
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 8;
  const int launches = argc > 2 ? atoi(argv[2]) : 300;
  const int64_t rows = 262144;
  const int N = 3072, K = 768;
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  g_grid = prop.multiProcessorCount / 8 * 8;
  if (g_grid > 256) g_grid = 256;   // (stamp / sink buffers are sized for 256)
  printf("# device %s, %d CUs, grid %d workgroups of %d threads, %d B LDS\n", prop.name, prop.multiProcessorCount, g_grid, T::THREADS, SMEM);

  bf16_t *W, *X;
  float *Y, *C0, *C1;
  unsigned long long* stamps;
  const int64_t vrows = 1000;   // verify: 4 token tiles, the last one ragged (232 live rows, not a multiple of 16)
  CHECK(hipMalloc(&W, (size_t)N * K * 2)); CHECK(hipMalloc(&X, (size_t)rows * K * 2));
  CHECK(hipMalloc(&Y, (size_t)256 * T::THREADS * 4)); CHECK(hipMalloc(&stamps, 256 * 4 * 8));
  CHECK(hipMalloc(&C0, (size_t)vrows * N * 4)); CHECK(hipMalloc(&C1, (size_t)vrows * N * 4));
  CHECK(hipMemset(stamps, 0, 256 * 4 * 8));
  std::vector<bf16_t> hx((size_t)rows * K), hw((size_t)N * K);
  uint64_t sd = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (uint32_t)(sd >> 24); };
  // random sign, four exponents and all 7 mantissa bits: |v| in [0.25, 4)
  auto rbf = [&]() { const uint32_t r = rnd(); return (bf16_t)(0x3e80 + (r & 0x1ff) + ((r >> 9 & 1) << 15)); };
  for (auto& v : hx) v = rbf();
  for (auto& v : hw) v = rbf();
  CHECK(hipMemcpy(X, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(W, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
  for (void* fn : {(void*)k_proto<0, false>, (void*)k_proto<1, false>, (void*)k_proto<0, true>, (void*)k_proto<1, true>}) {
    CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
    hipFuncAttributes fa;
    CHECK(hipFuncGetAttributes(&fa, fn));
    printf("# kernel regs %d  scratch %zu B  static LDS %zu B\n", fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes);
  }

  // ---- verify: both bodies on [1000, 768] x [3072, 768]^T against each other and a host reference -------------------------
  {
    Args v{W, X, Y, C0, vrows, N, K, N / T::TR, (int)((vrows + T::TL - 1) / T::TL), stamps};
    CHECK(hipMemset(C0, 0xff, (size_t)vrows * N * 4)); CHECK(hipMemset(C1, 0xff, (size_t)vrows * N * 4));
    launch(k_proto<0, true>, v);
    v.C = C1;
    launch(k_proto<1, true>, v);
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
    std::vector<float> c0((size_t)vrows * N), c1((size_t)vrows * N);
    CHECK(hipMemcpy(c0.data(), C0, c0.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(c1.data(), C1, c1.size() * 4, hipMemcpyDeviceToHost));
    double dmax = 0, rmax0 = 0, rmax1 = 0, scale = 0;
    size_t bad = 0;
    for (size_t i = 0; i < c0.size(); ++i) {
      if (!(std::isfinite(c0[i]) && std::isfinite(c1[i]))) { ++bad; continue; }
      dmax = std::max(dmax, (double)std::fabs(c0[i] - c1[i]));
    }
    for (int smp = 0; smp < 4096; ++smp) {
      const int64_t t = smp < 64 ? vrows - 1 - smp : rnd() % vrows;
      const int f = rnd() % N;
      double ref = 0, mag = 0;
      for (int k = 0; k < K; ++k) { const double p = (double)bf16_host(hx[t * K + k]) * bf16_host(hw[(size_t)f * K + k]); ref += p; mag += std::fabs(p); }
      rmax0 = std::max(rmax0, std::fabs(c0[t * N + f] - ref));
      rmax1 = std::max(rmax1, std::fabs(c1[t * N + f] - ref));
      scale = std::max(scale, mag);
    }
    // fp32 accumulation of K = 768 exact bf16 products: |error| <= K * 2^-24 * sum |products| (a loose, reasoned bound)
    const double bound = K * std::ldexp(1.0, -24) * scale;
    printf("# verify: non-finite / unwritten %zu, max |32x32x16 - 16x16x32| %.3g, max |body - fp64 host| %.3g / %.3g (bound %.3g)\n",
           bad, dmax, rmax0, rmax1, bound);
    if (bad || rmax0 > bound || rmax1 > bound) { printf("VERIFY FAILED\n"); return 1; }
  }

  // ---- timing ---------------------------------------------------------------------------------------------------------------
  Args a{W, X, Y, nullptr, rows, N, K, N / T::TR, (int)(rows / T::TL), stamps};
  const int steps_per_wg = (int)((int64_t)a.tilesN * a.tilesT / g_grid) * (K / GEMM_BK);
  printf("# FFN1 shape %lld x %d x %d, %d tiles, %d K steps per workgroup, %d rounds per body of %d launches, order A B B A ...\n",
         (long long)rows, K, N, a.tilesN * a.tilesT, steps_per_wg, rounds, launches);
  // warm-up: > 2 s of back-to-back launches so that the clock has settled under load
  for (int i = 0; i < 1200; ++i) { launch(k_proto<0, false>, a); launch(k_proto<1, false>, a); }
  CHECK(hipDeviceSynchronize());
  std::vector<Round> res[2];
  printf("# round body        ms/launch  us/Kstep(wall)  ticks/Kstep  clock MHz   TFLOP/s\n");
  for (int r = 0; r < 2 * rounds; ++r) {
    const int body = ((r + 1) >> 1) & 1;   // A B B A A B B A ...
    const Round x = body ? timed_round(k_proto<1, false>, a, launches, steps_per_wg) : timed_round(k_proto<0, false>, a, launches, steps_per_wg);
    res[body].push_back(x);
    printf("%5d  %s  %9.4f  %13.4f  %11.1f  %9.0f  %8.0f\n", r, body ? "16x16x32" : "32x32x16", x.ms, x.ms * 1e3 / steps_per_wg,
           x.ticks_per_step, x.clock_mhz, 2.0 * rows * N * K / x.ms / 1e9);
    fflush(stdout);
  }
  double med[2], mn[2], mx[2];
  for (int b = 0; b < 2; ++b) {
    std::vector<double> ms, tk, ck;
    for (auto& x : res[b]) { ms.push_back(x.ms); tk.push_back(x.ticks_per_step); ck.push_back(x.clock_mhz); }
    med[b] = median(ms); mn[b] = *std::min_element(ms.begin(), ms.end()); mx[b] = *std::max_element(ms.begin(), ms.end());
    printf("# %s: wall per K step median %.4f us  min %.4f us  (ms/launch median %.4f min %.4f max %.4f, spread %.4f) | ticks/Kstep median %.1f | clock median %.0f MHz\n",
           b ? "16x16x32" : "32x32x16", med[b] * 1e3 / steps_per_wg, mn[b] * 1e3 / steps_per_wg, med[b], mn[b], mx[b], mx[b] - mn[b],
           median(tk), median(ck));
  }
  const double gain = med[0] - med[1], spread = mx[0] - mn[0];
  printf("# 16x16x32 against 32x32x16 by median wall: %+.4f ms per launch (%+.2f %%); spread of the 32x32x16 rounds %.4f ms; rule: gain > 3 x spread -> %s\n",
         -gain, -100.0 * gain / med[0], spread, gain > 3 * spread ? "GO" : "NO-GO");
  return 0;
}
