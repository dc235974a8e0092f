// Prototype (NOT product): the main loop of k_gemm_resid_ln (gemm_ln.hpp: three 48 KB weight slots + two 8 KB activation
// slots, LDS-DMA by role -- LN_W_WAVES / LN_A_WAVES --, counted vmcnt, one lds_barrier per 32-wide K slice, K-slice-major
// weights, blocked activations) against the SAME staging with the wave's 192 x 64 tile computed by v_mfma_f32_16x16x32_bf16
// (ln_mainloop_m16 of gemm_ln.hpp, LDS image swizzled by ln16_swz), at the FFN2 shape (262,144 x 3,072 -> 768) and the
// attention-output shape (K = 768): 2,048 workgroups of 128 tokens, one per CU at a time, no epilogue.  Question, as in
// mfma16_proto.hip: does the higher clock the chip holds on the 16x16x32 shape show as wall time in THIS kernel's K step?
//
// Bodies: 0 = the 32x32x16 loop (a copy of k_gemm_resid_ln's, rolling fragment prefetch included), 1 = ln_mainloop_m16<0>
// (6 reads before the first MFMA), 2 = ln_mainloop_m16<1> (units 0 / 1 split over the token blocks, still 6 reads ahead),
// 3 = ln_mainloop_m16<2> (the same with the fragments of token blocks 2-3 read behind the first two MFMAs: 4 reads ahead).
// All bodies run as interleaved rounds A B C D D C B A ... in ONE process on random operands; wall per K step (hipEvent) and the
// in-kernel clock (s_memtime / s_memrealtime stamps of every workgroup, written to a buffer nothing else reads) are reported
// per round, then median / min / max per body.  `verify` first checks the bodies against each other and a host reference on a
// small ragged problem at both K.
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I convdr_amd/csrc tools/proto/ln_mfma16_proto.hip -o tools/proto/bin/ln_mfma16_proto
// Run:    tools/proto/bin/ln_mfma16_proto [cycles of A B C D D C B A = 2] [launches per round = 100]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gemm_ln.hpp"

using namespace convdr;

struct Args {
  GemmLnArgs g;                 // Wks, A (blocked), rows, K are used
  float* Y;                     // [workgroups * 512] sink
  float* C;                     // VERIFY: [rows, 768] fp32
  unsigned long long* stamps;   // [min(workgroups, 2048)][4]: s_memtime, s_memrealtime at the start and the end of the workgroup
};

using T = TileLN;

template <int BODY, bool VERIFY>
__global__ void __launch_bounds__(512, 2) k_proto(const Args p) {
  const GemmLnArgs& a = p.g;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WavePos<T> w;
  const int64_t t0 = (int64_t)blockIdx.x * T::TL;
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    p.stamps[blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime();
    p.stamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime();
  }
  const int nk = a.K / LN_SLICE;
  float sink = 0.f;
  if constexpr (BODY == 0) {
    // ---- k_gemm_resid_ln, from its first line to the end of its main loop (trace stamps removed) ----
    char* sW = smem;
    char* sA = smem + 3 * LN_R_BYTES;
    GemmAcc<T> acc;
    acc.zero();
    const int sw = (w.li >> 2) & 3;
    const int offR = (w.wr * T::MT * 32 + w.li) * 64;
    const int offL = (w.wl * T::NT * 32 + w.li) * 64;
    StageSrc srcW = a.Wks ? ln_stage_src<LN_W_WAVES, LN_W_FIRST>(a.Wks, LN_SLICE, 0, (int64_t)T::TR * (a.K / LN_SLICE), w.wave, w.lane)
                          : ln_stage_src<LN_W_WAVES, LN_W_FIRST>(a.W, a.K, 0, T::TR, w.wave, w.lane);
    const uint32_t w_slice_stride = a.Wks ? T::TR * LN_SLICE * 2 : LN_SLICE * 2;
    StageSrc srcA = ln_stage_src<LN_A_WAVES, LN_A_FIRST>(a.A, a.K, t0, a.rows, w.wave, w.lane);
    uint32_t a_slice_stride = LN_SLICE * 2;
    if (a.a_blocked) {
      const int64_t rows32 = (a.rows + 31) & ~(int64_t)31;
      const int64_t blk_elems = (int64_t)(a.K >> 3) * 256;
      int64_t bytes = (rows32 - t0) / 32 * blk_elems * 2;
      bytes = bytes < 0 ? 0 : (bytes > 0xffffffffll ? 0xffffffffll : bytes);
      const uint64_t base = (uint64_t)(a.A + (t0 >> 5) * blk_elems);
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
      const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
      const uint32_t nb = __builtin_amdgcn_readfirstlane((uint32_t)bytes);
      srcA.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
      const int wv = w.wave >= LN_A_FIRST ? w.wave - LN_A_FIRST : 0;
      const int row = wv * 16 + (w.lane >> 2);
      const int gch = (w.lane & 3) ^ ((row >> 2) & 3);
      srcA.voff = (uint32_t)((row >> 5) * blk_elems * 2 + gch * 512 + (row & 31) * 16);
      srcA.round_pitch = __builtin_amdgcn_readfirstlane((uint32_t)((16 * LN_A_WAVES / 32) * blk_elems * 2));
      a_slice_stride = 4 * 512;
    }
    constexpr int LN_W_DPW = T::TR / (16 * LN_W_WAVES);
    const bool w_wave = w.wave >= LN_W_FIRST && w.wave < LN_W_FIRST + LN_W_WAVES;
    ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(srcW, 0, sW, w.wave, w_slice_stride);
    ln_stage32<T::TL, LN_A_WAVES, LN_A_FIRST, LN_A_AUX>(srcA, 0, sA, w.wave, a_slice_stride);
    if (nk > 1) ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(srcW, 1, sW + LN_R_BYTES, w.wave, w_slice_stride);
    int wslot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk && w_wave) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LN_W_DPW) : "memory");
      else lds_dma_wait_all();
      lds_barrier();
      if (kt + 1 < nk) ln_stage32<T::TL, LN_A_WAVES, LN_A_FIRST, LN_A_AUX>(srcA, kt + 1, sA + ((kt + 1) & 1) * LN_L_BYTES, w.wave, a_slice_stride);
      const bool issue_w = kt + 2 < nk;
      char* w_dst = sW + (wslot == 0 ? 2 : wslot - 1) * LN_R_BYTES;
      const char* tR = sW + wslot * LN_R_BYTES + offR;
      const char* tL = sA + (kt & 1) * LN_L_BYTES + offL;
      wslot = wslot == 2 ? 0 : wslot + 1;
      {
        constexpr int UNITS = 2 * T::MT;
        const int ch0 = ((0 + w.hi) ^ sw) * 16, ch1 = ((2 + w.hi) ^ sw) * 16;
        bf16x8 fb[2][T::NT], fa[3];
        auto load_a = [&](int u) { fa[u % 3] = *(const bf16x8*)(tR + (u % T::MT) * 32 * 64 + (u < T::MT ? ch0 : ch1)); };
#pragma unroll
        for (int j = 0; j < T::NT; ++j) fb[0][j] = *(const bf16x8*)(tL + j * 32 * 64 + ch0);
        load_a(0);
        load_a(1);
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
          if (u + 2 < UNITS) load_a(u + 2);
          if (u == 2) {
#pragma unroll
            for (int j = 0; j < T::NT; ++j) fb[1][j] = *(const bf16x8*)(tL + j * 32 * 64 + ch1);
          }
#pragma unroll
          for (int j = 0; j < T::NT; ++j)
            acc.c[u % T::MT][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[u % 3], fb[u / T::MT][j], acc.c[u % T::MT][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, T::NT + 2, 0);
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
          if (u + 2 < UNITS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (u == 2) __builtin_amdgcn_sched_group_barrier(0x100, T::NT, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, T::NT, 0);
        }
      }
      if (issue_w) ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(srcW, kt + 2, w_dst, w.wave, w_slice_stride);
    }
#pragma unroll
    for (int i = 0; i < T::MT; ++i)
#pragma unroll
      for (int j = 0; j < T::NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if constexpr (VERIFY) {
            const int64_t t = t0 + w.l_index(j);
            const int f = w.r_index(i, r);
            if (t < a.rows) p.C[t * T::TR + f] = acc.c[i][j][r];
          } else sink += acc.c[i][j][r];
        }
  } else {
    GemmAcc16<T> acc;
    acc.zero();
    const Ln16Src s = ln16_sources(a, t0, w);
    ln_mainloop_m16<BODY - 1>(s, nk, smem, acc, w);
#pragma unroll
    for (int i = 0; i < 2 * T::MT; ++i)
#pragma unroll
      for (int j = 0; j < 2 * T::NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (VERIFY) {
            const int64_t t = t0 + w.wl * T::NT * 32 + 16 * j + (w.lane & 15);
            const int f = w.wr * T::MT * 32 + 16 * i + 4 * (w.lane >> 4) + r;
            if (t < a.rows) p.C[t * T::TR + f] = acc.c[i][j][r];
          } else sink += acc.c[i][j][r];
        }
  }
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    p.stamps[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memtime();
    p.stamps[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
  }
  if constexpr (!VERIFY) p.Y[(size_t)blockIdx.x * 512 + threadIdx.x] = sink;
}

// random sign, four exponents and all 7 mantissa bits: |v| in [0.25, 4)
__global__ void k_fill(bf16_t* p, size_t n, uint64_t seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t x = (i + seed) * 0x9e3779b97f4a7c15ull;
    x ^= x >> 29; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 32;
    const uint32_t r = (uint32_t)x;
    p[i] = (bf16_t)(0x3e80 + (r & 0x1ff) + ((r >> 9 & 1) << 15));
  }
}

#define CHECK(e)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (e);                                                               \
    if (e_ != hipSuccess) {                                                            \
      printf("%s failed: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__);        \
      exit(2);                                                                         \
    }                                                                                  \
  } while (0)

constexpr int NBODY = 4;
static const char* BODY_NAME[NBODY] = {"32x32x16   ", "16x16x32/6 ", "16x16x32/6s", "16x16x32/4s"};

static void launch(int body, bool verify, const Args& a) {
  const dim3 grid((unsigned)((a.g.rows + T::TL - 1) / T::TL)), block(512);
#define L_(B, V) hipLaunchKernelGGL((k_proto<B, V>), grid, block, LN_SMEM_BYTES, 0, a)
  if (verify) { if (body == 0) L_(0, true); else if (body == 1) L_(1, true); else if (body == 2) L_(2, true); else L_(3, true); }
  else { if (body == 0) L_(0, false); else if (body == 1) L_(1, false); else if (body == 2) L_(2, false); else L_(3, false); }
#undef L_
}

static float bf16_host(bf16_t v) { uint32_t u = (uint32_t)v << 16; float f; memcpy(&f, &u, 4); return f; }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.size() & 1 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]); }

struct Round { double ms, ticks_per_step, clock_mhz; };

static Round timed_round(int body, const Args& a, int launches) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < launches; ++i) launch(body, false, a);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  float ms = 0;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  const int wgs = 2048;
  std::vector<unsigned long long> s((size_t)wgs * 4);
  CHECK(hipMemcpy(s.data(), a.stamps, s.size() * 8, hipMemcpyDeviceToHost));   // the round's last launch
  std::vector<double> ticks, mhz;
  for (int b = 0; b < wgs; ++b) {
    const double dt = (double)(s[b * 4 + 2] - s[b * 4 + 0]), dr = (double)(s[b * 4 + 3] - s[b * 4 + 1]);
    ticks.push_back(dt / (a.g.K / LN_SLICE));
    if (dr > 0) mhz.push_back(dt / dr * 100.0);
  }
  return Round{ms / launches, median(ticks), median(mhz)};
}

int main(int argc, char** argv) {
  const int cycles = argc > 1 ? atoi(argv[1]) : 2;
  const int launches = argc > 2 ? atoi(argv[2]) : 100;
  const int64_t rows = 262144;
  const int KMAX = 3072;
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("# device %s, %d CUs, %lld workgroups of 512 threads (128 tokens x 768 features), %d B LDS\n", prop.name,
         prop.multiProcessorCount, (long long)(rows / T::TL), LN_SMEM_BYTES);

  bf16_t *W, *X;
  float *Y, *C[NBODY];
  unsigned long long* stamps;
  const int64_t vrows = 1000;   // verify: 8 token tiles, the last one ragged (104 live rows, not a multiple of 16)
  CHECK(hipMalloc(&W, (size_t)T::TR * KMAX * 2)); CHECK(hipMalloc(&X, (size_t)rows * KMAX * 2));
  CHECK(hipMalloc(&Y, (size_t)2048 * 512 * 4)); CHECK(hipMalloc(&stamps, 2048 * 4 * 8));
  for (auto& c : C) CHECK(hipMalloc(&c, (size_t)vrows * T::TR * 4));
  CHECK(hipMemset(stamps, 0, 2048 * 4 * 8));
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, X, (size_t)rows * KMAX, 1ull);
  hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, 0, W, (size_t)T::TR * KMAX, 0x51ull << 40);
  CHECK(hipDeviceSynchronize());
  for (void* fn : {(void*)k_proto<0, false>, (void*)k_proto<1, false>, (void*)k_proto<2, false>, (void*)k_proto<3, false>,
                   (void*)k_proto<0, true>, (void*)k_proto<1, true>, (void*)k_proto<2, true>, (void*)k_proto<3, true>}) {
    CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LN_SMEM_BYTES));
    hipFuncAttributes fa;
    CHECK(hipFuncGetAttributes(&fa, fn));
    printf("# kernel regs %d  scratch %zu B  static LDS %zu B\n", fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes);
  }
  auto args = [&](int64_t r, int K, float* c) {
    Args a{};
    a.g.Wks = W; a.g.A = X; a.g.rows = r; a.g.K = K; a.g.a_blocked = 1;
    a.Y = Y; a.C = c; a.stamps = stamps;
    return a;
  };

  // ---- verify: the bodies on [1000, K] x [768, K]^T (K-slice-major W, blocked A) against each other and a host reference ----
  for (int K : {768, 3072}) {
    const int64_t vrows32 = (vrows + 31) / 32 * 32;
    std::vector<bf16_t> hw((size_t)T::TR * K), hx((size_t)vrows32 * K);
    CHECK(hipMemcpy(hw.data(), W, hw.size() * 2, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hx.data(), X, hx.size() * 2, hipMemcpyDeviceToHost));
    std::vector<float> c[NBODY];
    for (int b = 0; b < NBODY; ++b) {
      CHECK(hipMemset(C[b], 0xff, (size_t)vrows * T::TR * 4));
      launch(b, true, args(vrows, K, C[b]));
      CHECK(hipDeviceSynchronize());
      CHECK(hipGetLastError());
      c[b].resize((size_t)vrows * T::TR);
      CHECK(hipMemcpy(c[b].data(), C[b], c[b].size() * 4, hipMemcpyDeviceToHost));
    }
    size_t bad = 0;
    double dmax[NBODY] = {}, rmax[NBODY] = {}, scale = 0;
    for (size_t i = 0; i < c[0].size(); ++i)
      for (int b = 0; b < NBODY; ++b) {
        if (!std::isfinite(c[b][i])) { ++bad; continue; }
        if (std::isfinite(c[0][i])) dmax[b] = std::max(dmax[b], (double)std::fabs(c[b][i] - c[0][i]));
      }
    uint64_t sd = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (uint32_t)(sd >> 24); };
    for (int smp = 0; smp < 4096; ++smp) {
      const int64_t t = smp < 64 ? vrows - 1 - smp : rnd() % vrows;
      const int f = rnd() % T::TR;
      double ref = 0, mag = 0;
      for (int k = 0; k < K; ++k) {
        const float wv = bf16_host(hw[((size_t)(k / 32) * T::TR + f) * 32 + k % 32]);                        // [K / 32][768][32]
        const float xv = bf16_host(hx[(((size_t)(t / 32) * (K / 8) + k / 8) * 32 + t % 32) * 8 + k % 8]);    // [rows / 32][K / 8][32][8]
        const double pr = (double)wv * xv;
        ref += pr; mag += std::fabs(pr);
      }
      for (int b = 0; b < NBODY; ++b) rmax[b] = std::max(rmax[b], std::fabs(c[b][t * T::TR + f] - ref));
      scale = std::max(scale, mag);
    }
    // fp32 accumulation of K exact bf16 products: |error| <= K * 2^-24 * sum |products| (a loose, reasoned bound)
    const double bound = K * std::ldexp(1.0, -24) * scale;
    printf("# verify K = %d: non-finite / unwritten %zu, max |body - 32x32x16| %.3g / %.3g / %.3g, max |body - fp64 host| %.3g / %.3g / %.3g / %.3g (bound %.3g)\n",
           K, bad, dmax[1], dmax[2], dmax[3], rmax[0], rmax[1], rmax[2], rmax[3], bound);
    if (bad || rmax[0] > bound || rmax[1] > bound || rmax[2] > bound || rmax[3] > bound) { printf("VERIFY FAILED\n"); return 1; }
  }

  // ---- timing ---------------------------------------------------------------------------------------------------------------
  for (int K : {3072, 768}) {
    const Args a = args(rows, K, nullptr);
    const int nk = K / LN_SLICE;
    const double steps_per_cu = (double)(rows / T::TL) / prop.multiProcessorCount * nk;
    printf("# shape %lld x %d -> 768: %d K steps per workgroup, %.0f per CU, %d rounds per body of %d launches, order A B C D D C B A ...\n",
           (long long)rows, K, nk, steps_per_cu, 2 * cycles, launches);
    // warm-up: > 2 s of back-to-back launches so that the clock has settled under load
    for (int i = 0; i < (K == 3072 ? 2400 : 7200); ++i) launch(i % NBODY, false, a);
    CHECK(hipDeviceSynchronize());
    std::vector<Round> res[NBODY];
    printf("# round body          ms/launch  us/Kstep(wall)  ticks/Kstep  clock MHz   TFLOP/s\n");
    for (int r = 0; r < 2 * NBODY * cycles; ++r) {
      const int ph = r % (2 * NBODY);
      const int body = ph < NBODY ? ph : 2 * NBODY - 1 - ph;
      const Round x = timed_round(body, a, launches);
      res[body].push_back(x);
      printf("%5d  %s  %9.4f  %13.4f  %11.1f  %9.0f  %8.0f\n", r, BODY_NAME[body], x.ms, x.ms * 1e3 / steps_per_cu, x.ticks_per_step,
             x.clock_mhz, 2.0 * rows * T::TR * K / x.ms / 1e9);
      fflush(stdout);
    }
    double mn[NBODY], mx[NBODY];
    for (int b = 0; b < NBODY; ++b) {
      std::vector<double> ms, tk, ck;
      for (auto& x : res[b]) { ms.push_back(x.ms); tk.push_back(x.ticks_per_step); ck.push_back(x.clock_mhz); }
      mn[b] = *std::min_element(ms.begin(), ms.end()); mx[b] = *std::max_element(ms.begin(), ms.end());
      printf("# K = %d %s: wall per K step median %.4f us  min %.4f  max %.4f  (ms/launch median %.4f) | ticks/Kstep median %.1f | clock median %.0f MHz\n",
             K, BODY_NAME[b], median(ms) * 1e3 / steps_per_cu, mn[b] * 1e3 / steps_per_cu, mx[b] * 1e3 / steps_per_cu, median(ms),
             median(tk), median(ck));
    }
    for (int b = 1; b < NBODY; ++b)
      printf("# K = %d %s against 32x32x16: every round faster than every 32x32x16 round: %s (slowest %.4f ms, fastest 32x32x16 %.4f ms)\n",
             K, BODY_NAME[b], mx[b] < mn[0] ? "yes" : "NO", mx[b], mn[0]);
  }
  return 0;
}
