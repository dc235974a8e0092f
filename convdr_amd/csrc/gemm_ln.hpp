// Row-complete GEMM with fused residual + LayerNorm epilogue (inference path, hidden size 768):
//     X_out[t, :] = LayerNorm( A[t, :] . W^T + bias + R[t, :] ) * gamma + beta        (bf16 out)
// replaces  k_gemm<EPI_RESID_F32> (fp32 pre-LN sums to HBM) + k_layernorm (read them back): one workgroup owns
// 128 tokens x ALL 768 output features, so the row statistics are available on chip and the 3 KB/token fp32
// round trip (27 % of the encoder's HBM traffic) disappears.
//   HF call sites: BertSelfOutput / BertOutput  (dense -> dropout -> LayerNorm(x + residual)).
// Geometry: 8 waves = 4 (features) x 2 (tokens); wave tile 192 features x 64 tokens = 12 x 4 blocks of 16 x 16 on
// v_mfma_f32_16x16x32_bf16 (GemmAcc16<TileLN>, 192 accumulator VGPRs).  That shape because these GEMMs run power-capped and
// the chip holds a higher clock on it than on 32x32x16 (gemm_nt.hpp, gemm_nt_mainloop_r3_m16; profiles/ln_mfma16_proto.txt,
// profiles/ln_mfma16_ab.txt).  Operands staged by LDS-DMA in 32-wide K slices, one slice = one MFMA K step:
// W slice 768 x 64 B = 48 KB in three slots, A slice 128 x 64 B = 8 KB in two  -> LN_SMEM_BYTES = 160 KB, one workgroup per CU.
// 64-byte LDS rows: an operand fragment is row (lane & 15), 16-byte chunk (lane >> 4); the chunk index XOR ln_swz(row) keeps
// that ds_read_b128 conflict-free (applied to the DMA source address, LDS-DMA writes lane-linear).
#pragma once
#include "gemm_nt.hpp"

namespace convdr {

using TileLN = TileCfg<4, 2, 6, 2>;   // TR = 768 features, TL = 128 tokens
constexpr int LN_SLICE = 32;
constexpr int LN_R_BYTES = TileLN::TR * 64, LN_L_BYTES = TileLN::TL * 64;
constexpr int LN_SMEM_BYTES = 3 * LN_R_BYTES + 2 * LN_L_BYTES;   // 160 KB: three weight slots + two activation slots

struct GemmLnArgs {
  const bf16_t* W;      // [768, K]
  const bf16_t* A;      // [rows, K]
  int64_t rows;
  int K;
  const float* bias;    // [768]
  const bf16_t* R;      // residual [rows, 768]
  const float *gamma, *beta;
  float eps;
  bf16_t* X;            // out [rows, 768] (may alias R: a workgroup reads its residual rows before it writes them)
  const bf16_t* Wks;    // W in K-slice-major order [K / 32][768][32] (or null: stream the row-major W)
  int a_blocked;        // A is in the blocked layout [rows / 32][K / 8][32][8] the FFN1 epilogue EPI_GELU_BLK writes
  // Trace library only (trace_knobs.hpp; empty in the product).  skip_epi: timing experiment, the kernel ends after its main
  // loop (garbage results); trace: [workgroup][16] s_memtime stamps of thread 0 (or null)
  [[no_unique_address]] TraceKnobs knobs;
};
#ifdef CONVDR_ENABLE_TRACE   // make TRACE=1: stamps for tools/gemm_trace_ln.py
#define CONVDR_LN_TRACE(ph) \
  if (a.knobs.trace() && threadIdx.x == 0) a.knobs.trace()[(size_t)blockIdx.x * 16 + (ph)] = __builtin_amdgcn_s_memtime();
// per-wave stamps of K step 8 (and the top of step 9): trace[2048 * 16 + wg * 64 + wave * 8 + i]
#define CONVDR_LN_STEP(i)                                                 \
  if (trace && kt == 8 + (i) / 5 && w.lane == 0 && blockIdx.x < 256)      \
    trace[2048 * 16 + blockIdx.x * 64 + w.wave * 8 + (i)] = __builtin_amdgcn_s_memtime();
#else
#define CONVDR_LN_TRACE(ph)
#define CONVDR_LN_STEP(i)
#endif

// 32-wide K slices: 64-byte LDS rows, 16 rows per wave per round, rounds 16 x (issuing waves) rows apart.  Same
// buffer-descriptor addressing as gemm_nt.hpp's gemm_stage.
// Who issues the LDS-DMA, as R3Issue in gemm_nt.hpp: the older wave of each SIMD (waves 0-3), which the matrix pipe serves
// first and which then idles in the barrier, issues the WHOLE weight slice of step t + 2 after its MFMAs; the younger
// (waves 4-7) issues the activation slice of step t + 1 at the top of the step (FFN2 12.95 -> 12.44 ms per 12 layers).
constexpr int LN_DMA_WAVES = 8, LN_DMA_FIRST = 0;                 // cooperative loads outside the main loop
constexpr int LN_W_WAVES = 4, LN_W_FIRST = 0;                     // weight slices
constexpr int LN_A_WAVES = 4, LN_A_FIRST = 4;                     // activation slices
constexpr int LN_A_AUX = 2;   // cache policy of the activation-slice DMA (2 = nt: every activation row is read by ONE workgroup)

// LDS chunk c of row `row` holds source chunk c ^ ln_swz(row).  (With chunk ^ ((row >> 2) & 3), conflict-free for 32-row
// fragments, the 16-row fragment read is 2-way bank-conflicted in each of the four ds_read_b128 lane groups.)
constexpr int ln_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// the four 16-lane groups one ds_read_b128 is served in: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and both + 32
constexpr bool ln_frag_read_conflict_free() {
  for (int g = 0; g < 4; ++g) {
    unsigned seen = 0;
    for (int l = 0; l < 64; ++l) {
      const int m = l & 31;
      const bool first = m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
      if ((l >> 5) != (g >> 1) || first != ((g & 1) == 0)) continue;
      const int row = l & 15, q = l >> 4;
      const int slot = ((row * 64 + ((q ^ ln_swz(row)) << 4)) >> 4) & 15;   // 16-byte slot of the 256 B the 64 banks span
      if ((seen >> slot) & 1u) return false;
      seen |= 1u << slot;
    }
    if (seen != 0xffffu) return false;
  }
  return true;
}
static_assert(ln_frag_read_conflict_free(), "16-row fragment read: 16 distinct 16-byte slots in every ds_read_b128 lane group");
static_assert(ln_swz(0) == ln_swz(16) && ln_swz(5) == ln_swz(5 + 16 * LN_W_WAVES), "the swizzle term is round-independent");

// the window rows [row0, nrows) of G as a buffer (rows past the end read as zeros, stores to them are dropped).  .voff and
// .round_pitch address a 32-wide slice for WAVES issuing waves, the first of which is wave FIRST.
template <int WAVES = LN_DMA_WAVES, int FIRST = LN_DMA_FIRST>
__device__ __forceinline__ StageSrc ln_stage_src(const bf16_t* __restrict__ G, int64_t ld, int64_t row0, int64_t nrows,
                                                  int wave, int lane) {
  StageSrc s;
  wave = wave >= FIRST ? wave - FIRST : 0;
  int64_t bytes = (nrows - row0) * ld * 2;
  bytes = bytes < 0 ? 0 : (bytes > 0xffffffffll ? 0xffffffffll : bytes);
  const uint64_t base = (uint64_t)(G + row0 * ld);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  const uint32_t nb = __builtin_amdgcn_readfirstlane((uint32_t)bytes);
  s.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
  const int row = wave * 16 + (lane >> 2);
  const int gch = (lane & 3) ^ ln_swz(row);   // source chunk of the slice for LDS chunk (lane & 3)
  s.voff = (uint32_t)(row * ld * 2) + gch * 16;
  s.round_pitch = __builtin_amdgcn_readfirstlane((uint32_t)(16 * WAVES * ld * 2));
  return s;
}

template <int ROWS, int WAVES = LN_DMA_WAVES, int FIRST = LN_DMA_FIRST, int AUX = 0>
__device__ __forceinline__ void ln_stage32(const StageSrc& s, int ks, char* lds_tile, int wave,
                                           uint32_t slice_stride = LN_SLICE * 2) {
  if (wave < FIRST || wave >= FIRST + WAVES) return;   // wave-uniform
  wave -= FIRST;
  constexpr int ROUNDS = ROWS / (16 * WAVES);
  static_assert(ROUNDS * 16 * WAVES == ROWS, "rows must be a multiple of 16 x issuing waves");
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(s.rsrc, (lptr_t)(lds_tile + (i * WAVES + wave) * 16 * 64), 16, s.voff,
                                             i * s.round_pitch + ks * slice_stride, 0, AUX);
}

constexpr int LN_RED_SLOTS = 16;                       // partial row sums per token: wr * 4 + (lane >> 4)
constexpr int LN_IMG_OFF = 20480;                      // 9 KB parameters + 8 KB partials + 1 KB statistics, then the image
static_assert((3 * 768 + 128 * LN_RED_SLOTS + 256) * 4 <= LN_IMG_OFF && LN_IMG_OFF + 64 * 1536 <= LN_SMEM_BYTES, "epilogue LDS");

struct LnSrc {
  StageSrc W, A;
  uint32_t w_slice_stride, a_slice_stride;
};

// The operand windows, the source chunk swizzled by ln_swz.
// Weights come from the K-slice-major copy when there is one: a 32-wide slice of the row-major [768, K] matrix is 768 half
// cache lines, every line is fetched twice (once per slice) and the 112 KB that leaves L2 per CU per step made this kernel
// L2-bandwidth-bound (5.2 k cycles per 1,536-cycle step); in slice-major order a slice is 48 KB of whole lines.
__device__ __forceinline__ LnSrc ln_sources(const GemmLnArgs& a, int64_t t0, const WavePos<TileLN>& w) {
  using T = TileLN;
  LnSrc s;
  s.W = a.Wks ? ln_stage_src<LN_W_WAVES, LN_W_FIRST>(a.Wks, LN_SLICE, 0, (int64_t)T::TR * (a.K / LN_SLICE), w.wave, w.lane)
              : ln_stage_src<LN_W_WAVES, LN_W_FIRST>(a.W, a.K, 0, T::TR, w.wave, w.lane);
  s.w_slice_stride = a.Wks ? T::TR * LN_SLICE * 2 : LN_SLICE * 2;
  s.A = ln_stage_src<LN_A_WAVES, LN_A_FIRST>(a.A, a.K, t0, a.rows, w.wave, w.lane);
  s.a_slice_stride = LN_SLICE * 2;
  static_assert((16 * LN_A_WAVES) % 32 == 0 && TileLN::TL % (16 * LN_A_WAVES) == 0, "blocked A staging: rounds of whole 32-token blocks");
  if (a.a_blocked) {
    // blocked activations: a 16-token x 4-octet DMA instruction reads 4 runs of 256 contiguous bytes (whole lines; the
    // row-major form reads 16 half lines).  Window: from this tile's first 32-token block to the end of the last block.
    const int64_t rows32 = (a.rows + 31) & ~(int64_t)31;
    const int64_t blk_elems = (int64_t)(a.K >> 3) * 256;            // one 32-token block, all K
    int64_t bytes = (rows32 - t0) / 32 * blk_elems * 2;
    bytes = bytes < 0 ? 0 : (bytes > 0xffffffffll ? 0xffffffffll : bytes);
    const uint64_t base = (uint64_t)(a.A + (t0 >> 5) * blk_elems);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    const uint32_t nb = __builtin_amdgcn_readfirstlane((uint32_t)bytes);
    s.A.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
    const int wv = w.wave >= LN_A_FIRST ? w.wave - LN_A_FIRST : 0;
    const int row = wv * 16 + (w.lane >> 2);                        // token inside a round of 16 x LN_A_WAVES tokens
    const int gch = (w.lane & 3) ^ ln_swz(row);                     // source octet of the slice for LDS chunk (lane & 3)
    s.A.voff = (uint32_t)((row >> 5) * blk_elems * 2 + gch * 512 + (row & 31) * 16);
    // rounds are 16 * LN_A_WAVES tokens apart: a multiple of 32, so (row & 31) is round-independent and a round advances
    // whole 32-token blocks
    s.A.round_pitch = __builtin_amdgcn_readfirstlane((uint32_t)((16 * LN_A_WAVES / 32) * blk_elems * 2));
    s.a_slice_stride = 4 * 512;                                     // four octets per 32-wide slice
  }
  return s;
}

// Main loop.  Three weight slots, two activation slots: the weight slice of step t + 2 is issued at step t.  With one slice
// in flight (two stages) the stream was bound by bytes in flight / latency -- 56 KB per CU over a ~2 us loaded L2 round
// trip = 28 GB/s per CU, 4.5 k cycles per 1,536-cycle step -- so a third 48 KB slot buys a second weight slice in flight.
// Issue order per step: A(t+1), then W(t+2); completion is in issue order, so "W(t), A(t) landed" = all but the newest
// weight group (LN_W_DPW instructions per issuing wave) retired.
// One slice is 12 weight fragments x 4 activation fragments = 48 MFMAs per wave, walked feature-major: unit u = weight
// fragment u and its 4 MFMAs.  There is no room beside 192 accumulators for a second fragment set, and left to itself hipcc
// reads each weight fragment right before its MFMAs and waits for it at once.  So 4 activation fragments + three rotating
// weight fragments (28 VGPRs), the fragment of unit u + 2 read before the MFMAs of unit u -- one ds_read_b128 per 64 MFMA
// cycles, one exposed LDS round trip per slice (right after the barrier, where nothing can be prefetched).  Units 0 and 1 run
// on token blocks 0-1 first, then on blocks 2-3; all six first fragments are read ahead of the first MFMA.
// sched_group_barrier pins the order.
// profiles/ln_mfma16_proto.txt, wall per K step at K = 3,072: 1.319 us on 32x32x16; here 1.223, 1.239 with units 0 and 1 on all four blocks at once, 1.226 with fb(2), fb(3) read behind the first two MFMAs
__device__ __forceinline__ void ln_mainloop(const LnSrc& s, int nk, char* smem, GemmAcc16<TileLN>& acc,
                                            const WavePos<TileLN>& w, unsigned long long* trace) {
  using T = TileLN;
  constexpr int MB = GemmAcc16<T>::MB, NB = GemmAcc16<T>::NB;
  static_assert(MB == 12 && NB == 4, "TileLN: 12 x 4 blocks per wave");
  char* sW = smem;                       // 3 weight slots
  char* sA = smem + 3 * LN_R_BYTES;      // 2 activation slots
  const int r16 = w.lane & 15;
  const int ch = ((w.lane >> 4) ^ ln_swz(r16)) * 16;
  const int offR = (w.wr * T::MT * 32 + r16) * 64 + ch;
  const int offL = (w.wl * T::NT * 32 + r16) * 64 + ch;
  constexpr int LN_W_DPW = T::TR / (16 * LN_W_WAVES);   // weight DMA instructions per issuing wave per slice
  const bool w_wave = w.wave >= LN_W_FIRST && w.wave < LN_W_FIRST + LN_W_WAVES;   // (wave-uniform) this wave has weight slices in flight
  ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(s.W, 0, sW, w.wave, s.w_slice_stride);
  ln_stage32<T::TL, LN_A_WAVES, LN_A_FIRST, LN_A_AUX>(s.A, 0, sA, w.wave, s.a_slice_stride);
  if (nk > 1) ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(s.W, 1, sW + LN_R_BYTES, w.wave, s.w_slice_stride);
  int wslot = 0;   // kt % 3
  for (int kt = 0; kt < nk; ++kt) {
    CONVDR_LN_STEP(5)
    CONVDR_LN_STEP(0)
    if (kt + 1 < nk && w_wave) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LN_W_DPW) : "memory");
    else lds_dma_wait_all();   // (a wave without weight slices has only this step's activation slice outstanding)
    CONVDR_LN_STEP(1)
    lds_barrier();   // NOT __syncthreads(): its fence would add vmcnt(0) and drain the slice that must stay in flight
    CONVDR_LN_STEP(2)
    if (kt + 1 < nk) ln_stage32<T::TL, LN_A_WAVES, LN_A_FIRST, LN_A_AUX>(s.A, kt + 1, sA + ((kt + 1) & 1) * LN_L_BYTES, w.wave, s.a_slice_stride);
    const bool issue_w = kt + 2 < nk;
    char* w_dst = sW + (wslot == 0 ? 2 : wslot - 1) * LN_R_BYTES;   // slot (kt + 2) % 3
    CONVDR_LN_STEP(3)
    const char* tR = sW + wslot * LN_R_BYTES + offR;
    const char* tL = sA + (kt & 1) * LN_L_BYTES + offL;
    wslot = wslot == 2 ? 0 : wslot + 1;
    {
      bf16x8 fb[NB], fa[3];
      auto load_a = [&](int u) { fa[u % 3] = *(const bf16x8*)(tR + u * 16 * 64); };
      auto load_b = [&](int j) { fb[j] = *(const bf16x8*)(tL + j * 16 * 64); };
      auto mm = [&](int u, int j) { acc.c[u][j] = mfma_16x16x32<false>(fa[u % 3], fb[j], acc.c[u][j]); };
      load_b(0); load_b(1);
      load_a(0); load_a(1);
      load_b(2); load_b(3);
      mm(0, 0); mm(0, 1);
      mm(1, 0); mm(1, 1);
      load_a(2);
      mm(0, 2); mm(0, 3);
      load_a(3);
      mm(1, 2); mm(1, 3);
#pragma unroll
      for (int u = 2; u < MB; ++u) {
        if (u + 2 < MB) load_a(u + 2);
#pragma unroll
        for (int j = 0; j < NB; ++j) mm(u, j);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                        // fb(0), fb(1), fa(0), fa(1)
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                        // fb(2), fb(3)
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // fa(2)
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // fa(3)
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#pragma unroll
      for (int u = 2; u < MB; ++u) {
        if (u + 2 < MB) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // fa(u + 2)
        __builtin_amdgcn_sched_group_barrier(0x008, NB, 0);                     // the unit's 4 MFMAs
      }
    }
    // the weight slice of step t + 2 once this wave's MFMAs of the step are in the pipe: the ~60-cycle issue stalls then
    // cost no matrix-pipe time (two steps of slack for the landing)
    if (issue_w) ln_stage32<T::TR, LN_W_WAVES, LN_W_FIRST>(s.W, kt + 2, w_dst, w.wave, s.w_slice_stride);
    CONVDR_LN_STEP(4)
  }
}

// Epilogue: + bias + residual, LayerNorm over the 768 features of each token.
// In the accumulator layout a lane holds 4 features of one token, so direct residual loads / output stores touch 16 rows x
// 8 B per instruction.  Both tiles therefore pass through LDS in full rows: the residual half-tile (64 tokens x 1536 B)
// arrives by LDS-DMA, the normalised half-tile is parked in the same image and leaves 16 B per lane.  Image row lr holds a
// token's 96 chunks of 16 B; chunk position p holds feature chunk (p & ~31) | ((p ^ lr) & 31) -- the swizzle spreads the
// per-lane 8-byte accesses (many rows x the same feature chunk) over the banks.
// With q = lane >> 4, t = lane & 15, block (i, j) register r is feature wr * 192 + 16 i + 4 q + r of token wl * 64 + 16 j + t.
// Image half h holds token blocks 2h, 2h + 1; a token's image row is lrl = wl * 32 + 16 (j & 1) + t, the lane's 8 bytes are
// half (q & 1) of feature chunk wr * 24 + 2 i + (q >> 1).  A token's row statistics come in LN_RED_SLOTS partial sums
// (4 feature waves x 4 lane quarters).
__global__ void __launch_bounds__(512, 2) k_gemm_resid_ln(const GemmLnArgs a) {
  using T = TileLN;
  constexpr int MB = GemmAcc16<T>::MB, NB = GemmAcc16<T>::NB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WavePos<T> w;
  const int64_t t0 = (int64_t)blockIdx.x * T::TL;
  GemmAcc16<T> acc;
  acc.zero();
  CONVDR_LN_TRACE(0)
  {
    const LnSrc src = ln_sources(a, t0, w);
    ln_mainloop(src, a.K / LN_SLICE, smem, acc, w, a.knobs.trace());
  }
  if (a.knobs.skip_epi()) {   // (keeps the accumulators alive; a constant 0 in the product)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc.c[i][j][r];
    if (s == 12345.678f) a.X[0] = f32_to_bf16(s);
    return;
  }
  CONVDR_LN_TRACE(1)
  __syncthreads();   // operand buffers are dead
  float* sBias = (float*)smem;           // [768]
  float* sGam = sBias + 768;
  float* sBet = sGam + 768;
  float* sRed = sBet + 768;              // [128 tokens][16 partial slots]
  float* sStat = sRed + 128 * LN_RED_SLOTS;   // [128] mean, [128] rstd
  char* sC = smem + LN_IMG_OFF;          // [64][1536 B] residual / output image
  const int q = w.lane >> 4, t16 = w.lane & 15;
  const int slot = w.wr * 4 + q;
  const int f0 = w.wr * T::MT * 32 + 4 * q;   // block i: features f0 + 16 i ... + 3
  // residual and output windows [t0, rows) as buffers: residual rows past the end read as zeros, output rows past it are dropped
  const StageSrc srcR = ln_stage_src(a.R, 768, t0, a.rows, w.wave, w.lane);   // (only .rsrc is used)
  const __amdgpu_buffer_rsrc_t dstX = ln_stage_src(a.X, 768, t0, a.rows, w.wave, w.lane).rsrc;
  // Byte offset of this lane's 8 bytes of feature chunk `chunk` in image row lrl
  //     = lrl * 1536 + (((chunk & ~31) | ((chunk ^ lrl) & 31)) << 4) + (q & 1) * 8,
  // evaluated as ONE v_xor per access: the row base lrl * 1536 and the image base have zeros in bits 4-8, so with
  // B = base + lrl * 1536 + ((lrl & 31) << 4) + (q & 1) * 8 the address is (B ^ ((chunk & 31) << 4)) + ((chunk & ~31) << 4),
  // the second term a compile-time DS offset.  The lane's chunks wr * 24 + 2 i + (q >> 1) have wr * 24 + 2 i even, so the
  // (q >> 1) is one more XOR into B.  (The closed form cost ~5 integer instructions per access, 96 accesses per wave: the
  // epilogue is VALU-bound.)
  typedef __attribute__((address_space(3))) u32x2_t lds_u2_t;
  static_assert((LN_IMG_OFF & 511) == 0, "the image base must leave bits 4-8 to the swizzle");
  auto img_base = [&](int lrl) {
    return (lds_off(sC) + (uint32_t)(lrl * 1536 + ((lrl & 31) << 4) + (q & 1) * 8)) ^ (uint32_t)((q >> 1) << 4);
  };
  auto img_at = [&](uint32_t B, int chunk) {   // chunk even
    return (lds_u2_t*)(uintptr_t)((B ^ (uint32_t)((chunk & 31) << 4)) + (uint32_t)((chunk & ~31) << 4));
  };
  // lrl / tid are handed in as opaque per-phase copies: with 192 accumulators live, addresses that the compiler CSEs across
  // phases end up in scratch
  auto opaque = [](int x) {
    asm volatile("" : "+v"(x));
    return x;
  };
  CONVDR_LN_TRACE(2)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();   // every lane has consumed the previous half
    // 6144 chunks: thread t fills positions i * 512 + t (lane-linear per wave instruction, as LDS-DMA requires)
    // (position idx = i * 512 + t is row idx / 96, chunk idx % 96: one division for i = 0, then 512 = 5 * 96 + 32)
    const int tid_a = opaque((int)threadIdx.x);
    int lr = tid_a / 96, pp = tid_a - lr * 96;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int c = (pp & ~31) | ((pp ^ lr) & 31);
      const int tok = (lr >> 5) * 64 + h * 32 + (lr & 31);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srcR.rsrc, (lptr_t)(sC + (i * 512 + w.wave * 64) * 16), 16,
                                               (uint32_t)(tok * 1536 + c * 16), 0, 0, 0);
      pp += 32; lr += 5;
      if (pp >= 96) { pp -= 96; lr += 1; }
    }
    if (h == 0) {
      // the LayerNorm parameters ride under the first residual half's flight (staged before it, their loads and the
      // residual's round trip were two exposed latencies in a row)
      for (int i = threadIdx.x; i < 768; i += 512) { sBias[i] = a.bias[i]; sGam[i] = a.gamma[i]; sBet[i] = a.beta[i]; }
      CONVDR_LN_TRACE(8)
    }
    lds_dma_wait_all();
    if (h == 0) { CONVDR_LN_TRACE(9) }
    __syncthreads();           // (first half: also publishes the LayerNorm parameters)
    if (h == 0) { CONVDR_LN_TRACE(10) }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = 2 * h + jj;
      float s = 0.f;
      const uint32_t imgB = img_base(opaque(w.wl * 32 + 16 * jj + t16));
#pragma unroll
      for (int i0 = 0; i0 < MB; i0 += 4) {
        u32x2_t res[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) res[g] = *img_at(imgB, w.wr * 24 + 2 * (i0 + g));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4& v = acc.c[i0 + g][j];
          const float4 bv = *(const float4*)(sBias + f0 + 16 * (i0 + g));
          const u32x2_t r = res[g];
          v[0] += bv.x + __uint_as_float(r.x << 16);
          v[1] += bv.y + __uint_as_float(r.x & 0xffff0000u);
          v[2] += bv.z + __uint_as_float(r.y << 16);
          v[3] += bv.w + __uint_as_float(r.y & 0xffff0000u);
          s += (v[0] + v[1]) + (v[2] + v[3]);
        }
      }
      sRed[(w.wl * 64 + 16 * j + t16) * LN_RED_SLOTS + slot] = s;
    }
    if (h == 0) { CONVDR_LN_TRACE(11) }
  }
  CONVDR_LN_TRACE(3)
  __syncthreads();
  CONVDR_LN_TRACE(4)
  auto sum16 = [](const float* p) {
    return ((((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) +
            (((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15]))));
  };
  if (threadIdx.x < 128) sStat[threadIdx.x] = sum16(sRed + threadIdx.x * LN_RED_SLOTS) * (1.f / 768.f);
  __syncthreads();
  float mean[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    mean[j] = sStat[w.wl * 64 + 16 * j + t16];
    float qs = 0.f;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = acc.c[i][j][r] - mean[j];
        qs += d * d;
      }
    sRed[(w.wl * 64 + 16 * j + t16) * LN_RED_SLOTS + slot] = qs;
  }
  CONVDR_LN_TRACE(5)
  __syncthreads();
  if (threadIdx.x < 128) {
    const float var = sum16(sRed + threadIdx.x * LN_RED_SLOTS) * (1.f / 768.f);
    sStat[128 + threadIdx.x] = rsqrtf(var + a.eps);
  }
  __syncthreads();
  CONVDR_LN_TRACE(6)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();   // the previous half has been read out
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = 2 * h + jj;
      const float rstd = sStat[128 + w.wl * 64 + 16 * j + t16];
      const uint32_t imgB = img_base(opaque(w.wl * 32 + 16 * jj + t16));
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int f = f0 + 16 * i;
        const float4 gg = *(const float4*)(sGam + f), bb = *(const float4*)(sBet + f);
        const f32x4& v = acc.c[i][j];
        u32x2_t o;
        o.x = pack_bf16x2((v[0] - mean[j]) * rstd * gg.x + bb.x, (v[1] - mean[j]) * rstd * gg.y + bb.y);
        o.y = pack_bf16x2((v[2] - mean[j]) * rstd * gg.z + bb.z, (v[3] - mean[j]) * rstd * gg.w + bb.w);
        *img_at(imgB, w.wr * 24 + 2 * i) = o;
      }
    }
    if (h == 0) { CONVDR_LN_TRACE(12) }
    __syncthreads();
    if (h == 0) { CONVDR_LN_TRACE(13) }
    const int tid_s = opaque((int)threadIdx.x);
    int lr = tid_s / 96, pp = tid_s - lr * 96;
#pragma unroll
    for (int i0 = 0; i0 < 12; i0 += 4) {
      u32x4_t v4[4];
#pragma unroll
      for (int jv = 0; jv < 4; ++jv) v4[jv] = *(const u32x4_t*)(sC + ((i0 + jv) * 512 + tid_s) * 16);
#pragma unroll
      for (int jv = 0; jv < 4; ++jv) {
        const int c = (pp & ~31) | ((pp ^ lr) & 31);
        const int tok = (lr >> 5) * 64 + h * 32 + (lr & 31);
        // through the output window [t0, rows): rows past the end are dropped by the bounds check; one 32-bit offset
        __builtin_amdgcn_raw_buffer_store_b128(v4[jv], dstX, (uint32_t)(tok * 1536 + c * 16), 0, NT_LN ? 2 : 0);
        pp += 32; lr += 5;
        if (pp >= 96) { pp -= 96; lr += 1; }
      }
    }
    if (h == 0) { CONVDR_LN_TRACE(14) }
  }
  CONVDR_LN_TRACE(7)
}

}  // namespace convdr
