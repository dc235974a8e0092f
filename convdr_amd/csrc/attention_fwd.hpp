// k_attention_fwd: self-attention of the inference forward (the training forward and backward: attention_train.hpp).
#pragma once
#include "gemm_nt.hpp"

namespace convdr {

// ---------------------------------------------------------------------------------------------
// Self-attention, head_dim 64, varlen (one sequence per blockIdx.z, no padding keys exist).
// Workgroup = 4 waves = 128 queries of one (sequence, head); K and V^T tiles of 64 keys staged in LDS by
// LDS-DMA and shared by the 4 waves; each wave owns 32 queries.  Everything per query is LANE-LOCAL:
//   S^T = K Q^T   (A = K rows, B = Q)  -> lane = query, registers = keys
//   O^T = V^T P^T (A = V^T rows, B = P straight from the S^T registers) -> lane = query, registers = head dims
// The K rows feeding MFMA row i are permuted (bits 2 and 3 of i swapped) so that the 8 S^T registers
// 8s..8s+7 of a lane hold exactly the keys 16 s + 8 (lane >> 5) + 0..7 that MFMA expects as the lane's
// B-operand k-slots in the P.V step: no cross-lane shuffles, no LDS round trip for P.
// Online softmax over key tiles; lanes q and q+32 hold the two halves of a query's keys / head dims and
// exchange only the running max and the final row sum.  Writes LSE (natural log) when lse != nullptr.
// ---------------------------------------------------------------------------------------------
constexpr int ATT_KV_AUX = 2;   // cache policy of the K / V^T tile DMA of k_attention_fwd (nt: read by this workgroup only; 3.61 -> 3.29 ms per 12 layers)
struct AttnArgs {
  const bf16_t *Q, *K, *Vt;
  int64_t ldt;
  const int32_t *cu, *lens;
  int H;
  int64_t ldq;      // row stride of Q and K in elements (H, or 3H when they live in a fused [rows, 3H] buffer)
  bf16_t* ctx;
  float* lse;       // [heads, ldt] or nullptr
  float scale;      // 1 / sqrt(head_dim)
  [[no_unique_address]] TraceKnobs knobs;   // trace library only (trace_knobs.hpp): trace = [workgroup][8] s_memtime stamps of thread 0 (or null)
};
#ifdef CONVDR_ENABLE_TRACE
#define CONVDR_ATT_TRACE(i)                                                                                  \
  if (a.knobs.trace() && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x == 0 && blockIdx.z < 2048)        \
    a.knobs.trace()[blockIdx.z * 8 + (i)] = __builtin_amdgcn_s_memtime();
#else
#define CONVDR_ATT_TRACE(i)
#endif

constexpr int ATT_TILE_PAIR = 2 * 64 * 128;   // K tile + V^T tile, 8 KB each
constexpr int ATT_SMEM_BYTES = 2 * ATT_TILE_PAIR;  // double buffered

// A wave's 32 x 64 output tile (MFMA layout: lane (li, hi) holds 8-byte pieces of row li) -> global rows in whole
// 128-byte lines.  Stored straight from the registers a wave instruction touches 32 rows with 16 bytes each (256
// partial-line operations per wave against 32 for its K / V^T tiles); here the wave parks the tile in 4 KB of dead LDS
// (16-byte chunk index XOR row & 7) and each store instruction writes 8 whole rows.  `so`: the wave's 4 KB (every wave
// of the workgroup must be done with whatever lived there); dst: element (row 0, column 0) of the tile; rows < nvalid
// are written.  Attention forward 4.08 -> 3.86 ms per 12 layers.
__device__ __forceinline__ void attn_park_store(char* so, const f32x16 (&o)[2], float scale, int lane, bf16_t* dst,
                                                int64_t pitch, int nvalid) {
  const int li = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 ov;
      ov.x = pack_bf16x2(o[dt][4 * g + 0] * scale, o[dt][4 * g + 1] * scale);
      ov.y = pack_bf16x2(o[dt][4 * g + 2] * scale, o[dt][4 * g + 3] * scale);
      *(uint2*)(so + li * 128 + (((dt * 4 + g) ^ (li & 7)) << 4) + hi * 8) = ov;
    }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (a wave's LDS operations execute in order; this pins the compiler's)
  const int c8 = lane & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (lane >> 3) + 8 * i;
    const uint4 v = *(const uint4*)(so + row * 128 + ((c8 ^ (row & 7)) << 4));
    if (row < nvalid) *(uint4*)(dst + row * pitch + c8 * 8) = v;
  }
  __builtin_amdgcn_wave_barrier();   // (the region may be parked into again)
}

// CLS_Q (last layer of an inference pass): only the CLS row of every sequence is needed downstream.  Q is then a
// [B, H] matrix of CLS queries (row b), the workgroup still streams the sequence's K / V^T tiles, wave 0 alone does the
// arithmetic (all of its 32 query columns carry the same query) and one lane pair stores ctx[b] ([B, H]).
// CTX_BLK: the output goes to the blocked layout [rows / 32][H / 8][32 tokens][8 dims] (hm_blocked_offset) that the
// row-complete output projection stages with whole-line LDS-DMA: lanes (query, hi = 0 / 1) hold the two halves of a dim
// octet, one v_permlane32_swap per dword gives each lane 16 bytes, and runs of 8 tokens are whole 128-byte lines
// (sequences start at multiples of 8 rows) -- no LDS park, no barrier before the stores.
// QK_BLK: Q and K arrive in the same blocked layout (written by the QKV projection's blocked epilogue): a K tile's
// LDS-DMA pieces are runs of 8 tokens x 16 bytes = whole lines as before, and the Q fragment loads -- four 16-byte
// loads per lane that touched 32 rows x 32 bytes per instruction in the row-major form (128 of a wave's 224 line
// operations) -- read 512 contiguous bytes per half-wave.  (CLS_Q keeps its [B, H] row-major query matrix.)
template <bool CLS_Q, bool CTX_BLK = false, bool QK_BLK = false>
static __global__ void __launch_bounds__(256, 4) k_attention_fwd(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.z, h = blockIdx.y;
  const int len = a.lens[b];
  const int q0 = blockIdx.x * 128;
  if (q0 >= len) return;
  CONVDR_ATT_TRACE(0)
  const int64_t base = a.cu[b];
  const int plen = a.cu[b + 1] - (int)base;  // len rounded up to the row alignment (fetched with the other scalars: a
                                             // scalar load issued in the epilogue costs a full ~4 k-cycle round trip)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, li = lane & 31;
  const int q = CLS_Q ? 0 : q0 + wave * 32 + li;
  const int qc = q < len ? q : len - 1;
  const int H = a.H;
  CONVDR_ATT_TRACE(1)

  bf16x8 qf[4];
  if constexpr (QK_BLK && !CLS_Q) {
    const int64_t t = base + qc;
    const bf16_t* qp = a.Q + ((t >> 5) * (a.H >> 3) + h * 8 + hi) * 256 + (t & 31) * 8;
#pragma unroll
    for (int s = 0; s < 4; ++s) {   // dims 16 s + 8 hi .. + 7 = octet 2 s + hi
      qf[s] = __builtin_nontemporal_load((const bf16x8*)(qp + 2 * s * 256));   // (read by this workgroup only)
    }
  } else {
    const bf16_t* qp = CLS_Q ? a.Q + (int64_t)b * a.ldq + h * 64 + 8 * hi : a.Q + (base + qc) * a.ldq + h * 64 + 8 * hi;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
  }
  const float c = a.scale * 1.44269504088896341f;  // exp(x * scale) = exp2(x * c)
  float m = -INFINITY, l = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }

  const int sw = (lane >> 1) & 7;
  const int krow = (li & ~12) | ((li & 4) << 1) | ((li & 8) >> 1);  // bits 2 <-> 3
  const int ksw = (krow >> 1) & 7;

  // K / V^T tiles are double buffered: the LDS-DMA of tile t+1 flies under the MFMAs of tile t
  auto stage_tile = [&](int kv0, int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // 64 rows x 128 B per tile = 2 LDS-DMA rounds of 256 lanes x 16 B
      const int r0 = (i * 4 + wave) * 8;
      const int row = r0 + (lane >> 3);
      const int gch = (lane & 7) ^ ((row >> 1) & 7);
      if constexpr (QK_BLK) {
        const int64_t t = base + kv0 + row;
        glds16_aux<ATT_KV_AUX>((const char*)(a.K + ((t >> 5) * (a.H >> 3) + h * 8 + gch) * 256 + (t & 31) * 8), smem + buf * ATT_TILE_PAIR + r0 * 128);
      } else {
        glds16_aux<ATT_KV_AUX>((const char*)(a.K + (base + kv0 + row) * a.ldq + h * 64) + gch * 16, smem + buf * ATT_TILE_PAIR + r0 * 128);
      }
      glds16_aux<ATT_KV_AUX>((const char*)(a.Vt + (int64_t)(h * 64 + row) * a.ldt + base + kv0) + gch * 16,
             smem + buf * ATT_TILE_PAIR + 64 * 128 + r0 * 128);
    }
  };
  // Both buffers are filled up front: the kernel is bound by memory latency x bytes in flight (a workgroup's whole
  // working set is 64 KB and its arithmetic ~1 us), so the second tile's round trip must not start after the first's
  // has completed -- for the 128-token passages of the corpus that is the entire K/V of the head.
  stage_tile(0, 0);
  if (len > 64) stage_tile(64, 1);
  for (int kv0 = 0, it = 0; kv0 < len; kv0 += 64, ++it) {
    const int buf = it & 1;
    lds_dma_wait_all();  // explicit: hipcc's automatic vmcnt wait for LDS-DMA is not reliable (gemm_nt.hpp)
    __syncthreads();     // tile `it` landed for everyone; everyone finished reading tile it-1 (the other buffer)
    if (it >= 1 && kv0 + 64 < len) stage_tile(kv0 + 64, buf ^ 1);
    if (it == 0) { CONVDR_ATT_TRACE(2) }
    if (it == 1) { CONVDR_ATT_TRACE(3) }
    if (CLS_Q && wave != 0) continue;   // (has staged its share and passed the barrier)
    const char* sK = smem + buf * ATT_TILE_PAIR;
    const char* sV = sK + 64 * 128;

    // ---- S^T = K Q^T for the 64 keys of this tile ----
    f32x16 st[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
      const char* kp = sK + (kt * 32 + krow) * 128;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 kf = *(const bf16x8*)(kp + (((2 * s + hi) ^ ksw) * 16));
        st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[kt], 0, 0, 0);
      }
    }
    // register r of tile kt <-> key kv0 + 32 kt + 16 (r >> 3) + 8 hi + (r & 7)
    float mx = -INFINITY;
    if (kv0 + 64 > len) {  // ragged last tile only (workgroup-uniform): mask the keys past the sequence
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0 + 32 * kt + 16 * (r >> 3) + 8 * hi + (r & 7);
          if (key >= len) st[kt][r] = -INFINITY;
        }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);               // finite: every tile has >= 1 valid key
    const float mnc = mn * c;
    const float alpha = __builtin_amdgcn_exp2f(m * c - mnc);   // m = -inf on the first tile -> 0
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[kt][r], c, -mnc));   // one FMA + one v_exp_f32 per score
        st[kt][r] = p;
        ps += p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }

    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {  // 16 keys per step
      const int kt = s4 >> 1, r0 = (s4 & 1) * 8;
      union { bf16x8 v; uint32_t u[4]; } pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) pb.u[j] = pack_bf16x2(st[kt][r0 + 2 * j], st[kt][r0 + 2 * j + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const bf16x8 vf = *(const bf16x8*)(sV + (dt * 32 + li) * 128 + (((2 * s4 + hi) ^ sw) * 16));
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb.v, o[dt], 0, 0, 0);
      }
    }
  }

  CONVDR_ATT_TRACE(4)
  l += __shfl_xor(l, 32, 64);
  if constexpr (CLS_Q) {
    if (wave == 0 && li == 0) {
      const float inv = 1.f / l;
      bf16_t* dst = a.ctx + (int64_t)b * H + h * 64;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          uint2 ov;
          ov.x = pack_bf16x2(o[dt][4 * g + 0] * inv, o[dt][4 * g + 1] * inv);
          ov.y = pack_bf16x2(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
          *(uint2*)(dst + dt * 32 + 8 * g + 4 * hi) = ov;
        }
    }
    return;
  }
  if constexpr (CTX_BLK) {
    // (lane-dependent addresses from an opaque copy of the thread index: otherwise hipcc computes them ahead of the key
    //  loop and spills them across it -- 7 VGPR spills at this kernel's 128-register budget)
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int q_e = q0 + (tid_e >> 6) * 32 + (tid_e & 31), hi_e = (tid_e >> 5) & 1;
    const float inv = q_e < len ? 1.f / l : 0.f;     // alignment rows [len, plen) get zeros
    const int64_t t = base + q_e;
    bf16_t* blk = a.ctx + ((t >> 5) * (H >> 3) + h * 8) * 256 + (t & 31) * 8;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t x0 = pack_bf16x2(o[dt][8 * j + 0] * inv, o[dt][8 * j + 1] * inv);
        const uint32_t y0 = pack_bf16x2(o[dt][8 * j + 2] * inv, o[dt][8 * j + 3] * inv);
        const uint32_t x1 = pack_bf16x2(o[dt][8 * j + 4] * inv, o[dt][8 * j + 5] * inv);
        const uint32_t y1 = pack_bf16x2(o[dt][8 * j + 6] * inv, o[dt][8 * j + 7] * inv);
        const auto sx = __builtin_amdgcn_permlane32_swap(x0, x1, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(y0, y1, false, false);
        u32x4_t v;
        v.x = sx[0]; v.y = sy[0]; v.z = sx[1]; v.w = sy[1];
        if (q_e < plen) store16<NT_ATT>(blk + (dt * 4 + 2 * j + hi_e) * 256, v);
      }
    if (q_e < plen && a.lse && hi_e == 0) a.lse[(int64_t)h * a.ldt + base + q_e] = q_e < len ? m * a.scale + logf(l) : 0.f;
    CONVDR_ATT_TRACE(5)
    return;
  }
  __syncthreads();   // every wave is done with the last K / V^T tile: its buffers take the output tiles (attn_park_store)
  {
    // alignment rows [len, plen) get zeros: they feed later GEMMs / V^T columns and must stay finite
    const float inv = q < len ? 1.f / l : 0.f;
    const int r0 = q0 + wave * 32;
    attn_park_store(smem + wave * 4096, o, inv, lane, a.ctx + (base + r0) * H + h * 64, H, plen - r0);
    if (q < plen && a.lse && hi == 0) a.lse[(int64_t)h * a.ldt + base + q] = q < len ? m * a.scale + logf(l) : 0.f;
  }
  CONVDR_ATT_TRACE(5)
}
}  // namespace convdr
