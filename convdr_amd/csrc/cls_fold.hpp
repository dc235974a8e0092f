// Last layer of the inference forward when only the CLS row is live: the key and value projections folded through the
// single query of each (sequence, head), so that K and V of the other tokens are never formed.
//   scores   s_t = 0.125 q_h . (Wk_h x_t + bk_h) = u_h . x_t + const,   u_h = 0.125 Wk_h^T q_h   (the constant cancels in
//            the softmax, so bk is not read)
//   context  ctx_h = sum_t p_t (Wv_h x_t + bv_h) = Wv_h z_h + bv_h,     z_h = sum_t p_t x_t       (sum_t p_t = 1)
// Three launches replace the N = 2 H projection over every row and the CLS-query attention:
//   k_cls_key_fold    U[b, h, :] = 0.125 sum_j q[b, 64 h + j] Wk[64 h + j, :]          fp32 [B, heads, H]
//   k_cls_pool        Z[b, h, :] = softmax_t(U[b, h, :] . x_t) weighted sum of x_t     fp32 [B, heads, H], one pass over X
//   k_cls_value_fold  ctx[b, 64 h + j] = Wv[64 h + j, :] . Z[b, h, :] + bv[64 h + j]   bf16 [B, H]
// All three run on v_mfma_f32_16x16x32_bf16 with the weight / token index on the M side (accumulator registers: 4
// consecutive outputs per lane, one 16-byte store) and sequences / heads on the N side (lanes).  fp32 operands (U, the
// softmax weights, Z) enter the matrix unit as a bf16 high part plus a bf16 remainder -- two instructions, ~16 mantissa
// bits -- so the fold adds no bf16 rounding of its own; the work is too small for that to show in the time.
// Every reduction has a fixed order and there are no atomics: results are bitwise repeatable.
#pragma once
#include "gemm_nt.hpp"

namespace convdr {

union Frag8 {   // one lane's 8 bf16 of an MFMA operand
  bf16x8 v;
  uint32_t u[4];
  uint4 q;
  uint2 d[2];
};

// x[0..8) ~ hi + lo, both bf16 (round to nearest even)
__device__ __forceinline__ void split_bf16x8(const float* x, Frag8& hi, Frag8& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t h = pack_bf16x2(x[2 * i], x[2 * i + 1]);
    hi.u[i] = h;
    lo.u[i] = pack_bf16x2(x[2 * i] - __uint_as_float(h << 16), x[2 * i + 1] - __uint_as_float(h & 0xffff0000u));
  }
}

// Packed rows from which the fold replaces the K / V projection (measured: NOTEBOOK.md, "the last layer without K and V").
constexpr int64_t CLS_FOLD_MIN_ROWS = 16384;
constexpr int FOLD_ROWS = 64;            // sequences per workgroup of the two fold kernels (16 per wave)
constexpr int FOLD_NC = 128;             // Wk columns staged in LDS per step
constexpr int FOLD_LDW = FOLD_NC + 4;    // LDS row stride (elements): the 4 lane groups of a transposed read, 8 rows apart,
                                         // land 16 banks apart

// U[b, h, n] = scale * sum_j Q[b, 64 h + j] Wk[64 h + j, n].  grid (ceil(B / 64), heads), 256 threads.
// Wk ([H out][H in] row-major, the rows H .. 2 H of wqkv) has the contraction index on its rows, so its tiles pass
// through LDS and are read back transposed (2-byte reads); it is read once per 64 sequences.
static __global__ void __launch_bounds__(256) k_cls_key_fold(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Wk, int B,
                                                             int H, float scale, float* __restrict__ U) {
  __shared__ __attribute__((aligned(16))) bf16_t ws[64 * FOLD_LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, heads = H >> 6;
  const int b = blockIdx.x * FOLD_ROWS + wave * 16 + lr;
  const int bc = b < B ? b : B - 1;
  Frag8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks].q = *(const uint4*)(Q + (int64_t)bc * H + h * 64 + ks * 32 + g * 8);
  const bf16_t* wk = Wk + (int64_t)h * 64 * H;
  float* up = U + ((int64_t)bc * heads + h) * H;
  for (int n0 = 0; n0 < H; n0 += FOLD_NC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // 64 rows x 128 columns = 1024 16-byte pieces
      const int idx = i * 256 + tid, r = idx >> 4, c = (idx & 15) * 8;
      const uint4 v = *(const uint4*)(wk + (int64_t)r * H + n0 + c);
      *(uint2*)(ws + r * FOLD_LDW + c) = make_uint2(v.x, v.y);
      *(uint2*)(ws + r * FOLD_LDW + c + 4) = make_uint2(v.z, v.w);
    }
    __syncthreads();
#pragma unroll 2
    for (int nt = 0; nt < FOLD_NC / 16; ++nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16_t* wp = ws + (ks * 32 + g * 8) * FOLD_LDW + nt * 16 + lr;
        Frag8 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a.u[i] = (uint32_t)wp[(2 * i) * FOLD_LDW] | ((uint32_t)wp[(2 * i + 1) * FOLD_LDW] << 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, qf[ks].v, acc, 0, 0, 0);
      }
      if (b < B) *(float4*)(up + n0 + nt * 16 + g * 4) = make_float4(scale * acc[0], scale * acc[1], scale * acc[2], scale * acc[3]);
    }
  }
}

// ctx[b, 64 h + j] = sum_k Wv[64 h + j, k] Z[b, h, k] + bv[64 h + j].  grid (ceil(B / 64), heads), 256 threads.
// Both operands have the contraction index contiguous: fragments come straight from global memory (Wv from cache:
// a head's 64 rows are shared by the four waves and read once per 64 sequences from L2).
static __global__ void __launch_bounds__(256) k_cls_value_fold(const float* __restrict__ Z, const bf16_t* __restrict__ Wv,
                                                               const float* __restrict__ bv, int B, int H,
                                                               bf16_t* __restrict__ ctx) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, heads = H >> 6;
  const int b = blockIdx.x * FOLD_ROWS + wave * 16 + lr;
  const int bc = b < B ? b : B - 1;
  const float* zp = Z + ((int64_t)bc * heads + h) * H + g * 8;
  const bf16_t* wv = Wv + ((int64_t)h * 64 + lr) * H + g * 8;
  f32x4 acc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < H; k0 += 128) {   // H % 128 == 0; the four steps' loads of Z are issued together
    f32x4 z[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      z[2 * i] = __builtin_nontemporal_load((const f32x4*)(zp + k0 + i * 32));
      z[2 * i + 1] = __builtin_nontemporal_load((const f32x4*)(zp + k0 + i * 32 + 4));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x[8] = {z[2 * i][0], z[2 * i][1], z[2 * i][2], z[2 * i][3], z[2 * i + 1][0], z[2 * i + 1][1], z[2 * i + 1][2], z[2 * i + 1][3]};
      Frag8 zh, zl;
      split_bf16x8(x, zh, zl);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        Frag8 a;
        a.q = *(const uint4*)(wv + (int64_t)mt * 16 * H + k0 + i * 32);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, zh.v, acc[mt], 0, 0, 0);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, zl.v, acc[mt], 0, 0, 0);
      }
    }
  }
  if (b >= B) return;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int j0 = h * 64 + mt * 16 + g * 4;
    const float4 bias = *(const float4*)(bv + j0);
    uint2 o;
    o.x = pack_bf16x2(acc[mt][0] + bias.x, acc[mt][1] + bias.y);
    o.y = pack_bf16x2(acc[mt][2] + bias.z, acc[mt][3] + bias.w);
    *(uint2*)(ctx + (int64_t)b * H + j0) = o;
  }
}

constexpr int POOL_T = 32;   // tokens per step of the pool kernel = the contraction length of one MFMA
template <int HC>
constexpr int pool_smem_bytes() { return POOL_T * (128 * HC + 4) * 2 + 4 * POOL_T * 16 * 4; }

// Z[b, h, :] = sum_t p_t x_t,  p = softmax_t(U[b, h, :] . x_t) over the sequence's `len` tokens.  H = 128 HC, heads = 2 HC.
// One workgroup (4 waves) per sequence streams its rows of X once, POOL_T at a time, through LDS (the next step's rows
// are in flight in registers meanwhile) with an online softmax:
//   scores   S[t, h] = sum_k X[t, k] U[h, k]: tokens on M, heads on N; each wave contracts its quarter of H against the
//            U fragments it holds for the whole kernel, the four partial sums meet in LDS and are added in wave order;
//   softmax  every lane owns head (lane & 15) and tokens 8 (lane >> 4) .. + 7 -- the B fragment of the second product;
//            running max / sum per head, tokens at or past `len` get weight 0 (their LDS rows are zero, never loaded);
//   pool     Z^T[n, h] += sum_t X[t, n] P[t, h]: features on M (each wave its quarter of H, X read back transposed),
//            heads on N, so the rescale by exp(m_old - m_new) is per lane.
template <int HC>
static __global__ void __launch_bounds__(256, HC <= 6 ? 2 : 1) k_cls_pool(const bf16_t* __restrict__ X, const float* __restrict__ U,
                                                         const int32_t* __restrict__ cu, const int32_t* __restrict__ lens,
                                                         float* __restrict__ Z) {
  constexpr int H = 128 * HC, LDX = H + 4, HEADS = 2 * HC, NLD = H / 64, HQ = H / 4, RP = H / 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
  bf16_t* xs = (bf16_t*)pool_smem;                          // [POOL_T][LDX]
  float* sp = (float*)(pool_smem + POOL_T * LDX * 2);       // [4 waves][POOL_T][16 heads]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const int64_t base = cu[b];
  const int len = lens[b];
  const int nchunks = (len + POOL_T - 1) / POOL_T;

  u32x4_t pre[NLD];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + tid, r = idx / RP, cs = idx % RP, t = c * POOL_T + r;
      pre[i] = u32x4_t{0u, 0u, 0u, 0u};
      if (t < len) pre[i] = __builtin_nontemporal_load((const u32x4_t*)(X + (base + t) * H + cs * 8));
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + tid, r = idx / RP, cs = idx % RP;
      *(uint2*)(xs + r * LDX + cs * 8) = make_uint2(pre[i][0], pre[i][1]);
      *(uint2*)(xs + r * LDX + cs * 8 + 4) = make_uint2(pre[i][2], pre[i][3]);
    }
  };
  fetch(0);

  // this wave's quarter of U[b, head lr, :] (heads past HEADS: zero columns, never stored)
  Frag8 uh[HC], ul[HC];
  {
    const float* up = U + ((int64_t)b * HEADS + (lr < HEADS ? lr : 0)) * H + wave * HQ + g * 8;
#pragma unroll
    for (int ks = 0; ks < HC; ++ks) {
      const f32x4 u0 = __builtin_nontemporal_load((const f32x4*)(up + ks * 32));
      const f32x4 u1 = __builtin_nontemporal_load((const f32x4*)(up + ks * 32 + 4));
      const float m = lr < HEADS ? 1.f : 0.f;
      const float x[8] = {m * u0[0], m * u0[1], m * u0[2], m * u0[3], m * u1[0], m * u1[1], m * u1[2], m * u1[3]};
      split_bf16x8(x, uh[ks], ul[ks]);
    }
  }
  f32x4 acc[NLD];
#pragma unroll
  for (int nt = 0; nt < NLD; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  stash();
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    if (c + 1 < nchunks) fetch(c + 1);
    // partial scores of this wave's quarter of the contraction
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      const bf16_t* xp = xs + (mt * 16 + lr) * LDX + wave * HQ + g * 8;
#pragma unroll
      for (int ks = 0; ks < HC; ++ks) {
        Frag8 a;
        a.d[0] = *(const uint2*)(xp + ks * 32);
        a.d[1] = *(const uint2*)(xp + ks * 32 + 4);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, uh[ks].v, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, ul[ks].v, s, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) sp[(wave * POOL_T + mt * 16 + g * 4 + i) * 16 + lr] = s[i];
    }
    __syncthreads();
    // head lr, tokens 8 g .. 8 g + 7 of this step (every wave computes the same values)
    float sv[8], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = g * 8 + j;
      float v = sp[t * 16 + lr];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += sp[(w * POOL_T + t) * 16 + lr];
      sv[j] = c * POOL_T + t < len ? v : -INFINITY;
      mx = fmaxf(mx, sv[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);        // finite: token c * POOL_T of this step is below len
    const float alpha = __expf(m_run - m_new);   // 0 on the first step
    float pv[8], ps = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pv[j] = __expf(sv[j] - m_new);
      ps += pv[j];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * alpha + ps;
    m_run = m_new;
    Frag8 ph, pl;
    split_bf16x8(pv, ph, pl);
#pragma unroll
    for (int nt = 0; nt < NLD; ++nt) {
      const bf16_t* xp = xs + (g * 8) * LDX + wave * HQ + nt * 16 + lr;
      Frag8 a;
#pragma unroll
      for (int i = 0; i < 4; ++i) a.u[i] = (uint32_t)xp[(2 * i) * LDX] | ((uint32_t)xp[(2 * i + 1) * LDX] << 16);
      acc[nt] *= alpha;
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, ph.v, acc[nt], 0, 0, 0);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, pl.v, acc[nt], 0, 0, 0);
    }
    __syncthreads();
    if (c + 1 < nchunks) {
      stash();
      __syncthreads();
    }
  }
  if (lr < HEADS) {
    const float inv = 1.f / l_run;
    float* zp = Z + ((int64_t)b * HEADS + lr) * H + wave * HQ + g * 4;
#pragma unroll
    for (int nt = 0; nt < NLD; ++nt)
      *(float4*)(zp + nt * 16) = make_float4(acc[nt][0] * inv, acc[nt][1] * inv, acc[nt][2] * inv, acc[nt][3] * inv);
  }
}

template <int HC>
static int launch_cls_pool_hc(const bf16_t* X, const float* U, const int32_t* cu, const int32_t* lens, int B, float* Z, hipStream_t st) {
  static DeviceOnce attr_done;
  if (attr_done.first())
    CONVDR_CHECK_HIP(hipFuncSetAttribute((const void*)k_cls_pool<HC>, hipFuncAttributeMaxDynamicSharedMemorySize, pool_smem_bytes<HC>()));
  hipLaunchKernelGGL(k_cls_pool<HC>, dim3(B), dim3(256), pool_smem_bytes<HC>(), st, X, U, cu, lens, Z);
  CONVDR_CHECK_LAUNCH("k_cls_pool");
  return 0;
}

static int launch_cls_pool(const bf16_t* X, const float* U, const int32_t* cu, const int32_t* lens, int B, int H, float* Z,
                           hipStream_t st) {
  switch (H / 128) {
    case 1: return launch_cls_pool_hc<1>(X, U, cu, lens, B, Z, st);
    case 2: return launch_cls_pool_hc<2>(X, U, cu, lens, B, Z, st);
    case 3: return launch_cls_pool_hc<3>(X, U, cu, lens, B, Z, st);
    case 4: return launch_cls_pool_hc<4>(X, U, cu, lens, B, Z, st);
    case 5: return launch_cls_pool_hc<5>(X, U, cu, lens, B, Z, st);
    case 6: return launch_cls_pool_hc<6>(X, U, cu, lens, B, Z, st);
    case 7: return launch_cls_pool_hc<7>(X, U, cu, lens, B, Z, st);
    case 8: return launch_cls_pool_hc<8>(X, U, cu, lens, B, Z, st);
  }
  set_error("cls fold: hidden %d is not a multiple of 128 <= 1024", H);
  return -1;
}

}  // namespace convdr
