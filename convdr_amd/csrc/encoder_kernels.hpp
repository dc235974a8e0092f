// Device kernels of the BERT/RoBERTa dual-encoder forward on gfx950 (shared by encoder.hip and train.hip).  Here: the pack, embedding,
// LayerNorm, gather and cast row kernels; the GEMM with fused epilogues is gemm_kernel.hpp, the self-attention attention_fwd.hpp (both
// included below, so an includer of this file sees every forward kernel).
//
// Replaces the third-party arithmetic behind  self.roberta(input_ids, attention_mask)
// (/root/reference/model/models.py:141-142) and BertModel.forward (:208-209): HF transformers==2.3.0
// embeddings + 12 x [self-attention, output dense + residual + LayerNorm, FFN + residual + LayerNorm].
//
// Data layout in HBM ("packed rows"): only tokens with attention_mask == 1 are computed.  Sequence b owns
// rows [cu[b], cu[b] + len[b]) of every [rows, *] activation matrix; cu[b] is a multiple of 8 so that 16-byte
// accesses along the token axis stay aligned.  CLS-only pooling (models.py:43, use_mean = False for every
// registered config) makes this identical to the reference's padded computation (SURVEY.md §7 hard part 7).
//   X    [rows, H]  bf16   layer input / LayerNorm output (MFMA operand and residual)
//   Y    [rows, H]  f32    pre-LayerNorm sums (GEMM epilogue output, LayerNorm input)
//   Q, K [rows, H]  bf16   row-major, head h = columns [64 h, 64 h + 64)
//   Vt   [H, ldt]   bf16   V transposed (feature-major, token-contiguous): the P.V contraction runs over keys,
//                          and MFMA wants the contraction index contiguous per lane, so the QKV GEMM epilogue
//                          writes V already transposed instead of transposing it inside the attention kernel
//   ctx  [rows, H]  bf16   attention output
//   Hm   [rows, I]  bf16   gelu(FFN1)
#pragma once
#include <type_traits>

#include "../../include/convdr_hip.h"
#include "attention_fwd.hpp"   // k_attention_fwd
#include "dropout.hpp"
#include "gemm_kernel.hpp"     // k_gemm and its epilogues
#include "gemm_nt.hpp"

namespace convdr {

// ---------------------------------------------------------------------------------------------
// pack: one wave per sequence.  Compacts the mask == 1 tokens of ids[b, :] to rows cu[b]..; position ids:
//   RoBERTa: cumsum(ids != pad_idx) * (ids != pad_idx) + pad_idx over the FULL row (masked positions count,
//            the reference pads with id 0 which is not RoBERTa's pad id 1 -- utils/util.py:146-185);
//   BERT:    the column index.
// Alignment rows [cu[b] + len, cu[b+1]) get token id -1 (embedding kernel writes zeros).
// ---------------------------------------------------------------------------------------------
// ids: int64 [B, L] (the drivers' .long() tensors) or int32 [B, L] (token-cache records, ids32 != 0);
// mask == nullptr means "prefix mask": position l is kept iff l < lens[b] (right padding).
static __global__ void __launch_bounds__(256) k_seq_pack(const void* __restrict__ ids_v, int ids32,
                                                  const int64_t* __restrict__ mask, const int32_t* __restrict__ lens,
                                                  int B, int L, const int32_t* __restrict__ cu, int kind, int pad_idx,
                                                  int max_pos, int vocab, int32_t* __restrict__ tok_id,
                                                  int32_t* __restrict__ tok_pos, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int base = cu[b], end = cu[b + 1];
  const int64_t* ids = (const int64_t*)ids_v;
  const int32_t* ids_i = (const int32_t*)ids_v;
  const int len_b = lens[b];
  int kept = 0, nonpad = 0;
  int flags = 0;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    const bool valid = l < L;
    int64_t id = valid ? (ids32 ? (int64_t)ids_i[(int64_t)b * L + l] : ids[(int64_t)b * L + l]) : (int64_t)pad_idx;
    const bool m = valid && (mask ? mask[(int64_t)b * L + l] != 0 : l < len_b);
    if (l == 0 && !m) flags |= CONVDR_ENC_STATUS_BAD_MASK;   // the CLS position must be unmasked
    const bool np = valid && id != pad_idx;
    const unsigned long long bm = __ballot(m), bnp = __ballot(np);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (m) {
      // The reference's embedding lookup raises IndexError for an id outside the table (models.py:141-142 -> nn.Embedding).
      // Here the id is clamped (no out-of-bounds read or atomic in the backward) and the batch is flagged; the host
      // raises at its next look at the status word.
      if (id < 0 || id >= (int64_t)vocab) { flags |= CONVDR_ENC_STATUS_BAD_TOKEN; id = 0; }
      const int row = base + kept + __popcll(bm & lt);
      if (row < end) {
        int p = kind == 0 ? (np ? nonpad + __popcll(bnp & (lt | (1ull << lane))) + pad_idx : pad_idx) : l;
        p = p < max_pos ? p : max_pos - 1;
        tok_id[row] = (int)id;
        tok_pos[row] = p;
      }
    }
    kept += __popcll(bm);
    nonpad += __popcll(bnp);
  }
  if (kept != len_b) flags |= CONVDR_ENC_STATUS_BAD_LENS;    // seq_lens[b] != mask[b].sum() (or > L)
  if (__ballot(flags != 0) != 0ull) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) flags |= __shfl_xor(flags, o, 64);
    if (lane == 0) atomicOr(status, flags);
  }
  for (int r = base + kept + lane; r < end; r += 64) {
    tok_id[r] = -1;
    tok_pos[r] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// pack, ragged input: one wave per sequence.  tokens[off[b] .. off[b+1]) are the UNMASKED tokens of sequence b, back to
// back with no padding between sequences; they go to rows cu[b].., and tok_id / tok_pos / status get exactly what k_seq_pack
// writes for the same sequences stored right-padded in a [B, L] matrix.
// Why the flat stream is enough: the reference's RoBERTa position of token l is
//   cumsum(ids[0..l] != pad_idx) * (ids[l] != pad_idx) + pad_idx   over the padded row,
// which depends only on the ids at or before l; under a prefix (right-padding) mask every one of those is a kept token, so
// the padding behind the sequence never enters a kept token's position.  (BERT: the index inside the sequence.)  A mask with
// holes has masked ids BEFORE kept ones, is not representable as a stream, and stays with k_seq_pack.
// Hardening: the offsets come from the caller.  A sequence is read only if 0 <= off[b] <= off[b+1] <= n_tokens,
// off[b+1] - off[b] == lens[b] and 1 <= lens[b] <= cu[b+1] - cu[b]; otherwise it is flagged CONVDR_ENC_STATUS_BAD_LENS, nothing
// of `tokens` is read for it and all its rows get id -1 / position 0.  So no read goes past tokens + n_tokens.
// ---------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_seq_pack_ragged(const int32_t* __restrict__ tokens, int64_t n_tokens,
                                                         const int32_t* __restrict__ off, const int32_t* __restrict__ lens,
                                                         int B, const int32_t* __restrict__ cu, int kind, int pad_idx,
                                                         int max_pos, int vocab, int32_t* __restrict__ tok_id,
                                                         int32_t* __restrict__ tok_pos, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int base = cu[b], end = cu[b + 1];
  const int64_t o0 = off[b], o1 = off[b + 1];
  const int len_b = lens[b];
  const bool ok = o0 >= 0 && o0 <= o1 && o1 <= n_tokens && o1 - o0 == (int64_t)len_b && len_b >= 1 &&
                  (int64_t)len_b <= (int64_t)end - (int64_t)base;
  const int n = ok ? len_b : 0;
  int kept = 0, nonpad = 0;
  int flags = ok ? 0 : CONVDR_ENC_STATUS_BAD_LENS;
  for (int l0 = 0; l0 < n; l0 += 64) {
    const int l = l0 + lane;
    const bool m = l < n;
    int id = m ? tokens[o0 + l] : pad_idx;
    const bool np = m && id != pad_idx;
    const unsigned long long bm = __ballot(m), bnp = __ballot(np);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (m) {
      if (id < 0 || id >= vocab) { flags |= CONVDR_ENC_STATUS_BAD_TOKEN; id = 0; }   // clamped + flagged, as in k_seq_pack
      const int row = base + kept + __popcll(bm & lt);
      int p = kind == 0 ? (np ? nonpad + __popcll(bnp & (lt | (1ull << lane))) + pad_idx : pad_idx) : l;
      p = p < max_pos ? p : max_pos - 1;
      tok_id[row] = id;
      tok_pos[row] = p;
    }
    kept += __popcll(bm);
    nonpad += __popcll(bnp);
  }
  if (__ballot(flags != 0) != 0ull) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) flags |= __shfl_xor(flags, o, 64);
    if (lane == 0) atomicOr(status, flags);
  }
  for (int r = base + kept + lane; r < end; r += 64) {
    tok_id[r] = -1;
    tok_pos[r] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm helpers: one wave per row, H <= 1024, H % 4 == 0; lane owns elements 256 j + 4 lane + c.
// Biased variance, eps inside the sqrt (torch.nn.LayerNorm).
// ---------------------------------------------------------------------------------------------
struct LnRow {
  float4 v[4];
};

__device__ __forceinline__ void ln_normalize(LnRow& x, int H, int lane, float eps, const float* __restrict__ g,
                                             const float* __restrict__ b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (256 * j + 4 * lane < H) s += x.v[j].x + x.v[j].y + x.v[j].z + x.v[j].w;
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (256 * j + 4 * lane < H) {
      const float a = x.v[j].x - mean, c = x.v[j].y - mean, d = x.v[j].z - mean, e = x.v[j].w - mean;
      q += a * a + c * c + d * d + e * e;
    }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e0 = 256 * j + 4 * lane;
    if (e0 < H) {
      const float4 gg = *(const float4*)(g + e0), bb = *(const float4*)(b + e0);
      x.v[j].x = (x.v[j].x - mean) * rstd * gg.x + bb.x;
      x.v[j].y = (x.v[j].y - mean) * rstd * gg.y + bb.y;
      x.v[j].z = (x.v[j].z - mean) * rstd * gg.z + bb.z;
      x.v[j].w = (x.v[j].w - mean) * rstd * gg.w + bb.w;
    }
  }
}

__device__ __forceinline__ void ln_store(const LnRow& x, int H, int lane, bf16_t* __restrict__ xb,
                                         float* __restrict__ xf) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e0 = 256 * j + 4 * lane;
    if (e0 < H) {
      if (xb) {
        uint2 o;
        o.x = pack_bf16x2(x.v[j].x, x.v[j].y);
        o.y = pack_bf16x2(x.v[j].z, x.v[j].w);
        *(uint2*)(xb + e0) = o;
      }
      if (xf) *(float4*)(xf + e0) = x.v[j];
    }
  }
}

// embeddings: LayerNorm(word[id] + pos[p] + type[0]) -> bf16 X
static __global__ void __launch_bounds__(256) k_embed_ln(const int32_t* __restrict__ tok_id,
                                                  const int32_t* __restrict__ tok_pos, int64_t rows, int H,
                                                  const float* __restrict__ word, const float* __restrict__ pos,
                                                  const float* __restrict__ type0, const float* __restrict__ g,
                                                  const float* __restrict__ b, float eps, bf16_t* __restrict__ X,
                                                  const DropSite drop) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int id = tok_id[row];
  LnRow x;
  if (id < 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    ln_store(x, H, lane, X + row * H, nullptr);
    return;
  }
  const float* w = word + (int64_t)id * H;
  const float* p = pos + (int64_t)tok_pos[row] * H;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e0 = 256 * j + 4 * lane;
    if (e0 < H) {
      const float4 a = *(const float4*)(w + e0), c = *(const float4*)(p + e0), t = *(const float4*)(type0 + e0);
      x.v[j] = make_float4(a.x + c.x + t.x, a.y + c.y + t.y, a.z + c.z + t.z, a.w + c.w + t.w);
    }
  }
  ln_normalize(x, H, lane, eps, g, b);
  if (drop.thresh) {   // embedding dropout (training)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e0 = 256 * j + 4 * lane;
      if (e0 < H) {
        float m0, m1, m2, m3;
        drop_hidden4(drop, row, e0, H, m0, m1, m2, m3);
        x.v[j].x *= m0; x.v[j].y *= m1; x.v[j].z *= m2; x.v[j].w *= m3;
      }
    }
  }
  ln_store(x, H, lane, X + row * H, nullptr);
}

// rows of fp32 Y -> LayerNorm -> bf16 Xb (and/or fp32 Xf).  `gather` (optional) maps output row -> input row.
static __global__ void __launch_bounds__(256) k_layernorm(const float* __restrict__ Y, int64_t rows, int H,
                                                   const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                   bf16_t* __restrict__ Xb, float* __restrict__ Xf) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  LnRow x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e0 = 256 * j + 4 * lane;
    if (e0 < H) x.v[j] = *(const float4*)(Y + row * H + e0);
  }
  ln_normalize(x, H, lane, eps, g, b);
  ln_store(x, H, lane, Xb ? Xb + row * H : nullptr, Xf ? Xf + row * H : nullptr);
}

// The same for H == 256 J with the bf16 output only (the encoder layers' case), as straight-line code: the kernel above keeps
// each 16-byte group behind an `e0 < H` guard, and hipcc gives every guarded load of gamma / beta -- which it cannot hoist
// over the guard -- its own block and its own s_waitcnt behind the two row reductions: three dependent L2 round trips per
// row.  Here the row, gamma and beta are requested together.  Same formulas (see k_layernorm_bwd_rows, train_kernels.hpp).
template <int J>
static __global__ void __launch_bounds__(256) k_layernorm_rows(const float* __restrict__ Y, int64_t rows,
                                                               const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                               bf16_t* __restrict__ Xb) {
  constexpr int H = 256 * J;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 x[J], gg[J], bb[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int e0 = 256 * j + 4 * lane;
    x[j] = *(const float4*)(Y + row * H + e0);
    gg[j] = *(const float4*)(g + e0);
    bb[j] = *(const float4*)(b + e0);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) s += x[j].x + x[j].y + x[j].z + x[j].w;
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float a = x[j].x - mean, c = x[j].y - mean, d = x[j].z - mean, e = x[j].w - mean;
    q += a * a + c * c + d * d + e * e;
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int e0 = 256 * j + 4 * lane;
    uint2 o;
    o.x = pack_bf16x2((x[j].x - mean) * rstd * gg[j].x + bb[j].x, (x[j].y - mean) * rstd * gg[j].y + bb[j].y);
    o.y = pack_bf16x2((x[j].z - mean) * rstd * gg[j].z + bb[j].z, (x[j].w - mean) * rstd * gg[j].w + bb[j].w);
    *(uint2*)(Xb + row * H + e0) = o;
  }
}

// Split-contraction projection + residual + LayerNorm for FEW rows (H == 256 J): a K = 3072 projection of a few thousand rows is
// 126 workgroups of 48 K steps -- a latency chain on a quarter of the chip (the frozen teacher's 64 x ~40-token targets, a query
// batch of the evaluation loop).  The launcher cuts the contraction into `nsplit` slices (EPI_SLAB_F32: slab[s][row][H], no
// bias), and this kernel finishes them: y = bias + sum_s slab[s] (fixed order) + residual, X = LayerNorm(y) -> bf16.
template <int J>
static __global__ void __launch_bounds__(256) k_slab_finish_ln(const float* __restrict__ slab, int nsplit, int64_t rows,
                                                               const float* __restrict__ bias, const bf16_t* __restrict__ R,
                                                               const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                               bf16_t* __restrict__ Xb) {
  constexpr int H = 256 * J;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 x[J], gg[J], bb[J], part[4][J];
  uint2 r[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int e0 = 256 * j + 4 * lane;
    x[j] = *(const float4*)(bias + e0);
    gg[j] = *(const float4*)(g + e0);
    bb[j] = *(const float4*)(b + e0);
    r[j] = *(const uint2*)(R + row * H + e0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      part[s][j] = *(const float4*)(slab + ((int64_t)(s < nsplit ? s : 0) * rows + row) * H + e0);   // (clamped: no branch around a load)
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < nsplit) { x[j].x += part[s][j].x; x[j].y += part[s][j].y; x[j].z += part[s][j].z; x[j].w += part[s][j].w; }
    x[j].x += __uint_as_float(r[j].x << 16); x[j].y += __uint_as_float(r[j].x & 0xffff0000u);
    x[j].z += __uint_as_float(r[j].y << 16); x[j].w += __uint_as_float(r[j].y & 0xffff0000u);
    sum += x[j].x + x[j].y + x[j].z + x[j].w;
  }
  const float mean = wave_sum(sum) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float a = x[j].x - mean, c = x[j].y - mean, d = x[j].z - mean, e = x[j].w - mean;
    q += a * a + c * c + d * d + e * e;
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int e0 = 256 * j + 4 * lane;
    uint2 o;
    o.x = pack_bf16x2((x[j].x - mean) * rstd * gg[j].x + bb[j].x, (x[j].y - mean) * rstd * gg[j].y + bb[j].y);
    o.y = pack_bf16x2((x[j].z - mean) * rstd * gg[j].z + bb[j].z, (x[j].w - mean) * rstd * gg[j].w + bb[j].w);
    *(uint2*)(Xb + row * H + e0) = o;
  }
}

// fp32 rows -> LayerNorm -> bf16 rows: the straight-line kernel where it applies (convdr_set_option "ln_rows" 0: never)
inline int64_t g_ln_rows = 1;
static inline void launch_layernorm_bf16(const float* Y, int64_t rows, int H, const float* g, const float* b, float eps, bf16_t* Xb,
                                         hipStream_t st) {
  if (g_ln_rows && H == 768)
    hipLaunchKernelGGL(k_layernorm_rows<3>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, Y, rows, g, b, eps, Xb);
  else
    hipLaunchKernelGGL(k_layernorm, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, Y, rows, H, g, b, eps, Xb, (float*)nullptr);
}

// out[b, :] = in[cu[b], :]  (CLS rows), bf16 and/or fp32
static __global__ void __launch_bounds__(256) k_gather_cls(const int32_t* __restrict__ cu, int B, int H,
                                                    const bf16_t* __restrict__ Xb, const float* __restrict__ Xf,
                                                    bf16_t* __restrict__ Ob, float* __restrict__ Of) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t row = cu[b];
  for (int e0 = 4 * lane; e0 < H; e0 += 256) {
    if (Ob) *(uint2*)(Ob + (int64_t)b * H + e0) = *(const uint2*)(Xb + row * H + e0);
    if (Of) *(float4*)(Of + (int64_t)b * H + e0) = *(const float4*)(Xf + row * H + e0);
  }
}

// EmbeddingMixin.masked_mean (models.py:32-35): out[b, :] = sum over the sequence's tokens of X[row, :] / len[b].
// One workgroup per sequence; thread t owns columns 4 t .. 4 t + 3 (H <= 1024); rows are read whole (coalesced).
static __global__ void __launch_bounds__(256) k_masked_mean(const bf16_t* __restrict__ X, const int32_t* __restrict__ cu,
                                                     const int32_t* __restrict__ lens, int H, bf16_t* __restrict__ Ob,
                                                     float* __restrict__ Of) {
  const int b = blockIdx.x, c = 4 * threadIdx.x;
  if (c >= H) return;
  const int64_t base = cu[b];
  const int len = lens[b];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = 0; t < len; ++t) {
    const uint2 v = *(const uint2*)(X + (base + t) * H + c);
    s.x += __uint_as_float(v.x << 16); s.y += __uint_as_float(v.x & 0xffff0000u);
    s.z += __uint_as_float(v.y << 16); s.w += __uint_as_float(v.y & 0xffff0000u);
  }
  const float inv = 1.f / (float)len;
  s.x *= inv; s.y *= inv; s.z *= inv; s.w *= inv;
  if (Of) *(float4*)(Of + (int64_t)b * H + c) = s;
  if (Ob) {
    uint2 o;
    o.x = pack_bf16x2(s.x, s.y);
    o.y = pack_bf16x2(s.z, s.w);
    *(uint2*)(Ob + (int64_t)b * H + c) = o;
  }
}

// fp32 rows -> bf16 rows (weight packing at load / after each optimizer step)
static __global__ void __launch_bounds__(256) k_cast_f32_bf16(const float* __restrict__ x, bf16_t* __restrict__ y, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = *(const float4*)(x + 4 * i);
    uint2 o;
    o.x = pack_bf16x2(v.x, v.y);
    o.y = pack_bf16x2(v.z, v.w);
    *(uint2*)(y + 4 * i) = o;
  }
}

}  // namespace convdr
