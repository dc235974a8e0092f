// Preparing operands for the similarity scan (included by ip_topk.hip after its constants): rows fp32 -> 16-bit scan
// operand with norms (k_rows_to_half: blocks and queries, bf16 and fp16), the half store (k_store_rows_f16), the column mean
// a block is centred by, the 8-bit store (column steps, codes, the queries' int8 operands), and the fill kernel of a given
// threshold.  The entries that launch them are in ip_topk.hip.
#pragma once

namespace convdr {

// ------------------------------------------------------------------------------------------
// rows fp32 -> bf16 of (x - centre) (+ per-row L2 norm of the centred row, + global max norm).
// Optional second output: the bf16 of the rounding remainder (x - centre) - hi, for the split-bf16 scan.
// One wave per row, float4 loads.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
  const f16x2_t r = {(_Float16)lo, (_Float16)hi};   // v_cvt_pkrtz is NOT used: round to nearest even
  return *(const uint32_t*)&r;
}
template <int KIND>
__device__ __forceinline__ uint32_t pack_half2(float lo, float hi) {
  return KIND == IP_KIND_F16 ? pack_f16x2(lo, hi) : pack_bf16x2(lo, hi);
}
template <int KIND>
__device__ __forceinline__ float half_lo_to_f32(uint32_t packed) {
  if constexpr (KIND == IP_KIND_F16) { const uint16_t h = (uint16_t)packed; return (float)*(const _Float16*)&h; }
  return bf16_to_f32((bf16_t)packed);
}
template <int KIND>
__device__ __forceinline__ float half_hi_to_f32(uint32_t packed) {
  if constexpr (KIND == IP_KIND_F16) { const uint16_t h = (uint16_t)(packed >> 16); return (float)*(const _Float16*)&h; }
  return bf16_to_f32((bf16_t)(packed >> 16));
}

// PER_ROW_SCALE (queries of the fp16 scan): every row is multiplied by its own power of two 2^(12 - e), |row| = m 2^e
// with m in [0.5, 1) (frexpf of the fp32 norm), so its scaled norm lies in [2^11, 2^12) -- one binade below the block's
// [2^12, 2^13), see IP_F16_TARGET_EXP; tests/test_scan_error_gpu.py asserts the interval.  row_norm receives the SCALED norm.  Otherwise `scale`
// (a power of two; 1 for bf16) multiplies every row and row_norm / max_norm are UNSCALED.
template <int KIND, bool PER_ROW_SCALE>
__global__ void __launch_bounds__(256) k_rows_to_half(const float* __restrict__ X, int64_t n, int d,
                                                      const float* __restrict__ centre, float scale, bf16_t* __restrict__ Y,
                                                      bf16_t* __restrict__ Ylo, float* __restrict__ row_norm,
                                                      float* __restrict__ max_norm, int64_t n_pad = 0,
                                                      uint32_t* __restrict__ zero_u32 = nullptr, int64_t zero_count = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wmax = 0.f;
  // query preparation of a search: the padding rows [n, n_pad) of Y / Ylo and the candidate counters are zeroed here
  // instead of by three memsets in front of this kernel (a search of <= 128 queries is a chain of short launches)
  for (int64_t row = n + (int64_t)blockIdx.x * 4 + wave; row < n_pad; row += (int64_t)gridDim.x * 4)
    for (int e = lane * 4; e < d; e += 256) {
      *(uint2*)(Y + row * d + e) = make_uint2(0u, 0u);
      if (Ylo) *(uint2*)(Ylo + row * d + e) = make_uint2(0u, 0u);
    }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < zero_count; i += (int64_t)gridDim.x * 256) zero_u32[i] = 0u;
  // Norms are summed in fp64: eps is proportional to them, and in fp32 the squares of elements below ~1e-19 underflow
  // (a block of tiny-magnitude embeddings would get norm 0 = "no rounding error").  The pass is HBM-bound either way.
  auto sq4 = [](const float4& v) {
    return (double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z + (double)v.w * (double)v.w;
  };
  auto wave_sum_f64 = [](double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
    const float* x = X + row * d;
    double ss = 0.0;
    float sc = scale;
    if constexpr (PER_ROW_SCALE) {
      for (int e = lane * 4; e < d; e += 256) ss += sq4(*(const float4*)(x + e));
      ss = wave_sum_f64(ss);
      int ex = 0;
      const float nm0 = (float)sqrt(ss);
      (void)frexpf(nm0, &ex);
      int sh = (int)IP_F16_TARGET_EXP - ex;
      sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
      sc = (nm0 > 0.f && nm0 < INFINITY) ? ldexpf(1.f, sh) : 1.f;
      ss = 0.0;
    }
    for (int e = lane * 4; e < d; e += 256) {
      float4 v = *(const float4*)(x + e);
      if (centre) {
        const float4 c = *(const float4*)(centre + e);
        v.x -= c.x; v.y -= c.y; v.z -= c.z; v.w -= c.w;
      }
      if constexpr (PER_ROW_SCALE) { v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
      ss += sq4(v);
      if (Y) {
        if constexpr (!PER_ROW_SCALE && KIND == IP_KIND_F16) { v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
        uint2 o;
        o.x = pack_half2<KIND>(v.x, v.y);
        o.y = pack_half2<KIND>(v.z, v.w);
        *(uint2*)(Y + row * d + e) = o;
        if (Ylo) {
          uint2 l;
          l.x = pack_half2<KIND>(v.x - half_lo_to_f32<KIND>(o.x), v.y - half_hi_to_f32<KIND>(o.x));
          l.y = pack_half2<KIND>(v.z - half_lo_to_f32<KIND>(o.y), v.w - half_hi_to_f32<KIND>(o.y));
          *(uint2*)(Ylo + row * d + e) = l;
        }
      }
    }
    ss = wave_sum_f64(ss);
    const float nm = (float)(sqrt(ss) * (1.0 + 1e-6));   // (rounded up: a bound)
    if (row_norm && lane == 0) row_norm[row] = nm;
    wmax = fmaxf(wmax, nm);
  }
  if (max_norm) {
    __shared__ float sm[4];
    if (lane == 0) sm[wave] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
      atomicMax((int*)max_norm, __float_as_int(m));  // non-negative floats order like ints
    }
  }
}

// ------------------------------------------------------------------------------------------
// The half store: the passage IS its stored half v; the resident copy holds 2^s v (scale = 2^s, s >= 0), which is at once
// the corpus (re-scored in fp64 and multiplied by 2^-s, see k_ip_rescore) and the un-centred fp16 scan operand.
// src: rows of halves (kept bit for bit) or fp32 rows (rounded to nearest even once, here).  store = half * scale; the
// rows' UNSCALED norm is folded into *max_norm.  flags |= 1: a value is not finite (after rounding); flags |= 2: the
// scaled value left the half range or does not divide back to the half (scaling a half by 2^s, s >= 0, is exact,
// subnormals included, unless it overflows -- this is the check of that).  `store` may be `src` (halves): the in-place
// rescale by 2^(s_new - s_old) <= 1 with s_new >= 0, equally exact; a lane reads its 8 bytes before it writes them.
// store == nullptr: norms and flag 1 only.  One wave per row, 8- / 16-byte loads and 8-byte stores, no LDS.
// ------------------------------------------------------------------------------------------
template <bool SRC_F32>
__global__ void __launch_bounds__(256) k_store_rows_f16(const void* src, int64_t n, int d, float scale, float inv_scale,
                                                        _Float16* store, float* __restrict__ max_norm,
                                                        int32_t* __restrict__ flags) {
  typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wmax = 0.f;
  int bad = 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
    double ss = 0.0;
    for (int e = lane * 4; e < d; e += 256) {
      f16x4_t h;
      if constexpr (SRC_F32) {
        const float4 v = *(const float4*)((const float*)src + row * d + e);
        h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};   // round to nearest even
      } else {
        const uint2 raw = *(const uint2*)((const _Float16*)src + row * d + e);
        h = *(const f16x4_t*)&raw;
      }
      f16x4_t o;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float f = (float)h[c];
        o[c] = (_Float16)(f * scale);          // fp32 product of a half and a power of two: exact; then one conversion
        // the sign comes from the source bits: a half of -0 stays -0 however the product above is contracted
        // (a multiply selected as a fused multiply-add with a +0 addend returns +0 for it)
        o[c] = __builtin_copysignf16(o[c], h[c]);
        const float back = (float)o[c];
        if (!(fabsf(f) <= 65504.f)) bad |= 1;
        else if (!(fabsf(back) <= 65504.f) || back * inv_scale != f) bad |= 2;
        ss += (double)f * (double)f;
      }
      if (store) *(uint2*)(store + row * d + e) = *(const uint2*)&o;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
    wmax = fmaxf(wmax, (float)(sqrt(ss) * (1.0 + 1e-6)));   // (rounded up: a bound; NaN rows raise flag 1 instead)
  }
  if (max_norm && lane == 0 && wmax > 0.f) atomicMax((int*)max_norm, __float_as_int(wmax));  // non-negative floats order like ints
  if (bad) atomicOr(flags, bad);
}

// column sums of fp32 rows: part[chunk][d]; grid (ceil(d / 256), chunks)
__global__ void __launch_bounds__(256) k_colsum_f32(const float* __restrict__ X, int64_t n, int d, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y;
  const int64_t t0 = per * blockIdx.y, t1 = t0 + per < n ? t0 + per : n;
  if (c >= d) return;
  float s = 0.f;
  for (int64_t t = t0; t < t1; ++t) s += X[t * d + c];
  part[(int64_t)blockIdx.y * d + c] = s;
}
__global__ void __launch_bounds__(256) k_colmean_finish(const float* __restrict__ part, int chunks, int d, int64_t n,
                                                        float* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  for (int p = 0; p < chunks; ++p) s += part[(int64_t)p * d + c];
  mean[c] = (float)(s / (double)n);
}

// ------------------------------------------------------------------------------------------
// The 8-bit store (storage="sq8"): the passage IS its row of d int8 codes, v_ij = fl(centre_j + fl(step_j c_ij)).
// ------------------------------------------------------------------------------------------
// column maxima of |x - centre| (fp32 subtraction, rounded once): part[chunk][d]; grid (ceil(d / 256), chunks), as k_colsum_f32
__global__ void __launch_bounds__(256) k_colabsdev_f32(const float* __restrict__ X, int64_t n, int d,
                                                       const float* __restrict__ centre, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y;
  const int64_t t0 = per * blockIdx.y, t1 = t0 + per < n ? t0 + per : n;
  if (c >= d) return;
  const float ce = centre[c];
  float m = 0.f;
  for (int64_t t = t0; t < t1; ++t) m = fmaxf(m, fabsf(__fsub_rn(X[t * d + c], ce)));
  part[(int64_t)blockIdx.y * d + c] = m;
}
// step[c] = max / 127 as fp32 (one IEEE division).  A quotient below the normal range (a column whose largest deviation is
// under 127 x 2^-126) counts as a constant column, step 0: every product step x code is then a normal number or zero, which
// the band's relative rounding bounds rely on.
__global__ void __launch_bounds__(256) k_colstep_finish(const float* __restrict__ part, int chunks, int d, float* __restrict__ step) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  float m = 0.f;
  for (int p = 0; p < chunks; ++p) m = fmaxf(m, part[(int64_t)p * d + c]);
  const float s = __fdiv_rn(m, 127.f);
  step[c] = s >= FLT_MIN ? s : 0.f;
}

// Rows fp32 -> codes c = clamp(rint((p - centre) / step), -127, 127) (fp32 subtraction and IEEE division, each rounded once,
// round half to even: numpy's float32 arithmetic gives the same codes); step 0: code 0; -128 is never written.  One wave per
// row, float4 loads, one 4-byte store per lane.  *max_l1 (float bits, atomicMax) takes the largest row sum of |c|, *flags |= 1
// for a value that is not finite, *saturated counts the values the clamp moved.
__global__ void __launch_bounds__(256) k_store_rows_q8(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ centre,
                                                       const float* __restrict__ step, int8_t* __restrict__ codes,
                                                       float* __restrict__ max_l1, int32_t* __restrict__ flags,
                                                       uint32_t* __restrict__ saturated) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int wmax = 0, bad = 0;
  uint32_t sat = 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
    int l1 = 0;
    for (int e = lane * 4; e < d; e += 256) {
      const float4 v = *(const float4*)(X + row * d + e);
      const float4 ce = *(const float4*)(centre + e);
      const float4 st = *(const float4*)(step + e);
      const float x[4] = {v.x, v.y, v.z, v.w}, c0[4] = {ce.x, ce.y, ce.z, ce.w}, s0[4] = {st.x, st.y, st.z, st.w};
      uint32_t packed = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(fabsf(x[i]) <= FLT_MAX)) bad = 1;
        int c = 0;
        if (s0[i] > 0.f) {
          const float t = rintf(__fdiv_rn(__fsub_rn(x[i], c0[i]), s0[i]));
          if (fabsf(t) > 127.f) ++sat;
          c = (int)fminf(fmaxf(t, -127.f), 127.f);      // (a NaN quotient comes from a non-finite value: flagged above)
        }
        l1 += c < 0 ? -c : c;
        packed |= (uint32_t)(uint8_t)(int8_t)c << (8 * i);
      }
      *(uint32_t*)(codes + row * d + e) = packed;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) l1 += __shfl_xor(l1, o, 64);
    wmax = l1 > wmax ? l1 : wmax;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sat += __shfl_xor(sat, o, 64);
  if (lane == 0 && wmax > 0) atomicMax((int*)max_l1, __float_as_int((float)wmax));   // (<= 127 x 1024: exact; non-negative floats order like ints)
  if (lane == 0 && sat) atomicAdd(saturated, sat);
  if (bad) atomicOr(flags, 1);
}

// Queries of the 8-bit store's scan, one wave per query.  q'_j = fl(q_j step_j); t the power of two with max |q'_j| / t in
// (8128, 16256]; Qi_j = rint(q'_j / t) = 128 hi_j + lo_j with hi = floor((Qi + 64) / 128) in [-127, 127] and lo in [-64, 63].
// Operand layout (ip_scan_q8.hpp): per 128 queries 256 rows of d int8 -- the query with local number l has its hi row at
// 64 (l >> 5) + (l & 31) and its lo row 32 rows further --, so that the two MFMA column tiles of a wave are hi and lo of the
// SAME 32 queries.  band[q] receives the query's own term A(q) of the error band (IpBand::eps, derivation in ip_certify.hpp),
// or +inf -- CONVDR_IP_RANGE -- for a query with a value that is not finite or with 0 < max |q'_j| < 2^-100.  The padding
// queries' rows and the hit counters are zeroed here, as k_rows_to_half does.
constexpr float IP_Q8_QMAX = 16256.f;          // 127 x 128
constexpr float IP_Q8_QFLOOR = 0x1p-100f;
__device__ __forceinline__ int64_t q8_query_row(int64_t q) {
  const int64_t l = q & 127;
  return (q >> 7) * 256 + (l >> 5) * 64 + (l & 31);
}
__global__ void __launch_bounds__(256) k_q8_queries(const float* __restrict__ Q, int64_t nq, int d, const float* __restrict__ centre,
                                                    const float* __restrict__ step, int8_t* __restrict__ Qhl,
                                                    float* __restrict__ band, int64_t nq_pad, uint32_t* __restrict__ zero_u32,
                                                    int64_t zero_count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < zero_count; i += (int64_t)gridDim.x * 256) zero_u32[i] = 0u;
  for (int64_t q = (int64_t)blockIdx.x * 4 + wave; q < nq_pad; q += (int64_t)gridDim.x * 4) {
    int8_t* hi_row = Qhl + q8_query_row(q) * d;
    int8_t* lo_row = hi_row + 32 * (int64_t)d;
    if (q >= nq) {
      for (int e = lane * 4; e < d; e += 256) { *(uint32_t*)(hi_row + e) = 0u; *(uint32_t*)(lo_row + e) = 0u; }
      if (lane == 0) band[q] = 0.f;
      continue;
    }
    const float* x = Q + q * d;
    float mx = 0.f;
    int bad = 0;
    for (int e = lane * 4; e < d; e += 256) {
      const float4 v = *(const float4*)(x + e);
      const float4 s = *(const float4*)(step + e);
      const float p[4] = {__fmul_rn(v.x, s.x), __fmul_rn(v.y, s.y), __fmul_rn(v.z, s.z), __fmul_rn(v.w, s.w)};
      const float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(fabsf(r[i]) <= FLT_MAX) || !(fabsf(p[i]) <= FLT_MAX)) bad = 1;
        mx = fmaxf(mx, fabsf(p[i]));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      bad |= __shfl_xor(bad, o, 64);
    }
    if (mx > 0.f && mx < IP_Q8_QFLOOR) bad = 1;
    int te = 0;                                    // t = 2^te
    if (!bad && mx > 0.f) {
      int ex = 0;
      (void)frexpf(mx, &ex);                       // mx = m 2^ex, m in [0.5, 1): mx / 2^(ex - 14) in [8192, 16384)
      te = ex - 14;
      if (ldexpf(mx, -te) > IP_Q8_QMAX) ++te;
    }
    double a = 0.0;
    for (int e = lane * 4; e < d; e += 256) {
      const float4 v = *(const float4*)(x + e);
      const float4 s = *(const float4*)(step + e);
      const float4 ce = *(const float4*)(centre + e);
      const float r[4] = {v.x, v.y, v.z, v.w}, s0[4] = {s.x, s.y, s.z, s.w}, c0[4] = {ce.x, ce.y, ce.z, ce.w};
      uint32_t ph = 0, pl = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int qi = 0;
        if (!bad) qi = (int)rintf(ldexpf(__fmul_rn(r[i], s0[i]), -te));    // (a power of two: exact, or below 1/2 and 0 either way)
        const int hi = (qi + 64) >> 7, lo = qi - 128 * hi;
        ph |= (uint32_t)(uint8_t)(int8_t)hi << (8 * i);
        pl |= (uint32_t)(uint8_t)(int8_t)lo << (8 * i);
        // rho_j = |centre_j| + 127 (2 + u) step_j bounds |v_ij - centre_j - step_j c_ij| / u for every code
        a += fabs((double)r[i]) * (fabs((double)c0[i]) + 127.0 * (2.0 + 0x1p-24) * (double)s0[i]);
      }
      *(uint32_t*)(hi_row + e) = ph;
      *(uint32_t*)(lo_row + e) = pl;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) {
      // A(q) = (u / t) sum_j |q_j| rho_j, rounded up: the fp64 sum by (1 + 1e-9), the conversion by (1 + 1e-6)
      const float A = (float)(ldexp(a, -24 - te) * (1.0 + 1e-9) * (1.0 + 1e-6));
      band[q] = bad ? INFINITY : A;
    }
  }
}

__global__ void k_fill_f32(float* p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace convdr
