// The exactness certificate of the search kernels, one copy of each piece (included by ip_select.hpp after its order-statistics
// helpers, before k_ip_cut).  Every result of the index is exact because of the arithmetic in this file:
//   IpBand              the error band eps of a query's scan scores and the norm-limit test              (every finishing kernel)
//   ip_topk_verdict     what a top-k cut proves: OK / OVERFLOW / TOO_FEW / UNCERTAIN / RANGE, the retry threshold
//                                                                                     (k_ip_cut, k_ip_finish, k_ip_cut_deep)
//   ip_list_verdict     what a complete-or-overflowed list proves: OK / OVERFLOW / RANGE
//                                                                   (k_ip_range_select, k_ip_rank_finish, k_ip_docrank_count)
//   ip_row_score        the canonical fp64 score of one (query, row) pair, one wave                       (every re-score)
//   ip_band_topk_lds    the exact top-k of a re-scored band held in LDS                              (k_ip_select, k_ip_finish)
//   ip_centre_sums, IpCentreTerms, ip_scan_units   an fp64 bound on q . p -> a scan threshold, every rounding pushed one way
//                                                                                          (k_ip_range_tau, k_ip_band_tau)
// The proofs stay with the kernels that use the pieces: the cut above k_ip_cut, range steps 1-5 above k_ip_range_tau,
// CLAIM LO / HI above k_ip_band_tau.  A change to the band is a change to IpBand::eps and nothing else.
#pragma once

namespace convdr {

// The hit counter of query q (one per 128-byte line: IP_COUNT_STRIDE), as the finishing kernels read it.
__device__ __forceinline__ uint32_t ip_hits(const uint32_t* __restrict__ counts, int q) { return counts[(int64_t)q * IP_COUNT_STRIDE]; }

// What bounds |S~ - exact scaled score| for every row of the block, per query: the coefficients of ip_eps_coef / ip_eps_abs,
// the norms they multiply and the limit above which an operand may hold inf.  IpBlock::band(qnorm) fills it (ip_host.hpp).
struct IpBand {
  const float* qnorm;        // [nq] the queries' norms, in scan units (fp16: the SCALED norm)
  const float* p_max_norm;   // device: largest UNSCALED row norm of the block
  float eps_coef, eps_abs;   // ip_eps_coef, ip_eps_abs
  float p_scale;             // power of two of the fp16 operand; 1 for bf16
  float norm_limit;          // IP_F16_NORM_LIMIT, or +inf for bf16
  float norm_floor;          // IP_BF16_NORM_FLOOR, or 0 for fp16 (whose operands are rescaled)
  float q8_coef = 0.f;       // 8-bit store: IP_Q8_COEF, and then qnorm holds A(q) and p_max_norm the largest row L1 norm of the codes

  // the largest passage norm in scan units
  __device__ __forceinline__ float pm() const { return p_max_norm[0] * p_scale; }
  // (scaled units for the fp16 scan: qnorm is the scaled query norm, pm the scaled largest passage norm)
  __device__ __forceinline__ float eps(int q) const {
    const float qn = qnorm[q], pmax = pm();
    if (q8_coef > 0.f) return (q8_coef * pmax + qn) * 1.001f + 1e-30f;   // (1/2 + r) max ||c||_1 + A(q): derivation at IP_Q8_COEF
    return (eps_coef * qn * pmax + eps_abs * (qn + pmax) + eps_abs * eps_abs) * 1.001f + 1e-30f;
  }
  // fp16 scan copy built with a scale too large for this block's norms -- or a query so long that its per-row power-of-two
  // scale hit the clamp (norm > ~8e34) --: elements of an operand may be inf, and no score of the query proves anything.
  // bf16 scan: a non-zero norm below the floor -- operands or products may be subnormal, which eps (relative terms only) does
  // not cover (derivation: IP_BF16_NORM_FLOOR, ip_topk.hip).  A zero norm stays in range: every score of the query, or of the
  // block, is exactly 0, and the + 1e-30f of eps covers it.
  __device__ __forceinline__ bool out_of_range(int q) const {
    const float qn = qnorm[q], pmax = pm();
    return pmax > norm_limit || qn > norm_limit || (pmax > 0.f && pmax < norm_floor) || (qn > 0.f && qn < norm_floor);
  }
};

// The certificate of a top-k cut (proof: above k_ip_cut).  cnt: the query's hits, c = min(cnt, cap) of them listed;
// need = min(k, rows); t: the threshold the list was emitted with; cut = S~(k) - 2 eps over the listed scores, -inf when
// fewer than `need` are listed.  retry: the threshold that makes the next pass complete (-inf: none needed, or none helps).
struct IpVerdict { int status; float retry; };
__device__ __forceinline__ IpVerdict ip_topk_verdict(uint32_t cnt, int cap, int c, int need, float t, float cut, float eps,
                                                     bool out_of_range) {
  IpVerdict v = {CONVDR_IP_OK, -INFINITY};
  if (cnt > (uint32_t)cap) {
    // stored candidates are a subset of {s~ >= tau}: their k-th s~ bounds the true s~(k) from below,
    // so `cut` is a valid (if loose) threshold; when it does not tighten tau the caller raises cap
    v.status = CONVDR_IP_OVERFLOW;
    const float cand = nextafterf(cut, -INFINITY);
    v.retry = cand > t ? cand : t;
  } else if (c < need) {
    v.status = CONVDR_IP_TOO_FEW;
    v.retry = t - 4.f * eps - 1e-3f * fabsf(t);
  } else if (need > 0 && t > -INFINITY && cut < t) {
    v.status = CONVDR_IP_UNCERTAIN;  // band reaches below tau: list incomplete in [cut, tau)
    v.retry = nextafterf(cut, -INFINITY);
  }
  if (out_of_range) {
    v.status = CONVDR_IP_RANGE;
    v.retry = -INFINITY;
  }
  return v;
}

// The certificate of a list that needs no k-th score (range search, rank): complete unless it overflowed.  bad: a
// non-finite intermediate of the query's thresholds (k_ip_band_tau), 0 where there is none.
__device__ __forceinline__ int ip_list_verdict(uint32_t cnt, int cap, uint32_t bad, bool out_of_range) {
  int st = CONVDR_IP_OK;
  if (cnt > (uint32_t)cap) st = CONVDR_IP_OVERFLOW;
  if (bad || out_of_range) st = CONVDR_IP_RANGE;
  return st;
}

// ------------------------------------------------------------------------------------------
// exact rescoring: canonical fp64 inner product (see oracle/search.py: lane l owns elements
// 256 j + 4 l + c, accumulated in (j, c) order; then butterfly 32,16,8,4,2,1)
// ------------------------------------------------------------------------------------------
// PT = the passage element type: float (the fp32 block) or _Float16 (the half store, which holds 2^s v for the stored
// half v).  A lane's 4 halves are one 8-byte load and widen to double exactly; the lane / (j, c) / butterfly order is
// the same.  Every product q (2^s v) is 2^s (q v) exactly, and every fp64 rounding of the fma chain and of the butterfly
// commutes with a power-of-two factor (|q| < 2^128, |2^s v| < 2^16, and the smallest non-zero product, 2^-149 2^-24 =
// 2^-173, is 849 binades above the fp64 subnormals: nothing overflows or loses bits to underflow), so the sum is 2^s times the
// oracle's sum bit for bit, and ONE multiplication by 2^-s after the butterfly (`unscale`, exact) gives the oracle's value.
// The 8-bit store's rows (PT = int8_t) are not a pointer but codes, centre and step: element j of a row is the fp32 value
// v_j = fl(centre_j + fl(step_j c_j)) -- one rounded multiplication, one rounded addition, no contraction --, which widens to
// double exactly.  A lane reads its 4 codes as one 4-byte load; the lane / (j, c) / butterfly order is unchanged.
struct IpQ8Rows { const int8_t* codes; const float* centre; const float* step; };
template <class PT> struct IpRows { typedef const PT* type; };       // what a kernel that reads rows of PT takes for them
template <> struct IpRows<int8_t> { typedef IpQ8Rows type; };
template <class PT>
__device__ __forceinline__ const PT* ip_row_at(const PT* P, int64_t row, int d) { return P + row * d; }
__device__ __forceinline__ IpQ8Rows ip_row_at(IpQ8Rows P, int64_t row, int d) { P.codes += row * d; return P; }

struct f64x4 { double x, y, z, w; };
__device__ __forceinline__ f64x4 ip_load4_f64(const IpQ8Rows& p, int e) {
  const uint32_t raw = *(const uint32_t*)(p.codes + e);
  const float4 c = *(const float4*)(p.centre + e);
  const float4 s = *(const float4*)(p.step + e);
  // (HIP's __fmul_rn / __fadd_rn are the plain operators, which hipcc contracts into ONE fma with a single rounding: the
  //  product goes through an opaque register, so that it is rounded to fp32 before the addition sees it)
  auto v = [](float ce, float st, uint32_t byte) {
    float m = st * (float)(int)(int8_t)byte;
    asm volatile("" : "+v"(m));
    return (double)(ce + m);
  };
  return {v(c.x, s.x, raw & 255u), v(c.y, s.y, (raw >> 8) & 255u), v(c.z, s.z, (raw >> 16) & 255u), v(c.w, s.w, raw >> 24)};
}
template <class PT>
__device__ __forceinline__ f64x4 ip_load4_f64(const PT* p, int e) {
  p += e;
  if constexpr (sizeof(PT) == 2) {
    typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
    const uint2 raw = *(const uint2*)p;
    const f16x4_t h = *(const f16x4_t*)&raw;
    return {(double)h[0], (double)h[1], (double)h[2], (double)h[3]};
  } else {
    const float4 y = *(const float4*)p;
    return {(double)y.x, (double)y.y, (double)y.z, (double)y.w};
  }
}

// The canonical fp64 score of one (query, row) pair, computed by one whole wave and returned on every lane of it: the one
// device implementation of the order above, and its one multiplication by `unscale` for the half store.  Every re-score
// calls it: k_ip_rescore, k_ip_finish, k_ip_score_rows and k_ip_score_docs (ip_docs.hpp).  The call is wave-uniform.
template <class PT>
__device__ __forceinline__ double ip_row_score(const float* __restrict__ qv, typename IpRows<PT>::type pv, int d, int lane,
                                               double unscale) {
  double acc = 0.0;
  for (int e = lane * 4; e < d; e += 256) {
    const float4 x = *(const float4*)(qv + e);
    const f64x4 y = ip_load4_f64(pv, e);
    acc = fma((double)x.x, y.x, acc);
    acc = fma((double)x.y, y.y, acc);
    acc = fma((double)x.z, y.z, acc);
    acc = fma((double)x.w, y.w, acc);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if constexpr (sizeof(PT) == 2) acc *= unscale;   // (the half store only: no other row type is scaled)
  return acc;
}

// ------------------------------------------------------------------------------------------
// top-k of a re-scored band by (exact score desc, index asc): select the k-th largest exact score, keep
// the candidates at or above it (more than k only when scores tie exactly at the boundary -- duplicate passages), and
// sort just those.
// s / id: the band's c exact scores and ids in LDS (c <= cap <= 8192, room for the next power of two), complete behind a
// barrier; sh_g: an LDS word zeroed before that barrier.  Writes row q of D / I [nq, k] with FAISS padding.
// CONTRACT: the whole workgroup calls it, and blockDim.x == IP_SELECT_THREADS -- the register lift below strides by the
// constant (IP_SELECT_PER_THREAD x IP_SELECT_THREADS = 8192 covers any band), the pad and the write stride by blockDim.x.
// Both callers are launched with dim3(IP_SELECT_THREADS) and carry __launch_bounds__(IP_SELECT_THREADS).
// ------------------------------------------------------------------------------------------
constexpr int IP_SELECT_THREADS = 1024;
constexpr int IP_SELECT_PER_THREAD = 8192 / IP_SELECT_THREADS;   // cap <= 8192
__device__ __forceinline__ void ip_band_topk_lds(double* s, uint32_t* id, int c, int k, int q, SelectScratch& sc, uint32_t& sh_g,
                                                 float* __restrict__ D, int64_t* __restrict__ I) {
  int g = c;
  if (c > k) {
    // Select on the high 32 key bits only (sign, exponent, 20 mantissa bits): a candidate whose high word is below the
    // k-th largest high word is below at least k candidates in the full order too, so the top k all survive; the few
    // extra survivors that share the boundary word are ordered exactly by the sort.
    const uint64_t kth =
        block_kth_largest<32>([&](int i) { return f64_order_key(s[i]) >> 32; }, c, (uint32_t)k, sc);
    // compact {high word >= kth} to the front: every thread lifts its elements into registers first
    double ms[IP_SELECT_PER_THREAD];
    uint32_t mi[IP_SELECT_PER_THREAD];
#pragma unroll
    for (int e = 0; e < IP_SELECT_PER_THREAD; ++e) {
      const int i = threadIdx.x + e * IP_SELECT_THREADS;
      ms[e] = i < c ? s[i] : 0.0;
      mi[e] = i < c ? id[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < IP_SELECT_PER_THREAD; ++e) {
      const int i = threadIdx.x + e * IP_SELECT_THREADS;
      if (i < c && (f64_order_key(ms[e]) >> 32) >= kth) {
        const uint32_t slot = atomicAdd(&sh_g, 1u);
        s[slot] = ms[e];
        id[slot] = mi[e];
      }
    }
    __syncthreads();
    g = (int)sh_g;
  }
  int np2 = 2;
  while (np2 < g) np2 <<= 1;
  for (int i = g + threadIdx.x; i < np2; i += blockDim.x) { s[i] = -INFINITY; id[i] = 0xffffffffu; }
  __syncthreads();
  bitonic_cand(s, id, np2);
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    D[(int64_t)q * k + j] = j < g ? (float)s[j] : -FLT_MAX;
    I[(int64_t)q * k + j] = j < g ? (int64_t)id[j] : -1;
  }
}

// ------------------------------------------------------------------------------------------
// From an fp64 bound on the score q . p to a threshold on the scan score: the query against the centre.
// ------------------------------------------------------------------------------------------
// The four fp64 sums of one query against the centre (0 when there is none), by one whole wave, on every lane of it:
// dot = fl(q . c), adot = sum |q_i c_i|, qq = |q|^2, cc = |c|^2.
struct IpCentreSums { double dot, adot, qq, cc; };
__device__ __forceinline__ IpCentreSums ip_centre_sums(const float* __restrict__ qv, const float* __restrict__ centre, int d,
                                                       int lane) {
  double dot = 0.0, adot = 0.0, qq = 0.0, cc = 0.0;
  for (int e = lane * 4; e < d; e += 256) {
    const float4 x = *(const float4*)(qv + e);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (centre) c = *(const float4*)(centre + e);
    const double xs[4] = {(double)x.x, (double)x.y, (double)x.z, (double)x.w};
    const double cs[4] = {(double)c.x, (double)c.y, (double)c.z, (double)c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dot = fma(xs[i], cs[i], dot);
      adot += fabs(xs[i] * cs[i]);
      qq = fma(xs[i], xs[i], qq);
      cc = fma(cs[i], cs[i], cc);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    dot += __shfl_xor(dot, o, 64);
    adot += __shfl_xor(adot, o, 64);
    qq += __shfl_xor(qq, o, 64);
    cc += __shfl_xor(cc, o, 64);
  }
  return {dot, adot, qq, cc};
}

// What the sums give (notation and proofs: k_ip_range_tau, k_ip_band_tau): with g = (d + 8) 2^-52,
//   e_c = g sum |q_i c_i|        bounds |fl(q . c) - q . c|,
//   e_x = g |q| (|c| + max|v|)   bounds |X(q, p) - q . p| for every row p = c + v of the block,
//   qs                           the query's power-of-two scale.  per_row_scale: the queries were scaled row by row
//                                (k_rows_to_half<F16, true>): qn holds the SCALED norm, and qs is recovered from its ratio
//                                to the unscaled norm summed here (the ratio is 2^k (1 +- 1e-6); a zero or non-finite
//                                query was left unscaled: qs = 1).
struct IpCentreTerms {
  double dot, e_c, e_x, qs;
  __device__ __forceinline__ IpCentreTerms(const IpCentreSums& s, int d, float qn, float p_max_norm, int per_row_scale) {
    const double nq_u = sqrt(s.qq) * (1.0 + 1e-9), nc = sqrt(s.cc) * (1.0 + 1e-9);   // (rounded up: bounds)
    qs = 1.0;
    if (per_row_scale && nq_u > 0.0 && nq_u < (double)INFINITY && qn > 0.f && qn < INFINITY)
      qs = ldexp(1.0, (int)rint(log2((double)qn / nq_u)));
    const double g = (double)(d + 8) * 2.220446049250313e-16;                      // (d + 8) 2^-52
    dot = s.dot;
    e_c = g * s.adot * (1.0 + 1e-9);
    e_x = g * nq_u * (nc + (double)p_max_norm * (1.0 + 1e-6)) * (1.0 + 1e-9);
  }
  // A bound on q . v for a row whose canonical score is x: x - fl(q . c) with e_c + e_x taken off (UP: added), every
  // operation's rounding (relative 2^-53) charged by 2^-50 of the operands' magnitudes.  Not above (UP: not below) the
  // real x - q . c -+ e_x.
  template <bool UP>
  __device__ __forceinline__ double bound(double x) const {
    const double charge = 8.881784197001252e-16 * (fabs(x) + fabs(dot) + e_c + e_x);   // 2^-50: the roundings of the line below
    return UP ? (x - dot + e_c + e_x) + charge : (x - dot - e_c - e_x) - charge;
  }
};

// A bound t on q . v in scan units: s = qs p_scale t (exact in fp64: powers of two; overflow to +-inf keeps the order),
// rounded to fp32 toward -inf (UP: toward +inf).  *s_out: s itself.
template <bool UP>
__device__ __forceinline__ float ip_scan_units(double t, double qs, float p_scale, double* s_out = nullptr) {
  const double s = t * qs * (double)p_scale;
  if (s_out) *s_out = s;
  float f = (float)s;                                                              // to nearest ...
  if (UP ? (double)f < s : (double)f > s) f = nextafterf(f, UP ? INFINITY : -INFINITY);   // ... then away
  return f;
}

}  // namespace convdr
