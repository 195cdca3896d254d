// Exact per-group skewness / kurtosis for CDNA4 (gfx950): power sums up to order 4 over a quantile
// producer's chunk-region records.
//
// The JIT producer (ops/jit.py A_QVAL) writes (u32 group key, order-preserving u64 value per
// column) records of the selected rows into its chunk regions (the layout quantile.hip reads); the
// kernels here add up a group's state (central_moments.h CmMode):
//
//  * integer / decimal columns whose stored range max - min is below 2^32, ONE pass: with `pivot`
//    the ordered u64 of the column's minimum, y = o - pivot is a u32 whatever the column's width
//    (10^12 + small qualifies), and both statistics are invariant under the shift.  The state is n,
//    S1 = sum y and carry-free digit sums of y^2 (one 32 x 32 product, two digits), y^3 (the 64 x 32
//    product, three) and, when a kurtosis asks, y^4 (the 64 x 64 product, four).  Every update is an
//    integer add: bitwise the same under any order of waves, workgroups and atomics.
//    cm_final_kernel normalises the digits, forms N2, N3 and N4 (central_moments.h) exactly in 320
//    bits, rounds each to double ONCE and evaluates N3 / (N2 sqrt N2) and N4 / N2^2 - 3.
//  * double columns and integer columns of a wider range, TWO passes: n and sum x give the mean
//    (cm_mean_kernel), then the sums of d, d^2, d^3 [, d^4] of d = x - mean, to which the finalise
//    applies the same N formulas in f64 (the sum of d corrects the rounded mean).  NOT exact, and
//    f64 adds do not commute bitwise: a few ulp between runs.
//
// Work split by key space (central_moments.h): cm_few (private LDS rows per wave, one cross-lane
// reduce-scatter of the whole state per distinct key of a wave's 64 records, no atomics), cm_lds
// (one LDS table per workgroup, LDS atomics, one pass per key slice), cm_global (global atomics
// after a per-wave merge of runs of equal keys).  Every record loop runs a workgroup-uniform trip
// count (the ragged end is masked per lane), so the cross-lane operations always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "central_moments.h"
#include "moments_dev.h"  // MSIGN, mom_add, mom_atomic, mom_f64, mom_region_end, co_reduce_scatter

namespace sdo {

static constexpr uint64_t CM_LOW = 0xffffffffull;

__device__ __forceinline__ uint64_t cm_bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ double cm_val(uint64_t b) { return __longlong_as_double((long long)b); }

// the words one record adds to its group's state (`pivot`: the integer modes; `dbl`: the column is
// a double, else its integer is converted -- the f64 modes; `mean` [G]: the DEV modes)
template <int MODE>
__device__ __forceinline__ void cm_contrib(uint64_t o, uint32_t g, uint64_t pivot, int dbl,
                                           const double* __restrict__ mean, uint64_t (&w)[cm_words(MODE)]) {
  if constexpr (MODE == CM_INT3 || MODE == CM_INT4) {
    const uint32_t y = (uint32_t)(o - pivot);  // (max - min < 2^32: no bit is dropped)
    const uint64_t y2 = (uint64_t)y * y;
    const uint64_t c_lo = y2 * y, c_hi = __umul64hi(y2, (uint64_t)y);  // y^3 < 2^96
    w[0] = 1ull;
    w[1] = y;
    w[2] = y2 & CM_LOW;
    w[3] = y2 >> 32;
    w[4] = c_lo & CM_LOW;
    w[5] = c_lo >> 32;
    w[6] = c_hi;
    if constexpr (MODE == CM_INT4) {
      const uint64_t q_lo = y2 * y2, q_hi = __umul64hi(y2, y2);
      w[7] = q_lo & CM_LOW;
      w[8] = q_lo >> 32;
      w[9] = q_hi & CM_LOW;
      w[10] = q_hi >> 32;
    }
  } else {
    const double x = dbl ? mom_f64(o) : (double)(int64_t)(o ^ MSIGN);
    if constexpr (MODE == CM_F64_SUM) {
      w[0] = 1ull;
      w[1] = cm_bits(x);
    } else {
      const double d = x - mean[g], d2 = d * d;
      w[0] = cm_bits(d);
      w[1] = cm_bits(d2);
      w[2] = cm_bits(d2 * d);
      if constexpr (MODE == CM_F64_DEV4) w[3] = cm_bits(d2 * d2);
    }
  }
}

// the CM_R records of this thread in the tile starting at record `b0` of a region ending at `hi`
// (a key of all ones: no record); every load is issued before the first add
__device__ __forceinline__ void cm_load(const uint32_t* __restrict__ recs, int rw, int voff, uint32_t b0, uint32_t hi,
                                        uint32_t (&g)[CM_R], uint64_t (&o)[CM_R]) {
#pragma unroll
  for (int u = 0; u < CM_R; ++u) {
    const uint32_t i = b0 + u * blockDim.x + threadIdx.x;
    g[u] = 0xffffffffu;
    o[u] = 0ull;
    if (i < hi) {
      const uint32_t* r = recs + (uint64_t)i * rw;
      g[u] = r[0];
      o[u] = (uint64_t)r[voff] | ((uint64_t)r[voff + 1] << 32);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// few groups: one reduce-scatter of the padded state across the wave per distinct key; lane l < P
// then adds word co_word_of<P>(l) to the wave's private LDS row

template <int MODE>
__global__ void __launch_bounds__(256) cm_few_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                            const uint32_t* __restrict__ seg_lo,
                                                            const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                            uint32_t G, uint64_t pivot, int dbl,
                                                            const double* __restrict__ mean,
                                                            uint64_t* __restrict__ state) {
  constexpr int W = cm_words(MODE);
  constexpr int C = cm_counts(MODE) ? 1 : 0;
  constexpr int V = W - C;
  constexpr int P = cm_pow2(V);
  constexpr bool F = cm_isf(MODE, 1);  // (every word but the count is of one kind)
  __shared__ uint64_t rows[CM_WAVES * CM_FEW_G * W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < CM_WAVES * CM_FEW_G * W; i += blockDim.x) rows[i] = 0ull;
  __syncthreads();
  uint64_t* row = rows + wave * CM_FEW_G * W;  // G <= CM_FEW_G (launcher)
  const int word = co_word_of<P>(lane);
  const bool writer = lane < P && word < V;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CM_R * blockDim.x) {
      uint32_t g[CM_R];
      uint64_t o[CM_R];
      cm_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < CM_R; ++u) {
        const bool ok = g[u] < G;  // (past the region's end, or a key outside the state: never fault)
        uint64_t w[W];
        cm_contrib<MODE>(o[u], ok ? g[u] : 0u, pivot, dbl, mean, w);
        uint64_t live = __ballot(ok);
        while (live) {  // (wave-uniform) one trip per distinct key among the wave's 64 records
          const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)g[u], __ffsll((unsigned long long)live) - 1);
          const bool mine = ok && g[u] == k;
          const uint64_t m = __ballot(mine);
          uint64_t a[P];
#pragma unroll
          for (int j = 0; j < P; ++j) a[j] = (j < V && mine) ? w[(j < V ? j : 0) + C] : 0ull;  // (the padding words: 0)
          co_reduce_scatter<F, P / 2, 0, P>(a, lane);
          if (writer) row[k * W + C + word] = mom_add(F, row[k * W + C + word], a[0]);
          if (C && lane == 63) row[k * W] += (uint64_t)__popcll(m);
          live &= ~m;
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < G * W; i += blockDim.x) {
    const bool f = cm_isf(MODE, (int)(i % W));
    uint64_t v = rows[i];
#pragma unroll
    for (int wv = 1; wv < CM_WAVES; ++wv) v = mom_add(f, v, rows[wv * CM_FEW_G * W + i]);
    if (v) mom_atomic(f, &state[i], v);
  }
}

// ---------------------------------------------------------------------------------------------
// one LDS table per workgroup for the key slice [g0, g0 + GL): [GL][V] u64 words (V = W without the
// count), then [GL] u32 counts.  Records of other slices are skipped before their products are
// formed: the launcher runs one pass per slice (central_moments.h CM_LDS_SLICES).

template <int MODE>
__global__ void __launch_bounds__(256) cm_lds_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                            const uint32_t* __restrict__ seg_lo,
                                                            const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                            uint32_t g0, uint32_t GL, uint64_t pivot, int dbl,
                                                            const double* __restrict__ mean,
                                                            uint64_t* __restrict__ state) {
  constexpr int W = cm_words(MODE);
  constexpr int C = cm_counts(MODE) ? 1 : 0;
  constexpr int V = W - C;
  extern __shared__ uint64_t cm_tab[];  // GL <= cm_lds_groups(MODE) (launcher)
  uint32_t* cnt = (uint32_t*)(cm_tab + (size_t)GL * V);
  for (uint32_t i = threadIdx.x; i < GL * V; i += blockDim.x) cm_tab[i] = 0ull;
  if (C)
    for (uint32_t i = threadIdx.x; i < GL; i += blockDim.x) cnt[i] = 0u;
  __syncthreads();
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CM_R * blockDim.x) {
      uint32_t g[CM_R];
      uint64_t o[CM_R];
      cm_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < CM_R; ++u) {
        const uint32_t k = g[u] - g0;  // (a key below the slice wraps past GL)
        if (k >= GL) continue;
        uint64_t w[W];
        cm_contrib<MODE>(o[u], g[u], pivot, dbl, mean, w);
        if (C) atomicAdd(&cnt[k], 1u);
#pragma unroll
        for (int j = 0; j < V; ++j)  // (a zero word -- the high digits of a small y -- costs nothing)
          if (w[j + C]) mom_atomic(cm_isf(MODE, j + C), &cm_tab[k * V + j], w[j + C]);
      }
    }
  }
  __syncthreads();
  uint64_t* out = state + (uint64_t)g0 * W;
  for (uint32_t i = threadIdx.x; i < GL; i += blockDim.x) {
    if (C) {
      if (!cnt[i]) continue;
      atomicAdd((unsigned long long*)&out[(uint64_t)i * W], (unsigned long long)cnt[i]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const uint64_t v = cm_tab[i * V + j];
      if (v) mom_atomic(cm_isf(MODE, j + C), &out[(uint64_t)i * W + j + C], v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// beyond LDS: global atomics.  Rows are stored sorted by time and dimension, so keys come in runs:
// every run of equal adjacent keys of a wave is summed towards its last lane (a segmented shuffle
// scan bounded by the run's first lane, stopping at the first distance no run of the wave reaches)
// and that lane issues the run's atomics.

template <int MODE>
__global__ void __launch_bounds__(256) cm_global_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                               const uint32_t* __restrict__ seg_lo,
                                                               const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                               uint32_t G, uint64_t pivot, int dbl,
                                                               const double* __restrict__ mean,
                                                               uint64_t* __restrict__ state) {
  constexpr int W = cm_words(MODE);
  constexpr int C = cm_counts(MODE) ? 1 : 0;
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CM_R * blockDim.x) {
      uint32_t g[CM_R];
      uint64_t o[CM_R];
      cm_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < CM_R; ++u) {
        const bool ok = g[u] < G;
        const uint32_t key = ok ? g[u] : 0xffffffffu;
        uint64_t w[W];
        cm_contrib<MODE>(o[u], ok ? g[u] : 0u, pivot, dbl, mean, w);
        const uint32_t prev = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || prev != key;
        const uint64_t heads = __ballot(head);
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // first lane of this run
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        for (int d = 1; d < 64; d <<= 1) {
          const bool take = lane - d >= first;
          if (!__ballot(take)) break;  // (wave-uniform) no run is longer than d lanes
#pragma unroll
          for (int j = C; j < W; ++j) {
            const uint64_t t = __shfl_up((unsigned long long)w[j], d, 64);
            if (take) w[j] = mom_add(cm_isf(MODE, j), w[j], t);
          }
        }
        if (!ok || !last) continue;
        uint64_t* s = state + (uint64_t)key * W;
        if (C) atomicAdd((unsigned long long*)s, (unsigned long long)(lane - first + 1));
#pragma unroll
        for (int j = C; j < W; ++j)
          if (w[j]) mom_atomic(cm_isf(MODE, j), s + j, w[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// mean[g] of the f64 path from its CM_F64_SUM state (0 for an empty group)
__global__ void __launch_bounds__(256) cm_mean_kernel(const uint64_t* __restrict__ sum, int G, double* __restrict__ mean) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint64_t n = sum[2 * (int64_t)g];
  mean[g] = n ? cm_val(sum[2 * (int64_t)g + 1]) / (double)n : 0.0;
}

// 320-bit two's-complement arithmetic of the finalise (l[0] the lowest limb; central_moments.h
// CM_LIMBS states why no intermediate wraps)
struct Cm320 {
  uint64_t l[CM_LIMBS];
};

__device__ __forceinline__ Cm320 cm_add(Cm320 a, Cm320 b) {
  Cm320 r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < CM_LIMBS; ++i) {
    const uint64_t t = a.l[i] + b.l[i];
    r.l[i] = t + c;
    c = (t < a.l[i]) | (r.l[i] < t);
  }
  return r;
}

__device__ __forceinline__ Cm320 cm_neg(Cm320 a) {
  Cm320 n, one = {{1ull, 0ull, 0ull, 0ull, 0ull}};
#pragma unroll
  for (int i = 0; i < CM_LIMBS; ++i) n.l[i] = ~a.l[i];
  return cm_add(n, one);
}

__device__ __forceinline__ Cm320 cm_sub(Cm320 a, Cm320 b) { return cm_add(a, cm_neg(b)); }

// a m for a non-negative a (the product stays below 2^320: central_moments.h)
__device__ __forceinline__ Cm320 cm_mul(Cm320 a, uint64_t m) {
  Cm320 r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < CM_LIMBS; ++i) {
    const uint64_t lo = a.l[i] * m, hi = __umul64hi(a.l[i], m);
    r.l[i] = lo + c;
    c = hi + (r.l[i] < lo);  // (hi <= 2^64 - 2: no carry out)
  }
  return r;
}

// sum_k d[k] 2^(32 k) of D <= 4 unsigned digit sums: the one place a carry moves
__device__ __forceinline__ Cm320 cm_digits(const uint64_t* d, int D) {
  Cm320 r = {{0ull, 0ull, 0ull, 0ull, 0ull}};
  for (int k = 0; k < D; ++k) {
    Cm320 t = {{0ull, 0ull, 0ull, 0ull, 0ull}};
    const int i = k >> 1;
    if (k & 1) {
      t.l[i] = d[k] << 32;
      t.l[i + 1] = d[k] >> 32;
    } else {
      t.l[i] = d[k];
    }
    r = cm_add(r, t);
  }
  return r;
}

// a signed 320-bit value as a double, rounded once: the leading 64 bits of the magnitude with
// everything below them folded into the lowest bit (a sticky bit for the conversion's rounding)
__device__ __forceinline__ double cm_f64(Cm320 a) {
  const bool neg = a.l[CM_LIMBS - 1] >> 63;
  if (neg) a = cm_neg(a);
  int t = CM_LIMBS - 1;
  while (t > 0 && !a.l[t]) --t;
  if (!a.l[t]) return 0.0;
  const int z = __clzll((long long)a.l[t]);
  const uint64_t below = t > 0 ? a.l[t - 1] : 0ull;
  const uint64_t top = z ? (a.l[t] << z) | (below >> (64 - z)) : a.l[t];
  uint64_t rest = z ? below << z : below;
  for (int i = 0; i < t - 1; ++i) rest |= a.l[i];
  const double v = ldexp((double)(top | (rest ? 1ull : 0ull)), 64 * t - z);
  return neg ? -v : v;
}

// out[g] = skewness (`order` 3: N3 / (N2 sqrt N2)) or excess kurtosis (4: N4 / N2^2 - 3) of group
// g; NaN where N2 = 0 (no row, one row, or one value).  The integer kurtosis squares N2 (below
// 2^128) exactly before its one rounding, so two rows of different values give exactly -2.
//  integer modes: `a` is the [G][W] state (order 4 needs CM_INT4)
//  CM_F64_DEV3/4: `a` is the CM_F64_SUM state (for n), `b` the DEV state (order 4 needs DEV4)
__global__ void __launch_bounds__(256) cm_final_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                      int G, int mode, int order, double* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const bool f64 = mode == CM_F64_DEV3 || mode == CM_F64_DEV4;
  const int W = cm_words(f64 ? CM_F64_SUM : mode);
  const uint64_t n = a[(int64_t)g * W];
  double n2, nk, n2sq;  // N2, N3 or N4, and N2^2 for the kurtosis
  if (f64) {
    const uint64_t* s = b + (int64_t)g * cm_words(mode);
    const double nd = (double)n, s1 = cm_val(s[0]), s2 = cm_val(s[1]), s3 = cm_val(s[2]);
    n2 = nd * s2 - s1 * s1;
    if (order == 3) {
      nk = nd * nd * s3 - 3.0 * nd * s1 * s2 + 2.0 * s1 * s1 * s1;
    } else {
      const double s4 = cm_val(s[3]);
      nk = nd * nd * nd * s4 - 4.0 * nd * nd * s1 * s3 + 6.0 * nd * s1 * s1 * s2 - 3.0 * s1 * s1 * s1 * s1;
    }
    n2sq = n2 * n2;
  } else {
    const uint64_t* s = a + (int64_t)g * W;
    const uint64_t s1 = s[1];
    const Cm320 S2 = cm_digits(s + 2, 2);
    const Cm320 S1 = {{s1, 0ull, 0ull, 0ull, 0ull}};
    const Cm320 S1_2 = cm_mul(S1, s1);
    const Cm320 nS2 = cm_mul(S2, n);
    const Cm320 N2 = cm_sub(nS2, S1_2);  // (never negative: Cauchy-Schwarz)
    n2 = cm_f64(N2);
    const Cm320 S1_3 = cm_mul(S1_2, s1);
    const Cm320 S3 = cm_digits(s + 4, 3);
    if (order == 3) {
      const Cm320 pos = cm_add(cm_mul(cm_mul(S3, n), n), cm_mul(S1_3, 2ull));
      nk = cm_f64(cm_sub(pos, cm_mul(cm_mul(nS2, s1), 3ull)));
    } else {
      const Cm320 S4 = cm_digits(s + 7, 4);
      const Cm320 pos = cm_add(cm_mul(cm_mul(cm_mul(S4, n), n), n), cm_mul(cm_mul(cm_mul(nS2, s1), s1), 6ull));
      const Cm320 sub = cm_add(cm_mul(cm_mul(cm_mul(cm_mul(S3, n), n), s1), 4ull), cm_mul(cm_mul(S1_3, s1), 3ull));
      nk = cm_f64(cm_sub(pos, sub));
      const Cm320 hi = cm_mul(N2, N2.l[1]);  // N2^2 = N2 l0 + 2^64 N2 l1
      const Cm320 hi64 = {{0ull, hi.l[0], hi.l[1], hi.l[2], hi.l[3]}};
      n2sq = cm_f64(cm_add(cm_mul(N2, N2.l[0]), hi64));
    }
  }
  if (!(n2 > 0.0)) {
    out[g] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  out[g] = order == 3 ? nk / (n2 * sqrt(n2)) : nk / n2sq - 3.0;
}

#define CM_INSTANTIATE(K, M, ...)                                                                                  \
  template __global__ void K<M>(const uint32_t*, int, int, const uint32_t*, const uint32_t*, int64_t, __VA_ARGS__, \
                                uint64_t, int, const double*, uint64_t*);
#define CM_INSTANTIATE_MODES(K, ...)                                                \
  CM_INSTANTIATE(K, CM_INT3, __VA_ARGS__) CM_INSTANTIATE(K, CM_INT4, __VA_ARGS__)   \
  CM_INSTANTIATE(K, CM_F64_SUM, __VA_ARGS__) CM_INSTANTIATE(K, CM_F64_DEV3, __VA_ARGS__) \
  CM_INSTANTIATE(K, CM_F64_DEV4, __VA_ARGS__)
CM_INSTANTIATE_MODES(cm_few_regions_kernel, uint32_t)
CM_INSTANTIATE_MODES(cm_lds_regions_kernel, uint32_t, uint32_t)
CM_INSTANTIATE_MODES(cm_global_regions_kernel, uint32_t)
#undef CM_INSTANTIATE_MODES
#undef CM_INSTANTIATE

}  // namespace sdo
