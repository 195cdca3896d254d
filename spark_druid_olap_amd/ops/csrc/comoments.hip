// Exact per-group covariance / correlation of a column pair for CDNA4 (gfx950): co-moment sums over
// a quantile producer's chunk-region records.
//
// The JIT producer (ops/jit.py A_QVAL) writes (u32 group key, order-preserving u64 value per
// column) records, so both values of a pair sit in one record; the kernels here read the two value
// offsets `voff_x`, `voff_y` and add up the pair's state (comoments.h CoMode, SQ = with the squares
// a correlation needs):
//
//  * integer / decimal pairs, ONE pass: n, Sx, Sy and carry-free digit sums of the signed product
//    x y (its top digit sign-extended into an int64 sum) and, with SQ, of x^2 and y^2.  Every update
//    is an integer add: bitwise the same under any order of waves, workgroups and atomics.
//    co_final_kernel normalises the digits and forms A = n Sxy - Sx Sy (and Vx = n Sxx - Sx^2, Vy)
//    exactly in 192-bit limbs, each rounded to double once.
//  * pairs with a double column, TWO passes: n, sum x, sum y give the means (co_mean_kernel), then
//    the sums of the deviations and of their products, finalised in the corrected two-pass form
//    Cxy = sum dx dy - sum dx sum dy / n.  An integer / decimal partner is converted to double on
//    entry (rounded once beyond 2^53).  f64 adds do not commute bitwise: a few ulp between runs.
//
// Work split by key space (comoments.h): co_few (private LDS rows per wave, one cross-lane
// reduce-scatter of the whole state per distinct key of a wave's 64 records), co_lds (one LDS table
// per workgroup, LDS atomics, one pass per key slice), co_global (global atomics after a per-wave
// merge of runs of equal keys).  Every record loop runs a workgroup-uniform trip count (the ragged
// end is masked per lane), so the cross-lane operations always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comoments.h"
#include "moments_dev.h"

namespace sdo {

static constexpr uint64_t CO_LOW = 0xffffffffull;

__device__ __forceinline__ uint64_t co_bits(double v) { return (uint64_t)__double_as_longlong(v); }

// a record value as a double: a double column's own value, else the integer converted
__device__ __forceinline__ double co_f64(uint64_t o, bool dbl) {
  return dbl ? mom_f64(o) : (double)(int64_t)(o ^ MSIGN);
}

// the D digits of |x|^2 (unsigned)
template <int D>
__device__ __forceinline__ void co_square(int64_t x, uint64_t* w) {
  const uint64_t ax = x < 0 ? 0ull - (uint64_t)x : (uint64_t)x;
  const uint64_t lo = ax * ax;
  w[0] = lo & CO_LOW;
  w[1] = lo >> 32;
  if constexpr (D == 4) {
    const uint64_t hi = __umul64hi(ax, ax);
    w[2] = hi & CO_LOW;
    w[3] = hi >> 32;
  }
}

// the words one record adds to its group's state (`mean` [G][2] is read in CO_F64_DEV only; `dbl`
// bit 0 / 1: x / y is a double column, read in the f64 modes only)
template <int MODE, bool SQ>
__device__ __forceinline__ void co_contrib(uint64_t ox, uint64_t oy, uint32_t g, int dbl,
                                           const double* __restrict__ mean, uint64_t (&w)[co_words(MODE, SQ)]) {
  if constexpr (MODE == CO_INT2 || MODE == CO_INT4) {
    constexpr int D = co_digits(MODE);
    const int64_t x = (int64_t)(ox ^ MSIGN), y = (int64_t)(oy ^ MSIGN);
    w[0] = 1ull;
    w[1] = (uint64_t)x;
    w[2] = (uint64_t)y;
    if constexpr (MODE == CO_INT2) {
      const int64_t p = x * y;  // (|x|, |y| <= 2^31: no overflow)
      w[3] = (uint64_t)p & CO_LOW;
      w[4] = (uint64_t)(p >> 32);  // signed top digit
    } else {
      const uint64_t lo = (uint64_t)x * (uint64_t)y;
      const int64_t hi = __mul64hi((long long)x, (long long)y);
      w[3] = lo & CO_LOW;
      w[4] = lo >> 32;
      w[5] = (uint64_t)hi & CO_LOW;
      w[6] = (uint64_t)(hi >> 32);  // signed top digit
    }
    if constexpr (SQ) {
      co_square<D>(x, &w[3 + D]);
      co_square<D>(y, &w[3 + 2 * D]);
    }
  } else if constexpr (MODE == CO_F64_SUM) {
    w[0] = 1ull;
    w[1] = co_bits(co_f64(ox, dbl & 1));
    w[2] = co_bits(co_f64(oy, dbl & 2));
  } else {
    const double dx = co_f64(ox, dbl & 1) - mean[2 * (uint64_t)g];
    const double dy = co_f64(oy, dbl & 2) - mean[2 * (uint64_t)g + 1];
    w[0] = co_bits(dx);
    w[1] = co_bits(dy);
    w[2] = co_bits(dx * dy);
    if constexpr (SQ) {
      w[3] = co_bits(dx * dx);
      w[4] = co_bits(dy * dy);
    }
  }
}

// the CO_R records of this thread in the tile starting at record `b0` of a region ending at `hi`
// (a key of all ones: no record)
__device__ __forceinline__ void co_load(const uint32_t* __restrict__ recs, int rw, int voff_x, int voff_y, uint32_t b0,
                                        uint32_t hi, uint32_t (&g)[CO_R], uint64_t (&ox)[CO_R], uint64_t (&oy)[CO_R]) {
#pragma unroll
  for (int u = 0; u < CO_R; ++u) {
    const uint32_t i = b0 + u * blockDim.x + threadIdx.x;
    g[u] = 0xffffffffu;
    ox[u] = oy[u] = 0ull;
    if (i < hi) {
      const uint32_t* r = recs + (uint64_t)i * rw;
      g[u] = r[0];
      ox[u] = (uint64_t)r[voff_x] | ((uint64_t)r[voff_x + 1] << 32);
      oy[u] = (uint64_t)r[voff_y] | ((uint64_t)r[voff_y + 1] << 32);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// few groups: one reduce-scatter of the state across the wave per distinct key

// (co_reduce_scatter, co_word_of: moments_dev.h)

template <int MODE, bool SQ>
__global__ void __launch_bounds__(256) co_few_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff_x,
                                                            int voff_y, const uint32_t* __restrict__ seg_lo,
                                                            const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                            uint32_t G, int dbl, const double* __restrict__ mean,
                                                            uint64_t* __restrict__ state) {
  constexpr int W = co_words(MODE, SQ);
  constexpr int C = co_counts(MODE) ? 1 : 0;
  constexpr int V = W - C;
  constexpr int P = co_pow2(V);
  constexpr bool F = co_isf(MODE, 1);  // (every word but the count is of one kind)
  __shared__ uint64_t rows[CO_WAVES * CO_FEW_G * W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < CO_WAVES * CO_FEW_G * W; i += blockDim.x) rows[i] = 0ull;
  __syncthreads();
  uint64_t* row = rows + wave * CO_FEW_G * W;  // G <= CO_FEW_G (launcher)
  const int word = co_word_of<P>(lane);
  const bool writer = lane < P && word < V;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CO_R * blockDim.x) {
      uint32_t g[CO_R];
      uint64_t ox[CO_R], oy[CO_R];
      co_load(recs, rw, voff_x, voff_y, b0, hi, g, ox, oy);
#pragma unroll
      for (int u = 0; u < CO_R; ++u) {
        const bool ok = g[u] < G;  // (past the region's end, or a key outside the state: never fault)
        uint64_t w[W];
        co_contrib<MODE, SQ>(ox[u], oy[u], ok ? g[u] : 0u, dbl, mean, w);
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
    const bool f = co_isf(MODE, (int)(i % W));
    uint64_t v = rows[i];
#pragma unroll
    for (int wv = 1; wv < CO_WAVES; ++wv) v = mom_add(f, v, rows[wv * CO_FEW_G * W + i]);
    if (v) mom_atomic(f, &state[i], v);
  }
}

// ---------------------------------------------------------------------------------------------
// one LDS table per workgroup for the key slice [g0, g0 + GL): [GL][V] u64 words (V = W without the
// count), then [GL] u32 counts.  Records of other slices are skipped before their products are
// formed: the launcher runs one pass per slice (comoments.h CO_LDS_SLICES).

template <int MODE, bool SQ>
__global__ void __launch_bounds__(256) co_lds_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff_x,
                                                            int voff_y, const uint32_t* __restrict__ seg_lo,
                                                            const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                            uint32_t g0, uint32_t GL, int dbl,
                                                            const double* __restrict__ mean,
                                                            uint64_t* __restrict__ state) {
  constexpr int W = co_words(MODE, SQ);
  constexpr int C = co_counts(MODE) ? 1 : 0;
  constexpr int V = W - C;
  extern __shared__ uint64_t co_tab[];  // GL <= co_lds_groups(MODE, SQ) (launcher)
  uint32_t* cnt = (uint32_t*)(co_tab + (size_t)GL * V);
  for (uint32_t i = threadIdx.x; i < GL * V; i += blockDim.x) co_tab[i] = 0ull;
  if (C)
    for (uint32_t i = threadIdx.x; i < GL; i += blockDim.x) cnt[i] = 0u;
  __syncthreads();
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CO_R * blockDim.x) {
      uint32_t g[CO_R];
      uint64_t ox[CO_R], oy[CO_R];
      co_load(recs, rw, voff_x, voff_y, b0, hi, g, ox, oy);
#pragma unroll
      for (int u = 0; u < CO_R; ++u) {
        const uint32_t k = g[u] - g0;  // (a key below the slice wraps past GL)
        if (k >= GL) continue;
        uint64_t w[W];
        co_contrib<MODE, SQ>(ox[u], oy[u], g[u], dbl, mean, w);
        if (C) atomicAdd(&cnt[k], 1u);
#pragma unroll
        for (int j = 0; j < V; ++j)  // (a zero word -- the high digits of a small square or of a small
                                     // positive product -- costs nothing)
          if (w[j + C]) mom_atomic(co_isf(MODE, j + C), &co_tab[k * V + j], w[j + C]);
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
      const uint64_t v = co_tab[i * V + j];
      if (v) mom_atomic(co_isf(MODE, j + C), &out[(uint64_t)i * W + j + C], v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// beyond LDS: global atomics.  Rows are stored sorted by time and dimension, so keys come in runs:
// when any two neighbouring lanes of a wave hold the same key, every run of equal adjacent keys is
// summed towards its last lane (a segmented shuffle scan bounded by the run's first lane) and that
// lane issues the run's atomics.  With up to 14 words a step the scan is the cost of this tier, so it
// stops at the first distance no run of the wave reaches.

template <int MODE, bool SQ>
__global__ void __launch_bounds__(256) co_global_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff_x,
                                                               int voff_y, const uint32_t* __restrict__ seg_lo,
                                                               const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                               uint32_t G, int dbl, const double* __restrict__ mean,
                                                               uint64_t* __restrict__ state) {
  constexpr int W = co_words(MODE, SQ);
  constexpr int C = co_counts(MODE) ? 1 : 0;
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += CO_R * blockDim.x) {
      uint32_t g[CO_R];
      uint64_t ox[CO_R], oy[CO_R];
      co_load(recs, rw, voff_x, voff_y, b0, hi, g, ox, oy);
#pragma unroll
      for (int u = 0; u < CO_R; ++u) {
        const bool ok = g[u] < G;
        const uint32_t key = ok ? g[u] : 0xffffffffu;
        uint64_t w[W];
        co_contrib<MODE, SQ>(ox[u], oy[u], ok ? g[u] : 0u, dbl, mean, w);
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
            if (take) w[j] = mom_add(co_isf(MODE, j), w[j], t);
          }
        }
        if (!ok || !last) continue;
        uint64_t* s = state + (uint64_t)key * W;
        if (C) atomicAdd((unsigned long long*)s, (unsigned long long)(lane - first + 1));
#pragma unroll
        for (int j = C; j < W; ++j)
          if (w[j]) mom_atomic(co_isf(MODE, j), s + j, w[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// mean[g] = (mean x, mean y) of a pair from its CO_F64_SUM state (0 for an empty group)
__global__ void __launch_bounds__(256) co_mean_kernel(const uint64_t* __restrict__ sum, int G, double* __restrict__ mean) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint64_t n = sum[3 * (int64_t)g];
  mean[2 * (int64_t)g] = n ? __longlong_as_double((long long)sum[3 * (int64_t)g + 1]) / (double)n : 0.0;
  mean[2 * (int64_t)g + 1] = n ? __longlong_as_double((long long)sum[3 * (int64_t)g + 2]) / (double)n : 0.0;
}

// 192-bit two's-complement arithmetic of the finalise (l[0] the lowest limb)
struct Co192 {
  uint64_t l[3];
};

__device__ __forceinline__ Co192 co_add192(Co192 a, Co192 b) {
  Co192 r;
  r.l[0] = a.l[0] + b.l[0];
  const uint64_t c0 = r.l[0] < a.l[0];
  const uint64_t t = a.l[1] + b.l[1];
  r.l[1] = t + c0;
  const uint64_t c1 = (t < a.l[1]) | (r.l[1] < t);
  r.l[2] = a.l[2] + b.l[2] + c1;
  return r;
}

__device__ __forceinline__ Co192 co_neg192(Co192 a) {
  const Co192 n = {{~a.l[0], ~a.l[1], ~a.l[2]}}, one = {{1ull, 0ull, 0ull}};
  return co_add192(n, one);
}

// sum_k d[k] 2^(32 k) of D digit sums, the top one an int64 when `sgn`: the one place a carry moves
__device__ __forceinline__ Co192 co_digits192(const uint64_t* d, int D, bool sgn) {
  Co192 r = {{0ull, 0ull, 0ull}};
  for (int k = 0; k < D; ++k) {
    const uint64_t v = d[k];
    const uint64_t ext = (sgn && k == D - 1 && (int64_t)v < 0) ? ~0ull : 0ull;
    Co192 t = {{ext, ext, ext}};
    const int i = k >> 1;
    if (i > 0) t.l[0] = 0ull;
    if (k & 1) {
      t.l[i] = v << 32;
      t.l[i + 1] = (v >> 32) | (ext << 32);
    } else {
      t.l[i] = v;
    }
    r = co_add192(r, t);
  }
  return r;
}

// n S - a b as (sign, magnitude rounded to double once): S a 192-bit two's-complement sum, a and b
// int64 sums (n < 2^32 rows a shard and |S| < n 2^126: every product stays below 2^191)
__device__ __forceinline__ double co_numerator(uint64_t n, Co192 S, int64_t a, int64_t b) {
  const bool sneg = S.l[2] >> 63;
  const Co192 m = sneg ? co_neg192(S) : S;
  const uint64_t h0 = __umul64hi(n, m.l[0]), t1 = n * m.l[1], h1 = __umul64hi(n, m.l[1]);
  Co192 P;
  P.l[0] = n * m.l[0];
  P.l[1] = t1 + h0;
  P.l[2] = n * m.l[2] + h1 + (P.l[1] < t1);
  if (sneg) P = co_neg192(P);
  const uint64_t ua = a < 0 ? 0ull - (uint64_t)a : (uint64_t)a, ub = b < 0 ? 0ull - (uint64_t)b : (uint64_t)b;
  Co192 Q = {{ua * ub, __umul64hi(ua, ub), 0ull}};
  if (!((a < 0) ^ (b < 0))) Q = co_neg192(Q);  // (subtracting Q: add its negation)
  Co192 A = co_add192(P, Q);
  const bool neg = A.l[2] >> 63;
  if (neg) A = co_neg192(A);
  const double v = mom_limbs_f64(A.l[2], A.l[1], A.l[0]);
  return neg ? -v : v;
}

__device__ __forceinline__ double co_unit(double r) { return r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r; }

// out[g]: kind CO_COVAR, the covariance with `ddof` delta degrees of freedom divided by `div`
// (10^(scale x + scale y) of decimals), NaN where n <= ddof; kind CO_CORR, the correlation, NaN where
// n < 2 or either column is constant in the group, clamped to [-1, 1].
//  integer modes: `a` is the [G][W] state (with squares when `sq`; CO_CORR needs them)
//  CO_F64_DEV:    `a` is the CO_F64_SUM state (for n), `b` the CO_F64_DEV state
__global__ void __launch_bounds__(256) co_final_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                      int G, int mode, int sq, int kind, int ddof, double div,
                                                      double* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int W = mode == CO_F64_DEV ? 3 : co_words(mode, sq);
  const uint64_t n = a[(int64_t)g * W];
  if (kind == CO_CORR ? n < 2 : n <= (uint64_t)ddof) {
    out[g] = nan;
    return;
  }
  if (mode == CO_F64_DEV) {
    const uint64_t* s = b + (int64_t)g * co_words(CO_F64_DEV, sq);
    const double sdx = __longlong_as_double((long long)s[0]), sdy = __longlong_as_double((long long)s[1]);
    const double cxy = __longlong_as_double((long long)s[2]) - sdx * sdy / (double)n;
    if (kind == CO_COVAR) {
      const double c = cxy / (double)(n - (uint64_t)ddof);
      out[g] = div != 1.0 ? c / div : c;
      return;
    }
    const double vx = __longlong_as_double((long long)s[3]) - sdx * sdx / (double)n;
    const double vy = __longlong_as_double((long long)s[4]) - sdy * sdy / (double)n;
    out[g] = (vx > 0.0 && vy > 0.0) ? co_unit(cxy / sqrt(vx * vy)) : nan;
    return;
  }
  const int D = co_digits(mode);
  const uint64_t* s = a + (int64_t)g * W;
  const int64_t sx = (int64_t)s[1], sy = (int64_t)s[2];
  const double A = co_numerator(n, co_digits192(s + 3, D, true), sx, sy);
  if (kind == CO_COVAR) {
    const double c = A / (double)(n * (n - (uint64_t)ddof));
    out[g] = div != 1.0 ? c / div : c;
    return;
  }
  // (never negative by Cauchy-Schwarz unless a sum wrapped, which the sum's contract leaves open)
  const double vx = co_numerator(n, co_digits192(s + 3 + D, D, false), sx, sx);
  const double vy = co_numerator(n, co_digits192(s + 3 + 2 * D, D, false), sy, sy);
  out[g] = (vx > 0.0 && vy > 0.0) ? co_unit(A / sqrt(vx * vy)) : nan;
}

#define CO_INSTANTIATE(K, M, Q, ...)                                                                                 \
  template __global__ void K<M, Q>(const uint32_t*, int, int, int, const uint32_t*, const uint32_t*, int64_t, \
                                   __VA_ARGS__, int, const double*, uint64_t*);
#define CO_INSTANTIATE_MODES(K, ...)                                                        \
  CO_INSTANTIATE(K, CO_INT2, false, __VA_ARGS__) CO_INSTANTIATE(K, CO_INT2, true, __VA_ARGS__) \
  CO_INSTANTIATE(K, CO_INT4, false, __VA_ARGS__) CO_INSTANTIATE(K, CO_INT4, true, __VA_ARGS__) \
  CO_INSTANTIATE(K, CO_F64_SUM, false, __VA_ARGS__)                                         \
  CO_INSTANTIATE(K, CO_F64_DEV, false, __VA_ARGS__) CO_INSTANTIATE(K, CO_F64_DEV, true, __VA_ARGS__)
CO_INSTANTIATE_MODES(co_few_regions_kernel, uint32_t)
CO_INSTANTIATE_MODES(co_lds_regions_kernel, uint32_t, uint32_t)
CO_INSTANTIATE_MODES(co_global_regions_kernel, uint32_t)
#undef CO_INSTANTIATE_MODES
#undef CO_INSTANTIATE

}  // namespace sdo
