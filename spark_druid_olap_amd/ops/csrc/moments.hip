// Exact per-group variance / standard deviation for CDNA4 (gfx950): power sums over a quantile
// producer's chunk-region records.
//
// The JIT producer (ops/jit.py A_QVAL) writes (u32 group key, order-preserving u64 value per
// column) records of the selected rows into its chunk regions (the layout quantile.hip reads); the
// kernels here decode the value back and add up a group's state (moments.h MomMode):
//
//  * integer / decimal columns, ONE pass: n, S1 = sum x, and sum x^2 as carry-free digit sums --
//    |x|^2 (the low product and __umul64hi) is split into 32-bit digits and every digit has its own
//    u64 sum.  Every update is an add; integer adds commute, so the result is bitwise the same
//    under any order of waves, workgroups and atomics.  mom_final_kernel normalises the digits and
//    evaluates (n S2 - S1^2) / (n (n - ddof)) in three 64-bit limbs: one rounding for the numerator,
//    one for the denominator, one for the division (and one for a decimal's scale).
//  * double columns, TWO passes over the same records: n and sum x give the mean (mom_mean_kernel),
//    then sum d and sum d^2 of d = x - mean, and M2 = sum d^2 - (sum d)^2 / n -- the corrected
//    two-pass form, whose error does not grow with (mean / sigma)^2.  f64 adds do not commute
//    bitwise: reproducible to a few ulp only.
//
// Work split by key space (moments.h): mom_few (private LDS rows per wave, a wave loop over the
// distinct keys of 64 records with DPP reductions, no atomics), mom_lds (one LDS table per
// workgroup, LDS atomics; key spaces of several tables take one pass per key slice), mom_global
// (global atomics after a per-wave merge of runs of equal keys).
// Every record loop runs a workgroup-uniform trip count (the ragged end is masked per lane), so the
// cross-lane operations always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moments.h"
#include "moments_dev.h"  // MSIGN, mom_add, mom_atomic, mom_f64, mom_region_end, mom_limbs_f64

namespace sdo {

// the words one record adds to its group's state (`mean` is read in MOM_F64_DEV only)
template <int MODE>
__device__ __forceinline__ void mom_contrib(uint64_t o, uint32_t g, const double* __restrict__ mean,
                                            uint64_t (&w)[mom_words(MODE)]) {
  if constexpr (MODE == MOM_INT2 || MODE == MOM_INT4) {
    const int64_t x = (int64_t)(o ^ MSIGN);
    const uint64_t ax = x < 0 ? 0ull - (uint64_t)x : (uint64_t)x;
    const uint64_t lo = ax * ax;
    w[0] = 1ull;
    w[1] = (uint64_t)x;
    w[2] = lo & 0xffffffffull;
    w[3] = lo >> 32;
    if constexpr (MODE == MOM_INT4) {
      const uint64_t hi = __umul64hi(ax, ax);
      w[4] = hi & 0xffffffffull;
      w[5] = hi >> 32;
    }
  } else if constexpr (MODE == MOM_F64_SUM) {
    w[0] = 1ull;
    w[1] = (uint64_t)__double_as_longlong(mom_f64(o));
  } else {
    const double d = mom_f64(o) - mean[g];
    w[0] = (uint64_t)__double_as_longlong(d);
    w[1] = (uint64_t)__double_as_longlong(d * d);
  }
}

// the R records of this thread in the tile starting at record `b0` of a region ending at `hi`
// (a key of all ones: no record)
__device__ __forceinline__ void mom_load(const uint32_t* __restrict__ recs, int rw, int voff, uint32_t b0, uint32_t hi,
                                         uint32_t (&g)[MOM_R], uint64_t (&o)[MOM_R]) {
#pragma unroll
  for (int u = 0; u < MOM_R; ++u) {
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
// few groups: DPP wave reductions into the wave's private LDS row

template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t mom_dpp(uint64_t v) {  // lanes the move does not reach read 0
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROWS, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xf, false);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// Inclusive scan of the wave in lane order; lane 63 ends with the total.  row_shr:1/2/4/8 scan the
// rows of 16 lanes, row_bcast:15 carries rows 0 and 2 into rows 1 and 3, row_bcast:31 the lower
// half into the upper.  All 64 lanes must be live.
__device__ __forceinline__ uint64_t mom_wave_scan(bool f, uint64_t v) {
  v = mom_add(f, v, mom_dpp<0x111, 0xf>(v));
  v = mom_add(f, v, mom_dpp<0x112, 0xf>(v));
  v = mom_add(f, v, mom_dpp<0x114, 0xf>(v));
  v = mom_add(f, v, mom_dpp<0x118, 0xf>(v));
  v = mom_add(f, v, mom_dpp<0x142, 0xa>(v));
  v = mom_add(f, v, mom_dpp<0x143, 0xc>(v));
  return v;
}

template <int MODE>
__global__ void __launch_bounds__(256) mom_few_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                             const uint32_t* __restrict__ seg_lo,
                                                             const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                             uint32_t G, const double* __restrict__ mean,
                                                             uint64_t* __restrict__ state) {
  constexpr int W = mom_words(MODE);
  __shared__ uint64_t rows[MOM_WAVES * MOM_FEW_G * W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < MOM_WAVES * MOM_FEW_G * W; i += blockDim.x) rows[i] = 0ull;
  __syncthreads();
  uint64_t* row = rows + wave * MOM_FEW_G * W;  // G <= MOM_FEW_G (launcher)
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += MOM_R * blockDim.x) {
      uint32_t g[MOM_R];
      uint64_t o[MOM_R];
      mom_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < MOM_R; ++u) {
        const bool ok = g[u] < G;  // (past the region's end, or a key outside the state: never fault)
        uint64_t w[W];
        mom_contrib<MODE>(o[u], ok ? g[u] : 0u, mean, w);
        uint64_t live = __ballot(ok);
        while (live) {  // (wave-uniform) one trip per distinct key among the wave's 64 records
          const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)g[u], __ffsll((unsigned long long)live) - 1);
          const bool mine = ok && g[u] == k;
          const uint64_t m = __ballot(mine);
#pragma unroll
          for (int j = 0; j < W; ++j) {
            const bool f = mom_isf(MODE, j);
            const uint64_t t = (j == 0 && mom_counts(MODE)) ? (uint64_t)__popcll(m)
                                                            : mom_wave_scan(f, mine ? w[j] : 0ull);
            if (lane == 63) row[k * W + j] = mom_add(f, row[k * W + j], t);
          }
          live &= ~m;
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < G * W; i += blockDim.x) {
    const bool f = mom_isf(MODE, (int)(i % W));
    uint64_t v = rows[i];
#pragma unroll
    for (int wv = 1; wv < MOM_WAVES; ++wv) v = mom_add(f, v, rows[wv * MOM_FEW_G * W + i]);
    if (v) mom_atomic(f, &state[i], v);
  }
}

// ---------------------------------------------------------------------------------------------
// one LDS table per workgroup for the key slice [g0, g0 + GL): [GL][V] u64 words (V = W without the
// count), then [GL] u32 counts.  Records of other slices are skipped: the launcher runs one pass per
// slice (moments.h MOM_LDS_SLICES).

template <int MODE>
__global__ void __launch_bounds__(256) mom_lds_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                             const uint32_t* __restrict__ seg_lo,
                                                             const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                             uint32_t g0, uint32_t GL, const double* __restrict__ mean,
                                                             uint64_t* __restrict__ state) {
  constexpr int W = mom_words(MODE);
  constexpr int C = mom_counts(MODE) ? 1 : 0;
  constexpr int V = W - C;
  extern __shared__ uint64_t mom_tab[];  // GL <= mom_lds_groups(MODE) (launcher)
  uint32_t* cnt = (uint32_t*)(mom_tab + (size_t)GL * V);
  for (uint32_t i = threadIdx.x; i < GL * V; i += blockDim.x) mom_tab[i] = 0ull;
  if (C)
    for (uint32_t i = threadIdx.x; i < GL; i += blockDim.x) cnt[i] = 0u;
  __syncthreads();
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += MOM_R * blockDim.x) {
      uint32_t g[MOM_R];
      uint64_t o[MOM_R];
      mom_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < MOM_R; ++u) {
        const uint32_t k = g[u] - g0;  // (a key below the slice wraps past GL)
        if (k >= GL) continue;
        uint64_t w[W];
        mom_contrib<MODE>(o[u], g[u], mean, w);
        if (C) atomicAdd(&cnt[k], 1u);
#pragma unroll
        for (int j = 0; j < V; ++j)  // (a zero word -- the high digits of a small value -- costs nothing)
          if (w[j + C]) mom_atomic(mom_isf(MODE, j + C), &mom_tab[k * V + j], w[j + C]);
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
      const uint64_t v = mom_tab[i * V + j];
      if (v) mom_atomic(mom_isf(MODE, j + C), &out[(uint64_t)i * W + j + C], v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// beyond LDS: global atomics.  Rows are stored sorted by time and dimension, so keys come in runs:
// when any two neighbouring lanes of a wave hold the same key, every run of equal adjacent keys is
// summed towards its last lane (a segmented shuffle scan bounded by the run's first lane) and that
// lane issues the run's atomics; a wave without equal neighbours skips the scan.

template <int MODE>
__global__ void __launch_bounds__(256) mom_global_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                                const uint32_t* __restrict__ seg_lo,
                                                                const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                                uint32_t G, const double* __restrict__ mean,
                                                                uint64_t* __restrict__ state) {
  constexpr int W = mom_words(MODE);
  constexpr int C = mom_counts(MODE) ? 1 : 0;
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = mom_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += MOM_R * blockDim.x) {
      uint32_t g[MOM_R];
      uint64_t o[MOM_R];
      mom_load(recs, rw, voff, b0, hi, g, o);
#pragma unroll
      for (int u = 0; u < MOM_R; ++u) {
        const bool ok = g[u] < G;
        const uint32_t key = ok ? g[u] : 0xffffffffu;
        uint64_t w[W];
        mom_contrib<MODE>(o[u], ok ? g[u] : 0u, mean, w);
        const uint32_t prev = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || prev != key;
        const uint64_t heads = __ballot(head);
        int first = lane;  // the first lane of this lane's run
        bool last = true;  // ... and whether this lane is its last
        if (heads != ~0ull) {  // (wave-uniform) some run is longer than one lane
          first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
          last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= first;
#pragma unroll
            for (int j = C; j < W; ++j) {
              const uint64_t t = __shfl_up((unsigned long long)w[j], d, 64);
              if (take) w[j] = mom_add(mom_isf(MODE, j), w[j], t);
            }
          }
        }
        if (!ok || !last) continue;
        uint64_t* s = state + (uint64_t)key * W;
        if (C) atomicAdd((unsigned long long*)s, (unsigned long long)(lane - first + 1));
#pragma unroll
        for (int j = C; j < W; ++j)
          if (w[j]) mom_atomic(mom_isf(MODE, j), s + j, w[j]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// mean[g] of a double column from its MOM_F64_SUM state (0 for an empty group)
__global__ void __launch_bounds__(256) mom_mean_kernel(const uint64_t* __restrict__ sum, int G, double* __restrict__ mean) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint64_t n = sum[2 * (int64_t)g];
  mean[g] = n ? __longlong_as_double((long long)sum[2 * (int64_t)g + 1]) / (double)n : 0.0;
}

// out[g] = variance of group g with `ddof` delta degrees of freedom; NaN where n <= ddof.
//  integer modes: `a` is the [G][W] state, (n S2 - S1^2) / (n (n - ddof)) / div, div = 10^(2 scale)
//  MOM_F64_DEV:   `a` is the MOM_F64_SUM state (for n), `b` the MOM_F64_DEV state
__global__ void __launch_bounds__(256) mom_final_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                       int G, int mode, int ddof, double div, double* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int W = mom_words(mode == MOM_F64_DEV ? MOM_F64_SUM : mode);
  const uint64_t n = a[(int64_t)g * W];
  if (n <= (uint64_t)ddof) {
    out[g] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  if (mode == MOM_F64_DEV) {
    const double sd = __longlong_as_double((long long)b[2 * (int64_t)g]);
    const double sd2 = __longlong_as_double((long long)b[2 * (int64_t)g + 1]);
    const double m2 = sd2 - sd * sd / (double)n;
    out[g] = (m2 > 0.0 ? m2 : 0.0) / (double)(n - (uint64_t)ddof);
    return;
  }
  // S2 = sum_k digit_k 2^(32 k) in three limbs (the one place a carry moves)
  uint64_t l0 = 0, l1 = 0, l2 = 0;
  for (int k = 0; k < W - 2; ++k) {
    const uint64_t v = a[(int64_t)g * W + 2 + k];
    const uint64_t vlo = (k & 1) ? v << 32 : v, vhi = (k & 1) ? v >> 32 : 0ull;
    if (k < 2) {
      l0 += vlo;
      const uint64_t c = l0 < vlo;
      l1 += vhi;  // (vhi < 2^32, l1 < 2^33: no carry out here)
      l1 += c;
    } else {
      l1 += vlo;
      const uint64_t c = l1 < vlo;
      l2 += vhi + c;
    }
  }
  // P = n S2 (n < 2^32 rows a shard: below 2^192)
  const uint64_t p0 = n * l0, h0 = __umul64hi(n, l0);
  const uint64_t t1 = n * l1, h1 = __umul64hi(n, l1);
  const uint64_t p1 = t1 + h0;
  const uint64_t p2 = n * l2 + h1 + (p1 < t1);
  // Q = S1^2
  const int64_t s1 = (int64_t)a[(int64_t)g * W + 1];
  const uint64_t a1 = s1 < 0 ? 0ull - (uint64_t)s1 : (uint64_t)s1;
  const uint64_t q0 = a1 * a1, q1 = __umul64hi(a1, a1);
  // P - Q: never negative (Cauchy-Schwarz) unless S1 wrapped, which the sum's contract leaves open
  const uint64_t d0 = p0 - q0;
  const uint64_t br0 = p0 < q0;
  const uint64_t u1 = p1 - q1;
  const uint64_t d1 = u1 - br0;
  const uint64_t br1 = (p1 < q1) | (u1 < br0);
  const uint64_t d2 = p2 - br1;
  const double num = p2 < br1 ? 0.0 : mom_limbs_f64(d2, d1, d0);
  const double var = num / (double)(n * (n - (uint64_t)ddof));
  out[g] = div != 1.0 ? var / div : var;
}

#define MOM_INSTANTIATE(K, M, ...) \
  template __global__ void K<M>(const uint32_t*, int, int, const uint32_t*, const uint32_t*, int64_t, __VA_ARGS__, \
                                const double*, uint64_t*);
#define MOM_INSTANTIATE_MODES(K, ...)       \
  MOM_INSTANTIATE(K, MOM_INT2, __VA_ARGS__) \
  MOM_INSTANTIATE(K, MOM_INT4, __VA_ARGS__) \
  MOM_INSTANTIATE(K, MOM_F64_SUM, __VA_ARGS__) MOM_INSTANTIATE(K, MOM_F64_DEV, __VA_ARGS__)
MOM_INSTANTIATE_MODES(mom_few_regions_kernel, uint32_t)
MOM_INSTANTIATE_MODES(mom_lds_regions_kernel, uint32_t, uint32_t)
MOM_INSTANTIATE_MODES(mom_global_regions_kernel, uint32_t)
#undef MOM_INSTANTIATE_MODES
#undef MOM_INSTANTIATE

}  // namespace sdo
