// Exact per-group order statistics for CDNA4 (gfx950): percentile / median / percentile_approx
// pushed down as a multi-level radix RANK select over a quantile producer's chunk-region records.
//
// The JIT producer (ops/jit.py A_QVAL) writes (u32 group key, order-preserving u64 value per
// quantile column) records of the selected rows into its chunk regions; every kernel here reads the
// regions in place (the layout sketch.hip theta_*_regions read).  Unlike the theta select -- one
// histogram of uniform hashes, then a sort of ~2k candidates -- metric values are duplicate heavy
// (l_quantity: 50 distinct values over 600M rows), so nothing here keeps candidates: the select
// resolves the value itself, B bits a level, and a bin holding every row costs nothing extra.
//
// State rows are (g, t): t indexes the group's rank targets (two per interpolated fraction -- the
// ranks floor(pos) and ceil(pos) -- one per non-interpolated fraction).
//
//  * qsel_stats_regions -- per-group count / min / max of the ordered value.  A thread folds runs
//    of equal keys in registers, a workgroup folds them in LDS tables (LDS atomics; groups beyond
//    the LDS budget go straight to global atomics), and each touched group costs one global
//    count / min / max update per workgroup.
//  * qsel_width -- per group the bit length w_g of (max - min), and the largest over the groups
//    (the host's one read before the result copy: it sets the digit width and the level count).
//  * qsel_hist_regions(level) -- per record and per target row of its group whose resolved prefix
//    equals the record's bits above this level's digit: one bump of bin `digit` in a per-workgroup
//    LDS histogram [rows][2^B] (level 0: no prefix yet, the group's targets share ONE row), flushed
//    with one global add per non-empty bin.  Above the LDS budget the bins are global.
//  * qsel_pick(level) -- one workgroup per row: wave-shuffle prefix scan of the row's bins, the bin
//    where the running count passes the row's remaining rank joins the prefix, the count below it
//    leaves the rank.  Level 0 first derives the rank from the group's count and the fraction.
//  * qsel_final -- min_g + prefix IS the order statistic: per (group, fraction) the raw element or
//    the interpolated double lo + (hi - lo) * (pos - floor(pos)).
//
// Group g works on d = value - min_g, w_g bits wide, in L_g = ceil(w_g / B) levels: level l reads
// the digit at bit B * (L_g - 1 - l), so a narrow group resolves its exact value in its first
// levels and idles afterwards (its records are skipped) while wide groups continue.
//
// Digit width B (host, engine/device_exec.py PreparedQuantile): the widest 4 <= B <= 12 for which
// [G x T][2^B] u32 bins fit the 64 KiB LDS budget the theta histogram uses, then narrowed to
// ceil(W / levels) -- the same number of passes over the records with the fewest bins, since every
// workgroup clears, scans and flushes all of its bins (the theta path measured that flush: 0.44 ms
// a pass for 14K bins x 4096 workgroups).  More rows than fit: global bins with B = 8 (256 bins a
// row keep a 5,000-group x 10-target state at 51 MB and 64-bit values at 8 levels).  Which B is
// fastest has not been measured; the choice only bounds passes and LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quantile.h"

namespace sdo {

static constexpr uint64_t QSIGN = 0x8000000000000000ull;

__device__ __forceinline__ int qsel_levels(int w, int B) { return (w + B - 1) / B; }

// 0-based rank of target t of a group of n rows (n >= 1): Spark's percentile reads the ranks
// floor(p (n-1)) and ceil(p (n-1)); percentile_approx the one rank max(0, ceil(p n) - 1).
__device__ __forceinline__ uint64_t qsel_rank(double p, uint64_t n, int interpolate, int t) {
  if (interpolate) {
    const double pos = p * (double)(n - 1);
    const double r = (t & 1) ? ceil(pos) : floor(pos);
    const uint64_t k = (uint64_t)r;
    return k > n - 1 ? n - 1 : k;
  }
  const double c = ceil(p * (double)n);
  const uint64_t k = c >= 1.0 ? (uint64_t)c - 1 : 0;
  return k > n - 1 ? n - 1 : k;
}

__global__ void __launch_bounds__(256) qsel_init_kernel(uint32_t* __restrict__ cnt, uint64_t* __restrict__ mn,
                                                       uint64_t* __restrict__ mx, int G, uint32_t* __restrict__ wmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) wmax[0] = 0u;
  if (i < G) {
    cnt[i] = 0u;
    mn[i] = ~0ull;
    mx[i] = 0ull;
  }
}

__global__ void __launch_bounds__(256) qsel_clear_kernel(uint32_t* __restrict__ p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

// LDS tables: cnt[GL] u32, then mn[GL], mx[GL] u64 (GL = min(G, groups the budget holds))
__global__ void __launch_bounds__(256) qsel_stats_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                                const uint32_t* __restrict__ seg_lo,
                                                                const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                                int G, int GL, uint32_t* __restrict__ cnt,
                                                                uint64_t* __restrict__ mn, uint64_t* __restrict__ mx) {
  extern __shared__ uint64_t qs_lds[];
  unsigned long long* lmn = (unsigned long long*)qs_lds;
  unsigned long long* lmx = lmn + GL;
  uint32_t* lcnt = (uint32_t*)(lmx + GL);
  for (int i = threadIdx.x; i < GL; i += blockDim.x) {
    lcnt[i] = 0u;
    lmn[i] = ~0ull;
    lmx[i] = 0ull;
  }
  __syncthreads();
  // the thread's current run of equal keys
  uint32_t cg = 0xffffffffu, cc = 0;
  uint64_t cmn = ~0ull, cmx = 0ull;
  auto flush = [&]() {
    if (cc == 0) return;
    if (cg < (uint32_t)GL) {
      atomicAdd(&lcnt[cg], cc);
      atomicMin(&lmn[cg], (unsigned long long)cmn);
      atomicMax(&lmx[cg], (unsigned long long)cmx);
    } else {
      atomicAdd(&cnt[cg], cc);
      atomicMin((unsigned long long*)&mn[cg], (unsigned long long)cmn);
      atomicMax((unsigned long long*)&mx[cg], (unsigned long long)cmx);
    }
  };
  constexpr int R = 4;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi], hi = seg_hi[sgi];
    for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += R * blockDim.x) {
      uint32_t g[R];
      uint64_t o[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const uint32_t i = i0 + u * blockDim.x;
        g[u] = 0xffffffffu;
        o[u] = 0;
        if (i < hi) {
          const uint32_t* r = recs + (uint64_t)i * rw;
          g[u] = r[0];
          o[u] = (uint64_t)r[voff] | ((uint64_t)r[voff + 1] << 32);
        }
      }
#pragma unroll
      for (int u = 0; u < R; ++u) {
        if (g[u] >= (uint32_t)G) continue;  // (past the region's end; never fault)
        if (g[u] != cg) {
          flush();
          cg = g[u];
          cc = 0;
          cmn = ~0ull;
          cmx = 0ull;
        }
        ++cc;
        cmn = o[u] < cmn ? o[u] : cmn;
        cmx = o[u] > cmx ? o[u] : cmx;
      }
    }
  }
  flush();
  __syncthreads();
  for (int i = threadIdx.x; i < GL; i += blockDim.x) {
    if (!lcnt[i]) continue;
    atomicAdd(&cnt[i], lcnt[i]);
    atomicMin((unsigned long long*)&mn[i], lmn[i]);
    atomicMax((unsigned long long*)&mx[i], lmx[i]);
  }
}

__global__ void __launch_bounds__(256) qsel_width_kernel(const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ mn,
                                                        const uint64_t* __restrict__ mx, int G,
                                                        uint32_t* __restrict__ width, uint32_t* __restrict__ wmax) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t w = 0;
  if (g < G) {
    if (cnt[g]) {
      const uint64_t d = mx[g] - mn[g];
      w = d ? 64u - (uint32_t)__builtin_clzll(d) : 0u;
    }
    width[g] = w;
  }
  // one atomic per wave
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t t = __shfl_xor(w, d, 64);
    w = t > w ? t : w;
  }
  if ((threadIdx.x & 63) == 0 && w) atomicMax(wmax, w);
}

__global__ void __launch_bounds__(256) qsel_hist_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                               const uint32_t* __restrict__ seg_lo,
                                                               const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                               QselState s, int level, int use_lds) {
  extern __shared__ uint32_t qh_lds[];
  const int G = s.G, T = s.T, B = s.B;
  const int64_t rows = level == 0 ? (int64_t)G : (int64_t)G * T;
  const int64_t nb = rows << B;
  const uint64_t dmask = (1ull << B) - 1ull;
  if (use_lds) {
    for (int64_t i = threadIdx.x; i < nb; i += blockDim.x) qh_lds[i] = 0u;
    __syncthreads();
  }
  uint32_t* hist = use_lds ? qh_lds : s.hist;
  constexpr int R = 4;  // records in flight per thread (loads issued before the atomics)
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi], hi = seg_hi[sgi];
    for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += R * blockDim.x) {
      uint32_t g[R];
      uint64_t o[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const uint32_t i = i0 + u * blockDim.x;
        g[u] = 0xffffffffu;
        o[u] = 0;
        if (i < hi) {
          const uint32_t* r = recs + (uint64_t)i * rw;
          g[u] = r[0];
          o[u] = (uint64_t)r[voff] | ((uint64_t)r[voff + 1] << 32);
        }
      }
#pragma unroll
      for (int u = 0; u < R; ++u) {
        if (g[u] >= (uint32_t)G) continue;  // (past the region's end; never fault)
        const int L = qsel_levels((int)s.width[g[u]], B);
        if (level >= L) continue;  // the group's value is resolved (or constant): idle
        const int sh = B * (L - 1 - level);  // < w_g <= 64
        const uint64_t d = o[u] - s.mn[g[u]];
        const uint32_t digit = (uint32_t)((d >> sh) & dmask);
        if (level == 0) {
          atomicAdd(&hist[((int64_t)g[u] << B) + digit], 1u);
          continue;
        }
        const uint64_t hp = d >> (sh + B);  // sh + B = B (L - level) <= B (L - 1) < w_g <= 64
        const int64_t r0 = (int64_t)g[u] * T;
        for (int t = 0; t < T; ++t)
          if (s.prefix[r0 + t] == hp) atomicAdd(&hist[((r0 + t) << B) + digit], 1u);
      }
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < nb; i += blockDim.x)
      if (qh_lds[i]) atomicAdd(&s.hist[i], qh_lds[i]);
  }
}

// one 256-thread workgroup per row (g, t); 2^B <= 4096 bins, <= 16 consecutive bins per thread
__global__ void __launch_bounds__(256) qsel_pick_kernel(QselState s, int level) {
  __shared__ uint32_t wsum[4];
  const int64_t row = blockIdx.x;
  const int g = (int)(row / s.T), t = (int)(row % s.T);
  const uint32_t n = s.cnt[g];
  const int L = qsel_levels((int)s.width[g], s.B);
  if (level == 0 && threadIdx.x == 0) {
    s.prefix[row] = 0ull;
    s.rank[row] = n ? qsel_rank(s.frac[s.interpolate ? (t >> 1) : t], n, s.interpolate, t) : 0ull;
  }
  if (n == 0 || level >= L) return;  // (uniform per workgroup)
  __syncthreads();
  const uint64_t want = s.rank[row];
  const int nb = 1 << s.B;
  const int per = nb >= 256 ? nb / 256 : 1;
  const uint32_t* h = s.hist + ((level == 0 ? (int64_t)g : row) << s.B);
  const int b0 = threadIdx.x * per;
  uint32_t v[16];
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = (j < per && b0 + j < nb) ? h[b0 + j] : 0u;
    mine += v[j];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint64_t before = 0;
  for (int w = 0; w < wave; ++w) before += wsum[w];
  uint64_t below = before + x - mine;  // rows of the bins before this thread's
  if (mine && below <= want && want < below + mine) {
    // (exactly one thread: the remaining rank is below the row's candidate count by induction)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (want < below + v[j]) {
        s.prefix[row] = (level == 0 ? 0ull : (s.prefix[row] << s.B)) | (uint64_t)(b0 + j);
        s.rank[row] = want - below;
        break;
      }
      below += v[j];
    }
  }
}

__device__ __forceinline__ double qsel_value(uint64_t o, int is_f64, double div) {
  if (is_f64) {
    const int64_t b = (int64_t)(o ^ QSIGN);  // the signed order f2ord gave
    return __longlong_as_double(b >= 0 ? b : (b ^ 0x7fffffffffffffffLL));
  }
  const double v = (double)(int64_t)(o ^ QSIGN);
  return div != 1.0 ? v / div : v;
}

// out[g][f] (64-bit): the interpolated double, or the element itself -- double bits for a double
// column, the raw int64 for an integer / decimal one (the host applies a decimal's scale)
__global__ void __launch_bounds__(256) qsel_final_kernel(QselState s, int nfrac, int is_f64, double div,
                                                        uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)s.G * nfrac) return;
  const int g = (int)(i / nfrac), f = (int)(i % nfrac);
  const uint32_t n = s.cnt[g];
  if (n == 0) {
    out[i] = 0ull;
    return;
  }
  const bool flat = s.width[g] == 0;  // constant group: no level ran
  const uint64_t m = s.mn[g];
  if (!s.interpolate) {
    const uint64_t o = flat ? m : m + s.prefix[(int64_t)g * s.T + f];
    if (is_f64) out[i] = (uint64_t)__double_as_longlong(qsel_value(o, 1, 1.0));
    else out[i] = o ^ QSIGN;
    return;
  }
  const int64_t r0 = (int64_t)g * s.T + 2 * f;
  const double lo = qsel_value(flat ? m : m + s.prefix[r0], is_f64, div);
  const double hi = qsel_value(flat ? m : m + s.prefix[r0 + 1], is_f64, div);
  const double pos = s.frac[f] * (double)(n - 1);
  // (anchored at the nearer rank, as numpy's lerp: no cancellation error when lo and hi differ in sign)
  const double gm = pos - floor(pos);
  const double res = gm >= 0.5 ? hi - (hi - lo) * (1.0 - gm) : lo + (hi - lo) * gm;
  out[i] = (uint64_t)__double_as_longlong(res);
}

}  // namespace sdo
