// Fixed-bucket histograms for CDNA4 (gfx950): per-group bucket counts over a quantile producer's
// chunk-region records.
//
// The JIT producer (ops/jit.py A_QVAL) writes (u32 group key, order-preserving u64 value per column)
// records of the selected rows into its chunk regions (the layout quantile.hip and moments.hip read).
// The host hands the bucket edges over as T = B + 1 ascending thresholds in that same ordered domain
// (ops/buckets.py), so binning is integer comparison only: a record's counter is its upper-bound
// count among the thresholds (histogram.h), and a group's state is S = B + 2 counters
// [below, c_0 .. c_{B-1}, above].  Every update is an integer add, so the counts are exact and
// bitwise the same under any order of lanes, waves, workgroups and atomics.
//
// Every kernel stages the thresholds into LDS once per workgroup, keeps the two top levels of the
// search tree in registers and searches the FBH_R records of a thread level by level together.  Work
// split by counter space (histogram.h): fbh_rep (lane-interleaved copies of the whole table in LDS),
// fbh_lds (one LDS table per key slice, one pass per slice), fbh_global (u64 global atomics after a
// per-wave merge of runs).  Every record loop runs a workgroup-uniform trip count (the ragged end is
// masked per lane), so the cross-lane operations always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "histogram.h"

namespace sdo {

__device__ __forceinline__ uint32_t fbh_region_end(uint32_t lo, uint32_t end) {
  return end < lo + FBH_REGION ? end : lo + FBH_REGION;
}

// the R records of this thread in the tile starting at record `b0` of a region ending at `hi`
// (a key of all ones: no record)
__device__ __forceinline__ void fbh_load(const uint32_t* __restrict__ recs, int rw, int voff, uint32_t b0, uint32_t hi,
                                         uint32_t (&g)[FBH_R], uint64_t (&o)[FBH_R]) {
#pragma unroll
  for (int u = 0; u < FBH_R; ++u) {
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

// The search tree of a workgroup: T thresholds in LDS and its two top levels in registers.
struct FbhTree {
  const uint64_t* thr;  // LDS, T entries
  uint32_t T;
  uint32_t h, q;        // steps of level 0 and 1: h = 2^(levels - 1) <= T, q = h / 2 >= 1 (T >= 2)
  uint64_t t0, t1lo, t1hi;
  bool hi_ok;           // h + q <= T: the upper probe of level 1 exists
  uint64_t nan_lo;
};

// copies the thresholds to `lds` (all threads of the workgroup; ends with a barrier) and reads the top
__device__ __forceinline__ FbhTree fbh_stage(uint64_t* lds, const uint64_t* __restrict__ thr, uint32_t T,
                                             uint64_t nan_lo) {
  for (uint32_t i = threadIdx.x; i < T; i += blockDim.x) lds[i] = thr[i];
  __syncthreads();
  FbhTree t;
  t.thr = lds;
  t.T = T;
  t.h = 1u << (31 - __builtin_clz(T));  // T >= 2 (launcher)
  t.q = t.h >> 1;
  t.hi_ok = t.h + t.q <= T;
  t.t0 = lds[t.h - 1];
  t.t1lo = lds[t.q - 1];
  t.t1hi = lds[(t.hi_ok ? t.h + t.q : T) - 1];
  t.nan_lo = nan_lo;
  return t;
}

// slot[u] = #{i : thr[i] <= o[u]} for the thread's R records, level by level together
__device__ __forceinline__ void fbh_slots(const FbhTree& t, const uint64_t (&o)[FBH_R], uint32_t (&slot)[FBH_R]) {
#pragma unroll
  for (int u = 0; u < FBH_R; ++u) {
    uint32_t pos = t.t0 <= o[u] ? t.h : 0u;
    const bool up = pos != 0u;
    const bool hit = (up ? t.t1hi : t.t1lo) <= o[u];
    if (hit && (!up || t.hi_ok)) pos += t.q;
    slot[u] = pos;
  }
  for (uint32_t step = t.q >> 1; step; step >>= 1) {  // (workgroup-uniform)
#pragma unroll
    for (int u = 0; u < FBH_R; ++u) {
      const uint32_t p = slot[u] + step;
      const uint64_t v = t.thr[(p < t.T ? p : t.T) - 1];
      if (p <= t.T && v <= o[u]) slot[u] = p;
    }
  }
#pragma unroll
  for (int u = 0; u < FBH_R; ++u)
    if (o[u] < t.nan_lo) slot[u] = t.T;
}

#define FBH_ARGS                                                                                                  \
  const uint32_t *__restrict__ recs, int rw, int voff, const uint32_t *__restrict__ seg_lo,                      \
      const uint32_t *__restrict__ seg_hi, int64_t nseg, const uint64_t *__restrict__ thr, uint32_t T, uint64_t nan_lo

// ---------------------------------------------------------------------------------------------
// few counters: R lane-interleaved copies of the [G][S] table, cnt[c * R + (lane & (R - 1))].
// LDS: T thresholds, then G S R <= FBH_LDS_COUNTERS u32 counters (launcher).

__global__ void __launch_bounds__(256) fbh_rep_regions_kernel(FBH_ARGS, uint32_t G, uint32_t R,
                                                             uint64_t* __restrict__ out) {
  extern __shared__ uint64_t fbh_lds[];
  const uint32_t S = T + 1, C = G * S;
  uint32_t* cnt = (uint32_t*)(fbh_lds + T);
  for (uint32_t i = threadIdx.x; i < C * R; i += blockDim.x) cnt[i] = 0u;
  const FbhTree tree = fbh_stage(fbh_lds, thr, T, nan_lo);  // (barrier: the counters are cleared too)
  const uint32_t copy = threadIdx.x & (R - 1);
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = fbh_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += FBH_R * blockDim.x) {
      uint32_t g[FBH_R], slot[FBH_R];
      uint64_t o[FBH_R];
      fbh_load(recs, rw, voff, b0, hi, g, o);
      fbh_slots(tree, o, slot);
#pragma unroll
      for (int u = 0; u < FBH_R; ++u)  // (past the region's end, or a key outside the state: never fault)
        if (g[u] < G) atomicAdd(&cnt[(g[u] * S + slot[u]) * R + copy], 1u);
    }
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < C; c += blockDim.x) {
    uint32_t n = 0;
    for (uint32_t r = 0; r < R; ++r) n += cnt[c * R + ((r + threadIdx.x) & (R - 1))];  // (rotated: fewer bank conflicts)
    if (n) atomicAdd((unsigned long long*)&out[c], (unsigned long long)n);
  }
}

// ---------------------------------------------------------------------------------------------
// one LDS table per workgroup for the key slice [g0, g0 + GL): [GL][S] u32 counters after the T
// thresholds, GL S <= FBH_LDS_COUNTERS (launcher).  Records of other slices are skipped: the launcher
// runs one pass per slice.

__global__ void __launch_bounds__(256) fbh_lds_regions_kernel(FBH_ARGS, uint32_t g0, uint32_t GL,
                                                             uint64_t* __restrict__ out) {
  extern __shared__ uint64_t fbh_lds[];
  const uint32_t S = T + 1, C = GL * S;
  uint32_t* cnt = (uint32_t*)(fbh_lds + T);
  for (uint32_t i = threadIdx.x; i < C; i += blockDim.x) cnt[i] = 0u;
  const FbhTree tree = fbh_stage(fbh_lds, thr, T, nan_lo);
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = fbh_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += FBH_R * blockDim.x) {
      uint32_t g[FBH_R], slot[FBH_R];
      uint64_t o[FBH_R];
      fbh_load(recs, rw, voff, b0, hi, g, o);
      fbh_slots(tree, o, slot);
#pragma unroll
      for (int u = 0; u < FBH_R; ++u) {
        const uint32_t k = g[u] - g0;  // (a key below the slice wraps past GL)
        if (k < GL) atomicAdd(&cnt[k * S + slot[u]], 1u);
      }
    }
  }
  __syncthreads();
  uint64_t* o64 = out + (uint64_t)g0 * S;
  for (uint32_t c = threadIdx.x; c < C; c += blockDim.x) {
    const uint32_t n = cnt[c];
    if (n) atomicAdd((unsigned long long*)&o64[c], (unsigned long long)n);
  }
}

// ---------------------------------------------------------------------------------------------
// beyond LDS: u64 global atomics.  Rows are stored sorted by time and dimension, so (group, slot)
// pairs come in runs: the last lane of every run of equal adjacent counters adds the run's length.
// LDS: the T thresholds only.

__global__ void __launch_bounds__(256) fbh_global_regions_kernel(FBH_ARGS, uint32_t G, uint64_t* __restrict__ out) {
  extern __shared__ uint64_t fbh_lds[];
  const uint32_t S = T + 1;
  const FbhTree tree = fbh_stage(fbh_lds, thr, T, nan_lo);
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = fbh_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += FBH_R * blockDim.x) {
      uint32_t g[FBH_R], slot[FBH_R];
      uint64_t o[FBH_R];
      fbh_load(recs, rw, voff, b0, hi, g, o);
      fbh_slots(tree, o, slot);
#pragma unroll
      for (int u = 0; u < FBH_R; ++u) {
        const bool ok = g[u] < G;
        const uint64_t c = ok ? (uint64_t)g[u] * S + slot[u] : ~0ull;  // (G S < 2^26: never all ones)
        const uint64_t prev = __shfl_up((unsigned long long)c, 1, 64);
        const uint64_t heads = __ballot(lane == 0 || prev != c);
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the first lane of this run
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (ok && last) atomicAdd((unsigned long long*)&out[c], (unsigned long long)(lane - first + 1));
      }
    }
  }
}

#undef FBH_ARGS

}  // namespace sdo
