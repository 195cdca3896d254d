// Exact COUNT(DISTINCT dim) for CDNA4 (gfx950): per-group dictionary-id bitsets over a distinct
// producer's chunk-region records, then a popcount per group.
//
// The JIT producer (ops/jit.py A_DISTINCT) writes (u32 group key, u32 dictionary id per counted
// column) records of the selected rows into its chunk regions (the layout quantile.hip reads); an
// id of all ones marks a row the aggregator's own filter rejected.  The ids lie in [0, D), so the
// exact answer is the popcount of a [G][Wg] u32 bit matrix, Wg = ceil(D / 32): no partitioning,
// hashing, sorting or second aggregation level, and a duplicate -- the common record by far, every
// value appears rows / (G x D) times -- costs one read.
//
//  * dcount_lds_regions -- G x Wg <= 16,384 words: every workgroup keeps a private copy of the
//    whole matrix in LDS, sets bits there (a plain LDS read first, an LDS atomic OR with no return
//    value only for a clear bit) and at the end flushes the words that add a bit to the global
//    word (plain load, then one global atomic OR).
//  * dcount_global_regions -- larger matrices live in HBM.  Per record test-then-set: the word is
//    loaded and only a clear bit is written.  When any lane of a wave has a bit to write, the lanes
//    of a run of equal (group, word) first OR their bits together (a segmented shuffle scan: rows
//    are stored sorted by time and dimension, so keys and ids come in runs) and the run's last
//    lane issues the one atomic.  A wave with nothing to write -- the steady state -- skips the scan.
//  * dcount_count -- popcount of a group's row without the bit of the "" entry (this engine's
//    NULL): one wave per row up to 128 words, one workgroup per row beyond, a cross-lane reduce and
//    one store per group.
//
// Every record loop runs a workgroup-uniform trip count (the ragged end is masked per lane), so the
// shuffles of the global tier always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distinct.h"

namespace sdo {

// the R records of this thread in the tile starting at record `b0` of a region ending at `hi`:
// word index (all ones: nothing to set) and bit of each
__device__ __forceinline__ void dcount_load(const uint32_t* __restrict__ recs, int rw, int voff, uint32_t b0, uint32_t hi,
                                            uint32_t G, uint32_t D, uint32_t Wg, uint32_t (&w)[DCOUNT_R],
                                            uint32_t (&bit)[DCOUNT_R]) {
  uint32_t g[DCOUNT_R], id[DCOUNT_R];
#pragma unroll
  for (int u = 0; u < DCOUNT_R; ++u) {
    const uint32_t i = b0 + u * blockDim.x + threadIdx.x;
    g[u] = 0xffffffffu;
    id[u] = 0xffffffffu;
    if (i < hi) {
      const uint32_t* r = recs + (uint64_t)i * rw;
      g[u] = r[0];
      id[u] = r[voff];
    }
  }
#pragma unroll
  for (int u = 0; u < DCOUNT_R; ++u) {
    // (past the region's end, a filtered-out row, or a key / id outside the matrix: never fault)
    const bool ok = g[u] < G && id[u] < D;
    w[u] = ok ? g[u] * Wg + (id[u] >> 5) : 0xffffffffu;
    bit[u] = 1u << (id[u] & 31u);
  }
}

__global__ void __launch_bounds__(256) dcount_lds_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                                const uint32_t* __restrict__ seg_lo,
                                                                const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                                uint32_t G, uint32_t D, uint32_t Wg,
                                                                uint32_t* __restrict__ state) {
  extern __shared__ uint32_t dc_lds[];
  const uint32_t nw = G * Wg;  // <= DCOUNT_LDS_WORDS (launcher)
  for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) dc_lds[i] = 0u;
  __syncthreads();
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t end = seg_hi[sgi];
    const uint32_t hi = end < lo + DCOUNT_REGION ? end : lo + DCOUNT_REGION;
    for (uint32_t b0 = lo; b0 < hi; b0 += DCOUNT_R * blockDim.x) {
      uint32_t w[DCOUNT_R], bit[DCOUNT_R];
      dcount_load(recs, rw, voff, b0, hi, G, D, Wg, w, bit);
#pragma unroll
      for (int u = 0; u < DCOUNT_R; ++u)
        if (w[u] != 0xffffffffu && !(dc_lds[w[u]] & bit[u])) atomicOr(&dc_lds[w[u]], bit[u]);  // (no return value)
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) {
    const uint32_t v = dc_lds[i];
    // (bits only ever appear in the global word: a stale plain load can only cause a spare atomic)
    if (v && (v & ~state[i])) atomicOr(&state[i], v);
  }
}

__global__ void __launch_bounds__(256) dcount_global_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                                   const uint32_t* __restrict__ seg_lo,
                                                                   const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                                   uint32_t G, uint32_t D, uint32_t Wg,
                                                                   uint32_t* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t end = seg_hi[sgi];
    const uint32_t hi = end < lo + DCOUNT_REGION ? end : lo + DCOUNT_REGION;
    for (uint32_t b0 = lo; b0 < hi; b0 += DCOUNT_R * blockDim.x) {
      uint32_t w[DCOUNT_R], bit[DCOUNT_R], add[DCOUNT_R];
      dcount_load(recs, rw, voff, b0, hi, G, D, Wg, w, bit);
#pragma unroll
      for (int u = 0; u < DCOUNT_R; ++u)  // the test: a duplicate ends here, on a cached read
        add[u] = (w[u] != 0xffffffffu && !(state[w[u]] & bit[u])) ? bit[u] : 0u;
#pragma unroll
      for (int u = 0; u < DCOUNT_R; ++u) {
        if (!__ballot(add[u] != 0u)) continue;  // (wave-uniform)
        // lanes of a run of equal words OR their new bits towards the run's last lane
        uint32_t acc = add[u];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t ow = __shfl_up(w[u], d, 64);
          const uint32_t oa = __shfl_up(acc, d, 64);
          if (lane >= d && ow == w[u]) acc |= oa;
        }
        const uint32_t next = __shfl_down(w[u], 1, 64);
        // (acc != 0 implies a valid word: invalid lanes carry no bits and only merge with each other)
        if (acc && (lane == 63 || next != w[u])) atomicOr(&state[w[u]], acc);
      }
    }
  }
}

// out[g] = popcount of row g without bit `null_id` (-1: none)
template <bool WAVE_ROW>
__global__ void __launch_bounds__(256) dcount_count_kernel(const uint32_t* __restrict__ state, uint32_t G, uint32_t Wg,
                                                          int64_t null_id, int64_t* __restrict__ out) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = WAVE_ROW ? blockIdx.x * 4u + (uint32_t)wave : blockIdx.x;
  const uint32_t nullw = null_id >= 0 ? (uint32_t)(null_id >> 5) : 0xffffffffu;
  const uint32_t nullm = null_id >= 0 ? ~(1u << (uint32_t)(null_id & 31)) : 0xffffffffu;
  uint32_t n = 0;
  if (g < G) {  // (uniform per wave / workgroup)
    const uint32_t* row = state + (uint64_t)g * Wg;
    for (uint32_t i = WAVE_ROW ? lane : threadIdx.x; i < Wg; i += WAVE_ROW ? 64u : blockDim.x) {
      const uint32_t v = row[i];
      n += __popc(i == nullw ? (v & nullm) : v);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if (WAVE_ROW) {
    if (lane == 0 && g < G) out[g] = (int64_t)n;
    return;
  }
  if (lane == 0) wsum[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0 && g < G) out[g] = (int64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template __global__ void dcount_count_kernel<true>(const uint32_t*, uint32_t, uint32_t, int64_t, int64_t*);
template __global__ void dcount_count_kernel<false>(const uint32_t*, uint32_t, uint32_t, int64_t, int64_t*);

}  // namespace sdo
