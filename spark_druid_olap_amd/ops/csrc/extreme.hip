// max_by / min_by for CDNA4 (gfx950): per-group packed-key extremes over a producer's chunk-region
// records.
//
// The JIT producer (ops/jit.py A_ROWID + A_QVAL) writes (u32 group key, u32 row id, order-preserving
// u64 value per ordering column) records of the selected rows into its chunk regions.  max_by(x, y)
// is the payload x of the row with the lexicographic maximum of (y, row id), min_by(x, y) that of the
// minimum: ONE u64 key per (group, direction) whose integer max / min is that extreme (extreme.h
// ExtMode).  Integer max / min is associative, commutative and idempotent, so the state is bitwise
// the same under any order of lanes, waves, workgroups and atomics.  The payload is not in the
// record: ext_final_kernel decodes the row id and gathers any number of payload columns by it.
//
//  * EXT_PACKED, one pass: ord32(y) << 32 | (row id + 1).
//  * EXT_WIDE_VAL then EXT_WIDE_ROW, two passes over the same records: the extreme of the ordered
//    u64, then the extreme of (row id + 1) among the records that hold it.
//
// Work split by key space (extreme.h): ext_few (a wave loop over the distinct keys of 64 records
// with DPP max / min into private LDS rows, no atomics), ext_lds (64-bit LDS atomic max / min on a
// per-workgroup table, one pass per key slice), ext_global (global atomics after a per-wave merge
// of runs of equal keys).  Every record loop runs a workgroup-uniform trip count (the ragged end is
// masked per lane), so the cross-lane operations always see 64 live lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "extreme.h"

namespace sdo {

static constexpr uint64_t EXT_ONES = ~0ull;

// identity of state word d of a DIRS state
template <int DIRS>
__device__ __forceinline__ constexpr uint64_t ext_ident(int d) {
  return (DIRS == EXT_MIN || d == 1) ? EXT_ONES : 0ull;
}
template <int DIRS>
__device__ __forceinline__ constexpr bool ext_ismax(int d) {
  return DIRS != EXT_MIN && d == 0;
}
__device__ __forceinline__ uint64_t ext_fold(bool mx, uint64_t a, uint64_t b) {
  return mx ? (a > b ? a : b) : (a < b ? a : b);
}
// (no return value used: one LDS / global 64-bit atomic max or min instruction)
__device__ __forceinline__ void ext_atomic(bool mx, uint64_t* p, uint64_t v) {
  if (mx) atomicMax((unsigned long long*)p, (unsigned long long)v);
  else atomicMin((unsigned long long*)p, (unsigned long long)v);
}

__device__ __forceinline__ uint32_t ext_region_end(uint32_t lo, uint32_t end) {
  return end < lo + EXT_REGION ? end : lo + EXT_REGION;
}

// the R records of this thread in the tile starting at record `b0` of a region ending at `hi`
// (a key of all ones: no record).  `voff` 0: the record carries no value (ordering by time).
__device__ __forceinline__ void ext_load(const uint32_t* __restrict__ recs, int rw, int voff, uint32_t b0, uint32_t hi,
                                         uint32_t (&g)[EXT_R], uint32_t (&rid)[EXT_R], uint64_t (&o)[EXT_R]) {
#pragma unroll
  for (int u = 0; u < EXT_R; ++u) {
    const uint32_t i = b0 + u * blockDim.x + threadIdx.x;
    g[u] = 0xffffffffu;
    rid[u] = 0u;
    o[u] = 0ull;
    if (i < hi) {
      const uint32_t* r = recs + (uint64_t)i * rw;
      g[u] = r[0];
      rid[u] = r[1];
      if (voff) o[u] = (uint64_t)r[voff] | ((uint64_t)r[voff + 1] << 32);
    }
  }
}

// the key one record offers to each word of its group's state (`ok`: a record of a group in range;
// `ext` is read in EXT_WIDE_ROW only)
template <int MODE, int DIRS>
__device__ __forceinline__ void ext_contrib(bool ok, uint32_t g, uint32_t rid, uint64_t o, int voff,
                                            const uint64_t* __restrict__ ext, uint64_t (&k)[ext_words(DIRS)]) {
  constexpr int D = ext_words(DIRS);
#pragma unroll
  for (int d = 0; d < D; ++d) k[d] = ext_ident<DIRS>(d);
  if (!ok) return;
  const uint64_t row1 = (uint64_t)rid + 1ull;
  if constexpr (MODE == EXT_PACKED) {
    const uint64_t key = (voff ? (uint64_t)((uint32_t)o ^ 0x80000000u) << 32 : 0ull) | row1;
#pragma unroll
    for (int d = 0; d < D; ++d) k[d] = key;
  } else if constexpr (MODE == EXT_WIDE_VAL) {
#pragma unroll
    for (int d = 0; d < D; ++d) k[d] = o;
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (ext[(uint64_t)g * D + d] == o) k[d] = row1;
  }
}

// ---------------------------------------------------------------------------------------------
// few groups: DPP wave reductions into the wave's private LDS row

template <int CTRL, int ROWS, bool MX>
__device__ __forceinline__ uint64_t ext_dpp(uint64_t v) {  // lanes the move does not reach read the identity
  constexpr int OLD = MX ? 0 : -1;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(OLD, (int)(uint32_t)v, CTRL, ROWS, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(OLD, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xf, false);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// Max / min of the wave; lane 63 ends with it.  row_shr:1/2/4/8 fold the rows of 16 lanes towards
// their last lane, row_bcast:15 carries rows 0 and 2 into rows 1 and 3, row_bcast:31 the lower half
// into the upper.  All 64 lanes must be live.
template <bool MX>
__device__ __forceinline__ uint64_t ext_wave_fold(uint64_t v) {
  v = ext_fold(MX, v, ext_dpp<0x111, 0xf, MX>(v));
  v = ext_fold(MX, v, ext_dpp<0x112, 0xf, MX>(v));
  v = ext_fold(MX, v, ext_dpp<0x114, 0xf, MX>(v));
  v = ext_fold(MX, v, ext_dpp<0x118, 0xf, MX>(v));
  v = ext_fold(MX, v, ext_dpp<0x142, 0xa, MX>(v));
  v = ext_fold(MX, v, ext_dpp<0x143, 0xc, MX>(v));
  return v;
}

template <int MODE, int DIRS>
__global__ void __launch_bounds__(256) ext_few_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                             const uint32_t* __restrict__ seg_lo,
                                                             const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                             uint32_t G, const uint64_t* __restrict__ ext,
                                                             uint64_t* __restrict__ state) {
  constexpr int D = ext_words(DIRS);
  __shared__ uint64_t rows[EXT_WAVES * EXT_FEW_G * D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < EXT_WAVES * EXT_FEW_G * D; i += blockDim.x) rows[i] = ext_ident<DIRS>(i % D);
  __syncthreads();
  uint64_t* row = rows + wave * EXT_FEW_G * D;  // G <= EXT_FEW_G (launcher)
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = ext_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += EXT_R * blockDim.x) {
      uint32_t g[EXT_R], rid[EXT_R];
      uint64_t o[EXT_R];
      ext_load(recs, rw, voff, b0, hi, g, rid, o);
#pragma unroll
      for (int u = 0; u < EXT_R; ++u) {
        const bool ok = g[u] < G;  // (past the region's end, or a key outside the state: never fault)
        uint64_t k[D];
        ext_contrib<MODE, DIRS>(ok, g[u], rid[u], o[u], voff, ext, k);
        uint64_t live = __ballot(ok);
        while (live) {  // (wave-uniform) one trip per distinct key among the wave's 64 records
          const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)g[u], __ffsll((unsigned long long)live) - 1);
          const bool mine = ok && g[u] == key;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            constexpr uint64_t I0 = ext_ident<DIRS>(0), I1 = ext_ident<DIRS>(1);
            const uint64_t v = mine ? k[d] : (d ? I1 : I0);
            const uint64_t t = ext_ismax<DIRS>(d) ? ext_wave_fold<true>(v) : ext_wave_fold<false>(v);
            if (lane == 63) row[key * D + d] = ext_fold(ext_ismax<DIRS>(d), row[key * D + d], t);
          }
          live &= ~__ballot(mine);
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < G * D; i += blockDim.x) {
    const int d = (int)(i % D);
    const bool mx = ext_ismax<DIRS>(d);
    uint64_t v = rows[i];
#pragma unroll
    for (int wv = 1; wv < EXT_WAVES; ++wv) v = ext_fold(mx, v, rows[wv * EXT_FEW_G * D + i]);
    if (v != ext_ident<DIRS>(d)) ext_atomic(mx, &state[i], v);
  }
}

// ---------------------------------------------------------------------------------------------
// one LDS table per workgroup for the key slice [g0, g0 + GL): [GL][D] u64 keys.  Records of other
// slices are skipped: the launcher runs one pass per slice (extreme.h EXT_LDS_SLICES).

template <int MODE, int DIRS>
__global__ void __launch_bounds__(256) ext_lds_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                             const uint32_t* __restrict__ seg_lo,
                                                             const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                             uint32_t g0, uint32_t GL, const uint64_t* __restrict__ ext,
                                                             uint64_t* __restrict__ state) {
  constexpr int D = ext_words(DIRS);
  extern __shared__ uint64_t ext_tab[];  // GL <= ext_lds_groups(DIRS) (launcher)
  for (uint32_t i = threadIdx.x; i < GL * D; i += blockDim.x) ext_tab[i] = ext_ident<DIRS>(i % D);
  __syncthreads();
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = ext_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += EXT_R * blockDim.x) {
      uint32_t g[EXT_R], rid[EXT_R];
      uint64_t o[EXT_R];
      ext_load(recs, rw, voff, b0, hi, g, rid, o);
#pragma unroll
      for (int u = 0; u < EXT_R; ++u) {
        const uint32_t s = g[u] - g0;  // (a key below the slice wraps past GL)
        if (s >= GL) continue;
        uint64_t k[D];
        ext_contrib<MODE, DIRS>(true, g[u], rid[u], o[u], voff, ext, k);
#pragma unroll
        for (int d = 0; d < D; ++d)  // (EXT_WIDE_ROW: a record that does not hold the extreme offers nothing)
          if (k[d] != ext_ident<DIRS>(d)) ext_atomic(ext_ismax<DIRS>(d), &ext_tab[s * D + d], k[d]);
      }
    }
  }
  __syncthreads();
  uint64_t* out = state + (uint64_t)g0 * D;
  for (uint32_t i = threadIdx.x; i < GL * D; i += blockDim.x) {
    const int d = (int)(i % D);
    const uint64_t v = ext_tab[i];
    if (v != ext_ident<DIRS>(d)) ext_atomic(ext_ismax<DIRS>(d), &out[i], v);
  }
}

// ---------------------------------------------------------------------------------------------
// beyond LDS: global atomics.  Rows are stored sorted by time and dimension, so keys come in runs:
// when any two neighbouring lanes of a wave hold the same key, every run of equal adjacent keys is
// folded towards its last lane (a segmented shuffle scan bounded by the run's first lane) and that
// lane issues the run's atomics; a wave without equal neighbours skips the scan.

template <int MODE, int DIRS>
__global__ void __launch_bounds__(256) ext_global_regions_kernel(const uint32_t* __restrict__ recs, int rw, int voff,
                                                                const uint32_t* __restrict__ seg_lo,
                                                                const uint32_t* __restrict__ seg_hi, int64_t nseg,
                                                                uint32_t G, const uint64_t* __restrict__ ext,
                                                                uint64_t* __restrict__ state) {
  constexpr int D = ext_words(DIRS);
  const int lane = threadIdx.x & 63;
  for (int64_t sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
    const uint32_t lo = seg_lo[sgi];
    const uint32_t hi = ext_region_end(lo, seg_hi[sgi]);
    for (uint32_t b0 = lo; b0 < hi; b0 += EXT_R * blockDim.x) {
      uint32_t g[EXT_R], rid[EXT_R];
      uint64_t o[EXT_R];
      ext_load(recs, rw, voff, b0, hi, g, rid, o);
#pragma unroll
      for (int u = 0; u < EXT_R; ++u) {
        const bool ok = g[u] < G;
        const uint32_t key = ok ? g[u] : 0xffffffffu;
        uint64_t k[D];
        ext_contrib<MODE, DIRS>(ok, g[u], rid[u], o[u], voff, ext, k);
        const uint32_t prev = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || prev != key;
        const uint64_t heads = __ballot(head);
        bool last = true;  // whether this lane is the last of its run
        if (heads != ~0ull) {  // (wave-uniform) some run is longer than one lane
          const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
          last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
          for (int s = 1; s < 64; s <<= 1) {
            const bool take = lane - s >= first;
#pragma unroll
            for (int d = 0; d < D; ++d) {
              const uint64_t t = __shfl_up((unsigned long long)k[d], s, 64);
              if (take) k[d] = ext_fold(ext_ismax<DIRS>(d), k[d], t);
            }
          }
        }
        if (!ok || !last) continue;
#pragma unroll
        for (int d = 0; d < D; ++d)
          if (k[d] != ext_ident<DIRS>(d)) ext_atomic(ext_ismax<DIRS>(d), &state[(uint64_t)key * D + d], k[d]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// state[i] = the identity of its word (a [G][D] state of `dirs`, n = G D words)
__global__ void __launch_bounds__(256) ext_init_kernel(uint64_t* __restrict__ state, int64_t n, int dirs) {
  const int D = ext_words(dirs);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    state[i] = (dirs == EXT_MIN || i % D == 1) ? EXT_ONES : 0ull;
}

// Per payload p (blockIdx.y) and group g: the row id in the low word of its state word, the payload
// of that row at its stored type, out[g] as int64 or f64 (a decimal: x / div).  A group no record
// reached still holds an identity (low word 0 or all ones: no row id) and answers 0.
__global__ void __launch_bounds__(256) ext_final_kernel(ExtFinalArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.G || (int)blockIdx.y >= a.n) return;
  const ExtPayload& p = a.p[blockIdx.y];
  const int64_t row = (int64_t)(uint32_t)p.state[(int64_t)g * p.D + p.word] - 1;
  const bool has = row >= 0 && row < a.rows;
  int64_t iv = 0;
  double fv = 0.0;
  if (has) {
    switch (p.type) {
      case EXT_I8: iv = ((const int8_t*)p.col)[row]; break;
      case EXT_U8: iv = ((const uint8_t*)p.col)[row]; break;
      case EXT_I16: iv = ((const int16_t*)p.col)[row]; break;
      case EXT_I32: iv = ((const int32_t*)p.col)[row]; break;
      case EXT_I64: iv = ((const int64_t*)p.col)[row]; break;
      case EXT_F32: fv = (double)((const float*)p.col)[row]; break;
      default: fv = ((const double*)p.col)[row]; break;
    }
  }
  if (p.type >= EXT_F32) p.out[g] = (uint64_t)__double_as_longlong(fv);
  else if (p.div != 0.0) p.out[g] = (uint64_t)__double_as_longlong((double)iv / p.div);
  else p.out[g] = (uint64_t)iv;
}

#define EXT_INSTANTIATE(K, M, DR, ...) \
  template __global__ void K<M, DR>(const uint32_t*, int, int, const uint32_t*, const uint32_t*, int64_t, __VA_ARGS__, \
                                    const uint64_t*, uint64_t*);
#define EXT_INSTANTIATE_ALL(K, ...)                                                        \
  EXT_INSTANTIATE(K, EXT_PACKED, EXT_MAX, __VA_ARGS__) EXT_INSTANTIATE(K, EXT_PACKED, EXT_MIN, __VA_ARGS__)     \
  EXT_INSTANTIATE(K, EXT_PACKED, EXT_BOTH, __VA_ARGS__) EXT_INSTANTIATE(K, EXT_WIDE_VAL, EXT_MAX, __VA_ARGS__)  \
  EXT_INSTANTIATE(K, EXT_WIDE_VAL, EXT_MIN, __VA_ARGS__) EXT_INSTANTIATE(K, EXT_WIDE_VAL, EXT_BOTH, __VA_ARGS__) \
  EXT_INSTANTIATE(K, EXT_WIDE_ROW, EXT_MAX, __VA_ARGS__) EXT_INSTANTIATE(K, EXT_WIDE_ROW, EXT_MIN, __VA_ARGS__)  \
  EXT_INSTANTIATE(K, EXT_WIDE_ROW, EXT_BOTH, __VA_ARGS__)
EXT_INSTANTIATE_ALL(ext_few_regions_kernel, uint32_t)
EXT_INSTANTIATE_ALL(ext_lds_regions_kernel, uint32_t, uint32_t)
EXT_INSTANTIATE_ALL(ext_global_regions_kernel, uint32_t)
#undef EXT_INSTANTIATE_ALL
#undef EXT_INSTANTIATE

}  // namespace sdo
