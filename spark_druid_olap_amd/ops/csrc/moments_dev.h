// Device helpers the per-group moment kernels share (moments.hip, comoments.hip,
// central_moments.hip): the record value decode, the add / atomic add of a state word that is
// either a u64 or the bits of a double, the cross-lane reduce-scatter of a state, and the
// once-rounded conversion of a 192-bit magnitude.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moments.h"

namespace sdo {

static constexpr uint64_t MSIGN = 0x8000000000000000ull;

__device__ __forceinline__ uint64_t mom_add(bool f, uint64_t a, uint64_t b) {
  return f ? (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b))
           : a + b;
}

// (no return value used: an LDS / global atomic add instruction, f64 ones included -- checked in the ISA)
__device__ __forceinline__ void mom_atomic(bool f, uint64_t* p, uint64_t v) {
  if (f) atomicAdd((double*)p, __longlong_as_double((long long)v));
  else atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

__device__ __forceinline__ double mom_f64(uint64_t o) {  // inverse of f2ord under the flipped sign bit
  const int64_t b = (int64_t)(o ^ MSIGN);
  return __longlong_as_double(b >= 0 ? b : (b ^ 0x7fffffffffffffffLL));
}

__device__ __forceinline__ uint32_t mom_region_end(uint32_t lo, uint32_t end) {
  return end < lo + MOM_REGION ? end : lo + MOM_REGION;
}

// the 32-bit value of lane ^ 2^S: quad permutes (DPP) inside a quad, ds_swizzle's xor mask inside
// 32 lanes, a bpermute across the halves.  All 64 lanes must be live.
template <int S>
__device__ __forceinline__ uint32_t co_xchg32(uint32_t v) {
  if constexpr (S == 0) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // [1,0,3,2]
  else if constexpr (S == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // [2,3,0,1]
  else if constexpr (S < 5) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, ((1 << S) << 10) | 0x1f);
  else return (uint32_t)__shfl_xor((int)v, 32, 64);
}

template <int S>
__device__ __forceinline__ uint64_t co_xchg(uint64_t v) {
  return (uint64_t)co_xchg32<S>((uint32_t)v) | ((uint64_t)co_xchg32<S>((uint32_t)(v >> 32)) << 32);
}

// Sums the P words a[] of every lane over the wave.  Step S (H = P / 2^(S+1) words kept): a lane
// whose bit S is clear keeps a[0..H) and hands a[H..2H) to lane ^ 2^S, which does the opposite; once
// one word a lane is left the remaining steps add it across.  Lane l < P ends with the wave's total
// of word co_word_of<P>(l) in a[0].
template <bool F, int H, int S, int P>
__device__ __forceinline__ void co_reduce_scatter(uint64_t (&a)[P], int lane) {
  if constexpr (H >= 1) {
    const bool up = (lane >> S) & 1;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const uint64_t send = up ? a[j] : a[j + H];
      const uint64_t keep = up ? a[j + H] : a[j];
      a[j] = mom_add(F, keep, co_xchg<S>(send));
    }
    co_reduce_scatter<F, H / 2, S + 1, P>(a, lane);
  } else if constexpr (S < 6) {
    a[0] = mom_add(F, a[0], co_xchg<S>(a[0]));
    co_reduce_scatter<F, 0, S + 1, P>(a, lane);
  }
}

template <int P>
__device__ __forceinline__ int co_word_of(int lane) {  // (the low log2 P bits of the lane, reversed)
  int idx = 0;
#pragma unroll
  for (int s = 0; (P >> (s + 1)) >= 1; ++s) idx += ((lane >> s) & 1) * (P >> (s + 1));
  return idx;
}

// the 192-bit value (l2, l1, l0) as a double, rounded once: the leading 64 bits with everything
// below them folded into the lowest bit (so the conversion's round-to-nearest sees a sticky bit)
__device__ __forceinline__ double mom_limbs_f64(uint64_t l2, uint64_t l1, uint64_t l0) {
  int e = 128;
  if (!l2) {
    l2 = l1, l1 = l0, l0 = 0ull, e = 64;
    if (!l2) l2 = l1, l1 = 0ull, e = 0;
  }
  if (!l2) return 0.0;
  const int z = __clzll((long long)l2);
  const uint64_t top = z ? (l2 << z) | (l1 >> (64 - z)) : l2;
  const uint64_t rest = (z ? l1 << z : l1) | l0;
  return ldexp((double)(top | (rest ? 1ull : 0ull)), e - z);
}

}  // namespace sdo
