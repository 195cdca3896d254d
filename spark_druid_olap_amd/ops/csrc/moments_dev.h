// Device helpers the per-group moment kernels share (moments.hip, comoments.hip): the record value
// decode, the add / atomic add of a state word that is either a u64 or the bits of a double, and
// the once-rounded conversion of a 192-bit magnitude.
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
