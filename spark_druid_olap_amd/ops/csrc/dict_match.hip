// LIKE / contains / fragment over a string dictionary's text, for CDNA4 (gfx950).
//
// Every string predicate is answered in the dictionary domain: one verdict per dictionary entry,
// packed into the id bitset the scan reads.  This kernel produces those verdicts from the
// dictionary's device text heap (segment/textheap.py): the UTF-8 bytes of all entries back to back
// and n + 1 u32 byte offsets.
//
// Work split.  A workgroup of 256 lanes owns 256 consecutive entries.  The heap is contiguous in id
// order, so their bytes are ONE span [off[e0], off[e0 + 256]): the workgroup stages it into LDS with
// 16-byte loads, 256 lanes wide (the first load aligned down to 16, the last rounded up; the bytes
// before and after the span are never read back, a lane only touches [off[e], off[e + 1])), and then
// every lane matches its own entry out of LDS, where divergent byte reads cost a bank conflict at
// worst -- in global memory each of them would be its own 64-byte request.  A span longer than the
// tile (one oversized comment among short names) runs the same matcher, templated on the byte
// source, straight on global memory: correct, not fast.
//
// LDS tile: 48 KiB.  With the 2.3 KiB pattern program a workgroup holds 50.3 KiB, so three fit the
// 160 KiB of a CU (12 waves): while one stages its span the other two match, which is what hides the
// staging loads -- a 64 KiB tile would leave two workgroups with nothing to overlap a barrier wait,
// and 32 KiB sends dictionaries with a mean entry above 128 bytes (user agents) to the global path.
// 48 KiB keeps entries of up to 192 bytes on average in LDS.
//
// Matching.  The program (dict_match.h) is up to 8 segments of literal bytes and "any one code
// point" positions.  LIKE: the pieces between '%'.  An anchored first piece is compared in place at
// the entry's start, every middle piece is found by leftmost search from the end of the previous
// match, an anchored last piece is compared backwards from the entry's end and must start at or
// after that point.  Pieces have a fixed length in code points, so the leftmost match of each also
// ends leftmost and the greedy rule is exact.  '_' consumes a lead byte plus its 10xxxxxx
// continuation bytes and never starts on a continuation byte, so matches stay on code point
// boundaries and LIKE / case-sensitive contains are exact over any valid UTF-8.  DM_ALL: the
// segments are independent needles, each searched from the entry's start.
//
// Case folding is ASCII only.  Lowering can turn a non-ASCII character into ASCII (U+0130, the
// Kelvin sign), so under DM_FOLD the kernel also writes the bitset of entries holding any byte
// >= 0x80 and the host re-evaluates exactly those; an all-ASCII entry's verdict stands.
//
// Output: one u64 a wave from a ballot (entry e is bit e % 64 of word e / 64), a plain vector
// store by the wave's first lane; lanes past n vote 0, so the last word's tail is zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dict_match.h"

namespace sdo {

static constexpr uint32_t DM_NONE = 0xffffffffu;

struct DmLdsBytes {   // the staged span; index = byte offset in the tile
  const uint8_t* b;
  __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return b[i]; }
};
struct DmGlobalBytes {  // the heap itself; index = byte offset in the heap
  const uint8_t* __restrict__ b;
  __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return b[i]; }
};

template <bool FOLD>
__device__ __forceinline__ uint32_t dm_fold(uint32_t c) {
  if (FOLD && c - (uint32_t)'A' < 26u) c |= 0x20u;
  return c;
}

__device__ __forceinline__ bool dm_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }

__device__ __forceinline__ bool dm_any(const DmProgram* P, int s, uint32_t j) {
  return (P->any[s][j >> 5] >> (j & 31u)) & 1u;
}

// Segment s compared forwards from byte p of a text ending at `end`: the byte after the match, or
// DM_NONE.
template <bool FOLD, typename Src>
__device__ __forceinline__ uint32_t dm_fwd(const DmProgram* P, int s, Src t, uint32_t p, uint32_t end) {
  const uint32_t m = P->len[s];
  uint32_t q = p;
  for (uint32_t j = 0; j < m; ++j) {
    if (q >= end) return DM_NONE;
    const uint32_t c = t[q];
    if (dm_any(P, s, j)) {
      if (dm_cont(c)) return DM_NONE;
      ++q;
      while (q < end && dm_cont(t[q])) ++q;
    } else {
      if (dm_fold<FOLD>(c) != P->lit[s][j]) return DM_NONE;
      ++q;
    }
  }
  return q;
}

// Segment s compared backwards from `end`, not reaching below `lo`: the match's first byte, or
// DM_NONE.
template <bool FOLD, typename Src>
__device__ __forceinline__ uint32_t dm_bwd(const DmProgram* P, int s, Src t, uint32_t lo, uint32_t end) {
  uint32_t q = end;
  for (uint32_t j = P->len[s]; j-- > 0;) {
    if (q <= lo) return DM_NONE;
    --q;
    if (dm_any(P, s, j)) {
      while (dm_cont(t[q])) {
        if (q <= lo) return DM_NONE;
        --q;
      }
    } else if (dm_fold<FOLD>(t[q]) != P->lit[s][j]) {
      return DM_NONE;
    }
  }
  return q;
}

// Leftmost match of segment s starting in [pos, end]: the byte after it, or DM_NONE.  (Every
// position takes at least one byte, so starts past end - len cannot match.)
template <bool FOLD, typename Src>
__device__ __forceinline__ uint32_t dm_find(const DmProgram* P, int s, Src t, uint32_t pos, uint32_t end) {
  const uint32_t m = P->len[s];
  for (uint32_t p = pos; p + m <= end; ++p) {
    const uint32_t q = dm_fwd<FOLD>(P, s, t, p, end);
    if (q != DM_NONE) return q;
  }
  return DM_NONE;
}

template <bool FOLD, typename Src>
__device__ bool dm_match(const DmProgram* P, Src t, uint32_t b, uint32_t end) {
  const int ns = P->nseg;
  const int flags = P->flags;
  if (flags & DM_ALL) {
    for (int s = 0; s < ns; ++s)
      if (dm_find<FOLD>(P, s, t, b, end) == DM_NONE) return false;
    return true;
  }
  uint32_t pos = b;
  int s = 0;
  if (flags & DM_ANCHOR_START) {
    pos = dm_fwd<FOLD>(P, 0, t, b, end);
    if (pos == DM_NONE) return false;
    if (ns == 1 && (flags & DM_ANCHOR_END)) return pos == end;  // no '%' at all: a full match
    s = 1;
  }
  const int last = (flags & DM_ANCHOR_END) ? ns - 1 : ns;
  for (; s < last; ++s) {
    pos = dm_find<FOLD>(P, s, t, pos, end);
    if (pos == DM_NONE) return false;
  }
  if (flags & DM_ANCHOR_END) return dm_bwd<FOLD>(P, ns - 1, t, pos, end) != DM_NONE;
  return true;
}

template <typename Src>
__device__ __forceinline__ bool dm_nonascii(Src t, uint32_t b, uint32_t end) {
  uint32_t acc = 0;
  for (uint32_t q = b; q < end; ++q) acc |= t[q];
  return (acc & 0x80u) != 0;
}

// heap: 16-byte aligned, readable up to the next multiple of 16 past off[n].  out / nonascii:
// ceil(n / 64) words (nonascii only under FOLD).
template <bool FOLD>
__global__ void __launch_bounds__(DM_BLOCK) dict_match_kernel(const uint8_t* __restrict__ heap,
                                                              const uint32_t* __restrict__ off, uint32_t n,
                                                              DmProgram prog, uint64_t* __restrict__ out,
                                                              uint64_t* __restrict__ nonascii) {
  __shared__ uint4 tile[DM_TILE_BYTES / 16];
  __shared__ DmProgram P;
  const uint32_t lane = threadIdx.x;
  const uint32_t e0 = blockIdx.x * (uint32_t)DM_BLOCK;  // (< n: the grid is ceil(n / 256))
  const uint32_t e1 = min(e0 + (uint32_t)DM_BLOCK, n);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&prog);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&P);
    for (uint32_t i = lane; i < sizeof(DmProgram) / 4; i += DM_BLOCK) dst[i] = src[i];
  }
  const uint32_t lo = off[e0], hi = off[e1];
  const uint32_t a0 = lo & ~15u;
  const bool in_lds = hi - a0 <= (uint32_t)DM_TILE_BYTES;  // (uniform: one branch a workgroup)
  const uint32_t e = e0 + lane;
  const bool valid = e < e1;
  uint32_t b = 0, end = 0;
  if (valid) {
    b = off[e];
    end = off[e + 1];
  }
  bool hit = false, wide = false;
  if (in_lds) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(heap + a0);
    const uint32_t nvec = (hi - a0 + 15u) >> 4;
    for (uint32_t i = lane; i < nvec; i += DM_BLOCK) tile[i] = src[i];
    __syncthreads();
    if (valid) {
      const DmLdsBytes t{reinterpret_cast<const uint8_t*>(tile)};
      hit = dm_match<FOLD>(&P, t, b - a0, end - a0);
      if (FOLD) wide = dm_nonascii(t, b - a0, end - a0);
    }
  } else {
    __syncthreads();  // (the program copy)
    if (valid) {
      const DmGlobalBytes t{heap};
      hit = dm_match<FOLD>(&P, t, b, end);
      if (FOLD) wide = dm_nonascii(t, b, end);
    }
  }
  const uint64_t hits = __ballot(hit);
  const uint64_t wides = FOLD ? __ballot(wide) : 0ull;
  if ((lane & 63u) == 0 && e < n) {  // (a wave wholly past n has no word)
    out[e >> 6] = hits;
    if (FOLD) nonascii[e >> 6] = wides;
  }
}

template __global__ void dict_match_kernel<false>(const uint8_t*, const uint32_t*, uint32_t, DmProgram, uint64_t*,
                                                  uint64_t*);
template __global__ void dict_match_kernel<true>(const uint8_t*, const uint32_t*, uint32_t, DmProgram, uint64_t*,
                                                 uint64_t*);

}  // namespace sdo
