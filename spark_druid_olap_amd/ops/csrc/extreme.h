// Shapes of the per-group packed-key extremes (extreme.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// What one accumulation pass over the (u32 group key, u32 row id, ordered u64 values ...) records
// folds into a group's state.  A state word is ONE u64 key per direction, the max word first:
//   EXT_PACKED    ord32(y) << 32 | (row id + 1): the ordering column is stored in at most 32 bits
//                 (ord32 = the low word of the record's value with the sign bit moved) or is the time
//                 of a time-sorted shard (ord32 = 0, no value in the record: voff 0).  One u64
//                 max / min resolves the value and the tie (max_by: the last row, min_by: the first).
//   EXT_WIDE_VAL  the ordered u64 itself (int64 / double columns), pass 1 of 2
//   EXT_WIDE_ROW  row id + 1 of the records whose value equals pass 1's extreme (`ext`), pass 2
// The low word of a PACKED or WIDE_ROW key is row id + 1 >= 1 and below 2^32 (the producer bounds a
// shard's rows), so the identities -- 0 under max, all ones under min -- are never real keys there:
// ext_final_kernel knows an untouched group without a count.
enum ExtMode : int { EXT_PACKED = 0, EXT_WIDE_VAL = 1, EXT_WIDE_ROW = 2 };
// directions of a state: bit 0 max_by, bit 1 min_by; both: 2 words a group
enum ExtDirs : int { EXT_MAX = 1, EXT_MIN = 2, EXT_BOTH = 3 };
constexpr int ext_words(int dirs) { return dirs == EXT_BOTH ? 2 : 1; }

static constexpr int64_t EXT_LDS_BYTES = 64 * 1024;  // (the budget of the moment tables: two workgroups a CU)
static constexpr int EXT_WAVES = 4;                  // waves of a 256-thread workgroup

// The three tiers by key space G (the split of moments.h):
//  * few  (G <= EXT_FEW_G): per 64 records a wave loops over the distinct keys present (a ballot),
//    reduces each key's lanes with DPP max / min and folds the result into its private LDS row
//    [EXT_WAVES][G][D] without atomics; the rows are combined at the end of the workgroup.
//  * lds  (G <= EXT_LDS_SLICES x ext_lds_groups(dirs)): one [GL][D] u64 table per workgroup,
//    64-bit LDS atomic max / min, one flush of the touched words with global atomics; a key space
//    of several tables takes one pass per key slice.  8,192 one-word or 4,096 two-word groups a table.
//  * global (beyond): global 64-bit atomic max / min after a per-wave merge of runs of equal keys.
// Measured at 600 M records (profiles/extreme_by_probe.json), the pass alone: 3 groups, few 2.3 ms
// against 1.9 ms forced to the LDS tier with one-word states and 3.2 against 3.3 ms with two-word
// ones -- the few tier gains nothing there over 64-bit LDS atomics, its bound is kept from
// moments.h and is not tuned; 3,750 groups, one LDS table 1.7 / 2.9 ms against 22.9 / 47.7 ms forced
// to global atomics, so 4 re-reads stay far below the global tier (more slices were not measured).
static constexpr int EXT_FEW_G = 16;
static constexpr int EXT_LDS_SLICES = 4;
constexpr int64_t ext_lds_groups(int dirs) { return EXT_LDS_BYTES / (8 * ext_words(dirs)); }
enum ExtTier : int { EXT_TIER_FEW = 0, EXT_TIER_LDS = 1, EXT_TIER_GLOBAL = 2 };
constexpr int ext_tier(int dirs, int64_t G) {
  return G <= EXT_FEW_G ? EXT_TIER_FEW : G <= EXT_LDS_SLICES * ext_lds_groups(dirs) ? EXT_TIER_LDS : EXT_TIER_GLOBAL;
}

static constexpr int EXT_R = 4;                   // records in flight per thread
static constexpr uint32_t EXT_REGION = 4096;      // records of a producer chunk region (ops/desc.py CHUNK_ROWS)

// One payload gather of ext_final_kernel: the row id of word `word` of the [G][D] `state`, the
// payload column at its stored type, out[g] as int64 (integers) or f64 (doubles; decimals: x / div).
enum ExtType : int { EXT_I8 = 0, EXT_U8 = 1, EXT_I16 = 2, EXT_I32 = 3, EXT_I64 = 4, EXT_F32 = 5, EXT_F64 = 6 };
struct ExtPayload {
  const void* col;
  const uint64_t* state;
  uint64_t* out;
  double div;      // 0: an integer payload, written as int64
  int32_t D;
  int32_t word;
  int32_t type;
  int32_t pad_;
};
static constexpr int EXT_FINAL_MAX = 16;  // payloads of one launch
struct ExtFinalArgs {
  int32_t n;
  int32_t G;
  int64_t rows;  // rows of the payload columns (a decoded row id beyond them writes 0, never reads)
  ExtPayload p[EXT_FINAL_MAX];
};

}  // namespace sdo
