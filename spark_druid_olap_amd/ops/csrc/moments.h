// Shapes of the per-group moment states (moments.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// What one accumulation pass over the records adds up per group.  A group's state is W 64-bit words:
//   MOM_INT2     n, S1 = sum x (int64), 2 digit sums of x^2   (|x| < 2^32: x^2 has two 32-bit digits)
//   MOM_INT4     n, S1,                 4 digit sums of x^2   (any int64)
//   MOM_F64_SUM  n, sum x (f64)                               (pass 1 of a double column)
//   MOM_F64_DEV  sum d, sum d^2 (f64), d = x - mean           (pass 2; no count word)
// A digit sum is a plain u64 sum of 32-bit digits: no add anywhere propagates a carry, and none can
// overflow below 2^32 rows.  The digits are normalised once, in mom_final_kernel.
enum MomMode : int { MOM_INT2 = 0, MOM_INT4 = 1, MOM_F64_SUM = 2, MOM_F64_DEV = 3 };

constexpr int mom_words(int mode) { return mode == MOM_INT2 ? 4 : mode == MOM_INT4 ? 6 : 2; }
constexpr bool mom_counts(int mode) { return mode != MOM_F64_DEV; }  // word 0 is the row count
constexpr bool mom_isf(int mode, int j) { return mode == MOM_F64_DEV || (mode == MOM_F64_SUM && j == 1); }

// LDS a workgroup's states may take (the budget of the quantile and distinct tables: two such
// workgroups fit a CU's 160 KiB)
static constexpr int64_t MOM_LDS_BYTES = 64 * 1024;
static constexpr int MOM_WAVES = 4;  // waves of a 256-thread workgroup

// The three tiers by key space G:
//  * few  (G <= MOM_FEW_G): every wave owns a private LDS row of G states, [MOM_WAVES][G][W] u64
//    (6 KiB at most), and adds to it without atomics: per 64 records it loops over the DISTINCT keys
//    present, reducing each key's lanes across the wave.  One trip costs W - 1 64-bit wave
//    reductions (~25 VALU each), so the bound is where ~G trips stop being cheaper than the
//    conflicts of 64 lanes' LDS atomics on G addresses; 16 is reasoned from instruction counts, not
//    measured.
//  * lds  (G <= MOM_LDS_SLICES x mom_lds_groups(mode)): one table per workgroup, the count as u32
//    and the other words as u64: 28 B (INT2), 44 B (INT4), 12 B (F64_SUM), 16 B (F64_DEV) a state,
//    so 2,340 / 1,489 / 5,461 / 4,096 groups a table; LDS atomic adds, one flush of the nonzero
//    words.  A key space of several tables takes one pass over the records per key slice, each
//    skipping the other slices' records.  At 600 M records and 3,750 groups the two slices take
//    3.4 ms together (profiles/moments_probe.json); the global tier took 112 ms on the same records
//    before the slices existed, so re-reading up to 8 times stays far below it.
//  * global (beyond): global atomics, a wave first merging each run of equal adjacent keys.
static constexpr int MOM_FEW_G = 16;
static constexpr int MOM_LDS_SLICES = 8;
constexpr int64_t mom_lds_groups(int mode) {
  return MOM_LDS_BYTES / (8 * (mom_words(mode) - (mom_counts(mode) ? 1 : 0)) + (mom_counts(mode) ? 4 : 0));
}
enum MomTier : int { MOM_TIER_FEW = 0, MOM_TIER_LDS = 1, MOM_TIER_GLOBAL = 2 };
constexpr int mom_tier(int mode, int64_t G) {
  return G <= MOM_FEW_G ? MOM_TIER_FEW : G <= MOM_LDS_SLICES * mom_lds_groups(mode) ? MOM_TIER_LDS : MOM_TIER_GLOBAL;
}

// records in flight per thread (all loads issued before the first add)
static constexpr int MOM_R = 4;
// records of a producer chunk region (ops/desc.py CHUNK_ROWS): no region end lies beyond it
static constexpr uint32_t MOM_REGION = 4096;

}  // namespace sdo
