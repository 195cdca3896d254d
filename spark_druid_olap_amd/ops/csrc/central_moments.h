// Shapes of the per-group power-sum states behind skewness / kurtosis (central_moments.hip), shared
// with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// What one accumulation pass over the records adds up per group.  A state is W 64-bit words:
//   CM_INT3      n, S1, 2 digit sums of y^2, 3 of y^3                     W = 7   (skewness)
//   CM_INT4      n, S1, 2 of y^2, 3 of y^3, 4 of y^4                      W = 11  (kurtosis asked)
//   CM_F64_SUM   n, sum x (f64)                                           W = 2   (pass 1 of the f64 path)
//   CM_F64_DEV3  sum d, sum d^2, sum d^3 (f64), d = x - mean; no count    W = 3   (pass 2)
//   CM_F64_DEV4  ... and sum d^4                                          W = 4
// The integer modes take y = o - pivot, o the record's ordered u64 and `pivot` the ordered u64 of
// the column's minimum: they apply when max - min < 2^32, so y is a u32 whatever the column's
// stored width, y^2 < 2^64 has two 32-bit digits, y^3 < 2^96 three and y^4 < 2^128 four.  S1 and
// every digit sum are plain u64 sums of values below 2^32: no add propagates a carry and none can
// overflow below 2^32 rows.  The digits are normalised once, in cm_final_kernel.  The f64 path
// (double columns, and integer columns of range >= 2^32, converted on entry) is not exact.
enum CmMode : int { CM_INT3 = 0, CM_INT4 = 1, CM_F64_SUM = 2, CM_F64_DEV3 = 3, CM_F64_DEV4 = 4 };

constexpr int cm_words(int mode) {
  return mode == CM_INT3 ? 7 : mode == CM_INT4 ? 11 : mode == CM_F64_SUM ? 2 : mode == CM_F64_DEV3 ? 3 : 4;
}
constexpr bool cm_counts(int mode) { return mode <= CM_F64_SUM; }  // word 0 is the row count
constexpr bool cm_isf(int mode, int j) { return mode > CM_F64_SUM || (mode == CM_F64_SUM && j > 0); }
// the state's words without the count, and the power of two the few tier pads them to
constexpr int cm_values(int mode) { return cm_words(mode) - (cm_counts(mode) ? 1 : 0); }
constexpr int cm_pow2(int v) { return v <= 2 ? 2 : v <= 4 ? 4 : v <= 8 ? 8 : 16; }

// The finalise forms, exactly, in CM_LIMBS 64-bit limbs (two's complement):
//   N2 = n S2 - S1^2                                      < 2^128
//   N3 = n^2 S3 - 3 n S1 S2 + 2 S1^3                      terms < 2^192, 2^194, 2^193
//   N4 = n^3 S4 - 4 n^2 S1 S3 + 6 n S1^2 S2 - 3 S1^4      terms < 2^256, 2^258, 2^259, 2^258
// for n < 2^32 and y < 2^32 (S1 < 2^64, S2 < 2^96, S3 < 2^128, S4 < 2^160).  Every partial sum stays
// below 2^261 in magnitude, so 320 bits hold each with its sign and no intermediate wraps.
static constexpr int CM_LIMBS = 5;

static constexpr int64_t CM_LDS_BYTES = 64 * 1024;  // (the budget of moments.h: two workgroups a CU)
static constexpr int CM_WAVES = 4;                  // waves of a 256-thread workgroup

// The three tiers by key space G, the shape of moments.h / comoments.h with the bounds restated for
// states of 7 and 11 words.  Every bound below is REASONED from those files' measurements, not tuned
// for this state.  MEASURED only at two points (600 M records, tools/central_moments_probe.py,
// profiles/central_moments_probe.json): 3 groups -- few 2.6 / 4.2 ms (7 / 11 words), forced lds
// 6.3-15.0 ms, forced global 4-8.6 s; 3,750 groups -- lds 5.9-6.5 ms in 3 slices / 12.2-13.3 ms in
// 5, forced global 111-269 ms.  A slice pass costs 2.0-2.7 ms, so 16 slices stay below the global
// tier there; the bounds between and beyond those points are not timed.
//  * few (G <= CM_FEW_G): every wave owns a private LDS row of G states ([CM_WAVES][G][W] u64,
//    5.5 KiB at most) and adds to it without atomics, one trip per DISTINCT key among its 64
//    records: ONE reduce-scatter of the padded words (8 for CM_INT3, 16 for CM_INT4: 10 / 17
//    exchange-adds, what comoments.hip pays for its 9- and 15-word states), then P lanes each add
//    one word.  16 is where comoments.h reasoned ~G trips stop being cheaper than 64 lanes' LDS
//    atomics on G addresses; the states here are no wider than its widest.
//  * lds (G <= CM_LDS_SLICES x cm_lds_groups): one table per workgroup, the count as u32 and the
//    other words as u64 -- 52 B (INT3), 84 B (INT4), 12 B (F64_SUM), 24 / 32 B (F64_DEV3 / 4) a
//    state, so 1,260 / 780 / 5,461 / 2,730 / 2,048 groups a table.  LDS atomic adds, one flush of
//    the nonzero words.  A key space of several tables takes one pass over the records per key
//    slice, each skipping the other slices' records before their products are formed.  16 slices
//    as comoments.h: it measured a slice pass of a 9-word state at about 1/65 of the global tier.
//  * global (beyond): u64 / f64 global atomics after a per-wave merge of runs of equal adjacent
//    keys; the merge stops at the wave's longest run.
// A zero word costs no atomic in the lds and global tiers: the high digits of small y.
static constexpr int CM_FEW_G = 16;
static constexpr int CM_LDS_SLICES = 16;
constexpr int64_t cm_state_bytes(int mode) { return 8 * cm_values(mode) + (cm_counts(mode) ? 4 : 0); }
constexpr int64_t cm_lds_groups(int mode) { return CM_LDS_BYTES / cm_state_bytes(mode); }
enum CmTier : int { CM_TIER_FEW = 0, CM_TIER_LDS = 1, CM_TIER_GLOBAL = 2 };
constexpr int cm_tier(int mode, int64_t G) {
  return G <= CM_FEW_G ? CM_TIER_FEW : G <= CM_LDS_SLICES * cm_lds_groups(mode) ? CM_TIER_LDS : CM_TIER_GLOBAL;
}

// records in flight per thread (one value a record; all loads issued before the first add)
static constexpr int CM_R = 4;

}  // namespace sdo
