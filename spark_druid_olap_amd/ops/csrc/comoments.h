// Shapes of the per-group co-moment states of a column pair (comoments.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// What one accumulation pass over the records adds up per group for the pair (x, y).  A state is W
// 64-bit words; SQ says whether the squares a correlation needs are kept beside the cross term:
//   CO_INT2     n, Sx, Sy (int64 sums), D = 2 digit sums of x y [, D of x^2, D of y^2]   W = 5 [9]
//               (both columns stored in at most 32 bits: the int64 product has two 32-bit digits)
//   CO_INT4     n, Sx, Sy,              D = 4 digit sums of x y [, D of x^2, D of y^2]   W = 7 [15]
//   CO_F64_SUM  n, sum x, sum y (f64)                                                    W = 3
//   CO_F64_DEV  sum dx, sum dy, sum dx dy [, sum dx^2, sum dy^2] (f64; no count word)    W = 3 [5]
// x^2 and y^2 are split as moments.h does: digits of the magnitude, unsigned u64 sums.  x y is the
// two's-complement product: its lower digits are unsigned u64 sums, its TOP digit is sign-extended
// and adds into an int64 sum, so the value is sum_k d_k 2^(32 k) with d_(D-1) signed.  No add
// propagates a carry and none can overflow below 2^32 rows (|top digit| <= 2^31); the digits are
// normalised once, in co_final_kernel.
enum CoMode : int { CO_INT2 = 0, CO_INT4 = 1, CO_F64_SUM = 2, CO_F64_DEV = 3 };

constexpr int co_digits(int mode) { return mode == CO_INT2 ? 2 : 4; }
constexpr int co_words(int mode, bool sq) {
  return mode == CO_F64_SUM ? 3 : mode == CO_F64_DEV ? (sq ? 5 : 3) : 3 + co_digits(mode) * (sq ? 3 : 1);
}
constexpr bool co_counts(int mode) { return mode != CO_F64_DEV; }  // word 0 is the row count
constexpr bool co_isf(int mode, int j) { return mode == CO_F64_DEV || (mode == CO_F64_SUM && j > 0); }
// the state's words without the count, and the power of two the few tier pads them to
constexpr int co_values(int mode, bool sq) { return co_words(mode, sq) - (co_counts(mode) ? 1 : 0); }
constexpr int co_pow2(int v) { return v <= 2 ? 2 : v <= 4 ? 4 : v <= 8 ? 8 : 16; }

static constexpr int64_t CO_LDS_BYTES = 64 * 1024;  // (the budget of moments.h: two workgroups a CU)
static constexpr int CO_WAVES = 4;                  // waves of a 256-thread workgroup

// The three tiers by key space G.  The states are up to 2.5 times as wide as moments.h's, which
// moves every bound:
//  * few (G <= CO_FEW_G): every wave owns a private LDS row of G states ([CO_WAVES][G][W] u64, 7.5
//    KiB at most) and adds to it without atomics, one trip per DISTINCT key among its 64 records.
//    A trip that reduced word by word (moments.hip: 6 DPP steps of ~4 VALU a word) would cost
//    14 x 25 = 350 VALU at W = 15.  Here a trip is ONE reduce-scatter over the padded words: at step
//    s every lane hands half of the words it still holds to lane ^ 2^s and keeps the other half, so
//    P words take P - 1 exchange-adds down to one word a lane and 6 - log2 P more to the wave total
//    -- 17 exchanges of ~8 VALU (two selects, the move, the add, per 32-bit half) = ~130 VALU at
//    P = 16, what a MOM_INT4 trip costs.  The bound therefore stays where moments.h reasoned it
//    (16: ~G trips against the conflicts of 64 lanes' LDS atomics on G addresses).  REASONED from
//    instruction counts; MEASURED only at G = 3 and the 9-word state (600 M records,
//    profiles/comoments_probe.json): 3.3 ms, against 11.9 ms for the same pass forced to the lds
//    tier (2.5 against 6.3 ms for the 5-word state).  The 15-word state is not timed: the flat
//    schema's metrics are all stored in 32 bits.
//  * lds (G <= CO_LDS_SLICES x co_lds_groups): one table per workgroup, the count as u32 and the
//    other words as u64 -- 36 / 68 B (INT2 without / with squares), 52 / 116 B (INT4), 20 B
//    (F64_SUM), 24 / 40 B (F64_DEV) a state, so 1,820 / 963, 1,260 / 564, 3,276, 2,730 / 1,638
//    groups a table.  A key space of several tables takes one pass over the records per key slice.
//    MEASURED at 600 M five-word records and 3,750 groups (profiles/comoments_probe.json): the
//    9-word state takes 12.1 ms in 4 slices against 197.5 ms forced to the global tier, the 5-word
//    state 7.6 ms in 3 slices against 112.0 ms -- a slice pass costs 2.5 - 3 ms, the global tier
//    about 65 of them.  16 slices (about 48 ms) is REASONED from that ratio to stay well below the
//    global tier while a correlation of wide integers still reaches 9,024 groups; more than 4
//    slices are not timed.
//    In this tier and the next a zero word costs no atomic.  That saves the high digits of squares
//    and of small NON-NEGATIVE products only: a small negative product is all ones above its low
//    digits (0xffffffff and a top digit of -1), so a negative pair pays every product atomic, 4 in
//    CO_INT4.  Not measured: the flat schema's metrics are all positive.
//  * global (beyond): global atomics after a per-wave merge of runs of equal adjacent keys; the
//    merge stops at the wave's longest run.
static constexpr int CO_FEW_G = 16;
static constexpr int CO_LDS_SLICES = 16;
constexpr int64_t co_state_bytes(int mode, bool sq) {
  return 8 * co_values(mode, sq) + (co_counts(mode) ? 4 : 0);
}
constexpr int64_t co_lds_groups(int mode, bool sq) { return CO_LDS_BYTES / co_state_bytes(mode, sq); }
enum CoTier : int { CO_TIER_FEW = 0, CO_TIER_LDS = 1, CO_TIER_GLOBAL = 2 };
constexpr int co_tier(int mode, bool sq, int64_t G) {
  return G <= CO_FEW_G ? CO_TIER_FEW : G <= CO_LDS_SLICES * co_lds_groups(mode, sq) ? CO_TIER_LDS : CO_TIER_GLOBAL;
}

// records in flight per thread: two values a record, so half of moments.h's four for the same
// registers (a 15-word contribution is live per record)
static constexpr int CO_R = 2;

// which finalise: a covariance (A / (n (n - ddof)) / div) or a correlation (A / sqrt(Vx Vy))
enum CoKind : int { CO_COVAR = 0, CO_CORR = 1 };

}  // namespace sdo
