// Shapes of the per-group fixed-bucket histograms (histogram.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// A histogram of B buckets is T = B + 1 ascending thresholds in the records' ordered-u64 domain and
// S = B + 2 counters a group: [below, c_0 .. c_{B-1}, above].  A record's counter is its slot
//   #{i : thr[i] <= o}   in [0, T] = [0, S - 1]
// (an upper-bound count; equal thresholds simply leave a bucket empty).  Ordered values below
// `nan_lo` -- the NaNs with the sign bit set, which f2ord orders below -inf -- take slot S - 1 like the
// other NaNs, which already order above +inf.
static constexpr int FBH_MAX_BUCKETS = 1022;  // S <= 1,024: the thresholds take at most 8 KiB of LDS
constexpr bool fbh_buckets_ok(int64_t B) { return B >= 1 && B <= FBH_MAX_BUCKETS; }

// The search.  The thresholds are staged into LDS once per workgroup and the slot is found with a
// branchless upper-bound binary search: `pos` counts the thresholds known to be <= o, every level
// tries pos + step against thr[pos + step - 1] (a probe beyond T is a miss, the index is clamped, so
// no padding value is needed -- all ones is a real ordered value).  fbh_levels(T) =
// ceil(log2(T + 1)) levels reach every one of the T + 1 outcomes: 3 for B = 5, 10 for B = 1022.
// The two top levels (three thresholds, the same for every record) are kept in registers, so a record
// costs levels - 2 dependent LDS reads; the FBH_R records a thread holds are searched level by level
// together, which keeps FBH_R independent reads in flight.  An arithmetic first guess for uniform
// buckets was NOT built: it needs a 64-bit multiply-high per record and still one or two corrections
// against the table, against 1-8 LDS reads here; nothing measured says it would win.
constexpr int fbh_levels(int T) {
  int k = 0;
  while ((1 << k) <= T) ++k;
  return k;  // 2^(k-1) <= T < 2^k
}

static constexpr int64_t FBH_LDS_COUNTERS = 16 * 1024;  // u32 counters of a workgroup: 64 KiB next to the thresholds
static constexpr int FBH_R = 4;                        // records in flight per thread
static constexpr uint32_t FBH_REGION = 4096;           // records of a producer chunk region (ops/desc.py CHUNK_ROWS)

// The three tiers by the counter space C = G S.  Counters are u32 in LDS -- a shard's records are
// bound below 2^32 by the producer, so none can wrap -- and u64 in the output.
//  * rep (C <= FBH_REP_COUNTERS): R lane-interleaved copies of the whole table,
//    cnt[c * R + (lane & (R - 1))], R the largest power of two <= 64 with C R <= FBH_LDS_COUNTERS.
//    The 64 lanes of a wave that hit one hot counter (600 M rows into 3 x 22 counters is the common
//    case) land on R different addresses in R different banks instead of serialising on one.  LDS
//    atomic adds without return; the flush sums the copies and adds the nonzero counters to the output.
//  * lds (G <= FBH_LDS_SLICES tables of fbh_lds_groups(S) whole groups): one copy of a key slice's
//    table, one pass over the records per slice, each skipping the other slices' records (the split
//    of moments.h).
//  * global (beyond, C * 8 <= FBH_GLOBAL_BYTES): u64 global atomics; a wave first merges every run of
//    equal adjacent (group, slot), whose last lane adds the run's length.
// The bounds 8,192 counters, R and 8 slices were reasoned, not tuned; the launcher takes a forced tier
// so that a probe can judge them.  What profiles/histogram_probe.json measured at 600 M records, the
// pass alone: 3 groups x 22 counters, rep (R = 64) 1.26 ms against 1.28 ms forced to one plain LDS
// table and 790 ms forced to global atomics -- the copies gain almost nothing over plain LDS atomics
// there, so R is harmless but unproven; 3,750 groups x 22 counters, 6 slices 13.6 ms against 27.0 ms
// global; 3,750 x 52, 12 slices (forced) 31.1 ms against 26.1 ms global.  A slice costs ~2.3-2.6 ms
// and the global tier ~26 ms, so the crossover lies near 10 slices and 8 is on the right side of it.
// Not measured: the 8,192-counter bound between rep and lds, R between 2 and 32.
static constexpr int64_t FBH_REP_COUNTERS = 8192;
static constexpr int FBH_LDS_SLICES = 8;
static constexpr int64_t FBH_GLOBAL_BYTES = 512ll << 20;
constexpr int fbh_rep(int64_t C) {
  int r = 64;
  while (r > 1 && C * r > FBH_LDS_COUNTERS) r >>= 1;
  return r;
}
constexpr int64_t fbh_lds_groups(int S) { return FBH_LDS_COUNTERS / S; }
enum FbhTier : int { FBH_TIER_REP = 0, FBH_TIER_LDS = 1, FBH_TIER_GLOBAL = 2 };
constexpr int fbh_tier(int64_t G, int S) {
  return G * S <= FBH_REP_COUNTERS ? FBH_TIER_REP
         : G <= FBH_LDS_SLICES * fbh_lds_groups(S) ? FBH_TIER_LDS
                                                   : FBH_TIER_GLOBAL;
}
// whether `tier` can hold the key space at all (a forced tier)
constexpr bool fbh_tier_holds(int tier, int64_t G, int S) {
  return tier == FBH_TIER_REP ? G * S <= FBH_LDS_COUNTERS
         : tier == FBH_TIER_LDS ? G <= 64 * fbh_lds_groups(S)
                                : tier == FBH_TIER_GLOBAL;
}

}  // namespace sdo
