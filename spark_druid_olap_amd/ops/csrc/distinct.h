// Shapes of the exact COUNT(DISTINCT) id bitsets (distinct.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

// u32 words a workgroup's private [G][Wg] bit matrix may take in LDS (64 KiB: the budget the
// quantile and theta histograms use; two such workgroups fit a CU's 160 KiB)
static constexpr int64_t DCOUNT_LDS_WORDS = 64 * 1024 / 4;
// rows of up to this many words are counted by one wave each (a lane reads at most 2 words),
// longer rows by one workgroup each
static constexpr int DCOUNT_WAVE_ROW_WORDS = 128;
// records in flight per thread (all loads issued before the first atomic)
static constexpr int DCOUNT_R = 4;
// records of a producer chunk region (ops/desc.py CHUNK_ROWS): no region end lies beyond it
static constexpr uint32_t DCOUNT_REGION = 4096;

}  // namespace sdo
