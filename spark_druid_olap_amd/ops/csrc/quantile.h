// Device state of one per-group radix rank select (quantile.hip), shared with the launchers.
#pragma once
#include <stdint.h>

namespace sdo {

struct QselState {
  int G;             // groups
  int T;             // rank targets per group (2 per interpolated fraction, else 1)
  int B;             // digit bits per level
  int interpolate;
  uint32_t* cnt;     // [G] selected rows
  uint64_t* mn;      // [G] smallest / largest ordered value
  uint64_t* mx;
  uint32_t* width;   // [G] bit length of mx - mn
  uint64_t* prefix;  // [G x T] resolved high bits of (value - mn)
  uint64_t* rank;    // [G x T] remaining rank among the rows sharing the prefix
  uint32_t* hist;    // [G x T][2^B] this level's bins (level 0: rows [G])
  const double* frac;  // [T / (interpolate ? 2 : 1)]
};

}  // namespace sdo
