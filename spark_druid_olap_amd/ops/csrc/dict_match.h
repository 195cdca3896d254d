// Pattern program of the dictionary text matcher (dict_match.hip), shared with the launcher and
// packed on the host by engine/dict_match.py (a numpy structured dtype of the same layout).
#pragma once
#include <stdint.h>

namespace sdo {

constexpr int DM_MAX_SEGS = 8;         // '%'-separated LIKE pieces, or AND-ed needles
constexpr int DM_MAX_SEG_LEN = 256;    // pattern positions a segment (literal bytes + '_' positions)
constexpr int DM_TILE_BYTES = 48 * 1024;  // LDS text tile of one workgroup (dict_match.hip: why 48 KiB)
constexpr int DM_BLOCK = 256;          // lanes == dictionary entries a workgroup

constexpr int DM_ANCHOR_START = 1;  // segment 0 matches at the entry's first byte
constexpr int DM_ANCHOR_END = 2;    // the last segment ends at the entry's last byte
constexpr int DM_FOLD = 4;          // entry bytes 'A'..'Z' compare as 'a'..'z' (the literals are lowered)
constexpr int DM_ALL = 8;           // segments are independent needles that must all occur

// 2,328 bytes: passed by value (kernel argument segment) and copied to LDS once a workgroup.
struct DmProgram {
  int32_t nseg;
  int32_t flags;
  uint16_t len[DM_MAX_SEGS];                  // positions per segment
  uint8_t lit[DM_MAX_SEGS][DM_MAX_SEG_LEN];   // literal byte of a position (unused where `any` is set)
  uint32_t any[DM_MAX_SEGS][DM_MAX_SEG_LEN / 32];  // bit j: position j is "any one code point" ('_')
};

}  // namespace sdo
