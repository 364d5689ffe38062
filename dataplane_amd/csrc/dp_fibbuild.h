// SPDX-License-Identifier: Apache-2.0
//
// Build lists and launch geometry of the device FIB build (DP_OPT_DEVICE_FIB,
// include/dpgpu.h), shared by the table compiler (dp_tables.cpp: it writes the
// lists), the kernels (dp_fibbuild.hip) and the runtime.  Host-only users
// include this without HIP.
#ifndef DP_FIBBUILD_H
#define DP_FIBBUILD_H

#include <stdint.h>

namespace dpb {

constexpr uint32_t kTpb = 256;              // both kernels' workgroup
constexpr uint32_t kSpl = 4;                // direct kernel: slots (/24s) a lane owns
constexpr uint32_t kTile = kTpb * kSpl;     // slots a workgroup paints (1024: an aligned /14)
constexpr uint32_t kStage = 1024;           // routes of a tile's run staged in LDS; the rest is read from HBM
constexpr uint32_t kSlots = 1u << 24;       // direct-table entries
constexpr uint32_t kTiles = kSlots / kTile;
constexpr uint32_t kBlockLanes = 64;        // block kernel: one wave a block, 4 host addresses a lane
constexpr uint32_t kBlockRoutes = 510;      // routes of length 25..32 one /24 can hold (2 + 4 + ... + 256)
constexpr uint32_t kBlockStage = 512;       // LDS words a wave stages them in
static_assert((kTile & (kTile - 1)) == 0, "a tile is an aligned power of two of slots: a prefix");

// A route of length <= 24, in (key, length) order -- a pre-order of the prefix
// tree.  `parent`: the index of the nearest enclosing short route; the /0
// (index 0) is its own.
struct Short {
  uint32_t slot;    // first /24 slot the route covers (its key >> 8)
  uint32_t len;     // 0..24
  uint32_t nh;      // < 0xffff
  uint32_t parent;
};
static_assert(sizeof(Short) == 16, "one 16-byte load a record");

// A route of length 25..32 packed in a word, in the same order: first host
// address (key & 0xff) | length << 8 | next hop << 16.
typedef uint32_t Long;

// One block: a /24 that holds long routes.  Blocks ascend with their slots;
// a block's index is its position in the list.
struct Block {
  uint32_t slot, first, count, pad;  // Long[first, first + count)
};
static_assert(sizeof(Block) == 16, "one 16-byte load a record");

// Device addresses of one FIB's lists and regions (a kernel argument).
struct Job {
  const Short *shorts;
  const Long *longs;
  const Block *blocks;
  uint32_t *direct;   // uint32_t[kSlots] inside the image
  uint16_t *block16;  // uint16_t[256 * n_blocks] inside the image
  uint32_t n_short, n_blocks;
};

#ifdef __HIPCC__
#define DPB_HD __host__ __device__
#else
#define DPB_HD
#endif
// does the short route (slot0, len) hold slot s?  (slots are < 2^24, so a /0 holds all)
DPB_HD inline bool covers(uint32_t slot0, uint32_t len, uint32_t s) { return ((slot0 ^ s) >> (24 - len)) == 0; }

}  // namespace dpb

#endif
