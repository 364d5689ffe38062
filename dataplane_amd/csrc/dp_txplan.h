// SPDX-License-Identifier: Apache-2.0
//
// Launch geometry and scratch layout of the TX plan (include/dpgpu.h "TX
// plan"), shared by the kernels (dp_txplan.hip) and the runtime.
#ifndef DP_TXPLAN_H
#define DP_TXPLAN_H

#include <stdint.h>

#include "../../include/dpgpu.h"

namespace dpt {

constexpr uint32_t kTpb = 256;                // count / scatter workgroup
constexpr uint32_t kRounds = 8;               // packets a lane takes
constexpr uint32_t kTile = kTpb * kRounds;    // packets a workgroup takes (2048)
constexpr uint32_t kBuckets = 64;             // DP_TX_MAX_PORTS + 2: a bucket is a wave lane
constexpr uint32_t kNoBucket = 0xffu;         // (in registers only: a lane past the burst's end)
static_assert(DP_TX_MAX_PORTS + 2 == kBuckets, "one wave lane a bucket");
static_assert((uint64_t)kTile * 65535 < (1ull << 32), "a tile's byte sums fit u32");

// The caller's port list as the kernels take it (a kernel argument).
struct Ports {
  uint32_t n;
  uint32_t oif[DP_TX_MAX_PORTS];
};

// Scratch of one plan over n packets: a bucket byte per packet, then per tile
// 64 counts, 64 byte sums and 64 bases (positions in `order`).
inline uint64_t tiles_of(uint32_t n) { return ((uint64_t)n + kTile - 1) / kTile; }
inline uint64_t bucket_bytes(uint32_t n) { return ((uint64_t)n + 255) & ~255ull; }
inline uint64_t scratch_bytes(uint32_t n) { return bucket_bytes(n) + tiles_of(n) * (3 * kBuckets * 4); }

}  // namespace dpt

#endif
