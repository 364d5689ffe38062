// SPDX-License-Identifier: Apache-2.0
//
// Device-side state of a context's packet capture (include/dpgpu.h "Packet
// capture"), shared by the kernels (dp_capture.hip) and the runtime.
#ifndef DP_CAPTURE_H
#define DP_CAPTURE_H

#include <stdint.h>

#include "../../include/dpgpu.h"

namespace dpc {

constexpr uint32_t kTpb = 256;    // select / copy workgroup
constexpr uint32_t kTile = 1024;  // packets a workgroup takes: four rounds of kTpb

// The capture buffer's counters, in device memory: a launch appends from them
// without a host round trip (dp_capture_scan_k), dp_capture_read copies them.
struct State {
  unsigned long long n_units;  // 16-byte units of frame bytes stored
  unsigned long long matched;  // packets the filter selected since open / reset
  unsigned long long lost;     // ... of which did not fit
  uint32_t n_recs;             // records stored
  uint32_t burst;              // capture launches since open / reset
  uint32_t cur_burst;          // the running launch's number (scan -> copy)
  uint32_t pad;
};

// What the scan leaves a tile's copy workgroup.
struct TileBase {
  unsigned long long unit_base;  // the tile's first unit in the capture bytes
  uint32_t rec_base;             // the tile's first record
  uint32_t keep;                 // records of the tile that are kept (a prefix of its matches)
};

// A select word (one per packet of the launch): the match bit and caplen.
constexpr uint32_t kSelMatch = 0x80000000u;

// dp_capture_filter_t as the select kernel takes it (a kernel argument, so it
// lives in scalar registers): prefixes as words in memory order with their
// byte masks, so frame words compare without a byte swap.
struct Filter {
  uint32_t clauses, l4_mask;
  unsigned long long done_mask;
  uint32_t src_vni, dst_vni;
  uint32_t src_fam, dst_fam;  // 4 / 6
  uint32_t src[4], src_mask[4], dst[4], dst_mask[4];
  uint32_t sport_lo, sport_hi, dport_lo, dport_hi;
  uint32_t snaplen;
};

// Scratch of one launch over n packets: the select words, then per tile the
// (matches, units) totals and the TileBase records.
inline uint64_t tiles_of(uint32_t n) { return ((uint64_t)n + kTile - 1) / kTile; }
inline uint64_t scratch_bytes(uint32_t n) {
  return (((uint64_t)n * 4 + 15) & ~15ull) + tiles_of(n) * (8 + sizeof(TileBase));
}

}  // namespace dpc

#endif
