// SPDX-License-Identifier: Apache-2.0
//
// Raw route records and launch geometry of the device route sort
// (DP_OPT_DEVICE_FIB = 2, include/dpgpu.h), shared by the table compiler
// (dp_tables.cpp: it packs the records), the kernels (dp_fibsort.hip), the
// runtime and the host restatement (scripts/fib_build_check.cpp).  The kernels
// turn a FIB's v4 routes in insertion order into the Short / Long / Block lists
// of dp_fibbuild.h.  Host-only users include this without HIP.
#ifndef DP_FIBSORT_H
#define DP_FIBSORT_H

#include <stdint.h>

#include "dp_fibbuild.h"

namespace dps {

constexpr uint32_t kTpb = 256;                // workgroup of the tile kernels
constexpr uint32_t kKpt = 8;                  // records a lane owns
constexpr uint32_t kTile = kTpb * kKpt;       // records a workgroup owns (2048)
constexpr uint32_t kWaveKeys = 64 * kKpt;     // a wave's contiguous share of the tile (512)
constexpr uint32_t kScanTpb = 1024;           // the one workgroup of the scan kernel
constexpr uint32_t kScanPer = 4;              // words a lane of it takes per step
constexpr uint32_t kDigits = 256;             // buckets of a radix pass (64 in the length pass)
constexpr uint32_t kPasses = 5;               // 6-bit length digit, then 4 address bytes, low to high
constexpr uint32_t kMaxRoutes = 1u << 26;     // a FIB with more routes takes the host sort
constexpr uint32_t kShift[kPasses] = {0, 6, 14, 22, 30};
constexpr uint32_t kMask[kPasses] = {63, 255, 255, 255, 255};

// One route, 8 bytes: length in bits 0..5, address in 6..37 -- together the
// 38-bit sort key (address, length) -- and the next hop (< 0xffff) in 38..53.
typedef uint64_t Raw;
constexpr uint64_t kKeyMask = (1ull << 38) - 1;
DPB_HD inline Raw pack(uint32_t addr, uint32_t len, uint32_t nh) { return (uint64_t)nh << 38 | (uint64_t)addr << 6 | len; }
DPB_HD inline uint64_t key_of(Raw r) { return r & kKeyMask; }
DPB_HD inline uint32_t addr_of(Raw r) { return (uint32_t)(r >> 6); }
DPB_HD inline uint32_t len_of(Raw r) { return (uint32_t)r & 63u; }
DPB_HD inline uint32_t nh_of(Raw r) { return (uint32_t)(r >> 38) & 0xffffu; }

// What element i of the sorted records contributes (prev / next: its
// neighbours, ignored at the ends).  It survives if it is the last of its run
// of equal keys; a survivor is short (length <= 24) or long; the first record
// of a /24's long records -- survivor or not, they are contiguous: the /24's
// short routes sort before them -- heads a block.
constexpr uint32_t kIsShort = 1, kIsLong = 2, kIsHead = 4;
DPB_HD inline uint32_t classify(Raw prev, Raw cur, Raw next, uint32_t i, uint32_t n) {
  const bool surv = i + 1 == n || key_of(next) != key_of(cur);
  const bool lng = len_of(cur) > 24;
  const bool head = lng && (i == 0 || len_of(prev) <= 24 || (addr_of(prev) >> 8) != (addr_of(cur) >> 8));
  return (surv && !lng ? kIsShort : 0) | (surv && lng ? kIsLong : 0) | (head ? kIsHead : 0);
}

// What the kernels found (read back by the runtime in one copy).
struct Counts {
  uint32_t n_short, n_long, n_blocks, pad;
};

constexpr uint32_t tiles_of(uint32_t n) { return (n + kTile - 1) / kTile; }
// words of the histogram / tile-count scratch: a pass scans kDigits * tiles
// words, the list positions 3 * tiles; one more for the grand total
constexpr uint64_t scratch_words(uint32_t n) { return (uint64_t)kDigits * tiles_of(n) + 1; }

// Device addresses of one FIB's sort (a kernel-launch argument).  `a` holds
// the n records in insertion order; the sorted records end in `b`.  The list
// capacities are host-side bounds (raw routes of each kind, the /24s that hold
// a long route), never exceeded: survivors are a subset.
struct SortJob {
  Raw *a, *b;
  uint32_t *scratch;  // scratch_words(n)
  dpb::Short *shorts;
  dpb::Long *longs;
  dpb::Block *blocks;
  Counts *counts;
  uint32_t n, cap_short, cap_long, cap_blocks;
};

}  // namespace dps

#endif
