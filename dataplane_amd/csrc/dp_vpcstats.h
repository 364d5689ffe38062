// SPDX-License-Identifier: Apache-2.0
//
// The per-VPC statistics table of a context (include/dpgpu.h "Per-VPC
// statistics"), shared by the kernel (dp_vpcstats.hip) and the runtime.
#ifndef DP_VPCSTATS_H
#define DP_VPCSTATS_H

#include <stdint.h>

#include "../../include/dpgpu.h"

namespace dpv {

// counter columns of a cell
enum { kFwdPackets = 0, kFwdBytes = 1, kDropPackets = 2, kDropBytes = 3 };

// One open-addressing table in device memory, zero when empty.  A cell's key
// is src_vni << 32 | dst_vni (never 0: a recorded cell has a source).  A slot
// is claimed by a 64-bit compare-and-swap on its key and never released
// before a reset; the claimer takes the next ticket of `count`.  Slots whose
// ticket is past DP_VPC_STATS_CELLS / 2 are over capacity: the read adds
// their packets to the lost count instead of reporting them, so whether a
// cell is reported is decided once, by the one lane that claimed its slot --
// a reported cell holds every update it ever got.  A cell that finds all
// DP_VPC_STATS_CELLS slots taken adds its packets to `lost`.
struct Table {
  unsigned long long key[DP_VPC_STATS_CELLS];
  unsigned long long ctr[DP_VPC_STATS_CELLS][4];
  uint32_t tick[DP_VPC_STATS_CELLS];  // claim ticket + 1
  uint32_t count;                     // tickets handed out
  uint32_t pad;
  unsigned long long lost;
};

// Persistent workgroups of one launch per compute unit: one of 16 waves --
// enough loads in flight to stream the records, and one flush per live cell
// and compute unit at the end.
constexpr uint32_t kBlocksPerCu = 1;

}  // namespace dpv

#endif
