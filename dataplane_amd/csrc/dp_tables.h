// SPDX-License-Identifier: Apache-2.0
// Host table compiler interface (dp_tables.cpp).
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/dpgpu.h"
#include "dp_device.h"
#include "dp_fibbuild.h"
#include "dp_fibsort.h"

namespace dpd {

// A masquerade expose as the tables hold it (dp_masq_expose_t, validated):
// one family, private and public prefixes, the port-forwarding claims on its
// public range.
struct MasqExpose {
  uint32_t src_vni, dst_vni;
  uint64_t idle_ns;
  int fam;
  std::vector<dp_prefix_t> priv, pub;
  std::vector<dp_masq_claim_t> claims;
};
// MasqueradeConfig: the exposes, their canonical bytes and the caller's tag
// (a flow table's allocator is kept across publishes of the same config,
// nat/src/masquerade/allocator_writer.rs:120-154).  The allocator itself is
// flow-table state (dp_masq.h), built from this when a table syncs.
struct MasqConfig {
  std::vector<MasqExpose> exposes;
  std::string canon;
  uint64_t tag = 0;
  bool randomize = false;  // MasqueradeConfig::set_randomize, and the permutations' seed
  uint64_t seed = 0;
  bool same(const MasqConfig &o) const {
    if (randomize != o.randomize || seed != o.seed) return false;
    return tag || o.tag ? tag == o.tag && o.tag != 0 : canon == o.canon;
  }
};

// A region of the image the host reserved and did not fill: the device builds
// it (DP_OPT_DEVICE_FIB).  Holes ascend and never touch.
struct ImageHole {
  uint64_t off, bytes;
};
// The lists one device-built DIR-24-8 FIB is made from (dp_fibbuild.h) and the
// image offsets of its two holes (block16 is host-built zeros when there is
// no block).  With the device route sort (DP_OPT_DEVICE_FIB = 2) the lists
// stay empty: `raw` holds the FIB's v4 routes in insertion order, the implicit
// /0 first (dp_fibsort.h), with how many of them are of length <= 24 and
// longer, and `n_blocks` the /24s that hold a longer one.
struct FibBuild {
  std::vector<dpb::Short> shorts;
  std::vector<dpb::Long> longs;
  std::vector<dpb::Block> blocks;
  uint64_t direct = 0, block16 = 0;
  std::vector<dps::Raw> raw;
  uint32_t raw_short = 0, raw_long = 0, n_blocks = 0;
};

struct BuiltImage {
  // host copy of the device image -- without the holes: the bytes of image
  // offset o are at o minus the holes below o (no hole unless build_image was
  // asked for device FIBs: then `bytes` is the image)
  std::vector<uint8_t> bytes;
  std::vector<ImageHole> holes;
  std::vector<FibBuild> fib_builds;
  Image im;                    // image offsets; im.bytes counts the holes
  uint64_t pt_nodes = 0;
  std::shared_ptr<const MasqConfig> masq;  // never null after a successful build
  // build_lpm: sort + dedupe + list prep (device route sort: the pass that packs the records); host table build
  uint64_t sort_us = 0, paint_us = 0;
};

// The port-forwarding entries of a device's current generation (the lineage
// PortFwTable::update carries from one publish to the next).
struct PfEntry {
  dp_portfw_rule_t r;
  uint32_t id;
};
struct PfLineage {
  std::vector<PfEntry> live;
  uint32_t next_id = 1;
};

// Validate + lower the descriptors; returns 0 or a negative errno.  `pf`:
// the device's port-forwarding lineage, updated with the new rule set (only
// when the build succeeds).  `device_fib` (the DP_OPT_DEVICE_FIB mode), 1: v4
// FIBs that take the DIR-24-8 form get holes and build lists instead of
// host-built tables; 2: holes and their unsorted route records.
int build_image(const dp_tables_desc_t *desc, BuiltImage &out, PfLineage *pf = nullptr, int device_fib = 0);

}  // namespace dpd
