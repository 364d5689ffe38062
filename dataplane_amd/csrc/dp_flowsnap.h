// SPDX-License-Identifier: Apache-2.0
//
// The flow-table snapshot's filter (include/dpgpu.h "Flow-table snapshot") in
// the form the scan evaluates, and its predicate -- one text for the device
// scan (dp_flowsnap.hip) and for dp_flow_filter_match on the host, over the
// 32 words of a flow slot (dp_flow.h FlowSlot).
//
// The slot's first 64 bytes decide every clause but GENID_*, EXPIRES_LE and
// NAT*; they are tested per 16-byte chunk (chunk_ok), so that four lanes can
// each test the chunk they loaded: chunk 0 state / src_vni / family+kind /
// ports, chunk 1 src, chunk 2 dst, chunk 3 status / flags / dst_vni.  The
// rest (second_ok) reads words 16-31 and the flags word.
#pragma once
#include <stdint.h>

#include "../../include/dpgpu.h"
#include "dp_flow.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace dpfs {

constexpr uint32_t kAllClauses = (DP_FLOWF_NAT_PORT << 1) - 1;
constexpr uint32_t kSecondClauses = DP_FLOWF_GENID_LT | DP_FLOWF_GENID_EQ | DP_FLOWF_EXPIRES_LE | DP_FLOWF_NAT |
                                    DP_FLOWF_NAT_IP | DP_FLOWF_NAT_PORT;

// A prefix as (mask, value) words in the order of the words it is compared
// with: AND + compare per word.
struct Pfx {
  uint32_t fam;
  uint32_t m[4], v[4];
};

struct Filter {
  uint32_t clauses;
  uint32_t src_vni, dst_vni;
  uint32_t family, kind_mask, status_mask, nat_mask;
  uint32_t flags_all, flags_none;
  uint32_t sport_lo, sport_hi, dport_lo, dport_hi, nport_lo, nport_hi;
  Pfx src, dst;  // key address words: the bytes as stored (memcpy order)
  Pfx nat;       // use_ip words: big-endian numbers, v4 in word 0
  int64_t genid;
  uint64_t expires_at;
};

__host__ __device__ inline bool pfx_ok(const Pfx &p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return (((a & p.m[0]) ^ p.v[0]) | ((b & p.m[1]) ^ p.v[1]) | ((c & p.m[2]) ^ p.v[2]) | ((d & p.m[3]) ^ p.v[3])) == 0;
}

// Words 4c .. 4c + 3 of a slot against the clauses that live there.
__host__ __device__ inline bool chunk_ok(const Filter &F, uint32_t c, uint32_t x, uint32_t y, uint32_t z,
                                         uint32_t w) {
  const uint32_t cl = F.clauses;
  if (c == 0) {  // state, src_vni, family | kind << 8, sport << 16 | dport
    const uint32_t fam = z & 0xffu, kind = (z >> 8) & 0xffu, sport = w >> 16, dport = w & 0xffffu;
    bool ok = (x & 3u) == dpf::FS_FULL;
    if (cl & DP_FLOWF_SRC_VNI) ok &= y == F.src_vni;
    if (cl & DP_FLOWF_FAMILY) ok &= fam == F.family;
    if (cl & DP_FLOWF_KIND) ok &= kind < 8 && ((F.kind_mask >> kind) & 1u);
    if (cl & DP_FLOWF_SRC) ok &= fam == F.src.fam;
    if (cl & DP_FLOWF_DST) ok &= fam == F.dst.fam;
    if (cl & DP_FLOWF_SPORT) ok &= sport >= F.sport_lo && sport <= F.sport_hi;
    if (cl & DP_FLOWF_DPORT) ok &= dport >= F.dport_lo && dport <= F.dport_hi;
    return ok;
  }
  if (c == 1) return !(cl & DP_FLOWF_SRC) || pfx_ok(F.src, x, y, z, w);
  if (c == 2) return !(cl & DP_FLOWF_DST) || pfx_ok(F.dst, x, y, z, w);
  // status, flags, dst_vni, related
  bool ok = true;
  if (cl & DP_FLOWF_STATUS) ok &= x < 8 && ((F.status_mask >> x) & 1u);
  if (cl & DP_FLOWF_FLAGS_ALL) ok &= ((y & 7u) & F.flags_all) == F.flags_all;
  if (cl & DP_FLOWF_FLAGS_NONE) ok &= ((y & 7u) & F.flags_none) == 0;
  if (cl & DP_FLOWF_DST_VNI) ok &= z == F.dst_vni;
  return ok;
}

// Words 16 .. 31 of a slot (h[0] = related_tag ... h[15] = nat_tag) and its
// flags word against GENID_*, EXPIRES_LE and NAT*.
__host__ __device__ inline bool second_ok(const Filter &F, uint32_t flags, const uint32_t *h) {
  const uint32_t cl = F.clauses;
  bool ok = true;
  const int64_t genid = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
  const uint64_t expires = ((uint64_t)h[5] << 32) | h[4];
  if (cl & DP_FLOWF_GENID_LT) ok &= genid < F.genid;
  if (cl & DP_FLOWF_GENID_EQ) ok &= genid == F.genid;
  if (cl & DP_FLOWF_EXPIRES_LE) ok &= expires <= F.expires_at;
  if (cl & (DP_FLOWF_NAT | DP_FLOWF_NAT_IP | DP_FLOWF_NAT_PORT)) {
    // a state exists where its flag is set and its action is not DP_PF_NONE
    const uint32_t pf = h[6];
    const bool act = (pf & 0xffu) != 0;
    const bool has_pf = act && (flags & dpf::kFlagPf), has_mq = act && (flags & dpf::kFlagMasq);
    const uint32_t cls = (has_pf ? (uint32_t)DP_FLOW_NAT_PF : 0u) | (has_mq ? (uint32_t)DP_FLOW_NAT_MASQ : 0u) |
                         (has_mq && h[13] ? (uint32_t)DP_FLOW_NAT_MASQ_ALLOC : 0u);
    if (cl & DP_FLOWF_NAT) ok &= (cls & F.nat_mask) != 0;
    if (cl & DP_FLOWF_NAT_IP) ok &= cls && h[12] == F.nat.fam && pfx_ok(F.nat, h[8], h[9], h[10], h[11]);
    if (cl & DP_FLOWF_NAT_PORT) ok &= cls && (pf >> 16) >= F.nport_lo && (pf >> 16) <= F.nport_hi;
  }
  return ok;
}

// The whole predicate over a slot's 32 words.
__host__ __device__ inline bool slot_ok(const Filter &F, const uint32_t *w) {
  bool ok = true;
  for (uint32_t c = 0; c < 4; c++) ok &= chunk_ok(F, c, w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
  if (ok && (F.clauses & kSecondClauses)) ok = second_ok(F, w[13], w + 16);
  return ok;
}

}  // namespace dpfs
