// SPDX-License-Identifier: Apache-2.0
//
// What the flow-table units share (dp_flows.hip: the table's calls;
// dp_flowsnap.hip: its snapshot): the launch width, a FlowKey's slot words, a
// stored flow's dp_flow_info_t and the management calls' stream discipline.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/dpgpu.h"
#include "dp_flows_rt.h"

namespace dpfl {

constexpr uint32_t kTB = 256;

__device__ inline void fill_info(const dpf::FlowSlot *slots, uint32_t mask, uint32_t sl, dp_flow_info_t &o) {
  const dpf::FlowSlot &s = slots[sl];
  o.ref = dpf::make_ref(sl, s.state);
  o.status = s.status;
  o.flags = s.flags;
  o.dst_vni = s.dst_vni;
  o.pad = 0;
  o.genid = s.genid;
  o.expires_at = s.expires_at;
  o.related = DP_FLOW_NONE;
  if (s.related <= mask && slots[s.related].state == s.related_tag)
    o.related = dpf::make_ref(s.related, s.related_tag);
  o.flags = s.flags & 7u;
  if (s.flags & dpf::kFlagMasq) {  // MasqueradeState (nat/src/masquerade/state.rs:13-20)
    o.masq = (uint8_t)(s.pf & 0xffu);
    o.pf_status = (uint8_t)((s.pf >> 8) & 0xffu);
    o.pf_port = (uint16_t)(s.pf >> 16);
    o.pf_family = (uint8_t)s.pf_fam;
    for (int j = 0; j < 4; j++)
      for (int b = 0; b < 4; b++) o.pf_ip[4 * j + b] = (uint8_t)(s.pf_ip[j] >> (24 - 8 * b));
    if (s.pf_fam == 4) for (int b = 4; b < 16; b++) o.pf_ip[b] = 0;
    o.masq_alloc = s.mq_rec != 0;
    o.idle_timeout_s = s.pf_rule;
  }
  if (s.flags & dpf::kFlagPf) {  // PortFwState (nat/src/portfw/flow_state.rs:29-35)
    o.pf = (uint8_t)(s.pf & 0xffu);
    o.pf_status = (uint8_t)((s.pf >> 8) & 0xffu);
    o.pf_port = (uint16_t)(s.pf >> 16);
    o.pf_rule = s.pf_rule;
    o.pf_family = (uint8_t)s.pf_fam;
    for (int j = 0; j < 4; j++)
      for (int b = 0; b < 4; b++) o.pf_ip[4 * j + b] = (uint8_t)(s.pf_ip[j] >> (24 - 8 * b));
  }
}

inline dpf::FKey key_words(const dp_flow_key_t &x) {
  dpf::FKey k{};
  k.w[0] = x.src_vni;
  k.w[1] = (uint32_t)x.family | ((uint32_t)x.kind << 8);
  k.w[2] = ((uint32_t)x.sport << 16) | x.dport;
  uint8_t s[16] = {0}, d[16] = {0};
  const size_t n = x.family == 4 ? 4 : 16;
  memcpy(s, x.src, n);
  memcpy(d, x.dst, n);
  memcpy(&k.w[3], s, 16);
  memcpy(&k.w[7], d, 16);
  return k;
}

// Run `f(stream)` with the table's device current and its stream; sync.
template <class F>
int run(dp_flow_table *ft, const char *what, F f) {
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ft->device);
  // after every flows burst launched before this call (dp_flows_rt.h)
  if (ft->burst_armed) (void)hipStreamWaitEvent(ft->stream, ft->last_burst, 0);
  int rc = f(ft->stream);
  hipError_t e = hipStreamSynchronize(ft->stream);
  if (!rc && e != hipSuccess) rc = dpr_fail(DP_EIO, what, e);
  if (!rc && (e = hipGetLastError()) != hipSuccess) rc = dpr_fail(DP_EIO, what, e);
  (void)hipSetDevice(prev);
  return rc;
}

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kTB - 1) / kTB); }

}  // namespace dpfl
